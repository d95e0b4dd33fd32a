/*
 * lbm_hip.h -- C-ABI boundary of the MI355X (gfx950) D2Q9-BGK lattice-Boltzmann engine.
 *
 * This is the drop-in boundary for the reference's timestep hot path.  The reference
 * (Xinran1205/LBM-Asynchronous) has no plugin / FFI layer: its boundary is five C functions
 * called from main()'s loop (SerialCode/d2q9-bgk.c:97-101,113,166-170) over caller-owned host
 * arrays.  Each entry point below names the reference interface it replaces.
 *
 * Plain C types only; no C++ or torch types cross this boundary.  One host thread per context.
 *
 * Error behaviour follows the reference: by default an error prints
 *     "Error at line <n> of file <f>:\n<message>\n"
 * to stderr and calls exit(EXIT_FAILURE), exactly like die() (SerialCode/d2q9-bgk.c:745-751).
 * A host that must survive errors (the Python test harness) switches to return codes with
 * lbm_set_error_mode(LBM_ERRORS_RETURN); functions then return LBM_FAILURE / NULL and
 * lbm_last_error() holds the message.  There is NO CPU fallback: without a usable HIP device
 * every compute entry point fails.
 *
 * Data layout on the device: structure-of-arrays interleaved by row, fp32 --
 * value (speed k, row y, column x) at base + (y*9 + k)*pitch + x -- with four halo rows below
 * and above the rows a slab owns (a K-step pass reads K rows beyond the slab, K <= 4); uint8 obstacle mask.
 * Host-facing arrays keep the reference's layouts: cells are array-of-structures
 * (9 consecutive floats per cell, cell index ii + jj*nx, SerialCode/d2q9-bgk.c:78-81),
 * obstacles are int[ny*nx] with 1 = blocked (:541, :570-601).
 */
#ifndef LBM_HIP_H
#define LBM_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_SUCCESS 0
#define LBM_FAILURE 1

#define LBM_ERRORS_DIE    0 /* reference behaviour: message to stderr + exit(EXIT_FAILURE) */
#define LBM_ERRORS_RETURN 1 /* return LBM_FAILURE / NULL, message kept for lbm_last_error() */

/* numerics mode of the collision kernel */
#define LBM_MATH_EXACT 0 /* reference operation order, IEEE / and sqrt, no FMA contraction:
                            the lattice is bit-identical to SerialCode's */
#define LBM_MATH_FAST  1 /* reciprocal multiplies + FMA; validated through the check.py rule */

/* How a pass across several slabs / ranks treats its halo rows */
#define LBM_HALO_SYNC  0 /* halo rows of the same timestep: the MPI_Waitall pattern
                            (MPI_Waitall/d2q9-bgk.c:225-253); results equal the single-domain run */
#define LBM_HALO_STALE 1 /* EXPERIMENTAL.  Halo rows one pass old: reproducible analogue of the reference's
                            MPI_Testall "stale halo" variant (MPI_Testall_OptimizedVersion/
                            d2q9-bgk.c:256-301); no pass ever waits for an exchange of its own.
                            Parity unpinned (the reference variant is non-deterministic, so no fixture
                            can exist); measured against the synchronous run by the check.py rule it
                            misses 1 % in dense decompositions: av_vels 4.7 % (128x256 / 2 slabs, step 2),
                            4.0 % (128x128 / 8 slabs, mid-transient), 1.2 % (256x256 / 4 slabs);
                            pressure stays within 0.01 % */
#define LBM_HALO_FRESHEST 2 /* EXPERIMENTAL.  The reference's rule itself -- post the exchange, relax the interior rows,
                            look ONCE whether the halo rows have arrived, relax the boundary rows either way
                            (MPI_Testall_OptimizedVersion/d2q9-bgk.c:262-290) -- with two guarantees the reference
                            does not give: a halo row is this step's or the step before's, never older (the stale
                            mode's exchange backs it), and never torn (whole rows are adopted, by a look at an id
                            that travels behind them).  Which of the two each side got in each step is logged
                            (lbm_read_halo_log); given the log the run is reproducible on the CPU
                            (tests/slab_model.py).  Results lie between the synchronous and the stale run and
                            differ from run to run.  Parity unpinned, as for LBM_HALO_STALE.  RCCL and
                            device-copy transports only */

/* Run constants: field-for-field the reference's t_param (SerialCode/d2q9-bgk.c:66-75). */
typedef struct {
  int   nx;           /* cells in x */
  int   ny;           /* cells in y */
  int   max_iters;    /* iterations (capacity of the av_vels record) */
  int   reynolds_dim; /* dimension for the Reynolds number */
  float density;      /* density per link */
  float accel;        /* density redistribution */
  float omega;        /* relaxation parameter */
} lbm_params;

typedef struct lbm_ctx lbm_ctx; /* opaque engine handle */

/* Static facts a host may query (no device needed). */
typedef struct {
  int    n_slabs;        /* row slabs this context owns (1 per GPU in single-process mode) */
  int    row_first;      /* first global row owned by this context */
  int    row_count;      /* number of global rows owned by this context */
  int    fluid_cells;    /* GLOBAL number of non-blocked cells (av_velocity's divisor) */
  int    steps_done;     /* timesteps advanced so far */
  int    math_mode;      /* LBM_MATH_EXACT or LBM_MATH_FAST */
  int    world_rank;     /* rank of this context in a multi-process run (0 otherwise) */
  int    world_size;     /* number of processes sharing the grid (1 otherwise) */
  int    steps_per_launch; /* timesteps one launch of the main kernel advances: 2-4 for the stream kernels
                              (three from 300 Ki cells, four from 3.5 Mi cells per slab), 3-4 for the LDS-tile
                              kernel (small single slabs), else 1 */
  int    halo_mode;      /* LBM_HALO_SYNC, LBM_HALO_STALE or LBM_HALO_FRESHEST (meaningful with several slabs / ranks) */
  int    band_rows;      /* launch geometry of the multi-step stream kernel: rows one wave sweeps ... */
  int    lane_cells;     /* ... and cells per lane (4 or 2); 0 / 0 when another kernel is the main one */
  int    nontemporal;    /* 1: the step kernels store with the nontemporal hint */
  int    graph_steps;    /* timesteps one hipGraph chunk replays (0: loop issued launch by launch) */
  int    resident_steps; /* > 0: lbm_run calls of at least resident_min_steps timesteps run as launches of the resident
                            kernel (lattice in registers, up to this many timesteps per launch); single periodic slabs of
                            at most 1024 x 4*CUs cells */
  int    resident_min_steps;
  int    resident_rows;      /* resident kernel: rows per band (4 or 2) ... */
  int    resident_group;     /* ... bands per workgroup (1, 2 or 4) ... */
  int    resident_one_xcd;   /* ... and 1 where the whole grid (at most 128 waves) runs on one XCD, one wave per SIMD */
  int    band_groups;    /* single periodic slab: full-depth stream-kernel passes issued as this many row groups on their
                            own streams, so that successive passes overlap (1: one launch per pass) */
} lbm_info;

/* ---- error handling -------------------------------------------------------------------- */
void        lbm_set_error_mode(int mode);
const char* lbm_last_error(void);

/* ---- library / device probes ------------------------------------------------------------ */
const char* lbm_version(void);     /* "lbm_hip <ver> gfx950" */
int         lbm_device_count(void); /* visible HIP devices; 0 when none (never dies) */

/*
 * Row decomposition used for slabs and ranks (host arithmetic only, no device):
 * part `index` of `parts` gets rows [*first, *first + *count) of ny.  Balanced blocks,
 * the first ny % parts parts get one row more.  (The reference's rule,
 * MPI_Waitall/d2q9-bgk.c:694-704, additionally forces 3 rows onto the last rank because its
 * acceleration pass runs after the halo rows were posted; here acceleration is fused into the
 * kernel that produces the row, so no such constraint exists.)  Returns LBM_FAILURE when a
 * part would own fewer than 2 rows.
 */
int lbm_partition_rows(int ny, int parts, int index, int* first, int* count);

/*
 * The halo exchange of one pass, as the engine posts it (host arithmetic only, no device): the reference's
 * MPI_Isend x2 + MPI_Irecv x2 (MPI_Waitall/d2q9-bgk.c:225-230) with whole boundary rows, `depth` rows per side.
 * out[0..3], in posting order: send my top rows to the north neighbour, send my bottom rows to the south
 * neighbour, receive my south halo from the south neighbour, receive my north halo from the north neighbour
 * (north = (index+1) % parts, south = (index-1+parts) % parts: the periodic ring of MPI/d2q9-bgk.c:210-211; with
 * two parts both neighbours are the same peer and the first send pairs with that peer's first receive).
 * row_first counts slab-local rows: 0 is the first owned row, negative rows are the south halo, rows >= `rows` the
 * north halo.  lbm_plan_halo_depth: the depth (= timesteps per pass) the engine uses for a grid cut into `parts`
 * row slabs with halos in the given math mode (environment overrides included); its own exchange is built from lbm_halo_plan, so a host
 * that replays the protocol (tests/test_multirank_gloo.py) cannot drift from it.
 */
typedef struct {
  int is_send;   /* 1: ncclSend / MPI_Isend, 0: ncclRecv / MPI_Irecv */
  int peer;      /* neighbour's index in the ring */
  int row_first; /* first slab-local row of the message */
  int row_count; /* rows in the message (each row: 9 planes x pitch floats on the device) */
} lbm_halo_op;
int lbm_halo_plan(int rows, int parts, int index, int depth, lbm_halo_op out[4]);
int lbm_plan_halo_depth(const lbm_params* params, int parts, int math_mode);

/* ---- create / destroy --------------------------------------------------------------------
 * Replaces the buffer set-up half of initialise() (SerialCode/d2q9-bgk.c:531-567) and
 * finalise() (:615-634).
 *
 * obstacles : int[ny*nx], 1 = blocked (the array initialise() builds, :570-601).
 * cells_aos : float[ny*nx*9] initial lattice in the reference's AoS layout, or NULL to start
 *             from the uniform equilibrium of :546-567 generated on the device.
 * n_gpus    : row slabs / devices to spread the grid over in THIS process (1..8).  Slab g runs
 *             on device g % lbm_device_count(); several slabs may share one device (used to
 *             test the halo path on a 1-GPU box).
 * math_mode : LBM_MATH_EXACT or LBM_MATH_FAST.
 */
lbm_ctx* lbm_create(const lbm_params* params, const int* obstacles, const float* cells_aos,
                    int n_gpus, int math_mode);

/*
 * One-process-per-GPU form (torchrun / RANK, WORLD_SIZE): this process owns the rows
 * lbm_partition_rows(ny, world_size, rank) of the global grid on HIP device `device`;
 * halo rows travel by RCCL send/recv (the GPU analogue of MPI_Isend/Irecv + Waitall,
 * MPI_Waitall/d2q9-bgk.c:225-243).  `unique_id` is the 128-byte RCCL id obtained by rank 0
 * from lbm_rccl_unique_id() and broadcast by the host (e.g. over torch.distributed).
 * obstacles is the GLOBAL mask (every rank parses the same file), cells_aos the GLOBAL
 * initial lattice or NULL.
 */
#define LBM_RCCL_ID_BYTES 128
int      lbm_rccl_unique_id(void* id_out);

/*
 * Which RCCL serves the halo exchange, and what it says about the ring -- the question "did RCCL see N ranks, and
 * which RCCL" of a multi-GPU run, answered from the run's own record (the reference prints "Process %d of %d started",
 * MPI/d2q9-bgk.c:151, from MPI_Comm_rank / MPI_Comm_size, MPI_Waitall/d2q9-bgk.c:143-147).
 * RCCL is bound at first use, not at link time, in this order: the file named by LBM_RCCL_LIB; a librccl.so.1 the
 * process has already mapped (a host that imported PyTorch carries PyTorch's bundled RCCL next to its bundled HIP
 * runtime -- a communicator has to come from the RCCL built for the HIP runtime in the process); ROCm's own
 * /opt/rocm/lib/librccl.so.1.  A single-GPU run never loads it.
 * ctx == NULL: binds the library and reports `loaded`, `version`, `library`.  With a context: its communicators
 * (n_comms: one per slab in the one-process form, one in the one-process-per-GPU form, none for a single slab or the
 * device-copy / hosted transports) and nranks / rank as ncclCommCount / ncclCommUserRank of the first one report them.
 */
typedef struct {
  int  loaded;        /* 1: a librccl is bound to this engine */
  int  version;       /* ncclGetVersion(), e.g. 22707 = 2.27.7 */
  int  n_comms;       /* communicators the context holds */
  int  nranks;        /* ranks in the ring as RCCL counts them (ncclCommCount); 0 without a communicator */
  int  rank;          /* this context's rank in it (ncclCommUserRank) */
  char library[512];  /* file the RCCL entry points were bound from */
} lbm_rccl_status;
int      lbm_rccl_info(const lbm_ctx* ctx, lbm_rccl_status* out);
lbm_ctx* lbm_create_rank(const lbm_params* params, const int* obstacles, const float* cells_aos,
                         int rank, int world_size, const void* unique_id, int device,
                         int math_mode);

/*
 * The same, without the global map on every rank -- the reference's scatter (rank 0 parses, every rank
 * receives only its rows, MPI_Waitall/d2q9-bgk.c:794-842):
 *   obstacle_rows  : int[(row_count + 2*LBM_MASK_HALO_ROWS) * nx] -- the rows lbm_partition_rows gives this
 *                    rank, preceded and followed by LBM_MASK_HALO_ROWS periodic neighbour rows (global rows
 *                    row_first - LBM_MASK_HALO_ROWS ... row_first + row_count + LBM_MASK_HALO_ROWS - 1, folded
 *                    into [0, ny)): a multi-step pass relaxes that many rows beyond the slab redundantly;
 *   cells_rows_aos : float[row_count * nx * 9], this rank's rows only, or NULL (uniform equilibrium).
 * The mask is built on the device; the fluid-cell count (av_velocity's divisor) is a device reduction over the
 * owned rows summed over the ranks by one all-reduce.  lbm_create and lbm_create_rank count the same way.
 */
#define LBM_MASK_HALO_ROWS 3
lbm_ctx* lbm_create_rank_rows(const lbm_params* params, const int* obstacle_rows, const float* cells_rows_aos,
                              int rank, int world_size, const void* unique_id, int device,
                              int math_mode);

/*
 * Obstacles given as a small tile repeated periodically over the grid: cell (x, y) is blocked iff the tile's cell
 * (x mod tile_nx, y mod tile_ny) is (tile: int[tile_ny*tile_nx]).  This is how BASELINE.md section 4 defines the
 * synthetic 8192x8192 and 16384x16384 grids (the reference's 1024x1024 map tiled); the mask is expanded on the
 * device from the tile, so a 16384x16384 run never holds a 1 GiB int map on the host.
 */
lbm_ctx* lbm_create_tiled(const lbm_params* params, const int* tile, int tile_nx, int tile_ny,
                          const float* cells_aos, int n_gpus, int math_mode);
lbm_ctx* lbm_create_rank_tiled(const lbm_params* params, const int* tile, int tile_nx, int tile_ny,
                               int rank, int world_size, const void* unique_id, int device,
                               int math_mode);

/*
 * One process per GPU with the HOST's own message passing instead of RCCL -- the closest fit to the reference's MPI
 * programs, which keep MPI_Isend / MPI_Irecv / MPI_Waitall (MPI_Waitall/d2q9-bgk.c:225-243) and MPI_Reduce
 * (:321): the engine hands the boundary rows of a pass to `exchange` in pinned host buffers and takes the halo rows
 * back, and sums its per-rank totals through `allreduce_sum`.
 *   exchange(user, 4, ops, buffers, floats): the four messages of lbm_halo_plan in posting order; for ops[i].is_send
 *     send buffers[i][0 .. floats) to rank ops[i].peer, else receive that many floats from it into buffers[i].  Post all
 *     four before waiting for any (two ranks are each other's north AND south neighbour).  Return 0 on success.
 *   allreduce_sum(user, values, n): in-place sum of n doubles over all ranks; every rank receives it.  Return 0.
 * The callbacks block the host, so this transport does not hide the exchange behind the interior rows; it exists for
 * MPI-launched hosts and to run the rank decomposition with several ranks on ONE device (tests).  obstacles /
 * cells_aos: the global arrays, as lbm_create_rank (the _rows / _tiled forms below take only a rank's share).
 * Every rank must issue the same sequence of calls.
 */
typedef struct {
  int (*exchange)(void* user, int n_ops, const lbm_halo_op* ops, float* const* buffers, size_t floats_per_message);
  int (*allreduce_sum)(void* user, double* values, int n);
  void* user;
} lbm_host_comm;
lbm_ctx* lbm_create_rank_hosted(const lbm_params* params, const int* obstacles, const float* cells_aos,
                                int rank, int world_size, const lbm_host_comm* comm, int device,
                                int math_mode);
/*
 * The same without the global arrays on every rank -- what the reference's MPI programs do: rank 0 parses the
 * obstacle file and sends every rank its rows (MPI_Waitall/d2q9-bgk.c:816-842).  Arguments as lbm_create_rank_rows
 * (this rank's rows with LBM_MASK_HALO_ROWS periodic neighbour rows on each side; this rank's cells or NULL) and
 * lbm_create_rank_tiled (a small tile repeated over the grid, expanded on the device).
 */
lbm_ctx* lbm_create_rank_hosted_rows(const lbm_params* params, const int* obstacle_rows, const float* cells_rows_aos,
                                     int rank, int world_size, const lbm_host_comm* comm, int device,
                                     int math_mode);
lbm_ctx* lbm_create_rank_hosted_tiled(const lbm_params* params, const int* tile, int tile_nx, int tile_ny,
                                      int rank, int world_size, const lbm_host_comm* comm, int device,
                                      int math_mode);

void     lbm_destroy(lbm_ctx* ctx);
int      lbm_get_info(const lbm_ctx* ctx, lbm_info* out);

/*
 * Halo treatment for the following lbm_run calls (default LBM_HALO_SYNC, or LBM_HALO_STALE / LBM_HALO_FRESHEST when
 * the environment holds LBM_HALO_MODE=stale / freshest).  Replaces the choice between the reference's
 * MPI_Waitall and MPI_Testall_OptimizedVersion programs (main loop :256-301 of the latter).
 * In stale mode every lbm_run call starts from freshly exchanged halos; from its second pass on, a
 * pass reads the halo rows its neighbours produced one pass earlier.  Every rank of a multi-process
 * run must select the same mode.  No effect on a single periodic slab.
 */
int      lbm_set_halo_mode(lbm_ctx* ctx, int mode);

/*
 * LBM_HALO_FRESHEST's record of what each look found: out[t * n_slabs + s], timesteps t < n_steps <= steps done,
 * slabs s of this context (n_slabs = info.n_slabs; 1 for rank contexts): bit 0 set = the south halo row of that
 * step was the neighbour's row of the same step, bit 1 = the north one; a clear bit = the row of the step before.
 * Steps run in the other modes read 3 (synchronous; first pass of every call) or are not recorded (stale).
 * The reference has no counterpart: its MPI_Testall result is discarded (d2q9-bgk.c:279-280).
 */
int      lbm_read_halo_log(lbm_ctx* ctx, unsigned char* out, int n_steps);

/* ---- the hot path ------------------------------------------------------------------------
 * lbm_run replaces n_steps trips of the driver loop (SerialCode/d2q9-bgk.c:166-170):
 *     timestep(params, cells, tmp_cells, obstacles);      // accelerate_flow, propagate,
 *                                                         // rebound, collision  (:207-407)
 *     av_vels[tt] = av_velocity(params, cells, obstacles); // (:409-458)
 * with no host round trip per step.  Per-step sums of |u| accumulate on the device.
 * lbm_sync waits for the device (call it before reading the clock, as the reference's
 * "Elapsed Compute time" brackets the loop, :162-185).
 *
 * A RESIDENT GIVE-UP FAILS THE CONTEXT FOR GOOD.  A launch of the resident kernel whose workgroups were not all running
 * at once gives up after its bound and leaves a status word; the lattice and every record are then invalid.  The call
 * that first sees the word -- lbm_sync, every reader (each synchronises first), lbm_run_timed, lbm_run_until and
 * lbm_run_until_residual, never lbm_run itself, which does not wait -- fails with "the resident kernel gave up ...", and
 * the context is FAILED until it is destroyed: every later call that takes it fails (NULL for pointer results) with
 *     "<function>: an earlier launch of the resident kernel gave up: the lattice and the records of this context or
 *      batch are invalid, and it stays failed until it is destroyed"
 * directly behind its NULL checks -- before "not armed", capacity and argument checks --, issues no device work, leaves
 * steps_done and the caller's output arrays as they were and sets its count outputs (*n_read, *n_samples, steps_run,
 * *kernel_ms_per_step) to 0.  lbm_destroy, lbm_get_info and lbm_rccl_info still work.  A batch fails as a whole: one
 * give-up in any of its launches fails the batch and every member, for every call but lbm_destroy_batch,
 * lbm_batch_get_info, lbm_batch_member and the three above on a member.  Nothing outlives the owner: a context created
 * afterwards is healthy.
 */
int lbm_run(lbm_ctx* ctx, int n_steps);
int lbm_sync(lbm_ctx* ctx);

/*
 * Same as lbm_run, additionally timing the step kernels with HIP events recorded on the
 * stream(s) the kernels are launched on.  *kernel_ms_per_step receives the average device
 * time of one timestep (max over slabs).
 */
int lbm_run_timed(lbm_ctx* ctx, int n_steps, float* kernel_ms_per_step);

/* ---- results -----------------------------------------------------------------------------
 * lbm_read_av_vels: out[t] = tot_u[t] / (float)fluid_cells for the first n recorded steps
 *   (the values main() stores at SerialCode/d2q9-bgk.c:169; fp32 division as :457).
 *   In a multi-process context the per-rank sums are first all-reduced (the reference's
 *   MPI_Reduce, MPI/d2q9-bgk.c:298-309); every rank receives the result.
 * lbm_read_cells: the owned rows of the lattice in the reference's AoS layout, so that
 *   write_values()/calc_reynolds() logic (:637-642, :662-743) can run on it unchanged.
 * lbm_read_final_state: u_x, u_y, |u|, pressure of the owned rows computed on the device
 *   with the formulas of write_values() (:684-719); blocked cells give 0,0,0,density*c_sq.
 * lbm_av_velocity: av_velocity() of the current lattice (:409-458) -- what calc_reynolds()
 *   (:637-642) multiplies; lbm_total_density: total_density() (:644-660).
 *   Both are global (all slabs / all ranks).
 */
int   lbm_read_av_vels(lbm_ctx* ctx, float* out, int n);
int   lbm_read_cells(lbm_ctx* ctx, float* cells_aos);
int   lbm_read_final_state(lbm_ctx* ctx, float* u_x, float* u_y, float* u_mag, float* pressure);
int   lbm_av_velocity(lbm_ctx* ctx, float* out);
int   lbm_total_density(lbm_ctx* ctx, double* out);
int   lbm_calc_reynolds(lbm_ctx* ctx, float* out);

/* ---- animation frames ----------------------------------------------------------------------
 * The reference's main loop writes a velocity-magnitude frame every 100 steps
 * (`if (tt % 100 == 0) write_animation_data(...)`, SerialCode/d2q9-bgk.c:171-173; the writer is :802-849).  Here the
 * running kernels record them on the device, without splitting the run:
 * lbm_set_frames(ctx, every, capacity): from now on, after global timestep tt (0-based, counted from the context's
 *   creation: the step that takes steps_done from tt to tt+1) with tt % every == 0, record the frame of the lattice after
 *   tt+1 timesteps: float[row_count][nx] over the owned rows, bit-identical to lbm_read_final_state's u_mag at that point
 *   (0 for blocked cells).  Recording never changes the lattice or av_vels.  Frames wait in a device buffer of `capacity`
 *   slots; an lbm_run / lbm_batch_run call that would record more frames than there are free slots fails before issuing
 *   any work.  every == 0 disarms and frees the buffer; re-arming discards unread frames.  Refused in LBM_HALO_STALE and
 *   LBM_HALO_FRESHEST (and lbm_set_halo_mode to those modes while armed).  Works on batch members too.
 * lbm_read_frames: drains up to max_frames oldest frames into out[n][row_count*nx] and steps[n] (their tt, may be NULL);
 *   out == NULL && steps == NULL: *n_read = frames waiting, nothing drained.  Synchronises like the other readers (a
 *   resident give-up: the rule at lbm_sync).
 */
int lbm_set_frames(lbm_ctx* ctx, int every, int capacity);
int lbm_read_frames(lbm_ctx* ctx, int max_frames, float* out, int* steps, int* n_read);

/* ---- point probes ---------------------------------------------------------------------------
 * The time series of the flow at chosen cells, recorded by the running kernels.  The reference can only print
 * av_vels per step (SerialCode/d2q9-bgk.c:169) and the whole field at the end (write_values, :662-743); a series at a
 * point costs it a write_values per step.
 * lbm_set_probes(ctx, n_probes, cells, every, capacity): from now on, after global timestep tt (0-based, counted from the
 *   context's creation, the numbering of lbm_set_frames) with tt % every == 0, record one sample row: for probe i the four
 *   values lbm_read_final_state gives at cells[i] (a GLOBAL cell) for the lattice after tt+1 timesteps, bit for bit; a
 *   blocked cell gives 0, 0, 0, density * c_sq.  every == 1 is the per-step series.  Duplicate cells are recorded twice;
 *   the order of a row is the caller's.  Recording never changes the lattice or av_vels.  Rows wait in a device ring of
 *   `capacity` rows (capacity * n_probes * 16 bytes); an lbm_run / lbm_batch_run call that would record more rows than are
 *   free fails before issuing any work.  n_probes == 0 or every == 0 disarms and frees; re-arming discards unread rows.
 *   Calls that run the resident kernel record inside it; other calls run as the sub-calls that end at their sample steps
 *   (every == 1: one-step passes -- correct, not fast; every a multiple of 4 keeps full-depth passes).
 *   Works on lbm_create / lbm_create_tiled contexts of any number of slabs and on batch members (each its own probes).
 *   Refused: n_probes outside [0, LBM_MAX_PROBES], a cell outside the grid, negative every, capacity < 1, a ring of
 *   2 GiB or more, rank contexts (lbm_create_rank*), LBM_HALO_STALE / LBM_HALO_FRESHEST (and lbm_set_halo_mode to those
 *   while armed), a context whose frames are armed (and lbm_set_frames while probes are armed: one recorder per
 *   context; in a batch one KIND of recorder per batch), lbm_run_until / lbm_batch_run_until while armed.
 * lbm_read_probes: drains up to max_samples oldest rows into out[n][n_probes] and steps[n] (their tt, may be NULL);
 *   out == NULL && steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises like the other readers (a
 *   resident give-up: the rule at lbm_sync).
 */
#define LBM_MAX_PROBES 256
typedef struct { int x, y; } lbm_probe;                               /* a GLOBAL cell, 0 <= x < nx, 0 <= y < ny */
typedef struct { float u_x, u_y, u_mag, pressure; } lbm_probe_sample; /* 16 bytes */
int lbm_set_probes(lbm_ctx* ctx, int n_probes, const lbm_probe* cells, int every, int capacity);
int lbm_read_probes(lbm_ctx* ctx, int max_samples, lbm_probe_sample* out /* [n][n_probes] */, int* steps, int* n_read);

/* ---- mean flow fields ------------------------------------------------------------------------
 * The time-averaged field of a flow that never settles (none of the reference's data sets does within maxIters,
 * SerialCode/d2q9-bgk.c:166; its only fields are the instant write_values prints at the end, :662-743): per-cell sums
 * over a window of samples, accumulated by the running kernels.  A million samples cost the memory of one.
 * lbm_set_mean(ctx, every), every >= 1: arms.  From now on, after global timestep tt (0-based, counted from the
 *   context's creation, the numbering of lbm_set_frames) with tt % every == 0, one sample is taken: at every owned cell
 *   the four floats lbm_read_final_state gives there for the lattice after tt+1 timesteps, bit for bit (a blocked cell
 *   gives 0, 0, 0, density * c_sq).  Each cell has four accumulators, each a DOUBLE that starts at +0.0 at arming and is
 *   updated as acc = acc + (double)sample, in step order.  The value after n samples is therefore defined exactly,
 *   whatever the calls, chunks, launches or kernels that produced it: it is what a float64 loop over the per-step
 *   final states gives.  (Sequential fp32 sums lose four to five digits over 10^5..10^6 samples of a value near 0.05.)
 *   There is no capacity: an armed lbm_run / lbm_batch_run never fails for lack of room.  Memory: 4 * 8 bytes per owned
 *   cell per slab, four planes double[rows][nx]; if they cannot be allocated the call fails, says the size, and leaves
 *   the context disarmed.  every == 0 disarms and frees; arming again zeroes the sums and the count.
 *   Recording never changes the lattice or av_vels.  Calls that run the resident kernel accumulate inside it
 *   (bit-identical lattice and av_vels); other calls run as the sub-calls that end at their sample steps, each followed
 *   by one accumulation pass (lattice and av_vels equal those of the same run issued as calls split there; every == 1:
 *   one-step passes -- correct, not fast; every a multiple of 4 keeps full-depth passes).
 *   Works on lbm_create / lbm_create_tiled contexts of any number of slabs and on batch members (each its own every;
 *   members arm independently).
 *   Refused: negative every; rank contexts (lbm_create_rank*); LBM_HALO_STALE / LBM_HALO_FRESHEST (and
 *   lbm_set_halo_mode to those while armed); a context whose frames or probes are armed (and lbm_set_frames /
 *   lbm_set_probes while the mean fields are: one recorder per context; in a batch one KIND of recorder per batch);
 *   lbm_run_until / lbm_batch_run_until while armed (a dropped look-ahead segment would have added its samples); on
 *   resident shapes with four-row bands, a lid row that is not an interior row of a band, and any shape whose mean form
 *   of the resident kernel does not fit a CU (the checks lbm_set_frames makes, against this form).
 * lbm_read_mean: the sums of the owned rows of all slabs, double[row_count * nx] each, row-major (y * nx + x); any of the
 *   four may be NULL; *n_samples (may be NULL) = samples since arming.  With all four NULL it only reports n_samples.
 *   It does NOT reset: for a windowed mean read, then arm again.  Synchronises like the other readers (a resident
 *   give-up: the rule at lbm_sync).  Fails on a context whose mean fields are not armed.
 */
int lbm_set_mean(lbm_ctx* ctx, int every);
int lbm_read_mean(lbm_ctx* ctx, double* sum_u_x, double* sum_u_y, double* sum_u_mag, double* sum_pressure,
                  long long* n_samples);

/* ---- second moments of the mean fields ---------------------------------------------------------
 * How much an unsteady flow moves about its mean: the variances of u_x, u_y and pressure and the Reynolds shear stress
 * <u'v'> follow from the sums above and the sums of the products u_x u_x, u_y u_y, u_x u_y, pressure pressure over the
 * same samples (var x = <x x> - <x>^2, <u'v'> = <u_x u_y> - <u_x><u_y>).
 * lbm_set_mean_order(ctx, every, order): order 1 is lbm_set_mean(ctx, every) in every respect
 *   but the name its error messages carry.  Order 2 arms the same
 *   recorder with EIGHT planes in one allocation per slab: planes 0..3 as lbm_set_mean defines them (bit-identical to
 *   an order-1 run), planes 4..7 the second moments.  On a sample step, with s = (u_x, u_y, |u|, pressure) the cell's
 *   four floats of that sample, additionally and in step order
 *     acc4 = acc4 + (double)u_x * (double)u_x        acc5 = acc5 + (double)u_y * (double)u_y
 *     acc6 = acc6 + (double)u_x * (double)u_y        acc7 = acc7 + (double)p   * (double)p
 *   This is defined exactly: the product of two floats has at most 24 + 24 = 48 significant bits and an exponent within
 *   2 * [-149, 128), so it is exact in a double (53 bits, exponents to +-1022); each update therefore has exactly ONE
 *   rounding, that of the addition, and gives the same bits whether the compiler evaluates it as a multiply and an add
 *   or contracts it into one fused multiply-add.  A blocked cell adds 0, 0, 0 and (density * c_sq)^2.
 *   Memory: 8 * 8 = 64 bytes per owned cell per slab; if that cannot be allocated the call fails, says the size, and
 *   leaves the context disarmed.  every == 0 disarms (any order 1 or 2); arming again, at either order, zeroes all
 *   sums and the count.  Everything lbm_set_mean refuses is refused, lbm_run_until / lbm_batch_run_until while armed
 *   too, and an order other than 1 or 2.  The resident kernel's mean form serves both orders (the order is a scalar it
 *   reads), so the fit check of lbm_set_mean is the check of the form that runs.  Batch members arm independently, each
 *   with its own every and its own order; orders may be mixed in a batch (one recorder kind).
 * lbm_read_mean2: the four sums of products, with the shape and rules of lbm_read_mean (any pointer may be NULL; all
 *   four NULL reports n_samples only; no reset; synchronises like the other readers; slabs stitched by their rows).
 *   Fails on a context that is not armed or armed at order 1.  lbm_read_mean works at either order.
 */
int lbm_set_mean_order(lbm_ctx* ctx, int every, int order);   /* order 1 or 2 */
int lbm_read_mean2(lbm_ctx* ctx, double* sum_uxux, double* sum_uyuy, double* sum_uxuy, double* sum_pp,
                   long long* n_samples);

/* ---- field frames -----------------------------------------------------------------------------
 * The time evolution of the flow field itself: what the reference's write_values prints once at the end
 * (SerialCode/d2q9-bgk.c:662-743; final_state.dat, which its visualize_4plots.py draws), recorded every N steps by the
 * running kernels, for a chosen subset of the four fields over a chosen rectangle -- the whole grid, a centreline
 * (the u_x / u_y profiles of the lid-driven cavity), or a region of interest on a grid whose whole frame is too large.
 * lbm_set_field_frames(ctx, every, capacity, fields, window): from now on, after global timestep tt (0-based, counted from
 *   the context's creation, the numbering of lbm_set_frames) with tt % every == 0, record one frame of the lattice after
 *   tt+1 timesteps: for every cell of the window and every selected field the float lbm_read_final_state gives there, bit
 *   for bit (a blocked cell gives 0, 0, 0, density * c_sq).  `fields` is a non-empty set of LBM_FIELD_* bits; `window`
 *   is a rectangle of GLOBAL cells [x0, x0+nx) x [y0, y0+ny) that does not wrap, NULL: the whole grid.  One frame is
 *   float[F][window.ny][window.nx], the F selected planes in ascending bit order: u_x, u_y, |u|, pressure.
 *   Frames wait in a device ring of `capacity` slots; an lbm_run / lbm_batch_run call that would record more field frames
 *   than there are free slots fails before issuing any work.  every == 0 disarms and frees; re-arming discards unread
 *   frames.  Memory: a slab holds only its own rows of the window (capacity * F * rows * window.nx * 4 bytes); a slab the
 *   window misses allocates nothing and does nothing on sample steps.  If a ring cannot be allocated the call fails, says
 *   the size, and leaves the context disarmed and whole.
 *   Recording never changes the lattice or av_vels.  Calls that run the resident kernel record inside it (bit-identical
 *   lattice and av_vels); other calls run as the sub-calls that end at their sample steps, each followed by one
 *   field_frame pass (lattice and av_vels equal those of the same run issued as calls split there).
 *   Works on lbm_create / lbm_create_tiled contexts of any number of slabs (frames are stitched by rows) and on batch
 *   members (each its own every, fields, window and capacity; in a batch one KIND of recorder per batch).
 *   Refused: negative every; capacity < 1 while arming; fields of 0 or outside LBM_FIELD_ALL; a window with nx < 1 or
 *   ny < 1 or one that leaves the grid; rank contexts (lbm_create_rank*); LBM_HALO_STALE / LBM_HALO_FRESHEST (and
 *   lbm_set_halo_mode to those while armed); a context with another recorder armed (and the other setters while this one
 *   is armed); lbm_run_until / lbm_batch_run_until while armed; on resident shapes with four-row bands, a lid row that is
 *   not an interior row of a band, and any shape whose field-frame form of the resident kernel does not fit a CU (the
 *   checks lbm_set_frames makes, against this form).
 * lbm_read_field_frames: drains up to max_frames oldest frames into out[n][F][window.ny][window.nx] and steps[n] (their
 *   tt, may be NULL); out == NULL && steps == NULL: *n_read = frames waiting, nothing drained.  Synchronises like the
 *   other readers (a resident give-up: the rule at lbm_sync).
 */
#define LBM_FIELD_UX       1
#define LBM_FIELD_UY       2
#define LBM_FIELD_UMAG     4
#define LBM_FIELD_PRESSURE 8
#define LBM_FIELD_ALL      15
typedef struct { int x0, y0, nx, ny; } lbm_window;   /* GLOBAL cells [x0, x0+nx) x [y0, y0+ny), no wrap */
int lbm_set_field_frames(lbm_ctx* ctx, int every, int capacity, int fields, const lbm_window* window /* NULL: whole grid */);
int lbm_read_field_frames(lbm_ctx* ctx, int max_frames, float* out, int* steps, int* n_read);

/* ---- obstacle forces ---------------------------------------------------------------------------
 * The force the fluid exerts on the obstacles -- drag, lift, the shedding frequency of a flow that oscillates (the
 * 1024x1024 data set) -- by momentum exchange over the boundary links.  The reference has no counterpart; the definition
 * rests on its lattice alone.  After a timestep the engine's lattice is bit-identical to the reference's, blocked cells
 * included: a blocked cell b then holds in speeds[k] the population that arrived over the link from b + c_k and was
 * turned round by rebound (SerialCode/d2q9-bgk.c, propagate + rebound, :239-301).  That population handed the solid the
 * momentum (c_opp(k) - c_k) f = -2 c_k f.
 * A BOUNDARY LINK is a pair (b, k), k in 1..8, with b blocked and b + c_k not blocked, the neighbour taken with both
 * periodic wraps.  For a set of links L the force of the step that produced the lattice `cells` is
 *     F_x = sum over (b,k) in L of (double)(-2 cx[k]) * (double)cells[b].speeds[k]
 *     F_y = sum over (b,k) in L of (double)(-2 cy[k]) * (double)cells[b].speeds[k]
 * Every term is exact in a double.  The sum is taken EXACTLY, in fixed point (csrc/lbm_exact_sum.h: integer additions of
 * the floats' mantissas at their places), and rounded to a double once, to nearest-even: the value Python's math.fsum
 * gives for the same terms.  It therefore has the same bits from run to run and from kernel path to kernel path -- a
 * single lbm_run, split calls, resident launches, stream launches, 1, 2 or 3 slabs -- which no double sum in a fixed order
 * can promise across slab counts (a slab's links are summed where the slab lives), and it differs from a double sum of
 * the same terms in any order by that sum's rounding only.  A population that is not finite makes the force of its body
 * NaN in that row.
 * Bodies: body_of_cell is an int[ny*nx] (GLOBAL cells, y * nx + x); entries on fluid cells are ignored, those on blocked
 * cells must lie in 0 .. n_bodies - 1.  A link belongs to the body of its blocked cell.  NULL: every blocked cell is body
 * 0 (n_bodies must then be 1 or more; bodies 1.. have no links).  1 <= n_bodies <= LBM_MAX_BODIES.  A body without links
 * reports 0, 0.
 * lbm_set_forces(ctx, n_bodies, body_of_cell, every, capacity): from now on, after global timestep tt (0-based, counted
 *   from the context's creation, the numbering of lbm_set_frames) with tt % every == 0, record one row: for each body
 *   {double f_x, f_y} of the lattice after tt+1 timesteps.  Rows wait in a device ring of `capacity` rows (capacity *
 *   n_bodies * 160 bytes per slab: the exact sums, rounded when read); an lbm_run call that would record more rows than are
 *   free fails before issuing any work.  every == 0 disarms and frees; re-arming discards unread rows.
 *   At arming each slab builds, on its device and from its uint8 mask (the neighbours of its first and last row are the
 *   mask's halo rows) and the labels, the list of the boundary links of its blocked cells, ordered by body, then cell
 *   index, then k: a context made by lbm_create_tiled needs no host map.  No step kernel records forces: every call runs
 *   as the sub-calls that end at its sample steps, each followed by one force_gather launch per slab on the slab's
 *   compute stream (every == 1: one-step passes -- correct, not fast).  On resident shapes the sub-calls of at least
 *   resident_min_steps timesteps run the resident kernel.  Recording never changes the lattice or av_vels: they equal
 *   those of the same run issued as calls split at the sample steps.
 *   Works on lbm_create / lbm_create_tiled contexts of any number of slabs; a link belongs to the slab that owns its
 *   blocked cell, and a row is the sum over the slabs.
 *   Refused: negative every; capacity < 1; n_bodies outside [1, LBM_MAX_BODIES]; a blocked cell whose body lies outside
 *   0 .. n_bodies - 1; a ring of 2 GiB or more; rank contexts (lbm_create_rank*); batch members (a batch arms them
 *   as a whole: lbm_batch_set_forces); LBM_HALO_STALE /
 *   LBM_HALO_FRESHEST (and lbm_set_halo_mode to those while armed); a context with another recorder armed (and the other
 *   setters while this one is armed); lbm_run_until while armed; a slab of more than 2^29 cells.
 *   Not offered: accumulation inside the resident or stream kernels, rank contexts, the double engine, torque.
 * lbm_read_forces: drains up to max_rows oldest rows into out[n][n_bodies][2] (f_x, f_y) and steps[n] (their tt, may be
 *   NULL); out == NULL && steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises like the other readers.
 * lbm_forces_links: links_per_body[b] = boundary links of body b over all slabs, b < n_bodies; fails unless armed.
 */
#define LBM_MAX_BODIES 64
int lbm_set_forces(lbm_ctx* ctx, int n_bodies, const int* body_of_cell /* or NULL */, int every, int capacity);
int lbm_read_forces(lbm_ctx* ctx, int max_rows, double* out /* [n][n_bodies][2] */, int* steps, int* n_read);
int lbm_forces_links(lbm_ctx* ctx, int* links_per_body /* [n_bodies] */);

/* ---- steady-state runs ----------------------------------------------------------------------
 * The reference runs a fixed number of timesteps (maxIters, SerialCode/d2q9-bgk.c:166); none of its data sets has
 * stopped changing by then.  lbm_run_until advances the lattice until its average velocity has, with the decision taken
 * on the device next to the per-step sums (four bytes come back per check), or until max_steps.
 * The criterion, with check_every = E >= 1, tol >= 0, patience = P >= 1, max_steps = N >= 0: the call runs segments of
 * E timesteps counted from its start.  After segment j (j = 1, 2, ...):
 *   av[s]  = the float lbm_read_av_vels returns for step s ((float)tot_u[s] / (float)fluid_cells), for its E steps;
 *   m_j    = (sum of av[s] as double) / (double)E, summed as a 64-lane reduction: lane i adds elements i, i+64, ... in
 *            turn, then acc[i] += acc[i+off] for off = 32, 16, ..., 1;
 *   r_j    = |m_j - m_(j-1)| / |m_j| from j = 2 on (m_j == 0: +inf, or 0 when both are 0); the check is met when
 *            r_j <= tol; `streak` counts consecutive checks met.
 * The run is steady when streak == P; the call ends with that segment, after j*E steps.  If N comes first the call ends
 * there, not steady; a last segment shorter than E is run and not checked.  Window means and patience rather than two
 * single values: an oscillating series (the 1024x1024 data set) crosses any single-value test on its zero crossings.
 * The call is synchronous (it returns when the answer is known) and advances steps_done by steps_run; lattice and
 * av_vels are exactly those of lbm_run(steps_run).  Single periodic slabs that run the resident kernel with
 * E >= resident_min_steps keep one segment in flight while the host waits for the verdict of the one before (segments of
 * at most resident_steps timesteps); a segment enqueued behind a "stop" is dropped without a trace.
 * Refused before any work is issued: steps_done + max_steps beyond the av_vels record, E < 1, P < 1, tol negative or
 * NaN, frames armed (lbm_set_frames), halo modes other than LBM_HALO_SYNC, multi-process (rank) contexts, contexts of
 * several slabs, batch members.
 * lbm_batch_run_until: the same for every member of a batch, one check launch for all; the batch stops when every member
 * is steady (or at N).  Members that are steady keep stepping with the others, so each stays bit-identical to an
 * lbm_create context advanced by *steps_run; out[i].steady_step tells when member i got there.
 */
typedef struct {
  int    steps_run;    /* timesteps this call advanced */
  int    steady;       /* 1: the criterion was met */
  int    steady_step;  /* steps of this call after which it was first met (-1: never) */
  int    checks;       /* checks made (r_j computed) until then */
  double last_rel;     /* r_j of the last of them (+inf when none was made) */
  double last_mean;    /* m_j of the last checked segment (0 when there was none) */
} lbm_steady_result;
int lbm_run_until(lbm_ctx* ctx, int max_steps, int check_every, double tol, int patience, lbm_steady_result* out);

/* ---- batches: many small lattices advanced together ---------------------------------------
 * A sweep over omega / accel / obstacle maps (each member reports its own calc_reynolds, :637-642) as ONE engine: B
 * independent single-slab lattices of one shape on one device, each advanced by n trips of the driver loop
 * (SerialCode/d2q9-bgk.c:166-170) per lbm_batch_run.  Every member's results are bit-identical to an lbm_create context
 * run on the same inputs.  Where the shape runs the resident kernel (lbm_info.resident_steps > 0), calls of at least
 * resident_min_steps timesteps advance members_per_launch members per launch of it -- 8 where one member fills one XCD
 * (lbm_info.resident_one_xcd), else as many as have a CU for each of their workgroups -- and launches_per_chunk launches,
 * one after the other on the batch's one stream, per chunk of up to resident_steps timesteps.  Shorter calls and other
 * shapes run the members one after another on the per-pass kernels (correct, not faster).
 *
 * params    : lbm_params[n_members]: one nx, ny and max_iters for all; density, accel, omega, reynolds_dim per member.
 * obstacles : int[n_members][ny*nx], as lbm_create's.
 * cells_aos : NULL (every member from the uniform equilibrium) or float[n_members][ny*nx*9].
 * lbm_batch_member: a borrowed handle of member `index`; the readers (lbm_read_av_vels, lbm_read_cells,
 *   lbm_read_final_state, lbm_av_velocity, lbm_total_density, lbm_calc_reynolds, lbm_get_info) work on it and see every
 *   batched launch; lbm_run / lbm_run_timed on it fail; lbm_destroy on it does nothing.  If a batched launch gives up
 *   waiting (its workgroups were not co-resident), the batch is failed as a whole (the rule at lbm_sync): the
 *   lbm_batch_sync that sees it reports it for every member, and afterwards every call on the batch or on any member
 *   fails, except lbm_destroy_batch, lbm_batch_get_info, lbm_batch_member and a member's lbm_get_info.
 */
typedef struct lbm_batch lbm_batch; /* opaque batch handle */
typedef struct {
  int members;            /* B */
  int members_per_launch; /* members one launch of the resident kernel advances (1 on the per-pass path) */
  int launches_per_chunk; /* ceil(members / members_per_launch): sub-batches, issued in turn on one stream */
  int resident_steps;     /* > 0: calls of at least resident_min_steps run batched, this many timesteps per chunk */
  int resident_min_steps;
  int steps_done;
} lbm_batch_info;
lbm_batch* lbm_create_batch(int n_members, const lbm_params* params, const int* obstacles, const float* cells_aos,
                            int math_mode);
lbm_ctx*   lbm_batch_member(lbm_batch* batch, int index);
int        lbm_batch_run(lbm_batch* batch, int n_steps);
int        lbm_batch_run_until(lbm_batch* batch, int max_steps, int check_every, double tol, int patience,
                               lbm_steady_result* out /* [members] */, int* steps_run);
int        lbm_batch_sync(lbm_batch* batch);
int        lbm_batch_get_info(const lbm_batch* batch, lbm_batch_info* out);
void       lbm_destroy_batch(lbm_batch* batch);

/* ---- obstacle forces of a batch -------------------------------------------------------------
 * A drag curve over omega or accel, or a comparison of obstacle shapes, as one engine: the forces of lbm_set_forces for
 * every member of a batch.  They are armed on the BATCH, not on a member: the batched launches must end at common sample
 * steps, so there is one `every` (and one n_bodies, one capacity) for all members.  The definition is lbm_set_forces',
 * member by member: the boundary links of the member's own obstacle map and labels, F = sum of (-2 c_k) f over a body's
 * links taken exactly and rounded once (math.fsum's value); a body of a member with a term that is not finite is NaN in
 * that row and nothing else is; a body without links reports +0, +0.
 * lbm_batch_set_forces(batch, n_bodies, body_of_cell, every, capacity): from now on, after global timestep tt (the
 *   batch's steps_done, the numbering of lbm_set_frames) with tt % every == 0, record one row: {double f_x, f_y} for every
 *   member and body.  body_of_cell is int[members][ny*nx], the labels of each member as lbm_set_forces takes them, or
 *   NULL: in every member all blocked cells are body 0.  1 <= n_bodies <= LBM_MAX_BODIES.  Rows wait in ONE device ring
 *   of `capacity` rows (capacity * members * n_bodies * 160 bytes); an lbm_batch_run that would record more rows than are
 *   free fails before issuing any work, and no member's steps_done moves.  every == 0 disarms and frees; re-arming
 *   discards unread rows.  At arming every member's list of links is built on the device as a slab's is.
 *   While armed, lbm_batch_run runs as the sub-calls that end at the sample steps: one of at least resident_min_steps
 *   timesteps on a resident shape is what lbm_batch_run of that length is otherwise (the batched resident kernel), a
 *   shorter one, or any on another shape, advances the members one after another on the per-pass kernels.  Behind each
 *   sub-call that ends at a sample step the batch's stream gets one memset of the row and ONE force_gather_batch launch for
 *   all members, whatever their number (every == 1: correct, not fast).  Member i's lattice, av_vels and rows are
 *   bit-identical to those of an lbm_create context with the same inputs, armed with lbm_set_forces(ctx, n_bodies, its
 *   labels, every, ...) and advanced by the same calls; recording never changes the lattice.
 *   Refused: negative every; capacity < 1; n_bodies outside [1, LBM_MAX_BODIES]; a blocked cell whose body lies outside
 *   0 .. n_bodies - 1 (the message names member, x, y and the label); a ring of 2 GiB or more; a member with a recorder
 *   armed (and every member-level setter while the batch's forces are armed: a batch records one kind);
 *   lbm_batch_run_until while armed.  lbm_set_forces on a member handle stays refused.
 * lbm_batch_read_forces: drains up to max_rows oldest rows into out[n][members][n_bodies][2] (f_x, f_y) and steps[n]
 *   (their tt, may be NULL); out == NULL && steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises.
 * lbm_batch_forces_links: links[m * n_bodies + b] = boundary links of body b of member m; fails unless armed.
 */
int lbm_batch_set_forces(lbm_batch* batch, int n_bodies, const int* body_of_cell /* [members][ny*nx] or NULL */,
                         int every, int capacity);
int lbm_batch_read_forces(lbm_batch* batch, int max_rows, double* out /* [n][members][n_bodies][2] */,
                          int* steps, int* n_read);
int lbm_batch_forces_links(lbm_batch* batch, int* links /* [members][n_bodies] */);

/* ---- lattice statistics ---------------------------------------------------------------------
 * Whether the lattice is still healthy, as a series: its mass (conserved by every step but accelerate_flow's rounding),
 * its momentum, the sum of |u|^2 (the distance from the low-Mach limit), the largest speed and where it is, and how
 * many cells have stopped being numbers.  The reference has av_vels and one end-of-run total_density (:644-660), a
 * double sum in one fixed order; a run that diverges tells neither when nor where.
 * One row describes a whole lattice.  For a cell with populations f[0..8], in fp32 without contraction, exactly as
 * lbm_read_final_state computes them (SerialCode/d2q9-bgk.c:684-719):
 *     rho  = ((((((((f0+f1)+f2)+f3)+f4)+f5)+f6)+f7)+f8)
 *     jx   = ((f1+f5)+f8) - ((f3+f6)+f7)        jy = ((f2+f5)+f6) - ((f4+f7)+f8)
 *     ux   = jx/rho    uy = jy/rho    usq = (ux*ux)+(uy*uy)    umag = sqrtf(usq)
 * A blocked cell contributes rho alone (it holds the populations rebound turned round, which are part of the mass); a
 * fluid cell contributes rho, jx, jy, usq and umag.  A cell is NON-FINITE when one of rho, jx, jy, usq is not finite
 * (a blocked cell: rho alone); such a cell contributes to nothing and is counted in `nonfinite`.
 *     mass = sum of rho over the finite cells;  mom_x, mom_y = sums of jx, jy over the finite fluid cells;
 *     sum_u_sq = sum of usq over them;  max_u = the largest umag among them, at the GLOBAL cell (max_x, max_y) -- of
 *     several cells with that umag the one with the smallest y*nx+x; 0 at -1, -1 when there is no finite fluid cell.
 * Every sum is taken EXACTLY (csrc/lbm_exact_sum.h, one float per cell and sum) and rounded to a double once: the value
 * math.fsum gives for the same terms.  The maximum does not depend on order either.  A row therefore has the same bits
 * from a single call, split calls, resident or per-pass kernels, 1, 2 or 3 slabs, a tiled context, a batch member, and
 * from run to run; `mass` differs from lbm_total_density by that function's double-sum rounding only.
 * lbm_set_stats(ctx, every, capacity): from now on, after global timestep tt (0-based, the numbering of lbm_set_frames)
 *   with tt % every == 0, record one row of the lattice after tt+1 timesteps.  Rows wait in a device ring of `capacity`
 *   rows (320 bytes per row and slab: the exact sums, rounded when read); an lbm_run that would record more rows than
 *   are free fails before issuing any work.  every == 0 disarms and frees; re-arming discards unread rows.  No step
 *   kernel records statistics: as with the forces every call runs as the sub-calls that end at its sample steps, each
 *   followed by one memset of the row and one stats_gather launch per slab (every == 1: correct, not fast).  Recording
 *   never changes the lattice or av_vels: they equal those of the same run issued as calls split at the sample steps.
 *   Refused: negative every; capacity < 1; a ring of 2 GiB or more; rank contexts (lbm_create_rank*); batch members (a
 *   batch arms them as a whole: lbm_batch_set_stats); LBM_HALO_STALE / LBM_HALO_FRESHEST (and lbm_set_halo_mode to
 *   those while armed); a context with another recorder armed (and the other setters while this one is armed);
 *   lbm_run_until while armed.  Not offered: the double engine, statistics inside the resident or stream kernels.
 * lbm_read_stats: drains up to max_rows oldest rows into out[n] and steps[n] (their tt, may be NULL); out == NULL &&
 *   steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises like the other readers.
 * lbm_batch_set_stats / lbm_batch_read_stats: the same for every member of a batch, armed on the BATCH with one `every`
 *   and ONE ring (capacity * members * 320 bytes); rows are out[n][members].  Behind each sub-call that ends at a sample
 *   step the batch's stream gets one memset of the row and ONE stats_gather_batch launch for all members.  Member i's
 *   rows, lattice and av_vels are bit-identical to those of an lbm_create context armed with lbm_set_stats and advanced
 *   by the same calls.  An lbm_batch_run without room fails before any work and moves no member's steps_done.  Refused
 *   as lbm_batch_set_forces refuses: a member with a recorder armed, the batch's forces armed (and every member-level
 *   setter and lbm_batch_set_forces while the statistics are armed); lbm_batch_run_until while armed.
 */
typedef struct {
  double    mass;         /* exact sum, rounded once */
  double    mom_x, mom_y;
  double    sum_u_sq;
  long long nonfinite;    /* cells left out of everything above and below */
  float     max_u;        /* largest |u| of a finite fluid cell; 0 when there is none */
  int       max_x, max_y; /* its GLOBAL cell; ties: the smallest y*nx+x; -1,-1 when there is none */
  int       reserved;     /* 0 */
} lbm_stats_row;          /* 56 bytes */
int lbm_set_stats(lbm_ctx* ctx, int every, int capacity);
int lbm_read_stats(lbm_ctx* ctx, int max_rows, lbm_stats_row* out, int* steps, int* n_read);
int lbm_batch_set_stats(lbm_batch* batch, int every, int capacity);
int lbm_batch_read_stats(lbm_batch* batch, int max_rows, lbm_stats_row* out /* [n][members] */, int* steps, int* n_read);

/* ---- velocity residuals ---------------------------------------------------------------------
 * How much the velocity field changed since it was last looked at, and where it still changes: the residual every CFD
 * code reports.  lbm_run_until decides on the change of ONE number, the mean of av_vels, in which local motion can
 * cancel; lbm_set_stats gives the sum of |u|^2 of an instant, not a change.
 * The REMEMBERED FIELD of a cell is the pair (u_x, u_y) that lbm_read_final_state gives for it: a fluid cell jx/rho,
 * jy/rho in fp32 with IEEE divide and no contraction (rho, jx, jy as in the statistics' text above), a blocked cell 0, 0.
 * lbm_set_residual(ctx, every, capacity) with every >= 1 takes the BASELINE: the field of the current lattice, after
 *   steps_done steps, stored in two planes float[rows][nx] per slab (8 bytes per owned cell).  From then on, after global
 *   timestep tt (0-based, the numbering of lbm_set_frames) with tt % every == 0, one row of the lattice after tt+1
 *   timesteps is recorded.  For every fluid cell, in fp32, no contraction, with (pux, puy) the remembered field:
 *       dux = ux - pux      duy = uy - puy      dsq = (dux*dux) + (duy*duy)      dmag = sqrtf(dsq)
 *       usq = (ux*ux) + (uy*uy)
 *   A fluid cell is NON-FINITE when one of rho, jx, jy, usq (the statistics' rule) or dsq is not finite; such a cell
 *   contributes to nothing and is counted in `nonfinite`.  Blocked cells contribute to nothing and are never counted.
 *   After the row is taken, the remembered field of every owned cell becomes the current (u_x, u_y), whatever its value.
 *       sum_du_sq, sum_u_sq = the sums of dsq and of usq over the finite fluid cells;  max_du = the largest dmag among
 *       them, at the GLOBAL cell (max_x, max_y) -- of several cells with that dmag the one with the smallest y*nx+x; 0 at
 *       -1, -1 when there is no finite fluid cell;  span = the timesteps between the remembered field and this sample:
 *       tt + 1 - (steps_done at arming) for the first row after arming, `every` afterwards.
 *   The relative L2 residual a user plots is sqrt(sum_du_sq / sum_u_sq), taken on the host in double.
 *   Every sum is taken EXACTLY (csrc/lbm_exact_sum.h) and rounded to a double once -- the value math.fsum gives for the
 *   same terms -- and the maximum does not depend on order.  A row therefore has the same bits from a single call, split
 *   calls, resident or per-pass sub-calls, 1, 2 or 3 slabs, a tiled context, a batch member, and from run to run.  With
 *   nonfinite == 0, sum_u_sq has the bits of lbm_stats_row.sum_u_sq at the same step.
 *   Rows wait in a device ring of `capacity` rows (160 bytes per row and slab: 2 x 9 limbs, the count, the key); an
 *   lbm_run that would record more rows than are free fails before issuing any work.  every == 0 disarms and frees the
 *   planes and the ring; arming again takes a new baseline and discards unread rows.  No step kernel records residuals:
 *   as with the statistics every call runs as the sub-calls that end at its sample steps, each followed by one memset of
 *   the row and one residual_gather launch per slab (every == 1: correct, not fast).  Recording never changes the lattice
 *   or av_vels: they equal those of the same run issued as calls split at the sample steps.  A failed allocation of the
 *   planes says their size and leaves the context disarmed.
 *   Refused, as lbm_set_stats refuses: negative every; capacity < 1; a ring of 2 GiB or more; rank contexts
 *   (lbm_create_rank*); batch members (a batch arms them as a whole: lbm_batch_set_residual); LBM_HALO_STALE /
 *   LBM_HALO_FRESHEST (and lbm_set_halo_mode to those while armed); a context with another recorder armed (and the other
 *   setters while this one is armed); lbm_run_until and lbm_run_until_residual while armed (the latter takes its own
 *   baseline and rows, see below).  Not offered: density or pressure residuals, the double engine, recording inside the
 *   resident or stream kernels.
 * lbm_read_residual: drains up to max_rows oldest rows into out[n] and steps[n] (their tt, may be NULL); out == NULL &&
 *   steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises like the other readers.
 * lbm_batch_set_residual / lbm_batch_read_residual: the same for every member of a batch, armed on the BATCH with one
 *   `every`, ONE ring (capacity * members * 160 bytes) and the planes of all members in one allocation; rows are
 *   out[n][members].  Arming takes ONE residual_gather_batch launch for the baselines of all members, and behind each
 *   sub-call that ends at a sample step the batch's stream gets one memset of the row and ONE launch for all members.
 *   Member i's rows, lattice and av_vels are bit-identical to those of an lbm_create context armed with lbm_set_residual
 *   and advanced by the same calls.  An lbm_batch_run without room fails before any work and moves no member's
 *   steps_done.  Refused as lbm_batch_set_stats refuses: a member with a recorder armed, the batch's forces or statistics
 *   armed (and every member-level setter, lbm_batch_set_forces and lbm_batch_set_stats while the residuals are armed);
 *   lbm_batch_run_until while armed.
 */
typedef struct {
  double    sum_du_sq;    /* exact sum of dsq over the finite fluid cells, rounded once (math.fsum's value) */
  double    sum_u_sq;     /* exact sum of usq over the same cells */
  long long nonfinite;
  float     max_du;       /* largest dmag of a finite fluid cell; 0 when there is none */
  int       max_x, max_y; /* its GLOBAL cell; ties: the smallest y*nx+x; -1,-1 when there is none */
  int       span;         /* timesteps between the remembered field and this sample */
} lbm_residual_row;       /* 40 bytes; offsets 0 8 16 24 28 32 36 */
int lbm_set_residual(lbm_ctx* ctx, int every, int capacity);
int lbm_read_residual(lbm_ctx* ctx, int max_rows, lbm_residual_row* out, int* steps, int* n_read);
int lbm_batch_set_residual(lbm_batch* batch, int every, int capacity);
int lbm_batch_read_residual(lbm_batch* batch, int max_rows, lbm_residual_row* out /* [n][members] */, int* steps, int* n_read);

/* ---- steady-state runs on the velocity residual ---------------------------------------------
 * lbm_run_until with the criterion every CFD code uses: the run is steady when the whole velocity field has stopped
 * changing, not when one number has (the mean of av_vels, in which local motion can cancel).  The quantity is the row of
 * lbm_set_residual, taken exactly, so a run stops at the same step and reports the same bits on every kernel path.  The
 * verdict is taken on the device (four bytes come back per check).  A run that blows up ends at the first check that
 * sees a fluid cell that is not finite, instead of stepping NaNs until max_steps.
 * With check_every = E >= 1, tol >= 0, patience = P >= 1, max_steps = N >= 0:
 *   BASELINE.  At its start the call takes the baseline: the remembered field (u_x, u_y) of the current lattice, exactly
 *     as lbm_set_residual defines it, into planes the call owns (8 bytes per cell, allocated by the first such call and
 *     kept with the context).  The recorder never sees them; nothing is armed before or after the call.
 *   ROW OF A CHECK.  The call runs segments of E timesteps counted from its start.  After segment j = 1, 2, ... one row is
 *     taken, precisely lbm_residual_row as lbm_set_residual defines it, with span = E; the sample then becomes the
 *     remembered field.  Because there is a baseline, segment 1 is already a check (unlike lbm_run_until): `checks`
 *     counts the segments judged.
 *   RESIDUAL.  r_j = sqrt(sum_du_sq / sum_u_sq) in IEEE double from the two exactly rounded sums, the division and the
 *     square root correctly rounded; both sums 0: r_j = 0; sum_u_sq == 0 < sum_du_sq: r_j = +inf (residual_l2's corners).
 *   VERDICT OF A CHECK.  nonfinite > 0: the check is not met, streak = 0, diverged = 1, and the call ends with this
 *     segment.  Otherwise the check is met iff r_j <= tol; `streak` counts consecutive checks met; the run is steady
 *     when streak == P, and the call ends with that segment, after j*E steps.
 *   CAP.  If N comes first the call ends there, not steady; a last segment shorter than E is run and not checked.
 *   WHAT THE CALL LEAVES.  The call is synchronous; lattice, av_vels and steps_done are exactly those of
 *     lbm_run(steps_run).
 *   HISTORY.  history[i], i < min(checks, history_capacity): the row of check i+1, taken after (i+1)*E steps of the call.
 *     history == NULL or history_capacity == 0: none.  The words of the rows stay on the device during the run (160
 *     bytes per row) and the rows are formed after it; the traffic per check stays the one stop word (0: go on, 1:
 *     steady, 2: diverged).
 *   Single periodic slabs that run the resident kernel keep one segment in flight as lbm_run_until does; everything a
 *   segment enqueued behind a "stop" would have done -- its acceleration, its sample, its check -- reads the stop word
 *   first, so it is dropped without a trace: no reported row, no state and no remembered cell moves.  Other shapes wait
 *   for each verdict.
 *   PRECISION.  In fp32 the residual does not fall to zero: on channel flows like the reference's it falls by four
 *   orders of magnitude and then sits on the rounding floor, r_j near 1e-5 (64x16 and 100x16, E = 512:
 *   1.0, 2.5e-4, 1.9e-5, 1.5e-5, 1.6e-5, ...).  A tol below that floor is never met.  r_j measures the change over E
 *   steps: above the floor it grows with E (a slowly drifting flow changes E times as much over E steps), so tol
 *   belongs to an E.
 *   Refused before any work is issued, everything lbm_run_until refuses: steps_done + max_steps beyond the av_vels
 *   record, E < 1, P < 1, tol negative or NaN, any recorder armed, halo modes other than LBM_HALO_SYNC, rank contexts,
 *   contexts of several slabs, batch members; also a negative history_capacity, a device history of 2 GiB or more, and
 *   planes or a history that cannot be allocated (the message says the size; the context stays usable).
 * lbm_batch_run_until_residual: the same for every member of a batch.  Every member has its own baseline, rows and
 *   verdict, taken by ONE residual_gather_batch launch and ONE check launch per segment whatever the number of members.
 *   A member's verdict freezes once it is steady or diverged; it keeps stepping with the others, so each member stays
 *   bit-identical to an lbm_create context advanced by *steps_run.  The batch ends when every member is steady or
 *   diverged, or at N.  history is [n][members], n = min(segments judged, history_capacity); a frozen member's later rows
 *   are still real rows (its out[i].last and last_rel are those of its own last check).  Refused: what
 *   lbm_batch_run_until refuses (a member or the batch with a recorder armed), and the history refusals above.
 */
typedef struct {
  int    steps_run;    /* timesteps this call advanced */
  int    steady;       /* 1: the criterion was met */
  int    steady_step;  /* steps of this call after which it was first met (-1: never) */
  int    checks;       /* checks made */
  int    diverged;     /* 1: the call ended at a check whose row has nonfinite > 0 */
  int    reserved;     /* 0 */
  double last_rel;     /* r_j of the last check (+inf when none was made) */
  lbm_residual_row last; /* the row of the last check (zeros, max_x = max_y = -1 when none) */
} lbm_residual_steady_result;   /* 72 bytes; offsets 0 4 8 12 16 20 24 32 */
int lbm_run_until_residual(lbm_ctx* ctx, int max_steps, int check_every, double tol, int patience,
                           lbm_residual_steady_result* out,
                           lbm_residual_row* history /* or NULL */, int history_capacity);
int lbm_batch_run_until_residual(lbm_batch* batch, int max_steps, int check_every, double tol, int patience,
                                 lbm_residual_steady_result* out /* [members] */, int* steps_run,
                                 lbm_residual_row* history /* [n][members] or NULL */, int history_capacity);

/* ---- line profiles --------------------------------------------------------------------------
 * The statistics resolved along one axis: one line of sums per row y (sums along x: u_x(y), the profile across the
 * channel) and one per column x (sums along y: the flow rate Q(x) = sum of jx, the mean density along the channel), every
 * `every` steps, without leaving the device.
 * Per fluid cell, in fp32 with IEEE divide and no contraction, rho, jx, jy, ux = jx/rho, uy = jy/rho and usq =
 * (ux*ux)+(uy*uy) exactly as the statistics' text above defines them.  A fluid cell is NON-FINITE when one of rho, jx, jy,
 * usq is not finite (the statistics' rule; usq finite implies ux and uy finite); such a cell adds to no sum and is
 * counted in `nonfinite` of its row line and of its column line.  Blocked cells contribute to nothing and are counted
 * nowhere.
 *     sum_rho, sum_jx, sum_jy, sum_ux, sum_uy = the sums over the line's finite fluid cells;  fluid = their number (the
 *     divisor of a mean);  nonfinite = the line's fluid cells left out.  fluid + nonfinite = the line's non-blocked cells.
 * Every sum is taken EXACTLY (csrc/lbm_exact_sum.h, one float per cell and sum) and rounded to a double once: the value
 * math.fsum gives for the same terms.  A line without finite fluid cells reports +0.0 five times and fluid == 0.  A
 * line therefore has the same bits from a single call, split calls, resident or per-pass kernels, 1, 2 or 3 slabs, a
 * tiled context, a batch member, and from run to run.
 * lbm_set_profiles(ctx, every, capacity, axes): from now on, after global timestep tt (0-based, the numbering of
 *   lbm_set_frames) with tt % every == 0, record one record of the lattice after tt+1 timesteps: ny row lines (line y,
 *   GLOBAL row) if axes & LBM_PROFILE_ROWS, then nx column lines (line x) if axes & LBM_PROFILE_COLUMNS; `lines` is ny, nx
 *   or ny + nx.  Records wait in a device ring of `capacity` slots.  A line occupies 48 int64 words (384 bytes: 5 x 9
 *   limbs, the two counts, one spare word); per slab one slot is (owned rows [if ROWS] + nx [if COLUMNS]) * 384 bytes: a
 *   slab's column lines hold its own rows' share, and the reader adds the slabs' limbs as integers before the one
 *   rounding.  An lbm_run that would record more records than there are free slots fails before issuing any work.
 *   every == 0 disarms and frees; re-arming discards unread records.  A failed allocation of the ring says its size and
 *   leaves the context disarmed.  No step kernel records profiles: as with the statistics every call runs as the sub-calls
 *   that end at its sample steps, each followed per slab by one memset of the record and one launch per selected axis
 *   (profile_rows, profile_columns; every == 1: correct, not fast).  Recording never changes the lattice or av_vels:
 *   they equal those of the same run issued as calls split at the sample steps.
 *   Refused, as lbm_set_stats refuses: negative every; capacity < 1; axes outside 1..3; a ring of 2 GiB or more; rank
 *   contexts (lbm_create_rank*); batch members (a batch arms them as a whole: lbm_batch_set_profiles); LBM_HALO_STALE /
 *   LBM_HALO_FRESHEST (and lbm_set_halo_mode to those while armed); a context with another recorder armed (and the other
 *   setters while this one is armed); lbm_run_until and lbm_run_until_residual while armed.  Not offered: the double
 *   engine, profiles inside the resident or stream kernels, windows, lines other than whole rows and columns.
 * lbm_read_profiles: drains up to max_records oldest records into out[n][lines] and steps[n] (their tt, may be NULL);
 *   out == NULL && steps == NULL: *n_read = records waiting, nothing drained.  Synchronises like the other readers.
 * lbm_batch_set_profiles / lbm_batch_read_profiles: the same for every member of a batch, armed on the BATCH with one
 *   `every`, one `axes` and ONE ring [slots][members][lines][48 words]; records are out[n][members][lines].  Behind each
 *   sub-call that ends at a sample step the batch's stream gets one memset of the record and ONE launch per selected axis
 *   for all members (profile_rows_batch, profile_columns_batch: grid z is the member).  Member i's records, lattice and
 *   av_vels are bit-identical to those of an lbm_create context armed with lbm_set_profiles and advanced by the same
 *   calls.  An lbm_batch_run without room fails before any work and moves no member's steps_done.  Refused as
 *   lbm_batch_set_stats refuses: a member with a recorder armed, the batch's forces, statistics or residuals armed (and
 *   every member-level setter and the three other batch-level setters while the profiles are armed); lbm_batch_run_until
 *   and lbm_batch_run_until_residual while armed.
 */
#define LBM_PROFILE_ROWS    1   /* one line per row y: sums along x -- u_x(y), the profile across the channel */
#define LBM_PROFILE_COLUMNS 2   /* one line per column x: sums along y -- Q(x), the pressure along the channel */
typedef struct {
  double sum_rho, sum_jx, sum_jy, sum_ux, sum_uy; /* exact sums over the line's finite fluid cells, each rounded once */
  int    fluid;      /* finite fluid cells on the line: the divisor of a mean */
  int    nonfinite;  /* fluid cells on the line left out of everything above */
} lbm_profile_line;  /* 48 bytes; offsets 0 8 16 24 32 40 44 */
int lbm_set_profiles(lbm_ctx* ctx, int every, int capacity, int axes);
int lbm_read_profiles(lbm_ctx* ctx, int max_records, lbm_profile_line* out /* [n][lines] */, int* steps, int* n_read);
int lbm_batch_set_profiles(lbm_batch* batch, int every, int capacity, int axes);
int lbm_batch_read_profiles(lbm_batch* batch, int max_records, lbm_profile_line* out /* [n][members][lines] */, int* steps, int* n_read);

/* ---- coarse frames --------------------------------------------------------------------------
 * The whole flow field at screen resolution: the line profiles' sums over the cells of a 2-D box instead of a line, so
 * that a frame of a grid far too large for per-cell frames (8192^2: 1 GiB for four fields) is a few hundred by a few
 * hundred lines that leave the device already rounded.
 * A box size is (bx, by) with 1 <= bx <= min(nx, LBM_COARSE_MAX_BOX) and 1 <= by <= min(ny, LBM_COARSE_MAX_BOX).  The
 * coarse grid has cx = ceil(nx / bx) by cy = ceil(ny / by) boxes; box (X, Y) covers the GLOBAL cells x in [X*bx,
 * min(nx, (X+1)*bx)) and y in [Y*by, min(ny, (Y+1)*by)).  The last box of an axis may be ragged; nothing wraps.
 * One box is one lbm_profile_line and holds exactly what a line of lbm_set_profiles holds, over the box's cells instead
 * of a line's: sum_rho, sum_jx, sum_jy, sum_ux, sum_uy over the box's finite fluid cells -- the per-cell values and the
 * rule for NON-FINITE cells are those of the line profiles' text above: the statistics' moments, IEEE divide, no
 * contraction -- fluid = the number of those cells, nonfinite = the box's fluid cells left out; blocked cells are counted
 * nowhere.  Every sum is taken EXACTLY and rounded to a double once: math.fsum's value, never -0.0; a box without finite
 * fluid cells reports +0.0 five times.  One frame is lbm_profile_line[cy][cx], row-major.
 * On the same lattice, bit for bit: with (bx, by) = (nx, 1) frame row Y is row line Y of lbm_set_profiles; with (1, ny)
 * box X is column line X; with (nx, ny) and nonfinite == 0, sum_jx and sum_jy are lbm_stats_row.mom_x and mom_y; with
 * (1, 1), on a finite fluid cell sum_ux and sum_uy are (double) of lbm_read_final_state's u_x and u_y, on a blocked cell
 * +0.0.  No bit depends on the slab count, on the kernel family that advanced the lattice, on how calls were split, on
 * batch membership, or on the run.
 * lbm_read_coarse(ctx, bx, by, out): the frame of the current lattice into out[cy][cx].  Needs nothing armed, changes
 *   nothing and works with any recorder armed (its slot is the call's own); synchronises like the other readers.  Works
 *   on lbm_create / lbm_create_tiled contexts of any slab count and on batch member handles; refused on rank contexts
 *   (lbm_create_rank*), whose boxes would be spread over the processes, and for a box outside the bounds above.
 * lbm_set_coarse_frames(ctx, every, capacity, bx, by): a gather kind with the semantics of lbm_set_profiles: from now on,
 *   after global timestep tt (0-based) with tt % every == 0, record one frame of the lattice after tt+1 timesteps into a
 *   device ring of `capacity` slots.  An lbm_run that would record more frames than there are free slots fails before
 *   issuing any work.  every == 0 disarms and frees; re-arming (with another box, too) discards unread frames.  No step
 *   kernel records: every call runs as the sub-calls that end at its sample steps, each followed per slab by one memset
 *   of the slot and ONE launch (coarse_gather); lattice and av_vels equal those of the same run issued as calls split at
 *   the sample steps.  A finished box leaves the device as its 48-byte line, rounded there (five roundings per box), not
 *   as its 48 limb words: a slab's slot is [its whole box rows][cx] lines, then -- only for its first and / or last box
 *   row where it shares that row with a neighbouring slab (one row where by exceeds the slab's rows) -- [0, 1 or 2
 *   partial box rows][cx] boxes of 48 int64 words (the line profiles' words), whose limbs the reader adds over the slabs
 *   as integers before the one rounding.  A single slab and a batch member have no partial rows: 48 bytes per box.
 *   Refused, as lbm_set_profiles refuses: negative every; capacity < 1; a ring of 2 GiB or more (the message gives the
 *   bytes per frame and slab); rank contexts; batch members (lbm_batch_set_coarse_frames arms the batch); LBM_HALO_STALE /
 *   LBM_HALO_FRESHEST (and lbm_set_halo_mode to those while armed); a context with another recorder armed (and every
 *   other setter while this one is armed); lbm_run_until and lbm_run_until_residual while armed; and a box side below
 *   1, above the grid's side, or above LBM_COARSE_MAX_BOX (the message names the side and the limit).  Not offered: the
 *   double engine, windows, boxes above 256 per side, recording inside the resident or stream kernels.
 * lbm_read_coarse_frames: drains up to max_frames oldest frames into out[n][cy][cx] and steps[n] (their tt, may be NULL);
 *   out == NULL && steps == NULL: *n_read = frames waiting, nothing drained.  Synchronises like the other readers.
 * lbm_batch_set_coarse_frames / lbm_batch_read_coarse_frames: the same for every member of a batch, armed on the BATCH
 *   with one `every`, one box and ONE ring [slots][members][cy][cx] of lines; frames are out[n][members][cy][cx].  Behind
 *   each sub-call that ends at a sample step the batch's stream gets one memset of the slot and ONE launch for all
 *   members (coarse_gather_batch: grid z is the member).  Member i's frames, lattice and av_vels are bit-identical to
 *   those of an lbm_create context armed with lbm_set_coarse_frames and advanced by the same calls.  An lbm_batch_run
 *   without room fails before any work and moves no member's steps_done.  Refused as lbm_batch_set_profiles refuses: a
 *   member with a recorder armed, another kind armed on the batch (and every member-level setter and the other
 *   batch-level setters while the coarse frames are armed); lbm_batch_run_until and lbm_batch_run_until_residual while
 *   armed.
 */
#define LBM_COARSE_MAX_BOX 256
int lbm_read_coarse(lbm_ctx* ctx, int bx, int by, lbm_profile_line* out /* [cy][cx] */);
int lbm_set_coarse_frames(lbm_ctx* ctx, int every, int capacity, int bx, int by);
int lbm_read_coarse_frames(lbm_ctx* ctx, int max_frames, lbm_profile_line* out /* [n][cy][cx] */, int* steps, int* n_read);
int lbm_batch_set_coarse_frames(lbm_batch* batch, int every, int capacity, int bx, int by);
int lbm_batch_read_coarse_frames(lbm_batch* batch, int max_frames, lbm_profile_line* out /* [n][members][cy][cx] */, int* steps, int* n_read);

/* ---- vorticity and enstrophy ----------------------------------------------------------------
 * The first field anyone draws of a lid-driven cavity or of a wake, and its integral: the series that tells whether a
 * shear layer is rolling up or decaying.  The one diagnostic here that is not local to a cell.
 * The velocity field U(x, y) = (u_x, u_y) is what lbm_read_final_state gives for the stored lattice: a fluid cell jx/rho,
 * jy/rho in fp32 with IEEE divide and no contraction (rho, jx, jy as in the statistics' text above), a blocked cell 0, 0
 * (the no-slip wall).  Neighbours are taken with both periodic wraps on the GLOBAL grid.  For every fluid cell, in fp32,
 * no contraction, in exactly this order (central differences over two cells, lattice units):
 *     dvdx = uy(x+1, y) - uy(x-1, y)        dudy = ux(x, y+1) - ux(x, y-1)
 *     w    = 0.5f * (dvdx - dudy)           wsq  = w * w
 * A blocked cell has w = 0 and contributes to nothing.  With nx == 1 or 2 the two x neighbours are the same cell and dvdx
 * is exactly 0 (of finite velocities); likewise ny == 2 and dudy.  A fluid cell is NON-FINITE when one of its own rho, jx,
 * jy, usq is not finite (the statistics' rule) or when w or wsq is not finite; such a cell adds to no sum and is counted
 * in `nonfinite`.  A NaN in one cell therefore counts that cell and its (up to four) fluid neighbours.
 *     enstrophy = sum of wsq over the finite fluid cells;  circulation = sum of w over them;  fluid = their number;
 *     max_abs_w = the largest |w| among them, at the GLOBAL cell (max_x, max_y) -- of several cells with that |w| the one
 *     with the smallest y*nx+x; 0 at -1, -1 when there is no finite fluid cell.
 * Both sums are taken EXACTLY (csrc/lbm_exact_sum.h, one float per cell and sum) and rounded to a double once: the value
 * math.fsum gives for the same terms.  The maximum is a 64-bit key (the bits of |w|, the cell) and does not depend on
 * order either.  A row therefore has the same bits from a single call, split calls, resident or per-pass sub-calls, 1, 2,
 * 3 or 8 slabs, a tiled context, a batch member, and from run to run.
 * lbm_read_vorticity(ctx, w): the field of the current lattice, w[row_count * nx] row-major, w as above, 0 on blocked
 *   cells; a non-finite w is stored as computed.  Synchronises like the other readers, needs nothing armed and changes
 *   nothing.  Works on lbm_create / lbm_create_tiled contexts of any slab count and on batch member handles; refused on
 *   rank contexts (lbm_create_rank*).
 * lbm_set_enstrophy(ctx, every, capacity): from now on, after global timestep tt (0-based, the numbering of
 *   lbm_set_frames) with tt % every == 0, record one row of the lattice after tt+1 timesteps.  Rows wait in a device ring
 *   of `capacity` rows (192 bytes per row and slab: the exact sums, rounded when read); an lbm_run that would record more
 *   rows than are free fails before issuing any work.  every == 0 disarms and frees; re-arming discards unread rows.  No
 *   step kernel records the enstrophy: as with the statistics every call runs as the sub-calls that end at its sample
 *   steps, each followed per slab by one memset of the row and one vorticity_gather launch (every == 1: correct, not
 *   fast).  The kernel reads the rows around a slab: on several slabs each slab keeps an edge buffer of two lattice rows,
 *   filled before every sample by device-to-device copies of its neighbours' boundary rows (behind their passes; their
 *   later passes run behind the copies) -- the lattice's halo rows are not used.  Recording never changes the lattice or
 *   av_vels: they equal those of the same run issued as calls split at the sample steps.
 *   Refused, as lbm_set_stats refuses: negative every; capacity < 1; a ring of 2 GiB or more; rank contexts
 *   (lbm_create_rank*); batch members (a batch arms it as a whole: lbm_batch_set_enstrophy); LBM_HALO_STALE /
 *   LBM_HALO_FRESHEST (and lbm_set_halo_mode to those while armed); a context with another recorder armed (and the other
 *   setters while this one is armed); lbm_run_until and lbm_run_until_residual while armed.  Not offered: the double
 *   engine, recording inside the resident or stream kernels, higher-order stencils, a command-line mode.  (The strain
 *   rate comes from the second moment, without a stencil: lbm_read_stress and lbm_set_stress below.)
 * lbm_read_enstrophy: drains up to max_rows oldest rows into out[n] and steps[n] (their tt, may be NULL); out == NULL &&
 *   steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises like the other readers.
 * lbm_batch_set_enstrophy / lbm_batch_read_enstrophy: the same for every member of a batch, armed on the BATCH with one
 *   `every` and ONE ring [slots][members][24 words]; rows are out[n][members].  Behind each sub-call that ends at a sample
 *   step the batch's stream gets one memset of the row and ONE vorticity_gather_batch launch for all members (grid z is
 *   the member).  Member i's rows, lattice and av_vels are bit-identical to those of an lbm_create context armed with
 *   lbm_set_enstrophy and advanced by the same calls.  An lbm_batch_run without room fails before any work and moves no
 *   member's steps_done.  Refused as lbm_batch_set_stats refuses: a member with a recorder armed, another kind armed on
 *   the batch (and every member-level setter and the four other batch-level setters while the enstrophy is armed);
 *   lbm_batch_run_until and lbm_batch_run_until_residual while armed.
 */
typedef struct {
  double    enstrophy;    /* exact sum of wsq over the finite fluid cells, rounded once (math.fsum's value) */
  double    circulation;  /* exact sum of w over the same cells */
  long long nonfinite;    /* fluid cells left out of everything above and below */
  float     max_abs_w;    /* largest |w| of a finite fluid cell; 0 when there is none */
  int       max_x, max_y; /* its GLOBAL cell; ties: the smallest y*nx+x; -1,-1 when there is none */
  int       fluid;        /* finite fluid cells counted */
} lbm_enstrophy_row;      /* 40 bytes; offsets 0 8 16 24 28 32 36 */
int lbm_read_vorticity(lbm_ctx* ctx, float* w /* [row_count*nx] */);
int lbm_set_enstrophy(lbm_ctx* ctx, int every, int capacity);
int lbm_read_enstrophy(lbm_ctx* ctx, int max_rows, lbm_enstrophy_row* out, int* steps, int* n_read);
int lbm_batch_set_enstrophy(lbm_batch* batch, int every, int capacity);
int lbm_batch_read_enstrophy(lbm_batch* batch, int max_rows, lbm_enstrophy_row* out /* [n][members] */, int* steps, int* n_read);

/* ---- stress and dissipation -----------------------------------------------------------------
 * The second moment of the populations: the one quantity a lattice Boltzmann code has locally that a finite-difference
 * code needs a stencil for.  The non-equilibrium momentum flux of a cell gives its strain-rate tensor, and from it the
 * viscous dissipation (the sink of the energy budget whose other terms are sum_u_sq, the forces and the enstrophy), the
 * shear rate and where it peaks, and the shear stress next to walls and obstacles.
 * Per cell from its populations f[0..8] of the stored lattice, in fp32 with IEEE divide and no contraction, in exactly
 * this order (rho, jx, jy, ux, uy and usq exactly as in the statistics' text above):
 *     a56 = f5+f6            a78 = f7+f8
 *     mxx = ((f1+f3)+a56)+a78          myy = ((f2+f4)+a56)+a78          mxy = (f5+f7)-(f6+f8)
 *     third = rho / 3.0f
 *     pxx = (mxx-third)-(jx*ux)        pyy = (myy-third)-(jy*uy)        pxy = mxy-(jx*uy)
 *     txx = pxx/rho    tyy = pyy/rho    txy = pxy/rho
 *     q   = ((txx*txx)+(tyy*tyy)) + (2.0f*(txy*txy))
 * (The second moments of the D2Q9 equilibrium are rho/3 + rho ux^2, rho/3 + rho uy^2 and rho ux uy exactly, so p_ab is
 * the non-equilibrium second moment Pi_ab.)  t_ab is the kinematic non-equilibrium stress of the STORED lattice, which is
 * post-collision: its non-equilibrium part is (1 - omega) times the pre-collision one, so the strain rate is
 *     S_ab = -c * t_ab,   c = 3 omega / (2 (1 - omega)),   S:S = c^2 * q,
 * and with nu = (1/omega - 1/2)/3 the dissipation of a row is 2 nu c^2 sum_q and its largest shear rate |c| sqrt(2 max_q).
 * The engine records t and q only: it does not know which omega the caller means to convert with, and at omega == 1 the
 * stored lattice is pure equilibrium and carries no stress -- t is rounding noise there (still well defined) and the
 * conversions of the Python package refuse it.
 * fp32 accuracy: mxx - third cancels rho/3 and keeps the roundings of mxx and of third, so txx and tyy carry an ABSOLUTE
 * error however small they are.  For populations >= 0, to first order in 2^-24 ("Stress and dissipation",
 * counts it from the expression tree; tests/stress_model.py asserts it cell by cell):
 *     |txx(fp32) - txx(exact)| <= 2^-24 * ((5 + 4|ux|) mxx/rho + 3 + 12 ux^2 + 10 |txx|)     about 4.7 * 2^-24; tyy alike
 *     |txy(fp32) - txy(exact)| <= 2^-24 * ((f5+f6+f7+f8 + |mxy| + 2 (|ux| myy + |uy| mxx) + |pxy|) / rho + 12 |ux uy| + 9 |txy|)
 * the second about (1/9 + 0.7 (|ux| + |uy|)) * 2^-24.  Measured on the 128 x 128 data set after 4000 steps: at most
 * 1.69 * 2^-24 in txx and tyy (1.01e-8 in pxx, pyy at rho = 0.1), 0.096 * 2^-24 in txy.
 * A blocked cell has t = 0 and q = 0 and contributes to nothing.  A fluid cell is NON-FINITE when one of rho, jx, jy, usq
 * (the statistics' rule), txx, tyy, txy or q is not finite; such a cell adds to no sum and is counted in `nonfinite`.
 *     sum_q = sum of q over the finite fluid cells;  sum_txy = sum of txy over them;  fluid = their number;
 *     max_q = the largest q among them, at the GLOBAL cell (max_x, max_y) -- of several cells with that q the one with
 *     the smallest y*nx+x; 0 at -1, -1 when there is no finite fluid cell.
 * Both sums are taken EXACTLY (csrc/lbm_exact_sum.h, one float per cell and sum) and rounded to a double once: the value
 * math.fsum gives for the same terms.  The maximum is the statistics' 64-bit key (the bits of q, which is >= +0, then
 * 0xffffffff - cell) and does not depend on order either.  A row therefore has the same bits from a single call, split
 * calls, resident or per-pass sub-calls, 1, 2, 3 or 8 slabs, a tiled context, a batch member, and from run to run.
 * lbm_read_stress(ctx, txx, txy, tyy): the three fields of the current lattice, each [row_count * nx] row-major, t as
 *   above, 0 on blocked cells; a non-finite value is stored as computed.  Any of the three may be NULL.  Synchronises like
 *   the other readers, needs nothing armed and changes nothing (a temporary device buffer per slab, freed before it
 *   returns).  Works on lbm_create / lbm_create_tiled contexts of any slab count and on batch member handles; refused on
 *   rank contexts (lbm_create_rank*).
 * lbm_set_stress(ctx, every, capacity): from now on, after global timestep tt (0-based, the numbering of lbm_set_frames)
 *   with tt % every == 0, record one row of the lattice after tt+1 timesteps.  Rows wait in a device ring of `capacity`
 *   rows (192 bytes per row and slab: the exact sums, rounded when read); an lbm_run that would record more rows than are
 *   free fails before issuing any work.  every == 0 disarms and frees; re-arming discards unread rows.  No step kernel
 *   records the stress: as with the statistics every call runs as the sub-calls that end at its sample steps, each
 *   followed per slab by one memset of the row and one stress_gather launch (every == 1: correct, not fast).  The kernel
 *   is pointwise: it reads a slab's owned rows only.  Recording never changes the lattice or av_vels: they equal those of
 *   the same run issued as calls split at the sample steps.
 *   Refused, as lbm_set_enstrophy refuses: negative every; capacity < 1; a ring of 2 GiB or more; rank contexts
 *   (lbm_create_rank*); batch members (a batch arms it as a whole: lbm_batch_set_stress); LBM_HALO_STALE /
 *   LBM_HALO_FRESHEST (and lbm_set_halo_mode to those while armed); a context with another recorder armed (and the other
 *   setters while this one is armed); lbm_run_until and lbm_run_until_residual while armed.  Not offered: a d2q9-bgk
 *   mode, the double engine, rank contexts, recording inside the resident or stream kernels, the pre-collision stress.
 * lbm_read_stress_rows: drains up to max_rows oldest rows into out[n] and steps[n] (their tt, may be NULL); out == NULL
 *   && steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises like the other readers.
 * lbm_batch_set_stress / lbm_batch_read_stress_rows: the same for every member of a batch, armed on the BATCH with one
 *   `every` and ONE ring [slots][members][24 words]; rows are out[n][members].  Behind each sub-call that ends at a sample
 *   step the batch's stream gets one memset of the row and ONE stress_gather_batch launch for all members (grid z is the
 *   member).  Member i's rows, lattice and av_vels are bit-identical to those of an lbm_create context armed with
 *   lbm_set_stress and advanced by the same calls.  An lbm_batch_run without room fails before any work and moves no
 *   member's steps_done.  Refused as lbm_batch_set_enstrophy refuses: a member with a recorder armed, another kind armed
 *   on the batch (and every member-level setter and the other batch-level setters while the stress is armed);
 *   lbm_batch_run_until and lbm_batch_run_until_residual while armed.
 */
typedef struct {
  double    sum_q;        /* exact sum of q over the finite fluid cells, rounded once (math.fsum's value) */
  double    sum_txy;      /* exact sum of txy over the same cells */
  long long nonfinite;    /* fluid cells left out of everything above and below */
  float     max_q;        /* largest q of a finite fluid cell; 0 when there is none */
  int       max_x, max_y; /* its GLOBAL cell; ties: the smallest y*nx+x; -1,-1 when there is none */
  int       fluid;        /* finite fluid cells counted */
} lbm_stress_row;         /* 40 bytes; offsets 0 8 16 24 28 32 36 */
int lbm_read_stress(lbm_ctx* ctx, float* txx /* [row_count*nx] or NULL */, float* txy /* likewise */, float* tyy /* likewise */);
int lbm_set_stress(lbm_ctx* ctx, int every, int capacity);
int lbm_read_stress_rows(lbm_ctx* ctx, int max_rows, lbm_stress_row* out, int* steps, int* n_read);
int lbm_batch_set_stress(lbm_batch* batch, int every, int capacity);
int lbm_batch_read_stress_rows(lbm_batch* batch, int max_rows, lbm_stress_row* out /* [n][members] */, int* steps, int* n_read);

/* ---- stream function ------------------------------------------------------------------------
 * The other field anyone draws of a lid-driven cavity, and the numbers it is validated by: the position of the primary
 * and the secondary vortex centres and psi at them (Ghia et al.).  The one recorded quantity that is a PREFIX along an
 * axis, not a total.
 * Mass flux: per cell of the stored lattice, in fp32, no contraction, jx = g1 + g5 + g8 - (g3 + g6 + g7) -- the jx of the
 * line profiles; rho, jy, ux, uy, usq as in the statistics' text above.  A fluid cell is NON-FINITE by the statistics'
 * rule: one of its rho, jx, jy, usq is not finite.
 * Term of a cell: t(x, y) = jx of a finite fluid cell; t(x, y) = 0 of a blocked cell and of a non-finite fluid cell.  (A
 * blocked cell holds rebounded populations whose jx is not 0: it adds nothing.)
 * The mass stream function is the inclusive prefix along y from the GLOBAL row 0:
 *     psi(x, y) = round_to_double( exact sum of t(x, y') for y' = 0 .. y )
 * The sum is taken EXACTLY (csrc/lbm_exact_sum.h) and rounded once, to nearest-even: math.fsum's value of the same terms.
 * It is defined at every cell, blocked ones included: inside a wall psi is the wall's constant.  The exact sum never
 * yields -0.0: a zero psi is +0.0.  Two ties to the rest, both bit for bit: psi(x, ny - 1) equals sum_jx of column line x
 * of lbm_set_profiles on the same lattice; and no psi depends on the number of slabs, on the band height of the scan
 * (LBM_PSI_BAND_ROWS), on the kernel family that advanced the lattice, or on how the calls were split.
 * Extrema: over the finite fluid cells, compared as the rounded doubles (+0.0 and -0.0 are equal): psi_min at the GLOBAL
 * cell (min_x, min_y), psi_max at (max_x, max_y); of several cells with that value the one with the smallest y*nx+x; 0 at
 * -1, -1 when there is no finite fluid cell.
 * lbm_read_psi(ctx, psi): the field of the current lattice, psi[row_count * nx] row-major.  Synchronises like the other
 *   readers, needs nothing armed and changes nothing.  Works on lbm_create / lbm_create_tiled contexts of any slab count
 *   and on batch member handles; refused on rank contexts (lbm_create_rank*).
 * lbm_set_psi(ctx, every, capacity): from now on, after global timestep tt (0-based, the numbering of lbm_set_frames)
 *   with tt % every == 0, record one row of the lattice after tt+1 timesteps.  Rows wait in a device ring of `capacity`
 *   rows (64 bytes per row and slab); an lbm_run that would record more rows than are free fails before issuing any
 *   work.  every == 0 disarms and frees; re-arming discards unread rows.  No step kernel records psi: as with the
 *   statistics every call runs as the sub-calls that end at its sample steps, each followed per slab by a scan of three
 *   sweeps over bands of rows -- psi_band_totals (a column's exact limbs per band), psi_band_bases (their exclusive
 *   prefix over the bands), psi_scan (the band's rows again from its base, one rounding per cell, the extrema kept) -- and
 *   psi_extrema (every == 1: correct, not fast).  On several slabs slab s+1 starts from the limbs of everything below
 *   it: slab s leaves them in a buffer of its own, copied device to device behind an event; only these recorder-owned
 *   buffers cross slabs -- the lattice's halo rows are not used.  The band height is chosen from the grid; LBM_PSI_BAND_ROWS
 *   (read once per context, at its first scan) overrides it and never changes a bit.  Recording never changes the lattice
 *   or av_vels: they equal those of the same run issued as calls split at the sample steps.
 *   Refused, as lbm_set_enstrophy refuses: negative every; capacity < 1; a ring of 2 GiB or more; rank contexts
 *   (lbm_create_rank*); batch members (a batch arms it as a whole: lbm_batch_set_psi); LBM_HALO_STALE /
 *   LBM_HALO_FRESHEST (and lbm_set_halo_mode to those while armed); a context with another recorder armed (and the other
 *   setters while this one is armed); lbm_run_until and lbm_run_until_residual while armed.  Not offered: psi of u
 *   instead of j, trapezoid weights, the double engine, rank contexts, recording inside the resident or stream kernels,
 *   a command-line (d2q9-bgk) mode.
 * lbm_read_psi_rows: drains up to max_rows oldest rows into out[n] and steps[n] (their tt, may be NULL); out == NULL &&
 *   steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises like the other readers.
 * lbm_batch_set_psi / lbm_batch_read_psi_rows: the same for every member of a batch, armed on the BATCH with one `every`
 *   and ONE ring [slots][members][8 words]; rows are out[n][members].  Behind each sub-call that ends at a sample step the
 *   batch's stream gets ONE launch of each of the four kernels for all members (grid z is the member).  Member i's rows,
 *   lattice and av_vels are bit-identical to those of an lbm_create context armed with lbm_set_psi and advanced by the
 *   same calls.  An lbm_batch_run without room fails before any work and moves no member's steps_done.  Refused as
 *   lbm_batch_set_enstrophy refuses: a member with a recorder armed, another kind armed on the batch (and every
 *   member-level setter and the five other batch-level setters while psi is armed); lbm_batch_run_until and
 *   lbm_batch_run_until_residual while armed.
 */
typedef struct {
  double    psi_min, psi_max;   /* over the finite fluid cells; 0, 0 when there is none */
  long long nonfinite;          /* fluid cells that added nothing and were left out of the extrema */
  int       min_x, min_y;       /* GLOBAL cell of psi_min; ties: smallest y*nx+x; -1,-1 when none */
  int       max_x, max_y;
  int       fluid;              /* finite fluid cells */
  int       reserved;           /* 0 */
} lbm_psi_row;                  /* 48 bytes; offsets 0 8 16 24 28 32 36 40 44 */
int lbm_read_psi(lbm_ctx* ctx, double* psi /* [row_count*nx] */);
int lbm_set_psi(lbm_ctx* ctx, int every, int capacity);
int lbm_read_psi_rows(lbm_ctx* ctx, int max_rows, lbm_psi_row* out, int* steps, int* n_read);
int lbm_batch_set_psi(lbm_batch* batch, int every, int capacity);
int lbm_batch_read_psi_rows(lbm_batch* batch, int max_rows, lbm_psi_row* out /* [n][members] */, int* steps, int* n_read);

/* ---- tracer particles -------------------------------------------------------------------------
 * Where the fluid goes: every other recorder says what happens at a cell.  n massless particles are advected on the
 * device through the velocity field of the stored lattice, once per sample step, and their positions recorded: pathlines,
 * streaklines, residence times, the stirring of a blob of dye, without the lattice leaving the device.
 *
 * A tracer is a position (x, y) in doubles, 0 <= x < nx and 0 <= y < ny; the centre of cell (i, j) lies at (i, j).
 * u(i, j) is the pair of floats lbm_read_final_state gives at that cell for the current lattice, bit for bit (the exact
 * arithmetic's moments; a blocked cell gives 0, 0), each widened to double.
 *   Interpolation V(x, y): i0 = floor(x), fx = x - i0, i1 = i0 + 1, or 0 when that equals nx; j0, fy, j1 likewise in y.
 *     Per component  a = u[j0][i0] + fx * (u[j0][i1] - u[j0][i0]),  b = u[j1][i0] + fx * (u[j1][i1] - u[j1][i0]),
 *     v = a + fy * (b - a).  Every +, -, * is one IEEE double operation in that order; nothing is fused.
 *   Wrap W(z, n) = z - n * floor(z / n); a result outside [0, n) (rounding: z = -1e-300 gives n) becomes 0.0.  W is total
 *     on the finite doubles and the identity on [0, n); of a z that is not finite it is NaN.
 *   One advance over a span of h timesteps, H = (double)h: the midpoint rule in the field of the sample step, held over
 *     the span:  v1 = V(x, y);  xm = W(x + (0.5 * H) * v1x, nx), ym likewise;  v2 = V(xm, ym);
 *     x' = W(x + H * v2x, nx), y' likewise.
 *   Lost tracers: if v1, v2, xm, ym, x' or y' is not finite the tracer is lost: its position becomes (NaN, NaN) and stays
 *     so.  No index is ever formed from a position that is not finite; a lost tracer is skipped and written through.
 *   The span h is the number of timesteps since the previous sample, or since arming for the first sample (the rule of
 *     lbm_residual_row.span): `every`, except for the first sample of a recorder armed between two sample steps.
 * (csrc/lbm_tracer_step.h is this definition as code, for the kernel and for the CPU check alike; tests/tracer_model.py
 * is its numpy model, written from the lines above.)
 * Guidance: keep h * |u| well under one cell -- the field is held over the span and the midpoint rule is second order
 * in h * |grad u|; every = 4 to 16 at the usual |u| <= 0.1 does that and keeps the passes at their full depth.  The
 * velocity falls linearly to 0 at the centres of blocked cells, so a tracer at rest inside a body stays there.  Tracers
 * seeded in row-major order (lbm_asynchronous_amd.tracer_seeds) share cache lines; a random order costs a line per cell.
 *
 * lbm_set_tracers(ctx, n, start, every, capacity): from now on, after global timestep tt (0-based, the numbering of
 *   lbm_set_frames) with tt % every == 0, all n tracers advance once over the span and the row, the n positions after the
 *   advance in the caller's order, goes into a device ring of `capacity` rows.  As with the statistics every call runs as
 *   the sub-calls that end at its sample steps, each followed by ONE tracer_advance launch, a lane per tracer, which reads
 *   the current lattice directly (two dependent gathers of 4 cells x 9 populations and 4 mask bytes) and updates the
 *   positions in place; no step kernel knows of it, and the lattice and av_vels equal those of the same run issued as
 *   calls split at the sample steps.  capacity == 0 arms WITHOUT a ring: nothing is recorded, no run lacks room,
 *   lbm_read_tracers refuses and the positions come from lbm_tracers_now -- for a cloud of many tracers read once at the
 *   end.  every == 0 or n == 0 disarms and frees; re-arming discards the positions and the rows.
 *   Refused, before anything is released: negative every or capacity; n outside 0 .. LBM_MAX_TRACERS; a NULL start; a
 *   context of more than one slab (a tracer's four cells can straddle two slabs, and a slab's lattice halo rows are not
 *   current after a pass); a ring of 2 GiB or more; rank contexts (lbm_create_rank*); batch members (a batch arms them
 *   as a whole: lbm_batch_set_tracers); a start position that is not finite or lies outside the grid (the first such
 *   index is named); LBM_HALO_STALE / LBM_HALO_FRESHEST (and lbm_set_halo_mode to those while armed); a context with
 *   another recorder armed (and the other setters while this one is armed); lbm_run_until and lbm_run_until_residual
 *   while armed.  Not offered: several slabs, rank contexts, the double engine, finite-size or inertial particles,
 *   unwrapped coordinates, seeding during a run.
 * lbm_read_tracers: drains up to max_rows oldest rows into out[n_read][n] and steps[n_read] (their tt, may be NULL);
 *   out == NULL && steps == NULL: *n_read = rows waiting, nothing drained.  Synchronises like the other readers.
 * lbm_tracers_now: the current positions, out[n]: those of the last sample (of arming before the first).  Drains nothing;
 *   synchronises like the readers.
 * lbm_batch_set_tracers / lbm_batch_read_tracers / lbm_batch_tracers_now: the same for every member of a batch, n tracers
 *   each, armed on the BATCH with one `every` and ONE ring [slots][members][n]; start and the positions are [members][n],
 *   rows out[n_read][members][n].  Behind each sub-call that ends at a sample step the batch's stream gets ONE
 *   tracer_advance_batch launch for all members (grid z is the member).  Member i's rows, lattice and av_vels are
 *   bit-identical to those of an lbm_create context armed with lbm_set_tracers and advanced by the same calls.  Refused
 *   as lbm_batch_set_stress refuses, and what lbm_set_tracers refuses of n, start and the ring.
 */
#define LBM_MAX_TRACERS (1 << 24)
typedef struct {
  double x, y;
} lbm_tracer;             /* 16 bytes */
int lbm_set_tracers(lbm_ctx* ctx, int n, const lbm_tracer* start /* [n] */, int every, int capacity);
int lbm_read_tracers(lbm_ctx* ctx, int max_rows, lbm_tracer* out /* [rows][n] */, int* steps, int* n_read);
int lbm_tracers_now(lbm_ctx* ctx, lbm_tracer* out /* [n] */);
int lbm_batch_set_tracers(lbm_batch* batch, int n, const lbm_tracer* start /* [members][n] */, int every, int capacity);
int lbm_batch_read_tracers(lbm_batch* batch, int max_rows, lbm_tracer* out /* [rows][members][n] */, int* steps, int* n_read);
int lbm_batch_tracers_now(lbm_batch* batch, lbm_tracer* out /* [members][n] */);

/* ---- double precision -----------------------------------------------------------------------
 * The reference's programs are `float`, but its published golden results (the .dat files of check/) are its algorithm evaluated in
 * IEEE double.  A double context computes exactly that: the driver loop of SerialCode/d2q9-bgk.c:166-170 with every
 * `float` read as `double`, `sqrtf` as `sqrt` and every `1.f`-style literal as a double literal.  Each expression tree of
 * :207-458 is kept, with IEEE / and sqrt and no contraction:
 *   accelerate_flow adds a1 = density*accel/9.0 and a2 = density*accel/36.0 (:219-220);
 *   the constant divides (u / c_sq, (u*u) / (2 c_sq c_sq), u_sq / (2 c_sq)) are divides -- the exhaustive check that let
 *     the fp32 kernels multiply instead cannot be made over doubles;
 *   tot_u[t] is the double sum of |u| over the fluid cells after step t+1 in the kernels' fixed order (the same bits
 *     from run to run), and av_vels[t] = tot_u[t] / (double)fluid_cells (:457);
 *   final_state's blocked cells give 0, 0, 0, density * c_sq.
 * The run constants are doubles: 1.85 is the double 1.85, not (double)1.85f.  Layouts are the fp32 entry points' with
 * double elements: cells_aos double[ny*nx*9], obstacles int[ny*nx], fields double[ny*nx] row-major.
 * lbm_double_ctx is NOT an lbm_ctx: no fp32 entry point takes one.  One periodic slab on device 0, one timestep per
 * launch (two cells per lane where nx is even, else one: lbm_double_info.lane_cells), every launch on one stream.
 * Not offered in double: several slabs and rank contexts; recorders (frames, probes, mean fields); batches;
 * lbm_run_until; the resident kernel and the multi-step kernels; hipGraph replay.
 * Errors, lbm_last_error and the die() message are those of the fp32 entry points; lbm_double_run fails before any
 * work when steps_done + n_steps exceeds max_iters.  The functions mirror their fp32 namesakes (lbm_create, lbm_run,
 * lbm_run_timed, lbm_sync, lbm_read_av_vels, lbm_read_cells, lbm_read_final_state, lbm_av_velocity, lbm_total_density,
 * lbm_calc_reynolds, lbm_get_info).
 */
typedef struct {
  int    nx, ny, max_iters, reynolds_dim; /* as lbm_params */
  double density, accel, omega;
} lbm_params_double;
typedef struct lbm_double_ctx lbm_double_ctx; /* opaque; not an lbm_ctx */
typedef struct {
  int fluid_cells; /* non-blocked cells (av_velocity's divisor) */
  int steps_done;
  int lane_cells;  /* 2: step_double (even nx), 1: step_double_scalar */
  int nontemporal; /* 1: step_double stores with the nontemporal hint (lattice pair beyond 512 MiB) */
} lbm_double_info;
lbm_double_ctx* lbm_double_create(const lbm_params_double* params, const int* obstacles, const double* cells_aos /* or NULL */);
void  lbm_double_destroy(lbm_double_ctx* ctx);
int   lbm_double_get_info(const lbm_double_ctx* ctx, lbm_double_info* out);
int   lbm_double_run(lbm_double_ctx* ctx, int n_steps);
int   lbm_double_run_timed(lbm_double_ctx* ctx, int n_steps, float* kernel_ms_per_step);
int   lbm_double_sync(lbm_double_ctx* ctx);
int   lbm_double_read_av_vels(lbm_double_ctx* ctx, double* out, int n);
int   lbm_double_read_cells(lbm_double_ctx* ctx, double* cells_aos);
int   lbm_double_read_final_state(lbm_double_ctx* ctx, double* u_x, double* u_y, double* u_mag, double* pressure);
int   lbm_double_av_velocity(lbm_double_ctx* ctx, double* out);
int   lbm_double_total_density(lbm_double_ctx* ctx, double* out);
int   lbm_double_calc_reynolds(lbm_double_ctx* ctx, double* out);

#ifdef __cplusplus
}
#endif
#endif /* LBM_HIP_H */
