// lbm_hip.hip -- host side of the C-ABI engine declared in include/lbm_hip.h.
//
// Owns the device lattices (row slabs, one per GPU), the per-step launch sequence, the halo
// exchange (RCCL send/recv on a side stream, overlapped with the interior rows -- the GPU
// analogue of /root/reference/MPI_Waitall/d2q9-bgk.c:225-253) and the result read-back.
// No CPU compute path exists here: without a HIP device every compute entry point fails.
#include "../../include/lbm_hip.h"
#include "lbm_kernels.hip.h"
#include "lbm_own.h"
#include "lbm_plan.h"
#include "lbm_ring.h"
#include "lbm_segments.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <dlfcn.h>
#include <algorithm>

#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

namespace {

// the kernel plan (lbm_plan.h): what plan_kernels decided for a context, and the arithmetic the launches share with it
using lbm_plan::KernelPlan;
using lbm_plan::PlanInput;
using lbm_plan::SlabRows;
using lbm_plan::HALO_SELF;
using lbm_plan::HALO_MEMCPY;
using lbm_plan::HALO_RCCL;
using lbm_plan::HALO_HOST;
using lbm_plan::ceil_div;
using lbm_plan::round_up;
using lbm_plan::env_int;
using lbm_plan::kMaxSlabs;
using lbm_plan::kMaxBandGroups;
using lbm_plan::kHaloRows;
using lbm_plan::kMaskHalo;
using lbm_plan::kTileDims;
static_assert(lbm_plan::kBlock == lbm::kBlock && lbm_plan::kNoRow == lbm::kNoRow, "lbm_plan.h mirrors the kernels' constants");
constexpr int kPartSlots = lbm::kPartSlotsMax;  // steps whose partial sums are buffered before one reduce launch

// ---- error handling (reference: die(), SerialCode/d2q9-bgk.c:745-751) -----------------------
int g_error_mode = LBM_ERRORS_DIE;
thread_local char g_last_error[1024] = "";

void raise_error(int line, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
  if (g_error_mode == LBM_ERRORS_DIE) {
    fprintf(stderr, "Error at line %d of file %s:\n", line, __FILE__);
    fprintf(stderr, "%s\n", g_last_error);
    fflush(stderr);
    exit(EXIT_FAILURE);
  }
}

#define LBM_FAIL(ret, ...)              \
  do {                                  \
    raise_error(__LINE__, __VA_ARGS__); \
    return ret;                         \
  } while (0)

#define HIP_TRY(ret, expr)                                                              \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) LBM_FAIL(ret, "HIP error: %s (%s)", hipGetErrorString(e_), #expr); \
  } while (0)

#define NCCL_TRY(ret, expr)                                                               \
  do {                                                                                    \
    ncclResult_t r_ = (expr);                                                             \
    if (r_ != ncclSuccess) LBM_FAIL(ret, "RCCL error: %s (%s)", g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?", #expr); \
  } while (0)

// ---- RCCL, bound at first use -----------------------------------------------------------------------------------
// The library is NOT a link-time dependency: a single-GPU run never loads it, and WHICH librccl serves a multi-GPU
// run is a decision taken here, not an accident of load order:
//   1. LBM_RCCL_LIB=<path>: that file (RTLD_LOCAL | RTLD_DEEPBIND);
//   2. a librccl.so.1 the process has already mapped -- a host that imported PyTorch first carries torch's bundled
//      RCCL together with torch's bundled HIP runtime (both resolve by soname before anything of this engine loads),
//      and a communicator must come from the RCCL built for the HIP runtime it runs on;
//   3. ROCm's own, /opt/rocm/lib/librccl.so.1 (then the bare soname): the C host program and torch-free hosts.
// lbm_rccl_info() reports which one it was, its version and what the communicator says about the ring.
struct RcclApi {
  void* handle = nullptr;
  char path[512] = "";
  ncclResult_t (*GetVersion)(int*) = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;
std::once_flag g_rccl_once;
char g_rccl_error[768] = "";

void rccl_bind() {
  RcclApi& r = g_rccl;
  const char* forced = getenv("LBM_RCCL_LIB");
  if (forced && *forced) {
    r.handle = dlopen(forced, RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
    if (!r.handle) { snprintf(g_rccl_error, sizeof(g_rccl_error), "LBM_RCCL_LIB=%s: %s", forced, dlerror()); return; }
  } else {
    r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);  // already in the process (e.g. PyTorch's)
    if (!r.handle) r.handle = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!r.handle) r.handle = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!r.handle) { snprintf(g_rccl_error, sizeof(g_rccl_error), "librccl.so.1 not found: %s", dlerror()); return; }
  }
  bool ok = true;
  auto sym = [&](const char* name) -> void* {
    void* p = dlsym(r.handle, name);
    if (!p) { ok = false; snprintf(g_rccl_error, sizeof(g_rccl_error), "librccl lacks %s", name); }
    return p;
  };
#define LBM_RCCL_SYM(field, name) r.field = reinterpret_cast<decltype(r.field)>(sym(name))
  LBM_RCCL_SYM(GetVersion, "ncclGetVersion");        LBM_RCCL_SYM(GetUniqueId, "ncclGetUniqueId");
  LBM_RCCL_SYM(CommInitRank, "ncclCommInitRank");    LBM_RCCL_SYM(CommInitAll, "ncclCommInitAll");
  LBM_RCCL_SYM(CommDestroy, "ncclCommDestroy");      LBM_RCCL_SYM(CommCount, "ncclCommCount");
  LBM_RCCL_SYM(CommUserRank, "ncclCommUserRank");    LBM_RCCL_SYM(GroupStart, "ncclGroupStart");
  LBM_RCCL_SYM(GroupEnd, "ncclGroupEnd");            LBM_RCCL_SYM(Send, "ncclSend");
  LBM_RCCL_SYM(Recv, "ncclRecv");                    LBM_RCCL_SYM(AllReduce, "ncclAllReduce");
  LBM_RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef LBM_RCCL_SYM
  if (!ok) { r.handle = nullptr; return; }
  Dl_info di;
  if (dladdr(reinterpret_cast<void*>(r.GetVersion), &di) && di.dli_fname) {
    char real[512];
    const char* shown = realpath(di.dli_fname, real) ? real : di.dli_fname;
    strncpy(r.path, shown, sizeof(r.path) - 1);
  }
}

// the bound RCCL, or nullptr with the reason in g_rccl_error
RcclApi* rccl() {
  std::call_once(g_rccl_once, rccl_bind);
  return g_rccl.handle ? &g_rccl : nullptr;
}

#define RCCL_OR_FAIL(ret)                                                       \
  RcclApi* rc_api_ = rccl();                                                    \
  if (!rc_api_) LBM_FAIL(ret, "RCCL is not available: %s", g_rccl_error)

// ---- owned device resources (lbm_own.h) -------------------------------------------------------------------------
// A member of one of these types is released with the struct that declares it; every release call of the file is here.
using lbm_own::Own;
template <class T> void free_device(T* p) { (void)hipFree(p); }
template <class T> void free_pinned(T* p) { (void)hipHostFree(p); }
void destroy_event(hipEvent_t e) { (void)hipEventDestroy(e); }
void destroy_stream(hipStream_t s) { (void)hipStreamDestroy(s); }
void destroy_graph(hipGraph_t g) { (void)hipGraphDestroy(g); }
void destroy_graph_exec(hipGraphExec_t g) { (void)hipGraphExecDestroy(g); }

// h takes what make(&raw) made, after releasing what it held (a failed make leaves it empty); returns make's verdict,
// for HIP_TRY or a message of the caller's own
template <class Handle, class Make>
hipError_t remake(Handle& h, Make make) {
  h.reset();
  decltype(h.get()) raw{};
  const hipError_t e = make(&raw);
  h.reset(raw);
  return e;
}
template <class T>
struct DeviceBuf : Own<T*, free_device<T>> {
  hipError_t alloc_bytes(size_t bytes) { return remake(*this, [&](T** p) { return hipMalloc(p, bytes); }); }
  hipError_t alloc(size_t count) { return alloc_bytes(count * sizeof(T)); }
};
template <class T>
struct PinnedBuf : Own<T*, free_pinned<T>> {
  hipError_t alloc(size_t count) { return remake(*this, [&](T** p) { return hipHostMalloc(p, count * sizeof(T)); }); }
};
struct Event : Own<hipEvent_t, destroy_event> {
  hipError_t create(unsigned flags) { return remake(*this, [&](hipEvent_t* e) { return hipEventCreateWithFlags(e, flags); }); }
};
struct Stream : Own<hipStream_t, destroy_stream> {
  hipError_t create() { return remake(*this, [](hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }); }
};
using Graph = Own<hipGraph_t, destroy_graph>;
using GraphExec = Own<hipGraphExec_t, destroy_graph_exec>;
// scope guards of the RCCL exchange: a stream capture that was begun is ended (and its graph dropped), an RCCL group that
// was opened is closed, on every way out; the success path takes them over with release() and ends them itself
void abandon_capture(hipStream_t st) {
  hipGraph_t g = nullptr;
  (void)hipStreamEndCapture(st, &g);
  Graph drop(g);
}
void close_group(const RcclApi* nc) { (void)nc->GroupEnd(); }
using OpenCapture = Own<hipStream_t, abandon_capture>;
using OpenGroup = Own<const RcclApi*, close_group>;

// What a slab owns, it declares: the members go in reverse order of declaration once ~Slab has run, so the streams come
// first (they go last, behind the events and buffers their work used) and the chunk graphs last (they go first).
struct Slab {
  int device = 0;
  int row_first = 0;  // global row of slab row 0
  int rows = 0;       // owned rows
  int accel_row = lbm::kNoRow;  // slab row (may be a halo row) holding global row ny-2
  int accel_row2 = lbm::kNoRow; // its second periodic image among the halo rows (a ring of ONE slab with 3-step passes)
  Stream compute_own, comm;
  hipStream_t compute = nullptr;  // the compute stream in use: compute_own, or (members 1.. of a batch, whose compute_own
                                  // is empty) member 0's, borrowed
  // band groups (single periodic slab, c->plan.band_groups > 1): interior bands of group g run on group_stream(g) -- the
  // compute stream for g = 0, group_extra[g - 1] after it -- and the seam bands on the comm stream
  Stream group_extra[kMaxBandGroups - 1];
  Event ev_boundary, ev_halo, ev_t0, ev_t1;
  Event ev_interior[2];               // interior kernel of step t -> [t & 1]
  Event ev_flush;                     // partials reduced: their slots may be reused
  Event ev_step;                      // stale-halo mode: whole-slab pass finished; graph replay: join
  Event ev_fork;                      // graph replay: the other streams join the capture / follow the chunks
  Event ev_x[2];                      // stale-halo mode: exchange for pass m landed -> [(m + 1) & 1]
  Event ev_gi[2][kMaxBandGroups];     // interior bands of group g in pass m done -> [m & 1][g]
  Event ev_gs[2];                     // seam bands of pass m done -> [m & 1]
  DeviceBuf<float> lat_alloc[2];      // (rows + 2*kHaloRows) x row_pitch each
  float* lat[2] = {nullptr, nullptr}; // row 0 of each lattice (= lat_alloc + kHaloRows rows)
  DeviceBuf<unsigned char> mask_alloc;  // (rows + 2*kMaskHalo) x pitch: neighbour rows below and above
  unsigned char* mask = nullptr;        // row 0 of the mask
  DeviceBuf<float> partials;     // kPartSlots x part_stride
  DeviceBuf<double> tot_u;       // capacity entries: per-step sum of |u| over this slab
  DeviceBuf<double> scratch;     // 2 x kSumBlocks doubles for lattice_sums
  DeviceBuf<double> reduce_buf;  // ranked contexts: capacity doubles for the av_vels all-reduce
  DeviceBuf<int> flushed_dev;    // graph replay: index of the first step of the chunk being reduced
  DeviceBuf<uint4> res_gran;               // resident kernel: seam granules {v, v, v, tag}: [2][bands][2][nx]
  DeviceBuf<float> res_part;               // resident kernel: per-band partial sums of a launch, [kResidentChunk][bands]
  DeviceBuf<int> res_status;               // resident kernel: 0, or the reason a workgroup gave up
  PinnedBuf<int> res_status_host;          // pinned copy of it, refreshed behind every launch (read by lbm_sync)
  DeviceBuf<float> frames;                 // lbm_set_frames: [frame slots][rows][nx] |u| of the owned rows
  DeviceBuf<lbm::probe_vec> probe_ring;    // lbm_set_probes: [rows of samples][probes]; a slab writes the probes in its rows
  DeviceBuf<lbm::ProbeEntry> probe_table;  // ... those, sorted by row (+ one word per band where the resident kernel runs)
  int probe_count = 0;                     // ... and how many they are
  DeviceBuf<double> mean_sums;             // lbm_set_mean: four planes [rows][nx]: sums of u_x, u_y, |u|, pressure of the owned rows;
                                           // lbm_set_mean_order(.., 2): eight, then u_x u_x, u_y u_y, u_x u_y, pressure pressure
  DeviceBuf<float> field_ring;             // lbm_set_field_frames: [slots][F][field_ny][window nx], this slab's rows of the window
  int field_y0 = 0, field_ny = 0;          // ... those rows: slab rows [field_y0, field_y0 + field_ny); none: no ring
  DeviceBuf<long long> gather_ring;        // the gather kinds (kGatherKinds): [slots][the kind's slot_words]: this slab's exact
                                           // sums (lbm_exact_sum.h) of a record, laid out as the kind's slot_words says
  DeviceBuf<unsigned> force_links;         // lbm_set_forces: the boundary links of the owned blocked cells, by body, cell, k ...
  DeviceBuf<unsigned> force_starts;        // ... [bodies + 1]: where each body's links start
  int force_groups = 0;                    // workgroups per body of force_gather (0: the slab has no links)
  DeviceBuf<float> residual_planes;        // lbm_set_residual: [2][rows][nx]: the remembered u_x and u_y of this slab's owned cells
  DeviceBuf<float> vort_edges;             // lbm_set_enstrophy, several slabs: [2][row_pitch]: the south and the north neighbour's
                                           // boundary row of the current lattice, copied in front of every vorticity_gather
  Event ev_vort_ready, ev_vort_done;       // ... this slab's rows may be copied / the copies of this slab's sample have been used
  DeviceBuf<long long> psi_totals;         // lbm_set_psi: [bands][nx][kExactLimbs]: the scan's band totals, then in place the bands' bases
  DeviceBuf<lbm::PsiCandidate> psi_cand;   // ... [bands][column groups]: the workgroups' extrema of a sample
  int psi_band_rows = 0;                   // ... rows of a band of this slab's scan
  DeviceBuf<long long> psi_in, psi_out;    // ... several slabs: [nx][kExactLimbs]: the limbs of every column below this slab (a copy of
                                           // the slab below's psi_out) and up to its last row
  Event ev_psi_out, ev_psi_taken;          // ... psi_out is written / the slab above has copied it
  DeviceBuf<lbm_tracer> tracer_state;      // lbm_set_tracers: [n]: the tracers' current positions, advanced in place at every sample
  // freshest-available mode (LBM_HALO_FRESHEST), allocated at its first use in this order: whole once ev_fresh[1] exists
  DeviceBuf<float> fresh_stage;          // [parity][side: 0 south halo, 1 north halo][row_pitch]: this pass's rows, if they make it
  DeviceBuf<unsigned> fresh_arrived;     // [parity][side]: id (global step + 1) of the step whose row the staging holds
  DeviceBuf<unsigned> fresh_id_src;      // [parity]: the id this slab ships behind its rows (device copies)
  DeviceBuf<int> fresh_decision;         // bit 0 / 1: south / north staging row adopted in the current pass
  DeviceBuf<unsigned char> fresh_log;    // [capacity]: the decision of every step (3 where the halos were fresh anyway)
  Event ev_fresh[2];                     // LBM_FRESH_FORCE=wait: this pass's rows and ids are out
  ncclComm_t nccl = nullptr;             // destroyed by ~Slab
  GraphExec chunk_graph[2];  // kPartSlots timesteps + their reduce, by lattice parity
  lbm::SlotCounts slot_counts;  // partials written into each buffered slot (launch geometries differ)
  int blocks_main = 0;      // interior rows (or all rows in HALO_SELF)
  int blocks_boundary = 0;  // rows 0 and rows-1 (halo modes)
  long fluid_cells = 0;     // non-blocked cells among the owned rows

  // the order-dependent part: graphs that captured RCCL operations hold on to the communicator, so they go first
  ~Slab() {
    if (!compute || hipSetDevice(device) != hipSuccess) return;  // never built: the compute stream is a slab's first resource
    for (GraphExec& g : chunk_graph) g.reset();
    if (nccl && g_rccl.CommDestroy) g_rccl.CommDestroy(nccl);
  }
};

constexpr int kSumBlocks = 1024;
constexpr int kResidentChunk = 4096;  // most timesteps one launch of the resident kernel advances
// the step_tile instantiation of every shape of lbm_plan::kTileDims, in both arithmetics
struct TileKernels { void (*exact)(const lbm::TileArgs); void (*fast)(const lbm::TileArgs); };
#define LBM_TILE_KERNELS(I)                                                                       \
  {lbm::step_tile<0, kTileDims[I].tw, kTileDims[I].th, kTileDims[I].kmax, kTileDims[I].threads>, \
   lbm::step_tile<1, kTileDims[I].tw, kTileDims[I].th, kTileDims[I].kmax, kTileDims[I].threads>}
const TileKernels kTileKernels[] = {LBM_TILE_KERNELS(0), LBM_TILE_KERNELS(1), LBM_TILE_KERNELS(2), LBM_TILE_KERNELS(3),
                                    LBM_TILE_KERNELS(4), LBM_TILE_KERNELS(5), LBM_TILE_KERNELS(6)};
static_assert(sizeof(kTileKernels) / sizeof(kTileKernels[0]) == lbm_plan::kTileShapeCount, "a kernel pair per tile shape");
static_assert(kMaskHalo == LBM_MASK_HALO_ROWS && kMaskHalo == kHaloRows - 1, "mask halo");

// where the obstacle flags come from (the reference: initialise() fills int[ny*nx] on rank 0 and, in the MPI variants,
// sends every rank its rows, MPI_Waitall/d2q9-bgk.c:794-842)
enum ObstacleKind { OBST_GLOBAL = 0, OBST_ROWS = 1, OBST_TILE = 2 };
struct ObstacleSource {
  int kind;
  const int* data;  // GLOBAL: int[ny*nx]; ROWS: this context's rows with kMaskHalo periodic neighbour rows each side;
                    // TILE: int[tile_ny*tile_nx], repeated periodically over the grid
  int tile_nx, tile_ny;
  bool local_cells;  // cells_aos holds only this context's rows (ROWS form)
};

// One host thread per slab for the issue loop of a one-process multi-GPU run: a pass enqueues
// ~10 runtime calls per slab, which a single thread issues at 25-30 us per slab -- more than an
// 8-GPU pass of 8192^2 takes on the devices.  The team runs the per-slab bodies of each phase
// concurrently (fork-join); phases stay ordered, so event records always precede the waits of the
// next phase.  Workers spin (yield) while a run is in flight and sleep on a condition variable
// between runs.  Single-slab contexts and the one-process-per-GPU form have no team.
struct SlabTeam {
  std::vector<std::thread> threads;
  std::function<int(int)> job;
  std::atomic<int> generation{0};
  std::atomic<int> pending{0};
  std::atomic<int> failed{0};
  std::atomic<bool> stop{false};
  std::atomic<bool> hot{false};
  std::mutex m;
  std::condition_variable cv;
  char error[kMaxSlabs][1024];

  void worker(int s) {
    int seen = 0;
    for (;;) {
      while (generation.load(std::memory_order_acquire) == seen && !stop.load(std::memory_order_acquire)) {
        if (hot.load(std::memory_order_acquire)) {
          std::this_thread::yield();
        } else {
          std::unique_lock<std::mutex> lk(m);
          cv.wait_for(lk, std::chrono::milliseconds(2));
        }
      }
      if (stop.load(std::memory_order_acquire)) return;
      seen = generation.load(std::memory_order_acquire);
      const int rc = job(s);
      if (rc != LBM_SUCCESS) {
        strncpy(error[s], g_last_error, sizeof(error[s]) - 1);
        failed.store(1, std::memory_order_release);
      }
      pending.fetch_sub(1, std::memory_order_release);
    }
  }
  void start(int n) {
    for (int s = 0; s < n; s++) {
      error[s][0] = 0;
      threads.emplace_back([this, s] { worker(s); });
    }
  }
  int run(int n, const std::function<int(int)>& f) {
    job = f;
    failed.store(0, std::memory_order_relaxed);
    pending.store(n, std::memory_order_release);
    generation.fetch_add(1, std::memory_order_release);
    if (!hot.load(std::memory_order_acquire)) cv.notify_all();
    while (pending.load(std::memory_order_acquire) > 0) std::this_thread::yield();
    if (failed.load(std::memory_order_acquire)) {
      for (int s = 0; s < n; s++)
        if (error[s][0]) {
          strncpy(g_last_error, error[s], sizeof(g_last_error) - 1);
          error[s][0] = 0;
          break;
        }
      return LBM_FAILURE;
    }
    return LBM_SUCCESS;
  }
  void shutdown() {
    stop.store(true, std::memory_order_release);
    cv.notify_all();
    for (auto& t : threads) t.join();
    threads.clear();
  }
};

}  // namespace

// A hipGraph chunk is BUILT, not captured: the issue code below runs against these virtual streams and events, which
// keep exactly the bookkeeping stream capture would (a stream's pending dependencies, an event's snapshot of them) and
// turn every launch / copy into an explicit node with explicit dependencies.  Multi-stream capture cannot be used:
// hip::Stream::EndCapture() of ROCm 7.2 recurses without end once three or more side streams have waited on each
// other's events (profiles/r03_graph_capture_defect.md, tools/capture_ring_repro.hip).
struct GraphBuilder {
  Graph graph;
  struct VStream { hipStream_t key; std::vector<hipGraphNode_t> last; };
  struct VEvent { hipEvent_t key; std::vector<hipGraphNode_t> nodes; };
  std::vector<VStream> streams;
  std::vector<VEvent> events;
  std::vector<hipGraphNode_t>& last_of(hipStream_t st) {
    for (auto& v : streams) if (v.key == st) return v.last;
    streams.push_back({st, {}});
    return streams.back().last;
  }
  std::vector<hipGraphNode_t>* snapshot_of(hipEvent_t ev, bool create) {
    for (auto& v : events) if (v.key == ev) return &v.nodes;
    if (!create) return nullptr;
    events.push_back({ev, {}});
    return &events.back().nodes;
  }
};

// One recorder per context: after global step tt with tt % every == 0 the running kernels store a record -- a frame
// (|u| of the owned rows, lbm_set_frames) or a row of probe samples (lbm_set_probes) -- into slot
// (tt / every - ord0) % slots of every slab's buffer of that kind.  The mean fields (lbm_set_mean) are the kind without
// slots: their record is added to per-cell sums, `written` counts the samples, `read`, `slots` and `ord0` stay unused.
// Field frames (lbm_set_field_frames) are slotted like the frames: chosen fields over a window instead of |u| everywhere.
// Obstacle forces (lbm_set_forces) are slotted like the probes: a row of per-body sums over the boundary links.  The one
// kind no kernel form records: every call runs as the sub-calls that end at its sample steps, each followed by force_gather.
// Lattice statistics (lbm_set_stats) are recorded the same way, by stats_gather: a row of whole-lattice sums.
// Velocity residuals (lbm_set_residual) likewise, by residual_gather, which also keeps a field between the samples: the
// velocities of the last sample (at first: of arming), which every sample compares with and replaces.
// Line profiles (lbm_set_profiles) likewise, by profile_rows and profile_columns: a record of per-row and per-column sums.
// The enstrophy (lbm_set_enstrophy) likewise, by vorticity_gather: a row of whole-lattice sums of the vorticity, the one
// kind whose kernel reads rows a slab does not own (Slab::vort_edges).
// The stream function (lbm_set_psi) likewise, by a scan of three sweeps and psi_extrema: a row of the extrema of psi, the
// one kind whose slabs depend on each other (Slab::psi_in, psi_out).
// Coarse frames (lbm_set_coarse_frames) likewise, by coarse_gather: a frame of per-box sums, rounded on the device except
// in the box rows that two slabs share.
// The stress (lbm_set_stress) likewise, by stress_gather: a row of whole-lattice sums of the second moment, pointwise.
// Tracer particles (lbm_set_tracers) likewise, by tracer_advance: a row of positions, the one kind whose state (the positions)
// persists between samples and whose ring may have no slots (capacity 0: the positions are read with lbm_tracers_now).
// These nine gather kinds share one ring of int64 words per slab, Slab::gather_ring; a batch arms them on itself
// (lbm_batch::rec) with one ring for all members.  What a gather kind is stands in one place, its entry of kGatherKinds.
enum { kRecNone = lbm::kRecNone, kRecFrames = lbm::kRecFrames, kRecProbes = lbm::kRecProbes, kRecMean = lbm::kRecMean,
       kRecFields = lbm::kRecFields, kRecForces = 5, kRecStats = 6, kRecResidual = 7, kRecProfiles = 8, kRecEnstrophy = 9,
       kRecPsi = 10, kRecCoarse = 11, kRecStress = 12, kRecTracers = 13, kRecKinds = 14, kRecGatherFirst = kRecForces };
// the kinds recorded by a gather launch behind the sub-call that ends at a sample step, whatever kernels advance the lattice
constexpr bool is_gather(int kind) { return kind >= kRecGatherFirst && kind < kRecKinds; }
// what a gather kind was armed with: the arguments of its setter that its slot's size, its launches and its reader depend on
struct GatherArgs {
  int bodies = 0;            // obstacle forces: bodies of the context, or of every member
  int axes = 0;              // line profiles: the LBM_PROFILE_* bits
  int box_x = 0, box_y = 0;  // coarse frames: the box's sides, cells
  int tracers = 0;           // tracer particles: tracers of the context, or of every member
  int base_steps = 0;        // steps_done at arming: the step of the residuals' baseline (the first row's span); the tracers' likewise
};
struct Recorder {
  int kind = kRecNone;
  int every = 0;
  int slots = 0;            // (0 while armed: a gather kind armed without a ring, GatherKind::ringless)
  int ord0 = 0;             // tt / every of the first record after arming
  long long written = 0;    // records issued since arming (ordinals 0 .. written - 1) ...
  long long read = 0;       // ... and drained by the kind's reader
  int order = 0;            // mean fields: 1 = the four sums, 2 = also the four sums of products (lbm_set_mean_order)
  int fields = 0;           // field frames: the LBM_FIELD_* bits ...
  lbm_window window = {0, 0, 0, 0};  // ... and the window, global cells
  GatherArgs args;          // a gather kind: what it was armed with
};
// what differs between the kinds in the host's messages (kRecNone keeps the empty defaults)
struct RecorderKind {
  const char* name = "";    // "<name> are armed"
  const char* noun = "";    // the short name
  const char* record = "";  // one record: "<record>s are waiting"
  const char* setter = "";
  const char* reader = "";
  const char* disarm = "";  // the call that disarms
  bool slotted = true;      // records wait in `slots` slots until read (false: they are accumulated, no call lacks room)
};
// the kinds the running kernels record themselves; the gather kinds' words stand in kGatherKinds (kind_words finds either)
constexpr RecorderKind kRecorderKinds[kRecGatherFirst] = {
    {},
    {.name = "animation frames", .noun = "frames", .record = "frame", .setter = "lbm_set_frames",
     .reader = "lbm_read_frames", .disarm = "lbm_set_frames(ctx, 0, 0)"},
    {.name = "point probes", .noun = "probes", .record = "sample", .setter = "lbm_set_probes",
     .reader = "lbm_read_probes", .disarm = "lbm_set_probes(ctx, 0, NULL, 0, 0)"},
    {.name = "mean fields", .noun = "mean fields", .record = "sample", .setter = "lbm_set_mean",
     .reader = "lbm_read_mean", .disarm = "lbm_set_mean(ctx, 0)", .slotted = false},
    {.name = "field frames", .noun = "field frames", .record = "field frame", .setter = "lbm_set_field_frames",
     .reader = "lbm_read_field_frames", .disarm = "lbm_set_field_frames(ctx, 0, 0, 0, NULL)"}};

// Whose records a reader converts: the slabs of a context (one lattice, `shares` slabs), or the members of a batch (each a
// lattice of one slab that starts at row 0).  The fetched words are [record][lattice][share][the share's slot]
struct GatherOwner {
  int nx = 0, ny = 0;
  size_t lattices = 1;          // per record
  int shares = 1;               // slabs per lattice
  int row_first[kMaxSlabs] = {0}, row_count[kMaxSlabs] = {0};
  size_t lattice_words = 0;     // ... and one lattice's shares are this many words
};
// A hook that allocates answers LBM_SUCCESS, LBM_FAILURE (it has said why) or kNoRoom: the driver then says that the ring
// and `also` could not be allocated.
constexpr int kNoRoom = 2;
// One gather kind: everything that differs between the nine, for a context and for a batch.  The drivers (arm_gather,
// arm_batch_gather, drain_gather, drain_batch_gather, take_record, lbm_batch_run) know no kind.
struct GatherKind {
  RecorderKind ctx;          // the words of a context's messages ...
  const char* batch_setter;  // ... and those of a batch's that differ
  const char* batch_reader;
  const char* batch_disarm;
  const char* stays_off;     // "cannot allocate ...; <stays_off>"
  const char* spread;        // multi-process contexts: "<spread> would be spread over the ranks"
  const char* of_a_batch;    // members: "so <of_a_batch> armed on the batch"
  const char* of = "";       // "cannot allocate 4 rows<of> ...", a format of args.bodies
  const char* also = "";     // "... (1.0 MiB per slab)<also>": what the kind's hook allocates besides, where kNoRoom tells of it
  bool per_slab = false;     // the slot's size depends on the slab: the messages name the slab
  bool ringless = false;     // capacity 0 arms the kind without a ring: its records go nowhere, no call lacks room, its reader refuses
  // int64 words of one slab's (or member's) slot
  size_t (*slot_words)(const lbm_ctx* c, const Slab& sl, const GatherArgs& a);
  // refuses the kind's own arguments, or nothing (nullptr); members: of the batch that arms, 0: a context does
  int (*check)(const char* who, const lbm_ctx* c, size_t members, int capacity, const GatherArgs& a) = nullptr;
  // the kind's buffers besides the ring, or none (nullptr): of slab s behind its ring, and of a batch behind its ring;
  // own: what the kind's setter hands to its hook
  int (*alloc_slab)(const char* who, lbm_ctx* c, int s, const GatherArgs& a, const void* own) = nullptr;
  int (*alloc_batch)(const char* who, lbm_batch* bt, const GatherArgs& a, const void* own) = nullptr;
  // one record of a context: every slab's share into its zeroed slot (take_per_slab: launch(c, s, slot) on every slab's
  // compute stream, side by side) ...
  int (*take)(lbm_ctx* c);
  int (*launch)(lbm_ctx* c, int s, long long* words) = nullptr;
  // ... and of a batch: all members' into `slot`, zeroed, on the batch's stream
  int (*take_batch)(lbm_batch* bt, long long* slot);
  // the words of the n oldest records, fetched, into the caller's rows (r.read: the ordinal of the first)
  void (*rows)(const GatherOwner& g, const Recorder& r, int n, const long long* words, void* out);
};
namespace {
const GatherKind& gather_kind(int kind);     // kGatherKinds[kind - kRecGatherFirst]
const RecorderKind& kind_words(int kind);    // of any kind, as a context speaks of it
}

struct lbm_ctx {
  lbm_params p;
  int pitch = 0;
  long plane_stride = 0;  // floats between the 9 planes of one row (= pitch + optional pad)
  long row_pitch = 0;     // floats between lattice rows (= 9 * plane_stride)
  int n_slabs = 0;
  Slab slab[kMaxSlabs];
  int cur = 0;  // lattice holding the current state
  int steps_done = 0;
  int capacity = 0;  // entries in tot_u
  int fluid_cells = 0;
  int math_mode = LBM_MATH_EXACT;
  int halo = HALO_SELF;
  int halo_mode = LBM_HALO_SYNC;  // LBM_HALO_STALE: passes consume the halos of the previous pass
  int rank = 0, world = 1;  // multi-process
  bool ranked = false;      // created by lbm_create_rank* (one process per GPU: rank / world describe the ring)
  bool hosted = false;      // ... with the host's own message passing instead of RCCL (lbm_create_rank_hosted)
  lbm_host_comm host_comm = {nullptr, nullptr, nullptr};
  PinnedBuf<float> host_send[2], host_recv[2];  // pinned staging buffers of the hosted exchange: kHaloRows rows each
  int row_first = 0, row_count = 0;
  int slot_fill = 0;  // partial slots used since the last reduce
  KernelPlan plan;    // which kernels advance this context and their launch geometry (lbm_plan.h: plan_kernels)
  bool groups_forked = false;       // band groups: the group and seam streams have been forked off the compute stream
  SlabTeam* team = nullptr;         // one issuing thread per slab (one-process multi-GPU), or null
  GraphBuilder* builder = nullptr;  // non-null while a chunk is being built: launches become graph nodes
  bool resident_used = false;       // a resident launch is in flight / unchecked: lbm_sync reads its status
  bool failed = false;              // a resident launch of this context gave up: failed until destroyed (a member: see lbm_batch::failed)
  lbm_batch* batch = nullptr;       // member of this batch (lbm_create_batch): advanced, synchronised and freed by it
  Recorder rec;                     // the one recorder: animation frames (lbm_set_frames), point probes (lbm_set_probes) or
                                    // mean fields (lbm_set_mean) or field frames (lbm_set_field_frames)
  std::vector<lbm_probe> probe_cells;  // the probed global cells, in the caller's order (a probes row has that many samples)
  std::vector<int> force_link_counts;  // lbm_set_forces: boundary links of each body, all slabs (a forces row has that many bodies)
  // checked runs (checked_run: lbm_run_until, lbm_run_until_residual), allocated by the first one in this order (steady_buffers):
  // whole once ev_steady[1] exists
  DeviceBuf<lbm::SteadyState> steady_state;  // device: the stop word of the current call (and what the average-velocity checks have found)
  PinnedBuf<int> steady_stop_host;  // pinned: the stop word after segment j, in slot j & 1 ...
  Event ev_steady[2];               // ... behind these events
  // the residual criterion's own set, allocated by the first lbm_run_until_residual and kept (until_state last: whole once
  // it exists).  The planes are the call's own: the recorder never sees them.
  DeviceBuf<float> until_planes;                    // device: [2][rows][nx]: the remembered u_x and u_y of slab 0
  DeviceBuf<long long> until_words;                 // device: [lbm_residual::kResidualWords]: the sample of the current segment
  DeviceBuf<lbm_residual::UntilState> until_state;  // device: what the checks of the current call have found
  DeviceBuf<long long> until_history;               // device: [until_history_rows][kResidualWords]: the words of the first checks
  size_t until_history_rows = 0;                    // (until_history_begin: kept from call to call while they suffice)
  int psi_band_env = -1;  // LBM_PSI_BAND_ROWS, read once at the context's first scan (psi_band_rows): 0: not set
};

// B independent single-slab lattices of one shape on one device, advanced together (lbm_create_batch).  The members
// are ordinary contexts that share ONE stream (member 0's compute stream), so every read through a member is ordered
// behind every batched launch.  Resident shapes run each chunk of up to kResidentChunk timesteps as launches of
// lbm::resident_band<..., BATCH = true>, members_per_launch members each, one after the other on that stream.
struct lbm_batch {
  std::vector<lbm_ctx*> members;
  hipStream_t stream = nullptr;      // member 0's compute stream, borrowed
  int resident = 0;                 // the members are resident-eligible: long calls run batched
  int member_wgs = 0;               // working workgroups of one member
  int members_per_launch = 1;       // co-resident members in one launch: 8 one-XCD members, else floor(CUs / member_wgs)
  int launches = 0;                 // launches per chunk (sub-batches)
  int cur = 0;                      // lattice of every member holding the current state
  int steps_done = 0;
  DeviceBuf<lbm::ResidentMember> table;  // device: [parity of cur][members]
  DeviceBuf<int> status;            // device: 0, or kResidentTimeout once a workgroup of any batched launch gave up
  PinnedBuf<int> status_host;       // pinned copy behind every run; every member's lbm_sync reports it
  bool failed = false;              // a batched launch gave up: the batch and all its members are failed until it is destroyed
  DeviceBuf<lbm::ResidentFrames> frame_table;  // device: [members], allocated when the first member arms frames
  DeviceBuf<lbm::ResidentProbes> probe_table;  // device: [members], allocated when the first member arms probes
  DeviceBuf<lbm::ResidentMean> mean_table;     // device: [members], allocated when the first member arms the mean fields
  DeviceBuf<lbm::ResidentFields> field_table;  // device: [members], allocated when the first member arms field frames
  int armed[kRecKinds] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // members with a recorder of each kind armed: batched launches run that kind's kernel
                                    // (a batch records one kind, so at most one count is non-zero; a gather kind is armed
                                    // on the batch, by its lbm_batch_set_*, and counts as one)
  // the gather kinds (kGatherKinds) of all members: the members' own recorders stay off, the batch keeps the one
  // recorder and the one ring (arm_batch_gather, drain_batch_gather, release_batch_recorder); every lbm_batch_run
  // runs as the sub-calls that end at its sample steps
  Recorder rec;                                  // a gather kind while armed
  DeviceBuf<long long> gather_ring;              // device: [slots][members][the kind's slot_words of a member]
  DeviceBuf<float> residual_planes;              // lbm_batch_set_residual: device: [members][2][rows][nx]: the members' remembered u_x and u_y
  DeviceBuf<lbm_tracer> tracer_state;            // lbm_batch_set_tracers: device: [members][n]: the members' tracers' current positions
  DeviceBuf<long long> psi_totals;               // lbm_batch_set_psi: device: [members][bands][nx][kExactLimbs]: the scan's totals, then bases
  DeviceBuf<lbm::PsiCandidate> psi_cand;         // ... [members][bands][column groups]
  int psi_band_rows = 0;                         // ... rows of a band of every member's scan
  int force_groups = 0;                          // lbm_batch_set_forces: workgroups per (member, body) of force_gather_batch (0: no member has a link)
  std::vector<int> force_link_counts;            // [members][bodies]
  std::vector<DeviceBuf<unsigned>> force_links;  // [members]: the member's boundary links, by body, cell, k ...
  std::vector<DeviceBuf<unsigned>> force_starts; // ... and [bodies + 1]: where each body's links start
  DeviceBuf<lbm::ForceMember> force_lists;       // device: [members], those pointers
  // checked runs (checked_batch_run: lbm_batch_run_until, lbm_batch_run_until_residual), allocated by the first one in
  // this order (steady_batch_buffers): whole once ev_steady exists
  DeviceBuf<lbm::SteadyBatch> steady_batch;  // device: the count of finished members and all_steady, the stop word
  PinnedBuf<int> steady_stop_host;  // pinned: all_steady after the last segment ...
  Event ev_steady;                  // ... behind this event
  // the average-velocity criterion's own set (lbm_batch_run_until); steady_state last: whole once it exists
  DeviceBuf<lbm::SteadyMember> steady_members;  // device: [members]
  DeviceBuf<lbm::SteadyState> steady_state;     // device: [members]
  // the residual criterion's own set (lbm_batch_run_until_residual), kept; until_state last: whole once it exists
  DeviceBuf<float> until_planes;                    // device: [members][2][rows][nx]
  DeviceBuf<long long> until_words;                 // device: [members][lbm_residual::kResidualWords]
  DeviceBuf<lbm_residual::UntilState> until_state;  // device: [members]
  DeviceBuf<long long> until_history;               // device: [until_history_rows][members][kResidualWords]
  size_t until_history_rows = 0;
};

namespace {

// ---- a resident give-up fails its owner for good ---------------------------------------------------------------------
// The owner of a lattice is its context, or for a batch member the batch: one give-up in any batched launch fails the
// batch and every member.  The flag is set where a non-zero status word is first seen (gave_up) and never cleared; every
// entry point but lbm_destroy, lbm_destroy_batch, lbm_get_info, lbm_batch_get_info, lbm_batch_member and lbm_rccl_info
// refuses a failed owner directly behind its NULL checks (REFUSE_FAILED), before any other check and any device work.
const char kFailedOwner[] = "%s: an earlier launch of the resident kernel gave up: the lattice and the records of this context or "
                            "batch are invalid, and it stays failed until it is destroyed";
bool owner_failed(const lbm_ctx* c) { return c->batch ? c->batch->failed : c->failed; }
bool owner_failed(const lbm_batch* bt) { return bt->failed; }
#define REFUSE_FAILED(ret, owner, who)                              \
  do {                                                              \
    if (owner_failed(owner)) LBM_FAIL(ret, kFailedOwner, who);      \
  } while (0)

// the status word that the resident launches of c (a member: of its batch) left on the host; non-zero fails the owner.
// The caller has waited for the copy behind those launches.
int gave_up(lbm_ctx* c) {
  const int status = c->batch ? *c->batch->status_host : *c->slab[0].res_status_host;
  if (status != 0) (c->batch ? c->batch->failed : c->failed) = true;
  return status;
}
// the first report of a give-up
int report_give_up(const lbm_ctx* c, int status) {
  LBM_FAIL(LBM_FAILURE, "the resident kernel gave up waiting for a neighbouring band after %.0f ms (status %d): its %d workgroups "
           "were not all running at once -- is another process using the device?  The lattice of this context is no "
           "longer valid; LBM_RESIDENT=0 selects the launch-per-pass kernels, LBM_RESIDENT_TIMEOUT_MS moves the bound",
           (double)c->plan.resident_timeout / 1e5, status, c->plan.resident_bands);
}

// the acceleration weights of the lid row (SerialCode/d2q9-bgk.c:219-220), and the a1 / a2 fields of a kernel's arguments
struct AccelWeights { float a1, a2; };
AccelWeights accel_weights(const lbm_params& p) { return {p.density * p.accel / 9.f, p.density * p.accel / 36.f}; }
template <class Args>
void set_accel_weights(Args& a, const lbm_params& p) {
  const AccelWeights w = accel_weights(p);
  a.a1 = w.a1;
  a.a2 = w.a2;
}

// run body(s) for every slab: concurrently on the slab team when there is one, else in order
int for_slabs(lbm_ctx* c, const std::function<int(int)>& body) {
  if (c->team) return c->team->run(c->n_slabs, body);
  for (int s = 0; s < c->n_slabs; s++)
    if (body(s) != LBM_SUCCESS) return LBM_FAILURE;
  return LBM_SUCCESS;
}

// ---- stream operations that become graph nodes / edges while a chunk is being built ---------------------------
int q_wait(lbm_ctx* c, hipStream_t st, hipEvent_t ev) {
  if (!c->builder) { HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(st, ev, 0)); return LBM_SUCCESS; }
  const std::vector<hipGraphNode_t>* snap = c->builder->snapshot_of(ev, false);
  if (!snap) return LBM_SUCCESS;  // never recorded inside this chunk: "ready when the chunk starts"
  std::vector<hipGraphNode_t>& last = c->builder->last_of(st);
  for (hipGraphNode_t n : *snap) {
    bool have = false;
    for (hipGraphNode_t m : last) have = have || (m == n);
    if (!have) last.push_back(n);
  }
  return LBM_SUCCESS;
}
int q_record(lbm_ctx* c, hipEvent_t ev, hipStream_t st) {
  if (!c->builder) { HIP_TRY(LBM_FAILURE, hipEventRecord(ev, st)); return LBM_SUCCESS; }
  const std::vector<hipGraphNode_t> now = c->builder->last_of(st);  // copy: snapshot_of may grow the event table
  *c->builder->snapshot_of(ev, true) = now;
  return LBM_SUCCESS;
}
// launch fn(args...) on st; `done` (optional, stream mode): event bound to the kernel's own completion signal
int q_kernel(lbm_ctx* c, hipStream_t st, const void* fn, dim3 grid, dim3 block, void** args, hipEvent_t done = nullptr) {
  if (c->builder) {
    hipKernelNodeParams kp;
    memset(&kp, 0, sizeof(kp));
    kp.func = const_cast<void*>(fn);
    kp.gridDim = grid;
    kp.blockDim = block;
    kp.kernelParams = args;
    std::vector<hipGraphNode_t>& last = c->builder->last_of(st);
    hipGraphNode_t node = nullptr;
    HIP_TRY(LBM_FAILURE, hipGraphAddKernelNode(&node, c->builder->graph, last.data(), last.size(), &kp));
    last.assign(1, node);
    if (done) *c->builder->snapshot_of(done, true) = last;
    return LBM_SUCCESS;
  }
  if (done) HIP_TRY(LBM_FAILURE, hipExtLaunchKernel(fn, grid, block, args, 0, st, nullptr, done, 0));
  else HIP_TRY(LBM_FAILURE, hipLaunchKernel(fn, grid, block, args, 0, st));
  return LBM_SUCCESS;
}
int q_copy(lbm_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t st) {
  if (!c->builder) { HIP_TRY(LBM_FAILURE, hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, st)); return LBM_SUCCESS; }
  std::vector<hipGraphNode_t>& last = c->builder->last_of(st);
  hipGraphNode_t node = nullptr;
  HIP_TRY(LBM_FAILURE, hipGraphAddMemcpyNode1D(&node, c->builder->graph, last.data(), last.size(), dst, src, bytes, hipMemcpyDeviceToDevice));
  last.assign(1, node);
  return LBM_SUCCESS;
}

// ---- launch helpers --------------------------------------------------------------------------
// where a slab's lattices lie, as every kernel is told: the view that reads lattice `from` and writes lattice `to`
// (from == to for the kernels that work in place), by default the current lattice into the other one
lbm::LatticeArgs lattice_args(const lbm_ctx* c, const Slab& sl, int from, int to) {
  return {sl.lat[from], sl.lat[to], sl.mask, c->plane_stride, c->row_pitch, c->pitch, c->p.nx};
}
lbm::LatticeArgs lattice_args(const lbm_ctx* c, const Slab& sl) { return lattice_args(c, sl, c->cur, c->cur ^ 1); }

// `done` (optional): event bound to the kernel's own completion signal (hipExtLaunchKernel's stop event)
// -- what hipEventRecord right after the launch would mark, without a barrier packet of its own
int launch_step(lbm_ctx* c, int s, hipStream_t stream, int row_first, int row_stride, int n_rows,
                int part_offset, bool accel_epilogue, hipEvent_t done = nullptr) {
  Slab& sl = c->slab[s];
  if (n_rows <= 0) return LBM_SUCCESS;
  lbm::StepArgs a;
  static_cast<lbm::LatticeArgs&>(a) = lattice_args(c, sl);
  a.rows = sl.rows;
  a.row_first = row_first;
  a.row_stride = row_stride;
  a.n_rows = n_rows;
  a.accel_row = accel_epilogue ? sl.accel_row : lbm::kNoRow;
  a.omega = c->p.omega;
  set_accel_weights(a, c->p);
  a.partials = sl.partials + (long)c->slot_fill * c->plan.part_stride + part_offset;
  a.reverse = (c->plan.snake && n_rows > 2) ? (c->cur & 1) : 0;
  a.wrap = (c->halo == HALO_SELF) ? 1 : 0;

  const bool exact = (c->math_mode == LBM_MATH_EXACT);
  if (c->plan.vec4) {
    const int blocks = ceil_div((long)(c->p.nx / 4) * n_rows, lbm::kBlock);
    // kernel flavour: [math][neighbour exchange][nontemporal stores]; tuned defaults, see DESIGN.md
    typedef void (*step_fn)(const lbm::StepArgs);
    static const step_fn table[2][3][2] = {
        {{lbm::step_vec4<0, 0, false>, lbm::step_vec4<0, 0, true>},
         {lbm::step_vec4<0, 1, false>, lbm::step_vec4<0, 1, true>},
         {lbm::step_vec4<0, 2, false>, lbm::step_vec4<0, 2, true>}},
        {{lbm::step_vec4<1, 0, false>, lbm::step_vec4<1, 0, true>},
         {lbm::step_vec4<1, 1, false>, lbm::step_vec4<1, 1, true>},
         {lbm::step_vec4<1, 2, false>, lbm::step_vec4<1, 2, true>}}};
    void* args[] = {&a};
    return q_kernel(c, stream, reinterpret_cast<const void*>(table[exact ? 0 : 1][c->plan.neigh][c->plan.nts]), dim3(blocks), dim3(lbm::kBlock), args, done);
  } else {
    const int blocks = ceil_div((long)c->p.nx * n_rows, lbm::kBlock);
    const auto fn = exact ? lbm::step_scalar<true> : lbm::step_scalar<false>;
    void* args[] = {&a};
    return q_kernel(c, stream, reinterpret_cast<const void*>(fn), dim3(blocks), dim3(lbm::kBlock), args, done);
  }
}

// two timesteps in one pass over the rows [row_first, row_end) of slab s, cut into band_count bands of
// band_rows rows that start band_pitch rows apart; writes the partials of steps t and t+1 into
// slots slot_fill and slot_fill+1
int launch_step2(lbm_ctx* c, int s, hipStream_t stream, const lbm_plan::StreamRow& row, int row_first, int row_end, int band_rows,
                 int band_pitch, int band_count, int part_offset, bool accel_after, hipEvent_t done = nullptr) {
  Slab& sl = c->slab[s];
  if (band_count <= 0) return LBM_SUCCESS;
  lbm::Step2Args a;
  static_cast<lbm::LatticeArgs&>(a) = lattice_args(c, sl);
  a.rows = sl.rows;
  a.wrap = (c->halo == HALO_SELF) ? 1 : 0;
  a.band_rows = band_rows;
  a.row_first = row_first;
  a.band_pitch = band_pitch;
  a.row_end = row_end;
  a.n_strips = c->plan.n_strips;
  a.accel_row = sl.accel_row;
  a.accel_after = accel_after ? 1 : 0;
  a.omega = c->p.omega;
  set_accel_weights(a, c->p);
  a.partials1 = sl.partials + (long)c->slot_fill * c->plan.part_stride + part_offset;
  a.partials2 = a.partials1 + c->plan.part_stride;
  const int waves = c->plan.n_strips * band_count;
  typedef void (*fn)(const lbm::Step2Args);
  // [math][nontemporal stores][cells per lane: 0 -> 4, 1 -> 2]
  static const fn table[2][2][2] = {
      {{lbm::step2_stream<0, false, 4>, lbm::step2_stream<0, false, 2>},
       {lbm::step2_stream<0, true, 4>, lbm::step2_stream<0, true, 2>}},
      {{lbm::step2_stream<1, false, 4>, lbm::step2_stream<1, false, 2>},
       {lbm::step2_stream<1, true, 4>, lbm::step2_stream<1, true, 2>}}};
  const fn kernel = table[row.math][row.nts][row.lane_cells == 2 ? 1 : 0];
  void* args[] = {&a};
  return q_kernel(c, stream, reinterpret_cast<const void*>(kernel), dim3(waves), dim3(64), args, done);
}

// row.k (2..4) timesteps in one pass over the rows [row_first, row_end) of slab s (4 cells per lane), cut into band_count
// bands of band_rows rows that start band_pitch rows apart; partials of step t+j go to slot slot_fill + j
int launch_stepk(lbm_ctx* c, int s, hipStream_t stream, const lbm_plan::StreamRow& row, int row_first, int row_end, int band_rows,
                 int band_pitch, int band_count, int part_offset, bool accel_after, hipEvent_t done = nullptr) {
  Slab& sl = c->slab[s];
  if (band_count <= 0) return LBM_SUCCESS;
  lbm::StepKArgs a;
  static_cast<lbm::LatticeArgs&>(a) = lattice_args(c, sl);
  a.rows = sl.rows;
  a.wrap = (c->halo == HALO_SELF) ? 1 : 0;
  a.band_rows = band_rows;
  a.row_first = row_first;
  a.band_pitch = band_pitch;
  a.row_end = row_end;
  a.n_strips = c->plan.n_strips;
  a.n_bands = band_count;
  a.chunk = c->plan.xcd_chunk;
  a.halo_lanes = c->plan.halo_lanes;
  a.accel_row = sl.accel_row;
  a.accel_row2 = sl.accel_row2;
  a.accel_after = accel_after ? 1 : 0;
  a.omega = c->p.omega;
  set_accel_weights(a, c->p);
  a.partials = sl.partials + (long)c->slot_fill * c->plan.part_stride + part_offset;
  a.slot_stride = c->plan.part_stride;
  int waves = c->plan.n_strips * band_count;
  if (a.chunk > 0) {
    const int chunks = band_count * ceil_div(c->plan.n_strips, a.chunk);
    waves = 8 * ceil_div(chunks, 8) * a.chunk;
  }
  typedef void (*fn)(const lbm::StepKArgs);
  // [math][nontemporal stores][k - 2][prefetch]
  // (K = 4 with the next row prefetched does not fit the register file -- 112 bytes of scratch per lane -- so that
  // request runs the kernel without prefetch: same results)
#define LBM_K_ROW(M, N) {{lbm::stepk_stream<M, N, 4, 2, false>, lbm::stepk_stream<M, N, 4, 2, true>}, \
                         {lbm::stepk_stream<M, N, 4, 3, false>, lbm::stepk_stream<M, N, 4, 3, true>}, \
                         {lbm::stepk_stream<M, N, 4, 4, false>, lbm::stepk_stream<M, N, 4, 4, false>}}
  static const fn table[2][2][3][2] = {{LBM_K_ROW(0, false), LBM_K_ROW(0, true)}, {LBM_K_ROW(1, false), LBM_K_ROW(1, true)}};
#undef LBM_K_ROW
  // exact arithmetic on pairs of cells (v_pk_* instructions): [nontemporal stores][k - 2][prefetch][windows in LDS]
  // (K = 4 prefetches only with two of its three windows in LDS: with fewer it spills, and runs without prefetch)
#define LBM_PK(N, KK, PF) {lbm::stepk_pk<N, KK, (PF && KK < 4), 0>, lbm::stepk_pk<N, KK, (PF && KK < 4), 1>, lbm::stepk_pk<N, KK, PF, (KK > 2 ? 2 : 1)>}
#define LBM_PK_ROW(N) {{LBM_PK(N, 2, false), LBM_PK(N, 2, true)}, {LBM_PK(N, 3, false), LBM_PK(N, 3, true)}, \
                       {LBM_PK(N, 4, false), LBM_PK(N, 4, true)}}
  // [nontemporal stores][k - 2][prefetch][windows in LDS]  (the QUAD form of stepk_pk -- both pairs of a lane in one
  // basic block -- measured the same speed with more registers and is not instantiated: profiles/r02_tuning.md)
  static const fn table_pk[2][3][2][3] = {LBM_PK_ROW(false), LBM_PK_ROW(true)};
#undef LBM_PK_ROW
#undef LBM_PK
  // two cells per lane (one pair): [nontemporal stores][k - 2][prefetch][windows in LDS: 0, 1]
#define LBM_PK1(N, KK, PF) {lbm::stepk_pk<N, KK, (PF && KK < 4), 0, false, 1>, lbm::stepk_pk<N, KK, PF, 1, false, 1>}
#define LBM_PK1_ROW(N) {{LBM_PK1(N, 2, false), LBM_PK1(N, 2, true)}, {LBM_PK1(N, 3, false), LBM_PK1(N, 3, true)}, \
                        {LBM_PK1(N, 4, false), LBM_PK1(N, 4, true)}}
  static const fn table_pk1[2][3][2][2] = {LBM_PK1_ROW(false), LBM_PK1_ROW(true)};
#undef LBM_PK1_ROW
#undef LBM_PK1
  // the packed kernels have one arithmetic (the exact one) and serve both math modes; lbm_plan::stream_row has folded
  // the requests without a kernel of their own onto the entries that run instead
  const fn kernel = row.family == lbm_plan::ROW_STEPK_PK1 ? table_pk1[row.nts][row.k - 2][row.prefetch][row.lds]
                    : row.family == lbm_plan::ROW_STEPK_PK ? table_pk[row.nts][row.k - 2][row.prefetch][row.lds]
                                                           : table[row.math][row.nts][row.k - 2][row.prefetch];
  void* args[] = {&a};
  return q_kernel(c, stream, reinterpret_cast<const void*>(kernel), dim3(waves), dim3(64), args, done);
}

// the stream kernel for a k-step pass: which instantiation runs is the planner's arithmetic (lbm_plan::stream_row)
int launch_pass(lbm_ctx* c, int s, hipStream_t stream, int k, int row_first, int row_end, int band_rows,
                int band_pitch, int band_count, int part_offset, bool accel_after, hipEvent_t done = nullptr) {
  const lbm_plan::StreamRow row = lbm_plan::stream_row(c->plan, k, c->math_mode == LBM_MATH_EXACT);
  if (row.family != lbm_plan::ROW_STEP2_STREAM)
    return launch_stepk(c, s, stream, row, row_first, row_end, band_rows, band_pitch, band_count, part_offset, accel_after, done);
  return launch_step2(c, s, stream, row, row_first, row_end, band_rows, band_pitch, band_count, part_offset, accel_after, done);
}

int tile_count(const lbm_ctx* c) { return lbm_plan::tile_count(c->p.nx, c->slab[0].rows, c->plan.tile_shape); }

// n_steps <= c->plan.tile_steps timesteps of the whole (single, periodic) slab from LDS tiles; partials of step j go
// to slot slot_fill + j
int launch_tile(lbm_ctx* c, hipStream_t stream, int n_steps, bool accel_after) {
  Slab& sl = c->slab[0];
  lbm::TileArgs a;
  static_cast<lbm::LatticeArgs&>(a) = lattice_args(c, sl);
  a.ny = sl.rows;
  a.n_steps = n_steps;
  a.accel_row = sl.accel_row;
  a.accel_after = accel_after ? 1 : 0;
  a.omega = c->p.omega;
  set_accel_weights(a, c->p);
  a.partials = sl.partials + (long)c->slot_fill * c->plan.part_stride;
  a.slot_stride = c->plan.part_stride;
  const lbm_plan::TileDims& t = kTileDims[c->plan.tile_shape];
  const TileKernels& kernels = kTileKernels[c->plan.tile_shape];
  a.tiles_x = ceil_div(c->p.nx, t.tw);
  void* args[] = {&a};
  return q_kernel(c, stream, reinterpret_cast<const void*>(c->math_mode == LBM_MATH_EXACT ? kernels.exact : kernels.fast),
                  dim3(tile_count(c)), dim3(t.threads), args);
}

int blocks_for_rows(const lbm_ctx* c, int n_rows) { return lbm_plan::blocks_for_rows(c->plan.vec4, c->p.nx, n_rows); }

// One halo exchange, enqueued on the comm streams: the `depth` boundary rows at each end of every
// slab's lattice `src` travel, whole (all 9 speeds, as MPI_Waitall/d2q9-bgk.c:225-230 ships
// them), into the halo rows of its ring neighbours' lattices `dst` -- zero copy on both sides,
// because halo rows and boundary rows are contiguous in the row-interleaved layout.
//   my rows [rows-depth, rows)  ->  north neighbour's rows [-depth, 0)
//   my rows [0, depth)          ->  south neighbour's rows [rows_s, rows_s + depth)
// north neighbour of slab s = s+1 (periodic), south = s-1; across processes the ring runs over
// ranks (MPI/d2q9-bgk.c:210-211).
// Synchronous pipeline (slot < 0): src == dst == the current lattice.  Precondition (stream order):
// the kernels that wrote the boundary rows are ordered before this on the comm stream.
// Stale-halo pipeline (slot 0/1): src = the lattice just produced, dst = the lattice the pass after
// next reads.  The comm stream first waits for ev_step of this slab (boundary rows written) and, where
// this slab writes into its neighbours' memory itself (memcpy), of the neighbours (they have finished
// reading the halo rows about to be overwritten); ev_x[slot] marks the arrival.
int exchange_halos(lbm_ctx* c, int depth, int src, int dst, int slot) {
  const long n = (long)depth * c->row_pitch;
  const bool stale = (slot >= 0);
  if (c->halo == HALO_RCCL) {
    if (stale) {
      for (int s = 0; s < c->n_slabs; s++) {
        Slab& sl = c->slab[s];
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        // a peer's receive is posted behind the peer's own ev_step wait, so nothing lands in halo
        // rows a running pass still reads
        HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.comm, sl.ev_step, 0));
      }
    }
    // one thread driving several communicators must group them; with one thread per slab each
    // thread groups its own four operations.  The guards (OpenGroup, OpenCapture) close a group once opened and end a
    // capture once begun on every path: an error must leave neither the communicator in group mode nor the comm
    // stream capturing.
    RCCL_OR_FAIL(LBM_FAILURE);
    const RcclApi& nc = *rc_api_;
    // while a chunk is being built: the group is captured on the (single) comm stream alone -- a capture with one
    // user stream, its origin -- and enters the chunk as a child-graph node behind the comm stream's dependencies
    const bool building = (c->builder != nullptr);
    OpenCapture capture;
    if (building) {
      if (c->n_slabs != 1) LBM_FAIL(LBM_FAILURE, "hipGraph chunk: the RCCL transport is built for one communicator per process");
      HIP_TRY(LBM_FAILURE, hipStreamBeginCapture(c->slab[0].comm, hipStreamCaptureModeRelaxed));
      capture.reset(c->slab[0].comm);
    }
    OpenGroup group;  // the one group of a context without a team
    if (!c->team) {
      NCCL_TRY(LBM_FAILURE, nc.GroupStart());
      group.reset(&nc);
    }
    int rc = for_slabs(c, [&](int s) -> int {
      Slab& sl = c->slab[s];
      float* from = sl.lat[src];
      float* to = sl.lat[dst];
      int me, parts;
      if (c->ranked) { me = c->rank; parts = c->world; } else { me = s; parts = c->n_slabs; }
      // the four operations in the posting order of lbm_halo_plan (the order matters when north == south, 2 parts:
      // the first send pairs with the peer's first receive)
      lbm_halo_op ops[4];
      if (lbm_halo_plan(sl.rows, parts, me, depth, ops) != LBM_SUCCESS) return LBM_FAILURE;
      OpenGroup own_group;  // with a team: this thread's
      if (c->team) {
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        NCCL_TRY(LBM_FAILURE, nc.GroupStart());
        own_group.reset(&nc);
      }
      ncclResult_t res = ncclSuccess;
      for (int i = 0; i < 4 && res == ncclSuccess; i++) {
        float* base = ops[i].is_send ? from : to;
        float* ptr = base + (long)ops[i].row_first * c->row_pitch;
        const size_t count = (size_t)ops[i].row_count * c->row_pitch;
        res = ops[i].is_send ? nc.Send(ptr, count, ncclFloat, ops[i].peer, sl.nccl, sl.comm)
                             : nc.Recv(ptr, count, ncclFloat, ops[i].peer, sl.nccl, sl.comm);
      }
      if (own_group) {
        const ncclResult_t end = own_group.release()->GroupEnd();
        if (res == ncclSuccess) res = end;
      }
      if (res != ncclSuccess) LBM_FAIL(LBM_FAILURE, "RCCL error in the halo exchange: %s", nc.GetErrorString(res));
      return LBM_SUCCESS;
    });
    if (group) {
      const ncclResult_t end = group.release()->GroupEnd();
      if (rc == LBM_SUCCESS && end != ncclSuccess) { raise_error(__LINE__, "RCCL error: %s (ncclGroupEnd)", nc.GetErrorString(end)); rc = LBM_FAILURE; }
    }
    if (capture) {
      Graph child;  // the node holds its own copy
      const hipError_t ended = remake(child, [&](hipGraph_t* g) { return hipStreamEndCapture(capture.release(), g); });
      if (rc == LBM_SUCCESS && ended != hipSuccess) { raise_error(__LINE__, "HIP error: %s (capture of the RCCL group)", hipGetErrorString(ended)); rc = LBM_FAILURE; }
      if (rc == LBM_SUCCESS) {
        std::vector<hipGraphNode_t>& last = c->builder->last_of(c->slab[0].comm);
        hipGraphNode_t node = nullptr;
        const hipError_t added = hipGraphAddChildGraphNode(&node, c->builder->graph, last.data(), last.size(), child);
        if (added != hipSuccess) { raise_error(__LINE__, "HIP error: %s (hipGraphAddChildGraphNode)", hipGetErrorString(added)); rc = LBM_FAILURE; }
        else last.assign(1, node);
      }
    }
    if (rc != LBM_SUCCESS) return rc;
    if (stale) {
      for (int s = 0; s < c->n_slabs; s++) {
        Slab& sl = c->slab[s];
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_x[slot], sl.comm));
      }
    }
    return LBM_SUCCESS;
  }
  if (c->halo == HALO_HOST) {
    // the host's own message passing (MPI in the reference: MPI_Isend / MPI_Irecv / MPI_Waitall, MPI_Waitall/
    // d2q9-bgk.c:225-243): boundary rows to pinned host buffers, the host's exchange callback, halo rows back.
    // The callback blocks the host, so this transport does not overlap the interior rows -- it exists so that the
    // decomposition can run under an MPI-style launcher and be tested with several ranks on one device.
    if (stale) LBM_FAIL(LBM_FAILURE, "the stale-halo mode is not available with the hosted exchange");
    Slab& sl = c->slab[0];
    lbm_halo_op ops[4];
    if (lbm_halo_plan(sl.rows, c->world, c->rank, depth, ops) != LBM_SUCCESS) return LBM_FAILURE;
    float* bufs[4] = {c->host_send[0], c->host_send[1], c->host_recv[0], c->host_recv[1]};
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    for (int i = 0; i < 2; i++)
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(bufs[i], sl.lat[src] + (long)ops[i].row_first * c->row_pitch, (size_t)n * sizeof(float),
                                          hipMemcpyDeviceToHost, sl.comm));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.comm));
    if (c->host_comm.exchange(c->host_comm.user, 4, ops, bufs, (size_t)n) != 0)
      LBM_FAIL(LBM_FAILURE, "the host's halo exchange callback failed");
    for (int i = 2; i < 4; i++)
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(sl.lat[dst] + (long)ops[i].row_first * c->row_pitch, bufs[i], (size_t)n * sizeof(float),
                                          hipMemcpyHostToDevice, sl.comm));
    return LBM_SUCCESS;
  }
  if (c->halo == HALO_MEMCPY) {
    // push model inside one process: slab s copies its boundary rows into its neighbours' halo rows
    // once the neighbours have finished with the previous contents (synchronous: their boundary
    // kernels, ev_boundary, recorded in the previous phase; stale: their whole-slab pass, ev_step);
    // the neighbours' next halo-reading kernels wait for ev_halo / ev_x[slot] of the pushing slabs.
    return for_slabs(c, [&](int s) -> int {
      Slab& sl = c->slab[s];
      const int north = (s + 1) % c->n_slabs, south = (s - 1 + c->n_slabs) % c->n_slabs;
      float* from = sl.lat[src];
      Slab& sn = c->slab[north];
      Slab& ss = c->slab[south];
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      if (stale && q_wait(c, sl.comm, sl.ev_step) != LBM_SUCCESS) return LBM_FAILURE;
      if (q_wait(c, sl.comm, stale ? sn.ev_step : sn.ev_boundary) != LBM_SUCCESS) return LBM_FAILURE;
      if (q_wait(c, sl.comm, stale ? ss.ev_step : ss.ev_boundary) != LBM_SUCCESS) return LBM_FAILURE;
      if (q_copy(c, sn.lat[dst] - n, from + (long)(sl.rows - depth) * c->row_pitch, n * sizeof(float), sl.comm) != LBM_SUCCESS) return LBM_FAILURE;
      if (q_copy(c, ss.lat[dst] + (long)ss.rows * c->row_pitch, from, n * sizeof(float), sl.comm) != LBM_SUCCESS) return LBM_FAILURE;
      return q_record(c, stale ? sl.ev_x[slot] : sl.ev_halo, sl.comm);
    });
  }
  return LBM_SUCCESS;
}

// reduce the buffered per-workgroup partials of the last slot_fill steps into tot_u[step_base...]
int flush_partials(lbm_ctx* c, int step_base) {
  if (c->slot_fill == 0) return LBM_SUCCESS;
  return for_slabs(c, [&](int s) -> int {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    // the boundary rows' partials are written on the comm stream
    const bool split = (c->halo != HALO_SELF && c->halo_mode == LBM_HALO_SYNC);
    if (split) HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, sl.ev_boundary, 0));
    hipLaunchKernelGGL(lbm::reduce_partials, dim3(c->slot_fill), dim3(lbm::kBlock), 0, sl.compute,
                       sl.partials, sl.slot_counts, c->plan.part_stride, sl.tot_u, step_base, (const int*)nullptr);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    if (split) {
      // the next boundary kernels (comm stream) reuse the partial slots just read
      HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_flush, sl.compute));
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.comm, sl.ev_flush, 0));
    }
    return LBM_SUCCESS;
  });
}

// the slab threads spin between phases while a run is in flight
struct HotGuard {
  SlabTeam* t;
  explicit HotGuard(SlabTeam* team) : t(team) { if (t) { t->hot.store(true); t->cv.notify_all(); } }
  ~HotGuard() { if (t) t->hot.store(false); }
};

// device time per timestep between ev_t0 (recorded by the caller at the start of the run) and now, on
// the compute streams the step kernels run on; max over slabs
int read_step_timing(lbm_ctx* c, int n_steps, float* kernel_ms) {
  float worst = 0.f;
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_t1, sl.compute));
  }
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    HIP_TRY(LBM_FAILURE, hipEventSynchronize(sl.ev_t1));
    float ms = 0.f;
    HIP_TRY(LBM_FAILURE, hipEventElapsedTime(&ms, sl.ev_t0, sl.ev_t1));
    if (ms > worst) worst = ms;
  }
  *kernel_ms = worst / (float)n_steps;
  if (c->resident_used) {
    // the status copy of run_resident lies in front of ev_t1 on the compute stream: a call that gave up fails here
    if (const int status = gave_up(c)) {
      c->resident_used = false;
      *kernel_ms = 0.f;
      return report_give_up(c, status);
    }
  }
  return LBM_SUCCESS;
}

// The timestep loop.  Single slab: one fused launch per pass (one to four timesteps).  Several slabs / ranks
// (the Waitall pattern of MPI_Waitall/d2q9-bgk.c:225-253, restructured for two HIP streams):
//
//   compute stream:  I(0) ─────────────► I(1) ─────────────► I(2) ...     rows that touch no halo row
//                      ▲ waits B(m-1)      ▲
//   comm stream:     X(0) → B(0) → X(1) → B(1) → X(2) → B(2) ...          halo exchange, halo-touching rows
//                            ▲ waits I(m-1)
//
// I(m) and B(m) both read lattice m and write disjoint rows of lattice m+1; B(m) additionally
// needs the halos X(m) (its own stream, in order) and writes the boundary rows X(m+1) sends.  The
// chain of interior kernels is the critical path; exchange and boundary rows hide beside it.
//
// K-step passes across slabs: an output row y reads source rows y-K .. y+K, so only rows [0, K) and
// [rows-K, rows) touch halo rows.  They form two K-row bands (short sweeps: low latency on the comm
// stream); rows [K, rows-K) are the interior region, cut into bands of band_rows.

// Pipeline events in a defined state: "I(-1)" = the lattice is ready (also orders the comm stream after everything
// on the compute stream), "B(-1)" done.  Called at the start of a run and after a graph replay (events recorded
// inside a stream capture cannot be waited for outside it).
int reset_pipeline(lbm_ctx* c) {
  return for_slabs(c, [&](int s) -> int {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_interior[1], sl.compute));
    HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.comm, sl.ev_interior[1], 0));
    HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_boundary, sl.comm));
    if (c->halo == HALO_MEMCPY) HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_halo, sl.comm));
    return LBM_SUCCESS;
  });
}

// Pass m of the pipeline: X(m) (with halos), I(m), B(m), and the bookkeeping of the partial slots it fills.
//   tile > 0: that many timesteps of the LDS-tile kernel;  k >= 2: a k-step pass of the stream kernel;  else one step.
//   accel_after: apply the acceleration of the step after this pass (false on the last pass of an lbm_run call).
//   bound_events: bind the pipeline events to the kernels' own completion signals (hipExtLaunchKernel); not inside a
//   stream capture, where hipEventRecord costs nothing (it becomes a graph edge).
int issue_pass(lbm_ctx* c, int m, int tile, int k, bool accel_after, bool bound_events) {
  const bool halo = (c->halo != HALO_SELF);
  const int adv = tile ? tile : (k ? k : 1);
  const int depth = c->plan.fuse2 ? c->plan.pass_steps : 1;  // a K-step pass reads K rows beyond the slab
  if (halo && exchange_halos(c, depth, c->cur, c->cur, -1) != LBM_SUCCESS) return LBM_FAILURE;
  // phase 1: rows that touch no halo row (or the whole slab) on the compute streams
  if (for_slabs(c, [&](int s) -> int {
        Slab& sl = c->slab[s];
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        if (halo && m > 0 && q_wait(c, sl.compute, sl.ev_boundary) != LBM_SUCCESS) return LBM_FAILURE;  // B(m-1)
        hipEvent_t done = (halo && bound_events) ? sl.ev_interior[m & 1] : nullptr;  // I(m) done
        if (tile) {
          if (launch_tile(c, sl.compute, tile, accel_after) != LBM_SUCCESS) return LBM_FAILURE;
        } else if (k) {
          const int r0 = halo ? k : 0, r1 = halo ? sl.rows - k : sl.rows;
          if (launch_pass(c, s, sl.compute, k, r0, r1, c->plan.band_rows, c->plan.band_rows, ceil_div(r1 - r0, c->plan.band_rows), 0,
                          accel_after, done) != LBM_SUCCESS)
            return LBM_FAILURE;
        } else if (!halo) {
          if (launch_step(c, s, sl.compute, 0, 1, sl.rows, 0, accel_after) != LBM_SUCCESS) return LBM_FAILURE;
        } else {
          if (launch_step(c, s, sl.compute, 1, 1, sl.rows - 2, 0, accel_after, done) != LBM_SUCCESS) return LBM_FAILURE;
        }
        if (halo && !done) return q_record(c, sl.ev_interior[m & 1], sl.compute);
        return LBM_SUCCESS;
      }) != LBM_SUCCESS)
    return LBM_FAILURE;
  // phase 2: halo-touching rows / bands on the comm streams, behind the exchange X(m)
  if (halo &&
      for_slabs(c, [&](int s) -> int {
        Slab& sl = c->slab[s];
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        if (q_wait(c, sl.comm, sl.ev_interior[(m + 1) & 1]) != LBM_SUCCESS) return LBM_FAILURE;  // I(m-1)
        if (c->halo == HALO_MEMCPY) {
          const int north = (s + 1) % c->n_slabs, south = (s - 1 + c->n_slabs) % c->n_slabs;
          if (q_wait(c, sl.comm, c->slab[north].ev_halo) != LBM_SUCCESS) return LBM_FAILURE;
          if (q_wait(c, sl.comm, c->slab[south].ev_halo) != LBM_SUCCESS) return LBM_FAILURE;
        }
        hipEvent_t bdone = bound_events ? sl.ev_boundary : nullptr;  // B(m) done
        if (k) {
          // rows [0, k) and [rows-k, rows) as two k-row bands in one launch
          const int off = c->plan.n_strips * ceil_div(sl.rows - 2 * k, c->plan.band_rows);
          if (launch_pass(c, s, sl.comm, k, 0, sl.rows, k, sl.rows - k, 2, off, accel_after, bdone) != LBM_SUCCESS) return LBM_FAILURE;
        } else {
          if (launch_step(c, s, sl.comm, 0, sl.rows - 1, 2, sl.blocks_main, accel_after, bdone) != LBM_SUCCESS) return LBM_FAILURE;
        }
        if (!bdone) return q_record(c, sl.ev_boundary, sl.comm);
        return LBM_SUCCESS;
      }) != LBM_SUCCESS)
    return LBM_FAILURE;
  // bookkeeping of the partial slots written by this pass
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    const int fused_waves = halo ? c->plan.n_strips * (ceil_div(sl.rows - 2 * k, c->plan.band_rows) + 2)
                                 : c->plan.n_strips * ceil_div(sl.rows, c->plan.band_rows);
    const int n_part = tile ? tile_count(c) : (k ? fused_waves : sl.blocks_main + sl.blocks_boundary);
    for (int j = 0; j < adv; j++) sl.slot_counts.n[c->slot_fill + j] = n_part;
  }
  c->cur ^= 1;
  c->slot_fill += adv;
  return LBM_SUCCESS;
}

// Band groups: the full-depth (K-step) passes of a single periodic slab, issued so that successive passes overlap.
// The rows are cut into G groups [lo_g, hi_g) (lo_g = g H, H = rows / G, the last group takes the remainder).  Of
// pass m, the interior rows [lo_g + K, hi_g - K) of group g are I_g(m), on group stream g; the 2K seam rows
// [lo_g - K, lo_g + K) around every group start (wrapping at row 0) are S(m), one launch of G bands H rows apart, on
// the comm stream.  All of them read lat[cur] and write lat[cur ^ 1]; an output row y reads rows y-K .. y+K.
//
//   group stream g:  I_g(0) ───────► I_g(1) ───────► I_g(2) ...
//                        ▲ waits S(m-1)   ▲
//   comm stream:     S(0) ───────► S(1) ───────► S(2) ...
//                        ▲ waits I_0(m-1) .. I_{G-1}(m-1)
//
//   I_g(m) reads rows [lo_g, hi_g) of lattice m: written by I_g(m-1) (stream order) and S(m-1) (waited for).  It
//     writes rows [lo_g + K, hi_g - K) of lattice m+1, which pass m-1 read in I_g(m-1) and S(m-1) only.
//   S(m) reads rows [lo_g - 2K, lo_g + 2K): written by S(m-1) (stream order) and the interiors of the two groups
//     that meet there (waited for).  It writes the seam rows, which pass m-1 read in S(m-1) and in the interiors of
//     both groups (waited for).
// No edge runs from I_g(m) to I_h(m+1) (h != g): the interior chains drift up to a pass apart and fill the end of
// each other's launches.  Every other kind of pass, the reduce of the partials, frames and the end of a call run on
// the compute stream behind group_join; the streams fork off it again (group_fork) before the next grouped pass.
hipStream_t group_stream(Slab& sl, int g) { return g == 0 ? sl.compute : sl.group_extra[g - 1]; }

// the other streams follow everything enqueued on the compute stream; pass m is the next grouped pass
int group_fork(lbm_ctx* c, int m) {
  Slab& sl = c->slab[0];
  const int prev = (m - 1) & 1;
  if (q_record(c, sl.ev_gs[prev], sl.compute) != LBM_SUCCESS) return LBM_FAILURE;
  for (int g = 0; g < c->plan.band_groups; g++)
    if (q_record(c, sl.ev_gi[prev][g], sl.compute) != LBM_SUCCESS) return LBM_FAILURE;
  c->groups_forked = true;
  return LBM_SUCCESS;
}

// the compute stream follows the last grouped pass m on every stream
int group_join(lbm_ctx* c, int m) {
  if (!c->groups_forked) return LBM_SUCCESS;
  Slab& sl = c->slab[0];
  if (q_wait(c, sl.compute, sl.ev_gs[m & 1]) != LBM_SUCCESS) return LBM_FAILURE;
  for (int g = 1; g < c->plan.band_groups; g++)
    if (q_wait(c, sl.compute, sl.ev_gi[m & 1][g]) != LBM_SUCCESS) return LBM_FAILURE;
  c->groups_forked = false;
  return LBM_SUCCESS;
}

// rows [lo, hi) of group g; returns the group height H (the last group also takes the remainder)
int group_rows(const lbm_ctx* c, int g, int* lo, int* hi) {
  return lbm_plan::group_rows(c->slab[0].rows, c->plan.band_groups, g, lo, hi);
}

// pass m (k steps) of the single periodic slab as band groups; the streams have been forked (group_fork)
int issue_grouped_pass(lbm_ctx* c, int m, int k, bool accel_after, bool bound_events) {
  Slab& sl = c->slab[0];
  const int G = c->plan.band_groups, now = m & 1, prev = now ^ 1;
  int off = 0, h = 0;
  for (int g = 0; g < G; g++) {
    int lo, hi;
    h = group_rows(c, g, &lo, &hi);
    const hipStream_t st = group_stream(sl, g);
    if (q_wait(c, st, sl.ev_gs[prev]) != LBM_SUCCESS) return LBM_FAILURE;  // S(m-1)
    const int bands = ceil_div(hi - lo - 2 * k, c->plan.band_rows);
    hipEvent_t done = bound_events ? sl.ev_gi[now][g] : nullptr;
    if (launch_pass(c, 0, st, k, lo + k, hi - k, c->plan.band_rows, c->plan.band_rows, bands, off, accel_after, done) != LBM_SUCCESS)
      return LBM_FAILURE;
    if (!done && q_record(c, sl.ev_gi[now][g], st) != LBM_SUCCESS) return LBM_FAILURE;
    off += c->plan.n_strips * bands;
  }
  for (int g = 0; g < G; g++)
    if (q_wait(c, sl.comm, sl.ev_gi[prev][g]) != LBM_SUCCESS) return LBM_FAILURE;  // I_g(m-1)
  // seam band g: output rows [g h - k, g h + k); band 0 starts below row 0 and the kernel folds it to the top rows
  hipEvent_t sdone = bound_events ? sl.ev_gs[now] : nullptr;
  if (launch_pass(c, 0, sl.comm, k, -k, (G - 1) * h + k, 2 * k, h, G, off, accel_after, sdone) != LBM_SUCCESS)
    return LBM_FAILURE;
  if (!sdone && q_record(c, sl.ev_gs[now], sl.comm) != LBM_SUCCESS) return LBM_FAILURE;
  off += c->plan.n_strips * G;
  for (int j = 0; j < k; j++) sl.slot_counts.n[c->slot_fill + j] = off;
  c->cur ^= 1;
  c->slot_fill += k;
  return LBM_SUCCESS;
}

// ---- hipGraph replay of the timestep loop ---------------------------------------------------------------------
// A chunk = an even number of passes (so that it starts and ends on the same lattice buffer) and the reduce of
// their partial sums, built ONCE per lattice parity -- both streams of every slab, the halo exchange (RCCL
// send/recv or device copies) inside the graph -- and replayed with one hipGraphLaunch (BASELINE.json
// configs[4]: "double-buffered halos + hipGraph-captured timestep").  The graph is built node by node from the very
// issue code of the stream pipeline (GraphBuilder: virtual streams and events); only an RCCL group is captured, on
// its single comm stream, and enters as a child graph.  All launch arguments of a chunk are the same
// every time except the index of the chunk's first step in tot_u, which the reduce kernel reads from device memory.
// Every pass of a chunk applies the next step's acceleration, so a chunk is only replayed while at least one more
// timestep follows it in the same lbm_run call.  A chunk begins with its own exchange X(0) and ends with every
// stream joined, i.e. one exchange per chunk is not hidden behind interior rows (1 of 20-32).
int chunk_passes(const lbm_ctx* c, int* steps_per_pass) {
  const int halo = (c->halo != HALO_SELF);
  const int adv = (!halo && c->plan.tile_steps) ? c->plan.tile_steps : (c->plan.fuse2 ? c->plan.pass_steps : 1);
  int passes = kPartSlots / adv;
  const int cap = env_int("LBM_GRAPH_PASSES", 0);  // experiments and tests: shorter chunks
  if (cap > 0 && passes > cap) passes = cap;
  passes -= passes & 1;
  *steps_per_pass = adv;
  return passes;
}

// LBM_GRAPH_DUMP=<path>: the chunk's graph, checked before hipGraphInstantiate sees it -- node and edge
// counts, self-edges, duplicate edges, and a topological sort (Kahn) that reports whether the graph is acyclic;
// the graph itself goes to <path> as a dot file.  Returns false when the graph must not be instantiated.
bool graph_is_sound(hipGraph_t graph, const char* dump_path) {
  size_t n_nodes = 0, n_edges = 0;
  if (hipGraphGetNodes(graph, nullptr, &n_nodes) != hipSuccess || hipGraphGetEdges(graph, nullptr, nullptr, &n_edges) != hipSuccess)
    return true;  // cannot look: leave the verdict to the runtime
  if (dump_path) fprintf(stderr, "lbm_hip graph: %zu nodes, %zu edges reported\n", n_nodes, n_edges);
  std::vector<hipGraphNode_t> nodes(n_nodes), from(n_edges), to(n_edges);
  if (n_nodes && hipGraphGetNodes(graph, nodes.data(), &n_nodes) != hipSuccess) return true;
  if (n_edges && hipGraphGetEdges(graph, from.data(), to.data(), &n_edges) != hipSuccess) return true;
  auto index_of = [&](hipGraphNode_t x) -> long {
    for (size_t i = 0; i < n_nodes; i++) if (nodes[i] == x) return (long)i;
    return -1;
  };
  std::vector<long> a(n_edges), b(n_edges);
  std::vector<int> indeg(n_nodes, 0);
  size_t self_edges = 0, dup_edges = 0, foreign = 0;
  for (size_t e = 0; e < n_edges; e++) {
    a[e] = index_of(from[e]);
    b[e] = index_of(to[e]);
    if (a[e] < 0 || b[e] < 0) { foreign++; continue; }
    if (a[e] == b[e]) self_edges++;
    for (size_t f = 0; f < e; f++) if (a[f] == a[e] && b[f] == b[e]) { dup_edges++; break; }
    indeg[(size_t)b[e]]++;
  }
  // Kahn: every node of an acyclic graph is eventually freed
  std::vector<long> ready;
  for (size_t i = 0; i < n_nodes; i++) if (indeg[i] == 0) ready.push_back((long)i);
  size_t sorted = 0;
  while (!ready.empty()) {
    const long v = ready.back();
    ready.pop_back();
    sorted++;
    for (size_t e = 0; e < n_edges; e++)
      if (a[e] == v && b[e] >= 0 && --indeg[(size_t)b[e]] == 0) ready.push_back(b[e]);
  }
  const bool acyclic = (sorted == n_nodes);
  if (dump_path) {
    fprintf(stderr, "lbm_hip: chunk graph: %zu nodes, %zu edges, %zu self-edges, %zu duplicate edges, %zu edges to foreign nodes, %s\n",
            n_nodes, n_edges, self_edges, dup_edges, foreign, acyclic ? "acyclic" : "CYCLIC");
    if (*dump_path && hipGraphDebugDotPrint(graph, dump_path, hipGraphDebugDotFlagsVerbose) != hipSuccess)
      fprintf(stderr, "lbm_hip: hipGraphDebugDotPrint(%s) failed\n", dump_path);
  }
  return acyclic && self_edges == 0 && foreign == 0;
}

int build_chunk(lbm_ctx* c, GraphExec& out) {
  const bool halo = (c->halo != HALO_SELF);
  int adv;
  const int passes = chunk_passes(c, &adv);
  if (passes < 2) LBM_FAIL(LBM_FAILURE, "hipGraph chunk: no even number of passes fits");
  for (int s = 1; s < c->n_slabs; s++)
    if (c->slab[s].device != c->slab[0].device) LBM_FAIL(LBM_FAILURE, "hipGraph chunk: the slabs of one graph must share a device");
  const int tile = (!halo && c->plan.tile_steps) ? c->plan.tile_steps : 0;
  const int k = (!tile && c->plan.fuse2) ? c->plan.pass_steps : 0;
  const int saved_cur = c->cur, saved_fill = c->slot_fill;
  GraphBuilder gb;
  HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[0].device));
  HIP_TRY(LBM_FAILURE, remake(gb.graph, [](hipGraph_t* g) { return hipGraphCreate(g, 0); }));
  c->builder = &gb;
  c->slot_fill = 0;
  // Nothing is recorded yet: the first waits of pass 0 (I(-1), B(-1), the previous exchange) find no snapshot and
  // add no dependency -- "ready when the chunk starts", which is what the launch stream's order guarantees.
  int rc = LBM_SUCCESS;
  for (int m = 0; m < passes && rc == LBM_SUCCESS; m++) rc = issue_pass(c, m, tile, k, true, false);
  for (int s = 0; s < c->n_slabs && rc == LBM_SUCCESS; s++) {
    Slab& sl = c->slab[s];
    if (halo) rc = q_wait(c, sl.compute, sl.ev_boundary);  // the boundary rows' partials
    const float* partials = sl.partials;
    long stride = c->plan.part_stride;
    double* tot_u = sl.tot_u;
    int zero = 0, fill = c->slot_fill;
    const int* base_dev = sl.flushed_dev;
    int* counter = sl.flushed_dev;
    void* reduce_args[] = {&partials, &sl.slot_counts, &stride, &tot_u, &zero, &base_dev};
    if (rc == LBM_SUCCESS)
      rc = q_kernel(c, sl.compute, reinterpret_cast<const void*>(lbm::reduce_partials), dim3(c->slot_fill), dim3(lbm::kBlock), reduce_args);
    void* advance_args[] = {&counter, &fill};
    if (rc == LBM_SUCCESS)
      rc = q_kernel(c, sl.compute, reinterpret_cast<const void*>(lbm::advance_counter), dim3(1), dim3(1), advance_args);
  }
  c->builder = nullptr;
  c->cur = saved_cur;  // an even number of passes
  c->slot_fill = saved_fill;
  if (rc != LBM_SUCCESS) return LBM_FAILURE;
  const char* dump_path = getenv("LBM_GRAPH_DUMP");
  if ((dump_path && !graph_is_sound(gb.graph, dump_path)) || env_int("LBM_GRAPH_DUMP_ONLY", 0))
    LBM_FAIL(LBM_FAILURE, "hipGraph chunk: the graph is not instantiated (unsound, or LBM_GRAPH_DUMP_ONLY)");
  HIP_TRY(LBM_FAILURE, remake(out, [&](hipGraphExec_t* e) { return hipGraphInstantiate(e, gb.graph, nullptr, nullptr, 0); }));
  return LBM_SUCCESS;  // gb.graph goes with gb: the executable graph holds its own copy
}

// replays as many whole chunks as fit in front of the last timestep of this call; returns the timesteps done
int replay_chunks(lbm_ctx* c, int n_steps, int first_step, int* done) {
  *done = 0;
  int adv;
  const int chunk_steps = chunk_passes(c, &adv) * adv;
  if (chunk_steps <= 0) return LBM_SUCCESS;
  const int n_chunks = (n_steps - 1) / chunk_steps;
  if (n_chunks <= 0 || c->slot_fill != 0) return LBM_SUCCESS;
  Slab& s0 = c->slab[0];
  GraphExec& exec = s0.chunk_graph[c->cur];
  if (!exec && build_chunk(c, exec) != LBM_SUCCESS) {
    // e.g. slabs on several devices: go on launch by launch
    fprintf(stderr, "lbm_hip: hipGraph chunk not built (%s); continuing with stream launches\n", g_last_error);
    c->plan.use_graph = 0;
    return LBM_SUCCESS;
  }
  // everything enqueued so far on the other streams precedes the chunks, which run "on" slab 0's compute stream
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    hipLaunchKernelGGL(lbm::set_counter, dim3(1), dim3(1), 0, sl.compute, sl.flushed_dev, first_step);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    if (s > 0) {
      HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_step, sl.compute));
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(s0.compute, sl.ev_step, 0));
    }
    if (c->halo != HALO_SELF) {
      HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_flush, sl.comm));
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(s0.compute, sl.ev_flush, 0));
    }
  }
  HIP_TRY(LBM_FAILURE, hipSetDevice(s0.device));
  for (int k = 0; k < n_chunks; k++) HIP_TRY(LBM_FAILURE, hipGraphLaunch(exec, s0.compute));
  // ... and everything that follows on the other streams comes after them
  if (c->n_slabs > 1 || c->halo != HALO_SELF) {
    HIP_TRY(LBM_FAILURE, hipEventRecord(s0.ev_fork, s0.compute));
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      if (s > 0) HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, s0.ev_fork, 0));
      if (c->halo != HALO_SELF) HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.comm, s0.ev_fork, 0));
    }
  }
  *done = n_chunks * chunk_steps;
  return LBM_SUCCESS;
}

int run_steps_stale(lbm_ctx* c, int n_steps, float* kernel_ms);

// seam granules: [2 directions][bands][2 slots][nx] + one XCC-id granule per band
size_t resident_gran_bytes(const lbm_ctx* c) {
  return (2UL * c->plan.resident_bands * 2 * c->p.nx + c->plan.resident_bands) * sizeof(uint4);
}

// The forms of lbm::resident_band, [batched][recorder compiled in] x the five shapes: MAXT 1024 / 512 with two-row
// bands, MAXT 1024 with four-row bands, MAXT 512 with four-row bands relaxed jointly or not.  The shape is
// lbm_plan::resident_form's answer (lbm_plan.h); tests/resident_forms.py names a GPU case for each of the 50 forms.
template <bool BATCH, int REC>
const void* resident_form(int shape) {
  switch (shape) {
    case 0: return reinterpret_cast<const void*>(lbm::resident_band<1024, false, 2, BATCH, REC>);
    case 1: return reinterpret_cast<const void*>(lbm::resident_band<512, false, 2, BATCH, REC>);
    case 2: return reinterpret_cast<const void*>(lbm::resident_band<1024, false, 4, BATCH, REC>);
    case 3: return reinterpret_cast<const void*>(lbm::resident_band<512, true, 4, BATCH, REC>);
    default: return reinterpret_cast<const void*>(lbm::resident_band<512, false, 4, BATCH, REC>);
  }
}
const void* resident_kernel(int nx, int rows, int joint, int rec, bool batch = false) {
  using Form = const void* (*)(int);
  static const Form forms[2][kRecGatherFirst] = {
      {resident_form<false, kRecNone>, resident_form<false, kRecFrames>, resident_form<false, kRecProbes>, resident_form<false, kRecMean>,
       resident_form<false, kRecFields>},
      {resident_form<true, kRecNone>, resident_form<true, kRecFrames>, resident_form<true, kRecProbes>, resident_form<true, kRecMean>,
       resident_form<true, kRecFields>}};
  // (the gather kinds run the plain form)
  return forms[batch][is_gather(rec) ? kRecNone : rec](lbm_plan::resident_form(nx, rows, joint));
}

// what the resident kernels read of a context's recorder (a batch keeps one such entry per member); all zero while that
// kind is not armed
lbm::ResidentFrames frames_entry(const lbm_ctx* c) {
  if (c->rec.kind != kRecFrames) return {};
  return {c->slab[0].frames, c->rec.every, c->rec.ord0, c->rec.slots};
}
lbm::ResidentProbes probes_entry(const lbm_ctx* c) {
  if (c->rec.kind != kRecProbes) return {};
  const Slab& s0 = c->slab[0];
  return {s0.probe_ring, s0.probe_table, c->rec.every, c->rec.ord0, c->rec.slots, s0.probe_count, c->p.density, 0};
}
lbm::ResidentMean mean_entry(const lbm_ctx* c) {
  if (c->rec.kind != kRecMean) return {};
  const Slab& s0 = c->slab[0];
  return {s0.mean_sums, (long)s0.rows * c->p.nx, c->rec.every, c->p.density, c->rec.order, 0};
}
lbm::ResidentFields fields_entry(const lbm_ctx* c) {
  if (c->rec.kind != kRecFields) return {};
  const Slab& s0 = c->slab[0];
  return {s0.field_ring, c->rec.every, c->rec.ord0, c->rec.slots, c->rec.fields, c->rec.window.x0, s0.field_y0, c->rec.window.nx,
          s0.field_ny, c->p.density, 0};
}

// the fields of ResidentArgs that plain and batched launches share: n timesteps from global step epoch0, last = the
// call's last launch
void fill_resident_args(lbm::ResidentArgs& a, const lbm_ctx* c, int n, bool last, int epoch0) {
  static_cast<lbm::LatticeArgs&>(a) = lattice_args(c, c->slab[0]);  // a batched launch reads the strides only
  a.ny = c->slab[0].rows;
  a.n_steps = n;
  a.accel_row = c->slab[0].accel_row;
  a.accel_last = last ? 0 : 1;
  a.gran_bytes = (unsigned)resident_gran_bytes(c);
  a.xcd_affinity = env_int("LBM_RESIDENT_XCD", 1) ? 1 : 0;
  a.epoch0 = (unsigned)epoch0;
  a.timeout_ticks = c->plan.resident_timeout;
  a.absent_band = env_int("LBM_RESIDENT_ABSENT_BAND", -1);  // tests of the give-up path
  a.group = c->plan.resident_group;
  a.one_xcd = c->plan.resident_one_xcd;
}

// The timestep loop of a cache-resident single slab: launches of lbm::resident_band, each advancing up to
// kResidentChunk timesteps with the lattice in registers (SerialCode/d2q9-bgk.c:166-170 as ONE launch), each followed
// by the reduce of its per-band partial sums.  The caller has applied the first step's accelerate_flow.
int run_resident(lbm_ctx* c, int n_steps) {
  Slab& sl = c->slab[0];
  HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
  const bool probes = (c->rec.kind == kRecProbes), mean = (c->rec.kind == kRecMean), fields = (c->rec.kind == kRecFields);
  for (int t = 0; t < n_steps;) {
    const int n = (n_steps - t < kResidentChunk) ? n_steps - t : kResidentChunk;
    lbm::ResidentFramesArgs fa;  // the frames form's arguments, ResidentArgs + the frame fields; the plain form reads its part
    lbm::ResidentProbesArgs pa;  // the probes form's: ResidentArgs + the probe fields
    lbm::ResidentMeanArgs ma;    // the mean form's: ResidentArgs + the mean fields
    lbm::ResidentFieldsArgs da;  // the field frames' form's: ResidentArgs + the field-frame fields
    lbm::ResidentArgs& a = probes ? static_cast<lbm::ResidentArgs&>(pa)
                           : mean ? static_cast<lbm::ResidentArgs&>(ma) : fields ? static_cast<lbm::ResidentArgs&>(da) : fa;
    da.fd = fields_entry(c);
    fa.fr = frames_entry(c);
    pa.pr = probes_entry(c);
    ma.mn = mean_entry(c);
    fill_resident_args(a, c, n, t + n == n_steps, c->steps_done + t);
    a.omega = c->p.omega;
    set_accel_weights(a, c->p);
    a.gran = sl.res_gran;
    a.partials = sl.res_part;
    a.status = sl.res_status;
#ifdef LBM_RESIDENT_PROFILE
    static long long* prof_dev = nullptr;
    if (!prof_dev) HIP_TRY(LBM_FAILURE, hipMalloc(&prof_dev, 1024 * 8 * sizeof(long long)));
    a.prof = prof_dev;
#endif
    void* args[] = {&a};  // (the form's own arguments start at the base's address)
    HIP_TRY(LBM_FAILURE, hipLaunchKernel(resident_kernel(c->p.nx, c->plan.resident_rows, c->plan.resident_joint, c->rec.kind),
                                         dim3(c->plan.resident_bands / a.group * (a.one_xcd ? 8 : 1)), dim3(c->p.nx * a.group), args, 0, sl.compute));
    hipLaunchKernelGGL(lbm::reduce_band_partials, dim3(n), dim3(64), 0, sl.compute, (const float*)sl.res_part,
                       c->plan.resident_bands, sl.tot_u, c->steps_done + t);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
#ifdef LBM_RESIDENT_PROFILE
    {
      static const char* const phase[8] = {"edges->LDS", "barrier", "shifts(+interior)", "first halo answer", "further polls", "collision", "publish+sum", "extra polls (count)"};
      std::vector<long long> h(c->plan.resident_bands * 8);
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
      HIP_TRY(LBM_FAILURE, hipMemcpy(h.data(), prof_dev, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
      fprintf(stderr, "resident profile %dx%d rows %d, %d steps (s_memtime ticks per step, wave 0 of each band: mean / min / max over bands)\n", c->p.nx, sl.rows, c->plan.resident_rows, n);
      for (int i = 0; i < 8; i++) {
        double sum = 0, lo = 1e30, hi = 0;
        for (int b = 0; b < c->plan.resident_bands; b++) { const double v = (double)h[b * 8 + i] / n; sum += v; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        fprintf(stderr, "  %-20s %9.2f %9.2f %9.2f\n", phase[i], sum / c->plan.resident_bands, lo, hi);
      }
      // the bands that wait least for their neighbours set the pace: who are they, and where does their time go?
      std::vector<int> order(c->plan.resident_bands);
      for (int b = 0; b < c->plan.resident_bands; b++) order[b] = b;
      std::sort(order.begin(), order.end(), [&](int x, int y) { return h[x * 8 + 4] < h[y * 8 + 4]; });
      for (int k = 0; k < 6 && k < c->plan.resident_bands; k++) {
        const int b = order[k];
        fprintf(stderr, "  band %3d:", b);
        for (int i = 0; i < 7; i++) fprintf(stderr, " %8.1f", (double)h[b * 8 + i] / n);
        fprintf(stderr, "\n");
      }
    }
#endif
    c->cur ^= 1;
    t += n;
  }
  // the verdict of these launches travels to the host behind them; lbm_sync looks at it
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(sl.res_status_host, sl.res_status, sizeof(int), hipMemcpyDeviceToHost, sl.compute));
  c->resident_used = true;
  return LBM_SUCCESS;
}

// run_resident for every member of a batch at once: the first step's accelerate_flow for all members, then per chunk
// the sub-batch launches of the batched kernel and ONE reduce of every member's partials, all on the batch's stream
int run_batch_resident(lbm_batch* bt, int n_steps) {
  lbm_ctx* c0 = bt->members[0];
  const Slab& sl0 = c0->slab[0];
  const int n_members = (int)bt->members.size();
  HIP_TRY(LBM_FAILURE, hipSetDevice(sl0.device));
  hipLaunchKernelGGL(lbm::accelerate_row_batch, dim3(ceil_div(c0->p.nx, 256), n_members), dim3(256), 0, bt->stream,
                     (const lbm::ResidentMember*)(bt->table + bt->cur * n_members), lattice_args(c0, sl0), sl0.accel_row);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  int rec = kRecNone;  // the one kind this batch has armed, if any
  for (int kind = kRecFrames; kind < kRecKinds; kind++)
    if (bt->armed[kind] > 0) rec = kind;
  const void* kernel = resident_kernel(c0->p.nx, c0->plan.resident_rows, c0->plan.resident_joint, rec, true);
  const int bands = c0->plan.resident_bands;
  for (int t = 0; t < n_steps;) {
    const int n = (n_steps - t < kResidentChunk) ? n_steps - t : kResidentChunk;
    const lbm::ResidentMember* tab = bt->table + bt->cur * n_members;
    lbm::ResidentBatchFramesArgs fa;  // the frames form's arguments: ResidentBatchArgs + the members' frame fields
    lbm::ResidentBatchProbesArgs pa;  // the probes form's: ResidentBatchArgs + the members' probe fields
    lbm::ResidentBatchMeanArgs ma;    // the mean form's: ResidentBatchArgs + the members' mean fields
    memset(&fa, 0, sizeof(fa));
    memset(&pa, 0, sizeof(pa));
    lbm::ResidentBatchFieldsArgs da;  // the field frames' form's: ResidentBatchArgs + the members' field-frame fields
    memset(&ma, 0, sizeof(ma));
    memset(&da, 0, sizeof(da));
    lbm::ResidentBatchArgs& a = (rec == kRecProbes) ? static_cast<lbm::ResidentBatchArgs&>(pa)
                                : (rec == kRecMean) ? static_cast<lbm::ResidentBatchArgs&>(ma)
                                : (rec == kRecFields) ? static_cast<lbm::ResidentBatchArgs&>(da) : fa;
    fill_resident_args(a, c0, n, t + n == n_steps, bt->steps_done + t);
    a.status = bt->status;
    a.member_wgs = bt->member_wgs;
    for (int first = 0; first < n_members; first += bt->members_per_launch) {
      a.members = tab + first;
      fa.frames = bt->frame_table ? bt->frame_table + first : nullptr;
      pa.probes = bt->probe_table ? bt->probe_table + first : nullptr;
      ma.means = bt->mean_table ? bt->mean_table + first : nullptr;
      da.fields = bt->field_table ? bt->field_table + first : nullptr;
      a.n_members = (n_members - first < bt->members_per_launch) ? n_members - first : bt->members_per_launch;
      const int grid = a.one_xcd ? bt->member_wgs * 8 : a.n_members * (int)round_up(bt->member_wgs, 8);
      void* args[] = {&a};
      HIP_TRY(LBM_FAILURE, hipLaunchKernel(kernel, dim3(grid), dim3(c0->p.nx * a.group), args, 0, bt->stream));
    }
    hipLaunchKernelGGL(lbm::reduce_band_partials_batch, dim3(n, n_members), dim3(64), 0, bt->stream, tab, bands,
                       bt->steps_done + t);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    bt->cur ^= 1;
    t += n;
  }
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(bt->status_host, bt->status, sizeof(int), hipMemcpyDeviceToHost, bt->stream));
  for (lbm_ctx* c : bt->members) {
    c->cur = bt->cur;
    c->resident_used = true;
  }
  return LBM_SUCCESS;
}

// records made by the global steps [from, to): those with tt % every == 0
long long recorded_between(const Recorder& r, long long from, long long to) {
  if (r.every <= 0) return 0;
  const long long e = r.every;
  return (to + e - 1) / e - (from + e - 1) / e;
}

// lbm_run / lbm_batch_run refuse a call whose records would not fit the free slots, before any work is issued; a kind
// that accumulates its records (the mean fields) has room for any call
int recorder_fits(const Recorder& r, int steps_done, int n_steps, const char* who, const char* reader) {
  const RecorderKind& k = kind_words(r.kind);
  if (!k.slotted || r.slots == 0) return LBM_SUCCESS;  // (no slots: a gather kind armed without a ring)
  const long long add = recorded_between(r, steps_done, (long long)steps_done + n_steps);
  const long long waiting = r.written - r.read;
  if (waiting + add > r.slots)
    LBM_FAIL(LBM_FAILURE, "%s: %d steps would record %lld %ss, but the %s buffer holds %d and %lld %ss are waiting (%s drains them)",
             who, n_steps, add, k.record, k.record, r.slots, waiting, k.record, reader);
  return LBM_SUCCESS;
}
int recorder_fits(const lbm_ctx* c, int n_steps, const char* who) {
  return recorder_fits(c->rec, c->steps_done, n_steps, who, kind_words(c->rec.kind).reader);
}

// workgroups of stats_gather / stats_gather_batch for `cells` cells of a slab or member, V at a time per lane: one unit
// per lane where the cap allows, the lanes striding over the rest
int stats_groups(long cells, int v) {
  const long groups = ceil_div(cells / v, lbm::kBlock);
  return groups > lbm::kStatsMaxGroups ? lbm::kStatsMaxGroups : (int)groups;
}
// cells per lane and unit: four (16-byte loads) where the rows allow it
int stats_vector(int nx) { return nx % 4 == 0 ? 4 : 1; }

// one statistics sample of a slab's current lattice into `words` (zeroed in front, on the same stream)
void launch_stats_gather(const lbm_ctx* c, const Slab& sl, long long* words) {
  const int v = stats_vector(c->p.nx);
  const dim3 grid(stats_groups((long)sl.rows * c->p.nx, v));
  const unsigned cell_first = (unsigned)sl.row_first * (unsigned)c->p.nx;
  if (v == 4)
    hipLaunchKernelGGL(lbm::stats_gather<4>, grid, dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl), sl.rows, cell_first, words);
  else
    hipLaunchKernelGGL(lbm::stats_gather<1>, grid, dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl), sl.rows, cell_first, words);
}

// one residual sample of a slab's current lattice against `planes` ([2][rows][nx]: the recorder's, or a checked run's
// own) into `words` (zeroed in front, on the same stream); baseline: the planes are filled from the lattice and nothing
// is reduced.  With a gate the sample stands back once the gate's stop word is set (residual_gather_unless).
void launch_residual_gather(const lbm_ctx* c, const Slab& sl, float* planes, long long* words, bool baseline,
                            const lbm::SteadyState* gate = nullptr) {
  const int v = stats_vector(c->p.nx);
  const dim3 grid(stats_groups((long)sl.rows * c->p.nx, v)), block(lbm::kBlock);
  const unsigned cell_first = (unsigned)sl.row_first * (unsigned)c->p.nx;
  float* px = planes;
  float* py = px + (size_t)sl.rows * c->p.nx;
  if (gate)
    hipLaunchKernelGGL(v == 4 ? lbm::residual_gather_unless<4> : lbm::residual_gather_unless<1>, grid, block, 0, sl.compute, lattice_args(c, sl),
                       sl.rows, cell_first, px, py, words, gate);
  else
    hipLaunchKernelGGL(v == 4 ? lbm::residual_gather<4> : lbm::residual_gather<1>, grid, block, 0, sl.compute, lattice_args(c, sl), sl.rows,
                       cell_first, px, py, words, (int)baseline);
}

// the stress of the rows [row_begin, row_begin + rows) of a slab's current lattice on its compute stream: into `field`
// (three dense planes of rows * nx floats; or null) and / or `words` (a zeroed slot of the ring; or null).  The deal is
// stats_gather's
void launch_stress_gather(const lbm_ctx* c, const Slab& sl, int row_begin, int rows, float* field, long long* words) {
  const int nx = c->p.nx;
  const bool v4 = stats_vector(nx) == 4;
  const dim3 grid(stats_groups((long)rows * nx, v4 ? 4 : 1));
  const unsigned cell_first = (unsigned)sl.row_first * (unsigned)nx;
  const auto kernel = field ? (v4 ? lbm::stress_gather<4, true> : lbm::stress_gather<1, true>)
                            : (v4 ? lbm::stress_gather<4, false> : lbm::stress_gather<1, false>);  // (the form without the fields' stores)
  hipLaunchKernelGGL(kernel, grid, dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl), row_begin, rows, cell_first, field, (long)rows * nx,
                     words);
}

// rows of a band of profile_columns / profile_columns_batch for `rows` rows of nx cells: about kProfileTargetGroups
// workgroups where the grid has that many bands of kProfileMinBand rows, so that small and large grids both fill the device
constexpr int kProfileTargetGroups = 1024;  // four workgroups per CU
int profile_band_rows(int rows, int nx) {
  const int col_groups = ceil_div(nx, lbm::kProfileColumns);
  const int bands = kProfileTargetGroups / col_groups > 1 ? kProfileTargetGroups / col_groups : 1;
  const int band_rows = ceil_div(rows, bands);
  return band_rows > lbm::kProfileMinBand ? band_rows : lbm::kProfileMinBand;
}

// one profile sample of a slab's current lattice into `lines` (zeroed in front, on the same stream): its row lines, then
// its share of the column lines
void launch_profiles(const lbm_ctx* c, const Slab& sl, long long* lines) {
  const int nx = c->p.nx;
  if (c->rec.args.axes & LBM_PROFILE_ROWS) {
    const dim3 grid(ceil_div(sl.rows, lbm::kBlock / 64));
    if (stats_vector(nx) == 4)
      hipLaunchKernelGGL(lbm::profile_rows<4>, grid, dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl), sl.rows, lines);
    else
      hipLaunchKernelGGL(lbm::profile_rows<1>, grid, dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl), sl.rows, lines);
    lines += (size_t)sl.rows * lbm_profile::kProfileWords;
  }
  if (c->rec.args.axes & LBM_PROFILE_COLUMNS) {
    const int band_rows = profile_band_rows(sl.rows, nx);
    hipLaunchKernelGGL(lbm::profile_columns, dim3(ceil_div(nx, lbm::kProfileColumns), ceil_div(sl.rows, band_rows)), dim3(lbm::kBlock), 0,
                       sl.compute, lattice_args(c, sl), sl.rows, band_rows, lines);
  }
}

// what a slab holds of the coarse grid of bx x by boxes (lbm_coarse_row.h), and the words of its slot
lbm_coarse::SlabBoxRows coarse_slab_boxes(const lbm_ctx* c, const Slab& sl, int bx, int by) {
  return lbm_coarse::slab_box_rows(c->p.nx, c->p.ny, bx, by, sl.row_first, sl.rows);
}
size_t coarse_slot_words(const lbm_ctx* c, const Slab& sl, int bx, int by) { return lbm_coarse::slot_words(coarse_slab_boxes(c, sl, bx, by)); }
// workgroups of coarse_gather for one box row: a box each where bx > 64, else four wave spans of floor(64 / bx) boxes
bool coarse_wide(int bx) { return bx > 64; }
int coarse_groups(const lbm_coarse::SlabBoxRows& g) {
  return coarse_wide(g.bx) ? g.cx : ceil_div(ceil_div(g.cx, 64 / g.bx), lbm::kBlock / 64);
}

// one coarse sample of a slab's current lattice into `words` (zeroed in front, on the same stream): its whole box rows as
// lines, its partial ones as limb words
void launch_coarse(const lbm_ctx* c, const Slab& sl, int bx, int by, long long* words) {
  const lbm_coarse::SlabBoxRows g = coarse_slab_boxes(c, sl, bx, by);
  const int groups = coarse_groups(g);
  const dim3 grid((unsigned)g.count * (unsigned)groups);
  hipLaunchKernelGGL(coarse_wide(bx) ? lbm::coarse_gather<true> : lbm::coarse_gather<false>, grid, dim3(lbm::kBlock), 0, sl.compute,
                     lattice_args(c, sl), g, groups, words);
}

// rows of a band of vorticity_gather / vorticity_gather_batch for `rows` rows of nx cells: about kVortTargetUnits units
// (a wave's strip of 64 * V columns of a band) where the grid has that many bands of kVortMinBand rows, so that small and
// large grids both fill the device and a large one reads few rows twice
constexpr int kVortTargetUnits = 4096;  // four waves per SIMD
int vorticity_strips(int nx) { return ceil_div(nx, 64 * stats_vector(nx)); }
int vorticity_band_rows(int rows, int nx) {
  const int strips = vorticity_strips(nx);
  const int bands = kVortTargetUnits / strips > 1 ? kVortTargetUnits / strips : 1;
  const int band_rows = ceil_div(rows, bands);
  return band_rows > lbm::kVortMinBand ? band_rows : lbm::kVortMinBand;
}
// ... and its workgroups, a unit per wave where the cap allows
int vorticity_groups(int rows, int nx, int band_rows) {
  const long groups = ceil_div((long)vorticity_strips(nx) * ceil_div(rows, band_rows), lbm::kBlock / 64);
  return groups > lbm::kVortMaxGroups ? lbm::kVortMaxGroups : (int)groups;
}

// the vorticity of a slab's rows [row_begin, row_end) of its current lattice on its compute stream: into `field` (dense,
// row row_begin first) and / or `words` (zeroed in front, on the same stream).  edges: [2][row_pitch], the rows below and
// above the slab; nullptr: the slab is the whole periodic grid and they are its own last and first row.
void launch_vorticity_gather(const lbm_ctx* c, const Slab& sl, const float* edges, int row_begin, int row_end, float* field, long long* words) {
  const int nx = c->p.nx, n = row_end - row_begin;
  const int band_rows = vorticity_band_rows(n, nx);
  const dim3 grid(vorticity_groups(n, nx, band_rows));
  const float* south = edges ? edges : sl.lat[c->cur] + (long)(sl.rows - 1) * c->row_pitch;
  const float* north = edges ? edges + c->row_pitch : sl.lat[c->cur];
  const unsigned cell_first = (unsigned)sl.row_first * (unsigned)nx;
  const bool v4 = stats_vector(nx) == 4;
  const auto kernel = field ? (v4 ? lbm::vorticity_gather<4, true> : lbm::vorticity_gather<1, true>)
                            : (v4 ? lbm::vorticity_gather<4, false> : lbm::vorticity_gather<1, false>);  // (the form without the field's store)
  hipLaunchKernelGGL(kernel, grid, dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl), south, north, sl.rows, row_begin, row_end, band_rows,
                     cell_first, field, words);
}

// The rows a slab does not own, for vorticity_gather on several slabs: slab s's `edges` ([2][row_pitch]) get the last row
// of its south neighbour's and the first row of its north neighbour's current lattice, by copies on s's compute stream
// behind the neighbours' ev_vort_ready (recorded by the caller on their compute streams, behind the pass that wrote the
// rows).  The lattice halo rows are not used: after a pass they are not defined to hold the neighbours' current rows.
int copy_vorticity_edges(lbm_ctx* c, int s, float* edges) {
  Slab& sl = c->slab[s];
  const Slab& ss = c->slab[(s - 1 + c->n_slabs) % c->n_slabs];
  const Slab& sn = c->slab[(s + 1) % c->n_slabs];
  const size_t row_bytes = (size_t)c->row_pitch * sizeof(float);
  HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, ss.ev_vort_ready, 0));
  HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, sn.ev_vort_ready, 0));
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(edges, ss.lat[c->cur] + (long)(ss.rows - 1) * c->row_pitch, row_bytes, hipMemcpyDefault, sl.compute));
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(edges + c->row_pitch, sn.lat[c->cur], row_bytes, hipMemcpyDefault, sl.compute));
  return LBM_SUCCESS;
}
// every slab's compute stream marks "my rows of the current lattice are written" (several slabs)
int mark_vorticity_ready(lbm_ctx* c) {
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    if (!sl.ev_vort_ready) HIP_TRY(LBM_FAILURE, sl.ev_vort_ready.create(hipEventDisableTiming));
    if (!sl.ev_vort_done) HIP_TRY(LBM_FAILURE, sl.ev_vort_done.create(hipEventDisableTiming));
    HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_vort_ready, sl.compute));
  }
  return LBM_SUCCESS;
}
// ... and, once every slab has recorded ev_vort_done behind its sample, waits for its neighbours': the later passes,
// which overwrite the current lattice two passes on, run behind the copies of its rows
int await_vorticity_done(lbm_ctx* c) {
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, c->slab[(s - 1 + c->n_slabs) % c->n_slabs].ev_vort_done, 0));
    HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, c->slab[(s + 1) % c->n_slabs].ev_vort_done, 0));
  }
  return LBM_SUCCESS;
}

// rows of a band of the stream function's scan (psi_band_totals, psi_band_bases, psi_scan) for `rows` rows of nx cells:
// LBM_PSI_BAND_ROWS where it is set (read once per context), else, as profile_band_rows, about kProfileTargetGroups
// workgroups where the grid has that many bands of kPsiMinBand rows.  The height changes no bit of any psi.
int psi_band_rows(lbm_ctx* c, int rows, int nx) {
  if (c->psi_band_env < 0) {
    const int env = lbm_plan::env_int("LBM_PSI_BAND_ROWS", 0);
    c->psi_band_env = env > 0 ? env : 0;
  }
  if (c->psi_band_env > 0) return c->psi_band_env;
  const int col_groups = ceil_div(nx, lbm::kPsiColumns);
  const int bands = kProfileTargetGroups / col_groups > 1 ? kProfileTargetGroups / col_groups : 1;
  const int band_rows = ceil_div(rows, bands);
  return band_rows > lbm::kPsiMinBand ? band_rows : lbm::kPsiMinBand;
}
// elements of the scan's two scratch buffers for one slab or member
size_t psi_total_words(int rows, int nx, int band_rows) { return (size_t)ceil_div(rows, band_rows) * nx * lbm_exact::kExactLimbs; }
size_t psi_candidates(int rows, int nx, int band_rows) { return (size_t)ceil_div(rows, band_rows) * ceil_div(nx, lbm::kPsiColumns); }

// the first two sweeps of a slab's scan on its compute stream: the band totals, then the bands' bases in place, from the
// limbs below the slab (`incoming`, nullptr: it is the lowest) and with the limbs up to its last row left in `outgoing`
// (nullptr: nobody asks)
void launch_psi_totals(const lbm_ctx* c, const Slab& sl, int band_rows, long long* totals) {
  const int nx = c->p.nx;
  hipLaunchKernelGGL(lbm::psi_band_totals, dim3(ceil_div(nx, lbm::kPsiColumns), ceil_div(sl.rows, band_rows)), dim3(lbm::kBlock), 0,
                     sl.compute, lattice_args(c, sl), sl.rows, band_rows, totals);
}
void launch_psi_bases(const lbm_ctx* c, const Slab& sl, int band_rows, long long* totals, const long long* incoming, long long* outgoing) {
  const int nx = c->p.nx;
  hipLaunchKernelGGL(lbm::psi_band_bases, dim3(ceil_div(nx * lbm_exact::kExactLimbs, lbm::kBlock)), dim3(lbm::kBlock), 0, sl.compute, nx, ceil_div(sl.rows, band_rows),
                     totals, incoming, outgoing);
}

// One stream-function sample of every slab into its zeroed slot of the ring.  The totals of all slabs run side by side;
// then the slabs are chained from the lowest up: slab s copies slab s-1's psi_out (behind its ev_psi_out) into its own
// psi_in, forms its bases and its psi_out, scans and reduces.  Slab s-1's next sample overwrites its psi_out only behind
// slab s's copy (ev_psi_taken).  Issued by the calling thread, slab after slab: the chain has an order.
size_t gather_slot_words(const lbm_ctx* c, const Slab& sl);
long long* zeroed_slot(long long* ring, size_t slot_words, const Recorder& r, hipStream_t stream, bool* ringless);
int take_psi_record(lbm_ctx* c) {
  const int nx = c->p.nx;
  const size_t base_bytes = (size_t)nx * lbm_exact::kExactLimbs * sizeof(long long);
  long long* words[kMaxSlabs];
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    bool ringless;
    if (!(words[s] = zeroed_slot(sl.gather_ring, gather_slot_words(c, sl), c->rec, sl.compute, &ringless))) return LBM_FAILURE;
    launch_psi_totals(c, sl, sl.psi_band_rows, sl.psi_totals);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
  }
  const bool chain = c->n_slabs > 1;
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    if (chain && s > 0) {
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, c->slab[s - 1].ev_psi_out, 0));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(sl.psi_in, c->slab[s - 1].psi_out, base_bytes, hipMemcpyDefault, sl.compute));
      HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_psi_taken, sl.compute));
    }
    const bool hands_on = chain && s + 1 < c->n_slabs;
    launch_psi_bases(c, sl, sl.psi_band_rows, sl.psi_totals, (chain && s > 0) ? sl.psi_in.get() : nullptr, hands_on ? sl.psi_out.get() : nullptr);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    if (hands_on) HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_psi_out, sl.compute));
    const dim3 grid(ceil_div(nx, lbm::kPsiColumns), ceil_div(sl.rows, sl.psi_band_rows));
    hipLaunchKernelGGL(lbm::psi_scan<false>, grid, dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl), sl.rows, sl.psi_band_rows, 0,
                       (const long long*)sl.psi_totals, (unsigned)sl.row_first * (unsigned)nx, (double*)nullptr, sl.psi_cand.get());
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    hipLaunchKernelGGL(lbm::psi_extrema, dim3(1), dim3(64), 0, sl.compute, (const lbm::PsiCandidate*)sl.psi_cand, (int)(grid.x * grid.y), words[s]);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
  }
  if (chain)
    for (int s = 0; s + 1 < c->n_slabs; s++) {  // the next sample's psi_band_bases of slab s runs behind slab s+1's copy
      HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[s].device));
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(c->slab[s].compute, c->slab[s + 1].ev_psi_taken, 0));
    }
  return LBM_SUCCESS;
}

// words of one slot of a slab's gather_ring: this slab's share of a record of the armed kind
size_t gather_slot_words(const lbm_ctx* c, const Slab& sl) { return gather_kind(c->rec.kind).slot_words(c, sl, c->rec.args); }
// ... and of a batch's: that of slab 0 for every member, one after the other
size_t gather_slot_words(const lbm_batch* bt) {
  const lbm_ctx* c0 = bt->members[0];
  return bt->members.size() * gather_kind(bt->rec.kind).slot_words(c0, c0->slab[0], bt->rec.args);
}

// the slot of the next record of a gather ring, zeroed on `stream` (the gather kernels add into it): nullptr where that failed
// -- and where the kind is armed without a ring (*ringless: nullptr is then no failure; the kind's launch records nowhere)
long long* zeroed_slot(long long* ring, size_t slot_words, const Recorder& r, hipStream_t stream, bool* ringless) {
  if ((*ringless = r.slots == 0)) return nullptr;
  long long* slot = ring + (size_t)(r.written % r.slots) * slot_words;
  HIP_TRY(nullptr, hipMemsetAsync(slot, 0, slot_words * sizeof(long long), stream));
  return slot;
}

// the n oldest waiting records of a ring of slot_words elements per slot into dst, record after record, over `stream` (of
// the current device); they are on the host when this returns
template <class T, class U>
int fetch_ring(const T* ring, size_t slot_words, const Recorder& r, int n, hipStream_t stream, U* dst) {
  static_assert(sizeof(T) == sizeof(U), "the host's element is the device's");
  const lbm_ring::Runs runs = lbm_ring::oldest_runs(r.read, r.slots, n);
  for (int j = 0; j < runs.n; j++) {
    const lbm_ring::Run& run = runs.run[j];
    HIP_TRY(LBM_FAILURE, hipMemcpyAsync(dst + (size_t)run.at * slot_words, ring + run.first * slot_words,
                                        (size_t)run.count * slot_words * sizeof(T), hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(LBM_FAILURE, hipStreamSynchronize(stream));
  return LBM_SUCCESS;
}

// the record of the current (stored) lattice into the next slot, on every slab's compute stream: the frame of its rows,
// or the gathered samples of the probes in its rows; or, for the mean fields, the sample of its rows added to their sums;
// or, for a gather kind, what its take says
int take_record(lbm_ctx* c) {
  if (is_gather(c->rec.kind)) {
    if (gather_kind(c->rec.kind).take(c) != LBM_SUCCESS) return LBM_FAILURE;
    c->rec.written++;
    return LBM_SUCCESS;
  }
  const size_t slot = kind_words(c->rec.kind).slotted ? (size_t)(c->rec.written % c->rec.slots) : 0;
  const size_t n_probes = c->probe_cells.size();
  if (for_slabs(c, [&](int s) -> int {
        Slab& sl = c->slab[s];
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        const long n = (long)sl.rows * c->p.nx;
        if (c->rec.kind == kRecFrames)
          hipLaunchKernelGGL(lbm::frame_umag, dim3(ceil_div(n, 256)), dim3(256), 0, sl.compute, lattice_args(c, sl), sl.rows,
                             sl.frames + slot * n);
        else if (c->rec.kind == kRecFields) {
          const lbm_window& w = c->rec.window;
          const long cells = (long)sl.field_ny * w.nx;  // 0: the window misses this slab
          if (cells > 0)
            hipLaunchKernelGGL(lbm::field_frame, dim3(ceil_div(cells, 256)), dim3(256), 0, sl.compute, lattice_args(c, sl), c->p.density,
                               c->rec.fields, w.x0, sl.field_y0, w.nx, sl.field_ny,
                               sl.field_ring + slot * (size_t)__builtin_popcount((unsigned)c->rec.fields) * (size_t)cells);
        } else if (c->rec.kind == kRecMean)
          hipLaunchKernelGGL(lbm::mean_accumulate, dim3(ceil_div(n, 256)), dim3(256), 0, sl.compute, lattice_args(c, sl), sl.rows,
                             c->p.density, sl.mean_sums, n, c->rec.order);
        else if (sl.probe_count > 0)
          hipLaunchKernelGGL(lbm::probe_gather, dim3(ceil_div(sl.probe_count, 64)), dim3(64), 0, sl.compute, lattice_args(c, sl),
                             c->p.density, (const lbm::ProbeEntry*)sl.probe_table, sl.probe_count, sl.probe_ring + slot * n_probes);
        HIP_TRY(LBM_FAILURE, hipGetLastError());
        return LBM_SUCCESS;
      }) != LBM_SUCCESS)
    return LBM_FAILURE;
  c->rec.written++;
  return LBM_SUCCESS;
}

// n_steps timesteps on the kernels chosen by `resident` (no timing read-out: the caller does it)
int run_passes(lbm_ctx* c, int n_steps, bool resident, bool record_t0) {
  const AccelWeights w = accel_weights(c->p);
  const bool halo = (c->halo != HALO_SELF);
  HotGuard hot_guard(c->team);

  // accelerate_flow() of the first step (later steps: epilogue of the step kernel)
  if (for_slabs(c, [&](int s) -> int {
        Slab& sl = c->slab[s];
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        if (sl.accel_row >= 0 && sl.accel_row < sl.rows) {
          hipLaunchKernelGGL(lbm::accelerate_row, dim3(ceil_div(c->p.nx, 256)), dim3(256), 0, sl.compute,
                             lattice_args(c, sl, c->cur, c->cur), sl.accel_row, w.a1, w.a2);
          HIP_TRY(LBM_FAILURE, hipGetLastError());
        }
        if (record_t0) HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_t0, sl.compute));
        return LBM_SUCCESS;
      }) != LBM_SUCCESS)
    return LBM_FAILURE;

  if (resident) {
    const long long records = recorded_between(c->rec, c->steps_done, (long long)c->steps_done + n_steps);
    if (run_resident(c, n_steps) != LBM_SUCCESS) return LBM_FAILURE;
    c->steps_done += n_steps;
    if (!is_gather(c->rec.kind)) c->rec.written += records;  // recorded by the kernel itself (a gather kind: by the caller, behind it)
    return LBM_SUCCESS;
  }

  int flushed_upto = c->steps_done;
  int t_first = 0;
  if (c->plan.use_graph) {
    if (replay_chunks(c, n_steps, flushed_upto, &t_first) != LBM_SUCCESS) return LBM_FAILURE;
    flushed_upto += t_first;
  }
  if (halo && reset_pipeline(c) != LBM_SUCCESS) return LBM_FAILURE;

  // passes launch by launch: pass_steps timesteps per pass where enabled and that many remain, else two, else one
  static const int ext_events = env_int("LBM_EXT_EVENTS", 1);
  const int slots_per_pass = c->plan.tile_steps > c->plan.pass_steps ? c->plan.tile_steps : c->plan.pass_steps;
  int m = 0;  // pass counter (event parity)
  for (int t = t_first; t < n_steps; m++) {
    const int tile = (!halo && c->plan.tile_steps) ? (c->plan.tile_steps < n_steps - t ? c->plan.tile_steps : n_steps - t) : 0;
    const int k = (!tile && c->plan.fuse2 && n_steps - t >= 2) ? (n_steps - t >= c->plan.pass_steps ? c->plan.pass_steps : 2) : 0;
    const int adv = tile ? tile : (k ? k : 1);
    const bool last = (t + adv == n_steps);
    // full-depth passes of a single periodic slab as band groups; every other pass behind a join
    const bool grouped = (c->plan.band_groups > 1 && !halo && !tile && k == c->plan.pass_steps);
    if (grouped) {
      if (!c->groups_forked && group_fork(c, m) != LBM_SUCCESS) return LBM_FAILURE;
      if (issue_grouped_pass(c, m, k, !last, ext_events != 0) != LBM_SUCCESS) return LBM_FAILURE;
    } else {
      if (group_join(c, m - 1) != LBM_SUCCESS) return LBM_FAILURE;
      if (issue_pass(c, m, tile, k, !last, ext_events != 0) != LBM_SUCCESS) return LBM_FAILURE;
    }
    t += adv;
    if (c->slot_fill + slots_per_pass > kPartSlots || last) {
      // the reduce reads the partials of every stream; the streams fork again after it
      if (grouped && group_join(c, m) != LBM_SUCCESS) return LBM_FAILURE;
      if (flush_partials(c, flushed_upto) != LBM_SUCCESS) return LBM_FAILURE;
      flushed_upto += c->slot_fill;
      c->slot_fill = 0;
    }
  }
  c->steps_done += n_steps;
  // (the last flush made every compute stream wait for its final boundary kernel)
  return LBM_SUCCESS;
}

int run_steps(lbm_ctx* c, int n_steps, float* kernel_ms) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_run: null context");
  if (n_steps < 0) LBM_FAIL(LBM_FAILURE, "lbm_run: negative step count");
  if (kernel_ms) *kernel_ms = 0.f;
  if (n_steps == 0) return LBM_SUCCESS;
  if (c->steps_done + n_steps > c->capacity)
    LBM_FAIL(LBM_FAILURE, "lbm_run: %d steps requested but the av_vels record holds %d (maxIters)",
             c->steps_done + n_steps, c->capacity);
  if (recorder_fits(c, n_steps, "lbm_run") != LBM_SUCCESS) return LBM_FAILURE;
  if (c->halo != HALO_SELF && c->halo_mode != LBM_HALO_SYNC) return run_steps_stale(c, n_steps, kernel_ms);

  // resident or per-pass: decided once per call, whether a recorder (frames or probes) is armed or not
  const bool resident = c->plan.resident && n_steps >= c->plan.resident_min_steps;
  const bool behind = is_gather(c->rec.kind);
  if (c->rec.kind != kRecNone && (!resident || behind)) {
    // per-pass kernels: the call runs as the sub-calls that end at its recorder steps, each followed by its frame or
    // its sample row (the step kernels themselves record nothing).  The gather kinds always run so, whatever kernels advance
    // the lattice: a sub-call long enough for the resident kernel runs it (its plain form), as a call of that length would
    const int e = c->rec.every;
    for (int t = 0; t < n_steps;) {
      const int tt = c->steps_done, r = tt % e;
      const long long rec_tt = r ? (long long)tt + (e - r) : tt;  // next recorder step
      const int seg = (rec_tt - tt + 1 < n_steps - t) ? (int)(rec_tt - tt + 1) : n_steps - t;
      const bool seg_resident = behind && c->plan.resident && seg >= c->plan.resident_min_steps;
      if (run_passes(c, seg, seg_resident, kernel_ms && t == 0) != LBM_SUCCESS) return LBM_FAILURE;
      if (c->steps_done - 1 == rec_tt && take_record(c) != LBM_SUCCESS) return LBM_FAILURE;
      t += seg;
    }
  } else if (run_passes(c, n_steps, resident, kernel_ms != nullptr) != LBM_SUCCESS) {
    return LBM_FAILURE;
  }
  return kernel_ms ? read_step_timing(c, n_steps, kernel_ms) : LBM_SUCCESS;
}

// ---- freshest-available halo mode ------------------------------------------------------------------------------
int ensure_fresh_buffers(lbm_ctx* c) {
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    if (sl.ev_fresh[1]) continue;  // created last: the set is whole (an attempt that failed half-way starts again)
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    HIP_TRY(LBM_FAILURE, sl.fresh_stage.alloc(4 * (size_t)c->row_pitch));
    HIP_TRY(LBM_FAILURE, sl.fresh_arrived.alloc(4));
    HIP_TRY(LBM_FAILURE, sl.fresh_id_src.alloc(2));
    HIP_TRY(LBM_FAILURE, sl.fresh_decision.alloc(1));
    HIP_TRY(LBM_FAILURE, sl.fresh_log.alloc((size_t)c->capacity));
    HIP_TRY(LBM_FAILURE, hipMemset(sl.fresh_arrived, 0, 4 * sizeof(unsigned)));
    HIP_TRY(LBM_FAILURE, hipMemset(sl.fresh_decision, 0, sizeof(int)));
    HIP_TRY(LBM_FAILURE, hipMemset(sl.fresh_log, 3, (size_t)c->capacity));  // synchronous and first passes: both sides fresh
    for (int i = 0; i < 2; i++) HIP_TRY(LBM_FAILURE, sl.ev_fresh[i].create(hipEventDisableTiming));
  }
  return LBM_SUCCESS;
}

// F(m): the boundary rows of the lattice `src` (timestep id - 1 of the run, just produced) travel towards the staging
// rows [par] of the ring neighbours, each followed in stream order by `id`.  Same preconditions as the stale exchange
// (exchange_halos, slot >= 0): behind ev_step of this slab and, where this slab writes into its neighbours' memory
// itself, of the neighbours -- their previous pass, the last reader of staging [par] (two passes ago), is over.
// Nobody ever waits for it (LBM_FRESH_FORCE=wait excepted: tests).
int fresh_exchange(lbm_ctx* c, int src, int par, unsigned id) {
  const long n = c->row_pitch;
  // tests: hold about half of the (step, slab) exchanges back by so many microseconds, so that looks miss them
  const int delay_us = env_int("LBM_FRESH_TEST_DELAY_US", 0);
  auto delayed = [&](int s) { return delay_us > 0 && ((((id * 2654435761u) >> 11) ^ (unsigned)s) & 1u) != 0; };
  if (c->halo == HALO_RCCL) {
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.comm, sl.ev_step, 0));
      if (delayed(s)) hipLaunchKernelGGL(lbm::fresh_test_delay, dim3(1), dim3(1), 0, sl.comm, (long long)delay_us * 100);
    }
    RCCL_OR_FAIL(LBM_FAILURE);
    const RcclApi& nc = *rc_api_;
    if (!c->team) NCCL_TRY(LBM_FAILURE, nc.GroupStart());
    int rc = for_slabs(c, [&](int s) -> int {
      Slab& sl = c->slab[s];
      int me, parts;
      if (c->ranked) { me = c->rank; parts = c->world; } else { me = s; parts = c->n_slabs; }
      lbm_halo_op ops[4];
      if (lbm_halo_plan(sl.rows, parts, me, 1, ops) != LBM_SUCCESS) return LBM_FAILURE;
      if (c->team) {
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        NCCL_TRY(LBM_FAILURE, nc.GroupStart());
      }
      ncclResult_t res = ncclSuccess;
      for (int i = 0; i < 4 && res == ncclSuccess; i++) {
        // a receive of halo row -1 (rows) lands in the south (north) staging row instead
        float* ptr = ops[i].is_send ? sl.lat[src] + (long)ops[i].row_first * c->row_pitch
                                    : sl.fresh_stage + ((long)par * 2 + (ops[i].row_first < 0 ? 0 : 1)) * n;
        res = ops[i].is_send ? nc.Send(ptr, (size_t)n, ncclFloat, ops[i].peer, sl.nccl, sl.comm)
                             : nc.Recv(ptr, (size_t)n, ncclFloat, ops[i].peer, sl.nccl, sl.comm);
      }
      if (c->team) {
        const ncclResult_t end = nc.GroupEnd();
        if (res == ncclSuccess) res = end;
      }
      if (res != ncclSuccess) LBM_FAIL(LBM_FAILURE, "RCCL error in the halo exchange: %s", nc.GetErrorString(res));
      return LBM_SUCCESS;
    });
    if (!c->team) {
      const ncclResult_t end = nc.GroupEnd();
      if (rc == LBM_SUCCESS && end != ncclSuccess) { raise_error(__LINE__, "RCCL error: %s (ncclGroupEnd)", nc.GetErrorString(end)); rc = LBM_FAILURE; }
    }
    if (rc != LBM_SUCCESS) return rc;
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      hipLaunchKernelGGL(lbm::fresh_mark, dim3(1), dim3(1), 0, sl.comm, sl.fresh_arrived + par * 2, sl.fresh_arrived + par * 2 + 1, id);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_fresh[par], sl.comm));
    }
    return LBM_SUCCESS;
  }
  if (c->halo == HALO_MEMCPY) {
    return for_slabs(c, [&](int s) -> int {
      Slab& sl = c->slab[s];
      Slab& sn = c->slab[(s + 1) % c->n_slabs];
      Slab& ss = c->slab[(s - 1 + c->n_slabs) % c->n_slabs];
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.comm, sl.ev_step, 0));
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.comm, sn.ev_step, 0));
      HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.comm, ss.ev_step, 0));
      if (delayed(s)) hipLaunchKernelGGL(lbm::fresh_test_delay, dim3(1), dim3(1), 0, sl.comm, (long long)delay_us * 100);
      hipLaunchKernelGGL(lbm::fresh_mark, dim3(1), dim3(1), 0, sl.comm, sl.fresh_id_src + par, (unsigned*)nullptr, id);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      // my top row is my north neighbour's south halo row, my row 0 my south neighbour's north halo row
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(sn.fresh_stage + ((long)par * 2 + 0) * n, sl.lat[src] + (long)(sl.rows - 1) * c->row_pitch,
                                          (size_t)n * sizeof(float), hipMemcpyDefault, sl.comm));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(sn.fresh_arrived + par * 2 + 0, sl.fresh_id_src + par, sizeof(unsigned), hipMemcpyDefault, sl.comm));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(ss.fresh_stage + ((long)par * 2 + 1) * n, sl.lat[src], (size_t)n * sizeof(float), hipMemcpyDefault, sl.comm));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(ss.fresh_arrived + par * 2 + 1, sl.fresh_id_src + par, sizeof(unsigned), hipMemcpyDefault, sl.comm));
      HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_fresh[par], sl.comm));
      return LBM_SUCCESS;
    });
  }
  LBM_FAIL(LBM_FAILURE, "the freshest-available halo mode is not available with the hosted exchange");
}

// Stale-halo ("asynchronous") timestep loop: the GPU analogue of the reference's research variant,
// MPI_Testall_OptimizedVersion/d2q9-bgk.c:256-301, which replaces MPI_Waitall by MPI_Testall and relaxes
// the boundary rows with whatever halo contents are there.  Here the staleness is pinned to exactly
// one pass, which keeps the run reproducible: pass m reads its own rows of lattice m but the halo
// rows its neighbours sent from lattice m-1 (pass 0 of every lbm_run call starts from fresh halos).
// Nothing on the compute stream ever waits for an exchange issued in the same pass:
//
//   compute stream:  S(0) ──────► S(1) ──────► S(2) ──────► S(3) ...    whole slab, one launch per pass
//                      │  ▲ X'(0)   │  ▲ X'(1)   │  ▲ X'(2)
//   comm stream:       └► X'(1) ────┴► X'(2) ────┴► X'(3) ...            X'(k): boundary rows of lattice k
//                                                                         -> halo rows S(k+1) reads
//
// X'(k) starts when S(k-1) has written lattice k and has a whole pass to land.  It writes the halo
// rows of the OTHER lattice buffer (the one S(k+1) reads), which S(k-1) finished reading and S(k)
// never touches, so there is no torn read -- unlike the reference, whose Irecv may land mid-row.
// Stale passes always advance ONE timestep, also where the synchronous pipeline uses the two-step kernel:
// then every population that crosses a slab boundary is simply delayed by one step -- nothing is lost or
// duplicated, steady states are unchanged, and the transient stays within 1 % (2 slabs) .. 4 % (8 slabs
// of 16 rows) of the synchronous run on the reference's 128x128 case.  With two steps per pass the
// redundantly relaxed halo-adjacent rows would be computed from stale data on one side of the seam and
// from fresh data on the other, which no longer conserves mass: measured, that variant drifts past the
// 1 % rule with 2 slabs and diverges to NaN after 2172 steps with 8 (profiles/r01_tuning.md).
//
// LBM_HALO_FRESHEST on top of that -- the reference's rule itself, "look once, never wait" (MPI_Testall_Optimized
// Version/d2q9-bgk.c:262-290: post the exchange, relax the interior rows, MPI_Testall, relax the boundary rows with
// whatever is there): the rows of lattice k ALSO travel (F(k), first on the comm stream) towards a staging row per
// side, followed by the step's id; S(k) is cut into interior rows, one look at the ids (fresh_decide: which sides have
// arrived, noted in the log), whole staging rows moved over the one-pass-old halo rows where they have (fresh_adopt),
// boundary rows.  Every halo row is the row of this pass or of the pass before -- never older, never torn -- and
// given the log of decisions the run is reproducible (tests/slab_model.py: run_slabs_freshest).
int run_steps_stale(lbm_ctx* c, int n_steps, float* kernel_ms) {
  const AccelWeights w = accel_weights(c->p);
  const int depth = 1;  // one timestep per pass (see above): only the adjacent row is read
  const bool freshest = (c->halo_mode == LBM_HALO_FRESHEST);
  // tests: "wait" makes every look find its rows (= the synchronous run), "never" sends none (= the stale mode)
  const char* force_env = freshest ? getenv("LBM_FRESH_FORCE") : nullptr;
  const bool force_wait = force_env && !strcmp(force_env, "wait"), force_never = force_env && !strcmp(force_env, "never");
  if (freshest && c->halo == HALO_HOST) LBM_FAIL(LBM_FAILURE, "the freshest-available halo mode is not available with the hosted exchange");
  if (freshest && ensure_fresh_buffers(c) != LBM_SUCCESS) return LBM_FAILURE;
  HotGuard hot_guard(c->team);

  // accelerate_flow() of the first step, then fresh halos for pass 0 (same lattice) and, from the same
  // rows, the one-pass-old halos of pass 1 (other lattice)
  if (for_slabs(c, [&](int s) -> int {
        Slab& sl = c->slab[s];
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        if (sl.accel_row >= 0 && sl.accel_row < sl.rows) {
          hipLaunchKernelGGL(lbm::accelerate_row, dim3(ceil_div(c->p.nx, 256)), dim3(256), 0, sl.compute,
                             lattice_args(c, sl, c->cur, c->cur), sl.accel_row, w.a1, w.a2);
          HIP_TRY(LBM_FAILURE, hipGetLastError());
        }
        HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_step, sl.compute));
        if (kernel_ms) HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_t0, sl.compute));
        return LBM_SUCCESS;
      }) != LBM_SUCCESS)
    return LBM_FAILURE;
  if (exchange_halos(c, depth, c->cur, c->cur, 1) != LBM_SUCCESS) return LBM_FAILURE;      // read by S(0)
  if (exchange_halos(c, depth, c->cur, c->cur ^ 1, 0) != LBM_SUCCESS) return LBM_FAILURE;  // read by S(1)

  int flushed_upto = c->steps_done;
  for (int m = 0; m < n_steps; m++) {  // pass m = timestep m of this call
    const bool last = (m + 1 == n_steps);
    const int slot = (m + 1) & 1;  // the exchange S(m) consumes: issued during pass m-2 (or the prologue)
    if (for_slabs(c, [&](int s) -> int {
          Slab& sl = c->slab[s];
          HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
          // own exchange: my halo rows have landed (RCCL) and the boundary rows of the lattice this pass
          // overwrites have been read out (the copies X'(m-1) made from it)
          HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, sl.ev_x[slot], 0));
          if (c->halo == HALO_MEMCPY) {
            // push model: my halo rows are written by the neighbours' streams
            const int north = (s + 1) % c->n_slabs, south = (s - 1 + c->n_slabs) % c->n_slabs;
            HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, c->slab[north].ev_x[slot], 0));
            HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, c->slab[south].ev_x[slot], 0));
          }
          if (!freshest) {
            if (launch_step(c, s, sl.compute, 0, 1, sl.rows, 0, !last) != LBM_SUCCESS) return LBM_FAILURE;
          } else {
            const int par = m & 1;
            const unsigned id = (unsigned)(c->steps_done + m) + 1u;
            if (launch_step(c, s, sl.compute, 1, 1, sl.rows - 2, 0, !last) != LBM_SUCCESS) return LBM_FAILURE;
            if (m > 0 && force_wait) {
              if (c->halo == HALO_MEMCPY) {
                const int north = (s + 1) % c->n_slabs, south = (s - 1 + c->n_slabs) % c->n_slabs;
                HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, c->slab[north].ev_fresh[par], 0));
                HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, c->slab[south].ev_fresh[par], 0));
              } else {
                HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, sl.ev_fresh[par], 0));
              }
            }
            hipLaunchKernelGGL(lbm::fresh_decide, dim3(1), dim3(1), 0, sl.compute, (const unsigned*)(sl.fresh_arrived + par * 2), id,
                               m == 0 ? 1 : 0, sl.fresh_decision, sl.fresh_log + c->steps_done + m);
            HIP_TRY(LBM_FAILURE, hipGetLastError());
            if (m > 0) {
              const long n = c->row_pitch;
              float* lat = sl.lat[c->cur];
              hipLaunchKernelGGL(lbm::fresh_adopt, dim3(ceil_div(n, 256)), dim3(256), 0, sl.compute, (const int*)sl.fresh_decision,
                                 (const unsigned*)(sl.fresh_stage + ((long)par * 2 + 0) * n), (const unsigned*)(sl.fresh_stage + ((long)par * 2 + 1) * n),
                                 (unsigned*)(lat - n), (unsigned*)(lat + (long)sl.rows * c->row_pitch), n);
              HIP_TRY(LBM_FAILURE, hipGetLastError());
            }
            if (launch_step(c, s, sl.compute, 0, sl.rows - 1, 2, sl.blocks_main, !last) != LBM_SUCCESS) return LBM_FAILURE;
          }
          HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_step, sl.compute));
          return LBM_SUCCESS;
        }) != LBM_SUCCESS)
      return LBM_FAILURE;
    for (int s = 0; s < c->n_slabs; s++)
      c->slab[s].slot_counts.n[c->slot_fill] = freshest ? c->slab[s].blocks_main + c->slab[s].blocks_boundary : blocks_for_rows(c, c->slab[s].rows);
    c->cur ^= 1;
    c->slot_fill += 1;
    // F(m+1): the rows S(m) just produced, for S(m+1) itself if they get there before its look
    if (!last && freshest && !force_never && fresh_exchange(c, c->cur, (m + 1) & 1, (unsigned)(c->steps_done + m + 1) + 1u) != LBM_SUCCESS)
      return LBM_FAILURE;
    // X'(m+1): the same rows, for S(m+2)
    if (!last && exchange_halos(c, depth, c->cur, c->cur ^ 1, slot) != LBM_SUCCESS) return LBM_FAILURE;
    if (c->slot_fill >= kPartSlots - 1 || last) {
      if (flush_partials(c, flushed_upto) != LBM_SUCCESS) return LBM_FAILURE;
      flushed_upto += c->slot_fill;
      c->slot_fill = 0;
    }
  }
  c->steps_done += n_steps;

  // leave the comm streams ordered before whatever the host enqueues on the compute streams next
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    for (int i = 0; i < 2; i++) HIP_TRY(LBM_FAILURE, hipStreamWaitEvent(sl.compute, sl.ev_x[i], 0));
  }
  return kernel_ms ? read_step_timing(c, n_steps, kernel_ms) : LBM_SUCCESS;
}

bool validate_params(const lbm_params* p) {
  // the cell count must fit the reference's int counters (tot_cells, SerialCode/d2q9-bgk.c:411)
  return p && p->nx >= 1 && p->ny >= 2 && p->max_iters >= 0 && (long)p->nx * (long)p->ny <= 2147483647L;
}

// Build one slab: allocate, build the mask on the device, fill the lattice.
int build_slab(lbm_ctx* c, int s, const ObstacleSource& obst, const float* cells_aos) {
  Slab& sl = c->slab[s];
  const lbm_params& p = c->p;
  HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
  HIP_TRY(LBM_FAILURE, sl.compute_own.create());
  sl.compute = sl.compute_own;
  HIP_TRY(LBM_FAILURE, sl.comm.create());
  HIP_TRY(LBM_FAILURE, sl.ev_boundary.create(hipEventDisableTiming));
  HIP_TRY(LBM_FAILURE, sl.ev_halo.create(hipEventDisableTiming));
  for (int i = 0; i < 2; i++) HIP_TRY(LBM_FAILURE, sl.ev_interior[i].create(hipEventDisableTiming));
  HIP_TRY(LBM_FAILURE, sl.ev_flush.create(hipEventDisableTiming));
  HIP_TRY(LBM_FAILURE, sl.ev_step.create(hipEventDisableTiming));
  HIP_TRY(LBM_FAILURE, sl.ev_fork.create(hipEventDisableTiming));
  for (int i = 0; i < 2; i++) HIP_TRY(LBM_FAILURE, sl.ev_x[i].create(hipEventDisableTiming));
  HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_halo, sl.comm));
  HIP_TRY(LBM_FAILURE, sl.ev_t0.create(hipEventDefault));
  HIP_TRY(LBM_FAILURE, sl.ev_t1.create(hipEventDefault));
  if (c->plan.band_groups > 1) {
    for (int g = 0; g < c->plan.band_groups - 1; g++) HIP_TRY(LBM_FAILURE, sl.group_extra[g].create());
    for (int i = 0; i < 2; i++) {
      HIP_TRY(LBM_FAILURE, sl.ev_gs[i].create(hipEventDisableTiming));
      for (int g = 0; g < c->plan.band_groups; g++) HIP_TRY(LBM_FAILURE, sl.ev_gi[i][g].create(hipEventDisableTiming));
    }
  }

  // lattices with kHaloRows halo rows below and above the owned rows (zeroed: pitch padding and
  // unused halo rows stay finite); lat[] points at owned row 0
  const size_t lat_bytes = (size_t)(sl.rows + 2 * kHaloRows) * c->row_pitch * sizeof(float);
  for (int i = 0; i < 2; i++) {
    HIP_TRY(LBM_FAILURE, sl.lat_alloc[i].alloc_bytes(lat_bytes));
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(sl.lat_alloc[i], 0, lat_bytes, sl.compute));
    sl.lat[i] = sl.lat_alloc[i] + (size_t)kHaloRows * c->row_pitch;
  }
  HIP_TRY(LBM_FAILURE, sl.partials.alloc((size_t)kPartSlots * c->plan.part_stride));
  HIP_TRY(LBM_FAILURE, hipMemsetAsync(sl.partials, 0, (size_t)kPartSlots * c->plan.part_stride * sizeof(float), sl.compute));
  HIP_TRY(LBM_FAILURE, sl.tot_u.alloc((size_t)(c->capacity > 0 ? c->capacity : 1)));
  HIP_TRY(LBM_FAILURE, hipMemsetAsync(sl.tot_u, 0, (size_t)(c->capacity > 0 ? c->capacity : 1) * sizeof(double), sl.compute));
  HIP_TRY(LBM_FAILURE, sl.scratch.alloc(2 * kSumBlocks));
  HIP_TRY(LBM_FAILURE, sl.flushed_dev.alloc(1));
  if (c->plan.resident) {
    // granules start at tag 0 = "nothing"; tags are global step indices + 1, so they never need clearing again
    const size_t gran_bytes = resident_gran_bytes(c);
    HIP_TRY(LBM_FAILURE, sl.res_gran.alloc_bytes(gran_bytes));
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(sl.res_gran, 0, gran_bytes, sl.compute));
    HIP_TRY(LBM_FAILURE, sl.res_part.alloc((size_t)kResidentChunk * c->plan.resident_bands));
    HIP_TRY(LBM_FAILURE, sl.res_status.alloc(1));
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(sl.res_status, 0, sizeof(int), sl.compute));
    HIP_TRY(LBM_FAILURE, sl.res_status_host.alloc(1));
    *sl.res_status_host = 0;
  }
  if (c->ranked) HIP_TRY(LBM_FAILURE, sl.reduce_buf.alloc((size_t)(c->capacity > 0 ? c->capacity : 1)));

  // obstacle mask: uint8 (rows + 2*kMaskHalo) x pitch with the (periodic) neighbour rows beyond the slab, which a
  // multi-step pass relaxes redundantly.  Built on the device: from the reference's host type (int, SerialCode/
  // d2q9-bgk.c:541) uploaded row range by row range through a bounded staging buffer, or expanded from a small tile.
  {
    const int mrows = sl.rows + 2 * kMaskHalo;
    const long mask_cells = (long)mrows * c->pitch;
    HIP_TRY(LBM_FAILURE, sl.mask_alloc.alloc((size_t)mask_cells));
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(sl.mask_alloc, 0, (size_t)mask_cells, sl.compute));
    sl.mask = sl.mask_alloc + (size_t)kMaskHalo * c->pitch;
    if (obst.kind == OBST_TILE) {
      const size_t tn = (size_t)obst.tile_nx * obst.tile_ny;
      std::vector<unsigned char> t8(tn);
      for (size_t i = 0; i < tn; i++) t8[i] = obst.data[i] ? 1 : 0;
      DeviceBuf<unsigned char> tile_dev;
      HIP_TRY(LBM_FAILURE, tile_dev.alloc(tn));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(tile_dev, t8.data(), tn, hipMemcpyHostToDevice, sl.compute));
      hipLaunchKernelGGL(lbm::mask_from_tile, dim3(ceil_div((long)p.nx * mrows, 256)), dim3(256), 0, sl.compute, tile_dev,
                         obst.tile_nx, obst.tile_ny, sl.mask_alloc, p.nx, c->pitch, sl.row_first - kMaskHalo, mrows, p.ny);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    } else {
      long chunk_rows = (32L << 20) / ((long)p.nx * sizeof(int));
      if (chunk_rows < 1) chunk_rows = 1;
      DeviceBuf<int> stage;
      HIP_TRY(LBM_FAILURE, stage.alloc((size_t)chunk_rows * p.nx));
      for (int r = 0; r < mrows;) {
        // source row of mask row r, and how many rows from there are contiguous in the source
        long src_row;
        int run = mrows - r;
        if (obst.kind == OBST_ROWS) {
          src_row = (long)(sl.row_first - c->row_first) + r;  // the caller's array starts kMaskHalo rows below its first row
        } else {
          const int g = ((sl.row_first - kMaskHalo + r) % p.ny + p.ny) % p.ny;
          src_row = g;
          if (run > p.ny - g) run = p.ny - g;
        }
        if (run > chunk_rows) run = (int)chunk_rows;
        HIP_TRY(LBM_FAILURE, hipMemcpyAsync(stage, obst.data + (size_t)src_row * p.nx, (size_t)run * p.nx * sizeof(int),
                                            hipMemcpyHostToDevice, sl.compute));
        hipLaunchKernelGGL(lbm::mask_from_int, dim3(ceil_div((long)p.nx * run, 256)), dim3(256), 0, sl.compute, stage,
                           sl.mask_alloc + (size_t)r * c->pitch, p.nx, c->pitch, run);
        HIP_TRY(LBM_FAILURE, hipGetLastError());
        HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));  // the staging buffer is reused
        r += run;
      }
    }
    // fluid cells of the owned rows (the reference counts them while parsing, MPI_Waitall/d2q9-bgk.c:794-804)
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(sl.scratch.get());
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), sl.compute));
    hipLaunchKernelGGL(lbm::count_blocked, dim3(ceil_div((long)c->pitch * sl.rows, 256 * 16)), dim3(256), 0, sl.compute,
                       sl.mask, (long)c->pitch * sl.rows, cnt);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    unsigned long long blocked = 0;
    HIP_TRY(LBM_FAILURE, hipMemcpyAsync(&blocked, cnt, sizeof(blocked), hipMemcpyDeviceToHost, sl.compute));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    sl.fluid_cells = (long)p.nx * sl.rows - (long)blocked;
  }

  // lattice: equilibrium or the caller's cells
  if (!cells_aos) {
    const float r0 = p.density * 4.f / 9.f;  // SerialCode/d2q9-bgk.c:546-548
    const float r1 = p.density / 9.f;
    const float r2 = p.density / 36.f;
    hipLaunchKernelGGL(lbm::init_equilibrium, dim3(ceil_div((long)p.nx * sl.rows, 256)), dim3(256), 0,
                       sl.compute, lattice_args(c, sl, 0, 0), sl.rows, r0, r1, r2);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
  } else {
    // upload in chunks of rows through a staging buffer, transposing AoS -> SoA on the device
    const int chunk_rows = (int)(((64L << 20) / ((long)p.nx * lbm::kQ * sizeof(float))) > 0
                                     ? ((64L << 20) / ((long)p.nx * lbm::kQ * sizeof(float)))
                                     : 1);
    DeviceBuf<float> stage;
    HIP_TRY(LBM_FAILURE, stage.alloc((size_t)chunk_rows * p.nx * lbm::kQ));
    for (int r0 = 0; r0 < sl.rows; r0 += chunk_rows) {
      const int nr = (sl.rows - r0 < chunk_rows) ? sl.rows - r0 : chunk_rows;
      const size_t n = (size_t)nr * p.nx * lbm::kQ;
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(stage, cells_aos + (size_t)(sl.row_first - (obst.local_cells ? c->row_first : 0) + r0) * p.nx * lbm::kQ,
                                          n * sizeof(float), hipMemcpyHostToDevice, sl.compute));
      hipLaunchKernelGGL(lbm::aos_to_soa, dim3(ceil_div((long)n, 256)), dim3(256), 0, sl.compute, stage,
                         lattice_args(c, sl, 0, 0), r0, nr);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    }
  }
  HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
  return LBM_SUCCESS;
}

// ---- create: the steps of create_common, in its order --------------------------------------------------------------
// 1. everything that can be refused before a context exists; *ndev: the visible devices
bool validate_create(const lbm_params* params, const ObstacleSource& obst, int n_slabs, int math_mode, int rank, int world, int* ndev) {
  if (!validate_params(params)) LBM_FAIL(false, "lbm_create: invalid parameters");
  if (!obst.data) LBM_FAIL(false, "lbm_create: obstacles is NULL");
  if (obst.kind == OBST_TILE && (obst.tile_nx < 1 || obst.tile_ny < 1))
    LBM_FAIL(false, "lbm_create: invalid obstacle tile %dx%d", obst.tile_nx, obst.tile_ny);
  if (math_mode != LBM_MATH_EXACT && math_mode != LBM_MATH_FAST)
    LBM_FAIL(false, "lbm_create: unknown math mode %d", math_mode);
  if (n_slabs < 1 || n_slabs > kMaxSlabs) LBM_FAIL(false, "lbm_create: n_gpus must be 1..%d", kMaxSlabs);
  if (hipGetDeviceCount(ndev) != hipSuccess || *ndev < 1)
    LBM_FAIL(false, "lbm_create: no HIP device available (this library has no CPU path)");
  // rows of this context, then of its slabs: no part thinner than 2 rows
  int row_count = 0;
  if (lbm_partition_rows(params->ny, world, rank, nullptr, &row_count) != LBM_SUCCESS) return false;
  if (n_slabs > 1 && lbm_partition_rows(row_count, n_slabs, 0, nullptr, nullptr) != LBM_SUCCESS) return false;
  return true;
}

// 2. how the halo rows travel ...
int decide_halo_kind(const lbm_ctx* c, int ndev) {
  const bool force_halo = env_int("LBM_FORCE_HALO", 0) != 0;
  if (c->world > 1 || (c->ranked && force_halo)) return c->hosted ? HALO_HOST : HALO_RCCL;
  if (c->n_slabs == 1 && !force_halo) return HALO_SELF;
  const char* h = getenv("LBM_HALO");
  const bool distinct = (c->n_slabs <= ndev);
  return (h && !strcmp(h, "memcpy")) ? HALO_MEMCPY : (h && !strcmp(h, "rccl")) ? HALO_RCCL : (distinct ? HALO_RCCL : HALO_MEMCPY);
}
// ... and how fresh they are (LBM_HALO_MODE); the experimental modes say so once per process and mode
void warn_experimental_halo_mode(const lbm_ctx* c, bool* warned, const char* text) {
  if (*warned || c->halo == HALO_SELF || c->rank != 0) return;
  *warned = true;
  fprintf(stderr, "lbm_hip: LBM_HALO_MODE=%s\n", text);
}
int decide_halo_mode(const lbm_ctx* c) {
  static bool warned_stale = false, warned_freshest = false;
  const char* hm = getenv("LBM_HALO_MODE");
  if (hm && !strcmp(hm, "stale")) {
    warn_experimental_halo_mode(c, &warned_stale,
                                "stale is EXPERIMENTAL: halo rows one pass old; results differ from the "
                                "synchronous run (measured up to 4.7 % on av_vels mid-transient, outside check.py's 1 % rule)");
    return LBM_HALO_STALE;
  }
  if (hm && !strcmp(hm, "freshest") && !c->hosted) {
    warn_experimental_halo_mode(c, &warned_freshest,
                                "freshest is EXPERIMENTAL: every halo row is this step's or the step before's, "
                                "whichever has arrived; results differ from the synchronous run and from run to run");
    return LBM_HALO_FRESHEST;
  }
  return LBM_HALO_SYNC;
}

// 3. what plan_kernels is asked: the grid and its decomposition, and what the devices say
PlanInput plan_input(const lbm_ctx* c, int ndev) {
  PlanInput in;
  in.nx = c->p.nx;
  in.ny = c->p.ny;
  in.world = c->world;
  in.rank = c->rank;
  in.n_slabs = c->n_slabs;
  in.halo = c->halo;
  in.n_devices = ndev;
  const int dev = c->slab[0].device;
  if (hipSetDevice(dev) != hipSuccess || hipDeviceGetAttribute(&in.cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) in.cus = 0;
  in.distinct_devices = c->n_slabs > 1;
  for (int a = 0; a < c->n_slabs; a++)
    for (int b = a + 1; b < c->n_slabs; b++)
      if (c->slab[a].device == c->slab[b].device) in.distinct_devices = false;
  return in;
}

// 4. the plan's resident candidate stands if the device can hold a workgroup of its kernel on a CU
bool resident_fits(const lbm_ctx* c) {
  int per_cu = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, resident_kernel(c->p.nx, c->plan.resident_rows, c->plan.resident_joint, kRecNone),
                                                      c->p.nx, 0) == hipSuccess && per_cu >= 1;
}

// 5. the slabs: their rows as the plan counted them, their buffers, mask and lattice
int build_slabs(lbm_ctx* c, const PlanInput& in, const ObstacleSource& obst, const float* cells_aos) {
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    const SlabRows r = lbm_plan::slab_rows(in, c->plan.vec4, s);
    sl.row_first = r.row_first;
    sl.rows = r.rows;
    sl.accel_row = r.accel_row;
    sl.accel_row2 = r.accel_row2;
    sl.blocks_main = r.blocks_main;
    sl.blocks_boundary = r.blocks_boundary;
    if (c->halo != HALO_SELF && sl.rows < 2) LBM_FAIL(LBM_FAILURE, "lbm_create: a slab needs at least 2 rows");
  }
  for (int s = 0; s < c->n_slabs; s++)
    if (build_slab(c, s, obst, cells_aos) != LBM_SUCCESS) return LBM_FAILURE;
  return LBM_SUCCESS;
}

// 6. what carries the halo rows between processes / slabs: pinned staging buffers for the host's message passing, or
// RCCL communicators
int connect_ranks(lbm_ctx* c, const void* unique_id) {
  if (c->hosted) {
    const size_t floats = (size_t)kHaloRows * c->row_pitch;
    for (int i = 0; i < 2; i++)
      if (c->host_send[i].alloc(floats) != hipSuccess || c->host_recv[i].alloc(floats) != hipSuccess)
        LBM_FAIL(LBM_FAILURE, "lbm_create_rank_hosted: cannot allocate the pinned exchange buffers");
  } else if (c->ranked) {
    // one process per GPU: the communicator spans the ranks (also used for the av_vels reduce)
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    RcclApi* nc = rccl();
    ncclResult_t res = ncclSuccess;
    if (!nc || hipSetDevice(c->slab[0].device) != hipSuccess ||
        (res = nc->CommInitRank(&c->slab[0].nccl, c->world, id, c->rank)) != ncclSuccess)
      LBM_FAIL(LBM_FAILURE, "lbm_create_rank: ncclCommInitRank(rank %d of %d) failed: %s", c->rank, c->world,
               nc ? nc->GetErrorString(res) : g_rccl_error);
  } else if (c->halo == HALO_RCCL) {
    ncclComm_t comms[kMaxSlabs];
    int devs[kMaxSlabs];
    for (int s = 0; s < c->n_slabs; s++) devs[s] = c->slab[s].device;
    RcclApi* nc = rccl();
    ncclResult_t res = ncclSuccess;
    if (!nc || (res = nc->CommInitAll(comms, c->n_slabs, devs)) != ncclSuccess)
      LBM_FAIL(LBM_FAILURE, "lbm_create: ncclCommInitAll failed: %s (set LBM_HALO=memcpy when slabs share a device)",
               nc ? nc->GetErrorString(res) : g_rccl_error);
    for (int s = 0; s < c->n_slabs; s++) c->slab[s].nccl = comms[s];
  }
  return LBM_SUCCESS;
}

// 7. global number of fluid cells (av_velocity's divisor): the slabs' device-side counts, summed over the ranks
// (the reference counts on rank 0 while parsing, MPI_Waitall/d2q9-bgk.c:794-804)
int count_fluid_cells(lbm_ctx* c) {
  long long fluid = 0;
  for (int s = 0; s < c->n_slabs; s++) fluid += c->slab[s].fluid_cells;
  if (c->hosted && c->world > 1) {
    double v = (double)fluid;  // exact: a cell count is below 2^31
    if (c->host_comm.allreduce_sum(c->host_comm.user, &v, 1) != 0)
      LBM_FAIL(LBM_FAILURE, "lbm_create_rank_hosted: the host's all-reduce callback failed");
    fluid = (long long)(v + 0.5);
  } else if (c->ranked && c->world > 1) {
    Slab& sl = c->slab[0];
    long long* dev = reinterpret_cast<long long*>(sl.scratch.get());
    if (hipSetDevice(sl.device) != hipSuccess ||
        hipMemcpy(dev, &fluid, sizeof(fluid), hipMemcpyHostToDevice) != hipSuccess ||
        !rccl() || g_rccl.AllReduce(dev, dev, 1, ncclInt64, ncclSum, sl.nccl, sl.comm) != ncclSuccess ||
        hipStreamSynchronize(sl.comm) != hipSuccess ||
        hipMemcpy(&fluid, dev, sizeof(fluid), hipMemcpyDeviceToHost) != hipSuccess)
      LBM_FAIL(LBM_FAILURE, "lbm_create_rank: all-reduce of the fluid-cell count failed");
  }
  c->fluid_cells = (int)fluid;
  return LBM_SUCCESS;
}

lbm_ctx* create_common(const lbm_params* params, const ObstacleSource& obst, const float* cells_aos,
                       int n_slabs, int math_mode, int rank, int world, const void* unique_id,
                       int device, const lbm_host_comm* host_comm = nullptr) {
  int ndev = 0;
  if (!validate_create(params, obst, n_slabs, math_mode, rank, world, &ndev)) return nullptr;

  lbm_ctx* c = new lbm_ctx();
  c->p = *params;
  c->math_mode = math_mode;
  c->rank = rank;
  c->world = world;
  c->capacity = params->max_iters;
  c->pitch = (int)round_up(params->nx, 64);
  c->plane_stride = c->pitch + env_int("LBM_PLANE_PAD_FLOATS", 0) / 4 * 4;
  c->row_pitch = 9 * c->plane_stride;
  c->n_slabs = n_slabs;
  const lbm_plan::RowSpan mine = lbm_plan::row_span(params->ny, world, rank);
  c->row_first = mine.first;
  c->row_count = mine.count;
  c->ranked = (unique_id != nullptr) || (host_comm != nullptr);
  c->hosted = (host_comm != nullptr);
  if (c->hosted) c->host_comm = *host_comm;
  for (int s = 0; s < n_slabs; s++) c->slab[s].device = c->ranked ? device : (s % ndev);
  c->halo = decide_halo_kind(c, ndev);
  c->halo_mode = decide_halo_mode(c);

  const PlanInput in = plan_input(c, ndev);
  c->plan = lbm_plan::plan_kernels(in);
  if (c->plan.resident && !resident_fits(c)) c->plan = lbm_plan::without_resident(c->plan);

  if (build_slabs(c, in, obst, cells_aos) != LBM_SUCCESS || connect_ranks(c, unique_id) != LBM_SUCCESS ||
      count_fluid_cells(c) != LBM_SUCCESS) {
    lbm_destroy(c);
    return nullptr;
  }
  if (c->plan.want_team) {
    c->team = new SlabTeam();
    c->team->start(n_slabs);
  }
  return c;
}

// ---- the recorder of a context: what the setters and the readers of every kind share -------------------------------
// a batch member's entry of the table the batched launches of one kind read; the table is allocated, all zero, when the
// first member arms that kind
template <class Entry>
int set_batch_entry(lbm_ctx* c, DeviceBuf<Entry>& table, const Entry& entry) {
  const lbm_batch* bt = c->batch;
  if (!table && entry.every == 0) return LBM_SUCCESS;
  int index = 0;
  while (bt->members[(size_t)index] != c) index++;
  HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[0].device));
  if (!table) {
    DeviceBuf<Entry> zeroed;  // moved into place once it is
    HIP_TRY(LBM_FAILURE, zeroed.alloc(bt->members.size()));
    HIP_TRY(LBM_FAILURE, hipMemset(zeroed, 0, bt->members.size() * sizeof(Entry)));
    table = std::move(zeroed);
  }
  HIP_TRY(LBM_FAILURE, hipMemcpy(table + index, &entry, sizeof(entry), hipMemcpyHostToDevice));
  return LBM_SUCCESS;
}
int write_batch_entry(lbm_ctx* c, int kind) {
  if (!c->batch) return LBM_SUCCESS;
  if (kind == kRecFrames) return set_batch_entry(c, c->batch->frame_table, frames_entry(c));
  if (kind == kRecProbes) return set_batch_entry(c, c->batch->probe_table, probes_entry(c));
  if (kind == kRecFields) return set_batch_entry(c, c->batch->field_table, fields_entry(c));
  return set_batch_entry(c, c->batch->mean_table, mean_entry(c));
}

// frees the record buffers of every slab and leaves the recorder off
void release_recorder(lbm_ctx* c) {
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    (void)hipSetDevice(sl.device);
    sl.frames.reset();
    sl.probe_ring.reset();
    sl.probe_table.reset();
    sl.mean_sums.reset();
    sl.field_ring.reset();
    sl.field_y0 = sl.field_ny = 0;
    sl.gather_ring.reset();
    sl.force_links.reset();
    sl.force_starts.reset();
    sl.force_groups = 0;
    sl.residual_planes.reset();
    sl.vort_edges.reset();
    sl.psi_totals.reset();
    sl.psi_cand.reset();
    sl.psi_in.reset();
    sl.psi_out.reset();
    sl.psi_band_rows = 0;
    sl.tracer_state.reset();
    sl.probe_count = 0;
  }
  c->probe_cells.clear();
  c->force_link_counts.clear();
  c->rec = Recorder{};
}

// What the setters of every kind (the gather kinds': arm_gather; for the mean fields: set_mean_order, behind lbm_set_mean and
// lbm_set_mean_order) share behind their own argument checks.  Arming (every > 0) is refused, with nothing touched,
// where this kind cannot record.  Then the launches in flight are awaited and a recorder of this kind is disarmed; to arm, allocate() provides the kind's buffers of every slab (and says what it could not) before the
// recorder's fields, the member's batch entry and the batch's count of armed members are set.
template <class Allocate>
int rearm_recorder(lbm_ctx* c, int kind, int every, int capacity, Allocate allocate, const char* who = nullptr) {
  const RecorderKind& k = kind_words(kind);
  const char* const setter = who ? who : k.setter;  // the kind's other setter (lbm_set_mean_order) speaks under its own name
  lbm_batch* bt = c->batch;
  if (every > 0) {
    if (c->halo_mode != LBM_HALO_SYNC)
      LBM_FAIL(LBM_FAILURE, "%s: the context runs the %s halo mode, where splitting a call at a %s would change the results "
               "(every call starts from freshly exchanged halos); %s need LBM_HALO_SYNC", setter,
               c->halo_mode == LBM_HALO_STALE ? "stale" : "freshest", k.record, k.noun);
    for (int other = kRecFrames; other < kRecKinds; other++) {  // every other kind
      if (other == kind) continue;
      const RecorderKind& o = kind_words(other);
      if (c->rec.kind == other)
        LBM_FAIL(LBM_FAILURE, "%s: %s are armed (%s) and a context has one recorder -- disarm them with %s first", setter, o.name,
                 o.setter, o.disarm);
      if (bt && bt->rec.kind == other)  // (a kind no member arms: the batch does)
        LBM_FAIL(LBM_FAILURE, "%s: this batch has %s armed (%s); a batch records one kind -- disarm them with %s first", setter, o.name,
                 gather_kind(other).batch_setter, gather_kind(other).batch_disarm);
      if (bt && bt->armed[other] > 0)
        LBM_FAIL(LBM_FAILURE, "%s: a member of this batch has %s armed (%s); a batch records one kind: frames, probes, mean fields or field frames",
                 setter, o.name, o.setter);
    }
    if (c->plan.resident && !is_gather(kind)) {  // (the gather kinds record behind the plain form, which every resident shape runs)
      // the recorder forms of four-row bands defer the acceleration of the interior pair only (lbm::resident_band): the lid
      // row (ny - 2) must be a band's row 2, which ny % 4 == 0 guarantees; and the form that will launch -- a batch member's
      // is the batched one, whose field-frame forms take a register or a scratch word more than their single twins
      // (profiles/resident_forms_resources.txt) -- must run one workgroup per CU
      if (c->plan.resident_rows == 4 && c->slab[0].accel_row % 4 != 2)
        LBM_FAIL(LBM_FAILURE, "%s: the lid row %d is not an interior row of a four-row band", setter, c->slab[0].accel_row);
      int per_cu = 0;
      HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[0].device));
      HIP_TRY(LBM_FAILURE, hipOccupancyMaxActiveBlocksPerMultiprocessor(
                               &per_cu, resident_kernel(c->p.nx, c->plan.resident_rows, c->plan.resident_joint, kind, bt != nullptr),
                               c->p.nx * c->plan.resident_group, 0));
      if (per_cu < 1) LBM_FAIL(LBM_FAILURE, "%s: the resident kernel's %s form does not fit a CU at this shape", setter, k.noun);
    }
  }
  // the buffers may still be written by launches in flight
  for (int s = 0; s < c->n_slabs; s++) {
    HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[s].device));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->slab[s].compute));
  }
  if (c->rec.kind == kind) {
    if (bt) bt->armed[kind]--;
    release_recorder(c);
    if (write_batch_entry(c, kind) != LBM_SUCCESS) return LBM_FAILURE;
  }
  if (every <= 0) return LBM_SUCCESS;
  if (allocate() != LBM_SUCCESS) {
    (void)hipGetLastError();  // a failed allocation must not surface at the next launch
    release_recorder(c);
    return LBM_FAILURE;
  }
  c->rec.kind = kind;
  c->rec.every = every;
  c->rec.slots = capacity;
  c->rec.ord0 = (int)(((long long)c->steps_done + every - 1) / every);
  if (write_batch_entry(c, kind) != LBM_SUCCESS) {
    release_recorder(c);
    return LBM_FAILURE;
  }
  if (bt) bt->armed[kind]++;
  return LBM_SUCCESS;
}

// What the readers of the slotted kinds share, a context's (drain_recorder) and a batch's (drain_batch_gather), once
// the work in flight has been awaited: without outputs the call tells how many records of `kind` wait in r; else copy(n)
// fetches the n oldest (at most max_records) before their steps are told and they are retired.
template <class Copy>
int drain_ring(Recorder& r, int kind, const char* reader, int max_records, bool has_out, int* steps, int* n_read, Copy copy) {
  const RecorderKind& k = kind_words(kind);
  if (r.kind == kind && r.slots == 0)
    LBM_FAIL(LBM_FAILURE, "%s: %s are armed without a ring (capacity 0): no %s is recorded", reader, k.name, k.record);
  const long long waiting = (r.kind == kind) ? r.written - r.read : 0;
  if (!has_out && !steps) {
    *n_read = (int)waiting;
    return LBM_SUCCESS;
  }
  if (!has_out) LBM_FAIL(LBM_FAILURE, "%s: NULL %s output", reader, k.record);
  if (max_records < 0) LBM_FAIL(LBM_FAILURE, "%s: negative max_%ss %d", reader, k.record, max_records);
  const int n = (waiting < max_records) ? (int)waiting : max_records;
  if (n > 0 && copy(n) != LBM_SUCCESS) return LBM_FAILURE;
  if (steps)
    for (int i = 0; i < n; i++) steps[i] = (int)((r.ord0 + r.read + i) * r.every);
  r.read += n;
  *n_read = n;
  return LBM_SUCCESS;
}
template <class Copy>
int drain_recorder(lbm_ctx* c, int kind, int max_records, bool has_out, int* steps, int* n_read, Copy copy) {
  const char* const reader = kind_words(kind).reader;
  if (!c || !n_read) LBM_FAIL(LBM_FAILURE, "%s: NULL argument", reader);
  *n_read = 0;
  REFUSE_FAILED(LBM_FAILURE, c, reader);
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  return drain_ring(c->rec, kind, reader, max_records, has_out, steps, n_read, copy);
}

// every slab's share of the n oldest records of a gather kind, gathered as records[record][slab's share]; *record_words:
// the words of one record, all shares.  The kind's rows hook merges the shares of a record.
int fetch_gather_records(lbm_ctx* c, int n, std::vector<long long>& records, size_t* record_words) {
  size_t share_at[kMaxSlabs + 1] = {0};  // where slab s's words start in a record's
  for (int s = 0; s < c->n_slabs; s++) share_at[s + 1] = share_at[s] + gather_slot_words(c, c->slab[s]);
  const size_t all = *record_words = share_at[c->n_slabs];
  records.resize((size_t)n * all);
  std::vector<long long> stage;
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    const size_t words = share_at[s + 1] - share_at[s];
    stage.resize((size_t)n * words);
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    if (fetch_ring(sl.gather_ring.get(), words, c->rec, n, sl.compute, stage.data()) != LBM_SUCCESS) return LBM_FAILURE;
    for (size_t i = 0; i < (size_t)n; i++) memcpy(&records[i * all + share_at[s]], &stage[i * words], words * sizeof(long long));
  }
  return LBM_SUCCESS;
}

// ---- the recorder of a batch: what the lbm_batch_set_* and lbm_batch_read_* share ------------------------------------
// what the batched kernels read of every member, [parity of cur][members]
std::vector<lbm::ResidentMember> member_table(const lbm_batch* bt) {
  const size_t n_members = bt->members.size();
  std::vector<lbm::ResidentMember> h(2 * n_members);
  for (int par = 0; par < 2; par++)
    for (size_t i = 0; i < n_members; i++) {
      const lbm_ctx* c = bt->members[i];
      const Slab& sl = c->slab[0];
      lbm::ResidentMember& m = h[(size_t)par * n_members + i];
      m.src = sl.lat[par];
      m.dst = sl.lat[par ^ 1];
      m.mask = sl.mask;
      m.gran = sl.res_gran;
      m.partials = sl.res_part;
      m.tot_u = sl.tot_u;
      m.omega = c->p.omega;
      set_accel_weights(m, c->p);  // as run_steps / run_resident
    }
  return h;
}
// ... on the device (the current one); false, with no table left behind, where that fails
bool upload_member_table(lbm_batch* bt) {
  const std::vector<lbm::ResidentMember> h = member_table(bt);
  if (bt->table.alloc(h.size()) == hipSuccess && hipMemcpy(bt->table, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice) == hipSuccess)
    return true;
  (void)hipGetLastError();
  bt->table.reset();
  return false;
}

// frees the batch's record buffers, whatever gather kind they served, and leaves its recorder off (release_recorder does
// so for a context)
void release_batch_recorder(lbm_batch* bt) {
  (void)hipSetDevice(bt->members[0]->slab[0].device);
  bt->gather_ring.reset();
  bt->residual_planes.reset();
  bt->psi_totals.reset();
  bt->psi_cand.reset();
  bt->psi_band_rows = 0;
  bt->tracer_state.reset();
  bt->force_lists.reset();
  bt->force_links.clear();
  bt->force_starts.clear();
  bt->force_link_counts.clear();
  bt->force_groups = 0;
  if (bt->rec.kind != kRecNone) bt->armed[bt->rec.kind] = 0;
  bt->rec = Recorder{};
}

// the batched gather kernels read the members' lattices from the member table: a batch of a shape the resident kernel
// does not take has none until a kind is first armed
int ensure_member_table(lbm_batch* bt, const char* who, const char* noun) {
  if (!bt->table && !upload_member_table(bt)) LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the member table; %s stay off", who, noun);
  return LBM_SUCCESS;
}

// a batch records one kind: no kind is armed on the batch while a member has its own recorder armed
int batch_members_free(const lbm_batch* bt, const char* who) {
  for (size_t i = 0; i < bt->members.size(); i++) {
    const Recorder& r = bt->members[i]->rec;
    if (r.kind != kRecNone)
      LBM_FAIL(LBM_FAILURE, "%s: member %d has %s armed (%s); a batch records one kind -- disarm them with %s first", who, (int)i,
               kind_words(r.kind).name, kind_words(r.kind).setter, kind_words(r.kind).disarm);
  }
  return LBM_SUCCESS;
}

// ---- obstacle forces: what lbm_set_forces (per slab) and lbm_batch_set_forces (per member) share ------------------
// the labels of a slab's owned cells (src: those of its first owned cell on) as bytes on its device, 255: outside
// 0 .. n_bodies - 1; *first_bad = the lowest blocked cell so marked, ~0u where there is none
constexpr unsigned kNoBadLabel = ~0u;
int upload_labels(lbm_ctx* c, Slab& sl, const int* src, int n_bodies, DeviceBuf<unsigned char>& labels, unsigned* first_bad) {
  const size_t n = (size_t)sl.rows * c->p.nx;
  std::vector<unsigned char> bytes(n);
  for (size_t i = 0; i < n; i++) bytes[i] = (src[i] < 0 || src[i] >= n_bodies) ? 255 : (unsigned char)src[i];
  HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
  DeviceBuf<unsigned> bad;
  *first_bad = kNoBadLabel;
  HIP_TRY(LBM_FAILURE, labels.alloc(n));
  HIP_TRY(LBM_FAILURE, bad.alloc(1));
  HIP_TRY(LBM_FAILURE, hipMemcpy(labels, bytes.data(), n, hipMemcpyHostToDevice));
  HIP_TRY(LBM_FAILURE, hipMemcpy(bad, first_bad, sizeof(*first_bad), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(lbm::label_check, dim3(ceil_div((long)n, 256)), dim3(256), 0, sl.compute, (const unsigned char*)sl.mask, c->pitch,
                     c->p.nx, (const unsigned char*)labels, (long)n, bad.get());
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(first_bad, bad, sizeof(*first_bad), hipMemcpyDeviceToHost, sl.compute));
  HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
  return LBM_SUCCESS;
}

// A slab's list of boundary links from its mask and the labels (nullptr: every blocked cell is body 0), on its device:
// links per (body, workgroup of cells), their prefix sums, then the links themselves at those offsets.  `starts` is the
// host's copy of starts_dev, [n_bodies + 1].
int build_link_list(const char* who, lbm_ctx* c, Slab& sl, const unsigned char* lab, int n_bodies, DeviceBuf<unsigned>& links,
                    DeviceBuf<unsigned>& starts_dev, std::vector<unsigned>& starts) {
  HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
  const long n = (long)sl.rows * c->p.nx;
  const int wgs = ceil_div(n, lbm::kLinkCells);
  const long m = (long)wgs * n_bodies;
  DeviceBuf<unsigned> counts;
  DeviceBuf<unsigned long long> total_dev;
  unsigned long long total = 0;
  starts.assign((size_t)n_bodies + 1, 0u);
  if (counts.alloc((size_t)m) != hipSuccess || total_dev.alloc(1) != hipSuccess || starts_dev.alloc(starts.size()) != hipSuccess)
    LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the link counts (%.1f MiB); forces stay off", who, (double)m * sizeof(unsigned) / 1048576.0);
  hipLaunchKernelGGL(lbm::link_count, dim3(wgs, n_bodies), dim3(lbm::kBlock), 0, sl.compute, (const unsigned char*)sl.mask, c->pitch,
                     c->p.nx, lab, n, counts.get());
  hipLaunchKernelGGL(lbm::link_scan, dim3(1), dim3(lbm::kBlock), 0, sl.compute, counts.get(), m, (long)wgs, starts_dev.get(),
                     total_dev.get());
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(&total, total_dev, sizeof(total), hipMemcpyDeviceToHost, sl.compute));
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(starts.data(), starts_dev, starts.size() * sizeof(unsigned), hipMemcpyDeviceToHost, sl.compute));
  HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
  if (total > 0x7fffffffull) LBM_FAIL(LBM_FAILURE, "%s: %llu boundary links in one slab, at most 2^31 - 1 are possible", who, total);
  if (links.alloc((size_t)(total ? total : 1)) != hipSuccess)
    LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the list of %llu boundary links (%.1f MiB); forces stay off", who, total,
             (double)total * sizeof(unsigned) / 1048576.0);
  if (total > 0) {
    hipLaunchKernelGGL(lbm::link_fill, dim3(wgs, n_bodies), dim3(lbm::kBlock), 0, sl.compute, (const unsigned char*)sl.mask, c->pitch,
                       c->p.nx, lab, n, (const unsigned*)counts.get(), links.get(), (unsigned)total);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
  }
  HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));  // counts (and the caller's labels) may be freed on return
  return LBM_SUCCESS;
}

// workgroups per body of force_gather / force_gather_batch where the largest body has `most` links: four links per lane
// where there are that many, at most 256 (0: no links at all)
int gather_groups(unsigned most) {
  const int groups = ceil_div((long)most, 4 * lbm::kBlock);
  return most == 0 ? 0 : (groups > 256 ? 256 : groups);
}

// n bodies' words of ring rows -> out[n][2]: each body's two exact sums rounded once and doubled (-2 c_k f)
void round_forces(const long long* words, size_t n, double* out) {
  constexpr int L = lbm_exact::kExactLimbs;
  for (size_t j = 0; j < n; j++) {
    const long long* w = words + j * lbm::kForceWords;
    long long fx[L], fy[L];
    for (int i = 0; i < L; i++) {
      fx[i] = w[i];
      fy[i] = w[L + i];
    }
    const bool finite = (w[2 * L] == 0);  // a population that is not finite makes the body's force of that row NaN
    out[2 * j] = finite ? 2.0 * lbm_exact::exact_sum_round(fx) : std::nan("");
    out[2 * j + 1] = finite ? 2.0 * lbm_exact::exact_sum_round(fy) : std::nan("");
  }
}


// ================================================================================================
// The gather kinds: each kind's hooks, the one table of them, and the drivers that arm and drain any kind
// ================================================================================================
// whose records a reader converts (lattice_words: the caller's, once the words are fetched)
GatherOwner context_owner(const lbm_ctx* c) {
  GatherOwner g;
  g.nx = c->p.nx;
  g.ny = c->p.ny;
  g.shares = c->n_slabs;
  for (int s = 0; s < c->n_slabs; s++) {
    g.row_first[s] = c->slab[s].row_first;
    g.row_count[s] = c->slab[s].rows;
  }
  return g;
}
GatherOwner members_owner(const lbm_batch* bt) {
  const lbm_ctx* c0 = bt->members[0];
  GatherOwner g;
  g.nx = c0->p.nx;
  g.ny = g.row_count[0] = c0->slab[0].rows;
  g.lattices = bt->members.size();
  return g;
}

// ---- one record of a batch (the forces': below) ------------------------------------------------------------------------
// the statistics: one stats_gather_batch for all members
int take_batch_stats(lbm_batch* bt, long long* row) {
  lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size();
  const Slab& sl0 = c0->slab[0];
  const int v = stats_vector(c0->p.nx);
  const dim3 grid((unsigned)stats_groups((long)sl0.rows * c0->p.nx, v), 1, (unsigned)n_members);
  const lbm::ResidentMember* tab = bt->table + (size_t)bt->cur * n_members;
  if (v == 4)
    hipLaunchKernelGGL(lbm::stats_gather_batch<4>, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows, row);
  else
    hipLaunchKernelGGL(lbm::stats_gather_batch<1>, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows, row);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}

// the enstrophy: one vorticity_gather_batch for all members, each a periodic slab of its own
int take_batch_enstrophy(lbm_batch* bt, long long* row) {
  lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size();
  const Slab& sl0 = c0->slab[0];
  const int nx = c0->p.nx, band_rows = vorticity_band_rows(sl0.rows, nx);
  const dim3 grid((unsigned)vorticity_groups(sl0.rows, nx, band_rows), 1, (unsigned)n_members);
  const lbm::ResidentMember* tab = bt->table + (size_t)bt->cur * n_members;
  hipLaunchKernelGGL(stats_vector(nx) == 4 ? lbm::vorticity_gather_batch<4> : lbm::vorticity_gather_batch<1>, grid, dim3(lbm::kBlock), 0,
                     bt->stream, lattice_args(c0, sl0), tab, sl0.rows, band_rows, row);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}

// the stress: one stress_gather_batch for all members
int take_batch_stress(lbm_batch* bt, long long* row) {
  lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size();
  const Slab& sl0 = c0->slab[0];
  const int v = stats_vector(c0->p.nx);
  const dim3 grid((unsigned)stats_groups((long)sl0.rows * c0->p.nx, v), 1, (unsigned)n_members);
  const lbm::ResidentMember* tab = bt->table + (size_t)bt->cur * n_members;
  hipLaunchKernelGGL(v == 4 ? lbm::stress_gather_batch<4> : lbm::stress_gather_batch<1>, grid, dim3(lbm::kBlock), 0, bt->stream,
                     lattice_args(c0, sl0), tab, sl0.rows, row);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}

// the stream function: ONE launch of each of the scan's kernels for all members (grid z is the member; psi_extrema: grid x),
// each member a grid of its own from row 0
int take_batch_psi(lbm_batch* bt, long long* row) {
  lbm_ctx* c0 = bt->members[0];
  const unsigned n_members = (unsigned)bt->members.size();
  const Slab& sl0 = c0->slab[0];
  const int nx = c0->p.nx, band_rows = bt->psi_band_rows, bands = ceil_div(sl0.rows, band_rows);
  const dim3 grid((unsigned)ceil_div(nx, lbm::kPsiColumns), (unsigned)bands, n_members);
  const lbm::ResidentMember* tab = bt->table + (size_t)bt->cur * n_members;
  hipLaunchKernelGGL(lbm::psi_band_totals_batch, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows, band_rows,
                     bt->psi_totals.get());
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  hipLaunchKernelGGL(lbm::psi_band_bases, dim3((unsigned)ceil_div(nx * lbm_exact::kExactLimbs, lbm::kBlock), 1, n_members), dim3(lbm::kBlock), 0, bt->stream, nx, bands,
                     bt->psi_totals.get(), (const long long*)nullptr, (long long*)nullptr);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  hipLaunchKernelGGL(lbm::psi_scan_batch, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows, band_rows,
                     (const long long*)bt->psi_totals, bt->psi_cand.get());
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  hipLaunchKernelGGL(lbm::psi_extrema, dim3(n_members), dim3(64), 0, bt->stream, (const lbm::PsiCandidate*)bt->psi_cand, (int)(grid.x * grid.y), row);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}

// ONE residual_gather_batch launch over all members' current (stored) lattices and planes, on the batch's stream:
// the baseline (`planes` filled, `row` unused) or a sample against `planes` into `row`, [members][kResidualWords], which
// the caller has zeroed in front
int launch_batch_residual(lbm_batch* bt, float* planes, long long* row, bool baseline) {
  lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size();
  const Slab& sl0 = c0->slab[0];
  const int v = stats_vector(c0->p.nx);
  const dim3 grid((unsigned)stats_groups((long)sl0.rows * c0->p.nx, v), 1, (unsigned)n_members);
  const lbm::ResidentMember* tab = bt->table + (size_t)bt->cur * n_members;
  HIP_TRY(LBM_FAILURE, hipSetDevice(sl0.device));
  if (v == 4)
    hipLaunchKernelGGL(lbm::residual_gather_batch<4>, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows,
                       planes, row, (int)baseline);
  else
    hipLaunchKernelGGL(lbm::residual_gather_batch<1>, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows,
                       planes, row, (int)baseline);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}

// the residuals: one sample launch against the members' remembered fields
int take_batch_residual(lbm_batch* bt, long long* row) { return launch_batch_residual(bt, bt->residual_planes, row, false); }

// the profiles: one launch per selected axis for all members
int take_batch_profiles(lbm_batch* bt, long long* record) {
  lbm_ctx* c0 = bt->members[0];
  const Slab& sl0 = c0->slab[0];
  const size_t n_members = bt->members.size();
  const int nx = c0->p.nx, axes = bt->rec.args.axes;
  const long member_words = (long)(gather_slot_words(bt) / n_members);
  const lbm::ResidentMember* tab = bt->table + (size_t)bt->cur * n_members;
  long long* lines = record;
  if (axes & LBM_PROFILE_ROWS) {
    const dim3 grid((unsigned)ceil_div(sl0.rows, lbm::kBlock / 64), 1, (unsigned)n_members);
    if (stats_vector(nx) == 4)
      hipLaunchKernelGGL(lbm::profile_rows_batch<4>, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows, lines, member_words);
    else
      hipLaunchKernelGGL(lbm::profile_rows_batch<1>, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows, lines, member_words);
    lines += (size_t)sl0.rows * lbm_profile::kProfileWords;
  }
  if (axes & LBM_PROFILE_COLUMNS) {
    const int band_rows = profile_band_rows(sl0.rows, nx);
    const dim3 grid((unsigned)ceil_div(nx, lbm::kProfileColumns), (unsigned)ceil_div(sl0.rows, band_rows), (unsigned)n_members);
    hipLaunchKernelGGL(lbm::profile_columns_batch, grid, dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, sl0), tab, sl0.rows, band_rows, lines,
                       member_words);
  }
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}

// one launch for all members; a member is one slab, so every box row is whole and leaves as lines
int take_batch_coarse(lbm_batch* bt, long long* frame) {
  lbm_ctx* c0 = bt->members[0];
  const Slab& sl0 = c0->slab[0];
  const size_t n_members = bt->members.size();
  const int bx = bt->rec.args.box_x;
  const lbm_coarse::SlabBoxRows g = coarse_slab_boxes(c0, sl0, bx, bt->rec.args.box_y);
  const int groups = coarse_groups(g);
  const long member_words = (long)lbm_coarse::slot_words(g);
  const lbm::ResidentMember* tab = bt->table + (size_t)bt->cur * n_members;
  const dim3 grid((unsigned)g.count * (unsigned)groups, 1, (unsigned)n_members);
  hipLaunchKernelGGL(coarse_wide(bx) ? lbm::coarse_gather_batch<true> : lbm::coarse_gather_batch<false>, grid, dim3(lbm::kBlock), 0, bt->stream,
                     lattice_args(c0, sl0), tab, g, groups, frame, member_words);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}

// ---- slot sizes ------------------------------------------------------------------------------------------------------
template <int Words>
size_t fixed_slot_words(const lbm_ctx*, const Slab&, const GatherArgs&) { return Words; }
size_t forces_slot_words(const lbm_ctx*, const Slab&, const GatherArgs& a) { return (size_t)a.bodies * lbm::kForceWords; }
// this slab's row lines, then its rows' share of every column line
size_t profiles_slot_words(const lbm_ctx* c, const Slab& sl, const GatherArgs& a) {
  return lbm_profile::profile_slab_lines(sl.rows, c->p.nx, a.axes) * lbm_profile::kProfileWords;
}
// the slab's whole box rows as lines, its partial ones as limb words
size_t coarse_frames_slot_words(const lbm_ctx* c, const Slab& sl, const GatherArgs& a) { return coarse_slot_words(c, sl, a.box_x, a.box_y); }

// ---- the kinds' own argument checks (no device needed) ---------------------------------------------------------------
// the forces speak of their ring in bodies, so they refuse it themselves (the drivers' check then finds nothing)
int check_forces(const char* who, const lbm_ctx* c, size_t members, int capacity, const GatherArgs& a) {
  if (a.bodies < 1 || a.bodies > LBM_MAX_BODIES)
    LBM_FAIL(LBM_FAILURE, "%s: %d bodies, between 1 and LBM_MAX_BODIES = %d are possible", who, a.bodies, LBM_MAX_BODIES);
  const int body_bytes = lbm::kForceWords * (int)sizeof(long long);
  const long long row_bytes = (long long)(members ? members : 1) * a.bodies * body_bytes;
  if ((long long)capacity * row_bytes >= (1LL << 31)) {
    if (!members)
      LBM_FAIL(LBM_FAILURE, "%s: a ring of %d rows of %d bodies is 2 GiB or more (%d bytes per body and row)", who, capacity, a.bodies, body_bytes);
    LBM_FAIL(LBM_FAILURE, "%s: a ring of %d rows of %d members of %d bodies is %.2f GiB, 2 GiB or more (%d bytes per body and row)", who,
             capacity, (int)members, a.bodies, (double)capacity * (double)row_bytes / 1073741824.0, body_bytes);
  }
  if (members && (size_t)c->p.nx * c->p.ny > ((size_t)1 << 29))
    LBM_FAIL(LBM_FAILURE, "%s: members of %d x %d cells; a link is cell * 8 + k - 1 in 32 bits (at most 2^29 cells)", who, c->p.nx, c->p.ny);
  return LBM_SUCCESS;
}
int check_profiles(const char* who, const lbm_ctx*, size_t, int, const GatherArgs& a) {
  if (a.axes < 1 || a.axes > (LBM_PROFILE_ROWS | LBM_PROFILE_COLUMNS))
    LBM_FAIL(LBM_FAILURE, "%s: axes %d, LBM_PROFILE_ROWS (1), LBM_PROFILE_COLUMNS (2) or both (3) are possible", who, a.axes);
  return LBM_SUCCESS;
}
// what every entry point refuses of a box
int coarse_box_ok(const char* who, const lbm_ctx* c, int bx, int by) {
  if (bx < 1 || by < 1) LBM_FAIL(LBM_FAILURE, "%s: box %d x %d, a box side is at least 1", who, bx, by);
  if (bx > c->p.nx) LBM_FAIL(LBM_FAILURE, "%s: box side bx %d is larger than the grid's nx %d", who, bx, c->p.nx);
  if (by > c->p.ny) LBM_FAIL(LBM_FAILURE, "%s: box side by %d is larger than the grid's ny %d", who, by, c->p.ny);
  if (bx > LBM_COARSE_MAX_BOX) LBM_FAIL(LBM_FAILURE, "%s: box side bx %d is larger than LBM_COARSE_MAX_BOX (%d)", who, bx, LBM_COARSE_MAX_BOX);
  if (by > LBM_COARSE_MAX_BOX) LBM_FAIL(LBM_FAILURE, "%s: box side by %d is larger than LBM_COARSE_MAX_BOX (%d)", who, by, LBM_COARSE_MAX_BOX);
  return LBM_SUCCESS;
}
int check_coarse_frames(const char* who, const lbm_ctx* c, size_t, int, const GatherArgs& a) { return coarse_box_ok(who, c, a.box_x, a.box_y); }

// ---- the kinds' buffers besides the ring -----------------------------------------------------------------------------
// the forces' own: every slab's (or member's) labels as bytes on its device while the lists are built; none: every
// blocked cell is body 0
using ForceLabels = std::vector<DeviceBuf<unsigned char>>;

// the links of one slab (or member) by body: its list on the device, the links of each body added to counts[bodies];
// *most: the largest body so far
int force_links_of(const char* who, lbm_ctx* c, Slab& sl, const unsigned char* labels, int n_bodies, DeviceBuf<unsigned>& links,
                   DeviceBuf<unsigned>& starts_dev, int* counts, unsigned* most) {
  std::vector<unsigned> starts;
  if (build_link_list(who, c, sl, labels, n_bodies, links, starts_dev, starts) != LBM_SUCCESS) return LBM_FAILURE;
  for (int b = 0; b < n_bodies; b++) {
    const unsigned n = starts[(size_t)b + 1] - starts[(size_t)b];
    counts[b] += (int)n;
    if (n > *most) *most = n;
  }
  return LBM_SUCCESS;
}
int alloc_forces_slab(const char* who, lbm_ctx* c, int s, const GatherArgs& a, const void* own) {
  const ForceLabels& labels = *static_cast<const ForceLabels*>(own);
  Slab& sl = c->slab[s];
  if (s == 0) c->force_link_counts.assign((size_t)a.bodies, 0);
  unsigned most = 0;
  if (force_links_of(who, c, sl, labels.empty() ? nullptr : labels[(size_t)s].get(), a.bodies, sl.force_links, sl.force_starts,
                     c->force_link_counts.data(), &most) != LBM_SUCCESS)
    return LBM_FAILURE;
  sl.force_groups = gather_groups(most);
  return LBM_SUCCESS;
}
int alloc_forces_batch(const char* who, lbm_batch* bt, const GatherArgs& a, const void* own) {
  const ForceLabels& labels = *static_cast<const ForceLabels*>(own);
  const size_t n_members = bt->members.size();
  if (bt->force_lists.alloc(n_members) != hipSuccess) return kNoRoom;
  bt->force_links.resize(n_members);
  bt->force_starts.resize(n_members);
  bt->force_link_counts.assign(n_members * (size_t)a.bodies, 0);
  std::vector<lbm::ForceMember> lists(n_members);
  unsigned most = 0;  // the x-extent suits the largest body of any member
  for (size_t i = 0; i < n_members; i++) {
    lbm_ctx* c = bt->members[i];
    if (force_links_of(who, c, c->slab[0], labels.empty() ? nullptr : labels[i].get(), a.bodies, bt->force_links[i], bt->force_starts[i],
                       &bt->force_link_counts[i * (size_t)a.bodies], &most) != LBM_SUCCESS)
      return LBM_FAILURE;
    lists[i] = {bt->force_links[i].get(), bt->force_starts[i].get()};
  }
  HIP_TRY(LBM_FAILURE, hipMemcpy(bt->force_lists, lists.data(), lists.size() * sizeof(lists[0]), hipMemcpyHostToDevice));
  bt->force_groups = gather_groups(most);
  return LBM_SUCCESS;
}

// the residuals: the remembered field, filled with the baseline, the field of the current lattice (the streams are idle:
// the arming waited for them)
int alloc_residual_slab(const char* who, lbm_ctx* c, int s, const GatherArgs&, const void*) {
  Slab& sl = c->slab[s];
  const size_t cells = (size_t)sl.rows * c->p.nx;
  if (sl.residual_planes.alloc(2 * cells) != hipSuccess)
    LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the remembered field of slab %d (%zu cells, %.1f MiB); residuals stay off", who, s, cells,
             (double)(2 * cells * sizeof(float)) / 1048576.0);
  launch_residual_gather(c, sl, sl.residual_planes, nullptr, true);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}
int alloc_residual_batch(const char* who, lbm_batch* bt, const GatherArgs&, const void*) {
  const lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size(), cells = (size_t)c0->slab[0].rows * c0->p.nx;
  if (bt->residual_planes.alloc(n_members * 2 * cells) != hipSuccess)
    LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the remembered fields of %d members (%zu cells each, %.1f MiB); residuals stay off", who,
             (int)n_members, cells, (double)(n_members * 2 * cells * sizeof(float)) / 1048576.0);
  return launch_batch_residual(bt, bt->residual_planes, nullptr, true);  // the baselines of all members: one launch
}

// the enstrophy on several slabs: where the neighbours' boundary rows are copied to
int alloc_enstrophy_slab(const char*, lbm_ctx* c, int s, const GatherArgs&, const void*) {
  return c->n_slabs > 1 && c->slab[s].vort_edges.alloc(2 * (size_t)c->row_pitch) != hipSuccess ? kNoRoom : LBM_SUCCESS;
}

// the stream function: the scan's scratch, and on several slabs what travels from slab to slab
int alloc_psi_slab(const char*, lbm_ctx* c, int s, const GatherArgs&, const void*) {
  Slab& sl = c->slab[s];
  const int nx = c->p.nx;
  const size_t base_words = (size_t)nx * lbm_exact::kExactLimbs;
  sl.psi_band_rows = psi_band_rows(c, sl.rows, nx);
  bool ok = sl.psi_totals.alloc(psi_total_words(sl.rows, nx, sl.psi_band_rows)) == hipSuccess &&
            sl.psi_cand.alloc(psi_candidates(sl.rows, nx, sl.psi_band_rows)) == hipSuccess;
  if (ok && c->n_slabs > 1) {
    ok = sl.psi_in.alloc(base_words) == hipSuccess && sl.psi_out.alloc(base_words) == hipSuccess;
    if (ok && !sl.ev_psi_out) ok = sl.ev_psi_out.create(hipEventDisableTiming) == hipSuccess;
    if (ok && !sl.ev_psi_taken) ok = sl.ev_psi_taken.create(hipEventDisableTiming) == hipSuccess;
  }
  return ok ? LBM_SUCCESS : kNoRoom;
}
int alloc_psi_batch(const char*, lbm_batch* bt, const GatherArgs&, const void*) {
  lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size();
  const int rows = c0->slab[0].rows, nx = c0->p.nx;
  bt->psi_band_rows = psi_band_rows(c0, rows, nx);
  return bt->psi_totals.alloc(n_members * psi_total_words(rows, nx, bt->psi_band_rows)) == hipSuccess &&
                 bt->psi_cand.alloc(n_members * psi_candidates(rows, nx, bt->psi_band_rows)) == hipSuccess
             ? LBM_SUCCESS
             : kNoRoom;
}

// ---- one record of a context -------------------------------------------------------------------------------------------
// the take of the kinds whose slabs record side by side: the kind's launch on every slab's compute stream, into the slab's
// zeroed slot
int take_per_slab(lbm_ctx* c) {
  const GatherKind& k = gather_kind(c->rec.kind);
  return for_slabs(c, [&](int s) -> int {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    bool ringless;
    long long* words = zeroed_slot(sl.gather_ring, gather_slot_words(c, sl), c->rec, sl.compute, &ringless);
    if ((!words && !ringless) || k.launch(c, s, words) != LBM_SUCCESS) return LBM_FAILURE;
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    return LBM_SUCCESS;
  });
}
int launch_forces(lbm_ctx* c, int s, long long* words) {
  const Slab& sl = c->slab[s];
  if (sl.force_groups > 0)  // a slab without links records the zeros
    hipLaunchKernelGGL(lbm::force_gather, dim3(sl.force_groups, (unsigned)c->rec.args.bodies), dim3(lbm::kBlock), 0, sl.compute,
                       lattice_args(c, sl), (const unsigned*)sl.force_links, (const unsigned*)sl.force_starts, words);
  return LBM_SUCCESS;
}
int launch_stats(lbm_ctx* c, int s, long long* words) {
  launch_stats_gather(c, c->slab[s], words);
  return LBM_SUCCESS;
}
int launch_residual(lbm_ctx* c, int s, long long* words) {
  launch_residual_gather(c, c->slab[s], c->slab[s].residual_planes, words, false);  // also replaces the slab's remembered field by this lattice's
  return LBM_SUCCESS;
}
int launch_profile_lines(lbm_ctx* c, int s, long long* words) {
  launch_profiles(c, c->slab[s], words);  // (profile_rows leaves a line's spare word as zeroed)
  return LBM_SUCCESS;
}
int launch_coarse_frame(lbm_ctx* c, int s, long long* words) {
  launch_coarse(c, c->slab[s], c->rec.args.box_x, c->rec.args.box_y, words);
  return LBM_SUCCESS;
}
// the enstrophy: on several slabs the sample reads the neighbours' boundary rows, so the slabs mark theirs as written in
// front of the launches and await the neighbours' use of them behind
int launch_enstrophy(lbm_ctx* c, int s, long long* words) {
  Slab& sl = c->slab[s];
  const bool edges = c->n_slabs > 1;
  if (edges && copy_vorticity_edges(c, s, sl.vort_edges) != LBM_SUCCESS) return LBM_FAILURE;
  launch_vorticity_gather(c, sl, edges ? sl.vort_edges.get() : nullptr, 0, sl.rows, nullptr, words);
  if (edges) HIP_TRY(LBM_FAILURE, hipEventRecord(sl.ev_vort_done, sl.compute));
  return LBM_SUCCESS;
}
int take_enstrophy(lbm_ctx* c) {
  if (c->n_slabs == 1) return take_per_slab(c);
  if (mark_vorticity_ready(c) != LBM_SUCCESS || take_per_slab(c) != LBM_SUCCESS) return LBM_FAILURE;
  return await_vorticity_done(c);
}
int launch_stress(lbm_ctx* c, int s, long long* words) {
  launch_stress_gather(c, c->slab[s], 0, c->slab[s].rows, nullptr, words);
  return LBM_SUCCESS;
}
// (the stream function's slabs depend on each other: take_psi_record issues them in their order)

// ---- one record of a batch: the members' current (stored) lattices into `row`, the record's slot, which lbm_batch_run
// has zeroed for all members at once, on the batch's stream (the current device's) ------------------------------------
// the forces: one force_gather_batch for all members
int take_batch_forces(lbm_batch* bt, long long* row) {
  lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size();
  if (bt->force_groups > 0) {
    hipLaunchKernelGGL(lbm::force_gather_batch, dim3((unsigned)bt->force_groups, (unsigned)bt->rec.args.bodies, (unsigned)n_members),
                       dim3(lbm::kBlock), 0, bt->stream, lattice_args(c0, c0->slab[0]),
                       (const lbm::ResidentMember*)(bt->table + (size_t)bt->cur * n_members), (const lbm::ForceMember*)bt->force_lists, row);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
  }
  return LBM_SUCCESS;
}

// ---- the fetched words of n records into the caller's rows -------------------------------------------------------------
// the kinds whose row is `from` of a lattice's shares, merged and rounded
template <class Row, Row (*from)(const long long*, int, int)>
void rows_merged(const GatherOwner& g, const Recorder&, int n, const long long* words, void* out) {
  for (size_t j = 0; j < (size_t)n * g.lattices; j++) static_cast<Row*>(out)[j] = from(words + j * g.lattice_words, g.shares, g.nx);
}
// the span of the row with ordinal `ord` since arming: from the baseline to the first sample, then `every`
int residual_span(const Recorder& r, long long ord) {
  return ord == 0 ? (int)((long long)r.ord0 * r.every + 1 - r.args.base_steps) : r.every;
}
void residual_rows(const GatherOwner& g, const Recorder& r, int n, const long long* words, void* out) {
  for (size_t j = 0; j < (size_t)n * g.lattices; j++)
    static_cast<lbm_residual_row*>(out)[j] = lbm_residual::residual_row_from_words(words + j * g.lattice_words, g.shares, g.nx,
                                                                                   residual_span(r, r.read + (long long)(j / g.lattices)));
}
// every share's words of a lattice's row, added word by word -- integers: the order of the slabs does not matter -- then
// each body's two sums rounded once and doubled (-2 c_k f)
void forces_rows(const GatherOwner& g, const Recorder& r, int n, const long long* words, void* out) {
  const size_t bodies = (size_t)r.args.bodies, share = g.lattice_words / (size_t)g.shares;
  std::vector<long long> sum(share);
  for (size_t j = 0; j < (size_t)n * g.lattices; j++) {
    const long long* w = words + j * g.lattice_words;
    sum.assign(w, w + share);
    for (int s = 1; s < g.shares; s++)
      for (size_t i = 0; i < share; i++) sum[i] += w[(size_t)s * share + i];
    round_forces(sum.data(), bodies, static_cast<double*>(out) + j * 2 * bodies);
  }
}
void profiles_rows(const GatherOwner& g, const Recorder& r, int n, const long long* words, void* out) {
  const size_t lines = lbm_profile::profile_slab_lines(g.ny, g.nx, r.args.axes);
  for (size_t j = 0; j < (size_t)n * g.lattices; j++)
    lbm_profile::profile_lines_from_words(words + j * g.lattice_words, g.shares, g.row_first, g.row_count, g.nx, g.ny, r.args.axes,
                                          static_cast<lbm_profile_line*>(out) + j * lines);
}
void coarse_frames_rows(const GatherOwner& g, const Recorder& r, int n, const long long* words, void* out) {
  const int bx = r.args.box_x, by = r.args.box_y;
  const size_t boxes = (size_t)lbm_coarse::coarse_boxes(g.nx, bx) * lbm_coarse::coarse_boxes(g.ny, by);
  for (size_t j = 0; j < (size_t)n * g.lattices; j++)
    lbm_coarse::coarse_frame_from_words(words + j * g.lattice_words, g.shares, g.row_first, g.row_count, g.nx, g.ny, bx, by,
                                        static_cast<lbm_profile_line*>(out) + j * boxes);
}

// ---- tracer particles: the one kind with state between its samples -------------------------------------------------------
size_t tracers_slot_words(const lbm_ctx*, const Slab&, const GatherArgs& a) { return 2 * (size_t)a.tracers; }  // a position: two doubles
int check_tracers(const char* who, const lbm_ctx* c, size_t, int, const GatherArgs& a) {
  if (a.tracers < 1 || a.tracers > LBM_MAX_TRACERS)
    LBM_FAIL(LBM_FAILURE, "%s: %d tracers, between 0 (none: disarms) and LBM_MAX_TRACERS = %d are possible", who, a.tracers, LBM_MAX_TRACERS);
  if (c->n_slabs > 1)
    LBM_FAIL(LBM_FAILURE, "%s: the context has %d slabs; a tracer's four cells can straddle two slabs, and a slab's lattice halo rows are "
             "not current after a pass: tracers need a context of one slab", who, c->n_slabs);
  return LBM_SUCCESS;
}
// what the setters refuse of the start positions, `lattices` x n of them, once nothing else is refused
int tracer_starts_ok(const char* who, const lbm_ctx* c, size_t lattices, int n, const lbm_tracer* start) {
  if (!start) LBM_FAIL(LBM_FAILURE, "%s: NULL start positions", who);
  for (size_t i = 0; i < lattices * (size_t)n; i++) {
    const lbm_tracer& t = start[i];
    if (std::isfinite(t.x) && std::isfinite(t.y) && t.x >= 0.0 && t.x < (double)c->p.nx && t.y >= 0.0 && t.y < (double)c->p.ny) continue;
    char of[32] = "";
    if (lattices > 1) snprintf(of, sizeof(of), " of member %d", (int)(i / (size_t)n));
    LBM_FAIL(LBM_FAILURE, "%s: tracer %d%s starts at (%g, %g), not a finite position with 0 <= x < %d and 0 <= y < %d", who, (int)(i % (size_t)n),
             of, t.x, t.y, c->p.nx, c->p.ny);
  }
  return LBM_SUCCESS;
}
// the positions, set to the caller's start (own)
int alloc_tracers_slab(const char* who, lbm_ctx* c, int s, const GatherArgs& a, const void* own) {
  Slab& sl = c->slab[s];
  if (sl.tracer_state.alloc((size_t)a.tracers) != hipSuccess)
    LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the positions of %d tracers (%.1f MiB); tracers stay off", who, a.tracers,
             (double)a.tracers * sizeof(lbm_tracer) / 1048576.0);
  HIP_TRY(LBM_FAILURE, hipMemcpy(sl.tracer_state, own, (size_t)a.tracers * sizeof(lbm_tracer), hipMemcpyHostToDevice));
  return LBM_SUCCESS;
}
int alloc_tracers_batch(const char* who, lbm_batch* bt, const GatherArgs& a, const void* own) {
  const size_t all = bt->members.size() * (size_t)a.tracers;
  if (bt->tracer_state.alloc(all) != hipSuccess)
    LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the positions of %d members' %d tracers (%.1f MiB); tracers stay off", who, (int)bt->members.size(),
             a.tracers, (double)all * sizeof(lbm_tracer) / 1048576.0);
  HIP_TRY(LBM_FAILURE, hipMemcpy(bt->tracer_state, own, all * sizeof(lbm_tracer), hipMemcpyHostToDevice));
  return LBM_SUCCESS;
}
// one advance of all tracers over the span that ends at this sample (residual_span: the record about to be written), the
// row into `words` (null: armed without a ring)
int launch_tracers(lbm_ctx* c, int s, long long* words) {
  const Slab& sl = c->slab[s];
  const int n = c->rec.args.tracers;
  hipLaunchKernelGGL(lbm::tracer_advance, dim3(ceil_div(n, lbm::kBlock)), dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl), c->p.ny, n,
                     residual_span(c->rec, c->rec.written), reinterpret_cast<double2*>(sl.tracer_state.get()), reinterpret_cast<double2*>(words));
  return LBM_SUCCESS;
}
int take_batch_tracers(lbm_batch* bt, long long* row) {
  lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size();
  const int n = bt->rec.args.tracers;
  hipLaunchKernelGGL(lbm::tracer_advance_batch, dim3(ceil_div(n, lbm::kBlock), 1, (unsigned)n_members), dim3(lbm::kBlock), 0, bt->stream,
                     lattice_args(c0, c0->slab[0]), (const lbm::ResidentMember*)(bt->table + (size_t)bt->cur * n_members), c0->p.ny, n,
                     residual_span(bt->rec, bt->rec.written), reinterpret_cast<double2*>(bt->tracer_state.get()), reinterpret_cast<double2*>(row));
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}
// a row's words are its doubles
void tracers_rows(const GatherOwner& g, const Recorder&, int n, const long long* words, void* out) {
  memcpy(out, words, (size_t)n * g.lattices * g.lattice_words * sizeof(long long));
}

// ---- the table ---------------------------------------------------------------------------------------------------------
// To add a gather kind: its number in front of kRecKinds, its entry here, its hooks above, and its entry points, which pack
// their arguments into GatherArgs and call arm_gather / drain_gather (arm_batch_gather / drain_batch_gather).
const GatherKind kGatherKinds[kRecKinds - kRecGatherFirst] = {
    {.ctx = {.name = "obstacle forces", .noun = "forces", .record = "row", .setter = "lbm_set_forces", .reader = "lbm_read_forces",
             .disarm = "lbm_set_forces(ctx, 0, NULL, 0, 0)"},
     .batch_setter = "lbm_batch_set_forces", .batch_reader = "lbm_batch_read_forces", .batch_disarm = "lbm_batch_set_forces(batch, 0, NULL, 0, 0)",
     .stays_off = "forces stay off", .spread = "a body's links", .of_a_batch = "the forces of a batch are", .of = " of %d bodies",
     .slot_words = forces_slot_words, .check = check_forces, .alloc_slab = alloc_forces_slab, .alloc_batch = alloc_forces_batch,
     .take = take_per_slab, .launch = launch_forces, .take_batch = take_batch_forces, .rows = forces_rows},
    {.ctx = {.name = "lattice statistics", .noun = "statistics", .record = "row", .setter = "lbm_set_stats", .reader = "lbm_read_stats",
             .disarm = "lbm_set_stats(ctx, 0, 0)"},
     .batch_setter = "lbm_batch_set_stats", .batch_reader = "lbm_batch_read_stats", .batch_disarm = "lbm_batch_set_stats(batch, 0, 0)",
     .stays_off = "statistics stay off", .spread = "a row's sums", .of_a_batch = "the statistics of a batch are",
     .slot_words = fixed_slot_words<lbm_stats::kStatsWords>,
     .take = take_per_slab, .launch = launch_stats, .take_batch = take_batch_stats,
     .rows = rows_merged<lbm_stats_row, lbm_stats::stats_row_from_words>},
    {.ctx = {.name = "velocity residuals", .noun = "residuals", .record = "row", .setter = "lbm_set_residual", .reader = "lbm_read_residual",
             .disarm = "lbm_set_residual(ctx, 0, 0)"},
     .batch_setter = "lbm_batch_set_residual", .batch_reader = "lbm_batch_read_residual", .batch_disarm = "lbm_batch_set_residual(batch, 0, 0)",
     .stays_off = "residuals stay off", .spread = "a row's sums", .of_a_batch = "the residuals of a batch are",
     .slot_words = fixed_slot_words<lbm_residual::kResidualWords>, .alloc_slab = alloc_residual_slab, .alloc_batch = alloc_residual_batch,
     .take = take_per_slab, .launch = launch_residual, .take_batch = take_batch_residual, .rows = residual_rows},
    {.ctx = {.name = "line profiles", .noun = "profiles", .record = "record", .setter = "lbm_set_profiles", .reader = "lbm_read_profiles",
             .disarm = "lbm_set_profiles(ctx, 0, 0, 0)"},
     .batch_setter = "lbm_batch_set_profiles", .batch_reader = "lbm_batch_read_profiles", .batch_disarm = "lbm_batch_set_profiles(batch, 0, 0, 0)",
     .stays_off = "profiles stay off", .spread = "a column's sums", .of_a_batch = "the profiles of a batch are", .per_slab = true,
     .slot_words = profiles_slot_words, .check = check_profiles,
     .take = take_per_slab, .launch = launch_profile_lines, .take_batch = take_batch_profiles, .rows = profiles_rows},
    {.ctx = {.name = "enstrophy rows", .noun = "enstrophy", .record = "row", .setter = "lbm_set_enstrophy", .reader = "lbm_read_enstrophy",
             .disarm = "lbm_set_enstrophy(ctx, 0, 0)"},
     .batch_setter = "lbm_batch_set_enstrophy", .batch_reader = "lbm_batch_read_enstrophy", .batch_disarm = "lbm_batch_set_enstrophy(batch, 0, 0)",
     .stays_off = "the enstrophy stays off", .spread = "a row's sums", .of_a_batch = "the enstrophy of a batch is",
     .slot_words = fixed_slot_words<lbm_enstrophy::kEnstrophyWords>, .alloc_slab = alloc_enstrophy_slab,
     .take = take_enstrophy, .launch = launch_enstrophy, .take_batch = take_batch_enstrophy,
     .rows = rows_merged<lbm_enstrophy_row, lbm_enstrophy::enstrophy_row_from_words>},
    {.ctx = {.name = "stream function rows", .noun = "the stream function", .record = "row", .setter = "lbm_set_psi",
             .reader = "lbm_read_psi_rows", .disarm = "lbm_set_psi(ctx, 0, 0)"},
     .batch_setter = "lbm_batch_set_psi", .batch_reader = "lbm_batch_read_psi_rows", .batch_disarm = "lbm_batch_set_psi(batch, 0, 0)",
     .stays_off = "the stream function stays off", .spread = "a column's prefix", .of_a_batch = "the stream function of a batch is",
     .also = " and the scan's buffers",
     .slot_words = fixed_slot_words<lbm_psi::kPsiWords>, .alloc_slab = alloc_psi_slab, .alloc_batch = alloc_psi_batch,
     .take = take_psi_record, .take_batch = take_batch_psi, .rows = rows_merged<lbm_psi_row, lbm_psi::psi_row_from_words>},
    {.ctx = {.name = "coarse frames", .noun = "coarse frames", .record = "frame", .setter = "lbm_set_coarse_frames",
             .reader = "lbm_read_coarse_frames", .disarm = "lbm_set_coarse_frames(ctx, 0, 0, 0, 0)"},
     .batch_setter = "lbm_batch_set_coarse_frames", .batch_reader = "lbm_batch_read_coarse_frames",
     .batch_disarm = "lbm_batch_set_coarse_frames(batch, 0, 0, 0, 0)",
     .stays_off = "coarse frames stay off", .spread = "a box's cells", .of_a_batch = "the coarse frames of a batch are", .per_slab = true,
     .slot_words = coarse_frames_slot_words, .check = check_coarse_frames,
     .take = take_per_slab, .launch = launch_coarse_frame, .take_batch = take_batch_coarse, .rows = coarse_frames_rows},
    {.ctx = {.name = "stress rows", .noun = "the stress", .record = "row", .setter = "lbm_set_stress", .reader = "lbm_read_stress_rows",
             .disarm = "lbm_set_stress(ctx, 0, 0)"},
     .batch_setter = "lbm_batch_set_stress", .batch_reader = "lbm_batch_read_stress_rows", .batch_disarm = "lbm_batch_set_stress(batch, 0, 0)",
     .stays_off = "the stress stays off", .spread = "a row's sums", .of_a_batch = "the stress of a batch is",
     .slot_words = fixed_slot_words<lbm_stress::kStressWords>,
     .take = take_per_slab, .launch = launch_stress, .take_batch = take_batch_stress,
     .rows = rows_merged<lbm_stress_row, lbm_stress::stress_row_from_words>},
    {.ctx = {.name = "tracer particles", .noun = "tracers", .record = "row", .setter = "lbm_set_tracers", .reader = "lbm_read_tracers",
             .disarm = "lbm_set_tracers(ctx, 0, NULL, 0, 0)"},
     .batch_setter = "lbm_batch_set_tracers", .batch_reader = "lbm_batch_read_tracers", .batch_disarm = "lbm_batch_set_tracers(batch, 0, NULL, 0, 0)",
     .stays_off = "tracers stay off", .spread = "a tracer's cells", .of_a_batch = "the tracers of a batch are", .ringless = true,
     .slot_words = tracers_slot_words, .check = check_tracers, .alloc_slab = alloc_tracers_slab, .alloc_batch = alloc_tracers_batch,
     .take = take_per_slab, .launch = launch_tracers, .take_batch = take_batch_tracers, .rows = tracers_rows}};
const GatherKind& gather_kind(int kind) { return kGatherKinds[kind - kRecGatherFirst]; }
const RecorderKind& kind_words(int kind) { return is_gather(kind) ? gather_kind(kind).ctx : kRecorderKinds[kind]; }

// ---- arming a context --------------------------------------------------------------------------------------------------
// " of 3 bodies" for the forces, nothing for every other kind
struct OfWhat {
  char text[32];
  OfWhat(const GatherKind& k, const GatherArgs& a) { snprintf(text, sizeof(text), k.of, a.bodies); }
};

// What every lbm_set_<gather kind> refuses of its arguments and of the context, in this order, with nothing touched
int gather_refusals(lbm_ctx* c, int kind, int every, int capacity, const GatherArgs& a) {
  const GatherKind& k = gather_kind(kind);
  const char* const who = k.ctx.setter;
  if (!c) LBM_FAIL(LBM_FAILURE, "%s: null context", who);
  REFUSE_FAILED(LBM_FAILURE, c, who);
  if (every < 0) LBM_FAIL(LBM_FAILURE, "%s: negative interval %d", who, every);
  if (every == 0) return LBM_SUCCESS;
  if (k.ringless && capacity < 0) LBM_FAIL(LBM_FAILURE, "%s: negative capacity %d (0: no ring)", who, capacity);
  if (!k.ringless && capacity < 1) LBM_FAIL(LBM_FAILURE, "%s: capacity %d, at least one %s is needed", who, capacity, k.ctx.record);
  if (k.check && k.check(who, c, 0, capacity, a) != LBM_SUCCESS) return LBM_FAILURE;
  for (int s = 0; s < c->n_slabs; s++) {
    const long long slot_bytes = (long long)(k.slot_words(c, c->slab[s], a) * sizeof(long long));
    if ((long long)capacity * slot_bytes >= (1LL << 31))
      LBM_FAIL(LBM_FAILURE, "%s: a ring of %d %ss is 2 GiB or more (%lld bytes per %s%s)", who, capacity, k.ctx.record, slot_bytes, k.ctx.record,
               k.per_slab ? " and slab" : "");
  }
  if (c->ranked || c->world > 1)
    LBM_FAIL(LBM_FAILURE, "%s: not available in a multi-process (rank) context: %s would be spread over the ranks", who, k.spread);
  if (c->batch)
    LBM_FAIL(LBM_FAILURE, "%s: not available on a member of a batch (lbm_create_batch): the batched launches need common sample steps to "
             "end at, so %s armed on the batch, with one `every` for all members (%s)", who, k.of_a_batch, k.batch_setter);
  return LBM_SUCCESS;
}
// ... and what it does once nothing is refused: rearm_recorder with every slab's ring and the kind's buffers behind it
int arm_gather_checked(lbm_ctx* c, int kind, int every, int capacity, GatherArgs a, const void* own = nullptr) {
  const GatherKind& k = gather_kind(kind);
  const char* const who = k.ctx.setter;
  const int status = rearm_recorder(c, kind, every, capacity, [&]() -> int {
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      const size_t ring_bytes = (size_t)capacity * k.slot_words(c, sl, a) * sizeof(long long);
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      int rc = ring_bytes && sl.gather_ring.alloc_bytes(ring_bytes) != hipSuccess ? kNoRoom : k.alloc_slab ? k.alloc_slab(who, c, s, a, own) : LBM_SUCCESS;
      if (rc == kNoRoom) {
        char where[32] = "per slab";
        if (k.per_slab) snprintf(where, sizeof(where), "for slab %d", s);
        LBM_FAIL(LBM_FAILURE, "%s: cannot allocate %d %ss%s (%.1f MiB %s)%s; %s", who, capacity, k.ctx.record, OfWhat(k, a).text,
                 (double)ring_bytes / 1048576.0, where, k.also, k.stays_off);
      }
      if (rc != LBM_SUCCESS) return LBM_FAILURE;
    }
    return LBM_SUCCESS;
  });
  if (status == LBM_SUCCESS && every > 0) {
    a.base_steps = c->steps_done;
    c->rec.args = a;
  }
  return status;
}
int arm_gather(lbm_ctx* c, int kind, int every, int capacity, const GatherArgs& a) {
  return gather_refusals(c, kind, every, capacity, a) != LBM_SUCCESS ? LBM_FAILURE : arm_gather_checked(c, kind, every, capacity, a);
}

// What the readers of the gather kinds share behind drain_recorder: the slabs' shares of the records, then the kind's rows
int drain_gather(lbm_ctx* c, int kind, int max_records, void* out, int* steps, int* n_read) {
  return drain_recorder(c, kind, max_records, out != nullptr, steps, n_read, [&](int n) -> int {
    std::vector<long long> records;  // [record][slab's share]
    GatherOwner g = context_owner(c);
    if (fetch_gather_records(c, n, records, &g.lattice_words) != LBM_SUCCESS) return LBM_FAILURE;
    gather_kind(kind).rows(g, c->rec, n, records.data(), out);
    return LBM_SUCCESS;
  });
}

// ---- arming a batch ----------------------------------------------------------------------------------------------------
// What every lbm_batch_set_<gather kind> refuses, in this order, with nothing touched (gather_refusals does so for a
// context).  Disarming while the batch's one recorder holds another kind is let through: arm_batch_gather_checked does
// nothing then.
int batch_gather_refusals(lbm_batch* bt, int kind, int every, int capacity, const GatherArgs& a) {
  const GatherKind& k = gather_kind(kind);
  const char* const who = k.batch_setter;
  if (!bt) LBM_FAIL(LBM_FAILURE, "%s: null batch", who);
  REFUSE_FAILED(LBM_FAILURE, bt, who);
  if (every < 0) LBM_FAIL(LBM_FAILURE, "%s: negative interval %d", who, every);
  if (every == 0) return LBM_SUCCESS;
  if (bt->rec.kind != kRecNone && bt->rec.kind != kind) {
    const GatherKind& o = gather_kind(bt->rec.kind);
    LBM_FAIL(LBM_FAILURE, "%s: this batch has %s armed (%s); a batch records one kind -- disarm them with %s first", who, o.ctx.name,
             o.batch_setter, o.batch_disarm);
  }
  const lbm_ctx* c0 = bt->members[0];
  const size_t n_members = bt->members.size();
  if (k.ringless && capacity < 0) LBM_FAIL(LBM_FAILURE, "%s: negative capacity %d (0: no ring)", who, capacity);
  if (!k.ringless && capacity < 1) LBM_FAIL(LBM_FAILURE, "%s: capacity %d, at least one %s is needed", who, capacity, k.ctx.record);
  if (k.check && k.check(who, c0, n_members, capacity, a) != LBM_SUCCESS) return LBM_FAILURE;
  const size_t member_bytes = k.slot_words(c0, c0->slab[0], a) * sizeof(long long), record_bytes = n_members * member_bytes;
  if ((long long)capacity * (long long)record_bytes >= (1LL << 31))
    LBM_FAIL(LBM_FAILURE, "%s: a ring of %d %ss of %d members is %.2f GiB, 2 GiB or more (%zu bytes per member and %s)", who, capacity,
             k.ctx.record, (int)n_members, (double)capacity * (double)record_bytes / 1073741824.0, member_bytes, k.ctx.record);
  return batch_members_free(bt, who);
}
// ... and what it does once nothing is refused (arm_gather_checked does so for a context): the launches in flight are
// awaited and a recorder of this kind is released; to arm, the ring of all members and the kind's buffers behind it are
// allocated before the recorder's fields are set
int arm_batch_gather_checked(lbm_batch* bt, int kind, int every, int capacity, GatherArgs a, const void* own = nullptr) {
  const GatherKind& k = gather_kind(kind);
  const char* const who = k.batch_setter;
  if (bt->rec.kind != kRecNone && bt->rec.kind != kind) return LBM_SUCCESS;  // (a disarming: a silent no-op)
  // the buffers may still be written by launches in flight
  HIP_TRY(LBM_FAILURE, hipSetDevice(bt->members[0]->slab[0].device));
  HIP_TRY(LBM_FAILURE, hipStreamSynchronize(bt->stream));
  release_batch_recorder(bt);
  if (every == 0) return LBM_SUCCESS;
  const auto allocate = [&]() -> int {
    const lbm_ctx* c0 = bt->members[0];
    const size_t n_members = bt->members.size();
    const size_t ring_bytes = (size_t)capacity * n_members * k.slot_words(c0, c0->slab[0], a) * sizeof(long long);
    const int rc = ring_bytes && bt->gather_ring.alloc_bytes(ring_bytes) != hipSuccess ? kNoRoom : k.alloc_batch ? k.alloc_batch(who, bt, a, own) : LBM_SUCCESS;
    if (rc == kNoRoom)
      LBM_FAIL(LBM_FAILURE, "%s: cannot allocate %d %ss of %d members%s (%.1f MiB)%s; %s", who, capacity, k.ctx.record, (int)n_members,
               OfWhat(k, a).text, (double)ring_bytes / 1048576.0, k.also, k.stays_off);
    return rc;
  };
  if (ensure_member_table(bt, who, k.ctx.noun) != LBM_SUCCESS || allocate() != LBM_SUCCESS) {
    (void)hipGetLastError();  // a failed allocation must not surface at the next launch
    release_batch_recorder(bt);
    return LBM_FAILURE;
  }
  bt->rec.kind = kind;
  bt->rec.every = every;
  bt->rec.slots = capacity;
  bt->rec.ord0 = (int)(((long long)bt->steps_done + every - 1) / every);
  a.base_steps = bt->steps_done;
  bt->rec.args = a;
  bt->armed[kind] = 1;
  return LBM_SUCCESS;
}
int arm_batch_gather(lbm_batch* bt, int kind, int every, int capacity, const GatherArgs& a) {
  return batch_gather_refusals(bt, kind, every, capacity, a) != LBM_SUCCESS ? LBM_FAILURE : arm_batch_gather_checked(bt, kind, every, capacity, a);
}

// What the lbm_batch_read_* share (drain_gather does so for a context): the words of the n oldest records,
// [record][member][a member's words], then the kind's rows
int drain_batch_gather(lbm_batch* bt, int kind, int max_records, void* out, int* steps, int* n_read) {
  const char* const reader = gather_kind(kind).batch_reader;
  if (!bt || !n_read) LBM_FAIL(LBM_FAILURE, "%s: NULL argument", reader);
  *n_read = 0;
  REFUSE_FAILED(LBM_FAILURE, bt, reader);
  if (lbm_batch_sync(bt) != LBM_SUCCESS) return LBM_FAILURE;
  return drain_ring(bt->rec, kind, reader, max_records, out != nullptr, steps, n_read, [&](int n) -> int {
    const size_t words = gather_slot_words(bt);
    std::vector<long long> stage((size_t)n * words);
    HIP_TRY(LBM_FAILURE, hipSetDevice(bt->members[0]->slab[0].device));
    if (fetch_ring(bt->gather_ring.get(), words, bt->rec, n, bt->stream, stage.data()) != LBM_SUCCESS) return LBM_FAILURE;
    GatherOwner g = members_owner(bt);
    g.lattice_words = words / g.lattices;
    gather_kind(kind).rows(g, bt->rec, n, stage.data(), out);
    return LBM_SUCCESS;
  });
}

}  // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

void lbm_set_error_mode(int mode) { g_error_mode = (mode == LBM_ERRORS_RETURN) ? LBM_ERRORS_RETURN : LBM_ERRORS_DIE; }
const char* lbm_last_error(void) { return g_last_error; }
const char* lbm_version(void) { return "lbm_hip 0.1 gfx950"; }

int lbm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int lbm_partition_rows(int ny, int parts, int index, int* first, int* count) {
  if (parts < 1 || index < 0 || index >= parts || ny < 1)
    LBM_FAIL(LBM_FAILURE, "lbm_partition_rows: bad arguments (ny=%d parts=%d index=%d)", ny, parts, index);
  const int base = ny / parts, rem = ny % parts;
  const int cnt = base + (index < rem ? 1 : 0);
  const int fst = index * base + (index < rem ? index : rem);
  if (parts > 1 && base < 2)  // some part (not necessarily this one) would be too thin
    LBM_FAIL(LBM_FAILURE, "lbm_partition_rows: %d rows over %d parts leaves a part with fewer than 2 rows", ny, parts);
  if (first) *first = fst;
  if (count) *count = cnt;
  return LBM_SUCCESS;
}

int lbm_halo_plan(int rows, int parts, int index, int depth, lbm_halo_op out[4]) {
  if (!out || rows < 1 || parts < 1 || index < 0 || index >= parts || depth < 1 || depth > rows)
    LBM_FAIL(LBM_FAILURE, "lbm_halo_plan: bad arguments (rows=%d parts=%d index=%d depth=%d)", rows, parts, index, depth);
  // ring with periodic wrap (MPI/d2q9-bgk.c:210-211): north = the part above, south = the part below
  const int north = (index + 1) % parts, south = (index - 1 + parts) % parts;
  out[0] = {1, north, rows - depth, depth};  // my top rows     -> north's rows [-depth, 0)
  out[1] = {1, south, 0, depth};             // my bottom rows  -> south's rows [rows_s, rows_s + depth)
  out[2] = {0, south, -depth, depth};        // my south halo  <-  south's top rows
  out[3] = {0, north, rows, depth};          // my north halo  <-  north's bottom rows
  return LBM_SUCCESS;
}

int lbm_plan_halo_depth(const lbm_params* params, int parts, int math_mode) {
  if (!validate_params(params) || parts < 1 || (math_mode != LBM_MATH_EXACT && math_mode != LBM_MATH_FAST))
    LBM_FAIL(0, "lbm_plan_halo_depth: bad arguments");
  PlanInput in;  // `parts` ranks of one slab each
  in.nx = params->nx;
  in.ny = params->ny;
  in.world = parts;
  in.halo = HALO_RCCL;
  const KernelPlan pl = lbm_plan::plan_kernels(in);
  return pl.fuse2 ? pl.pass_steps : 1;
}

lbm_ctx* lbm_create(const lbm_params* params, const int* obstacles, const float* cells_aos,
                    int n_gpus, int math_mode) {
  const ObstacleSource obst = {OBST_GLOBAL, obstacles, 0, 0, false};
  return create_common(params, obst, cells_aos, n_gpus, math_mode, 0, 1, nullptr, 0);
}

lbm_ctx* lbm_create_tiled(const lbm_params* params, const int* tile, int tile_nx, int tile_ny,
                          const float* cells_aos, int n_gpus, int math_mode) {
  const ObstacleSource obst = {OBST_TILE, tile, tile_nx, tile_ny, false};
  return create_common(params, obst, cells_aos, n_gpus, math_mode, 0, 1, nullptr, 0);
}

int lbm_rccl_unique_id(void* id_out) {
  if (!id_out) LBM_FAIL(LBM_FAILURE, "lbm_rccl_unique_id: NULL output");
  static_assert(sizeof(ncclUniqueId) == LBM_RCCL_ID_BYTES, "RCCL unique id size");
  ncclUniqueId id;
  RCCL_OR_FAIL(LBM_FAILURE);
  NCCL_TRY(LBM_FAILURE, rc_api_->GetUniqueId(&id));
  memcpy(id_out, &id, sizeof(id));
  return LBM_SUCCESS;
}

int lbm_rccl_info(const lbm_ctx* c, lbm_rccl_status* out) {
  if (!out) LBM_FAIL(LBM_FAILURE, "lbm_rccl_info: NULL output");
  memset(out, 0, sizeof(*out));
  // without a context: bind the library (as the first multi-GPU create would) and describe it; with one: describe
  // what the context uses, binding nothing on behalf of a context that never needed RCCL
  RcclApi* nc = nullptr;
  if (!c) {
    nc = rccl();
    if (!nc) LBM_FAIL(LBM_FAILURE, "RCCL is not available: %s", g_rccl_error);
  } else {
    for (int s = 0; s < c->n_slabs; s++) if (c->slab[s].nccl) out->n_comms++;
    if (out->n_comms > 0) nc = rccl();
  }
  if (!nc) return LBM_SUCCESS;
  out->loaded = 1;
  strncpy(out->library, nc->path, sizeof(out->library) - 1);
  NCCL_TRY(LBM_FAILURE, nc->GetVersion(&out->version));
  if (c && out->n_comms > 0) {
    for (int s = 0; s < c->n_slabs; s++)
      if (c->slab[s].nccl) {
        NCCL_TRY(LBM_FAILURE, nc->CommCount(c->slab[s].nccl, &out->nranks));
        NCCL_TRY(LBM_FAILURE, nc->CommUserRank(c->slab[s].nccl, &out->rank));
        break;
      }
  }
  return LBM_SUCCESS;
}

static bool rank_args_ok(int rank, int world_size, const void* unique_id) {
  if (world_size < 1 || rank < 0 || rank >= world_size) {
    raise_error(__LINE__, "lbm_create_rank: bad rank %d of %d", rank, world_size);
    return false;
  }
  if (!unique_id) {
    raise_error(__LINE__, "lbm_create_rank: unique_id is NULL");
    return false;
  }
  return true;
}

lbm_ctx* lbm_create_rank(const lbm_params* params, const int* obstacles, const float* cells_aos,
                         int rank, int world_size, const void* unique_id, int device, int math_mode) {
  if (!rank_args_ok(rank, world_size, unique_id)) return nullptr;
  const ObstacleSource obst = {OBST_GLOBAL, obstacles, 0, 0, false};
  return create_common(params, obst, cells_aos, 1, math_mode, rank, world_size, unique_id, device);
}

lbm_ctx* lbm_create_rank_rows(const lbm_params* params, const int* obstacle_rows, const float* cells_rows_aos,
                              int rank, int world_size, const void* unique_id, int device, int math_mode) {
  if (!rank_args_ok(rank, world_size, unique_id)) return nullptr;
  const ObstacleSource obst = {OBST_ROWS, obstacle_rows, 0, 0, true};
  return create_common(params, obst, cells_rows_aos, 1, math_mode, rank, world_size, unique_id, device);
}

static bool hosted_args_ok(int rank, int world_size, const lbm_host_comm* comm) {
  if (world_size < 1 || rank < 0 || rank >= world_size) {
    raise_error(__LINE__, "lbm_create_rank_hosted: bad rank %d of %d", rank, world_size);
    return false;
  }
  if (!comm || !comm->exchange || !comm->allreduce_sum) {
    raise_error(__LINE__, "lbm_create_rank_hosted: the exchange and all-reduce callbacks are required");
    return false;
  }
  return true;
}

lbm_ctx* lbm_create_rank_hosted(const lbm_params* params, const int* obstacles, const float* cells_aos,
                                int rank, int world_size, const lbm_host_comm* comm, int device, int math_mode) {
  if (!hosted_args_ok(rank, world_size, comm)) return nullptr;
  const ObstacleSource obst = {OBST_GLOBAL, obstacles, 0, 0, false};
  return create_common(params, obst, cells_aos, 1, math_mode, rank, world_size, nullptr, device, comm);
}

lbm_ctx* lbm_create_rank_hosted_rows(const lbm_params* params, const int* obstacle_rows, const float* cells_rows_aos,
                                     int rank, int world_size, const lbm_host_comm* comm, int device, int math_mode) {
  if (!hosted_args_ok(rank, world_size, comm)) return nullptr;
  const ObstacleSource obst = {OBST_ROWS, obstacle_rows, 0, 0, true};
  return create_common(params, obst, cells_rows_aos, 1, math_mode, rank, world_size, nullptr, device, comm);
}

lbm_ctx* lbm_create_rank_hosted_tiled(const lbm_params* params, const int* tile, int tile_nx, int tile_ny,
                                      int rank, int world_size, const lbm_host_comm* comm, int device, int math_mode) {
  if (!hosted_args_ok(rank, world_size, comm)) return nullptr;
  const ObstacleSource obst = {OBST_TILE, tile, tile_nx, tile_ny, false};
  return create_common(params, obst, nullptr, 1, math_mode, rank, world_size, nullptr, device, comm);
}

lbm_ctx* lbm_create_rank_tiled(const lbm_params* params, const int* tile, int tile_nx, int tile_ny,
                               int rank, int world_size, const void* unique_id, int device, int math_mode) {
  if (!rank_args_ok(rank, world_size, unique_id)) return nullptr;
  const ObstacleSource obst = {OBST_TILE, tile, tile_nx, tile_ny, false};
  return create_common(params, obst, nullptr, 1, math_mode, rank, world_size, unique_id, device);
}

void lbm_destroy(lbm_ctx* c) {
  if (!c || c->batch) return;  // a batch member belongs to its batch (lbm_destroy_batch)
  if (c->team) {
    c->team->shutdown();
    delete c->team;
    c->team = nullptr;
  }
  for (int s = 0; s < c->n_slabs; s++) {
    if (c->slab[s].compute) {
      (void)hipSetDevice(c->slab[s].device);
      (void)hipStreamSynchronize(c->slab[s].compute);
      (void)hipStreamSynchronize(c->slab[s].comm);
      for (hipStream_t g : c->slab[s].group_extra) if (g) (void)hipStreamSynchronize(g);
    }
  }
  delete c;  // what the context and its slabs own goes with them (~Slab)
}

int lbm_get_info(const lbm_ctx* c, lbm_info* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_get_info: NULL argument");
  out->n_slabs = c->n_slabs;
  out->row_first = c->row_first;
  out->row_count = c->row_count;
  out->fluid_cells = c->fluid_cells;
  out->steps_done = c->steps_done;
  out->math_mode = c->math_mode;
  out->world_rank = c->rank;
  out->world_size = c->world;
  const bool stale = (c->halo != HALO_SELF && c->halo_mode != LBM_HALO_SYNC);
  out->steps_per_launch = (c->plan.tile_steps && c->halo == HALO_SELF) ? c->plan.tile_steps : ((c->plan.fuse2 && !stale) ? c->plan.pass_steps : 1);
  out->halo_mode = c->halo_mode;
  const bool stream_kernel = c->plan.fuse2 && !stale && !(c->plan.tile_steps && c->halo == HALO_SELF);
  out->band_rows = stream_kernel ? c->plan.band_rows : 0;
  out->lane_cells = stream_kernel ? c->plan.lane_cells : 0;
  out->nontemporal = c->plan.nts;
  {
    int adv = 1;
    const int passes = chunk_passes(c, &adv);
    out->graph_steps = (c->plan.use_graph && !stale) ? passes * adv : 0;
  }
  out->resident_steps = c->plan.resident ? kResidentChunk : 0;
  out->resident_min_steps = c->plan.resident ? c->plan.resident_min_steps : 0;
  out->resident_rows = c->plan.resident ? c->plan.resident_rows : 0;
  out->resident_group = c->plan.resident ? c->plan.resident_group : 0;
  out->resident_one_xcd = c->plan.resident ? c->plan.resident_one_xcd : 0;
  out->band_groups = stream_kernel ? c->plan.band_groups : 1;
  return LBM_SUCCESS;
}

int lbm_set_halo_mode(lbm_ctx* c, int mode) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_set_halo_mode: null context");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_set_halo_mode");
  if (mode != LBM_HALO_SYNC && mode != LBM_HALO_STALE && mode != LBM_HALO_FRESHEST) LBM_FAIL(LBM_FAILURE, "lbm_set_halo_mode: unknown mode %d", mode);
  if (mode == LBM_HALO_FRESHEST && c->halo == HALO_HOST) LBM_FAIL(LBM_FAILURE, "lbm_set_halo_mode: the freshest-available mode is not available with the hosted exchange");
  if (mode != LBM_HALO_SYNC && c->rec.kind != kRecNone) {
    const RecorderKind& k = kind_words(c->rec.kind);
    LBM_FAIL(LBM_FAILURE, "lbm_set_halo_mode: %s are armed (%s); the stale and freshest halo modes cannot record them -- "
             "disarm with %s first", k.name, k.setter, k.disarm);
  }
  c->halo_mode = mode;
  return LBM_SUCCESS;
}

int lbm_set_frames(lbm_ctx* c, int every, int capacity) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_set_frames: null context");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_set_frames");
  if (every < 0) LBM_FAIL(LBM_FAILURE, "lbm_set_frames: negative interval %d", every);
  if (every > 0 && capacity < 1) LBM_FAIL(LBM_FAILURE, "lbm_set_frames: capacity %d, at least one frame slot is needed", capacity);
  return rearm_recorder(c, kRecFrames, every, capacity, [&]() -> int {
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      const size_t bytes = (size_t)capacity * (size_t)sl.rows * (size_t)c->p.nx * sizeof(float);
      if (sl.frames.alloc_bytes(bytes) != hipSuccess)
        LBM_FAIL(LBM_FAILURE, "lbm_set_frames: cannot allocate %d frame slots (%.1f MiB per slab); frames stay off", capacity,
                 (double)bytes / 1048576.0);
    }
    return LBM_SUCCESS;
  });
}

int lbm_read_frames(lbm_ctx* c, int max_frames, float* out, int* steps, int* n_read) {
  return drain_recorder(c, kRecFrames, max_frames, out != nullptr, steps, n_read, [&](int n) -> int {
    const size_t frame_cells = (size_t)c->row_count * c->p.nx;
    for (int i = 0; i < n; i++) {
      const size_t slot = (size_t)((c->rec.read + i) % c->rec.slots);
      for (int s = 0; s < c->n_slabs; s++) {
        Slab& sl = c->slab[s];
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        const size_t cells = (size_t)sl.rows * c->p.nx;
        HIP_TRY(LBM_FAILURE, hipMemcpyAsync(out + i * frame_cells + (size_t)(sl.row_first - c->row_first) * c->p.nx,
                                            sl.frames + slot * cells, cells * sizeof(float), hipMemcpyDeviceToHost, sl.compute));
      }
    }
    for (int s = 0; s < c->n_slabs; s++) {
      HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[s].device));
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->slab[s].compute));
    }
    return LBM_SUCCESS;
  });
}

int lbm_set_probes(lbm_ctx* c, int n_probes, const lbm_probe* cells, int every, int capacity) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_set_probes: null context");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_set_probes");
  if (n_probes < 0 || n_probes > LBM_MAX_PROBES)
    LBM_FAIL(LBM_FAILURE, "lbm_set_probes: %d probes, between 0 and LBM_MAX_PROBES = %d are possible", n_probes, LBM_MAX_PROBES);
  if (every < 0) LBM_FAIL(LBM_FAILURE, "lbm_set_probes: negative interval %d", every);
  const bool arm = n_probes > 0 && every > 0;
  if (arm) {
    if (!cells) LBM_FAIL(LBM_FAILURE, "lbm_set_probes: NULL cells");
    if (capacity < 1) LBM_FAIL(LBM_FAILURE, "lbm_set_probes: capacity %d, at least one row of samples is needed", capacity);
    if ((long long)capacity * n_probes * (long long)sizeof(lbm_probe_sample) >= (1LL << 31))
      LBM_FAIL(LBM_FAILURE, "lbm_set_probes: a ring of %d rows of %d samples is 2 GiB or more", capacity, n_probes);
    for (int i = 0; i < n_probes; i++)
      if (cells[i].x < 0 || cells[i].x >= c->p.nx || cells[i].y < 0 || cells[i].y >= c->p.ny)
        LBM_FAIL(LBM_FAILURE, "lbm_set_probes: probe %d is the cell (%d, %d), outside the %d x %d grid", i, cells[i].x, cells[i].y,
                 c->p.nx, c->p.ny);
    if (c->ranked || c->world > 1)
      LBM_FAIL(LBM_FAILURE, "lbm_set_probes: not available in a multi-process (rank) context: a row of samples would be spread over the ranks");
  }
  return rearm_recorder(c, kRecProbes, arm ? every : 0, capacity, [&]() -> int {
    const size_t ring_bytes = (size_t)capacity * (size_t)n_probes * sizeof(lbm::probe_vec);
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      // this slab's probes sorted by row (stable: ties keep the caller's order), then, where the resident kernel runs, the
      // word of every band: first entry | entries << 12 | (a probe on the lid row) << 31
      std::vector<int> mine;
      for (int i = 0; i < n_probes; i++)
        if (cells[i].y >= sl.row_first && cells[i].y < sl.row_first + sl.rows) mine.push_back(i);
      std::stable_sort(mine.begin(), mine.end(), [&](int p, int q) { return cells[p].y < cells[q].y; });
      const int bands = c->plan.resident ? c->plan.resident_bands : 0;
      std::vector<unsigned> words(2 * mine.size() + (size_t)bands, 0u);
      for (size_t j = 0; j < mine.size(); j++) {
        const int row = cells[mine[j]].y - sl.row_first;
        words[2 * j] = (unsigned)row;
        words[2 * j + 1] = (unsigned)cells[mine[j]].x | ((unsigned)mine[j] << 20);
        if (bands) {
          unsigned& w = words[2 * mine.size() + (size_t)(row / c->plan.resident_rows)];
          if (((w >> 12) & 0xfffu) == 0) w |= (unsigned)j;
          w += 1u << 12;
          if (row == sl.accel_row) w |= 1u << 31;
        }
      }
      static_assert(sizeof(lbm::ProbeEntry) == 2 * sizeof(unsigned), "a table entry is two words");
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      if (sl.probe_ring.alloc_bytes(ring_bytes) != hipSuccess ||
          sl.probe_table.alloc_bytes((words.size() + 2) * sizeof(unsigned)) != hipSuccess ||
          hipMemset(sl.probe_ring, 0, ring_bytes) != hipSuccess ||
          (!words.empty() && hipMemcpy(sl.probe_table, words.data(), words.size() * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess))
        LBM_FAIL(LBM_FAILURE, "lbm_set_probes: cannot allocate %d rows of %d samples (%.1f MiB per slab); probes stay off", capacity,
                 n_probes, (double)ring_bytes / 1048576.0);
      sl.probe_count = (int)mine.size();
    }
    c->probe_cells.assign(cells, cells + n_probes);
    return LBM_SUCCESS;
  });
}

int lbm_read_probes(lbm_ctx* c, int max_samples, lbm_probe_sample* out, int* steps, int* n_read) {
  return drain_recorder(c, kRecProbes, max_samples, out != nullptr, steps, n_read, [&](int n) -> int {
    const size_t np = c->probe_cells.size();
    // (a sample is one 16-byte store.)  One slab: straight into out, several: each slab's columns of a staged copy
    std::vector<lbm_probe_sample> stage(c->n_slabs > 1 ? (size_t)n * np : 0);
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      if (sl.probe_count == 0 && c->n_slabs > 1) continue;
      lbm_probe_sample* dst = c->n_slabs > 1 ? stage.data() : out;
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      if (fetch_ring(sl.probe_ring.get(), np, c->rec, n, sl.compute, dst) != LBM_SUCCESS) return LBM_FAILURE;
      if (c->n_slabs > 1)
        for (size_t p = 0; p < np; p++) {
          const int y = c->probe_cells[p].y;
          if (y < sl.row_first || y >= sl.row_first + sl.rows) continue;
          for (int i = 0; i < n; i++) out[(size_t)i * np + p] = stage[(size_t)i * np + p];
        }
    }
    return LBM_SUCCESS;
  });
}

// what lbm_set_mean and lbm_set_mean_order share: `who` names the caller, order 1 arms four planes, order 2 eight
static int set_mean_order(lbm_ctx* c, int every, int order, const char* who) {
  if (!c) LBM_FAIL(LBM_FAILURE, "%s: null context", who);
  REFUSE_FAILED(LBM_FAILURE, c, who);
  if (every < 0) LBM_FAIL(LBM_FAILURE, "%s: negative interval %d", who, every);
  if (order != 1 && order != 2) LBM_FAIL(LBM_FAILURE, "%s: order %d, the mean fields have order 1 (sums) or 2 (sums and sums of products)", who, order);
  if (every > 0 && (c->ranked || c->world > 1))
    LBM_FAIL(LBM_FAILURE, "%s: not available in a multi-process (rank) context", who);
  // (re-)arming starts from zero sums and a zero count: the planes are cleared on each slab's compute stream, behind the
  // quiesce of rearm_recorder and in front of whatever the next call enqueues there.  The resident kernel has one MEAN
  // form for both orders (the order is a run-time scalar), so rearm_recorder's fit check is made against the form that runs.
  const int planes = 4 * order;
  const int rc = rearm_recorder(c, kRecMean, every, 0, [&]() -> int {
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      const size_t bytes = (size_t)planes * sizeof(double) * (size_t)sl.rows * (size_t)c->p.nx;
      if (sl.mean_sums.alloc_bytes(bytes) != hipSuccess || hipMemsetAsync(sl.mean_sums, 0, bytes, sl.compute) != hipSuccess)
        LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the %s planes of sums (%d bytes per cell, %.1f MiB per slab); the mean fields stay off",
                 who, planes == 4 ? "four" : "eight", planes * 8, (double)bytes / 1048576.0);
    }
    c->rec.order = order;  // read by mean_entry when rearm_recorder writes the member's batch entry
    return LBM_SUCCESS;
  }, who);
  return rc;
}

int lbm_set_mean(lbm_ctx* c, int every) { return set_mean_order(c, every, 1, "lbm_set_mean"); }

int lbm_set_mean_order(lbm_ctx* c, int every, int order) {
  return set_mean_order(c, every, order, "lbm_set_mean_order");
}

int lbm_set_field_frames(lbm_ctx* c, int every, int capacity, int fields, const lbm_window* window) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_set_field_frames: null context");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_set_field_frames");
  if (every < 0) LBM_FAIL(LBM_FAILURE, "lbm_set_field_frames: negative interval %d", every);
  lbm_window w = {0, 0, c->p.nx, c->p.ny};
  if (every > 0) {
    if (capacity < 1) LBM_FAIL(LBM_FAILURE, "lbm_set_field_frames: capacity %d, at least one frame slot is needed", capacity);
    if (fields == 0 || (fields & ~LBM_FIELD_ALL) != 0)
      LBM_FAIL(LBM_FAILURE, "lbm_set_field_frames: fields 0x%x, a non-empty set of LBM_FIELD_* bits (within 0x%x) is needed", (unsigned)fields,
               (unsigned)LBM_FIELD_ALL);
    if (window) w = *window;
    if (w.nx < 1 || w.ny < 1)
      LBM_FAIL(LBM_FAILURE, "lbm_set_field_frames: a window of %d x %d cells, at least 1 x 1 is needed", w.nx, w.ny);
    if (w.x0 < 0 || w.y0 < 0 || w.x0 > c->p.nx - w.nx || w.y0 > c->p.ny - w.ny)
      LBM_FAIL(LBM_FAILURE, "lbm_set_field_frames: the window [%d, %lld) x [%d, %lld) leaves the %d x %d grid (windows do not wrap)", w.x0,
               (long long)w.x0 + w.nx, w.y0, (long long)w.y0 + w.ny, c->p.nx, c->p.ny);
    if (c->ranked || c->world > 1)
      LBM_FAIL(LBM_FAILURE, "lbm_set_field_frames: not available in a multi-process (rank) context: a frame would be spread over the ranks");
  }
  const size_t planes = (size_t)__builtin_popcount((unsigned)fields);
  return rearm_recorder(c, kRecFields, every, capacity, [&]() -> int {
    for (int s = 0; s < c->n_slabs; s++) {
      Slab& sl = c->slab[s];
      // this slab's rows of the window
      const int lo = (w.y0 > sl.row_first) ? w.y0 : sl.row_first;
      const int hi = (w.y0 + w.ny < sl.row_first + sl.rows) ? w.y0 + w.ny : sl.row_first + sl.rows;
      if (hi <= lo) continue;  // the window misses this slab: nothing to allocate, nothing to record
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      const size_t slot_bytes = planes * (size_t)(hi - lo) * (size_t)w.nx * sizeof(float);
      // (a slot is one buffer of the resident kernel's, 32-bit offsets; the ring's size is computed without overflow)
      if (slot_bytes > ((size_t)-1) / (size_t)capacity || sl.field_ring.alloc_bytes((size_t)capacity * slot_bytes) != hipSuccess)
        LBM_FAIL(LBM_FAILURE, "lbm_set_field_frames: cannot allocate %d frame slots of %d fields x %d x %d cells (%.1f MiB per slab); field frames stay off",
                 capacity, (int)planes, hi - lo, w.nx, (double)capacity * (double)slot_bytes / 1048576.0);
      sl.field_y0 = lo - sl.row_first;
      sl.field_ny = hi - lo;
    }
    c->rec.fields = fields;  // read by fields_entry when rearm_recorder writes the member's batch entry
    c->rec.window = w;
    return LBM_SUCCESS;
  });
}

int lbm_read_field_frames(lbm_ctx* c, int max_frames, float* out, int* steps, int* n_read) {
  return drain_recorder(c, kRecFields, max_frames, out != nullptr, steps, n_read, [&](int n) -> int {
    const lbm_window& w = c->rec.window;
    const size_t planes = (size_t)__builtin_popcount((unsigned)c->rec.fields);
    const size_t plane_cells = (size_t)w.ny * w.nx, frame_cells = planes * plane_cells;
    for (int i = 0; i < n; i++) {
      const size_t slot = (size_t)((c->rec.read + i) % c->rec.slots);
      for (int s = 0; s < c->n_slabs; s++) {
        Slab& sl = c->slab[s];
        if (sl.field_ny == 0) continue;
        HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
        // a slab's slot is float[F][field_ny][window nx]: its rows of every plane go to their place in the frame (one
        // copy where the slab holds the whole window)
        const size_t cells = (size_t)sl.field_ny * w.nx;
        const size_t row_off = (size_t)(sl.row_first + sl.field_y0 - w.y0) * w.nx;
        const float* src = sl.field_ring + slot * planes * cells;
        if (sl.field_ny == w.ny) {
          HIP_TRY(LBM_FAILURE, hipMemcpyAsync(out + i * frame_cells, src, frame_cells * sizeof(float), hipMemcpyDeviceToHost, sl.compute));
        } else {
          for (size_t j = 0; j < planes; j++)
            HIP_TRY(LBM_FAILURE, hipMemcpyAsync(out + i * frame_cells + j * plane_cells + row_off, src + j * cells, cells * sizeof(float),
                                                hipMemcpyDeviceToHost, sl.compute));
        }
      }
    }
    for (int s = 0; s < c->n_slabs; s++) {
      HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[s].device));
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->slab[s].compute));
    }
    return LBM_SUCCESS;
  });
}

int lbm_set_forces(lbm_ctx* c, int n_bodies, const int* body_of_cell, int every, int capacity) {
  GatherArgs a;
  a.bodies = n_bodies;
  if (gather_refusals(c, kRecForces, every, capacity, a) != LBM_SUCCESS) return LBM_FAILURE;
  ForceLabels labels((size_t)(every > 0 && body_of_cell ? c->n_slabs : 0));
  if (every > 0) {
    for (int s = 0; s < c->n_slabs; s++)
      if ((long)c->slab[s].rows * c->p.nx > (1L << 29))
        LBM_FAIL(LBM_FAILURE, "lbm_set_forces: a slab of %d x %d cells; a link is cell * 8 + k - 1 in 32 bits (at most 2^29 cells per slab)",
                 c->p.nx, c->slab[s].rows);
    for (size_t s = 0; s < labels.size(); s++) {
      Slab& sl = c->slab[s];
      const int* src = body_of_cell + (size_t)(sl.row_first - c->row_first) * c->p.nx;
      unsigned first_bad;
      if (upload_labels(c, sl, src, n_bodies, labels[s], &first_bad) != LBM_SUCCESS) return LBM_FAILURE;
      if (first_bad != kNoBadLabel)
        LBM_FAIL(LBM_FAILURE, "lbm_set_forces: the blocked cell (%d, %d) has body %d, outside 0 .. %d", (int)(first_bad % (unsigned)c->p.nx),
                 sl.row_first + (int)(first_bad / (unsigned)c->p.nx), src[first_bad], n_bodies - 1);
    }
  }
  return arm_gather_checked(c, kRecForces, every, capacity, a, &labels);
}

int lbm_read_forces(lbm_ctx* c, int max_rows, double* out, int* steps, int* n_read) {
  return drain_gather(c, kRecForces, max_rows, out, steps, n_read);
}

int lbm_forces_links(lbm_ctx* c, int* links_per_body) {
  if (!c || !links_per_body) LBM_FAIL(LBM_FAILURE, "lbm_forces_links: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_forces_links");
  if (c->rec.kind != kRecForces) LBM_FAIL(LBM_FAILURE, "lbm_forces_links: the obstacle forces are not armed (lbm_set_forces)");
  for (size_t b = 0; b < c->force_link_counts.size(); b++) links_per_body[b] = c->force_link_counts[b];
  return LBM_SUCCESS;
}

int lbm_set_stats(lbm_ctx* c, int every, int capacity) { return arm_gather(c, kRecStats, every, capacity, GatherArgs{}); }

int lbm_read_stats(lbm_ctx* c, int max_rows, lbm_stats_row* out, int* steps, int* n_read) {
  return drain_gather(c, kRecStats, max_rows, out, steps, n_read);
}

// ---- vorticity and enstrophy -------------------------------------------------------------------------------------------
int lbm_set_enstrophy(lbm_ctx* c, int every, int capacity) { return arm_gather(c, kRecEnstrophy, every, capacity, GatherArgs{}); }

int lbm_read_enstrophy(lbm_ctx* c, int max_rows, lbm_enstrophy_row* out, int* steps, int* n_read) {
  return drain_gather(c, kRecEnstrophy, max_rows, out, steps, n_read);
}

int lbm_read_vorticity(lbm_ctx* c, float* w) {
  if (!c || !w) LBM_FAIL(LBM_FAILURE, "lbm_read_vorticity: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_vorticity");
  if (c->ranked || c->world > 1)
    LBM_FAIL(LBM_FAILURE, "lbm_read_vorticity: not available in a multi-process (rank) context: the rows around this rank's belong to other processes");
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  const int nx = c->p.nx;
  long chunk_rows = (16L << 20) / ((long)nx * sizeof(float));
  if (chunk_rows < 1) chunk_rows = 1;
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    DeviceBuf<float> stage, edges;  // the call's own: nothing armed is touched
    HIP_TRY(LBM_FAILURE, stage.alloc((size_t)chunk_rows * nx));
    if (c->n_slabs > 1) {
      // every stream is idle (lbm_sync): the neighbours' boundary rows are copied in stream order, no events needed
      const Slab& ss = c->slab[(s - 1 + c->n_slabs) % c->n_slabs];
      const Slab& sn = c->slab[(s + 1) % c->n_slabs];
      const size_t row_bytes = (size_t)c->row_pitch * sizeof(float);
      HIP_TRY(LBM_FAILURE, edges.alloc(2 * (size_t)c->row_pitch));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(edges, ss.lat[c->cur] + (long)(ss.rows - 1) * c->row_pitch, row_bytes, hipMemcpyDefault, sl.compute));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(edges + c->row_pitch, sn.lat[c->cur], row_bytes, hipMemcpyDefault, sl.compute));
    }
    for (int r0 = 0; r0 < sl.rows; r0 += (int)chunk_rows) {
      const int nr = (sl.rows - r0 < chunk_rows) ? sl.rows - r0 : (int)chunk_rows;
      launch_vorticity_gather(c, sl, c->n_slabs > 1 ? edges.get() : nullptr, r0, r0 + nr, stage, nullptr);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(w + (size_t)(sl.row_first - c->row_first + r0) * nx, stage, (size_t)nr * nx * sizeof(float),
                                          hipMemcpyDeviceToHost, sl.compute));
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    }
  }
  return LBM_SUCCESS;
}

// ---- stress and dissipation --------------------------------------------------------------------------------------------
int lbm_set_stress(lbm_ctx* c, int every, int capacity) { return arm_gather(c, kRecStress, every, capacity, GatherArgs{}); }

int lbm_read_stress_rows(lbm_ctx* c, int max_rows, lbm_stress_row* out, int* steps, int* n_read) {
  return drain_gather(c, kRecStress, max_rows, out, steps, n_read);
}

int lbm_set_tracers(lbm_ctx* c, int n, const lbm_tracer* start, int every, int capacity) {
  GatherArgs a;
  a.tracers = n;
  if (n == 0) every = every < 0 ? every : 0;  // no tracers: disarms
  if (gather_refusals(c, kRecTracers, every, capacity, a) != LBM_SUCCESS) return LBM_FAILURE;
  if (every > 0 && tracer_starts_ok("lbm_set_tracers", c, 1, n, start) != LBM_SUCCESS) return LBM_FAILURE;
  return arm_gather_checked(c, kRecTracers, every, capacity, a, start);
}

int lbm_read_tracers(lbm_ctx* c, int max_rows, lbm_tracer* out, int* steps, int* n_read) {
  return drain_gather(c, kRecTracers, max_rows, out, steps, n_read);
}

int lbm_tracers_now(lbm_ctx* c, lbm_tracer* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_tracers_now: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_tracers_now");
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  if (c->rec.kind != kRecTracers) LBM_FAIL(LBM_FAILURE, "lbm_tracers_now: tracer particles are not armed (lbm_set_tracers)");
  HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[0].device));
  HIP_TRY(LBM_FAILURE, hipMemcpy(out, c->slab[0].tracer_state, (size_t)c->rec.args.tracers * sizeof(lbm_tracer), hipMemcpyDeviceToHost));
  return LBM_SUCCESS;
}

int lbm_read_stress(lbm_ctx* c, float* txx, float* txy, float* tyy) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_read_stress: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_stress");
  if (c->ranked || c->world > 1)
    LBM_FAIL(LBM_FAILURE, "lbm_read_stress: not available in a multi-process (rank) context: the fields of a rank's rows are not offered");
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  float* const out[3] = {txx, txy, tyy};
  const int nx = c->p.nx;
  long chunk_rows = (16L << 20) / ((long)nx * sizeof(float));
  if (chunk_rows < 1) chunk_rows = 1;
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    DeviceBuf<float> stage;  // the call's own, three planes of a chunk: nothing armed is touched
    HIP_TRY(LBM_FAILURE, stage.alloc(3 * (size_t)chunk_rows * nx));
    for (int r0 = 0; r0 < sl.rows; r0 += (int)chunk_rows) {
      const int nr = (sl.rows - r0 < chunk_rows) ? sl.rows - r0 : (int)chunk_rows;
      launch_stress_gather(c, sl, r0, nr, stage, nullptr);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      for (int i = 0; i < 3; i++)
        if (out[i])
          HIP_TRY(LBM_FAILURE, hipMemcpyAsync(out[i] + (size_t)(sl.row_first - c->row_first + r0) * nx, stage + (size_t)i * nr * nx,
                                              (size_t)nr * nx * sizeof(float), hipMemcpyDeviceToHost, sl.compute));
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    }
  }
  return LBM_SUCCESS;
}

// ---- stream function ---------------------------------------------------------------------------------------------------
int lbm_set_psi(lbm_ctx* c, int every, int capacity) { return arm_gather(c, kRecPsi, every, capacity, GatherArgs{}); }

int lbm_read_psi_rows(lbm_ctx* c, int max_rows, lbm_psi_row* out, int* steps, int* n_read) {
  return drain_gather(c, kRecPsi, max_rows, out, steps, n_read);
}

int lbm_read_psi(lbm_ctx* c, double* psi) {
  if (!c || !psi) LBM_FAIL(LBM_FAILURE, "lbm_read_psi: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_psi");
  if (c->ranked || c->world > 1)
    LBM_FAIL(LBM_FAILURE, "lbm_read_psi: not available in a multi-process (rank) context: the rows below this rank's belong to other processes");
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  const int nx = c->p.nx;
  const size_t base_words = (size_t)nx * lbm_exact::kExactLimbs;
  DeviceBuf<long long> below;  // the limbs up to the last row of the slab below, on that slab's device
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    // the call's own buffers: nothing armed is touched.  Every stream is idle (lbm_sync) and every slab is finished before
    // the next begins: no events needed
    const int band_rows = psi_band_rows(c, sl.rows, nx), bands = ceil_div(sl.rows, band_rows);
    long chunk_bands = (256L << 20) / ((long)band_rows * nx * (long)sizeof(double));  // a staging buffer of at most 256 MiB, or one band
    if (chunk_bands < 1) chunk_bands = 1;
    if (chunk_bands > bands) chunk_bands = bands;
    DeviceBuf<long long> totals, incoming, outgoing;
    DeviceBuf<double> stage;
    HIP_TRY(LBM_FAILURE, totals.alloc(psi_total_words(sl.rows, nx, band_rows)));
    HIP_TRY(LBM_FAILURE, stage.alloc((size_t)chunk_bands * band_rows * nx));
    if (s > 0) {
      HIP_TRY(LBM_FAILURE, incoming.alloc(base_words));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(incoming, below, base_words * sizeof(long long), hipMemcpyDefault, sl.compute));
    }
    if (s + 1 < c->n_slabs) HIP_TRY(LBM_FAILURE, outgoing.alloc(base_words));
    launch_psi_totals(c, sl, band_rows, totals);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    launch_psi_bases(c, sl, band_rows, totals, s > 0 ? incoming.get() : nullptr, s + 1 < c->n_slabs ? outgoing.get() : nullptr);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    for (int b0 = 0; b0 < bands; b0 += (int)chunk_bands) {
      const int nb = (bands - b0 < chunk_bands) ? bands - b0 : (int)chunk_bands;
      const int r0 = b0 * band_rows, r1 = (b0 + nb) * band_rows < sl.rows ? (b0 + nb) * band_rows : sl.rows;
      hipLaunchKernelGGL(lbm::psi_scan<true>, dim3(ceil_div(nx, lbm::kPsiColumns), nb), dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl),
                         sl.rows, band_rows, b0, (const long long*)totals, (unsigned)sl.row_first * (unsigned)nx, stage.get(),
                         (lbm::PsiCandidate*)nullptr);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(psi + (size_t)(sl.row_first - c->row_first + r0) * nx, stage, (size_t)(r1 - r0) * nx * sizeof(double),
                                          hipMemcpyDeviceToHost, sl.compute));
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    }
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    below = std::move(outgoing);
  }
  return LBM_SUCCESS;
}

int lbm_set_residual(lbm_ctx* c, int every, int capacity) { return arm_gather(c, kRecResidual, every, capacity, GatherArgs{}); }

int lbm_read_residual(lbm_ctx* c, int max_rows, lbm_residual_row* out, int* steps, int* n_read) {
  return drain_gather(c, kRecResidual, max_rows, out, steps, n_read);
}

int lbm_set_profiles(lbm_ctx* c, int every, int capacity, int axes) {
  GatherArgs a;
  a.axes = axes;
  return arm_gather(c, kRecProfiles, every, capacity, a);
}

int lbm_read_profiles(lbm_ctx* c, int max_records, lbm_profile_line* out, int* steps, int* n_read) {
  return drain_gather(c, kRecProfiles, max_records, out, steps, n_read);
}

// ---- coarse frames -----------------------------------------------------------------------------------------------------
int lbm_read_coarse(lbm_ctx* c, int bx, int by, lbm_profile_line* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_read_coarse: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_coarse");
  if (c->ranked || c->world > 1)
    LBM_FAIL(LBM_FAILURE, "lbm_read_coarse: not available in a multi-process (rank) context: a box's cells would be spread over the ranks");
  if (coarse_box_ok("lbm_read_coarse", c, bx, by) != LBM_SUCCESS) return LBM_FAILURE;
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  std::vector<long long> record;
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    const size_t words = coarse_slot_words(c, sl, bx, by), at = record.size();
    record.resize(at + words);
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    DeviceBuf<long long> slot;  // the call's own: nothing armed is touched
    if (slot.alloc(words) != hipSuccess) {
      (void)hipGetLastError();
      LBM_FAIL(LBM_FAILURE, "lbm_read_coarse: cannot allocate the frame's %.1f MiB of slab %d", (double)(words * sizeof(long long)) / 1048576.0, s);
    }
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(slot, 0, words * sizeof(long long), sl.compute));
    launch_coarse(c, sl, bx, by, slot);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    HIP_TRY(LBM_FAILURE, hipMemcpyAsync(record.data() + at, slot, words * sizeof(long long), hipMemcpyDeviceToHost, sl.compute));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
  }
  const GatherOwner g = context_owner(c);  // the slabs' slots of the one record (one after the other) -> the frame
  lbm_coarse::coarse_frame_from_words(record.data(), g.shares, g.row_first, g.row_count, g.nx, g.ny, bx, by, out);
  return LBM_SUCCESS;
}

int lbm_set_coarse_frames(lbm_ctx* c, int every, int capacity, int bx, int by) {
  GatherArgs a;
  a.box_x = bx;
  a.box_y = by;
  return arm_gather(c, kRecCoarse, every, capacity, a);
}

int lbm_read_coarse_frames(lbm_ctx* c, int max_frames, lbm_profile_line* out, int* steps, int* n_read) {
  return drain_gather(c, kRecCoarse, max_frames, out, steps, n_read);
}

// the planes [first, first + 4) of every slab's sums, stitched by row_first; lbm_read_mean and lbm_read_mean2
static int read_mean_planes(lbm_ctx* c, int first, double* const (&out)[4], long long* n_samples) {
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    const size_t cells = (size_t)sl.rows * c->p.nx;
    for (int j = 0; j < 4; j++)
      if (out[j])
        HIP_TRY(LBM_FAILURE, hipMemcpyAsync(out[j] + (size_t)(sl.row_first - c->row_first) * c->p.nx, sl.mean_sums + (size_t)(first + j) * cells,
                                            cells * sizeof(double), hipMemcpyDeviceToHost, sl.compute));
  }
  for (int s = 0; s < c->n_slabs; s++) {
    HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[s].device));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->slab[s].compute));
  }
  if (n_samples) *n_samples = c->rec.written;
  return LBM_SUCCESS;
}

int lbm_read_mean(lbm_ctx* c, double* sum_u_x, double* sum_u_y, double* sum_u_mag, double* sum_pressure, long long* n_samples) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_read_mean: null context");
  if (n_samples) *n_samples = 0;
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_mean");
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  if (c->rec.kind != kRecMean) LBM_FAIL(LBM_FAILURE, "lbm_read_mean: the mean fields are not armed (lbm_set_mean)");
  double* const out[4] = {sum_u_x, sum_u_y, sum_u_mag, sum_pressure};
  return read_mean_planes(c, 0, out, n_samples);
}

int lbm_read_mean2(lbm_ctx* c, double* sum_uxux, double* sum_uyuy, double* sum_uxuy, double* sum_pp, long long* n_samples) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_read_mean2: null context");
  if (n_samples) *n_samples = 0;
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_mean2");
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  if (c->rec.kind != kRecMean || c->rec.order != 2)
    LBM_FAIL(LBM_FAILURE, "lbm_read_mean2: the second moments are not armed (lbm_set_mean_order(ctx, every, 2))");
  double* const out[4] = {sum_uxux, sum_uyuy, sum_uxuy, sum_pp};
  return read_mean_planes(c, 4, out, n_samples);
}

static const char kMemberRun[] = "%s: this context is a member of a batch (lbm_create_batch); lbm_batch_run advances all its members";

int lbm_run(lbm_ctx* c, int n_steps) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_run: null context");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_run");
  if (c->batch) LBM_FAIL(LBM_FAILURE, kMemberRun, "lbm_run");
  return run_steps(c, n_steps, nullptr);
}

int lbm_run_timed(lbm_ctx* c, int n_steps, float* kernel_ms_per_step) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_run: null context");
  if (kernel_ms_per_step) *kernel_ms_per_step = 0.f;
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_run_timed");
  if (c->batch) LBM_FAIL(LBM_FAILURE, kMemberRun, "lbm_run_timed");
  if (!kernel_ms_per_step) LBM_FAIL(LBM_FAILURE, "lbm_run_timed: NULL output");
  return run_steps(c, n_steps, kernel_ms_per_step);
}

// what lbm_sync does behind its refusals, and what the library's own paths call: a path that has seen the give-up itself
// (checked_run's judge) still gets the first report from here
static int sync_ctx(lbm_ctx* c) {
  for (int s = 0; s < c->n_slabs; s++) {
    HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[s].device));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->slab[s].compute));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->slab[s].comm));
    for (hipStream_t g : c->slab[s].group_extra) if (g) HIP_TRY(LBM_FAILURE, hipStreamSynchronize(g));
  }
  if (c->resident_used) {
    // did every workgroup of the resident kernel get its neighbours' rows in time?  (a batch member: of any batched launch)
    c->resident_used = false;
    if (const int status = gave_up(c)) return report_give_up(c, status);
  }
  return LBM_SUCCESS;
}

int lbm_sync(lbm_ctx* c) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_sync: null context");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_sync");
  return sync_ctx(c);
}

int lbm_read_halo_log(lbm_ctx* c, unsigned char* out, int n) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_read_halo_log: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_halo_log");
  if (n < 0 || n > c->steps_done) LBM_FAIL(LBM_FAILURE, "lbm_read_halo_log: %d steps requested, %d recorded", n, c->steps_done);
  if (n == 0) return LBM_SUCCESS;
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  std::vector<unsigned char> part((size_t)n);
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    if (sl.fresh_log) {
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      HIP_TRY(LBM_FAILURE, hipMemcpy(part.data(), sl.fresh_log, (size_t)n, hipMemcpyDeviceToHost));
    } else {
      part.assign((size_t)n, 3);  // the mode was never used: every halo row was the row of its step
    }
    for (int t = 0; t < n; t++) out[(size_t)t * c->n_slabs + s] = part[(size_t)t];
  }
  return LBM_SUCCESS;
}

int lbm_read_av_vels(lbm_ctx* c, float* out, int n) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_read_av_vels: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_av_vels");
  if (n < 0 || n > c->steps_done) LBM_FAIL(LBM_FAILURE, "lbm_read_av_vels: %d steps requested, %d recorded", n, c->steps_done);
  if (n == 0) return LBM_SUCCESS;
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  std::vector<double> total((size_t)n, 0.0), part((size_t)n);
  for (int s = 0; s < c->n_slabs; s++) {
    HIP_TRY(LBM_FAILURE, hipSetDevice(c->slab[s].device));
    HIP_TRY(LBM_FAILURE, hipMemcpy(part.data(), c->slab[s].tot_u, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    for (int t = 0; t < n; t++) total[(size_t)t] += part[(size_t)t];
  }
  if (c->hosted) {
    // the reference's MPI_Reduce(av_vels, SUM) (MPI/d2q9-bgk.c:298-309) through the host's own all-reduce
    if (c->world > 1 && c->host_comm.allreduce_sum(c->host_comm.user, total.data(), n) != 0)
      LBM_FAIL(LBM_FAILURE, "the host's all-reduce callback failed");
  } else if (c->ranked) {
    // the reference's MPI_Reduce(av_vels, SUM) (MPI/d2q9-bgk.c:298-309), as an all-reduce
    Slab& sl = c->slab[0];
    double* tmp = sl.reduce_buf;  // allocated once at create: nothing to leak on an error return
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    HIP_TRY(LBM_FAILURE, hipMemcpy(tmp, total.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    RCCL_OR_FAIL(LBM_FAILURE);
    NCCL_TRY(LBM_FAILURE, rc_api_->AllReduce(tmp, tmp, (size_t)n, ncclDouble, ncclSum, sl.nccl, sl.comm));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.comm));
    HIP_TRY(LBM_FAILURE, hipMemcpy(total.data(), tmp, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  }
  const float cells = (float)c->fluid_cells;
  for (int t = 0; t < n; t++) out[t] = (float)total[(size_t)t] / cells;  // SerialCode/d2q9-bgk.c:457
  return LBM_SUCCESS;
}

int lbm_read_cells(lbm_ctx* c, float* cells_aos) {
  if (!c || !cells_aos) LBM_FAIL(LBM_FAILURE, "lbm_read_cells: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_cells");
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  const int nx = c->p.nx;
  long chunk_rows = (64L << 20) / ((long)nx * lbm::kQ * sizeof(float));
  if (chunk_rows < 1) chunk_rows = 1;
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    DeviceBuf<float> stage;
    HIP_TRY(LBM_FAILURE, stage.alloc((size_t)chunk_rows * nx * lbm::kQ));
    for (int r0 = 0; r0 < sl.rows; r0 += (int)chunk_rows) {
      const int nr = (sl.rows - r0 < chunk_rows) ? sl.rows - r0 : (int)chunk_rows;
      const size_t n = (size_t)nr * nx * lbm::kQ;
      hipLaunchKernelGGL(lbm::soa_to_aos, dim3(ceil_div((long)n, 256)), dim3(256), 0, sl.compute,
                         lattice_args(c, sl), stage, r0, nr);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(cells_aos + (size_t)(sl.row_first - c->row_first + r0) * nx * lbm::kQ, stage,
                                          n * sizeof(float), hipMemcpyDeviceToHost, sl.compute));
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    }
  }
  return LBM_SUCCESS;
}

int lbm_read_final_state(lbm_ctx* c, float* u_x, float* u_y, float* u_mag, float* pressure) {
  if (!c || !u_x || !u_y || !u_mag || !pressure) LBM_FAIL(LBM_FAILURE, "lbm_read_final_state: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_read_final_state");
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  const int nx = c->p.nx;
  long chunk_rows = (16L << 20) / ((long)nx * sizeof(float));
  if (chunk_rows < 1) chunk_rows = 1;
  float* outs[4] = {u_x, u_y, u_mag, pressure};
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    DeviceBuf<float> stage;
    const size_t chunk_cells = (size_t)chunk_rows * nx;
    HIP_TRY(LBM_FAILURE, stage.alloc(4 * chunk_cells));
    for (int r0 = 0; r0 < sl.rows; r0 += (int)chunk_rows) {
      const int nr = (sl.rows - r0 < chunk_rows) ? sl.rows - r0 : (int)chunk_rows;
      const size_t n = (size_t)nr * nx;
      hipLaunchKernelGGL(lbm::final_state, dim3(ceil_div((long)n, 256)), dim3(256), 0, sl.compute,
                         lattice_args(c, sl), r0, nr, c->p.density,
                         stage, stage + chunk_cells, stage + 2 * chunk_cells, stage + 3 * chunk_cells);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      const size_t off = (size_t)(sl.row_first - c->row_first + r0) * nx;
      for (int k = 0; k < 4; k++)
        HIP_TRY(LBM_FAILURE, hipMemcpyAsync(outs[k] + off, stage + k * chunk_cells, n * sizeof(float),
                                            hipMemcpyDeviceToHost, sl.compute));
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    }
  }
  return LBM_SUCCESS;
}

// global sums of |u| over fluid cells and of density over all cells
static int lattice_totals(lbm_ctx* c, double* speed, double* mass) {
  if (lbm_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  double tot[2] = {0.0, 0.0};
  std::vector<double> h(2 * kSumBlocks);
  for (int s = 0; s < c->n_slabs; s++) {
    Slab& sl = c->slab[s];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    hipLaunchKernelGGL(lbm::lattice_sums, dim3(kSumBlocks), dim3(lbm::kBlock), 0, sl.compute, lattice_args(c, sl),
                       sl.rows, sl.scratch, sl.scratch + kSumBlocks);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    HIP_TRY(LBM_FAILURE, hipMemcpyAsync(h.data(), sl.scratch, 2 * kSumBlocks * sizeof(double),
                                        hipMemcpyDeviceToHost, sl.compute));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.compute));
    for (int i = 0; i < kSumBlocks; i++) { tot[0] += h[i]; tot[1] += h[kSumBlocks + i]; }
  }
  if (c->hosted) {
    if (c->world > 1 && c->host_comm.allreduce_sum(c->host_comm.user, tot, 2) != 0)
      LBM_FAIL(LBM_FAILURE, "the host's all-reduce callback failed");
  } else if (c->ranked) {
    Slab& sl = c->slab[0];
    HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
    HIP_TRY(LBM_FAILURE, hipMemcpy(sl.scratch, tot, 2 * sizeof(double), hipMemcpyHostToDevice));
    RCCL_OR_FAIL(LBM_FAILURE);
    NCCL_TRY(LBM_FAILURE, rc_api_->AllReduce(sl.scratch, sl.scratch, 2, ncclDouble, ncclSum, sl.nccl, sl.comm));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(sl.comm));
    HIP_TRY(LBM_FAILURE, hipMemcpy(tot, sl.scratch, 2 * sizeof(double), hipMemcpyDeviceToHost));
  }
  *speed = tot[0];
  *mass = tot[1];
  return LBM_SUCCESS;
}

int lbm_av_velocity(lbm_ctx* c, float* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_av_velocity: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_av_velocity");
  double speed, mass;
  if (lattice_totals(c, &speed, &mass) != LBM_SUCCESS) return LBM_FAILURE;
  *out = (float)speed / (float)c->fluid_cells;
  return LBM_SUCCESS;
}

int lbm_total_density(lbm_ctx* c, double* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_total_density: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_total_density");
  double speed, mass;
  if (lattice_totals(c, &speed, &mass) != LBM_SUCCESS) return LBM_FAILURE;
  *out = mass;
  return LBM_SUCCESS;
}

int lbm_calc_reynolds(lbm_ctx* c, float* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_calc_reynolds: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, c, "lbm_calc_reynolds");
  float av;
  if (lbm_av_velocity(c, &av) != LBM_SUCCESS) return LBM_FAILURE;
  const float viscosity = 1.f / 6.f * (2.f / c->p.omega - 1.f);  // SerialCode/d2q9-bgk.c:639
  *out = av * c->p.reynolds_dim / viscosity;                     // :641
  return LBM_SUCCESS;
}

// ---- batches -----------------------------------------------------------------------------------------------------
void lbm_destroy_batch(lbm_batch* bt) {
  if (!bt) return;
  if (bt->stream) {
    (void)hipSetDevice(bt->members[0]->slab[0].device);
    (void)hipStreamSynchronize(bt->stream);
  }
  // members 1.. borrow member 0's compute stream, which member 0 owns: they go first
  for (size_t i = bt->members.size(); i-- > 0;) {
    lbm_ctx* c = bt->members[i];
    c->batch = nullptr;
    lbm_destroy(c);
  }
  delete bt;  // the batch's own tables go with it
}

lbm_batch* lbm_create_batch(int n_members, const lbm_params* params, const int* obstacles, const float* cells_aos,
                            int math_mode) {
  // everything that can be checked without a device is checked first
  if (n_members < 1) LBM_FAIL(nullptr, "lbm_create_batch: n_members must be at least 1 (got %d)", n_members);
  if (!params) LBM_FAIL(nullptr, "lbm_create_batch: params is NULL");
  if (!obstacles) LBM_FAIL(nullptr, "lbm_create_batch: obstacles is NULL");
  if (math_mode != LBM_MATH_EXACT && math_mode != LBM_MATH_FAST)
    LBM_FAIL(nullptr, "lbm_create_batch: unknown math mode %d", math_mode);
  for (int i = 0; i < n_members; i++) {
    const lbm_params& p = params[i];
    if (!validate_params(&p)) LBM_FAIL(nullptr, "lbm_create_batch: member %d has invalid parameters", i);
    if (p.nx != params[0].nx || p.ny != params[0].ny)
      LBM_FAIL(nullptr, "lbm_create_batch: member %d is %dx%d, member 0 is %dx%d", i, p.nx, p.ny, params[0].nx, params[0].ny);
    if (p.max_iters != params[0].max_iters)
      LBM_FAIL(nullptr, "lbm_create_batch: member %d has max_iters %d, member 0 has %d", i, p.max_iters, params[0].max_iters);
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    LBM_FAIL(nullptr, "lbm_create_batch: no HIP device available (this library has no CPU path)");

  lbm_batch* bt = new lbm_batch();
  const size_t cells = (size_t)params[0].nx * params[0].ny;
  for (int i = 0; i < n_members; i++) {
    const ObstacleSource obst = {OBST_GLOBAL, obstacles + i * cells, 0, 0, false};
    lbm_ctx* c = create_common(&params[i], obst, cells_aos ? cells_aos + i * cells * lbm::kQ : nullptr, 1, math_mode, 0, 1,
                               nullptr, 0);
    if (!c) {
      char why[sizeof(g_last_error)];
      strncpy(why, g_last_error, sizeof(why) - 1);
      why[sizeof(why) - 1] = 0;
      lbm_destroy_batch(bt);
      LBM_FAIL(nullptr, "lbm_create_batch: member %d: %s", i, why);
    }
    bt->members.push_back(c);
    c->batch = bt;
    const lbm_ctx* c0 = bt->members[0];
    if (c->halo != HALO_SELF || !lbm_plan::same_resident_launch(c->plan, c0->plan)) {
      lbm_destroy_batch(bt);
      LBM_FAIL(nullptr, "lbm_create_batch: member %d is not a single periodic slab like member 0 (is LBM_FORCE_HALO set?)", i);
    }
  }
  lbm_ctx* c0 = bt->members[0];
  Slab& sl0 = c0->slab[0];
  // one stream for all: members 1.. give theirs up (idle: creation ended with a synchronize)
  bt->stream = sl0.compute;
  for (int i = 1; i < n_members; i++) {
    Slab& sl = bt->members[i]->slab[0];
    sl.compute_own.reset();
    sl.compute = bt->stream;
  }
  bt->members_per_launch = 1;
  bt->launches = n_members;
  if (c0->plan.resident) {
    // co-residency, checked here once: one-XCD members take one XCD each; other shapes one workgroup per CU, and no XCD
    // may be dealt more working workgroups than it has CUs (member m's workgroup w runs on XCD w % 8)
    int cus = 0;
    if (hipSetDevice(sl0.device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sl0.device) != hipSuccess) {
      lbm_destroy_batch(bt);
      LBM_FAIL(nullptr, "lbm_create_batch: cannot query the device's CU count");
    }
    bt->resident = 1;
    bt->member_wgs = c0->plan.resident_bands / c0->plan.resident_group;
    int mpl = 8;
    if (!c0->plan.resident_one_xcd) {
      mpl = cus / bt->member_wgs;
      while (mpl > 1 && (long)mpl * ceil_div(bt->member_wgs, 8) > cus / 8) mpl--;
      if (mpl < 1) mpl = 1;
    }
    bt->members_per_launch = mpl;
    bt->launches = ceil_div(n_members, mpl);
    if (!upload_member_table(bt) || bt->status.alloc(1) != hipSuccess || hipMemset(bt->status, 0, sizeof(int)) != hipSuccess ||
        bt->status_host.alloc(1) != hipSuccess) {
      lbm_destroy_batch(bt);
      LBM_FAIL(nullptr, "lbm_create_batch: cannot allocate the member table");
    }
    *bt->status_host = 0;
  }
  return bt;
}

lbm_ctx* lbm_batch_member(lbm_batch* bt, int index) {
  if (!bt) LBM_FAIL(nullptr, "lbm_batch_member: null batch");
  if (index < 0 || index >= (int)bt->members.size())
    LBM_FAIL(nullptr, "lbm_batch_member: index %d out of range (the batch has %d members)", index, (int)bt->members.size());
  return bt->members[(size_t)index];
}

// n_steps timesteps of every member, as one call: batched on the resident kernel where the call is long enough for it
static int batch_advance(lbm_batch* bt, int n_steps) {
  lbm_ctx* c0 = bt->members[0];
  if (bt->resident && n_steps >= c0->plan.resident_min_steps) {
    if (run_batch_resident(bt, n_steps) != LBM_SUCCESS) return LBM_FAILURE;
    for (lbm_ctx* c : bt->members) {
      c->rec.written += recorded_between(c->rec, c->steps_done, (long long)c->steps_done + n_steps);
      c->steps_done += n_steps;
    }
  } else {
    // short calls and shapes the resident kernel does not take: the members one after another, per-pass kernels
    for (lbm_ctx* c : bt->members)
      if (run_steps(c, n_steps, nullptr) != LBM_SUCCESS) return LBM_FAILURE;
    bt->cur = c0->cur;
    // a member with frames (or probes) armed ran its call split at its recorder steps, i.e. possibly another number of passes: its
    // lattice may lie in the other buffer.  Batched launches take every member's lattice at the batch's parity
    // (bt->table), so such a member's lattice moves there (a device copy on the batch's stream).
    for (lbm_ctx* c : bt->members) {
      if (c->cur == bt->cur) continue;
      Slab& sl = c->slab[0];
      const size_t lat_bytes = (size_t)(sl.rows + 2 * kHaloRows) * c->row_pitch * sizeof(float);
      HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(sl.lat_alloc[bt->cur], sl.lat_alloc[c->cur], lat_bytes, hipMemcpyDeviceToDevice,
                                          bt->stream));
      c->cur = bt->cur;
    }
  }
  bt->steps_done += n_steps;
  return LBM_SUCCESS;
}

int lbm_batch_run(lbm_batch* bt, int n_steps) {
  if (!bt) LBM_FAIL(LBM_FAILURE, "lbm_batch_run: null batch");
  REFUSE_FAILED(LBM_FAILURE, bt, "lbm_batch_run");
  if (n_steps < 0) LBM_FAIL(LBM_FAILURE, "lbm_batch_run: negative step count");
  if (n_steps == 0) return LBM_SUCCESS;
  lbm_ctx* c0 = bt->members[0];
  if (bt->steps_done + n_steps > c0->capacity)
    LBM_FAIL(LBM_FAILURE, "lbm_batch_run: %d steps requested but the av_vels record holds %d (maxIters)",
             bt->steps_done + n_steps, c0->capacity);
  for (lbm_ctx* c : bt->members)  // every member's records must fit before any member runs
    if (recorder_fits(c, n_steps, "lbm_batch_run") != LBM_SUCCESS) return LBM_FAILURE;
  if (bt->rec.kind == kRecNone) return batch_advance(bt, n_steps);
  // a gather kind armed: the call runs as the sub-calls that end at the sample steps, each advanced as a call of its
  // length would be and followed by the record of all members into its zeroed slot (lbm_run does the same for one context,
  // run_steps and take_record)
  const GatherKind& kind = gather_kind(bt->rec.kind);
  if (recorder_fits(bt->rec, bt->steps_done, n_steps, "lbm_batch_run", kind.batch_reader) != LBM_SUCCESS) return LBM_FAILURE;
  const int e = bt->rec.every;
  for (int t = 0; t < n_steps;) {
    const int tt = bt->steps_done, r = tt % e;
    const long long rec_tt = r ? (long long)tt + (e - r) : tt;  // next sample step
    const int seg = (rec_tt - tt + 1 < n_steps - t) ? (int)(rec_tt - tt + 1) : n_steps - t;
    if (batch_advance(bt, seg) != LBM_SUCCESS) return LBM_FAILURE;
    if (bt->steps_done - 1 == rec_tt) {
      HIP_TRY(LBM_FAILURE, hipSetDevice(c0->slab[0].device));
      bool ringless;
      long long* slot = zeroed_slot(bt->gather_ring, gather_slot_words(bt), bt->rec, bt->stream, &ringless);
      if ((!slot && !ringless) || kind.take_batch(bt, slot) != LBM_SUCCESS) return LBM_FAILURE;
      bt->rec.written++;
    }
    t += seg;
  }
  return LBM_SUCCESS;
}

// what lbm_batch_sync does behind its refusals (sync_ctx does so for a context)
static int sync_batch(lbm_batch* bt) {
  int rc = LBM_SUCCESS;
  for (lbm_ctx* c : bt->members)  // every member reports the verdict of the launches it was part of; the first fails the batch
    if (sync_ctx(c) != LBM_SUCCESS) rc = LBM_FAILURE;
  return rc;
}

int lbm_batch_sync(lbm_batch* bt) {
  if (!bt) LBM_FAIL(LBM_FAILURE, "lbm_batch_sync: null batch");
  REFUSE_FAILED(LBM_FAILURE, bt, "lbm_batch_sync");
  return sync_batch(bt);
}

int lbm_batch_get_info(const lbm_batch* bt, lbm_batch_info* out) {
  if (!bt || !out) LBM_FAIL(LBM_FAILURE, "lbm_batch_get_info: NULL argument");
  const lbm_ctx* c0 = bt->members[0];
  out->members = (int)bt->members.size();
  out->members_per_launch = bt->members_per_launch;
  out->launches_per_chunk = bt->launches;
  out->resident_steps = bt->resident ? kResidentChunk : 0;
  out->resident_min_steps = bt->resident ? c0->plan.resident_min_steps : 0;
  out->steps_done = bt->steps_done;
  return LBM_SUCCESS;
}

// ---- the gather kinds of a batch -------------------------------------------------------------------------------------
int lbm_batch_set_forces(lbm_batch* bt, int n_bodies, const int* body_of_cell, int every, int capacity) {
  GatherArgs a;
  a.bodies = n_bodies;
  if (batch_gather_refusals(bt, kRecForces, every, capacity, a) != LBM_SUCCESS) return LBM_FAILURE;
  // the labels go to the device only once nothing is refused and no member is in the way
  ForceLabels labels(every > 0 && body_of_cell ? bt->members.size() : 0);
  for (size_t i = 0; i < labels.size(); i++) {
    lbm_ctx* c = bt->members[i];
    const int* src = body_of_cell + i * ((size_t)c->p.nx * c->p.ny);
    unsigned first_bad;
    if (upload_labels(c, c->slab[0], src, n_bodies, labels[i], &first_bad) != LBM_SUCCESS) return LBM_FAILURE;
    if (first_bad != kNoBadLabel)
      LBM_FAIL(LBM_FAILURE, "lbm_batch_set_forces: member %d: the blocked cell (%d, %d) has body %d, outside 0 .. %d", (int)i,
               (int)(first_bad % (unsigned)c->p.nx), (int)(first_bad / (unsigned)c->p.nx), src[first_bad], n_bodies - 1);
  }
  return arm_batch_gather_checked(bt, kRecForces, every, capacity, a, &labels);
}

int lbm_batch_read_forces(lbm_batch* bt, int max_rows, double* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecForces, max_rows, out, steps, n_read);
}

int lbm_batch_forces_links(lbm_batch* bt, int* links) {
  if (!bt || !links) LBM_FAIL(LBM_FAILURE, "lbm_batch_forces_links: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, bt, "lbm_batch_forces_links");
  if (bt->rec.kind != kRecForces)
    LBM_FAIL(LBM_FAILURE, "lbm_batch_forces_links: the obstacle forces are not armed (lbm_batch_set_forces)");
  for (size_t j = 0; j < bt->force_link_counts.size(); j++) links[j] = bt->force_link_counts[j];
  return LBM_SUCCESS;
}

int lbm_batch_set_stats(lbm_batch* bt, int every, int capacity) { return arm_batch_gather(bt, kRecStats, every, capacity, GatherArgs{}); }

int lbm_batch_read_stats(lbm_batch* bt, int max_rows, lbm_stats_row* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecStats, max_rows, out, steps, n_read);
}

int lbm_batch_set_enstrophy(lbm_batch* bt, int every, int capacity) { return arm_batch_gather(bt, kRecEnstrophy, every, capacity, GatherArgs{}); }

int lbm_batch_read_enstrophy(lbm_batch* bt, int max_rows, lbm_enstrophy_row* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecEnstrophy, max_rows, out, steps, n_read);
}

int lbm_batch_set_stress(lbm_batch* bt, int every, int capacity) { return arm_batch_gather(bt, kRecStress, every, capacity, GatherArgs{}); }

int lbm_batch_read_stress_rows(lbm_batch* bt, int max_rows, lbm_stress_row* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecStress, max_rows, out, steps, n_read);
}

int lbm_batch_set_tracers(lbm_batch* bt, int n, const lbm_tracer* start, int every, int capacity) {
  GatherArgs a;
  a.tracers = n;
  if (n == 0) every = every < 0 ? every : 0;  // no tracers: disarms
  if (batch_gather_refusals(bt, kRecTracers, every, capacity, a) != LBM_SUCCESS) return LBM_FAILURE;
  if (every > 0 && tracer_starts_ok("lbm_batch_set_tracers", bt->members[0], bt->members.size(), n, start) != LBM_SUCCESS) return LBM_FAILURE;
  return arm_batch_gather_checked(bt, kRecTracers, every, capacity, a, start);
}

int lbm_batch_read_tracers(lbm_batch* bt, int max_rows, lbm_tracer* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecTracers, max_rows, out, steps, n_read);
}

int lbm_batch_tracers_now(lbm_batch* bt, lbm_tracer* out) {
  if (!bt || !out) LBM_FAIL(LBM_FAILURE, "lbm_batch_tracers_now: NULL argument");
  REFUSE_FAILED(LBM_FAILURE, bt, "lbm_batch_tracers_now");
  if (lbm_batch_sync(bt) != LBM_SUCCESS) return LBM_FAILURE;
  if (bt->rec.kind != kRecTracers) LBM_FAIL(LBM_FAILURE, "lbm_batch_tracers_now: tracer particles are not armed (lbm_batch_set_tracers)");
  HIP_TRY(LBM_FAILURE, hipSetDevice(bt->members[0]->slab[0].device));
  HIP_TRY(LBM_FAILURE, hipMemcpy(out, bt->tracer_state, bt->members.size() * (size_t)bt->rec.args.tracers * sizeof(lbm_tracer),
                                 hipMemcpyDeviceToHost));
  return LBM_SUCCESS;
}

int lbm_batch_set_psi(lbm_batch* bt, int every, int capacity) { return arm_batch_gather(bt, kRecPsi, every, capacity, GatherArgs{}); }

int lbm_batch_read_psi_rows(lbm_batch* bt, int max_rows, lbm_psi_row* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecPsi, max_rows, out, steps, n_read);
}

int lbm_batch_set_residual(lbm_batch* bt, int every, int capacity) { return arm_batch_gather(bt, kRecResidual, every, capacity, GatherArgs{}); }

int lbm_batch_read_residual(lbm_batch* bt, int max_rows, lbm_residual_row* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecResidual, max_rows, out, steps, n_read);
}

int lbm_batch_set_profiles(lbm_batch* bt, int every, int capacity, int axes) {
  GatherArgs a;
  a.axes = axes;
  return arm_batch_gather(bt, kRecProfiles, every, capacity, a);
}

int lbm_batch_read_profiles(lbm_batch* bt, int max_records, lbm_profile_line* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecProfiles, max_records, out, steps, n_read);
}

int lbm_batch_set_coarse_frames(lbm_batch* bt, int every, int capacity, int bx, int by) {
  GatherArgs a;
  a.box_x = bx;
  a.box_y = by;
  return arm_batch_gather(bt, kRecCoarse, every, capacity, a);
}

int lbm_batch_read_coarse_frames(lbm_batch* bt, int max_frames, lbm_profile_line* out, int* steps, int* n_read) {
  return drain_batch_gather(bt, kRecCoarse, max_frames, out, steps, n_read);
}

// ---- checked runs: to steady state on the average velocity (lbm_run_until) or the velocity residual (..._residual) ----
// A checked run is segments of check_every steps, each followed by its criterion's check, which sets a stop word on the
// device that travels to the host; checked_run drives a context, checked_batch_run a batch, and an entry point adds its
// criterion: what starts a call (begin), the launches of one check, and the result.
// argument checks shared by the four entry points (no device needed)
static int steady_args_ok(const char* who, int steps_done, int capacity, int max_steps, int check_every, double tol, int patience) {
  if (max_steps < 0) LBM_FAIL(LBM_FAILURE, "%s: negative step count", who);
  if ((long long)steps_done + max_steps > capacity)
    LBM_FAIL(LBM_FAILURE, "%s: %lld steps requested but the av_vels record holds %d (maxIters)", who,
             (long long)steps_done + max_steps, capacity);
  if (check_every < 1) LBM_FAIL(LBM_FAILURE, "%s: check_every must be at least 1 (got %d)", who, check_every);
  if (patience < 1) LBM_FAIL(LBM_FAILURE, "%s: patience must be at least 1 (got %d)", who, patience);
  if (!(tol >= 0.0)) LBM_FAIL(LBM_FAILURE, "%s: tol must be a non-negative number (got %g)", who, tol);
  return LBM_SUCCESS;
}
static const char kSteadyRecorder[] = "%s: %s are armed (%s); a steady-state run does not record %s";

static void steady_fill(lbm_steady_result* out, const lbm::SteadyState& st, int steps_run) {
  out->steps_run = steps_run;
  out->steady = st.stop ? 1 : 0;
  out->steady_step = st.steady_step;
  out->checks = st.checks;
  out->last_rel = st.last_rel;
  out->last_mean = st.prev_mean;
}

// the stop word of a checked run, its pinned pair and their events (slab 0's device is current)
static int steady_buffers(lbm_ctx* c) {
  if (c->ev_steady[1]) return LBM_SUCCESS;  // created last: the set is whole (an attempt that failed half-way starts again)
  HIP_TRY(LBM_FAILURE, c->steady_state.alloc(1));
  HIP_TRY(LBM_FAILURE, c->steady_stop_host.alloc(2));
  for (int i = 0; i < 2; i++) HIP_TRY(LBM_FAILURE, c->ev_steady[i].create(hipEventDisableTiming));
  return LBM_SUCCESS;
}

// ... and of a batch: the finished-count with its stop word (all_steady), the pinned copy and its event
static int steady_batch_buffers(lbm_batch* bt) {
  if (bt->ev_steady) return LBM_SUCCESS;  // created last: the set is whole (an attempt that failed half-way starts again)
  HIP_TRY(LBM_FAILURE, bt->steady_batch.alloc(1));
  HIP_TRY(LBM_FAILURE, bt->steady_stop_host.alloc(1));
  HIP_TRY(LBM_FAILURE, bt->ev_steady.create(hipEventDisableTiming));
  return LBM_SUCCESS;
}

// the verdict of the runtime on the launches in front
static int launched() {
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  return LBM_SUCCESS;
}

// a stop word on its way to the host behind a check: 4 bytes into a pinned slot, and the event that says they are there
static int post_stop_word(const int* word, int* slot, hipEvent_t ev, hipStream_t stream) {
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(slot, word, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIP_TRY(LBM_FAILURE, hipEventRecord(ev, stream));
  return LBM_SUCCESS;
}
static int wait_stop_word(hipEvent_t ev, const int* slot, bool* stop) {
  HIP_TRY(LBM_FAILURE, hipEventSynchronize(ev));
  *stop = *slot != 0;
  return LBM_SUCCESS;
}

// no recorder of a context (or batch member) may be armed in a checked run
static int steady_recorder_off(const lbm_ctx* c, const char* who) {
  if (c->rec.kind == kRecNone) return LBM_SUCCESS;
  const RecorderKind& k = kind_words(c->rec.kind);
  LBM_FAIL(LBM_FAILURE, kSteadyRecorder, who, k.name, k.setter, k.noun);
}

// what `who` refuses of a context before any work (no device needed); `noun`: what its check reads of the one slab
static int checked_ctx_ok(const lbm_ctx* c, const char* who, const char* noun, int max_steps, int check_every, double tol, int patience) {
  if (c->batch) LBM_FAIL(LBM_FAILURE, kMemberRun, who);
  if (steady_args_ok(who, c->steps_done, c->capacity, max_steps, check_every, tol, patience) != LBM_SUCCESS) return LBM_FAILURE;
  if (steady_recorder_off(c, who) != LBM_SUCCESS) return LBM_FAILURE;
  if (c->halo_mode != LBM_HALO_SYNC) LBM_FAIL(LBM_FAILURE, "%s: only LBM_HALO_SYNC runs can be checked (the halo mode is %d)", who, c->halo_mode);
  if (c->ranked || c->world > 1)
    LBM_FAIL(LBM_FAILURE, "%s: not available in a multi-process context (every rank would have to take the same decision)", who);
  if (c->n_slabs != 1)
    LBM_FAIL(LBM_FAILURE, "%s: the context has %d slabs; the check reads one slab's %s (single-slab contexts only)", who, c->n_slabs, noun);
  return LBM_SUCCESS;
}
// ... and of a batch
static int checked_batch_ok(const lbm_batch* bt, const char* who, int max_steps, int check_every, double tol, int patience) {
  if (steady_args_ok(who, bt->steps_done, bt->members[0]->capacity, max_steps, check_every, tol, patience) != LBM_SUCCESS) return LBM_FAILURE;
  for (const lbm_ctx* c : bt->members)
    if (steady_recorder_off(c, who) != LBM_SUCCESS) return LBM_FAILURE;
  if (bt->rec.kind != kRecNone)  // a gather kind armed on the batch
    LBM_FAIL(LBM_FAILURE, kSteadyRecorder, who, kind_words(bt->rec.kind).name, gather_kind(bt->rec.kind).batch_setter,
             kind_words(bt->rec.kind).noun);
  return LBM_SUCCESS;
}

// The E steps of one segment of a context.  On the resident path what lbm_run issues for them (first-step acceleration, the
// launches of run_resident with accel_last = 0 on the last one), except that the acceleration stands back once a check has
// said "stop" (accelerate_row_unless); else the passes of lbm_run.  Slab 0's device is current afterwards.
static int issue_segment(lbm_ctx* c, bool resident, int E) {
  Slab& sl = c->slab[0];
  if (!resident && run_passes(c, E, false, false) != LBM_SUCCESS) return LBM_FAILURE;
  HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
  if (!resident) return LBM_SUCCESS;
  const AccelWeights w = accel_weights(c->p);
  hipLaunchKernelGGL(lbm::accelerate_row_unless, dim3(ceil_div(c->p.nx, 256)), dim3(256), 0, sl.compute,
                     lattice_args(c, sl, c->cur, c->cur), sl.accel_row, w.a1, w.a2, (const lbm::SteadyState*)c->steady_state);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  if (run_resident(c, E) != LBM_SUCCESS) return LBM_FAILURE;
  c->steps_done += E;
  return LBM_SUCCESS;
}

// One checked run of a context that checked_ctx_ok has passed: begin() starts the criterion (its buffers, its reset
// launches behind steady_reset, its baseline), check(index, first) launches the check of segment `index`, whose steps
// began at step `first`; the check sets SteadyState::stop when the run is to end.  The call's steps are run and waited for
// when this returns; the caller reads its criterion's state.
static int checked_run(lbm_ctx* c, int max_steps, int E, const std::function<int()>& begin, const std::function<int(int, int)>& check) {
  Slab& sl = c->slab[0];
  HIP_TRY(LBM_FAILURE, hipSetDevice(sl.device));
  if (steady_buffers(c) != LBM_SUCCESS) return LBM_FAILURE;
  hipLaunchKernelGGL(lbm::steady_reset, dim3(1), dim3(64), 0, sl.compute, c->steady_state, 1, (lbm::SteadyBatch*)nullptr);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  if (begin() != LBM_SUCCESS) return LBM_FAILURE;

  const int n_seg = max_steps / E;
  const bool resident = c->plan.resident && E >= c->plan.resident_min_steps;
  // One segment of look-ahead where a segment is ONE launch of the resident kernel: it reads the lattice the segment in
  // front left and writes the other one, so dropping it is one flip of `cur`.  A longer segment (several launches, which
  // would write both lattices) runs for milliseconds; there the host waits for each verdict first, as on the per-pass path.
  const int depth = (resident && E <= kResidentChunk) ? 2 : 1;
  int waited = LBM_SUCCESS;
  const auto issue = [&](int index) {  // the segment, its check, and the stop word on its way to slot index & 1 of the pinned pair
    const int first = c->steps_done, slot = index & 1;
    return issue_segment(c, resident, E) == LBM_SUCCESS && check(index, first) == LBM_SUCCESS &&
           post_stop_word(&c->steady_state.get()->stop, c->steady_stop_host + slot, c->ev_steady[slot], sl.compute) == LBM_SUCCESS;
  };
  const auto judge = [&](int index) {
    bool stop = false;
    if ((waited = wait_stop_word(c->ev_steady[index & 1], c->steady_stop_host + (index & 1), &stop)) != LBM_SUCCESS) return lbm_segments::kBreak;
    if (stop) return lbm_segments::kStop;
    // a launch gave up (its status travels in front of the stop word): the context is failed, sync_ctx below reports it
    return resident && gave_up(c) != 0 ? lbm_segments::kBreak : lbm_segments::kGoOn;
  };
  const lbm_segments::Outcome o = lbm_segments::run(n_seg, depth, issue, judge);
  if (o.failed || waited != LBM_SUCCESS) return LBM_FAILURE;
  if (o.issued > o.judged) {
    // The look-ahead segment is dropped: its acceleration did not happen (accelerate_row_unless), its one launch wrote
    // the other lattice, everything enqueued behind that launch -- a sample, the check -- read the stop word first and
    // changed nothing, and its tot_u entries lie beyond steps_done.  Its seam granules carry the tags of steps that will
    // be run again, so they are cleared as at creation.
    c->cur ^= 1;
    c->steps_done -= E;
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(sl.res_gran, 0, resident_gran_bytes(c), sl.compute));
  }
  if (!o.stopped && !owner_failed(c) && max_steps - n_seg * E > 0) {
    // the rest of the cap, shorter than a segment: run as lbm_run runs it, not checked
    const int rest = max_steps - n_seg * E;
    if (run_passes(c, rest, c->plan.resident && rest >= c->plan.resident_min_steps, false) != LBM_SUCCESS) return LBM_FAILURE;
  }
  return sync_ctx(c);  // also reports a resident give-up
}

// One checked run of a batch that checked_batch_ok has passed, with begin() and check() as for a context; the checks set
// SteadyBatch::all_steady once every member has finished.  Per segment the launches of lbm_batch_run, then the check; the
// host waits for each verdict (a dropped segment of B lattices would cost more than the wait), which is the loop of
// lbm_segments::run at depth 1.  Finished members keep stepping with the others, so every whole segment that ran was checked.
static int checked_batch_run(lbm_batch* bt, int max_steps, int E, const std::function<int()>& begin, const std::function<int(int, int)>& check) {
  const int device = bt->members[0]->slab[0].device;
  HIP_TRY(LBM_FAILURE, hipSetDevice(device));
  if (steady_batch_buffers(bt) != LBM_SUCCESS) return LBM_FAILURE;
  if (begin() != LBM_SUCCESS) return LBM_FAILURE;
  const int n_seg = max_steps / E;
  bool stop = false;
  for (int index = 0; index < n_seg && !stop; index++) {
    const int first = bt->steps_done;
    if (lbm_batch_run(bt, E) != LBM_SUCCESS) return LBM_FAILURE;
    HIP_TRY(LBM_FAILURE, hipSetDevice(device));
    if (check(index, first) != LBM_SUCCESS) return LBM_FAILURE;
    if (post_stop_word(&bt->steady_batch.get()->all_steady, bt->steady_stop_host, bt->ev_steady, bt->stream) != LBM_SUCCESS) return LBM_FAILURE;
    if (wait_stop_word(bt->ev_steady, bt->steady_stop_host, &stop) != LBM_SUCCESS) return LBM_FAILURE;
    // a batched launch gave up (its status travels in front of the stop word): the batch is failed, sync_batch below reports it
    if (bt->resident && gave_up(bt->members[0]) != 0) break;
  }
  if (!stop && !owner_failed(bt) && max_steps - n_seg * E > 0 && lbm_batch_run(bt, max_steps - n_seg * E) != LBM_SUCCESS) return LBM_FAILURE;
  return sync_batch(bt);
}

// ---- ... on the average velocity: the check reads the segment's tot_u entries; SteadyState holds its state too
int lbm_run_until(lbm_ctx* c, int max_steps, int check_every, double tol, int patience, lbm_steady_result* out) {
  static const char who[] = "lbm_run_until";
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "%s: NULL argument", who);
  out->steps_run = 0;
  REFUSE_FAILED(LBM_FAILURE, c, who);
  if (checked_ctx_ok(c, who, "sums", max_steps, check_every, tol, patience) != LBM_SUCCESS) return LBM_FAILURE;
  const Slab& sl = c->slab[0];
  const int E = check_every, start = c->steps_done;
  const auto begin = [] { return LBM_SUCCESS; };  // steady_reset has done it
  const auto check = [&](int index, int first) {
    hipLaunchKernelGGL(lbm::steady_check, dim3(1), dim3(64), 0, sl.compute, (const double*)sl.tot_u, first, E, (float)c->fluid_cells, tol,
                       patience, (index + 1) * E, c->steady_state);
    return launched();
  };
  if (checked_run(c, max_steps, E, begin, check) != LBM_SUCCESS) return LBM_FAILURE;
  lbm::SteadyState st;
  HIP_TRY(LBM_FAILURE, hipMemcpy(&st, c->steady_state, sizeof(st), hipMemcpyDeviceToHost));
  steady_fill(out, st, c->steps_done - start);
  return LBM_SUCCESS;
}

int lbm_batch_run_until(lbm_batch* bt, int max_steps, int check_every, double tol, int patience, lbm_steady_result* out,
                        int* steps_run) {
  static const char who[] = "lbm_batch_run_until";
  if (!bt || !out || !steps_run) LBM_FAIL(LBM_FAILURE, "%s: NULL argument", who);
  *steps_run = 0;
  REFUSE_FAILED(LBM_FAILURE, bt, who);
  if (checked_batch_ok(bt, who, max_steps, check_every, tol, patience) != LBM_SUCCESS) return LBM_FAILURE;
  const int n_members = (int)bt->members.size(), E = check_every, start = bt->steps_done;
  const auto begin = [&]() -> int {
    if (!bt->steady_state) {  // allocated last: the set is whole (an attempt that failed half-way starts again)
      std::vector<lbm::SteadyMember> h((size_t)n_members);
      for (int i = 0; i < n_members; i++) h[(size_t)i] = {bt->members[(size_t)i]->slab[0].tot_u, (float)bt->members[(size_t)i]->fluid_cells};
      HIP_TRY(LBM_FAILURE, bt->steady_members.alloc(h.size()));
      HIP_TRY(LBM_FAILURE, hipMemcpy(bt->steady_members, h.data(), h.size() * sizeof(h[0]), hipMemcpyHostToDevice));
      HIP_TRY(LBM_FAILURE, bt->steady_state.alloc((size_t)n_members));
    }
    hipLaunchKernelGGL(lbm::steady_reset, dim3(ceil_div(n_members, 64)), dim3(64), 0, bt->stream, bt->steady_state, n_members,
                       bt->steady_batch);
    return launched();
  };
  const auto check = [&](int index, int first) {  // one check of every member
    hipLaunchKernelGGL(lbm::steady_check_batch, dim3(n_members), dim3(64), 0, bt->stream,
                       (const lbm::SteadyMember*)bt->steady_members, n_members, first, E, tol, patience, (index + 1) * E,
                       bt->steady_state, bt->steady_batch);
    return launched();
  };
  if (checked_batch_run(bt, max_steps, E, begin, check) != LBM_SUCCESS) return LBM_FAILURE;
  std::vector<lbm::SteadyState> st((size_t)n_members);
  HIP_TRY(LBM_FAILURE, hipMemcpy(st.data(), bt->steady_state, st.size() * sizeof(st[0]), hipMemcpyDeviceToHost));
  *steps_run = bt->steps_done - start;
  for (int i = 0; i < n_members; i++) steady_fill(&out[i], st[(size_t)i], *steps_run);
  return LBM_SUCCESS;
}

// ---- ... on the velocity residual: the check reads a sample of the lattice against the planes of the check before ----
// The history of a call on a context (bt null: one lattice) or on a batch: its arguments (no device needed; *rows = rows
// kept on the device), then room for them in `words` (`have` rows so far) on `device`, kept while it suffices.
static int until_history_begin(const char* who, DeviceBuf<long long>& words, size_t& have, const void* history, int history_capacity,
                               int n_seg, const lbm_batch* bt, int device, size_t* rows) {
  if (history_capacity < 0) LBM_FAIL(LBM_FAILURE, "%s: negative history capacity %d", who, history_capacity);
  const size_t n_members = bt ? bt->members.size() : 1;
  *rows = history ? (size_t)(history_capacity < n_seg ? history_capacity : n_seg) : 0;
  constexpr size_t kRowBytes = lbm_residual::kResidualWords * sizeof(long long);
  const size_t bytes = *rows * n_members * kRowBytes;
  if (bytes >= ((size_t)1 << 31))
    LBM_FAIL(LBM_FAILURE, "%s: a history of %zu rows of %zu lattices is %.2f GiB on the device, 2 GiB or more (%d bytes per lattice and row)", who,
             *rows, n_members, (double)bytes / 1073741824.0, (int)kRowBytes);
  if (*rows <= have) return LBM_SUCCESS;
  HIP_TRY(LBM_FAILURE, hipSetDevice(device));
  have = 0;
  if (words.alloc_bytes(bytes) != hipSuccess) {
    (void)hipGetLastError();
    if (bt)
      LBM_FAIL(LBM_FAILURE, "%s: cannot allocate a history of %zu rows of %zu members (%.1f MiB); nothing was run", who, *rows, n_members,
               (double)bytes / 1048576.0);
    LBM_FAIL(LBM_FAILURE, "%s: cannot allocate a history of %zu rows (%.1f MiB); nothing was run", who, *rows, (double)bytes / 1048576.0);
  }
  have = *rows;
  return LBM_SUCCESS;
}
// its first n rows of one lattice each, formed from the words after the run
static int until_history_read(const long long* device_words, size_t n, int nx, int span, lbm_residual_row* history) {
  constexpr size_t kWords = lbm_residual::kResidualWords;
  std::vector<long long> words(n * kWords);
  if (n > 0) HIP_TRY(LBM_FAILURE, hipMemcpy(words.data(), device_words, words.size() * sizeof(long long), hipMemcpyDeviceToHost));
  for (size_t j = 0; j < n; j++) history[j] = lbm_residual::residual_row_from_words(words.data() + j * kWords, 1, nx, span);
  return LBM_SUCCESS;
}

static void until_fill(lbm_residual_steady_result* out, const lbm_residual::UntilState& st, int steps_run, int nx, int span) {
  std::memset(out, 0, sizeof(*out));
  out->steps_run = steps_run;
  out->steady = st.stop == lbm_residual::kUntilSteady ? 1 : 0;
  out->steady_step = st.steady_step;
  out->checks = st.checks;
  out->diverged = st.stop == lbm_residual::kUntilDiverged ? 1 : 0;
  out->last_rel = st.last_rel;
  out->last = lbm_residual::residual_row_from_words(st.last, 1, nx, st.checks > 0 ? span : 0);  // (no check: zeros at -1, -1)
}

int lbm_run_until_residual(lbm_ctx* c, int max_steps, int check_every, double tol, int patience, lbm_residual_steady_result* out,
                           lbm_residual_row* history, int history_capacity) {
  static const char who[] = "lbm_run_until_residual";
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "%s: NULL argument", who);
  out->steps_run = 0;
  REFUSE_FAILED(LBM_FAILURE, c, who);
  if (checked_ctx_ok(c, who, "words", max_steps, check_every, tol, patience) != LBM_SUCCESS) return LBM_FAILURE;
  const Slab& sl = c->slab[0];
  const int E = check_every, start = c->steps_done;
  size_t hist_rows = 0;
  if (until_history_begin(who, c->until_history, c->until_history_rows, history, history_capacity, max_steps / E, nullptr, sl.device,
                          &hist_rows) != LBM_SUCCESS)
    return LBM_FAILURE;
  const auto begin = [&]() -> int {
    if (!c->until_state) {  // allocated last: the set is whole
      const size_t cells = (size_t)sl.rows * c->p.nx;
      if (c->until_planes.alloc(2 * cells) != hipSuccess) {
        (void)hipGetLastError();
        LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the remembered field (%zu cells, %.1f MiB); nothing was run", who, cells,
                 (double)(2 * cells * sizeof(float)) / 1048576.0);
      }
      HIP_TRY(LBM_FAILURE, c->until_words.alloc(lbm_residual::kResidualWords));
      HIP_TRY(LBM_FAILURE, c->until_state.alloc(1));
    }
    hipLaunchKernelGGL(lbm::residual_until_reset, dim3(1), dim3(64), 0, sl.compute, c->until_state.get(), c->until_words.get(), 1,
                       (lbm::SteadyBatch*)nullptr);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    launch_residual_gather(c, sl, c->until_planes, c->until_words, true);  // the baseline: the field of the current lattice into the call's planes
    return launched();
  };
  const auto check = [&](int index, int) -> int {  // the sample of the lattice the segment left, standing back behind a stop, and its check
    launch_residual_gather(c, sl, c->until_planes, c->until_words, false, c->steady_state);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    long long* hist = (size_t)index < hist_rows ? c->until_history + (size_t)index * lbm_residual::kResidualWords : nullptr;
    hipLaunchKernelGGL(lbm::residual_check, dim3(1), dim3(64), 0, sl.compute, c->until_words.get(), hist, tol, patience, (index + 1) * E,
                       c->until_state.get(), c->steady_state.get());
    return launched();
  };
  if (checked_run(c, max_steps, E, begin, check) != LBM_SUCCESS) return LBM_FAILURE;
  lbm_residual::UntilState st;
  HIP_TRY(LBM_FAILURE, hipMemcpy(&st, c->until_state, sizeof(st), hipMemcpyDeviceToHost));
  until_fill(out, st, c->steps_done - start, c->p.nx, E);
  return until_history_read(c->until_history, std::min((size_t)st.checks, hist_rows), c->p.nx, E, history);
}

int lbm_batch_run_until_residual(lbm_batch* bt, int max_steps, int check_every, double tol, int patience, lbm_residual_steady_result* out,
                                 int* steps_run, lbm_residual_row* history, int history_capacity) {
  static const char who[] = "lbm_batch_run_until_residual";
  if (!bt || !out || !steps_run) LBM_FAIL(LBM_FAILURE, "%s: NULL argument", who);
  *steps_run = 0;
  REFUSE_FAILED(LBM_FAILURE, bt, who);
  if (checked_batch_ok(bt, who, max_steps, check_every, tol, patience) != LBM_SUCCESS) return LBM_FAILURE;
  const lbm_ctx* c0 = bt->members[0];
  const Slab& sl0 = c0->slab[0];
  const size_t n_members = bt->members.size(), row_words = n_members * (size_t)lbm_residual::kResidualWords;
  const int E = check_every, start = bt->steps_done;
  size_t hist_rows = 0;
  if (until_history_begin(who, bt->until_history, bt->until_history_rows, history, history_capacity, max_steps / E, bt, sl0.device,
                          &hist_rows) != LBM_SUCCESS)
    return LBM_FAILURE;
  const auto begin = [&]() -> int {
    // (a shape the resident kernel does not take: the gather still reads the members' lattices from the table)
    if (!bt->table && !upload_member_table(bt)) LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the member table; nothing was run", who);
    if (!bt->until_state) {  // allocated last: the set is whole
      const size_t cells = (size_t)sl0.rows * c0->p.nx;
      if (bt->until_planes.alloc(n_members * 2 * cells) != hipSuccess) {
        (void)hipGetLastError();
        LBM_FAIL(LBM_FAILURE, "%s: cannot allocate the remembered fields of %zu members (%zu cells each, %.1f MiB); nothing was run", who,
                 n_members, cells, (double)(n_members * 2 * cells * sizeof(float)) / 1048576.0);
      }
      HIP_TRY(LBM_FAILURE, bt->until_words.alloc(row_words));
      HIP_TRY(LBM_FAILURE, bt->until_state.alloc(n_members));
    }
    hipLaunchKernelGGL(lbm::residual_until_reset, dim3(ceil_div((long)n_members, 64)), dim3(64), 0, bt->stream, bt->until_state.get(),
                       bt->until_words.get(), (int)n_members, bt->steady_batch.get());
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    return launch_batch_residual(bt, bt->until_planes, nullptr, true);  // the baselines: one launch
  };
  const auto check = [&](int index, int) -> int {  // ONE sample launch and ONE check launch for all members; finished members are still sampled
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(bt->until_words, 0, row_words * sizeof(long long), bt->stream));
    if (launch_batch_residual(bt, bt->until_planes, bt->until_words, false) != LBM_SUCCESS) return LBM_FAILURE;
    long long* hist = (size_t)index < hist_rows ? bt->until_history + (size_t)index * row_words : nullptr;
    hipLaunchKernelGGL(lbm::residual_check_batch, dim3((unsigned)n_members), dim3(64), 0, bt->stream, bt->until_words.get(), hist,
                       (int)n_members, tol, patience, (index + 1) * E, bt->until_state.get(), bt->steady_batch.get());
    return launched();
  };
  if (checked_batch_run(bt, max_steps, E, begin, check) != LBM_SUCCESS) return LBM_FAILURE;
  std::vector<lbm_residual::UntilState> st(n_members);
  HIP_TRY(LBM_FAILURE, hipMemcpy(st.data(), bt->until_state, st.size() * sizeof(st[0]), hipMemcpyDeviceToHost));
  *steps_run = bt->steps_done - start;
  for (size_t i = 0; i < n_members; i++) until_fill(&out[i], st[i], *steps_run, c0->p.nx, E);
  // (every whole segment that ran was checked, and the history holds a row of each while it has room)
  return until_history_read(bt->until_history, std::min((size_t)(*steps_run / E), hist_rows) * n_members, c0->p.nx, E, history);
}

}  // extern "C"

// the double-precision engine (lbm_double_*): a handle type, entry points and kernels of its own
#include "lbm_double.hip.h"
