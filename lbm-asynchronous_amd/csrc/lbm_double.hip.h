// lbm_double.hip.h -- host side of the double-precision engine (lbm_double_* of include/lbm_hip.h).  Included at the end of
// lbm_hip.hip, whose error handling (LBM_FAIL, HIP_TRY) and owning handles (DeviceBuf, Stream, Event) it uses; the
// kernels are lbm_kernels_double.hip.h.  Nothing here touches an lbm_ctx: a double context is a type of its own, one
// periodic slab on device 0, one stream, one timestep per launch.
#pragma once
#include "lbm_kernels_double.hip.h"

namespace {
constexpr int kPartSlotsD = 64;  // steps whose per-workgroup partial sums wait in the ring before one reduce launch
constexpr int kSumBlocksD = 256;
}  // namespace

// streams first: members go in reverse order of declaration, so the stream outlives the buffers its work used
struct lbm_double_ctx {
  lbm_params_double p{};
  int device = 0;
  Stream stream;
  Event ev_t0, ev_t1;
  DeviceBuf<double> lat[2];         // the two lattices; lat[cur] is the current one
  DeviceBuf<unsigned char> mask;    // ny x pitch
  DeviceBuf<double> tot_u;          // capacity entries: per-step sum of |u|
  DeviceBuf<double> partials;       // kPartSlotsD x n_blocks
  DeviceBuf<double> scratch;        // 2 x kSumBlocksD: lattice_sums_d
  int cur = 0;
  int pitch = 0;                    // doubles between planes = bytes between mask rows
  int capacity = 0;
  int fluid_cells = 0;
  int steps_done = 0;
  int lane_cells = 2;
  int nts = 0;
  int n_blocks = 0;                 // workgroups of one step launch
};

namespace {

lbm::LatticeArgsD lattice_args_d(const lbm_double_ctx* c, const double* src, double* dst) {
  lbm::LatticeArgsD a;
  a.src = src;
  a.dst = dst;
  a.mask = c->mask;
  a.plane_stride = c->pitch;
  a.row_pitch = 9L * c->pitch;
  a.pitch = c->pitch;
  a.nx = c->p.nx;
  return a;
}

bool validate_params_d(const lbm_params_double* p) {
  // the cell count must fit the reference's int counters (tot_cells, SerialCode/d2q9-bgk.c:411)
  return p && p->nx >= 1 && p->ny >= 2 && p->max_iters >= 0 && (long)p->nx * (long)p->ny <= 2147483647L;
}

int build_double(lbm_double_ctx* c, const int* obstacles, const double* cells_aos) {
  const lbm_params_double& p = c->p;
  const long cells = (long)p.nx * p.ny;
  HIP_TRY(LBM_FAILURE, hipSetDevice(c->device));
  HIP_TRY(LBM_FAILURE, c->stream.create());
  HIP_TRY(LBM_FAILURE, c->ev_t0.create(hipEventDefault));
  HIP_TRY(LBM_FAILURE, c->ev_t1.create(hipEventDefault));
  const size_t lat_doubles = (size_t)p.ny * 9 * (size_t)c->pitch;
  for (int i = 0; i < 2; i++) {
    HIP_TRY(LBM_FAILURE, c->lat[i].alloc(lat_doubles));
    HIP_TRY(LBM_FAILURE, hipMemsetAsync(c->lat[i], 0, lat_doubles * sizeof(double), c->stream));
  }
  const size_t cap = (size_t)(c->capacity > 0 ? c->capacity : 1);
  HIP_TRY(LBM_FAILURE, c->tot_u.alloc(cap));
  HIP_TRY(LBM_FAILURE, hipMemsetAsync(c->tot_u, 0, cap * sizeof(double), c->stream));
  HIP_TRY(LBM_FAILURE, c->partials.alloc((size_t)kPartSlotsD * c->n_blocks));
  HIP_TRY(LBM_FAILURE, c->scratch.alloc(2 * kSumBlocksD));
  // obstacle mask: the fp32 engine's uint8 rows, built on the device from the int map
  const size_t mask_bytes = (size_t)p.ny * c->pitch;
  HIP_TRY(LBM_FAILURE, c->mask.alloc(mask_bytes));
  HIP_TRY(LBM_FAILURE, hipMemsetAsync(c->mask, 0, mask_bytes, c->stream));
  {
    DeviceBuf<int> stage;
    HIP_TRY(LBM_FAILURE, stage.alloc((size_t)cells));
    HIP_TRY(LBM_FAILURE, hipMemcpyAsync(stage, obstacles, (size_t)cells * sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(lbm::mask_from_int, dim3(ceil_div(cells, 256)), dim3(256), 0, c->stream, stage.get(), c->mask.get(), p.nx,
                       c->pitch, p.ny);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->stream));
  }
  const lbm::LatticeArgsD a = lattice_args_d(c, c->lat[0], c->lat[0]);
  if (cells_aos) {
    long chunk_rows = (64L << 20) / ((long)p.nx * lbm::kQ * (long)sizeof(double));
    if (chunk_rows < 1) chunk_rows = 1;
    if (chunk_rows > p.ny) chunk_rows = p.ny;
    DeviceBuf<double> stage;
    HIP_TRY(LBM_FAILURE, stage.alloc((size_t)chunk_rows * p.nx * lbm::kQ));
    for (int r0 = 0; r0 < p.ny; r0 += (int)chunk_rows) {
      const int nr = (p.ny - r0 < chunk_rows) ? p.ny - r0 : (int)chunk_rows;
      const size_t n = (size_t)nr * p.nx * lbm::kQ;
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(stage, cells_aos + (size_t)r0 * p.nx * lbm::kQ, n * sizeof(double),
                                          hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(lbm::aos_to_soa_d, dim3(ceil_div((long)n, 256)), dim3(256), 0, c->stream, stage.get(), a, r0, nr);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
      HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->stream));
    }
  } else {
    // SerialCode/d2q9-bgk.c:546-548 read as double
    const double w0 = p.density * 4.0 / 9.0, w1 = p.density / 9.0, w2 = p.density / 36.0;
    hipLaunchKernelGGL(lbm::init_equilibrium_d, dim3(ceil_div(cells, 256)), dim3(256), 0, c->stream, a, p.ny, w0, w1, w2);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->stream));
  }
  return LBM_SUCCESS;
}

int run_double(lbm_double_ctx* c, int n_steps, float* kernel_ms, const char* who) {
  if (!c) LBM_FAIL(LBM_FAILURE, "%s: null context", who);
  if (n_steps < 0) LBM_FAIL(LBM_FAILURE, "%s: negative step count", who);
  if (kernel_ms) *kernel_ms = 0.f;
  if (n_steps == 0) return LBM_SUCCESS;
  if (c->steps_done + n_steps > c->capacity)
    LBM_FAIL(LBM_FAILURE, "%s: %d steps requested but the av_vels record holds %d (maxIters)", who,
             c->steps_done + n_steps, c->capacity);
  HIP_TRY(LBM_FAILURE, hipSetDevice(c->device));
  const lbm_params_double& p = c->p;
  const int lid = p.ny - 2;
  const double a1 = p.density * p.accel / 9.0, a2 = p.density * p.accel / 36.0;  // SerialCode/d2q9-bgk.c:219-220
  if (kernel_ms) HIP_TRY(LBM_FAILURE, hipEventRecord(c->ev_t0, c->stream));
  // the first step's accelerate_flow; the later ones come from the epilogue of the step before
  hipLaunchKernelGGL(lbm::accelerate_row_d, dim3(ceil_div(p.nx, 256)), dim3(256), 0, c->stream,
                     lattice_args_d(c, c->lat[c->cur], c->lat[c->cur]), lid, a1, a2);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  for (int t = 0; t < n_steps; t++) {
    const int slot = t % kPartSlotsD;
    lbm::StepArgsD a;
    static_cast<lbm::LatticeArgsD&>(a) = lattice_args_d(c, c->lat[c->cur], c->lat[c->cur ^ 1]);
    a.rows = p.ny;
    a.accel_row = (t + 1 < n_steps) ? lid : lbm::kNoRow;
    a.omega = p.omega;
    a.a1 = a1;
    a.a2 = a2;
    a.partials = c->partials + (size_t)slot * c->n_blocks;
    auto kernel = c->lane_cells == 1 ? lbm::step_double_scalar : (c->nts ? lbm::step_double<true> : lbm::step_double<false>);
    hipLaunchKernelGGL(kernel, dim3(c->n_blocks), dim3(lbm::kBlock), 0, c->stream, a);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    c->cur ^= 1;
    if (slot == kPartSlotsD - 1 || t == n_steps - 1) {
      hipLaunchKernelGGL(lbm::reduce_partials_d, dim3(slot + 1), dim3(lbm::kBlock), 0, c->stream, c->partials.get(),
                         c->n_blocks, (long)c->n_blocks, c->tot_u.get(), c->steps_done + t - slot);
      HIP_TRY(LBM_FAILURE, hipGetLastError());
    }
  }
  c->steps_done += n_steps;
  if (kernel_ms) {
    HIP_TRY(LBM_FAILURE, hipEventRecord(c->ev_t1, c->stream));
    HIP_TRY(LBM_FAILURE, hipEventSynchronize(c->ev_t1));
    float ms = 0.f;
    HIP_TRY(LBM_FAILURE, hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
    *kernel_ms = ms / (float)n_steps;
  }
  return LBM_SUCCESS;
}

// sums of |u| over fluid cells and of density over all cells of the current lattice
int lattice_totals_d(lbm_double_ctx* c, double* speed, double* mass) {
  HIP_TRY(LBM_FAILURE, hipSetDevice(c->device));
  double h[2 * kSumBlocksD];
  hipLaunchKernelGGL(lbm::lattice_sums_d, dim3(kSumBlocksD), dim3(lbm::kBlock), 0, c->stream,
                     lattice_args_d(c, c->lat[c->cur], c->lat[c->cur]), c->p.ny, c->scratch.get(), c->scratch + kSumBlocksD);
  HIP_TRY(LBM_FAILURE, hipGetLastError());
  HIP_TRY(LBM_FAILURE, hipMemcpyAsync(h, c->scratch, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->stream));
  double s = 0.0, m = 0.0;
  for (int i = 0; i < kSumBlocksD; i++) { s += h[i]; m += h[kSumBlocksD + i]; }
  *speed = s;
  *mass = m;
  return LBM_SUCCESS;
}

}  // namespace

extern "C" {

void lbm_double_destroy(lbm_double_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  delete c;
}

lbm_double_ctx* lbm_double_create(const lbm_params_double* params, const int* obstacles, const double* cells_aos) {
  if (!validate_params_d(params)) LBM_FAIL(nullptr, "lbm_double_create: invalid parameters");
  if (!obstacles) LBM_FAIL(nullptr, "lbm_double_create: obstacles is NULL");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    LBM_FAIL(nullptr, "lbm_double_create: no HIP device available (this library has no CPU path)");
  lbm_double_ctx* c = new lbm_double_ctx();
  c->p = *params;
  c->capacity = params->max_iters;
  c->pitch = (int)round_up(params->nx, 64);
  const long cells = (long)params->nx * params->ny;
  long blocked = 0;
  for (long i = 0; i < cells; i++) blocked += obstacles[i] ? 1 : 0;
  c->fluid_cells = (int)(cells - blocked);
  // two cells per lane wherever a row is made of pairs (LBM_DOUBLE_LANE_CELLS=1: the one-cell kernel, for comparison)
  c->lane_cells = (params->nx % 2 == 0 && env_int("LBM_DOUBLE_LANE_CELLS", 2) != 1) ? 2 : 1;
  // nontemporal stores pay once the two lattices no longer fit the 256 MiB Infinity Cache (the fp32 plan's rule)
  const double pair_bytes = 2.0 * 9.0 * sizeof(double) * (double)c->pitch * params->ny;
  c->nts = env_int("LBM_DOUBLE_NTS", pair_bytes > 512.0 * 1024 * 1024 ? 1 : 0) ? 1 : 0;
  c->n_blocks = (int)ceil_div(cells / c->lane_cells, lbm::kBlock);
  if (build_double(c, obstacles, cells_aos) != LBM_SUCCESS) {
    (void)hipGetLastError();
    lbm_double_destroy(c);
    return nullptr;
  }
  return c;
}

int lbm_double_get_info(const lbm_double_ctx* c, lbm_double_info* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_double_get_info: NULL argument");
  out->fluid_cells = c->fluid_cells;
  out->steps_done = c->steps_done;
  out->lane_cells = c->lane_cells;
  out->nontemporal = c->lane_cells == 2 ? c->nts : 0;
  return LBM_SUCCESS;
}

int lbm_double_run(lbm_double_ctx* c, int n_steps) { return run_double(c, n_steps, nullptr, "lbm_double_run"); }

int lbm_double_run_timed(lbm_double_ctx* c, int n_steps, float* kernel_ms_per_step) {
  if (!kernel_ms_per_step) LBM_FAIL(LBM_FAILURE, "lbm_double_run_timed: NULL output");
  return run_double(c, n_steps, kernel_ms_per_step, "lbm_double_run_timed");
}

int lbm_double_sync(lbm_double_ctx* c) {
  if (!c) LBM_FAIL(LBM_FAILURE, "lbm_double_sync: null context");
  HIP_TRY(LBM_FAILURE, hipSetDevice(c->device));
  HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->stream));
  return LBM_SUCCESS;
}

int lbm_double_read_av_vels(lbm_double_ctx* c, double* out, int n) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_double_read_av_vels: NULL argument");
  if (n < 0 || n > c->steps_done) LBM_FAIL(LBM_FAILURE, "lbm_double_read_av_vels: %d steps requested, %d recorded", n, c->steps_done);
  if (n == 0) return LBM_SUCCESS;
  if (lbm_double_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  HIP_TRY(LBM_FAILURE, hipMemcpy(out, c->tot_u, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  const double cells = (double)c->fluid_cells;
  for (int t = 0; t < n; t++) out[t] = out[t] / cells;  // SerialCode/d2q9-bgk.c:457
  return LBM_SUCCESS;
}

int lbm_double_read_cells(lbm_double_ctx* c, double* cells_aos) {
  if (!c || !cells_aos) LBM_FAIL(LBM_FAILURE, "lbm_double_read_cells: NULL argument");
  if (lbm_double_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  const int nx = c->p.nx, ny = c->p.ny;
  long chunk_rows = (64L << 20) / ((long)nx * lbm::kQ * (long)sizeof(double));
  if (chunk_rows < 1) chunk_rows = 1;
  if (chunk_rows > ny) chunk_rows = ny;
  DeviceBuf<double> stage;
  HIP_TRY(LBM_FAILURE, stage.alloc((size_t)chunk_rows * nx * lbm::kQ));
  const lbm::LatticeArgsD a = lattice_args_d(c, c->lat[c->cur], c->lat[c->cur]);
  for (int r0 = 0; r0 < ny; r0 += (int)chunk_rows) {
    const int nr = (ny - r0 < chunk_rows) ? ny - r0 : (int)chunk_rows;
    const size_t n = (size_t)nr * nx * lbm::kQ;
    hipLaunchKernelGGL(lbm::soa_to_aos_d, dim3(ceil_div((long)n, 256)), dim3(256), 0, c->stream, a, stage.get(), r0, nr);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    HIP_TRY(LBM_FAILURE, hipMemcpyAsync(cells_aos + (size_t)r0 * nx * lbm::kQ, stage, n * sizeof(double), hipMemcpyDeviceToHost,
                                        c->stream));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->stream));
  }
  return LBM_SUCCESS;
}

int lbm_double_read_final_state(lbm_double_ctx* c, double* u_x, double* u_y, double* u_mag, double* pressure) {
  if (!c || !u_x || !u_y || !u_mag || !pressure) LBM_FAIL(LBM_FAILURE, "lbm_double_read_final_state: NULL argument");
  if (lbm_double_sync(c) != LBM_SUCCESS) return LBM_FAILURE;
  const int nx = c->p.nx, ny = c->p.ny;
  long chunk_rows = (16L << 20) / ((long)nx * (long)sizeof(double));
  if (chunk_rows < 1) chunk_rows = 1;
  if (chunk_rows > ny) chunk_rows = ny;
  double* outs[4] = {u_x, u_y, u_mag, pressure};
  DeviceBuf<double> stage;
  const size_t chunk_cells = (size_t)chunk_rows * nx;
  HIP_TRY(LBM_FAILURE, stage.alloc(4 * chunk_cells));
  const lbm::LatticeArgsD a = lattice_args_d(c, c->lat[c->cur], c->lat[c->cur]);
  for (int r0 = 0; r0 < ny; r0 += (int)chunk_rows) {
    const int nr = (ny - r0 < chunk_rows) ? ny - r0 : (int)chunk_rows;
    const size_t n = (size_t)nr * nx;
    hipLaunchKernelGGL(lbm::final_state_d, dim3(ceil_div((long)n, 256)), dim3(256), 0, c->stream, a, r0, nr, c->p.density,
                       stage.get(), stage + chunk_cells, stage + 2 * chunk_cells, stage + 3 * chunk_cells);
    HIP_TRY(LBM_FAILURE, hipGetLastError());
    for (int k = 0; k < 4; k++)
      HIP_TRY(LBM_FAILURE, hipMemcpyAsync(outs[k] + (size_t)r0 * nx, stage + k * chunk_cells, n * sizeof(double),
                                          hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(LBM_FAILURE, hipStreamSynchronize(c->stream));
  }
  return LBM_SUCCESS;
}

int lbm_double_av_velocity(lbm_double_ctx* c, double* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_double_av_velocity: NULL argument");
  double speed, mass;
  if (lattice_totals_d(c, &speed, &mass) != LBM_SUCCESS) return LBM_FAILURE;
  *out = speed / (double)c->fluid_cells;
  return LBM_SUCCESS;
}

int lbm_double_total_density(lbm_double_ctx* c, double* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_double_total_density: NULL argument");
  double speed, mass;
  if (lattice_totals_d(c, &speed, &mass) != LBM_SUCCESS) return LBM_FAILURE;
  *out = mass;
  return LBM_SUCCESS;
}

int lbm_double_calc_reynolds(lbm_double_ctx* c, double* out) {
  if (!c || !out) LBM_FAIL(LBM_FAILURE, "lbm_double_calc_reynolds: NULL argument");
  double av;
  if (lbm_double_av_velocity(c, &av) != LBM_SUCCESS) return LBM_FAILURE;
  const double viscosity = 1.0 / 6.0 * (2.0 / c->p.omega - 1.0);  // SerialCode/d2q9-bgk.c:639
  *out = av * c->p.reynolds_dim / viscosity;                      // :641
  return LBM_SUCCESS;
}

}  // extern "C"
