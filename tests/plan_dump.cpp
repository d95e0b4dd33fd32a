// plan_dump: prints what lbm_plan.h decides for one context, as one JSON object -- "plan" and "slabs", the fields of
// tests/golden/kernel_plans.json, and "stream_rows", the stream-kernel instantiations an exact context with this plan
// launches (tests/stream_rows.py), and "resident_form", the shape of the resident kernel it launches
// (tests/resident_forms.py).  Host arithmetic only; the LBM_* knobs come from the environment.
//   plan_dump nx ny world rank n_slabs halo cus n_devices distinct_devices
// halo: 0 none, 1 device copies, 2 RCCL, 3 the host's message passing (lbm_plan::HaloKind)
#include "../lbm-asynchronous_amd/csrc/lbm_plan.h"

#include <cstdio>

int main(int argc, char** argv) {
  if (argc != 10) {
    fprintf(stderr, "usage: %s nx ny world rank n_slabs halo cus n_devices distinct_devices\n", argv[0]);
    return 2;
  }
  lbm_plan::PlanInput in;
  in.nx = atoi(argv[1]);
  in.ny = atoi(argv[2]);
  in.world = atoi(argv[3]);
  in.rank = atoi(argv[4]);
  in.n_slabs = atoi(argv[5]);
  in.halo = atoi(argv[6]);
  in.cus = atoi(argv[7]);
  in.n_devices = atoi(argv[8]);
  in.distinct_devices = atoi(argv[9]) != 0;
  if (in.nx < 1 || in.ny < 2 || in.world < 1 || in.rank < 0 || in.rank >= in.world || in.n_slabs < 1 ||
      in.n_slabs > lbm_plan::kMaxSlabs || in.halo < 0 || in.halo > 3) {
    fprintf(stderr, "plan_dump: bad arguments\n");
    return 2;
  }
  const lbm_plan::KernelPlan p = lbm_plan::plan_kernels(in);
  printf("{\"plan\":{\"vec4\":%d,\"neigh\":%d,\"nts\":%d,\"snake\":%d,\"fuse2\":%d,\"pass_steps\":%d,\"lane_cells\":%d,"
         "\"halo_lanes\":%d,\"n_strips\":%d,\"packed\":%d,\"lds_windows\":%d,\"prefetch\":%d,\"xcd_chunk\":%d,\"use_stepk\":%d,"
         "\"band_groups\":%d,\"band_rows\":%d,\"tile_steps\":%d,\"tile_shape\":%d,\"part_stride\":%ld,\"use_graph\":%d,\"want_team\":%d,"
         "\"resident\":%d,\"resident_rows\":%d,\"resident_bands\":%d,\"resident_joint\":%d,\"resident_group\":%d,\"resident_one_xcd\":%d,"
         "\"resident_min_steps\":%d,\"resident_timeout\":%lld},\"slabs\":[",
         p.vec4 ? 1 : 0, p.neigh, p.nts, p.snake, p.fuse2, p.pass_steps, p.lane_cells, p.halo_lanes, p.n_strips, p.packed,
         p.lds_windows, p.prefetch, p.xcd_chunk, p.use_stepk, p.band_groups, p.band_rows, p.tile_steps, p.tile_shape, p.part_stride,
         p.use_graph, p.want_team, p.resident, p.resident_rows, p.resident_bands, p.resident_joint, p.resident_group,
         p.resident_one_xcd, p.resident_min_steps, p.resident_timeout);
  for (int s = 0; s < in.n_slabs; s++) {
    const lbm_plan::SlabRows sl = lbm_plan::slab_rows(in, p.vec4, s);
    printf("%s{\"rows\":%d,\"accel_row\":%d,\"accel_row2\":%d,\"blocks_main\":%d,\"blocks_boundary\":%d}", s ? "," : "", sl.rows,
           sl.accel_row, sl.accel_row2, sl.blocks_main, sl.blocks_boundary);
  }
  // the stream kernels an exact context with this plan launches (lbm_plan::stream_row): the full pass at pass_steps,
  // the two-step pass of a remainder of two or three, and -- not a stream kernel -- the one-step kernel of the odd last
  // step.  Empty where no stream kernel runs (no fuse2, or LDS tiles on a periodic slab).
  printf("],\"stream_rows\":[");
  if (p.fuse2 && !(p.tile_steps && in.halo == lbm_plan::HALO_SELF)) {
    static const char* const family[] = {"step2_stream", "stepk_stream", "stepk_pk", "stepk_pk1"};
    for (int i = 0; i < 2; i++) {
      const lbm_plan::StreamRow r = lbm_plan::stream_row(p, i == 0 ? p.pass_steps : 2, true);
      printf("{\"family\":\"%s\",\"math\":%d,\"nts\":%d,\"lane_cells\":%d,\"k\":%d,\"prefetch\":%d,\"lds\":%d},", family[r.family],
             r.math, r.nts, r.lane_cells, r.k, r.prefetch, r.lds);
    }
    printf("{\"family\":\"%s\",\"math\":0,\"nts\":%d,\"neigh\":%d}", p.vec4 ? "step_vec4" : "step_scalar", p.nts, p.neigh);
  }
  // the shape of lbm::resident_band a context with this plan launches (lbm_plan::resident_form), -1 without the resident kernel
  printf("],\"resident_form\":%d}\n", p.resident ? lbm_plan::resident_form(in.nx, p.resident_rows, p.resident_joint) : -1);
  return 0;
}
