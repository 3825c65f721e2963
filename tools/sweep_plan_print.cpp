// tools/sweep_plan_print.cpp — the tile plan of one whole-field launch of the overlapped-strip sweep, printed: what
// csrc/sweep_plan.cpp makes of the arguments, which are SweepPlanIn's (part 0).  No device, no HIP; compiled with plain
// g++ beside csrc/sweep_plan.cpp, as tools/sweep_plan_host_check.cpp is.  tests/test_sweep_plan_shapes_host.py pins the
// tables of the shapes whose GPU tests count on a tail and on all eight regions.
//   sweep_plan_print nx ny T div_mode bc rows_per_chunk tuned_rows tail_split wide      (bc: four of d n p, as "dddd")
// prints  plan: nregions ntiles tail_blocks nblocks rows nstrips wide
// and per region  region: t_end strip0 nstrip j0 j1 ry x0 wide
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sweep_plan.hpp"

int main(int argc, char** argv) {
    if (argc != 10 || std::strlen(argv[5]) != 4) {
        std::fprintf(stderr, "usage: %s nx ny T div_mode bc rows_per_chunk tuned_rows tail_split wide\n", argv[0]);
        return 2;
    }
    csim::SweepPlanIn in{};
    in.nx = std::atoi(argv[1]), in.ny = std::atoi(argv[2]), in.T = std::atoi(argv[3]), in.div_mode = std::atoi(argv[4]);
    for (int k = 0; k < 4; ++k) {
        const char c = argv[5][k];
        if (c != 'd' && c != 'n' && c != 'p') return 2;
        in.kind[k] = c == 'd' ? CSIM_BC_DIRICHLET : c == 'n' ? CSIM_BC_NEUMANN : CSIM_BC_PERIODIC;
    }
    in.part = 0;
    in.rows_per_chunk = std::atoi(argv[6]), in.tuned_rows = std::atoi(argv[7]), in.tail_split = std::atoi(argv[8]);
    in.frame_rows = 0;
    in.wide = std::atoi(argv[9]);
    if (in.nx < 1 || in.ny < 1 || in.T < 2 || in.T > csim::MAX_FUSE) return 2;
    const csim::SweepPlan p = csim::sweep_plan(in);
    std::printf("plan: %d %d %d %d %d %d %d\n", p.tl.nregions, p.tl.ntiles, p.tl.tail_blocks, p.nblocks, p.rows, p.nstrips,
                static_cast<int>(p.wide));
    for (int q = 0; q < p.tl.nregions && q < 8; ++q) {
        const csim::TileRegion& r = p.tl.r[q];
        std::printf("region: %d %d %d %d %d %d %d %d\n", r.t_end, r.strip0, r.nstrip, r.j0, r.j1, r.ry, r.x0, r.wide);
    }
    return 0;
}
