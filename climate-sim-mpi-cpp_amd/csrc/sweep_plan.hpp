// sweep_plan.hpp — how a launch of the overlapped-strip sweep is cut into tiles: host arithmetic without a device or
// the HIP headers (sweep_plan.cpp).  The geometry of a strip and the rounding rules are constexpr functions of plain
// ints, which the device side (sweep_core.hpp: OverlapGeom, SPECIALISE_EDGES) turns into compile-time constants;
// sweep_plan() is everything a launcher decides before it fills the kernel's arguments.
// tools/sweep_plan_host_check.cpp compiles it with plain g++, restates the kernel's tile decode and checks every plan
// of its enumeration on the CPU (tools/obsop_sanitize.sh: under AddressSanitizer + UndefinedBehaviorSanitizer).
#pragma once

#include "csim.h"

namespace csim {

// columns one wavefront covers per row: 64 lanes x NC doubles.  NC = 2 everywhere but in the WIDE strips of an interior
// without a screen (sweepO_march, NC = 4), which pay the same lane shifts and the same overlap for twice the columns
constexpr int wave_cols(int NC) { return 64 * NC; }
constexpr int WAVE_COLS = wave_cols(2);
constexpr int MAX_FUSE = 7;     // deepest temporal blocking (123 VGPRs: still 4 waves/SIMD; 8 would drop to 3)

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// strips of T steps per pass overlap by 2 * TP columns (see VAR_OVERLAP in sweep_core.hpp)
constexpr int strip_overlap(int T) { return 2 * ((T + 1) / 2); }                  // TP: T rounded up to even
constexpr int strip_stride(int T, int NC = 2) { return wave_cols(NC) - 2 * strip_overlap(T); }  // output columns per wavefront

// the march runs whole groups of six iterations: `rows` rounded up so that rows + 2 (T - 1) is a multiple of six
constexpr int whole_groups(int T, int rows) { return rows + (6 - (rows + 2 * (T - 1)) % 6) % 6; }

// Which instantiations get the straight-line edge flavours (seven more march bodies, ~13 KB of code each): the
// arithmetic modes and depths that long runs are made of.  The others (IEEE division, contracted arithmetic, the
// shallow depths of remainder passes) run every edge tile through the generic body, as round 2 did.
constexpr bool specialise_edges(int div, int T) { return (div == 0 || div == 1) && T >= 4; }

// Which instantiations exist with wide strips (k_sweepO_dpp<..., WIDE>): the depths long runs of large fields are made of
constexpr bool wide_strips_compiled(int div, int T) { return specialise_edges(div, T) && (T == 6 || T == 7); }

// Tiles of one launch: up to four rectangular regions of (strip, chunk) tiles, numbered
// consecutively; wavefront w of block b owns tile 4 b + w.  One region (all strips x all rows) is
// the whole-field launch; a multi-rank pass splits the field into the FRAME (bottom band, top
// band, left strip(s), right strip(s): thin tiles, finished early so that the faces can travel
// while the rest computes) and the BULK (everything else).
struct TileRegion {
    int t_end;          // tiles [t_end of the previous region, t_end)
    int strip0, nstrip; // strips strip0 .. strip0 + nstrip - 1 (narrow regions that start at column 0: of the field's
                        // narrow strips; otherwise in the order left, wide, right of a wide plan)
    int j0, j1, ry;     // rows j0 .. j1 in chunks of ry
    int x0, wide;       // first output column (0-based interior index) of the region's first strip; 1: its strips are
                        // wide (4 columns per lane, strip_stride(T, 4) apart), 0: narrow
};
struct Tiling {
    TileRegion r[8];
    int nregions, ntiles;
    // merged launch (frame + bulk in one grid): tiles [0, frame_tiles) are the frame, owned by blocks
    // [0, frame_blocks) in plain order so that they are dispatched first and spread over all XCDs; the
    // bulk tiles follow from tile 4 * frame_blocks on, XCD-remapped among themselves.  0 = not merged.
    int frame_tiles, frame_blocks;
    // TAIL region: the last tail_blocks blocks own, in plain order, the tiles of the last region(s) — the top
    // eighth of the (bulk of the) field cut into chunks of half the height, dispatched last, so that the
    // chip drains in half-height steps instead of idling behind the last full-height wavefronts
    // (17 468 wavefronts are 4.26 rounds of 4096 slots on 16384^2: the partial last round was 7 % of the
    // launch).  The main tiles before them fill their blocks exactly and are XCD-remapped.  0 = no tail.
    int tail_blocks;
};
// SweepArgs (sweep_core.hpp) holds a Tiling by value and is read from the kernel-argument segment at a fixed offset
static_assert(sizeof(TileRegion) == 32 && sizeof(Tiling) == 8 * 32 + 5 * 4, "Tiling is part of k_sweepO_dpp's arguments");

// What a launch is planned from.  kind[s]: CSIM_BC_* on physical sides, 3 on neighbour sides.  part: 0 = every tile,
// 1 = frame tiles only, 2 = all but the frame tiles, 3 = frame and bulk in one grid.  The last four are SweepCfg's.
struct SweepPlanIn {
    int nx, ny, T, div_mode;
    int kind[4];
    int part;
    int rows_per_chunk, tuned_rows, tail_split, frame_rows;
    int wide;  // 1: part 0 takes wide strips in the middle columns wherever one fits (see sweep_plan.cpp); the caller
               // asks only where the launch may run the wide kernel's unscreened bodies
};
struct SweepPlan {
    int nx, ny, T;   // as given
    int nstrips;
    int rows;        // the chunk height actually used (of the whole field / the bulk; the frame's heights are fixed)
    Tiling tl;
    int nblocks;     // the grid: workgroups of four wavefronts
    unsigned nframe; // part 3: wavefronts that count themselves before the flag is stored
    bool signals;    // part 3: the launch keeps its FrameSync
    bool empty;      // nothing to launch: part 2 of a field that is all frame
    bool wide;       // some region is wide: the launch needs k_sweepO_dpp<..., WIDE>
};
SweepPlan sweep_plan(const SweepPlanIn& in);

// Chunk height of the ensemble's sweep: `count` members of nstrips strips x ny rows each in one launch
int ens_chunk_rows(int T, int count, int nstrips, int ny);

}  // namespace csim
