// sweep_plan.cpp — the tile plan of the overlapped-strip sweep (sweep_plan.hpp): chunk height, frame and bulk, thin
// bands along physical edges, the 7/8 + tail split, the merged launch's frame blocks.  Pure host arithmetic; the kernel
// (k_sweepO_dpp, sweepO.hpp) believes every number of it.
#include "sweep_plan.hpp"

#include <algorithm>

namespace csim {

SweepPlan sweep_plan(const SweepPlanIn& in) {
    const int nx = in.nx, ny = in.ny, T = in.T, part = in.part;
    const bool specialised = specialise_edges(in.div_mode, T);
    const int STRIDE = strip_stride(T);
    SweepPlan plan{};
    plan.nx = nx, plan.ny = ny, plan.T = T;
    const int nstrips = cdiv(nx, STRIDE);
    int ry = in.rows_per_chunk;
    if (ry <= 0) {
        if (in.tuned_rows > 0) {
            ry = in.tuned_rows;
        } else {
            ry = 64;
            while (ry > 16 && static_cast<long>(nstrips) * cdiv(ny, ry) < 8192) ry >>= 1;
            // tiles too small for the on-device trial (< 4 M cells): a launch is at most a round or two of
            // wavefronts and the length of a wavefront's march decides — the shortest chunks win although
            // they double the overhead rows (512^2: +52 %, 1024^2: +37 %, 2048^2: +25 % against 18 rows)
            if (static_cast<long>(nx) * ny < (1L << 22)) ry = 6;
        }
        // the march runs whole groups of six iterations: make ry + 2 (T - 1) a multiple of six so
        // that only a ragged last chunk computes surplus rows
        ry = whole_groups(T, ry);
    }
    if (ry > ny) ry = ny;
    plan.nstrips = nstrips, plan.rows = ry;
    // part 0: the whole field.  part 1 / 2 (multi-rank pass): FRAME / BULK.  The frame is the
    // bottom and top bands (hf rows, all strips) plus the first strip and the last one or two
    // strips (>= MAX_FUSE columns) over the rows in between, in chunks of hf rows: thin tiles,
    // one short round of wavefronts, so the faces are ready ~15 us into the pass.
    const int hf = whole_groups(T, 12);  // >= the deepest face (8-row bands were measured slower: more, even thinner tiles)
    const int nright = (nx - (nstrips - 1) * STRIDE >= MAX_FUSE) ? 1 : 2;
    const bool split = ny >= 2 * hf + 1 && nstrips >= nright + 2;
    // A band along a PHYSICAL bottom / top edge runs the generic edge body (ghost rows), about twice as slow per
    // iteration as the other frame tiles, and the frame launch lasts as long as its slowest tile (47 us instead of 34 on
    // a 4096 x 8192 tile with one physical side): such a band is only as high as the ghost rows require (T-1 rows,
    // rounded so that its march is whole groups of six: 18 iterations at T = 7 instead of 24).  The tiles above it then
    // start at row T and read the ghost row itself as level-0 input — in a bulk-first pass BEFORE this pass's ghost
    // fill has run: fine for Dirichlet and Periodic sides, whose ghost ring never changes, not for Neumann ones, which
    // keep the band of hf >= T rows.
    const int hphys = whole_groups(T, T - 1);
    auto thin = [&](int side) {
        return specialised && in.kind[side] != 3 && in.kind[side] != CSIM_BC_NEUMANN;
    };
    const int hfb = thin(CSIM_BOTTOM) ? std::min(hf, hphys) : hf;
    const int hft = thin(CSIM_TOP) ? std::min(hf, hphys) : hf;
    Tiling& tl = plan.tl;
    auto add_at = [&](int strip0, int nstrip, int j0, int j1, int rows, int x0, int wide) {
        if (nstrip <= 0 || j1 < j0) return;
        TileRegion& r = tl.r[tl.nregions++];
        r.strip0 = strip0, r.nstrip = nstrip, r.j0 = j0, r.j1 = j1, r.ry = rows, r.x0 = x0, r.wide = wide;
        tl.ntiles += nstrip * cdiv(j1 - j0 + 1, rows);
        r.t_end = tl.ntiles;
    };
    // WIDE strips (in.wide, part 0 of a field whose four sides are physical): the rows between the bottom and top bands
    // are cut into one narrow strip on the left (it holds the left ghost column), as many wide strips as fit, and narrow
    // strips with an origin of their own from where the wide ones end to nx (the last holds the right ghost column).
    // A wide strip loads wave_cols(4) columns from TP left of its first output: all of them interior columns, so
    // x0 >= TP (the left narrow strip sees to that) and x0 + STRIDE4 + TP <= nx.  Its rows lie between the bands, so
    // no level of it meets a ghost row and it is never a frame tile of a final pass.
    const int TP = strip_overlap(T), STRIDE4 = strip_stride(T, 4);
    int nwide = 0;  // wide strips per row of tiles: set below, once the bands are known
    auto add = [&](int strip0, int nstrip, int j0, int j1, int rows) { add_at(strip0, nstrip, j0, j1, rows, strip0 * STRIDE, 0); };
    auto add_cols = [&](int strip0, int nstrip, int j0, int j1, int rows) {  // add, or all columns cut left / wide / right
        if (nwide == 0) return add(strip0, nstrip, j0, j1, rows);
        const int xr = STRIDE + nwide * STRIDE4;
        add_at(0, 1, j0, j1, rows, 0, 0);
        add_at(1, nwide, j0, j1, rows, STRIDE, 1);
        add_at(1 + nwide, cdiv(nx - xr, STRIDE), j0, j1, rows, xr, 0);
    };
    // rows j0..j1 of `nstrip` strips: full-height chunks, or — on launches of two or more rounds of wavefronts —
    // a main region of 7/8 of the chunks (a multiple of four, so that its tiles fill whole blocks whatever the
    // number of strips) followed by a tail region at half the height; returns the tail tiles
    auto add_rows = [&](int strip0, int nstrip, int j0, int j1, int rows) -> int {
        const int nrows = j1 - j0 + 1;
        if (nstrip <= 0 || nrows <= 0) return 0;
        const int nchunks = cdiv(nrows, rows);
        // a round of the wide kernel is half as many wavefronts (two per SIMD), and a wide plan has about half as many strips
        const long per_row = nwide ? 1 + nwide + cdiv(nx - STRIDE - nwide * STRIDE4, STRIDE) : nstrip;
        if (!in.tail_split || rows < 48 || nchunks < 16 || per_row * nchunks < (nwide ? 4096 : 8192)) {
            add_cols(strip0, nstrip, j0, j1, rows);
            return 0;
        }
        const bool two_level = in.tail_split != 2;  // default: 7/8 of the chunks full height + the rest at half height;
                                                    // 2 (experiment): 3/4 + half + quarter height — measured no better
        const int main_chunks = (nchunks * (two_level ? 7 : 3) / (two_level ? 8 : 4)) / 4 * 4;
        const int j_main = j0 + main_chunks * rows - 1;
        const int half = whole_groups(T, rows / 2), quarter = whole_groups(T, rows / 4);
        const int rest = j1 - j_main;                       // rows left for the tail regions
        const int j_half = two_level ? j1 : j_main + (rest * 2 / 3) / half * half;  // about two thirds of them at half height
        add_cols(strip0, nstrip, j0, j_main, rows);
        const int before = tl.ntiles;
        add_cols(strip0, nstrip, j_main + 1, j_half, half);
        add_cols(strip0, nstrip, j_half + 1, j1, quarter);
        return tl.ntiles - before;
    };
    int tail_tiles = 0;
    if (part == 0 || ((part == 1 || part == 3) && !split)) {
        // Physical bottom / top edges: the rows whose chunks can produce ghost ROWS of the intermediate levels (the
        // first and last T-1) go into thin bands of their own, so that only those few short tiles run the generic
        // edge body and every other tile of the first / last strips a straight-line column flavour (sweepO_march).
        // The bands come last in the tile order, with the tail region: they are the shortest tiles of the launch.
        const int hb = whole_groups(T, T - 1);
        const bool bands = specialised && ny >= 2 * hb + 6;
        const bool band_b = bands && in.kind[CSIM_BOTTOM] != 3, band_t = bands && in.kind[CSIM_TOP] != 3;
        // (tail_split 2 would need nine regions with wide strips: it keeps the narrow plan)
        const bool lone = in.kind[CSIM_LEFT] != 3 && in.kind[CSIM_RIGHT] != 3;
        if (in.wide && part == 0 && wide_strips_compiled(in.div_mode, T) && band_b && band_t && lone && in.tail_split != 2)
            nwide = std::max(0, (nx - TP - STRIDE) / STRIDE4);
        plan.wide = nwide > 0;
        tail_tiles = add_rows(0, nstrips, band_b ? hb + 1 : 1, band_t ? ny - hb : ny, ry);
        const int before = tl.ntiles;
        if (band_b) add(0, nstrips, 1, hb, hb);
        if (band_t) add(0, nstrips, ny - hb + 1, ny, hb);
        tail_tiles += tl.ntiles - before;
        nwide = 0;
    } else if (part == 1 || part == 3) {
        add(0, nstrips, 1, hfb, hfb);
        add(0, nstrips, ny - hft + 1, ny, hft);
        int hs = hf;  // side strips: taller chunks waste fewer warm-up rows (2 (T - 1) per chunk) but finish later
        if (in.frame_rows >= MAX_FUSE) hs = whole_groups(T, in.frame_rows);
        add(0, 1, hfb + 1, ny - hft, hs);
        add(nstrips - nright, nright, hfb + 1, ny - hft, hs);
    }
    if (part == 3 && split) {  // merged launch: the frame tiles above, then the bulk in the same grid
        tl.frame_tiles = tl.ntiles;
        tl.frame_blocks = cdiv(tl.ntiles, 4);
        plan.nframe = static_cast<unsigned>(tl.frame_tiles);
        plan.signals = true;
        const int before = tl.ntiles;
        tail_tiles = add_rows(1, nstrips - 1 - nright, hfb + 1, ny - hft, std::min(ry, ny - hfb - hft));
        plan.nblocks = tl.frame_blocks + cdiv(tl.ntiles - before, 4);
    } else if (part == 3) {  // a tile that is all frame: every tile counts for the flag
        tl.frame_tiles = tl.ntiles;
        tl.frame_blocks = cdiv(tl.ntiles, 4);
        tl.tail_blocks = 0;
        tail_tiles = 0;
        plan.nframe = static_cast<unsigned>(tl.frame_tiles);
        plan.signals = true;
        plan.nblocks = tl.frame_blocks;
    } else {
        if (part == 2 && split) tail_tiles = add_rows(1, nstrips - 1 - nright, hfb + 1, ny - hft, std::min(ry, ny - hfb - hft));
        if (tl.ntiles == 0) {  // part 2 of a field that is all frame
            plan.empty = true;
            return plan;
        }
        plan.nblocks = cdiv(tl.ntiles, 4);
    }
    tl.tail_blocks = cdiv(tail_tiles, 4);
    return plan;
}

int ens_chunk_rows(int T, int count, int nstrips, int ny) {
    // Chunk height: as tall as keeps two rounds of wavefronts (8192 tiles) on the chip — every chunk marches
    // 2 (T - 1) rows more than it stores — down to 6 rows, the single stepper's choice for small lone tiles.
    int ry = 64;
    while (ry > 6 && static_cast<long>(count) * nstrips * cdiv(ny, ry) < 8192) ry >>= 1;
    if (ry < 6) ry = 6;
    ry = whole_groups(T, ry);  // whole groups of six march iterations
    if (ry > ny) ry = ny;
    return ry;
}

}  // namespace csim
