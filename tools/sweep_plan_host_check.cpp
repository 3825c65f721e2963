// tools/sweep_plan_host_check.cpp — the tile plan of the overlapped-strip sweep (csrc/sweep_plan.cpp, sweep_plan.hpp)
// checked on the CPU, stand-alone: no device, no HIP, nothing loaded into another process (tools/obsop_sanitize.sh runs
// it under AddressSanitizer + UndefinedBehaviorSanitizer; tests/test_sweep_plan_host.py without).  k_sweepO_dpp
// (csrc/sweepO.hpp) believes a plan blindly: it fills no bound check into Tiling::r[8], maps blocks to tiles by
// frame_blocks / tail_blocks, and a merged launch releases the comm stream when nframe wavefronts have counted
// themselves — a miscounted frame parks that stream for good.  This program restates the kernel's decode (block ->
// tile -> region -> strip, jb, je; xcd_remap copied in, both swz values) and checks, for every plan of the enumeration
// below:
//   A  regions well formed    nregions <= 8; t_end strictly increasing, the last == ntiles; per region nstrip >= 1,
//                             0 <= strip0, strip0 + nstrip <= nstrips, 1 <= j0 <= j1 <= ny, ry >= 1
//   B  block map a bijection  over nblocks x 4 wavefronts the decode reaches every tile of [0, ntiles) exactly once
//                             (padding wavefronts none), every decoded tile has jb <= je
//   C  coverage               every (strip, interior row) is an output of exactly one tile of part 0; of part 3; of
//                             parts 1 and 2 together; part 2 is "nothing to launch" exactly when part 1 covers all
//   D  frame identity         tiles [0, frame_tiles) of part 3 are part 1's tiles in part 1's order;
//                             nframe == frame_tiles == ntiles(part 1); parts 0, 1, 2 do not signal
//   E  frame reach            on every side of kind 3 the part-1 tiles hold the min(MAX_FUSE, nx or ny) interior lines
//                             next to it over its full length (the next pass's faces are packed from them)
//   F  wide tiles interior    (plans with wide strips, SweepPlanIn::wide) every tile of a wide region loads 256 interior
//                             columns from an even column on, no level of it meets a ghost row, and it is no frame tile
//                             of a final pass (not the first or last strip, not the first or last row); wide regions
//                             exist only in part 0 of a field without neighbours, at the depths the wide kernel has
// and folds every plan into one 64-bit hash, in enumeration order, which must be the recorded one: a plan that
// changes is then a decision, not an accident.  The plans asked for wide strips are a second enumeration with a hash
// of its own (which also folds each region's origin and kind); there C counts every interior CELL, since strips of
// two widths share a row, and a request that no wide strip fits must give the narrow plan unchanged.
// Prints "sweep plan host ok" and returns 0, or says what failed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "sweep_plan.hpp"

namespace {

using csim::SweepPlan;
using csim::SweepPlanIn;
using csim::Tiling;

constexpr std::uint64_t EXPECT_HASH = 0xeec39933f7ad892cull;  // of the run that agreed with the planner as it was inside sweepO_div
constexpr long EXPECT_PLANS = 485400;
constexpr std::uint64_t EXPECT_HASH_WIDE = 0xc292f82455edc798ull;  // of the enumeration that asks for wide strips
constexpr long EXPECT_PLANS_WIDE = 207376;

int g_fail = 0;
SweepPlanIn g_in;  // the plan under check, for the report
#define EXPECT(cond)                                                                                              \
    do {                                                                                                          \
        if (!(cond)) {                                                                                            \
            if (g_fail++ < 20)                                                                                    \
                std::printf("FAILED line %d: %s  [nx %d ny %d T %d div %d kind %d%d%d%d part %d rows %d tuned %d "  \
                            "tail %d frame_rows %d]\n", __LINE__, #cond, g_in.nx, g_in.ny, g_in.T, g_in.div_mode,  \
                            g_in.kind[0], g_in.kind[1], g_in.kind[2], g_in.kind[3], g_in.part, g_in.rows_per_chunk, \
                            g_in.tuned_rows, g_in.tail_split, g_in.frame_rows);                                   \
            return false;                                                                                         \
        }                                                                                                         \
    } while (0)

// ---- the kernel's decode, restated (k_sweepO_dpp, csrc/sweepO.hpp; xcd_remap: csrc/sweep_core.hpp) -------------------
int xcd_remap(int b, int nb, int enable) {
    if (!enable || nb < 16) return b;
    const int per = nb >> 3, rem = nb & 7;
    const int xcd = b & 7, q = b >> 3;
    return xcd < rem ? xcd * (per + 1) + q : rem * (per + 1) + (xcd - rem) * per + q;
}
// the tile of wavefront `wave` of block b in a grid of nblocks, -1 where the wavefront returns
int block_tile(const Tiling& tl, int nblocks, int swz, int b, int wave) {
    int tile;
    if (b < tl.frame_blocks) {
        tile = 4 * b + wave;
        if (tile >= tl.frame_tiles) return -1;  // padding of the last frame block
    } else {
        const int lb = b - tl.frame_blocks, nb_mid = nblocks - tl.frame_blocks - tl.tail_blocks;
        tile = tl.frame_tiles + (lb < nb_mid ? xcd_remap(lb, nb_mid, swz) : lb) * 4 + wave;
    }
    return tile >= tl.ntiles ? -1 : tile;
}
// strip: the region's strip0 + the strip's place in its region (what conditions C - E of the narrow plans count by);
// g0, wide: what the kernel marches from — the first loaded column (0-based interior index, -TP for the first strip)
// and the strip's kind
struct Tile {
    int strip, jb, je, g0, wide;
    bool operator==(const Tile& o) const { return strip == o.strip && jb == o.jb && je == o.je && g0 == o.g0 && wide == o.wide; }
};
Tile locate(const Tiling& tl, int tile, int T) {
    int t0 = 0, q_used = 0;
    for (int q = 1; q < 8; ++q)
        if (q < tl.nregions && tile >= tl.r[q - 1].t_end) t0 = tl.r[q - 1].t_end, q_used = q;
    const csim::TileRegion& r = tl.r[q_used];
    const int local = tile - t0;
    const int jb = r.j0 + local / r.nstrip * r.ry;
    const int g0 = r.x0 + local % r.nstrip * csim::strip_stride(T, r.wide ? 4 : 2) - csim::strip_overlap(T);
    return Tile{r.strip0 + local % r.nstrip, jb, jb + r.ry - 1 < r.j1 ? jb + r.ry - 1 : r.j1, g0, r.wide};
}

// ---- the conditions ------------------------------------------------------------------------------------------------
std::uint64_t g_hash = 0xcbf29ce484222325ull, g_hash_wide = 0xcbf29ce484222325ull;
long g_plans = 0, g_plans_wide = 0, g_wide_tiles = 0;
bool g_wide_run = false;  // the second enumeration: its own hash and count
void fold(std::uint64_t v) {
    std::uint64_t& h = g_wide_run ? g_hash_wide : g_hash;
    h = (h ^ v) * 0x100000001b3ull;
}
void fold_plan(const SweepPlan& p) {
    for (const csim::TileRegion& r : p.tl.r) {
        for (int v : {r.t_end, r.strip0, r.nstrip, r.j0, r.j1, r.ry}) fold(static_cast<std::uint32_t>(v));
        if (g_wide_run)
            for (int v : {r.x0, r.wide}) fold(static_cast<std::uint32_t>(v));
    }
    if (g_wide_run) {
        fold(static_cast<std::uint32_t>(p.wide));
        ++g_plans_wide;
        --g_plans;
    }
    for (int v : {p.tl.nregions, p.tl.ntiles, p.tl.frame_tiles, p.tl.frame_blocks, p.tl.tail_blocks, p.nstrips, p.rows,
                  p.nblocks, static_cast<int>(p.nframe), static_cast<int>(p.signals), static_cast<int>(p.empty)})
        fold(static_cast<std::uint32_t>(v));
    ++g_plans;
}

std::vector<int> g_seen;
// A and B of one plan
bool check_plan(const SweepPlanIn& in, const SweepPlan& p) {
    g_in = in;
    const Tiling& tl = p.tl;
    EXPECT(p.nx == in.nx && p.ny == in.ny && p.T == in.T);
    EXPECT(p.nstrips == csim::cdiv(in.nx, csim::strip_stride(in.T)));
    EXPECT(p.rows >= 1 && p.rows <= in.ny);
    EXPECT(tl.nregions >= 0 && tl.nregions <= 8);
    if (p.empty) {
        EXPECT(tl.ntiles == 0 && tl.nregions == 0 && p.nblocks == 0);
        return true;
    }
    EXPECT(tl.nregions >= 1 && p.nblocks >= 1);
    for (int q = 0; q < tl.nregions; ++q) {
        const csim::TileRegion& r = tl.r[q];
        EXPECT(r.t_end > (q ? tl.r[q - 1].t_end : 0));
        EXPECT(r.nstrip >= 1 && r.strip0 >= 0 && r.strip0 + r.nstrip <= p.nstrips);
        EXPECT(1 <= r.j0 && r.j0 <= r.j1 && r.j1 <= in.ny && r.ry >= 1);
        EXPECT((r.wide == 0 || r.wide == 1) && r.x0 >= 0 && r.x0 % 2 == 0 && (p.wide || r.wide == 0));
        if (!p.wide) EXPECT(r.x0 == r.strip0 * csim::strip_stride(in.T));  // a narrow plan: every strip of the field's own grid
    }
    {
        bool any = false;
        for (int q = 0; q < tl.nregions; ++q) any = any || tl.r[q].wide;
        EXPECT(any == p.wide);
        // where a wide region may exist at all
        if (p.wide) {
            EXPECT(in.wide && in.part == 0 && csim::wide_strips_compiled(in.div_mode, in.T));
            for (int k = 0; k < 4; ++k) EXPECT(in.kind[k] != 3);
        }
    }
    const int TP = csim::strip_overlap(in.T);
    EXPECT(tl.r[tl.nregions - 1].t_end == tl.ntiles);
    EXPECT(tl.frame_tiles >= 0 && tl.frame_tiles <= tl.ntiles && tl.frame_blocks >= 0 && tl.tail_blocks >= 0);
    EXPECT(tl.frame_blocks + tl.tail_blocks <= p.nblocks);
    for (int swz = 0; swz <= 1; ++swz) {
        g_seen.assign(tl.ntiles, 0);
        for (int b = 0; b < p.nblocks; ++b)
            for (int wave = 0; wave < 4; ++wave) {
                const int tile = block_tile(tl, p.nblocks, swz, b, wave);
                if (tile < 0) continue;
                EXPECT(tile < tl.ntiles);
                EXPECT(g_seen[tile]++ == 0);
                EXPECT((b < tl.frame_blocks) == (tile < tl.frame_tiles));  // the kernel's frame_tile
                const Tile t = locate(tl, tile, in.T);
                EXPECT(t.jb <= t.je && t.jb >= 1 && t.je <= in.ny && t.strip >= 0 && t.strip < p.nstrips);
                EXPECT(t.g0 >= -TP && t.g0 % 2 == 0 && t.g0 + TP < in.nx);  // aligned pairs; at least one output column
                if (t.wide) {  // F
                    EXPECT(t.g0 >= 0 && t.g0 + csim::wave_cols(4) <= in.nx);
                    EXPECT(t.jb - (in.T - 1) >= 1 && t.je + (in.T - 1) <= in.ny);
                    EXPECT(tile >= tl.frame_tiles && tl.frame_tiles == 0);
                    EXPECT(t.g0 != -TP && t.g0 + TP + csim::strip_stride(in.T, 4) < in.nx && t.jb != 1 && t.je != in.ny);
                    g_wide_tiles += swz;
                }
            }
        for (int t = 0; t < tl.ntiles; ++t) EXPECT(g_seen[t] == 1);
    }
    return true;
}

// += 1 on every (strip, row) a tile of the plan writes
void cover(const SweepPlan& p, std::vector<int>* c) {
    for (int t = 0; t < p.tl.ntiles; ++t) {
        const Tile x = locate(p.tl, t, p.T);
        for (int j = x.jb; j <= x.je; ++j) (*c)[static_cast<size_t>(x.strip) * (p.ny + 1) + j] += 1;
    }
}
// the same by CELL, from what the kernel stores: columns [g0 + TP, g0 + TP + STRIDE) of the strip's kind, clipped to nx
bool cells_once(const SweepPlan& p) {
    std::vector<unsigned char> c(static_cast<size_t>(p.nx) * p.ny, 0);
    for (int t = 0; t < p.tl.ntiles; ++t) {
        const Tile x = locate(p.tl, t, p.T);
        const int c0 = x.g0 + csim::strip_overlap(p.T), c1 = c0 + csim::strip_stride(p.T, x.wide ? 4 : 2);
        for (int j = x.jb; j <= x.je; ++j)
            for (int i = c0; i < c1 && i < p.nx; ++i)
                if (++c[static_cast<size_t>(j - 1) * p.nx + i] > 1) return false;
    }
    for (unsigned char v : c)
        if (v != 1) return false;
    return true;
}
bool all_are(const std::vector<int>& c, int nstrips, int ny, int v) {
    for (int s = 0; s < nstrips; ++s)
        for (int j = 1; j <= ny; ++j)
            if (c[static_cast<size_t>(s) * (ny + 1) + j] != v) return false;
    return true;
}

// a region of half-height chunks on top of a region of full-height ones, owned by the last blocks
long g_tails = 0;
bool has_tail(const SweepPlan& p) {
    for (int q = 1; q < p.tl.nregions; ++q) {
        const csim::TileRegion &a = p.tl.r[q - 1], &b = p.tl.r[q];
        if (p.tl.tail_blocks > 0 && a.strip0 == b.strip0 && a.nstrip == b.nstrip && b.j0 == a.j1 + 1 && a.ry == p.rows &&
            b.ry == csim::whole_groups(p.T, p.rows / 2))
            return true;
    }
    return false;
}
// one input in its four parts: A, B of each, then C, D, E
bool check_set(SweepPlanIn in) {
    SweepPlan p[4];
    for (int part = 0; part < 4; ++part) {
        in.part = part;
        p[part] = csim::sweep_plan(in);
        fold_plan(p[part]);
        if (!check_plan(in, p[part])) return false;
        g_tails += has_tail(p[part]);
    }
    in.part = -1;
    g_in = in;
    const int ns = p[0].nstrips, ny = in.ny;
    for (int part = 1; part < 4; ++part) EXPECT(p[part].nstrips == ns);
    EXPECT(p[0].rows == p[2].rows && p[0].rows == p[3].rows);
    const size_t cells = static_cast<size_t>(ns) * (ny + 1);
    // C
    std::vector<int> c(cells, 0);
    if (p[0].wide) {
        EXPECT(cells_once(p[0]));
    } else {
        cover(p[0], &c);
        EXPECT(all_are(c, ns, ny, 1));
    }
    if (in.wide) {  // asked for wide strips: only part 0 may differ from the narrow plans, and only where one fits
        SweepPlanIn nin = in;
        nin.wide = 0;
        for (int part = 0; part < 4; ++part) {
            nin.part = part;
            const SweepPlan n = csim::sweep_plan(nin);
            const bool same = std::memcmp(&n.tl, &p[part].tl, sizeof(Tiling)) == 0 && n.nblocks == p[part].nblocks &&
                              n.rows == p[part].rows && n.nstrips == p[part].nstrips;
            EXPECT(same == !p[part].wide);
        }
        const int fits = (in.nx - csim::strip_overlap(in.T) - csim::strip_stride(in.T)) / csim::strip_stride(in.T, 4);
        bool lone = true;
        for (int k = 0; k < 4; ++k) lone = lone && in.kind[k] != 3;
        const int hb = csim::whole_groups(in.T, in.T - 1);
        EXPECT(p[0].wide == (fits >= 1 && lone && csim::wide_strips_compiled(in.div_mode, in.T) && ny >= 2 * hb + 6 &&
                             in.tail_split != 2));
    }
    c.assign(cells, 0);
    cover(p[3], &c);
    EXPECT(all_are(c, ns, ny, 1));
    std::vector<int> frame(cells, 0);
    cover(p[1], &frame);
    EXPECT(p[2].empty == all_are(frame, ns, ny, 1));
    c = frame;
    if (!p[2].empty) cover(p[2], &c);
    EXPECT(all_are(c, ns, ny, 1));
    // D
    EXPECT(!p[0].signals && !p[1].signals && !p[2].signals && p[3].signals);
    EXPECT(p[0].nframe == 0 && p[1].nframe == 0 && p[2].nframe == 0);
    EXPECT(!p[0].empty && !p[1].empty && !p[3].empty);
    EXPECT(p[3].tl.frame_tiles == p[1].tl.ntiles && p[3].nframe == static_cast<unsigned>(p[1].tl.ntiles));
    EXPECT(p[3].tl.frame_blocks == csim::cdiv(p[3].tl.frame_tiles, 4));
    for (int part = 0; part < 3; ++part) EXPECT(p[part].tl.frame_tiles == 0 && p[part].tl.frame_blocks == 0);
    for (int t = 0; t < p[1].tl.ntiles; ++t) EXPECT(locate(p[3].tl, t, in.T) == locate(p[1].tl, t, in.T));
    // E
    const int S = csim::strip_stride(in.T);
    const int hx = in.nx < csim::MAX_FUSE ? in.nx : csim::MAX_FUSE, hy = ny < csim::MAX_FUSE ? ny : csim::MAX_FUSE;
    auto in_frame = [&](int s, int j) { return frame[static_cast<size_t>(s) * (ny + 1) + j] == 1; };
    if (in.kind[CSIM_LEFT] == 3)
        for (int s = 0; s <= (hx - 1) / S; ++s)
            for (int j = 1; j <= ny; ++j) EXPECT(in_frame(s, j));
    if (in.kind[CSIM_RIGHT] == 3)
        for (int s = (in.nx - hx) / S; s < ns; ++s)
            for (int j = 1; j <= ny; ++j) EXPECT(in_frame(s, j));
    for (int s = 0; s < ns; ++s) {
        if (in.kind[CSIM_BOTTOM] == 3)
            for (int j = 1; j <= hy; ++j) EXPECT(in_frame(s, j));
        if (in.kind[CSIM_TOP] == 3)
            for (int j = ny - hy + 1; j <= ny; ++j) EXPECT(in_frame(s, j));
    }
    return true;
}

}  // namespace

int main() {
    const int D = CSIM_BC_DIRICHLET, N = CSIM_BC_NEUMANN, P = CSIM_BC_PERIODIC;
    const int kinds[][4] = {{3, 3, 3, 3}, {D, D, D, D}, {N, N, N, N}, {P, P, P, P}, {3, D, N, P}, {D, 3, D, D},
                            {N, N, 3, N}, {P, D, P, 3}, {3, 3, P, P}, {D, N, 3, 3}, {3, 3, 3, D}, {N, 3, 3, 3}};
    const int nys[] = {1, 2, 6, 7, 11, 12, 17, 18, 24, 25, 29, 30, 37, 61, 100};
    for (int T = 2; T <= csim::MAX_FUSE; ++T) {
        const int S = csim::strip_stride(T);
        if (S != csim::WAVE_COLS - 4 * ((T + 1) / 2) || csim::strip_overlap(T) < T || csim::strip_overlap(T) % 2) {
            std::printf("FAILED: strip geometry at T = %d\n", T);
            return 1;
        }
        const int nxs[] = {1, 5, 7, 8, 100, S, S + 1, S + 6, S + 7, 2 * S + 3, 3 * S, 3 * S + 6, 4 * S + 7, 700};
        for (int div : {0, 2})
            for (const auto& kind : kinds)
                for (int nx : nxs)
                    for (int ny : nys)
                        for (int rows : {0, 5})
                            for (int frame_rows : {0, 30}) {
                                const SweepPlanIn in{nx, ny, T, div, {kind[0], kind[1], kind[2], kind[3]}, 0,
                                                     rows, 0, 1, frame_rows};
                                if (!check_set(in)) return 1;
                            }
    }
    // the tail split: shapes that cross the 8192-tile threshold, and must produce a tail region
    for (int T : {4, 7}) {
        const int S = csim::strip_stride(T);
        const int shapes[][3] = {{64 * S, 48 * 130 + 5, 48}, {66 * S + 3, 48 * 128, 48}, {40 * S, 60 * 210 + 1, 60},
                                 {70 * S, 48 * 130 + 5, 48}, {44 * S + 1, 60 * 210 + 1, 60}};  // the last two: the bulk too
        for (const auto& sh : shapes)
            for (int ts : {0, 1, 2})
                for (const auto& kind : {kinds[0], kinds[1], kinds[4], kinds[9]}) {
                    const SweepPlanIn in{sh[0], sh[1], T, 0, {kind[0], kind[1], kind[2], kind[3]}, 0, sh[2], 0, ts, 0};
                    const long before = g_tails;
                    if (!check_set(in)) return 1;
                    // the whole-field launch ends in a tail (the last two shapes: the bulk of parts 2 and 3 as well);
                    // tail_split 0 has none
                    const long want = ts == 0 ? 0 : (&sh - shapes >= 3 ? 3 : 1);
                    if (ts == 0 ? g_tails != before : g_tails - before < want) {
                        std::printf("FAILED: tail regions %ld at nx %d ny %d T %d rows %d tail_split %d\n",
                                    g_tails - before, sh[0], sh[1], T, sh[2], ts);
                        return 1;
                    }
                }
    }
    // the heuristic and tuned heights, at sizes on both sides of 1 << 22 cells
    for (int T = 2; T <= csim::MAX_FUSE; ++T)
        for (int tuned : {0, 42, 118})
            for (const auto& sh : {std::pair<int, int>{2048, 2047}, {2048, 2048}, {4096, 8192}, {16384, 16384}, {777, 9001}})
                for (const auto& kind : {kinds[0], kinds[1], kinds[5]}) {
                    const SweepPlanIn in{sh.first, sh.second, T, 1, {kind[0], kind[1], kind[2], kind[3]}, 0, 0, tuned, 1, 0};
                    if (!check_set(in)) return 1;
                }
    // the ensemble's chunk height
    for (int T = 2; T <= csim::MAX_FUSE; ++T)
        for (int count : {1, 3, 64, 1000})
            for (int nstrips : {1, 2, 5, 40})
                for (int ny : {1, 2, 5, 6, 7, 11, 12, 13, 64, 100, 256, 1000, 4096}) {
                    const int ry = csim::ens_chunk_rows(T, count, nstrips, ny);
                    if (ry < 1 || ry > ny || (ry < ny && ((ry + 2 * (T - 1)) % 6 != 0 || ry < 6))) {
                        std::printf("FAILED: ens_chunk_rows(%d, %d, %d, %d) = %d\n", T, count, nstrips, ny, ry);
                        return 1;
                    }
                    fold(static_cast<std::uint32_t>(ry));
                }
    // ---- the second enumeration: the same conditions over plans that ask for wide strips -------------------------
    g_wide_run = true;
    const int dnpd[4] = {D, N, P, D};
    for (int T = 4; T <= csim::MAX_FUSE; ++T) {
        const int S = csim::strip_stride(T), S4 = csim::strip_stride(T, 4), TP = csim::strip_overlap(T);
        if (S4 != csim::wave_cols(4) - 2 * TP || csim::wave_cols(4) != 256) {
            std::printf("FAILED: wide strip geometry at T = %d\n", T);
            return 1;
        }
        // no wide strip fits / exactly one / one and a remainder / odd nx / several and a short remainder / none left over
        const int nxs[] = {S, S + TP + S4 - 1, S + TP + S4, 608, 849, 1100, S + 3 * S4 + TP, S + 2 * S4 + TP + 1, 2 * S + 3 * S4 + 5};
        for (int div : {0, 1, 2})
            for (const int* kind : {kinds[1], kinds[2], kinds[3], dnpd, kinds[4], kinds[5]})
                for (int nx : nxs)
                    for (int ny : {12, 17, 18, 21, 22, 30, 37, 40, 64, 100})
                        for (int rows : {0, 5, 6, 13})
                            for (int ts : {1, 2}) {
                                const SweepPlanIn in{nx, ny, T, div, {kind[0], kind[1], kind[2], kind[3]}, 0, rows, 0, ts, 0, 1};
                                if (!check_set(in)) return 1;
                            }
    }
    // wide plans with a tail region (half as many tiles make a round), and the bench grid with a tuned height
    for (int T : {6, 7})
        for (const auto& sh : {std::pair<int, int>{8192, 48 * 130 + 5}, {4096, 48 * 260 + 1}}) {
            const SweepPlanIn in{sh.first, sh.second, T, 0, {D, D, D, D}, 0, 48, 0, 1, 0, 1};
            const long before = g_tails;
            if (!check_set(in)) return 1;
            if (g_tails == before) {
                std::printf("FAILED: no tail region in the wide plan of %d x %d at T = %d\n", sh.first, sh.second, T);
                return 1;
            }
        }
    if (g_wide_tiles == 0) {
        std::printf("FAILED: the second enumeration saw no wide tile\n");
        return 1;
    }
    g_wide_run = false;
    std::printf("%ld plans asked for wide strips, hash 0x%016llx\n", g_plans_wide, static_cast<unsigned long long>(g_hash_wide));
    if (g_plans_wide != EXPECT_PLANS_WIDE || g_hash_wide != EXPECT_HASH_WIDE) {
        std::printf("FAILED: expected %ld plans, hash 0x%016llx: a plan with wide strips changed\n", EXPECT_PLANS_WIDE,
                    static_cast<unsigned long long>(EXPECT_HASH_WIDE));
        return 1;
    }
    std::printf("%ld plans, hash 0x%016llx\n", g_plans, static_cast<unsigned long long>(g_hash));
    if (g_plans != EXPECT_PLANS || g_hash != EXPECT_HASH) {
        std::printf("FAILED: expected %ld plans, hash 0x%016llx: a plan changed\n", EXPECT_PLANS,
                    static_cast<unsigned long long>(EXPECT_HASH));
        return 1;
    }
    std::printf("sweep plan host ok\n");
    return 0;
}
