// tools/gram_plan_host_check.cpp — the plan and the geometry of the Gram sums (csrc/gram_plan.hpp) checked on the
// CPU, stand-alone: no device, no HIP, nothing loaded into another process (tools/obsop_sanitize.sh runs it under
// AddressSanitizer + UndefinedBehaviorSanitizer; tests/test_gram_plan_host.py without).  GramTile (csrc/gram_tile.hpp)
// believes this geometry blindly: a block nobody owns is a hole in G, a block owned twice is a race on the class's
// partial, and a read past the row is another row's data.  For every cols = 1 .. 257 and NB = 1, 2, 4:
//   A  the block triangle   gram_nblk, gram_nblocks and gram_block_of against the enumeration row by row
//   B  ownership            over all shares, slots u and lanes every block has exactly one owner (mine), which holds
//                           that block; a lane past the end holds the last block and does not own it; gram_shares is
//                           the least number of workgroups that reaches every block
//   C  idle waves           gram_wave_on is false exactly for the waves none of whose lanes owns a block
//   D  the packed triangle  gram_packed is a bijection of the pairs a <= b < cols onto 0 .. gram_pairs - 1, and the
//                           pairs a <= b < cols of the owned blocks are each pair once
//   E  the LDS row          gram_stride is even and holds the padded width, and 4 ib + 3 < stride: the two 16-byte
//                           reads of a block side stay inside the row and are aligned
// for the rectangle of the ensemble-space dot (DotTile of csrc/ensemble_dot.hip believes it as blindly), every
// M = 1 .. 256 and K = 1 .. 16:
//   F  ownership            every 4 x 4 block of the M x K rectangle has exactly one owning lane among the 256
//                           (dot_owned), which holds that block; a lane past the end holds the last block and owns
//                           nothing; every entry k < M, r < K is stored once
//   G  idle waves           dot_wave_on is false exactly for the waves none of whose lanes owns a block
//   H  the LDS rows         dot_fstride is even and holds the padded width, the two 16-byte reads of either side (4 im
//                           in a row of gram_stride(M), 4 ik in a row of dot_fstride(K)) stay inside their row and are
//                           aligned, the field rows start on a 16-byte boundary, and dot_lds_doubles is the rows, the
//                           means and the field rows; at (256, 16) the bytes the launcher raises the dynamic limit to
// and, for the plan: segments and classes against brute force at the cap seams of both callers (M and M + 1 columns),
// every segment in exactly one class and no class empty, the automatic form and the blocks per lane of a form.
// Prints "gram plan host ok" and returns 0, or says what failed.
#include <cstdio>
#include <utility>
#include <vector>

#include "gram_plan.hpp"

namespace {

using namespace csim;

int g_cols = 0, g_nb = 0;
#define EXPECT(cond)                                                                                   \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            std::printf("FAILED line %d: %s  [cols %d NB %d]\n", __LINE__, #cond, g_cols, g_nb);        \
            return false;                                                                              \
        }                                                                                              \
    } while (0)

bool check_geometry(int cols, int NB) {
    g_cols = cols, g_nb = NB;
    // A
    int nblk = 0;
    while (GRAM_TB * nblk < cols) ++nblk;
    std::vector<std::pair<int, int>> blocks;
    for (int ia = 0; ia < nblk; ++ia)
        for (int ib = ia; ib < nblk; ++ib) blocks.push_back({ia, ib});
    const int nblocks = static_cast<int>(blocks.size());
    EXPECT(gram_nblk(cols) == nblk && gram_nblocks(cols) == nblocks && nblocks >= 1);
    for (int i = 0; i < nblocks; ++i) {
        const GramBlock at = gram_block_of(i, nblk);
        EXPECT(at.ia == blocks[i].first && at.ib == blocks[i].second);
    }
    // E
    const int stride = gram_stride(cols);
    EXPECT(stride % 2 == 0 && stride >= GRAM_TB * nblk && GRAM_TB * nblk >= cols);
    for (const auto& b : blocks) EXPECT(GRAM_TB * b.second + GRAM_TB - 1 < stride && b.first <= b.second);
    // B, C
    const int per = NB * GRAM_THREADS, shares = gram_shares(cols, NB);
    EXPECT(shares >= 1 && shares * per >= nblocks && (shares - 1) * per < nblocks);
    std::vector<int> owners(blocks.size(), 0);
    std::vector<int> stored(gram_pairs(cols), 0);
    for (int share = 0; share < shares; ++share)
        for (int wave = 0; wave < GRAM_THREADS / 64; ++wave) {
            bool any = false;
            for (int lane = 64 * wave; lane < 64 * wave + 64; ++lane)
                for (int u = 0; u < NB; ++u) {
                    const GramOwned o = gram_owned(share, NB, u, lane, cols);
                    const int bidx = (share * NB + u) * GRAM_THREADS + lane;
                    EXPECT(o.mine == (bidx < nblocks));
                    const std::pair<int, int>& want = blocks[o.mine ? bidx : nblocks - 1];
                    EXPECT(o.at.ia == want.first && o.at.ib == want.second);
                    if (!o.mine) continue;
                    any = true;
                    ++owners[bidx];
                    // what GramTile::store writes of this block
                    for (int i = 0; i < GRAM_TB; ++i)
                        for (int j = 0; j < GRAM_TB; ++j) {
                            const int a = GRAM_TB * o.at.ia + i, b = GRAM_TB * o.at.ib + j;
                            if (a <= b && b < cols) {
                                const size_t at = gram_packed(a, b, cols);
                                EXPECT(at < stored.size());
                                ++stored[at];
                            }
                        }
                }
            for (int lane = 64 * wave; lane < 64 * wave + 64; ++lane) EXPECT(gram_wave_on(share, NB, lane, cols) == any);
        }
    for (int n : owners) EXPECT(n == 1);
    for (int n : stored) EXPECT(n == 1);
    // D
    EXPECT(gram_pairs(cols) == static_cast<size_t>(cols) * (cols + 1) / 2);
    size_t next = 0;  // row by row, without a gap
    for (int a = 0; a < cols; ++a)
        for (int b = a; b < cols; ++b) EXPECT(gram_packed(a, b, cols) == next++);
    EXPECT(next == gram_pairs(cols));
    return true;
}

bool check_dot(int M, int K) {
    g_cols = M, g_nb = K;  // printed as "cols M NB K"
    const int nbm = gram_nblk(M), nbk = gram_nblk(K), nblocks = nbm * nbk;
    EXPECT(nblocks >= 1 && nblocks <= GRAM_THREADS);
    // F, G
    std::vector<int> owners(static_cast<size_t>(nblocks), 0), stored(static_cast<size_t>(M) * K, 0);
    for (int wave = 0; wave < GRAM_THREADS / 64; ++wave) {
        bool any = false;
        for (int lane = 64 * wave; lane < 64 * wave + 64; ++lane) {
            const DotOwned o = dot_owned(lane, M, K);
            EXPECT(o.mine == (lane < nblocks));
            const int b = o.mine ? lane : nblocks - 1;
            EXPECT(o.im == b / nbk && o.ik == b % nbk && o.im < nbm && o.ik < nbk);
            if (!o.mine) continue;
            any = true;
            ++owners[static_cast<size_t>(o.im) * nbk + o.ik];
            // what DotTile::store writes of this block
            for (int i = 0; i < GRAM_TB; ++i)
                for (int j = 0; j < GRAM_TB; ++j) {
                    const int k = GRAM_TB * o.im + i, r = GRAM_TB * o.ik + j;
                    if (k < M && r < K) ++stored[static_cast<size_t>(k) * K + r];
                }
        }
        for (int lane = 64 * wave; lane < 64 * wave + 64; ++lane) EXPECT(dot_wave_on(lane, M, K) == any);
    }
    for (int n : owners) EXPECT(n == 1);
    for (int n : stored) EXPECT(n == 1);
    // H: offsets in doubles from the 16-byte aligned start of LDS, so an even offset is an aligned read
    const int stride = gram_stride(M), fstride = dot_fstride(K);
    EXPECT(fstride % 2 == 0 && fstride >= GRAM_TB * nbk && GRAM_TB * nbk >= K);
    EXPECT(stride % 2 == 0 && gram_lds_doubles(M) % 2 == 0);
    for (int lane = 0; lane < GRAM_THREADS; ++lane) {
        const DotOwned o = dot_owned(lane, M, K);
        EXPECT(GRAM_TB * o.im + GRAM_TB - 1 < stride && GRAM_TB * o.ik + GRAM_TB - 1 < fstride);
    }
    EXPECT(gram_lds_doubles(M) == static_cast<size_t>(GRAM_SEG) * stride + GRAM_SEG);
    EXPECT(dot_lds_doubles(M, K) == static_cast<size_t>(GRAM_SEG) * (stride + fstride) + GRAM_SEG);
    return true;
}

bool check_plan() {
    g_cols = g_nb = 0;
    EXPECT(GRAM_SEG == 64 && GRAM_THREADS == 256 && GRAM_TB == 4 && GRAM_FORMS == 3 && ESPACE_MAX_MEMBERS == 256);
    // the dynamic LDS limits that launch_gram and ens_launch_dot raise their kernels to, in bytes, within 160 KiB
    EXPECT(DOT_MAX_FIELDS == 16 && sizeof(double) * gram_lds_doubles(ESPACE_MAX_MEMBERS) == 8 * (64 * 258 + 64));
    EXPECT(sizeof(double) * dot_lds_doubles(ESPACE_MAX_MEMBERS, DOT_MAX_FIELDS) == 8 * (64 * (258 + 18) + 64));
    EXPECT(sizeof(double) * dot_lds_doubles(ESPACE_MAX_MEMBERS, DOT_MAX_FIELDS) <= 160 * 1024);
    EXPECT(gram_cap(0) == 0 && gram_cap(-3) == 0 && gram_cap(ESPACE_MAX_MEMBERS + 1) == 0);
    const long seams[] = {1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 16383, 16384, 16385, 65535, 65536, 65537,
                          1L << 20, (1L << 22) + 1};
    for (int M = 1; M <= ESPACE_MAX_MEMBERS; ++M) {
        g_cols = M;
        const int cap = M <= 64 ? 1024 : M <= 128 ? 256 : 64;
        EXPECT(gram_cap(M) == cap);
        EXPECT(gram_auto_form(M) == (M <= 64 ? 1 : M <= 128 ? 2 : 3));
        if (M != 1 && M != 2 && M != 3 && (M < 63 || M > 66) && (M < 127 || M > 130) && M < 255) continue;
        for (long rows : seams) {
            long segs = 0;
            for (long q = 0; q < rows; q += 64) ++segs;
            const int classes = gram_classes(M, rows);
            EXPECT(gram_segments(rows) == segs && classes == (segs < cap ? segs : cap) && classes >= 1);
            // every segment belongs to exactly one class, and no class is empty
            std::vector<int> owner(static_cast<size_t>(segs), -1), count(static_cast<size_t>(classes), 0);
            for (int g = 0; g < classes; ++g)
                for (long q = g; q < segs; q += classes) {
                    EXPECT(owner[static_cast<size_t>(q)] == -1);
                    owner[static_cast<size_t>(q)] = g, ++count[static_cast<size_t>(g)];
                }
            for (int v : owner) EXPECT(v >= 0);
            for (int v : count) EXPECT(v >= 1);
        }
    }
    // more rows than an int holds
    EXPECT(gram_segments(3L << 31) == 3L << 25 && gram_classes(256, 3L << 31) == 64);
    EXPECT(gram_form_nb(1) == 1 && gram_form_nb(2) == 2 && gram_form_nb(3) == 4);
    // the steps of the workgroup count that the forms' tests sit at
    EXPECT(gram_shares(4, 1) == 1 && gram_shares(88, 1) == 1 && gram_shares(89, 1) == 2);
    EXPECT(gram_shares(124, 2) == 1 && gram_shares(125, 2) == 2 && gram_shares(176, 4) == 1 && gram_shares(177, 4) == 2);
    return true;
}

}  // namespace

int main() {
    for (int cols = 1; cols <= ESPACE_MAX_MEMBERS + 1; ++cols)
        for (int NB : {1, 2, 4})
            if (!check_geometry(cols, NB)) return 1;
    for (int M = 1; M <= ESPACE_MAX_MEMBERS; ++M)
        for (int K = 1; K <= DOT_MAX_FIELDS; ++K)
            if (!check_dot(M, K)) return 1;
    if (!check_plan()) return 1;
    std::printf("gram plan host ok\n");
    return 0;
}
