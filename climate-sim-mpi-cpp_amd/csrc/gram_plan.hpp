// gram_plan.hpp — the plan and the geometry of a Gram sum G = X^T X over the rows of X, `cols` columns wide:
// csim_ensemble_gram (rows: interior cells, cols = M) and csim_ensemble_obs_gram (rows: plan positions of a network,
// cols = M + 1).  Plain host code without the HIP headers; the device part is gram_tile.hpp, and
// tools/gram_plan_host_check.cpp checks what is here on the CPU.
// The plan: segments of GRAM_SEG rows; class g of Gc = min(segments, cap(M)) sums the segments g, g + Gc, ... in order,
// and the classes' partials are folded in class order.  The geometry: the upper triangle of G in blocks of GRAM_TB x
// GRAM_TB pairs, nblk per side, numbered row by row; workgroup `share` of a class gives its lane `lane` the NB blocks
// (share NB + u) GRAM_THREADS + lane, u < NB, and a lane past the end works on the last block and stores nothing.
// The ensemble-space dot (csim_ensemble_dot: rows interior cells, M columns against K field columns) takes the plan as
// it is and has a rectangle for a geometry: its blocks, its field rows in LDS and its LDS size are at the end.
#pragma once

#include <cstddef>

#if defined(__HIP__)
#define CSIM_GRAM_HD __host__ __device__
#else
#define CSIM_GRAM_HD
#endif

namespace csim {

constexpr int ESPACE_MAX_MEMBERS = 256;  // CSIM_ESPACE_MAX_MEMBERS
constexpr int DOT_MAX_FIELDS = 16;       // CSIM_DOT_MAX_FIELDS
constexpr int GRAM_SEG = 64;             // rows per segment
constexpr int GRAM_FORMS = 3;            // gram_form, obs_gram_form 1 .. 3: 1, 2, 4 blocks of 4 x 4 pairs per lane
constexpr int GRAM_THREADS = 256;        // lanes of a workgroup
constexpr int GRAM_TB = 4;               // pairs per block side

// classes of the sum for M forecast members (0: M out of range)
inline int gram_cap(int M) { return M < 1 ? 0 : M <= 64 ? 1024 : M <= 128 ? 256 : M <= ESPACE_MAX_MEMBERS ? 64 : 0; }
inline long gram_segments(long rows) { return (rows + GRAM_SEG - 1) / GRAM_SEG; }
inline int gram_classes(int M, long rows) {
    const long nseg = gram_segments(rows);
    return static_cast<int>(nseg < gram_cap(M) ? nseg : gram_cap(M));
}
// the form taken for gram_form = 0, and the blocks per lane of a form
inline int gram_auto_form(int M) { return M <= 64 ? 1 : M <= 128 ? 2 : 3; }
constexpr int gram_form_nb(int form) { return form == 1 ? 1 : form == 2 ? 2 : 4; }

CSIM_GRAM_HD inline int gram_nblk(int cols) { return (cols + GRAM_TB - 1) / GRAM_TB; }
CSIM_GRAM_HD inline int gram_nblocks(int cols) { return gram_nblk(cols) * (gram_nblk(cols) + 1) / 2; }
// doubles between a segment's rows in LDS: even and past the padded width, so a block side is two aligned 16-byte reads
CSIM_GRAM_HD inline int gram_stride(int cols) { return gram_nblk(cols) * GRAM_TB + 2; }
// workgroups per class
inline int gram_shares(int cols, int NB) { return (gram_nblocks(cols) + NB * GRAM_THREADS - 1) / (NB * GRAM_THREADS); }

// the packed upper triangle: gram_pairs entries, (a, b) with a <= b at gram_packed
CSIM_GRAM_HD inline size_t gram_pairs(int cols) { return static_cast<size_t>(cols) * (cols + 1) / 2; }
CSIM_GRAM_HD inline size_t gram_packed(int a, int b, int cols) {
    return static_cast<size_t>(a) * cols - static_cast<size_t>(a) * (a - 1) / 2 + (b - a);
}

// block bidx of the triangle: ia <= ib < nblk
struct GramBlock {
    int ia, ib;
};
CSIM_GRAM_HD inline GramBlock gram_block_of(int bidx, int nblk) {
    int r = bidx, a = 0;
    while (r >= nblk - a) r -= nblk - a, ++a;
    return {a, a + r};
}
// slot u of a lane: its block and whether the lane owns it
struct GramOwned {
    GramBlock at;
    bool mine;
};
CSIM_GRAM_HD inline GramOwned gram_owned(int share, int NB, int u, int lane, int cols) {
    const int bidx = (share * NB + u) * GRAM_THREADS + lane, nblocks = gram_nblocks(cols);
    return {gram_block_of(bidx < nblocks ? bidx : nblocks - 1, gram_nblk(cols)), bidx < nblocks};
}
// false: none of the lanes of this lane's wave owns a block
CSIM_GRAM_HD inline bool gram_wave_on(int share, int NB, int lane, int cols) {
    return share * NB * GRAM_THREADS + (lane & ~63) < gram_nblocks(cols);
}

// doubles of LDS for a segment's rows of `cols` columns and their GRAM_SEG means
CSIM_GRAM_HD inline size_t gram_lds_doubles(int cols) { return static_cast<size_t>(GRAM_SEG) * gram_stride(cols) + GRAM_SEG; }

// The rectangle of the dot, M x K sums in blocks of GRAM_TB x GRAM_TB numbered row by row, nbk = gram_nblk(K) per
// row: at most 64 x 4 = GRAM_THREADS of them, so one workgroup per class holds them all.  Lane l owns block l, member
// block l / nbk and field block l % nbk; a lane past the end works on the last block and stores nothing.
struct DotOwned {
    int im, ik;
    bool mine;
};
CSIM_GRAM_HD inline DotOwned dot_owned(int lane, int M, int K) {
    const int nbk = gram_nblk(K), nblocks = gram_nblk(M) * nbk;
    const int b = lane < nblocks ? lane : nblocks - 1;
    return {b / nbk, b % nbk, lane < nblocks};
}
// false: none of the lanes of this lane's wave owns a block
CSIM_GRAM_HD inline bool dot_wave_on(int lane, int M, int K) { return (lane & ~63) < gram_nblk(M) * gram_nblk(K); }
// doubles between the field rows of a segment in LDS: even and past the padded width, as gram_stride
CSIM_GRAM_HD inline int dot_fstride(int K) { return gram_nblk(K) * GRAM_TB + 2; }
// doubles of LDS: the rows and the means of the Gram sum, then the field rows
CSIM_GRAM_HD inline size_t dot_lds_doubles(int M, int K) {
    return gram_lds_doubles(M) + static_cast<size_t>(GRAM_SEG) * dot_fstride(K);
}

}  // namespace csim

#undef CSIM_GRAM_HD
