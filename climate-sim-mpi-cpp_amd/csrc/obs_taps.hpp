// obs_taps.hpp — the host-only part of the observations that needs neither a device nor the HIP headers (as
// assim_plan.hpp on top of it): the byte layouts of the buffers of the analysis (ensemble_da.cpp) and of a network
// (ensemble_obs.cpp) and, in obs_taps.cpp, the tap builders and the check of linear observations (csim_obs_taps_bilinear,
// csim_obs_taps_box, csim_obs_linear_check).  tools/*_host_check.cpp compile them with plain g++ under AddressSanitizer.
#pragma once
#include <cstddef>
#include <string>

#include "csim.h"

namespace csim {

int fail(int code, const std::string& msg);  // api.cpp
// the argument check of every host unit (stepper.hpp's CSIM_REQUIRE is this one)
#define OBS_REQUIRE(cond, msg)                                \
    do {                                                      \
        if (!(cond)) return ::csim::fail(CSIM_ERR_ARG, msg);  \
    } while (0)

// every array of a device buffer starts at a multiple of 256 bytes
inline size_t up(size_t b) { return (b + 255) & ~size_t(255); }

// byte layout of csim_ensemble_assimilate's buffer: the staged inputs (y, r, table, i, j, input index), then the
// device-only scalars (3 per observation), prior and posterior diagnostics (2 each) and one batch's h'_k
struct AssimLayout {
    size_t y, r, rho, i, j, idx, staged, scal, prior, post, hp, total;
};
inline AssimLayout assim_layout(size_t n, size_t tcells, size_t hp) {
    AssimLayout l{};
    l.y = 0;
    l.r = up(l.y + 8 * n);
    l.rho = up(l.r + 8 * n);
    l.i = up(l.rho + 8 * tcells);
    l.j = up(l.i + 4 * n);
    l.idx = up(l.j + 4 * n);
    l.staged = up(l.idx + 4 * n);
    l.scal = l.staged;
    l.prior = up(l.scal + 24 * n);
    l.post = up(l.prior + 16 * n);
    l.hp = up(l.post + 16 * n);
    l.total = up(l.hp + 8 * hp);
    return l;
}

// Written once at create: i, j, idx, r, sr (plan order), pos (by input index), the table, and of a linear network the
// taps: tstart (plan order, n + 1 values), toff (the packed cell offset dj * pitch + di of each tap) and tw, both in
// plan order of their observations.  Then y and xt (plan order), the analysis's scalars and one batch's h'_k, the
// background and posterior diagnostics (2 per input index each), the chunk sums of the last record and the log.
// Screening comes last, so that everything before it stays where it was: the active mask and the status bytes (plan
// order), (hb, vb) of an unrecorded background check (2 per input index, never fetched), the chunk counts and the
// screen log.
struct ObsLayout {
    size_t i, j, idx, pos, r, sr, rho, tstart, toff, tw, fixed, y, xt, scal, bg, post, part, hp, log, mask, status, sbg,
        cnt, slog, total;
};
// n observations, ntaps taps in all (0: a point network, which has no tap arrays), tcells table cells, hp doubles of
// h'_k, part doubles of chunk sums, logd doubles of log, cnt ints of chunk counts, slogd doubles of screen log
inline ObsLayout obs_layout(size_t n, size_t ntaps, size_t tcells, size_t hp, size_t part, size_t logd, size_t cnt = 0,
                            size_t slogd = 0) {
    ObsLayout l{};
    l.i = 0;
    l.j = up(l.i + 4 * n);
    l.idx = up(l.j + 4 * n);
    l.pos = up(l.idx + 4 * n);
    l.r = up(l.pos + 4 * n);
    l.sr = up(l.r + 8 * n);
    l.rho = up(l.sr + 8 * n);
    l.tstart = up(l.rho + 8 * tcells);
    l.toff = up(l.tstart + (ntaps ? 4 * (n + 1) : 0));
    l.tw = up(l.toff + 4 * ntaps);
    l.fixed = up(l.tw + 8 * ntaps);
    l.y = l.fixed;
    l.xt = up(l.y + 8 * n);
    l.scal = up(l.xt + 8 * n);
    l.bg = up(l.scal + 24 * n);
    l.post = up(l.bg + 16 * n);
    l.part = up(l.post + 16 * n);
    l.hp = up(l.part + 8 * part);
    l.log = up(l.hp + 8 * hp);
    l.mask = up(l.log + 8 * logd);
    l.status = up(l.mask + n);
    l.sbg = up(l.status + n);
    l.cnt = up(l.sbg + 16 * n);
    l.slog = up(l.cnt + 4 * cnt);
    l.total = up(l.slog + 8 * slogd);
    return l;
}

// the taps of a linear network in plan order: observation idx[q] of the input is plan position q.  tstart: n + 1
// values, toff / tw: start[n] values each; a tap's offset from its anchor in a member's slab is dj * pitch + di
inline void obs_taps_plan_order(int n, const int* idx, const int* start, const int* di, const int* dj, const double* w,
                                int pitch, int* tstart, int* toff, double* tw) {
    int at = 0;
    for (int q = 0; q < n; ++q) {
        const int o = idx[q];
        tstart[q] = at;
        for (int s = start[o]; s < start[o + 1]; ++s, ++at) toff[at] = dj[s] * pitch + di[s], tw[at] = w[s];
    }
    tstart[n] = at;
}

}  // namespace csim
