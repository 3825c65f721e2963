// obs_taps.hpp — the host-only part of the observation networks that needs neither a device nor the HIP headers: the
// byte layout of a network's device buffer (used by ensemble_obs.cpp) and, in obs_taps.cpp, the tap builders and the
// check of linear observations (csim_obs_taps_bilinear, csim_obs_taps_box, csim_obs_linear_check of include/csim.h).
// tools/obsop_host_check.cpp compiles both with plain g++ under AddressSanitizer.
#pragma once
#include <cstddef>
#include <string>

#include "csim.h"

namespace csim {

int fail(int code, const std::string& msg);  // api.cpp

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
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
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
