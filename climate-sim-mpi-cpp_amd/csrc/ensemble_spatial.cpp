// ensemble_spatial.cpp — neighbourhood and probability verification (csim_ensemble_verify_spatial*, kernels in
// ensemble_spatial.hip): the argument checks, the layout of the one device buffer, the two launches and the capture.
// The host-only halves, the overflow bound and the finishing of the integer tables into scores, are spatial_scores.cpp.
#include <cstring>

#include "ensemble_host.hpp"
#include "spatial_scores.hpp"

using namespace csim;

namespace {

typedef unsigned long long u64;

// the device buffer, in bytes: what the second pass adds into (zeroed per call), the fields of the first pass, and,
// never copied, the scratch planes of a split first pass
struct SpatialLayout {
    size_t table, nbh, cells, flags, counts, fields_end, acc, total;
};
SpatialLayout spatial_layout(int M, int nt, int ns, size_t ncell, int split) {
    SpatialLayout l{};
    l.table = 0;
    l.nbh = l.table + sizeof(u64) * nt * 2 * (static_cast<size_t>(M) + 1);
    l.cells = l.nbh + sizeof(u64) * nt * 3 * ns;
    l.flags = l.cells + 2 * sizeof(u64);
    l.counts = l.flags + sizeof(unsigned) * ncell;
    l.fields_end = l.counts + sizeof(unsigned short) * nt * ncell;
    l.acc = (l.fields_end + 15) & ~static_cast<size_t>(15);
    l.total = l.acc + (split > 1 ? sizeof(unsigned) * (nt + 1) * ncell : 0);
    return l;
}

// checks the arguments, prepares the capture (pinned: `copy` bytes of it), stages a host truth, and enqueues the
// zeroing and both passes on the ensemble's stream after everything enqueued so far.  *forecast, *split: of this call
int spatial_launch(csim_ensemble* e, const double* truth, int truth_member, int nt, const double* thr, int ns,
                   const int* half, bool pinned, bool fields, int* forecast, int* split) {
    CSIM_REQUIRE((truth != nullptr) != (truth_member >= 0), "give exactly one truth: a host field or a member");
    int M = 0, t = 0;
    CSIM_TRY(forecast_split(e->g.members, truth_member, &M, &t));
    CSIM_REQUIRE(nt >= 1 && nt <= VERIFY_MAX_THRESHOLDS, "nt must be 1 .. 16");
    CSIM_REQUIRE(thr, "null thresholds");
    CSIM_REQUIRE(ns >= 0 && ns <= SPATIAL_MAX_SCALES, "ns must be 0 .. 8");
    CSIM_REQUIRE(ns == 0 || half, "null half-widths");
    int hmax = 0;
    for (int s = 0; s < ns; ++s) {
        CSIM_REQUIRE(half[s] >= 0 && half[s] <= SPATIAL_MAX_HALF, "half-widths must be 0 .. 32");
        hmax = std::max(hmax, half[s]);
    }
    CSIM_REQUIRE(M >= 1, "no forecast members: a truth member needs at least two members");
    CSIM_TRY(spatial_limit(M, e->g.nx, e->g.ny, hmax));
    const size_t ncell = static_cast<size_t>(e->g.nx) * e->g.ny;
    if (ncell > (size_t(1) << 27))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_ensemble_verify_spatial: more than 2^27 interior cells");

    csim_ensemble::Spatial& v = e->spatial;
    SpatialArgs a{};
    a.forecast = M, a.truth_member = t, a.nt = nt, a.ns = ns, a.hmax = hmax;
    a.grid_max = v.grid_max;
    const int want = v.member_split > 0 ? std::min(v.member_split, M) : ens_spatial_split(static_cast<int>(ncell), M);
    const int part = (M + want - 1) / want;
    a.split = (M + part - 1) / part;  // no empty part
    for (int s = 0; s < ns; ++s) a.half[s] = half[s];
    for (int k = 0; k < nt; ++k) a.thr[k] = thr[k];

    const SpatialLayout l = spatial_layout(M, nt, ns, ncell, a.split);
    // nothing reads the buffers once the copy in flight and the kernels enqueued so far are done
    CSIM_TRY(v.cap.prepare(l.total, false, e->st));
    const size_t copy = fields ? l.fields_end : l.flags;
    if (pinned && copy > v.cap.host.cap) {
        v.cap.pending = false;  // a replaced pinned buffer has nothing to fetch any more
        CSIM_TRY(v.cap.host.reserve(copy));
    }
    if (truth) {
        const size_t bytes = sizeof(double) * stats_cells(e);
        void* h = nullptr;
        CSIM_TRY(v.truth.reserve(bytes, e->st));
        CSIM_TRY(v.stage.acquire(bytes, &h));
        std::memcpy(h, truth, bytes);
        CSIM_TRY(v.stage.send(v.truth.p, bytes, e->st));
        a.truth = v.truth.as();
    }
    void* const d = v.cap.dev.p;
    SpatialOut o{};
    o.table = buf_at<u64>(d, l.table);
    o.nbh = buf_at<u64>(d, l.nbh);
    o.cells = buf_at<u64>(d, l.cells);
    o.flags = buf_at<unsigned>(d, l.flags);
    o.counts = buf_at<unsigned short>(d, l.counts);
    o.acc = buf_at<unsigned>(d, l.acc);
    CSIM_HIP(hipMemsetAsync(d, 0, l.flags, e->st));
    CSIM_HIP(ens_launch_spatial_counts(e->g, e->base(e->cur), a, o, e->st));
    CSIM_HIP(ens_launch_spatial_scores(e->g, a, o, e->st));
    *forecast = M;
    *split = a.split;
    return CSIM_OK;
}

}  // namespace

extern "C" {

int csim_ensemble_verify_spatial(csim_ensemble* e, const double* truth, int truth_member, int nt, const double* thr,
                                 int ns, const int* half, unsigned long long* table, unsigned long long* nbh,
                                 unsigned short* counts, unsigned int* flags, unsigned long long* cells,
                                 unsigned long long* nan_cells) {
    CSIM_REQUIRE(e, "null ensemble");
    int M = 0, split = 0;
    CSIM_TRY(spatial_launch(e, truth, truth_member, nt, thr, ns, half, false, false, &M, &split));
    const size_t ncell = static_cast<size_t>(e->g.nx) * e->g.ny;
    const SpatialLayout l = spatial_layout(M, nt, ns, ncell, split);
    const char* const d = e->spatial.cap.dev.as<char>();
    u64 both[2] = {0, 0};
    const auto fetch = [&](void* dst, size_t from, size_t bytes) {
        return (dst && bytes) ? hipMemcpyAsync(dst, d + from, bytes, hipMemcpyDeviceToHost, e->st) : hipSuccess;
    };
    CSIM_HIP(fetch(table, l.table, l.nbh - l.table));
    CSIM_HIP(fetch(nbh, l.nbh, l.cells - l.nbh));
    CSIM_HIP(fetch(both, l.cells, sizeof(both)));
    CSIM_HIP(fetch(flags, l.flags, l.counts - l.flags));
    CSIM_HIP(fetch(counts, l.counts, l.fields_end - l.counts));
    CSIM_HIP(hipStreamSynchronize(e->st));
    if (cells) *cells = both[0];
    if (nan_cells) *nan_cells = both[1];
    return CSIM_OK;
}

int csim_ensemble_verify_spatial_begin(csim_ensemble* e, const double* truth, int truth_member, int nt,
                                       const double* thr, int ns, const int* half, int fields) {
    CSIM_REQUIRE(e, "null ensemble");
    CSIM_REQUIRE(fields == 0 || fields == 1, "fields must be 0 or 1");
    int M = 0, split = 0;
    CSIM_TRY(spatial_launch(e, truth, truth_member, nt, thr, ns, half, true, fields != 0, &M, &split));
    csim_ensemble::Spatial& v = e->spatial;
    const SpatialLayout l = spatial_layout(M, nt, ns, static_cast<size_t>(e->g.nx) * e->g.ny, split);
    CSIM_TRY(v.cap.begin(fields ? l.fields_end : l.flags, e->st));
    v.forecast = M, v.nt = nt, v.ns = ns, v.fields = fields;
    return CSIM_OK;
}

int csim_ensemble_verify_spatial_wait(csim_ensemble* e, const unsigned long long** table,
                                      const unsigned long long** nbh, const unsigned short** counts,
                                      const unsigned int** flags, unsigned long long* cells,
                                      unsigned long long* nan_cells) {
    CSIM_REQUIRE(e, "null ensemble");
    csim_ensemble::Spatial& v = e->spatial;
    CSIM_TRY(v.cap.wait("no spatial verification in flight: csim_ensemble_verify_spatial_begin first"));
    const SpatialLayout l = spatial_layout(v.forecast, v.nt, v.ns, static_cast<size_t>(e->g.nx) * e->g.ny, 1);
    void* const h = v.cap.host.p;
    if (table) *table = buf_at<u64>(h, l.table);
    if (nbh) *nbh = buf_at<u64>(h, l.nbh);
    if (counts) *counts = v.fields ? buf_at<unsigned short>(h, l.counts) : nullptr;
    if (flags) *flags = v.fields ? buf_at<unsigned>(h, l.flags) : nullptr;
    if (cells) *cells = buf_at<u64>(h, l.cells)[0];
    if (nan_cells) *nan_cells = buf_at<u64>(h, l.cells)[1];
    return CSIM_OK;
}

}  // extern "C"
