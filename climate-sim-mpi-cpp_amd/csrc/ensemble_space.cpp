// ensemble_space.cpp — the ensemble-space calls: csim_ensemble_gram, _project, _transform and their composite
// csim_ensemble_eofs (kernels in ensemble_space.hip, the eigensolver in sym_eigen.cpp), and csim_ensemble_dot (kernels
// in ensemble_dot.hip; its two steps are shared with csim_ensemble_obs_impact_global of ensemble_obs_impact.cpp).  Every
// argument check on the members is csim_ensemble_space_check, which needs no device.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ensemble_host.hpp"
#include "sym_eigen.hpp"

#pragma clang fp contract(off)

using namespace csim;

namespace {

// the checks of a call on ensemble e; *M forecast members without member *t
int space_check(const csim_ensemble* e, int truth_member, int centered, int K, int has_wbar, int n_modes, int* M,
                int* t) {
    CSIM_TRY(csim_ensemble_space_check(e->g.members, truth_member, centered, K, has_wbar, n_modes));
    CSIM_REQUIRE(e->g.slab <= 0x7fffffffL, "grid too large for the ensemble-space kernels");
    return forecast_split(e->g.members, truth_member, M, t);
}

// W (rows x cols) and, behind it, wbar (rows values; null: none) to the device, copied before the call returns
int stage_weights(csim_ensemble* e, int rows, int cols, const double* W, const double* wbar) {
    csim_ensemble::Espace& x = e->espace;
    const size_t nw = static_cast<size_t>(rows) * cols, n = nw + (wbar ? rows : 0);
    void* h = nullptr;
    CSIM_TRY(x.w.reserve(sizeof(double) * n, e->st));
    CSIM_TRY(x.stage.acquire(sizeof(double) * n, &h));
    std::copy(W, W + nw, static_cast<double*>(h));
    if (wbar) std::copy(wbar, wbar + rows, static_cast<double*>(h) + nw);
    return x.stage.send(x.w.p, sizeof(double) * n, e->st);
}

// G (M x M) of the current state, synchronous
int gram(csim_ensemble* e, int M, int t, bool centered, double* G) {
    const EnsGeom& g = e->g;
    csim_ensemble::Espace& x = e->espace;
    const size_t gbytes = sizeof(double) * static_cast<size_t>(M) * M;
    CSIM_TRY(x.partial.reserve(sizeof(double) * gram_classes(M, static_cast<long>(g.nx) * g.ny) * gram_pairs(M), e->st));
    CSIM_TRY(x.gram.reserve(gbytes, e->st));
    CSIM_HIP(ens_launch_gram(g, e->base(e->cur), M, t, centered, x.partial.as(), x.gram.as(), x.gram_form, e->st));
    CSIM_HIP(hipMemcpyAsync(G, x.gram.p, gbytes, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

// K dense fields out_r = sum_k p_k W[k K + r] of the current state, synchronous
int project(csim_ensemble* e, int M, int t, bool centered, int K, const double* W, double* out) {
    csim_ensemble::Espace& x = e->espace;
    const size_t bytes = sizeof(double) * stats_cells(e) * K;
    CSIM_TRY(x.out.reserve(bytes, e->st));
    CSIM_TRY(stage_weights(e, M, K, W, nullptr));
    CSIM_HIP(ens_launch_project(e->g, e->base(e->cur), M, t, centered, K, x.w.as(), x.out.as(), x.project_form, e->st));
    CSIM_HIP(hipMemcpyAsync(out, x.out.p, bytes, hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

}  // namespace

namespace csim {

int dot_stage_fields(csim_ensemble* e, int K, const double* fields) {
    csim_ensemble::Espace& x = e->espace;
    const EnsGeom& g = e->g;
    const size_t nx = static_cast<size_t>(g.nx), nx2 = nx + 2, inner = nx * g.ny, dense = stats_cells(e);
    const size_t bytes = sizeof(double) * inner * K;
    void* h = nullptr;
    CSIM_TRY(x.dot_fields.reserve(bytes, e->st));
    CSIM_TRY(x.stage.acquire(bytes, &h));
    auto* packed = static_cast<double*>(h);
    for (int r = 0; r < K; ++r)
        for (int j = 1; j <= g.ny; ++j) {
            const double* src = fields + r * dense + j * nx2 + 1;
            std::copy(src, src + nx, packed + r * inner + (j - 1) * nx);
        }
    return x.stage.send(x.dot_fields.p, bytes, e->st);
}

int dot_enqueue(csim_ensemble* e, int M, int t, bool centered, int K) {
    csim_ensemble::Espace& x = e->espace;
    CSIM_TRY(x.dot_partial.reserve(sizeof(double) * ens_dot_partial_doubles(e->g, M, K), e->st));
    CSIM_TRY(x.dot_out.reserve(sizeof(double) * static_cast<size_t>(M) * K, e->st));
    CSIM_HIP(ens_launch_dot(e->g, e->base(e->cur), M, t, centered, K, x.dot_fields.as(), x.dot_partial.as(),
                            x.dot_out.as(), e->st));
    return CSIM_OK;
}

}  // namespace csim

extern "C" {

int csim_ensemble_space_check(int members, int truth_member, int centered, int K, int has_wbar, int n_modes) {
    CSIM_REQUIRE(members >= 1, "members must be >= 1");
    int M = 0, t = 0;
    CSIM_TRY(forecast_split(members, truth_member, &M, &t, 1, "no forecast member", ESPACE_MAX_MEMBERS,
                            "ensemble space: at most CSIM_ESPACE_MAX_MEMBERS forecast members"));
    CSIM_REQUIRE(centered == 0 || centered == 1, "centered must be 0 or 1");
    CSIM_REQUIRE(K >= 0 && K <= M, "K must be 1 .. M");
    CSIM_REQUIRE(!(has_wbar && !centered), "wbar needs centered = 1");
    CSIM_REQUIRE(n_modes >= 0 && n_modes <= M - 1 + (n_modes == 0), "n_modes must be 1 .. M - 1");
    return CSIM_OK;
}

int csim_ensemble_gram_plan(int M, int nx, int ny, long* nseg, int* classes) {
    CSIM_REQUIRE(M >= 1 && nx >= 1 && ny >= 1, "M, nx and ny must be >= 1");
    if (M > ESPACE_MAX_MEMBERS)
        return fail(CSIM_ERR_UNSUPPORTED, "ensemble space: at most CSIM_ESPACE_MAX_MEMBERS forecast members");
    const long cells = static_cast<long>(nx) * ny;
    if (nseg) *nseg = gram_segments(cells);
    if (classes) *classes = gram_classes(M, cells);
    return CSIM_OK;
}

int csim_sym_eigen(int n, const double* A, double* lambda, double* V, int* sweeps) {
    CSIM_REQUIRE(A && lambda && V, "null argument");
    CSIM_REQUIRE(n >= 1, "n must be >= 1");
    if (n > SYM_EIGEN_MAX_N) return fail(CSIM_ERR_UNSUPPORTED, "csim_sym_eigen: n is at most CSIM_SYM_EIGEN_MAX_N");
    CSIM_REQUIRE(sym_eigen(n, A, lambda, V, sweeps), "csim_sym_eigen: a non-finite entry");
    return CSIM_OK;
}

int csim_sym_eigen_ordered(int n, const double* A, int order, double* lambda, double* V, int* sweeps) {
    CSIM_REQUIRE(A && lambda && V, "null argument");
    CSIM_REQUIRE(n >= 1, "n must be >= 1");
    if (n > SYM_EIGEN_MAX_N) return fail(CSIM_ERR_UNSUPPORTED, "csim_sym_eigen: n is at most CSIM_SYM_EIGEN_MAX_N");
    CSIM_REQUIRE(order == CSIM_EIGEN_ROWS || order == CSIM_EIGEN_ROUND_ROBIN,
                 "order must be CSIM_EIGEN_ROWS or CSIM_EIGEN_ROUND_ROBIN");
    CSIM_REQUIRE(sym_eigen_ordered(n, A, order, lambda, V, sweeps), "csim_sym_eigen: a non-finite entry");
    return CSIM_OK;
}

int csim_sym_eigen_device_form(int n, int form, int* chosen, int* max_n) {
    CSIM_REQUIRE(form >= 0 && form <= EIGEN_FORMS, "form must be 0 (automatic) or 1 .. 3");
    CSIM_REQUIRE(n >= 1, "n must be >= 1");
    if (n > SYM_EIGEN_MAX_N) return fail(CSIM_ERR_UNSUPPORTED, "csim_sym_eigen: n is at most CSIM_SYM_EIGEN_MAX_N");
    if (max_n) *max_n = form ? eigen_form_max_n(form) : SYM_EIGEN_MAX_N;
    if (!eigen_device_form(n, form))
        return fail(CSIM_ERR_UNSUPPORTED, "csim_sym_eigen_device_form: the form does not admit this n");
    if (chosen) *chosen = eigen_device_form(n, form);
    return CSIM_OK;
}

int csim_sym_eigen_batch_gpu(int n, int batch, const double* A, double* lambda, double* V, int* sweeps, int* status,
                             int form) {
    CSIM_REQUIRE(A && lambda && V, "null argument");
    CSIM_REQUIRE(n >= 1, "n must be >= 1");
    CSIM_REQUIRE(batch >= 1 && batch <= CSIM_SYM_EIGEN_MAX_BATCH, "batch must be 1 .. CSIM_SYM_EIGEN_MAX_BATCH");
    CSIM_TRY(csim_sym_eigen_device_form(n, form, nullptr, nullptr));
    // the call owns what it needs: a stream and one buffer for a chunk of the batch (inputs, working matrices, V, lambda
    // and info), at most 512 MiB, so that any batch runs in bounded memory
    const size_t nn = static_cast<size_t>(n) * n, per = 4 * nn + n + 1;  // doubles per matrix
    const int chunk = static_cast<int>(std::clamp<size_t>((size_t(1) << 26) / per, 1, static_cast<size_t>(batch)));
    DeviceBuf buf;
    hipStream_t st = nullptr;
    CSIM_HIP(hipStreamCreate(&st));
    auto run = [&]() -> int {
        CSIM_TRY(buf.reserve(sizeof(double) * per * chunk));
        double* dA = buf.as();
        double* work = dA + nn * chunk;
        double* dV = work + 2 * nn * chunk;
        double* dl = dV + nn * chunk;
        int* info = reinterpret_cast<int*>(dl + static_cast<size_t>(n) * chunk);
        std::vector<int> got(2 * static_cast<size_t>(chunk));
        for (int b0 = 0; b0 < batch; b0 += chunk) {
            const int nb = std::min(chunk, batch - b0);
            CSIM_HIP(hipMemcpyAsync(dA, A + nn * b0, sizeof(double) * nn * nb, hipMemcpyHostToDevice, st));
            CSIM_HIP(ens_launch_sym_eigen(n, nb, dA, n, static_cast<long>(nn), work, dl, dV, info, form, st));
            CSIM_HIP(hipMemcpyAsync(lambda + static_cast<size_t>(n) * b0, dl, sizeof(double) * n * nb,
                                    hipMemcpyDeviceToHost, st));
            CSIM_HIP(hipMemcpyAsync(V + nn * b0, dV, sizeof(double) * nn * nb, hipMemcpyDeviceToHost, st));
            CSIM_HIP(hipMemcpyAsync(got.data(), info, sizeof(int) * 2 * nb, hipMemcpyDeviceToHost, st));
            CSIM_HIP(hipStreamSynchronize(st));
            for (int b = 0; b < nb; ++b) {
                if (sweeps) sweeps[b0 + b] = got[2 * static_cast<size_t>(b)];
                if (status) status[b0 + b] = got[2 * static_cast<size_t>(b) + 1];
            }
        }
        return CSIM_OK;
    };
    int rc = CSIM_OK;
    try {
        rc = run();
    } catch (const std::bad_alloc&) {
        rc = fail(CSIM_ERR_STATE, "csim_sym_eigen_batch_gpu: out of host memory");
    }
    (void)hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    buf.release();
    return rc;
}

int csim_ensemble_gram(csim_ensemble* e, int truth_member, int centered, double* G) {
    CSIM_REQUIRE(e && G, "null argument");
    int M = 0, t = 0;
    CSIM_TRY(space_check(e, truth_member, centered, 0, 0, 0, &M, &t));
    return gram(e, M, t, centered == 1, G);
}

int csim_ensemble_project(csim_ensemble* e, int truth_member, int centered, int K, const double* W, double* out) {
    CSIM_REQUIRE(e && W && out, "null argument");
    CSIM_REQUIRE(K >= 1, "K must be 1 .. M");
    int M = 0, t = 0;
    CSIM_TRY(space_check(e, truth_member, centered, K, 0, 0, &M, &t));
    return project(e, M, t, centered == 1, K, W, out);
}

int csim_ensemble_dot(csim_ensemble* e, int truth_member, int centered, int K, const double* fields, double* out) {
    CSIM_REQUIRE(e, "null ensemble");
    int M = 0, t = 0;
    CSIM_TRY(space_check(e, truth_member, centered, 0, 0, 0, &M, &t));
    CSIM_REQUIRE(K >= 1 && K <= DOT_MAX_FIELDS, "K must be 1 .. CSIM_DOT_MAX_FIELDS");
    CSIM_REQUIRE(fields && out, "null argument");
    for (int r = 0; r < K; ++r)
        CSIM_REQUIRE(interior_finite(fields + r * stats_cells(e), e->g.nx, e->g.ny),
                     "every interior value of a field must be finite");
    CSIM_TRY(dot_stage_fields(e, K, fields));
    CSIM_TRY(dot_enqueue(e, M, t, centered == 1, K));
    CSIM_HIP(hipMemcpyAsync(out, e->espace.dot_out.p, sizeof(double) * static_cast<size_t>(M) * K,
                            hipMemcpyDeviceToHost, e->st));
    CSIM_HIP(hipStreamSynchronize(e->st));
    return CSIM_OK;
}

int csim_ensemble_transform(csim_ensemble* e, int truth_member, int centered, const double* W, const double* wbar) {
    CSIM_REQUIRE(e && W, "null argument");
    int M = 0, t = 0;
    CSIM_TRY(space_check(e, truth_member, centered, 0, wbar != nullptr, 0, &M, &t));
    CSIM_TRY(stage_weights(e, M, M, W, wbar));
    const double* w = e->espace.w.as();
    // Only interior cells of the forecast members in the current buffer are written, as by csim_ensemble_relax:
    // nothing cached goes stale (see there)
    CSIM_HIP(ens_launch_transform(e->g, e->base(e->cur), M, t, centered == 1, w,
                                  wbar ? w + static_cast<size_t>(M) * M : nullptr, e->espace.project_form, e->st));
    return CSIM_OK;
}

int csim_ensemble_eofs(csim_ensemble* e, int truth_member, int n_modes, double* lambda, double* pcs, double* patterns,
                       int* n_valid) {
    CSIM_REQUIRE(e && lambda && pcs, "null argument");
    CSIM_REQUIRE(n_modes >= 1, "n_modes must be 1 .. M - 1");
    int M = 0, t = 0;
    CSIM_TRY(space_check(e, truth_member, 1, 0, 0, n_modes, &M, &t));
    const size_t m = static_cast<size_t>(M), K = static_cast<size_t>(n_modes);
    std::vector<double> G(m * m), lam(m), V(m * m), W(m * K);
    CSIM_TRY(gram(e, M, t, true, G.data()));
    CSIM_REQUIRE(sym_eigen(M, G.data(), lam.data(), V.data(), nullptr),
                 "csim_ensemble_eofs: the Gram matrix has a non-finite entry");
    const double floor = (static_cast<double>(M) * 0x1p-52) * lam[0];
    std::vector<char> null_mode(K);
    int valid = 0;
    for (size_t r = 0; r < K; ++r) {
        lambda[r] = lam[r];
        null_mode[r] = lam[r] <= floor || lam[r] <= 0.0;
        valid += !null_mode[r];
        const double root = null_mode[r] ? 0.0 : std::sqrt(lam[r]);
        for (size_t k = 0; k < m; ++k) {
            W[k * K + r] = null_mode[r] ? 0.0 : V[k * m + r] / root;
            pcs[k * K + r] = null_mode[r] ? 0.0 : V[k * m + r] * root;
        }
    }
    if (n_valid) *n_valid = valid;
    if (!patterns) return CSIM_OK;
    CSIM_TRY(project(e, M, t, true, n_modes, W.data(), patterns));
    const size_t cells = stats_cells(e);
    for (size_t r = 0; r < K; ++r)
        if (null_mode[r]) std::fill(patterns + r * cells, patterns + (r + 1) * cells, 0.0);
    return CSIM_OK;
}

}  // extern "C"
