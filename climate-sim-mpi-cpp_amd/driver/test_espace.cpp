// test_espace.cpp — the ensemble-space calls through climate::Ensemble (include/climate/ensemble.hpp) on a GPU:
// Ensemble::gram, project, transform, eofs and climate::sym_eigen against the C entry points on a twin (the same bits)
// on one 130 x 67 case of 12 forecast members, and what is refused.
// Prints "espace ok" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstring>
#include <random>

#include "climate/ensemble.hpp"

#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            return 1;                                                  \
        }                                                              \
    } while (0)

template <class F> static bool throws(F&& f) {
    try {
        f();
    } catch (const std::exception&) {
        return true;
    }
    return false;
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0);
}

int main() {
    const int B = 13, t = 4, M = B - 1, nx = 130, ny = 67, K = 3, bc[4] = {0, 1, 2, 0};
    const std::size_t cells = static_cast<std::size_t>(nx + 2) * (ny + 2);
    std::mt19937_64 gen(7);
    std::normal_distribution<double> normal;
    std::vector<double> X(static_cast<std::size_t>(B) * cells);
    for (double& v : X) v = 2.0 + normal(gen);
    std::vector<double> W(static_cast<std::size_t>(M) * K), T(static_cast<std::size_t>(M) * M), wbar(M);
    for (double& v : W) v = normal(gen);
    for (double& v : T) v = 0.1 * normal(gen);
    for (int k = 0; k < M; ++k) T[static_cast<std::size_t>(k) * M + k] += 1.0;
    for (double& v : wbar) v = 0.1 * normal(gen);

    // the C++ methods on one ensemble, the C entry points on its twin
    climate::Ensemble a(B, nx, ny, 1.0, 1.0, bc);
    a.upload_all(X);
    csim_ensemble* eb = nullptr;
    EXPECT(csim_ensemble_create(B, nx, ny, 1, 1.0, 1.0, bc, 0.0, &eb) == CSIM_OK);
    EXPECT(csim_ensemble_upload_all(eb, X.data()) == CSIM_OK);

    std::vector<double> G(static_cast<std::size_t>(M) * M), out(K * cells);
    EXPECT(csim_ensemble_gram(eb, t, 1, G.data()) == CSIM_OK);
    EXPECT(same_bits(a.gram(t), G));
    for (int p = 0; p < M; ++p)
        for (int q = 0; q < M; ++q) EXPECT(G[p * M + q] == G[q * M + p] && (p != q || G[p * M + q] > 0.0));
    EXPECT(csim_ensemble_gram(eb, -1, 0, std::vector<double>(B * B).data()) == CSIM_OK);
    EXPECT(a.gram(-1, false).size() == static_cast<std::size_t>(B) * B);
    EXPECT(csim_ensemble_project(eb, t, 1, K, W.data(), out.data()) == CSIM_OK);
    EXPECT(same_bits(a.project(W, K, t), out));

    // the eigensolver and the composite
    const climate::SymEigen e = climate::sym_eigen(G, M);
    std::vector<double> lam(M), V(static_cast<std::size_t>(M) * M);
    int sweeps = -1;
    EXPECT(csim_sym_eigen(M, G.data(), lam.data(), V.data(), &sweeps) == CSIM_OK);
    EXPECT(same_bits(e.lambda, lam) && same_bits(e.V, V) && e.sweeps == sweeps && sweeps > 0);
    for (int r = 0; r + 1 < M; ++r) EXPECT(lam[r] >= lam[r + 1]);
    const climate::EnsembleEOFs f = a.eofs(K, t);
    std::vector<double> flam(K), fpcs(static_cast<std::size_t>(M) * K), fpat(K * cells);
    int valid = -1;
    EXPECT(csim_ensemble_eofs(eb, t, K, flam.data(), fpcs.data(), fpat.data(), &valid) == CSIM_OK);
    EXPECT(same_bits(f.lambda, flam) && same_bits(f.pcs, fpcs) && same_bits(f.patterns, fpat));
    EXPECT(f.n_valid == valid && valid == K && f.variance[0] == flam[0] / (M - 1) && flam[0] == lam[0]);
    EXPECT(a.eofs(K, t, false).patterns.empty());

    // the transform: enqueued, the truth member and the ghost ring keep their bits
    a.transform(T, wbar, t);
    EXPECT(csim_ensemble_transform(eb, t, 1, T.data(), wbar.data()) == CSIM_OK);
    std::vector<double> A = a.download_all(), Bv(X.size());
    EXPECT(csim_ensemble_download_all(eb, Bv.data()) == CSIM_OK);
    EXPECT(same_bits(A, Bv) && !same_bits(A, X));
    EXPECT(std::memcmp(&A[t * cells], &X[t * cells], sizeof(double) * cells) == 0);
    EXPECT(std::memcmp(A.data(), X.data(), sizeof(double) * (nx + 2)) == 0 && A[(nx + 2) + 1] != X[(nx + 2) + 1]);
    a.transform(T, {}, t, false);
    EXPECT(csim_ensemble_transform(eb, t, 0, T.data(), nullptr) == CSIM_OK);
    A = a.download_all();
    EXPECT(csim_ensemble_download_all(eb, Bv.data()) == CSIM_OK);
    EXPECT(same_bits(A, Bv));

    // refused
    EXPECT(throws([&] { a.project(W, K + 1, t); }));                      // W is not M x K
    EXPECT(throws([&] { a.project(std::vector<double>(M * (M + 1)), M + 1, t); }));  // K > M
    EXPECT(throws([&] { a.transform(T, wbar, t, false); }));              // wbar without centering
    EXPECT(throws([&] { a.transform(W, {}, t); }));
    EXPECT(throws([&] { a.eofs(M, t); }));                                // n_modes > M - 1
    EXPECT(throws([&] { a.gram(B); }));
    EXPECT(throws([&] { climate::sym_eigen({1.0, 2.0, 3.0}, 2); }));
    EXPECT(throws([&] { climate::sym_eigen({}, 0); }));
    EXPECT(same_bits(a.download_all(), A));

    EXPECT(csim_ensemble_destroy(eb) == CSIM_OK);
    std::printf("espace ok\n");
    return 0;
}
