// letkf_nodes.hpp — the geometry of csim_ensemble_assimilate_letkf (include/csim.h) that the host and the kernels
// share, said once: the lattice of analysis nodes, a cell's place between them, and the bytes of a call's node storage.
// Plain code without the HIP headers; tools/letkf_plan_host_check.cpp checks what is here on the CPU.
// Along an axis of n interior cells with spacing s >= 1 there are na = 1 (n = 1) or ceil((n - 1) / s) + 1 nodes, node a
// at the cell min(1 + a s, n): the first cell, every s-th after it, and the last cell.  Cell i lies in the interval
// a = min((i - 1) / s, na - 2) and has the weight t = (i - i_a) / (i_{a+1} - i_a) on its upper node, 1 - t on the lower.
#pragma once

#include <cstddef>

#include "sym_eigen.hpp"

#if defined(__HIP__)
#define CSIM_LETKF_HD __host__ __device__
#else
#define CSIM_LETKF_HD
#endif

namespace csim {

constexpr int LETKF_MAX_NODES = 65535;            // CSIM_LETKF_MAX_NODES: the batch limit of the device eigensolver
constexpr long long LETKF_MAX_BYTES = 1LL << 30;  // CSIM_LETKF_MAX_BYTES
constexpr int LETKF_OK = 0, LETKF_IDLE = 1, LETKF_NONFINITE = 2, LETKF_NOT_CONVERGED = 3;  // CSIM_LETKF_*
constexpr int LETKF_FORMS = 1;                    // letkf_form 1: a cell's members in LDS whatever M

CSIM_LETKF_HD inline int letkf_axis_nodes(int n, int s) {
    return n <= 1 ? 1 : static_cast<int>((static_cast<long long>(n) - 2) / s) + 2;
}
CSIM_LETKF_HD inline int letkf_node_at(int a, int s, int n) {
    const long long p = 1 + static_cast<long long>(a) * s;
    return p < n ? static_cast<int>(p) : n;
}
// the interval of cell i and the weight of its upper node; one node along the axis: interval 0, weight +0
struct LetkfAxis {
    int a;
    double t;
};
CSIM_LETKF_HD inline LetkfAxis letkf_axis_blend(int i, int s, int n, int na) {
    if (na < 2) return {0, 0.0};
    const long long q = (static_cast<long long>(i) - 1) / s;
    const int a = static_cast<int>(q < na - 2 ? q : na - 2);
    const int lo = letkf_node_at(a, s, n), hi = letkf_node_at(a + 1, s, n);
    return {a, static_cast<double>(i - lo) / static_cast<double>(hi - lo)};
}
// the four weights of a cell in the order (a, b), (a + 1, b), (a, b + 1), (a + 1, b + 1)
CSIM_LETKF_HD inline void letkf_weights4(double tx, double ty, double beta[4]) {
    const double ax = 1.0 - tx, ay = 1.0 - ty;
    beta[0] = ay * ax, beta[1] = ay * tx, beta[2] = ty * ax, beta[3] = ty * tx;
}

// Byte layout of the node storage of one call for M forecast members: per node A ((M + 1)^2), what the solver's form
// keeps in global memory (nothing, or its 2 M^2 doubles), V, lambda, W, wbar and dfs, then the integers: the solver's (sweeps,
// status), the count of local observations, and the sweeps and the status that csim_ensemble_letkf_info reports.
// form: a storage form of the solver that admits M (eigen_device_form).
struct LetkfLayout {
    size_t A, work, V, lam, W, wbar, dfs, info, count, sweeps, status, bytes;
};
inline LetkfLayout letkf_layout(int M, long nodes, int form) {
    auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
    const size_t m = static_cast<size_t>(M), n = static_cast<size_t>(nodes), d = sizeof(double);
    const size_t work = form == EIGEN_FORM_LDS ? 0 : 2 * m * m;  // the solver's stride from matrix to matrix
    LetkfLayout l{};
    l.A = 0;
    l.work = up(l.A + d * n * (m + 1) * (m + 1));
    l.V = up(l.work + d * n * work);
    l.lam = up(l.V + d * n * m * m);
    l.W = up(l.lam + d * n * m);
    l.wbar = up(l.W + d * n * m * m);
    l.dfs = up(l.wbar + d * n * m);
    l.info = up(l.dfs + d * n);
    l.count = up(l.info + sizeof(int) * 2 * n);
    l.sweeps = up(l.count + sizeof(int) * n);
    l.status = up(l.sweeps + sizeof(int) * n);
    l.bytes = up(l.status + sizeof(int) * n);
    return l;
}

}  // namespace csim

#undef CSIM_LETKF_HD
