// sym_eigen_device.hip — the Jacobi eigensolver on the device, in the round-robin order of include/csim.h
// (CSIM_EIGEN_ROUND_ROBIN), and the ETKF's weights from its result: of one matrix (k_etkf_weights, the global ETKF) and
// of a batch, one workgroup per node of an LETKF (k_letkf_weights), on the same arithmetic.  One workgroup per matrix, blockIdx.x the matrix of
// a batch; nothing synchronises across workgroups.  Every * + - / sqrt is one IEEE fp64 operation (-ffp-contract=off;
// fp64 division and square root are the correctly rounded ones), so the bits are those of sym_eigen_ordered and
// csim_etkf_weights_ordered on the host.
//
// A step of the sweep has two stages with a workgroup barrier after each:
//   1. lane k < m/2 takes slot k: its pair from eigen_rr_pair, the decisions of the host's rotate_pair on a_pp, a_qq
//      and a_pq, then s and tau into LDS; it writes the slot's own three entries (no other slot touches them);
//   2. one lane per 2 x 2 block of two slots K < L rotates the block as rows by K, then as columns by L, and stores it
//      with its mirror; further lanes rotate the rows p, q of v of every slot.  All of these are disjoint.
// Three storage forms, the same bits in each: a and v in LDS (n <= 96), a in LDS and v in global memory (n <= 128), both
// in global memory (n <= 256), where one workgroup's 16 n^2 bytes stay in L2.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ensemble.hpp"
#include "ensemble_cell.hpp"
#include "letkf_nodes.hpp"
#include "sym_eigen.hpp"

namespace csim {

namespace {

constexpr int EIGEN_SLOTS = SYM_EIGEN_MAX_N / 2;
constexpr int EIGEN_THREADS = 1024;

__device__ inline void jacobi_rotate(double& x, double& y, double s, double tau) {
    const double xn = x - s * (y + x * tau);
    const double yn = y + s * (x - y * tau);
    x = xn, y = yn;
}

struct EigenArgs {
    int n, lda;        // the matrix is n x n, its rows lda doubles apart
    long a_stride;     // doubles from one matrix of the batch to the next
    const double* A;   // input: the upper triangle is used, every entry is tested
    double* work;      // 2 n^2 doubles per matrix for what the form keeps in global memory (v, then a)
    double* lambda;    // n per matrix
    double* V;         // n x n per matrix, row-major, column r the vector of lambda[r]
    int* info;         // per matrix: sweeps, status
};

template <int FORM>
__global__ __launch_bounds__(EIGEN_THREADS) void k_sym_eigen_rr(EigenArgs g) {
    extern __shared__ __attribute__((aligned(16))) double held[];
    __shared__ double rot_s[EIGEN_SLOTS], rot_tau[EIGEN_SLOTS];
    __shared__ int rot_p[EIGEN_SLOTS], rot_q[EIGEN_SLOTS], rot_on[EIGEN_SLOTS];
    __shared__ int perm[SYM_EIGEN_MAX_N], flip[SYM_EIGEN_MAX_N];
    __shared__ int flag;

    const int n = g.n, m = n + (n & 1), S = m / 2, nn = n * n;
    const int tid = threadIdx.x, nt = blockDim.x;
    const size_t mat = blockIdx.x;
    const double* __restrict__ A = g.A + mat * g.a_stride;
    double* const work = g.work + mat * 2 * static_cast<size_t>(nn);
    double* const a = FORM == EIGEN_FORM_GLOBAL ? work + nn : held;
    double* const v = FORM == EIGEN_FORM_LDS ? held + nn : work;
    double* __restrict__ lam = g.lambda + mat * n;
    double* __restrict__ V = g.V + mat * nn;

    if (tid == 0) flag = 0;
    __syncthreads();
    for (int idx = tid; idx < nn; idx += nt) {
        const int i = idx / n, j = idx - i * n;
        if (!isfinite(A[static_cast<size_t>(i) * g.lda + j])) flag = 1;
        a[idx] = A[static_cast<size_t>(min(i, j)) * g.lda + max(i, j)];
        v[idx] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    if (flag) {  // the same for every lane: the workgroup leaves together
        const double nan = __longlong_as_double(0x7ff8000000000000LL);
        for (int idx = tid; idx < nn; idx += nt) V[idx] = nan;
        for (int idx = tid; idx < n; idx += nt) lam[idx] = nan;
        if (tid == 0) g.info[2 * mat] = 0, g.info[2 * mat + 1] = EIGEN_NONFINITE;
        return;
    }

    // the items of stage 2: the blocks K < L, rows K and S-1-K of the triangle folded into one row of S-1 blocks, then
    // n columns of v per slot
    const int fold_rows = (S + 1) / 2, fold_cols = S - 1;
    const int nblocks = fold_rows * fold_cols, nitems = nblocks + S * n;

    int done = 0;
    for (; done < SYM_EIGEN_MAX_SWEEPS; ++done) {
        __syncthreads();  // the last sweep's flag has been read, its last step is complete
        if (tid == 0) flag = 0;
        __syncthreads();
        for (int idx = tid; idx < nn; idx += nt) {
            const int i = idx / n, j = idx - i * n;
            if (i < j && a[idx] != 0.0) flag = 1;
        }
        __syncthreads();
        if (!flag) break;  // the same for every lane
        for (int t = 0; t + 1 < m; ++t) {
            if (tid < S) {
                int p, q, on = 0;
                double s = 0.0, tau = 0.0;
                eigen_rr_pair(m, t, tid, &p, &q);
                if (q < n) {
                    const double apq = a[p * n + q];
                    if (apq != 0.0) {
                        const double ga = fabs(apq);
                        const double app = a[p * n + p], aqq = a[q * n + q];
                        if (fabs(app) + ga == fabs(app) && fabs(aqq) + ga == fabs(aqq)) {
                            a[p * n + q] = a[q * n + p] = 0.0;
                        } else {
                            double h = aqq - app;
                            double tt;
                            if (fabs(h) + ga == fabs(h)) {
                                tt = apq / h;
                            } else {
                                const double theta = (0.5 * h) / apq;
                                tt = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                                if (theta < 0.0) tt = -tt;
                            }
                            const double c = 1.0 / sqrt(tt * tt + 1.0);
                            s = tt * c;
                            tau = s / (1.0 + c);
                            h = tt * apq;
                            a[p * n + p] = app - h;
                            a[q * n + q] = aqq + h;
                            a[p * n + q] = a[q * n + p] = 0.0;
                            on = 1;
                        }
                    }
                }
                rot_p[tid] = p, rot_q[tid] = q, rot_on[tid] = on, rot_s[tid] = s, rot_tau[tid] = tau;
            }
            __syncthreads();
            for (int idx = tid; idx < nitems; idx += nt) {
                if (idx < nblocks) {
                    const int r = idx / fold_cols, c = idx - r * fold_cols;
                    int K, L;
                    if (c < S - 1 - r) {
                        K = r, L = r + 1 + c;
                    } else {
                        K = S - 1 - r, L = c + 1;
                        if (K == r) continue;  // the middle row of an odd S is its own partner
                    }
                    const int onK = rot_on[K], onL = rot_on[L];
                    if (!(onK | onL)) continue;
                    const int pK = rot_p[K], qK = rot_q[K], pL = rot_p[L], qL = rot_q[L];
                    const bool hasK = qK < n, hasL = qL < n;  // an idle slot has a lone index p
                    double x00 = a[pK * n + pL];
                    double x01 = hasL ? a[pK * n + qL] : 0.0;
                    double x10 = hasK ? a[qK * n + pL] : 0.0;
                    double x11 = hasK && hasL ? a[qK * n + qL] : 0.0;
                    if (onK) {
                        const double s = rot_s[K], tau = rot_tau[K];
                        jacobi_rotate(x00, x10, s, tau);
                        jacobi_rotate(x01, x11, s, tau);
                    }
                    if (onL) {
                        const double s = rot_s[L], tau = rot_tau[L];
                        jacobi_rotate(x00, x01, s, tau);
                        jacobi_rotate(x10, x11, s, tau);
                    }
                    a[pK * n + pL] = a[pL * n + pK] = x00;
                    if (hasL) a[pK * n + qL] = a[qL * n + pK] = x01;
                    if (hasK) a[qK * n + pL] = a[pL * n + qK] = x10;
                    if (hasK && hasL) a[qK * n + qL] = a[qL * n + qK] = x11;
                } else {
                    const int w = idx - nblocks;
                    const int k = w / n, j = w - k * n;
                    if (!rot_on[k]) continue;
                    const int p = rot_p[k], q = rot_q[k];
                    double x = v[p * n + j], y = v[q * n + j];
                    jacobi_rotate(x, y, rot_s[k], rot_tau[k]);
                    v[p * n + j] = x, v[q * n + j] = y;
                }
            }
            __syncthreads();
        }
    }

    // descending, ties to the lower index: the rank of a diagonal entry is the count of those before it
    for (int i = tid; i < n; i += nt) perm[i] = i;
    __syncthreads();
    for (int i = tid; i < n; i += nt) {
        const double d = a[i * n + i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double e = a[j * n + j];
            rank += e > d || (e == d && j < i);
        }
        perm[rank] = i;
    }
    __syncthreads();
    for (int r = tid; r < n; r += nt) {
        const int src = perm[r];
        lam[r] = a[src * n + src];
        int big = 0;
        for (int j = 1; j < n; ++j)
            if (fabs(v[src * n + j]) > fabs(v[src * n + big])) big = j;
        flip[r] = v[src * n + big] < 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < nn; idx += nt) {
        const int j = idx / n, r = idx - j * n;
        const double x = v[perm[r] * n + j];
        V[idx] = flip[r] ? -x : x;
    }
    if (tid == 0) {
        g.info[2 * mat] = done;
        g.info[2 * mat + 1] = done == SYM_EIGEN_MAX_SWEEPS ? EIGEN_NOT_CONVERGED : EIGEN_OK;
    }
}

size_t eigen_lds_bytes(int n, int form) {
    const size_t nn = static_cast<size_t>(n) * n;
    return sizeof(double) * (form == EIGEN_FORM_LDS ? 2 * nn : form == EIGEN_FORM_MIXED ? nn : 0);
}

// lanes of the workgroup: enough for the items of a step, in whole waves
int eigen_threads(int n) { return n <= 8 ? 64 : n <= 24 ? 256 : n <= 48 ? 512 : EIGEN_THREADS; }

template <int FORM>
hipError_t launch_eigen(const EigenArgs& g, int batch, hipStream_t st) {
    if (FORM != EIGEN_FORM_GLOBAL) {
        const hipError_t attr = dynamic_lds_once<k_sym_eigen_rr<FORM>>(eigen_lds_bytes(eigen_form_max_n(FORM), FORM));
        if (attr != hipSuccess) return attr;
    }
    hipLaunchKernelGGL(k_sym_eigen_rr<FORM>, dim3(batch), dim3(eigen_threads(g.n)), eigen_lds_bytes(g.n, FORM), st, g);
    return hipGetLastError();
}

constexpr int WEIGHTS_THREADS = 256;

// The arithmetic of csim_etkf_weights_ordered that k_etkf_weights and k_letkf_weights share, one function per line of
// the csim.h block.  A is ma x ma, ma = M + 1; V is M x M.
__device__ __forceinline__ double etkf_clamp(double lam) { return lam > 0.0 ? lam : 0.0; }
__device__ __forceinline__ double etkf_f(double kappa, double G) { return 1.0 / (kappa + G); }
__device__ __forceinline__ double etkf_g(int M, double f) { return sqrt(static_cast<double>(M - 1) * f); }
__device__ __forceinline__ double etkf_u(int M, const double* __restrict__ V, const double* __restrict__ A, int r) {
    const int ma = M + 1;
    double u = 0.0;
    for (int a = 0; a < M; ++a) u = u + V[static_cast<size_t>(a) * M + r] * A[static_cast<size_t>(a) * ma + M];
    return u;
}
__device__ __forceinline__ double etkf_wbar_entry(int M, const double* __restrict__ V, const double* fu, int a) {
    double s = 0.0;
    for (int r = 0; r < M; ++r) s = s + V[static_cast<size_t>(a) * M + r] * fu[r];
    return s;
}
__device__ __forceinline__ double etkf_dfs(int M, const double* __restrict__ lam, double kappa) {
    double d = 0.0;
    for (int r = 0; r < M; ++r) {
        const double G = etkf_clamp(lam[r]);
        d = d + G * etkf_f(kappa, G);
    }
    return d;
}
__device__ __forceinline__ double etkf_w_entry(int M, const double* __restrict__ V, const double* gs, int a, int b) {
    double s = 0.0;
    for (int r = 0; r < M; ++r) s = s + (V[static_cast<size_t>(a) * M + r] * gs[r]) * V[static_cast<size_t>(b) * M + r];
    return s;
}

// The weights of csim_etkf_weights_ordered from A (ma x ma, ma = M + 1) and the solver's lambda, V and info.  Every
// workgroup computes f and g of every mode into LDS and then takes entries (a, b >= a) of W in a grid stride, one lane
// per entry.  Workgroup 0 also tests A, computes u, wbar, gamma and dfs and writes the record.
__global__ __launch_bounds__(WEIGHTS_THREADS) void k_etkf_weights(int M, const double* __restrict__ A,
                                                                  const double* __restrict__ lam,
                                                                  const double* __restrict__ V,
                                                                  const int* __restrict__ info, double inflation,
                                                                  double* __restrict__ W, double* __restrict__ wbar,
                                                                  EtkfRecord* __restrict__ rec,
                                                                  double* __restrict__ gamma) {
    __shared__ double gs[ESPACE_MAX_MEMBERS], fu[ESPACE_MAX_MEMBERS];
    __shared__ int bad;
    const int tid = threadIdx.x, nt = blockDim.x, ma = M + 1;
    const double rho = inflation * inflation;
    const double kappa = static_cast<double>(M - 1) / rho;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int r = tid; r < M; r += nt) {
        const double G = etkf_clamp(lam[r]);
        const double f = etkf_f(kappa, G);
        gs[r] = etkf_g(M, f);
        if (blockIdx.x == 0) {
            fu[r] = f * etkf_u(M, V, A, r);
            gamma[r] = G;
        }
    }
    if (blockIdx.x == 0)
        for (int k = tid; k < ma * ma; k += nt)
            if (!isfinite(A[k])) bad = 1;
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int a = tid; a < M; a += nt) wbar[a] = etkf_wbar_entry(M, V, fu, a);
        if (tid == 0) {
            const double d = etkf_dfs(M, lam, kappa);
            long long used;
            memcpy(&used, A + static_cast<size_t>(ma) * ma + M, sizeof used);  // the count travels behind loglik
            rec->dfs = d, rec->chi2 = A[static_cast<size_t>(ma) * ma - 1], rec->n_used = used;
            rec->sweeps = info[0];
            rec->status = bad ? ETKF_NONFINITE : used == 0 && inflation == 1.0 ? ETKF_SKIP : info[1] == EIGEN_NOT_CONVERGED ? ETKF_NOT_CONVERGED : ETKF_OK;
        }
    }
    const long pairs = static_cast<long>(M) * M;
    for (long e = static_cast<long>(blockIdx.x) * nt + tid; e < pairs; e += static_cast<long>(gridDim.x) * nt) {
        const int a = static_cast<int>(e / M), b = static_cast<int>(e - static_cast<long>(a) * M);
        if (b < a) continue;
        W[static_cast<size_t>(a) * M + b] = W[static_cast<size_t>(b) * M + a] = etkf_w_entry(M, V, gs, a, b);
    }
}

// The weights of every node of an LETKF, one workgroup per node (blockIdx.x): csim_etkf_weights_ordered with inflation
// 1 from the node's A, lambda and V.  A node without a local observation (count 0) is IDLE, one with a non-finite entry
// of A NONFINITE; both report dfs = +0 and sweeps = 0, and their W and wbar are not written.
__global__ __launch_bounds__(WEIGHTS_THREADS) void k_letkf_weights(int M, const double* __restrict__ Aall,
                                                                   const double* __restrict__ lamall,
                                                                   const double* __restrict__ Vall,
                                                                   const int* __restrict__ info,
                                                                   const int* __restrict__ count,
                                                                   double* __restrict__ Wall, double* __restrict__ wbarall,
                                                                   double* __restrict__ dfs, int* __restrict__ sweeps,
                                                                   int* __restrict__ status) {
    __shared__ double gs[ESPACE_MAX_MEMBERS], fu[ESPACE_MAX_MEMBERS];
    __shared__ int bad;
    const int tid = threadIdx.x, nt = blockDim.x, ma = M + 1;
    const size_t node = blockIdx.x, mm = static_cast<size_t>(M) * M;
    const double* __restrict__ A = Aall + node * ma * ma;
    const double* __restrict__ lam = lamall + node * M;
    const double* __restrict__ V = Vall + node * mm;
    double* __restrict__ W = Wall + node * mm;
    double* __restrict__ wbar = wbarall + node * M;
    const int n = count[node];  // the same for every lane: the workgroup leaves together
    if (tid == 0) bad = 0;
    __syncthreads();
    if (n != 0)
        for (int k = tid; k < ma * ma; k += nt)
            if (!isfinite(A[k])) bad = 1;
    __syncthreads();
    if (n == 0 || bad) {
        if (tid == 0) dfs[node] = 0.0, sweeps[node] = 0, status[node] = n == 0 ? LETKF_IDLE : LETKF_NONFINITE;
        return;
    }
    const double rho = 1.0 * 1.0;
    const double kappa = static_cast<double>(M - 1) / rho;
    for (int r = tid; r < M; r += nt) {
        const double f = etkf_f(kappa, etkf_clamp(lam[r]));
        gs[r] = etkf_g(M, f);
        fu[r] = f * etkf_u(M, V, A, r);
    }
    __syncthreads();
    for (int a = tid; a < M; a += nt) wbar[a] = etkf_wbar_entry(M, V, fu, a);
    if (tid == 0) {
        dfs[node] = etkf_dfs(M, lam, kappa);
        sweeps[node] = info[2 * node];
        status[node] = info[2 * node + 1] == EIGEN_NOT_CONVERGED ? LETKF_NOT_CONVERGED : LETKF_OK;
    }
    for (int e = tid; e < M * M; e += nt) {
        const int a = e / M, b = e - a * M;
        if (b < a) continue;
        W[static_cast<size_t>(a) * M + b] = W[static_cast<size_t>(b) * M + a] = etkf_w_entry(M, V, gs, a, b);
    }
}

}  // namespace

hipError_t ens_launch_sym_eigen(int n, int batch, const double* A, int lda, long a_stride, double* work,
                                double* lambda, double* V, int* info, int form, hipStream_t st) {
    form = eigen_device_form(n, form);
    if (!form || batch < 1 || batch > 65535 || lda < n) return hipErrorInvalidValue;
    EigenArgs g{};
    g.n = n, g.lda = lda, g.a_stride = a_stride;
    g.A = A, g.work = work, g.lambda = lambda, g.V = V, g.info = info;
    if (form == EIGEN_FORM_LDS) return launch_eigen<EIGEN_FORM_LDS>(g, batch, st);
    if (form == EIGEN_FORM_MIXED) return launch_eigen<EIGEN_FORM_MIXED>(g, batch, st);
    return launch_eigen<EIGEN_FORM_GLOBAL>(g, batch, st);
}

hipError_t ens_launch_etkf_weights(int M, const double* A, const double* lambda, const double* V, const int* info,
                                   double inflation, double* W, double* wbar, EtkfRecord* rec, double* gamma,
                                   hipStream_t st) {
    if (M < 2 || M > ESPACE_MAX_MEMBERS) return hipErrorInvalidValue;
    const long pairs = static_cast<long>(M) * M;
    const int blocks = static_cast<int>(std::min<long>((pairs + WEIGHTS_THREADS - 1) / WEIGHTS_THREADS, 256));
    hipLaunchKernelGGL(k_etkf_weights, dim3(blocks), dim3(WEIGHTS_THREADS), 0, st, M, A, lambda, V, info, inflation, W,
                       wbar, rec, gamma);
    return hipGetLastError();
}

hipError_t ens_launch_letkf_weights(int M, int nodes, const double* A, const double* lambda, const double* V,
                                    const int* info, const int* count, double* W, double* wbar, double* dfs, int* sweeps,
                                    int* status, hipStream_t st) {
    if (M < 2 || M > ESPACE_MAX_MEMBERS || nodes < 1 || nodes > LETKF_MAX_NODES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_letkf_weights, dim3(nodes), dim3(WEIGHTS_THREADS), 0, st, M, A, lambda, V, info, count, W, wbar,
                       dfs, sweeps, status);
    return hipGetLastError();
}

}  // namespace csim
