// sym_eigen.hpp — the symmetric eigensolver of csim_sym_eigen (include/csim.h): cyclic Jacobi, plain host code without
// the HIP headers, compiled without FMA contraction so that every caller gets the same bits.  Two orders of the pairs
// of a sweep: by rows (CSIM_EIGEN_ROWS), and the round robin (CSIM_EIGEN_ROUND_ROBIN) whose steps are disjoint pairs,
// which is the order the device solver (sym_eigen_device.hip) takes.
#pragma once

namespace csim {

constexpr int SYM_EIGEN_MAX_N = 256;      // CSIM_SYM_EIGEN_MAX_N
constexpr int SYM_EIGEN_MAX_SWEEPS = 64;  // CSIM_SYM_EIGEN_MAX_SWEEPS
constexpr int EIGEN_ROWS = 0;             // CSIM_EIGEN_ROWS
constexpr int EIGEN_ROUND_ROBIN = 1;      // CSIM_EIGEN_ROUND_ROBIN

// the status word of the device solver
constexpr int EIGEN_OK = 0, EIGEN_NONFINITE = 1, EIGEN_NOT_CONVERGED = 2;  // CSIM_EIGEN_OK, _NONFINITE, _NOT_CONVERGED

// the storage forms of the device solver and the largest n each admits (csim_sym_eigen_device_form)
constexpr int EIGEN_FORMS = 3;
constexpr int EIGEN_FORM_LDS = 1, EIGEN_FORM_MIXED = 2, EIGEN_FORM_GLOBAL = 3;
constexpr int EIGEN_LDS_MAX_N = 96;     // a and v in LDS: 16 n^2 = 144 KiB
constexpr int EIGEN_MIXED_MAX_N = 128;  // a in LDS, v in global memory: 8 n^2 = 128 KiB
inline int eigen_form_max_n(int form) {
    return form == EIGEN_FORM_LDS ? EIGEN_LDS_MAX_N : form == EIGEN_FORM_MIXED ? EIGEN_MIXED_MAX_N : SYM_EIGEN_MAX_N;
}
// the form the launcher takes for n when `forced` is 0, else `forced`; 0: n or the form out of range, or n above what
// the forced form admits
inline int eigen_device_form(int n, int forced) {
    if (n < 1 || n > SYM_EIGEN_MAX_N || forced < 0 || forced > EIGEN_FORMS) return 0;
    if (forced) return n <= eigen_form_max_n(forced) ? forced : 0;
    return n <= EIGEN_LDS_MAX_N ? EIGEN_FORM_LDS : n <= EIGEN_MIXED_MAX_N ? EIGEN_FORM_MIXED : EIGEN_FORM_GLOBAL;
}

// The round robin: m = n rounded up to even; slot k (0 .. m/2-1) of step t (0 .. m-2) is the pair *p < *q.  A slot
// with *q >= n (odd n: always slot 0) is idle.  Host and device take the pairs from here.
#if defined(__HIP__)
__host__ __device__
#endif
inline void eigen_rr_pair(int m, int t, int k, int* p, int* q) {
    int x, y;
    if (k == 0) {
        x = m - 1, y = t;
    } else {
        x = t + k, y = t - k;
        if (x >= m - 1) x -= m - 1;
        if (y < 0) y += m - 1;
    }
    *p = x < y ? x : y, *q = x < y ? y : x;
}

// A: n x n row-major, its upper triangle is read.  lambda: n eigenvalues, descending (ties: the lower original index
// first).  V: n x n row-major, column r the unit vector of lambda[r], its first component of largest magnitude
// positive.  *sweeps (may be null): sweeps made.  false: n out of range or a non-finite entry; nothing is written.
bool sym_eigen(int n, const double* A, double* lambda, double* V, int* sweeps);
// the same with the pairs of a sweep in the given order (EIGEN_ROWS: sym_eigen's own bits); false also for an unknown
// order
bool sym_eigen_ordered(int n, const double* A, int order, double* lambda, double* V, int* sweeps);

}  // namespace csim
