// sym_eigen.hpp — the symmetric eigensolver of csim_sym_eigen (include/csim.h): cyclic Jacobi, plain host code without
// the HIP headers, compiled without FMA contraction so that every caller gets the same bits.
#pragma once

namespace csim {

constexpr int SYM_EIGEN_MAX_N = 256;      // CSIM_SYM_EIGEN_MAX_N
constexpr int SYM_EIGEN_MAX_SWEEPS = 64;  // CSIM_SYM_EIGEN_MAX_SWEEPS

// A: n x n row-major, its upper triangle is read.  lambda: n eigenvalues, descending (ties: the lower original index
// first).  V: n x n row-major, column r the unit vector of lambda[r], its first component of largest magnitude
// positive.  *sweeps (may be null): sweeps made.  false: n out of range or a non-finite entry; nothing is written.
bool sym_eigen(int n, const double* A, double* lambda, double* V, int* sweeps);

}  // namespace csim
