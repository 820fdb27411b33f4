// The covariance families, stated once.  Every kernel that evaluates k(x, y) or one of its derivatives takes the arithmetic from here, so
// that the K build, the refinement residual, the small and the tile predict path and the fused and the replicated inference perform the
// same operations on the same operands.  gfx950 only.
//
// With r2 = sum_q ((x_q - y_q) / l_q)^2, r = sqrt(r2), s2 = variance:
//   family 0 (kernel ids 0 RBF and 1 SE)  k = s2 e^{-r2/2}                           GPy/kern/src/rbf.py:42-43, se.py:57-60
//   family 2 (Matern52)                   k = s2 (1 + sqrt5 r + 5/3 r2) e^{-sqrt5 r}  stationary.py:529-530
//   family 3 (Matern32)                   k = s2 (1 + sqrt3 r) e^{-sqrt3 r}           stationary.py:440-441
// and f(r) = -(1/r) dk/dr = -invdist * dK_dr (stationary.py:312-331, se.py:135-148):
//   family 0  k(r);   family 2  (5/3) s2 (1 + sqrt5 r) e^{-sqrt5 r};   family 3  3 s2 e^{-sqrt3 r}.
// f is what the derivatives share:
//   dk(x, y)/dx_q = -f(r) (x_q - y_q) / l_q^2        input gradients of the posterior (gp.py:438-490) and of the look-ahead covariance
//   dk/dl_q       =  f(r) (x_q - y_q)^2 / l_q^3      hyper-gradients (stationary.py:203-212,236-237, se.py:183)
//
// Both are an amplitude times the same exponential, k = A_k e^{-u} and f = A_f e^{-u}, and the pieces below are u, A_k and A_f, keyed by
// the compile-time family FAM in {0, 2, 3}.  A caller that needs both k and f, or keeps the exponential for later, takes
// u = kern_decay<FAM>(r2) and e = bocf_exp_nonpos(-u) once and multiplies the amplitudes by e itself; everybody else calls the two
// wrappers at the end, which take the runtime (or template-constant) kernel id.  The wrappers hand the amplitude to the exponential's
// final ldexp (bocf_exp_nonpos_times): the same bits as A * e wherever e is a normal number (u < 708.39), and one rounding instead of an
// amplified one where e is subnormal -- the K builds hold |K - K_true| <= one subnormal ulp there (tests/test_gpu_extremes.py).  A caller
// that keeps e sums its products, and a term of 1e-317 with 367 or 9e4 ulps of error leaves no trace in a sum.
#pragma once
#include "bocf_internal.h"

#define KERN_SQRT5 2.23606797749978969641
#define KERN_SQRT3 1.73205080756887729353

// family 0 needs nothing but e: a caller that kept e may skip r2 (the amplitudes then ignore r2 and u)
template <int FAM>
constexpr bool kern_uses_r = FAM != 0;

// u: the argument of the exponential is -u = -r2/2, -sqrt5 r, -sqrt3 r.  (The pieces share u and not -u: the Matern polynomials are
// written in +sqrt5 r / +sqrt3 r, and the negation is free where the exponential's first instruction takes it.)
template <int FAM>
__device__ __forceinline__ double kern_decay(double r2) {
  static_assert(FAM == 0 || FAM == 2 || FAM == 3, "covariance family");
  if constexpr (FAM == 0) return 0.5 * r2;
  else return (FAM == 2 ? KERN_SQRT5 : KERN_SQRT3) * sqrt(r2);
}

// A_k from u = kern_decay<FAM>(r2):  k = kern_value_amp * e^{-u}
template <int FAM>
__device__ __forceinline__ double kern_value_amp(double variance, double r2, double u) {
  if constexpr (FAM == 0) return variance;
  else if constexpr (FAM == 2) return variance * (1.0 + u + (5.0 / 3.0) * r2);
  else return variance * (1.0 + u);
}

// A_f from the same u:  f = kern_f_amp * e^{-u}
template <int FAM>
__device__ __forceinline__ double kern_f_amp(double variance, double u) {
  if constexpr (FAM == 0) return variance;
  else if constexpr (FAM == 2) return (5.0 / 3.0) * variance * (1.0 + u);
  else return 3.0 * variance;
}

template <int FAM>
__device__ __forceinline__ double kern_of_r2_family(double variance, double r2) {
  const double u = kern_decay<FAM>(r2);
  return bocf_exp_nonpos_times(-u, kern_value_amp<FAM>(variance, r2, u));      // (A_k e^{-u}, rounded once where e^{-u} is subnormal)
}
template <int FAM>
__device__ __forceinline__ double kern_dfac_family(double variance, double r2) {
  const double u = kern_decay<FAM>(r2);
  return bocf_exp_nonpos_times(-u, kern_f_amp<FAM>(-variance, u));   // (-f: A_f is linear in the variance, the sign rides on it -- exact)
}

// k(r) and -f(r) by kernel id (ids 0 and 1 are family 0): a template constant in the family-templated kernels, the launch's runtime id in
// grad_kernel<D>, cov_grad_kernel<D> and cov_column_kernel
__device__ __forceinline__ double kern_of_r2(int kernel_id, double variance, double r2) {
  if (kernel_id <= 1) return kern_of_r2_family<0>(variance, r2);
  if (kernel_id == 2) return kern_of_r2_family<2>(variance, r2);
  return kern_of_r2_family<3>(variance, r2);
}
__device__ __forceinline__ double kern_dfac(int kernel_id, double variance, double r2) {
  if (kernel_id <= 1) return kern_dfac_family<0>(variance, r2);
  if (kernel_id == 2) return kern_dfac_family<2>(variance, r2);
  return kern_dfac_family<3>(variance, r2);
}
