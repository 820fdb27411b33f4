// f(r) of dk(x, y)/dx_q = f(r) (x_q - y_q) / l_q^2 for the covariance families, shared by the posterior gradients (predict.hip grad_kernel)
// and the covariance gradient of the look-ahead posterior (kg.hip cov_grad_kernel): one statement of every family's derivative.
#pragma once
#include "bocf_internal.h"

__device__ __forceinline__ double kern_dfac(int kernel_id, double variance, double r2) {
  if (kernel_id <= 1) return -variance * bocf_exp_nonpos(-0.5 * r2);
  const double r = sqrt(r2);
  if (kernel_id == 2) {
    const double s5r = 2.23606797749978969641 * r;
    return -(5.0 / 3.0) * variance * (1.0 + s5r) * bocf_exp_nonpos(-s5r);
  }
  return -3.0 * variance * bocf_exp_nonpos(-1.73205080756887729353 * r);
}
