// Closed-form expected utilities shared by the expected-utility kernel (eu.hip) and the knowledge-gradient kernels (kg.hip): one
// definition, so both evaluate psi and its partials with the same operations in the same order.
#pragma once
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"

// psi(theta, mu, var) and its partial derivatives in mu (A) and in var (B) for the device utilities that have a closed-form
// expectation under independent Gaussian outputs (the psi / psi_gradient of test_1a.py:101-112, test_2a.py:70-83, test_5a.py:64-77)
__device__ __forceinline__ double eu_closed(int kind, const double* __restrict__ theta, const double (&mu)[BOCF_MAX_M],
                                            const double (&s2)[BOCF_MAX_M], int m, double (&A)[BOCF_MAX_M], double (&B)[BOCF_MAX_M]) {
  if (kind == BOCF_UTIL_NEG_SQ_DIST) {            // -||mu - theta||^2 - sum var
    double sq = 0.0, sv = 0.0;
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < m) {
        const double t = mu[j] - theta[j];
        sq += t * t;
        sv += s2[j];
        A[j] = -2.0 * t;
        B[j] = -1.0;
      }
    return -sq - sv;
  }
  if (kind == BOCF_UTIL_NEG_SUM_EXP) {            // -sum exp(mu + var / 2)
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < m) {
        const double e = exp(mu[j] + 0.5 * s2[j]);
        v -= e;
        A[j] = -e;
        B[j] = -0.5 * e;
      }
    return v;
  }
  // BOCF_UTIL_ROSENBROCK: -sum_{j<h} (a - mu_j)^2 + 100 mu_{j+h}^2 + var_j + 100 var_{j+h}, h = m / 2
  const int h = m >> 1;
  const double a = theta[0];
  double v = 0.0;
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M / 2; ++j)
    if (j < h) {
      const double t = a - mu[j];
      v -= t * t + 100.0 * (mu[j + h] * mu[j + h]) + s2[j] + 100.0 * s2[j + h];
      A[j] = 2.0 * t;
      A[j + h] = -200.0 * mu[j + h];
      B[j] = -1.0;
      B[j + h] = -100.0;
    }
  return v;
}
