// U(theta, y) and dU/dy of the device utilities, shared by the acquisition kernels (acq.hip) and the expected-utility kernel
// (eu.hip): one definition, so both evaluate the utilities with the same operations in the same order.
#pragma once
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"

#define PI_D 3.14159265358979323846

// U(theta, y): the utilities of the reference's experiment scripts (see include/bocf_hip.h)
__device__ __forceinline__ double utility_eval(int kind, const double* __restrict__ theta, const double* __restrict__ params,
                                               const double (&y)[BOCF_MAX_M], int m) {
  double acc = 0.0;
  if (kind == BOCF_UTIL_LINEAR) {
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < m) acc += theta[j] * y[j];
    return acc;
  }
  if (kind == BOCF_UTIL_NEG_SQ_DIST) {
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < m) {
        const double t = y[j] - theta[j];
        acc += t * t;
      }
    return -acc;
  }
  if (kind == BOCF_UTIL_NEG_SUM_EXP) {
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < m) acc += -exp(y[j]);
    return acc;
  }
  if (kind == BOCF_UTIL_NEG_EXP_COS) {
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < m) acc += params[j] * (exp(-y[j] / PI_D) * cos(PI_D * y[j]));
    return -acc;
  }
  // BOCF_UTIL_ROSENBROCK: val -= (a - y_j)^2 + 100 y_{j+h}^2, h = m/2 (test_5a.py:48-52)
  const int h = m >> 1;
  const double a = theta[0];
  double val = 0.0;
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M / 2; ++j)
    if (j < h) {
      const double t = a - y[j];
      val -= t * t + 100.0 * (y[j + h] * y[j + h]);
    }
  return val;
}

// dU/dy: the analytic derivatives the experiment scripts pass as dfunc (test_1a.py:94-96,
// test_2a.py:64-65, test_3a.py:60-66, test_5a.py:54-59; linear: theta)
__device__ __forceinline__ void utility_grad(int kind, const double* __restrict__ theta, const double* __restrict__ params,
                                             const double (&y)[BOCF_MAX_M], int m, double (&g)[BOCF_MAX_M]) {
  const int h = m >> 1;
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    double v = 0.0;
    if (j < m) {
      if (kind == BOCF_UTIL_LINEAR) v = theta[j];
      else if (kind == BOCF_UTIL_NEG_SQ_DIST) v = -2.0 * (y[j] - theta[j]);
      else if (kind == BOCF_UTIL_NEG_SUM_EXP) v = -exp(y[j]);
      else if (kind == BOCF_UTIL_NEG_EXP_COS) {
        const double e = exp(-y[j] / PI_D);
        v = params[j] * (PI_D * e * sin(PI_D * y[j]) + e * cos(PI_D * y[j]) / PI_D);
      } else {
        v = j < h ? 2.0 * (theta[0] - y[j]) : (j < 2 * h ? -200.0 * y[j] : 0.0);
      }
    }
    g[j] = v;
  }
}
