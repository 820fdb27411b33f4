// The smoothed feasibility phi(y) of the resident output constraints and the wave-uniform move, shared by the constrained acquisition
// kernels (cacq.hip) and the constrained expected-utility kernels (ceu.hip): one definition, so both weigh a sample with the same
// operations in the same order (DESIGN.md sections 17 and 18).
#pragma once
#include "bocf_internal.h"

// phi(y) = prod_k s(-c_k / eta_k), k in index order, with exp of a non-positive argument on both branches:
//   e = exp(-|t|):  s(t) = 1 / (1 + e) for t >= 0, e / (1 + e) for t < 0   (and 1 - s(t) the other one of the two).
// GRAD: q_j = sum_k (1 - s_k) A_kj / eta_k, so that d phi / d y_j = -phi q_j.
template <int MC, bool GRAD>
__device__ __forceinline__ double cacq_phi(const double* __restrict__ tab, int K, int m_, const double (&y)[BOCF_MAX_M], double (&q)[BOCF_MAX_M]) {
  constexpr int MM = MC > 0 ? MC : BOCF_MAX_M;
  const double* __restrict__ b = tab + K * m_;
  const double* __restrict__ ie = b + K;
  double phi = 1.0;
  if (GRAD) {
#pragma unroll
    for (int j = 0; j < MM; ++j) q[j] = 0.0;
  }
  for (int k = 0; k < K; ++k) {
    const double* __restrict__ Ak = tab + k * m_;
    double c = 0.0;
#pragma unroll
    for (int j = 0; j < MM; ++j)
      if (MC > 0 || j < m_) c += Ak[j] * y[j];
    c -= b[k];
    const double t = -c * ie[k];
    const double e = bocf_exp_nonpos(-fabs(t));
    const double hi = 1.0 / (1.0 + e), lo = e * hi;
    phi *= t >= 0.0 ? hi : lo;
    if (GRAD) {
      const double u = (t >= 0.0 ? lo : hi) * ie[k];
#pragma unroll
      for (int j = 0; j < MM; ++j)
        if (MC > 0 || j < m_) q[j] += u * Ak[j];
    }
  }
  return phi;
}

// A value that is the same in every lane of the wave, moved to scalar registers: the candidate's mean and sigma stay out of the vector file
__device__ __forceinline__ double wave_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
