// The q x q Cholesky factor of the joint q-point acquisition (joint.hip) and its reverse pass, q <= 8: one definition for the device kernels
// and for the host driver of the CPU suite (tests/joint_chol_driver.cpp), as refine_step.h and pending_host.h are shared.  No HIP include.
//
// Row-wise (Cholesky-Banachiewicz) with a pivot floor: for k = 0 .. q - 1
//   C[k][i] = (A[k][i] - sum_{t < i} C[k][t] C[i][t]) / C[i][i],  i = 0 .. k - 1        (the lower triangle of A is read)
//   p_k     = A[k][k] + tau - sum_{i < k} C[k][i]^2;   where !(p_k > 1e-10): p_k := 1e-10 and pivot k is marked floored
//   C[k][k] = sqrt(p_k)
// No matrix can fail.  A floored pivot is a constant: the reverse pass drops its adjoint.  tau is a constant too.
// Every sum runs in increasing index order with fused multiply-adds, the same on both sides.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JOINT_HD __host__ __device__
#else
#define JOINT_HD
#endif

#define JOINT_MAX_Q 8
#define JOINT_PIVOT_FLOOR 1e-10

// tau = 1e-8 max(mean diag A, 1e-10): rung 0 of the jitter ladder of the pending points (pending_host.h), the only rung here
JOINT_HD inline double joint_chol_tau(const double* A, int q, int lda) {
  double t = 0.0;
  for (int k = 0; k < q; ++k) t += A[k * lda + k];
  t /= q;
  return 1e-8 * (t > 1e-10 ? t : 1e-10);
}

// A (q rows of lda, lower triangle read) + tau I -> C (q rows of ldc, lower triangle written, the rest untouched).  Returns the mask of the
// floored pivots (bit k = pivot k).
JOINT_HD inline unsigned joint_chol_floor(const double* A, int lda, int q, double tau, double* C, int ldc) {
  unsigned floored = 0u;
  for (int k = 0; k < q; ++k) {
    double p = A[k * lda + k] + tau;
    for (int i = 0; i < k; ++i) {
      double n = A[k * lda + i];
      for (int t = 0; t < i; ++t) n = fma(-C[k * ldc + t], C[i * ldc + t], n);
      const double c = n / C[i * ldc + i];
      C[k * ldc + i] = c;
      p = fma(-c, c, p);
    }
    if (!(p > JOINT_PIVOT_FLOOR)) {
      p = JOINT_PIVOT_FLOOR;
      floored |= 1u << k;
    }
    C[k * ldc + k] = sqrt(p);
  }
  return floored;
}

// Reverse pass, in place: G holds d alpha / dC (lower triangle, rows of ldg) on entry and d alpha / dA of the lower-triangle entries the
// factorization read on exit (one entry per pair: the symmetric convention d alpha = sum_ab Abar_ab dA_ab has Abar_aa = G[a][a] and
// Abar_ab = Abar_ba = G[max][min] / 2).  Rows k = q - 1 .. 0: the pivot's adjoint first, then the off-diagonal numerators i = k - 1 .. 0.
JOINT_HD inline void joint_chol_adjoint(const double* C, int ldc, int q, unsigned floored, double* G, int ldg) {
  for (int k = q - 1; k >= 0; --k) {
    double pb = 0.0;
    if (!((floored >> k) & 1u)) pb = G[k * ldg + k] / (2.0 * C[k * ldc + k]);
    G[k * ldg + k] = pb;
    for (int i = 0; i < k; ++i) G[k * ldg + i] = fma(-2.0 * pb, C[k * ldc + i], G[k * ldg + i]);
    for (int i = k - 1; i >= 0; --i) {
      const double nb = G[k * ldg + i] / C[i * ldc + i];
      G[i * ldg + i] = fma(-nb, C[k * ldc + i], G[i * ldg + i]);
      for (int t = 0; t < i; ++t) {
        G[k * ldg + t] = fma(-nb, C[i * ldc + t], G[k * ldg + t]);
        G[i * ldg + t] = fma(-nb, C[k * ldc + t], G[i * ldg + t]);
      }
      G[k * ldg + i] = nb;
    }
  }
}
