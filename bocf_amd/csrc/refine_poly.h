// The polynomial test objective of the refinement's state machine (quadratic plus cubic with a neighbour coupling; multiplications,
// additions and subtractions only, contraction off as in refine_step.h -- REFINE_FP_STRICT in every body for clang and hipcc, the REFINE_FP_BEGIN / REFINE_FP_END
// brackets for GCC -- so x86 and gfx950 give the same bits).  Shared by
// tests/refine_step_driver.cpp and the probes-build hook bocf_refine_probe_poly (capi_probe.hip):
//   u_k = x_k - c_k,  c_k = 0.25 (k mod 4) - 0.3,  a_k = 1 + 0.5 (k mod 3),  n = (k + 1) mod d
//   f   = sum_k a_k u_k^2 + 0.05 u_k^3 + 0.1 u_k u_n
//   g_k = 2 a_k u_k + 0.15 u_k^2 + 0.1 (u_n + u_p),  p = (k - 1) mod d
#pragma once
#include "refine_step.h"

REFINE_FP_BEGIN

REFINE_HD static inline double refine_poly_u(const double* x, int k) {
  REFINE_FP_STRICT
  return x[k] - (0.25 * (double)(k % 4) - 0.3);
}

REFINE_HD static inline double refine_poly(const double* x, int d, double* g) {
  REFINE_FP_STRICT
  double f = 0.0;
  for (int k = 0; k < d; ++k) {
    const double a = 1.0 + 0.5 * (double)(k % 3);
    const double u = refine_poly_u(x, k), un = refine_poly_u(x, (k + 1) % d), up = refine_poly_u(x, (k + d - 1) % d);
    f += a * u * u + 0.05 * u * u * u + 0.1 * u * un;
    g[k] = 2.0 * a * u + 0.15 * u * u + 0.1 * (un + up);
  }
  return f;
}

REFINE_FP_END
