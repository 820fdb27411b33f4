// Posterior expected utility of the recommendation step (cbo.py:121-235, CBO._current_marginal_argmax): value and input gradient of
//   v_c = scale * sum_h E_h[ U(theta_{p[c]}, f(x_c)) ]
// at every resident candidate c, each with its OWN utility parameter index p[c], so that the L independent argmax problems of one
// _current_max_value advance as one batch.  Three forms, as in the reference:
//   MEAN    theta . mu_h                                 (utility.linear, cbo.py:124-157)
//   CLOSED  psi(theta, mu_h, var_h), psi = E[U] in closed form   (expectation_utility given, cbo.py:159-188)
//   MC      sum_s U(theta, mu_h + sigma_h o Z_s), Z the parameter's own (S, m) normals   (cbo.py:190-231)
// The value is a SUM over samples (and hyper-samples), not a mean: the reference's is "not normalized" (cbo.py:160).
// One wave per candidate; in MC mode the lanes stride the S samples and the partial sums meet in a fixed __shfl_xor butterfly
// (deterministic).  The kernel writes its own outputs only.
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"
#include "utility_dev.h"
#include "eu_dev.h"

// (MC = the output count as a template argument, 1 ... 8, or 0 = read it from the arguments, as in acq_mc_grad_kernel)
template <int MC>
__global__ __launch_bounds__(256) void eu_kernel(EuArgs a) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.C) return;                         // wave-uniform
  const int m_ = MC > 0 ? MC : a.m;
  constexpr int MM = MC > 0 ? MC : BOCF_MAX_M;
  const int p = a.rows[c];
  const double* th = a.theta + (long)p * a.theta_dim;
  const bool grad = a.grad != nullptr;
  double mu[BOCF_MAX_M], s2[BOCF_MAX_M], A[BOCF_MAX_M], B[BOCF_MAX_M];
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    mu[j] = j < m_ ? a.mean[(long)j * a.ld + c] : 0.0;
    s2[j] = (a.mode != BOCF_EU_MEAN && j < m_) ? a.var[(long)j * a.ld + c] : 0.0;
    A[j] = 0.0;
    B[j] = 0.0;
  }
  double v = 0.0;
  if (a.mode == BOCF_EU_MEAN) {
#pragma unroll
    for (int j = 0; j < MM; ++j)
      if (j < m_) {
        v += th[j] * mu[j];
        A[j] = th[j];
      }
  } else if (a.mode == BOCF_EU_CLOSED) {
    v = eu_closed(a.util_kind, th, mu, s2, m_, A, B);
  } else {
    double* sg = s2;                                // sigma in place of the variance (the variance is not needed again)
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) sg[j] = j < m_ ? sqrt(s2[j]) : 1.0;
    const double* Z = a.Zt + (long)p * m_ * a.S;   // (m, S) normals of this candidate's parameter
    double part = 0.0;
    for (int s = lane; s < a.S; s += 64) {
      double y[BOCF_MAX_M], g[BOCF_MAX_M];
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = mu[j] + sg[j] * (j < m_ ? Z[(long)j * a.S + s] : 0.0);
      part += utility_eval(a.util_kind, th, a.util_params, y, m_);
      if (grad) {
        utility_grad(a.util_kind, th, a.util_params, y, m_, g);
#pragma unroll
        for (int j = 0; j < MM; ++j) {
          A[j] += g[j];
          B[j] += j < m_ ? g[j] * Z[(long)j * a.S + s] : 0.0;      // (re-read from the cache: one array less in registers)
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    v = part;
    if (grad) {
#pragma unroll
      for (int j = 0; j < MM; ++j) {
        if (j < m_) {
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            A[j] += __shfl_xor(A[j], o, 64);
            B[j] += __shfl_xor(B[j], o, 64);
          }
          B[j] *= 0.5 / sg[j];                  // d sigma / dx = (d var / dx) / (2 sigma)  (cbo.py:218-219)
        }
      }
    }
  }
  if (lane == 0) a.val[c] = (a.accumulate ? a.val[c] : 0.0) + v * a.scale;
  if (grad && lane < a.d) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < MM; ++j)
      if (j < m_) t += A[j] * a.dmean[((long)j * a.ldg + c) * a.d + lane] + B[j] * a.dvar[((long)j * a.ldg + c) * a.d + lane];
    a.grad[(long)c * a.d + lane] = (a.accumulate ? a.grad[(long)c * a.d + lane] : 0.0) + t * a.scale;
  }
}

void launch_eu(const EuArgs& a, hipStream_t s) {
  if (a.C == 0) return;
  if (a.util_kind == BOCF_UTIL_PROGRAM && a.mode == BOCF_EU_MC) {   // (the mean form ignores the kind; the entry point rejects the closed form)
    launch_eu_prog(a, s);
    return;
  }
  const dim3 grid((unsigned)((a.C + 3) / 4));
  if (a.m >= 1 && a.m <= 8) {
#define LM(M) case M: BOCF_LAUNCH((eu_kernel<M>), grid, dim3(256), 0, s, a); break;
    switch (a.m) { LM(1) LM(2) LM(3) LM(4) LM(5) LM(6) LM(7) LM(8) default: break; }
#undef LM
    return;
  }
  BOCF_LAUNCH((eu_kernel<0>), grid, dim3(256), 0, s, a);
}
