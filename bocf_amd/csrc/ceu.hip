// Constrained expected utility of the recommendation step: the Monte-Carlo form of eu_kernel (eu.hip) with every
// sample weighed by the smoothed feasibility phi of the resident output constraints (cacq_dev.h), an infeasible outcome worth u0:
//   y_s = mu + sigma o Z_s,  T_s = phi(y_s) (U(theta, y_s) - u0),  G = scale sum_h sum_s [u0 + T_s],  P = (1 / (n_h S)) sum_h sum_s phi(y_s)
//   dT/dy_j = phi (dU/dy_j - (U - u0) q_j),  A_j = sum_s dT/dy_j,  B_j = sum_s dT/dy_j Z_sj / (2 sigma_j),
//   dG/dx_q = scale sum_h sum_j A_j dmu_j/dx_q + B_j dsigma^2_j/dx_q
// Geometry of eu_kernel: one wave per candidate, four per workgroup, lanes stride the S samples, a fixed __shfl_xor butterfly, no atomics --
// a candidate's bits do not depend on its batch.  Every row has its own parameter index p[c]: theta, u0 and the Z block are that
// parameter's.  y_s is formed once per sample and serves phi, q and U.  The table A | b | 1 / eta is read at wave-uniform addresses.
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"
#include "utility_dev.h"
#include "cacq_dev.h"

// (MC = the output count as a template argument, 1 ... 8, or 0 = read it from the arguments, m <= 16)
template <int MC, bool GRAD>
__global__ __launch_bounds__(256) void ceu_kernel(CeuArgs a) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (c >= a.C) return;                         // wave-uniform
  const int m_ = MC > 0 ? MC : a.m;
  constexpr int MM = MC > 0 ? MC : BOCF_MAX_M;
  constexpr int MG = GRAD ? MM : 1;
  const int p = __builtin_amdgcn_readfirstlane(a.rows[c]);
  const double* __restrict__ th = a.theta + (long)p * a.theta_dim;
  const double* __restrict__ Z = a.Zt + (long)p * m_ * a.S;   // (m, S) normals of this candidate's parameter
  const double u0 = a.u0[p];
  double mu[MM], sg[MM], Aj[MG], Bj[MG];
#pragma unroll
  for (int j = 0; j < MM; ++j) {
    const bool on = MC > 0 || j < m_;
    mu[j] = on ? a.mean[(long)j * a.ld + c] : 0.0;
    sg[j] = on ? wave_uniform(sqrt(a.var[(long)j * a.ld + c])) : (GRAD ? 1.0 : 0.0);
  }
#pragma unroll
  for (int j = 0; j < MG; ++j) Aj[j] = Bj[j] = 0.0;
  double part = 0.0, pphi = 0.0;
  for (int s = lane; s < a.S; s += 64) {
    double y[BOCF_MAX_M], q[BOCF_MAX_M], g[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = 0.0;
#pragma unroll
    for (int j = 0; j < MM; ++j)
      if (MC > 0 || j < m_) y[j] = mu[j] + sg[j] * Z[(long)j * a.S + s];
    const double t = utility_eval(a.util_kind, th, a.util_params, y, m_) - u0;
    if (GRAD) utility_grad(a.util_kind, th, a.util_params, y, m_, g);
    const double phi = cacq_phi<MC, GRAD>(a.tab, a.K, m_, y, q);   // (after the utility: q is not live across it)
    part += u0 + phi * t;
    pphi += phi;
    if (GRAD) {
#pragma unroll
      for (int j = 0; j < MM; ++j)
        if (MC > 0 || j < m_) {
          const double dT = phi * (g[j] - t * q[j]);
          Aj[j] += dT;
          Bj[j] += dT * (0.5 * Z[(long)j * a.S + s] / sg[j]);       // (the normal is read again: a cache hit, one register pair less)
        }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    part += __shfl_xor(part, o, 64);
    pphi += __shfl_xor(pphi, o, 64);
  }
  if (lane == 0) {
    a.val[c] = (a.accumulate ? a.val[c] : 0.0) + part * a.scale;
    a.pof[c] = (a.accumulate ? a.pof[c] : 0.0) + pphi * a.pscale;
  }
  if (GRAD) {
    double tq = 0.0;
#pragma unroll
    for (int j = 0; j < MM; ++j)
      if (MC > 0 || j < m_) {
        double As = Aj[j], Bs = Bj[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          As += __shfl_xor(As, o, 64);
          Bs += __shfl_xor(Bs, o, 64);
        }
        if (lane < a.d) tq += As * a.dmean[((long)j * a.ldg + c) * a.d + lane] + Bs * a.dvar[((long)j * a.ldg + c) * a.d + lane];
      }
    if (lane < a.d) a.grad[(long)c * a.d + lane] = (a.accumulate ? a.grad[(long)c * a.d + lane] : 0.0) + tq * a.scale;
  }
}

// feasible_best_kernel (cacq.hip) without the feasibility test: one workgroup per parameter l, the range of U(theta_l, mu(X_i)) over all
// i < N, LDS reduction in a fixed order
__global__ __launch_bounds__(256) void train_utility_range_kernel(const double* __restrict__ mu_train, int N, int m, int util_kind,
                                                                  const double* __restrict__ theta, int theta_dim, const double* __restrict__ params,
                                                                  double* __restrict__ mn_out, double* __restrict__ mx_out) {
  const int l = blockIdx.x;
  const double* th = theta + (long)l * theta_dim;
  double mx = -INFINITY, mn = INFINITY;
  for (int i = threadIdx.x; i < N; i += 256) {
    double y[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = j < m ? mu_train[(long)j * N + i] : 0.0;
    const double u = utility_eval(util_kind, th, params, y, m);
    mx = fmax(mx, u);
    mn = fmin(mn, u);
  }
  __shared__ double rmx[256], rmn[256];
  rmx[threadIdx.x] = mx;
  rmn[threadIdx.x] = mn;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      rmx[threadIdx.x] = fmax(rmx[threadIdx.x], rmx[threadIdx.x + o]);
      rmn[threadIdx.x] = fmin(rmn[threadIdx.x], rmn[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    mx_out[l] = rmx[0];
    mn_out[l] = rmn[0];
  }
}

void launch_train_utility_range(const double* mu_train, int N, int m, int util_kind, const double* theta, int theta_dim, int L, const double* util_params,
                                double* min_out, double* max_out, hipStream_t s) {
  BOCF_LAUNCH(train_utility_range_kernel, dim3((unsigned)L), dim3(256), 0, s, mu_train, N, m, util_kind, theta, theta_dim, util_params, min_out, max_out);
}

void launch_ceu(const CeuArgs& a, bool grad, hipStream_t s) {
  if (a.C == 0) return;
  const dim3 grid((unsigned)((a.C + 3) / 4));
#define LM(M)                                                                              \
  case M:                                                                                  \
    if (grad) BOCF_LAUNCH((ceu_kernel<M, true>), grid, dim3(256), 0, s, a);                \
    else BOCF_LAUNCH((ceu_kernel<M, false>), grid, dim3(256), 0, s, a);                    \
    break;
  switch (a.m >= 1 && a.m <= 8 ? a.m : 0) {
    LM(1) LM(2) LM(3) LM(4) LM(5) LM(6) LM(7) LM(8) default: LM(0)
  }
#undef LM
}
