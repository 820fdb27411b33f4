// Constrained Monte-Carlo expected improvement of a composite utility: K <= 8 linear constraints on the outputs,
//   c_k(y) = sum_j A_kj y_j - b_k <= 0,
// weigh every sample of the Monte-Carlo sum by the smoothed feasibility phi(y) = prod_k s(-c_k(y) / eta_k), s the logistic function:
//   alpha(x) = sum_l p_l (1/S) sum_s I_ls phi(y_s),   y_s = mu + sigma o W_s,
//   I_ls = max(U(theta_l, y_s) - best_l, 0) with best_l over the FEASIBLE training points, or 1 when there is none.
// Geometry of acq_mc_m_kernel (acq.hip): one wave per candidate, four per workgroup, lanes stride the S samples, a fixed __shfl_xor
// butterfly, no atomics -- a candidate's bits do not depend on its batch.  y_s is formed once per sample and serves the constraints and
// all L parameters (l in index order).  The table A | b | 1 / eta (at most 152 doubles) is read from memory at wave-uniform addresses,
// i.e. through the scalar cache; it is not staged in LDS.
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"
#include "utility_dev.h"
#include "cacq_dev.h"   // cacq_phi, wave_uniform

// (MC = the output count as a template argument, 1 ... 8, or 0 = read it from the arguments, m <= 16)
template <int MC>
__global__ __launch_bounds__(256) void cacq_kernel(CacqArgs a) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (c >= a.C) return;                         // wave-uniform
  const int m_ = MC > 0 ? MC : a.m;
  constexpr int MM = MC > 0 ? MC : BOCF_MAX_M;
  double mu[MM], sg[MM];
#pragma unroll
  for (int j = 0; j < MM; ++j) {
    const bool on = MC > 0 || j < m_;
    mu[j] = on ? a.mean[(long)j * a.ld + c] : 0.0;
    sg[j] = on ? wave_uniform(sqrt(a.var[(long)j * a.ld + c])) : 0.0;
  }
  const bool incumbent = a.nfeas[0] > 0;
  double psum = 0.0;
  for (int l = 0; l < a.L; ++l) psum += a.prob[l];
  double part = 0.0;
  for (int s = lane; s < a.S; s += 64) {
    double y[BOCF_MAX_M], q[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = 0.0;
#pragma unroll
    for (int j = 0; j < MM; ++j)
      if (MC > 0 || j < m_) y[j] = mu[j] + sg[j] * a.Wt[(long)j * a.S + s];
    const double phi = cacq_phi<MC, false>(a.tab, a.K, m_, y, q);
    double t = psum;
    if (incumbent) {
      t = 0.0;
      for (int l = 0; l < a.L; ++l) {
        const double v = utility_eval(a.util_kind, a.theta + (long)l * a.theta_dim, a.util_params, y, m_);
        t += a.prob[l] * fmax(v - a.best[l], 0.0);
      }
    }
    part += t * phi;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) a.acq[c] = (a.accumulate ? a.acq[c] : 0.0) + (part / (double)a.S) * a.scale;
}

// Value and input gradient.  With T = (sum_l p_l I_ls) phi:
//   dT/dy_j = phi (sum_l p_l 1[U_l > best_l] dU_l/dy_j  -  (sum_l p_l I_ls) q_j),
//   A_j = sum_s dT/dy_j,  B_j = sum_s dT/dy_j W_sj / (2 sigma_j),  d alpha / dx_q = (1/S) sum_j A_j dmu_j/dx_q + B_j dsigma^2_j/dx_q
// -- the same traversal as the value kernel, the assembly of acq_mc_grad_kernel (lane q < d owns d alpha / dx_q).
template <int MC>
__global__ __launch_bounds__(256) void cacq_grad_kernel(CacqArgs a) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (c >= a.C) return;
  const int m_ = MC > 0 ? MC : a.m;
  constexpr int MM = MC > 0 ? MC : BOCF_MAX_M;
  double mu[MM], sg[MM], Aj[MM], Bj[MM];
#pragma unroll
  for (int j = 0; j < MM; ++j) {
    const bool on = MC > 0 || j < m_;
    mu[j] = on ? a.mean[(long)j * a.ld + c] : 0.0;
    sg[j] = on ? wave_uniform(sqrt(a.var[(long)j * a.ld + c])) : 1.0;
    Aj[j] = 0.0;
    Bj[j] = 0.0;
  }
  const bool incumbent = a.nfeas[0] > 0;
  double psum = 0.0;
  for (int l = 0; l < a.L; ++l) psum += a.prob[l];
  double part = 0.0;
  for (int s = lane; s < a.S; s += 64) {
    double y[BOCF_MAX_M], q[BOCF_MAX_M], u[MM];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = 0.0;
#pragma unroll
    for (int j = 0; j < MM; ++j) {
      u[j] = 0.0;
      if (MC > 0 || j < m_) y[j] = mu[j] + sg[j] * a.Wt[(long)j * a.S + s];
    }
    double t = psum;
    if (incumbent) {
      t = 0.0;
      for (int l = 0; l < a.L; ++l) {
        const double* th = a.theta + (long)l * a.theta_dim;
        const double v = utility_eval(a.util_kind, th, a.util_params, y, m_);
        const double best = a.best[l], p = a.prob[l];
        t += p * fmax(v - best, 0.0);
        if (v > best) {
          double g[BOCF_MAX_M];
          utility_grad(a.util_kind, th, a.util_params, y, m_, g);
#pragma unroll
          for (int j = 0; j < MM; ++j) u[j] += p * g[j];
        }
      }
    }
    const double phi = cacq_phi<MC, true>(a.tab, a.K, m_, y, q);   // (after the utilities: q is not live across them)
    part += t * phi;
#pragma unroll
    for (int j = 0; j < MM; ++j)
      if (MC > 0 || j < m_) {
        const double dT = phi * (u[j] - t * q[j]);
        Aj[j] += dT;
        Bj[j] += dT * (0.5 * a.Wt[(long)j * a.S + s] / sg[j]);       // (the normal is read again: a cache hit, one register pair less)
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (lane == 0) a.acq[c] = (a.accumulate ? a.acq[c] : 0.0) + (part / (double)a.S) * a.scale;
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
  if (lane < a.d) {
    a.dacq[(long)c * a.d + lane] = (a.accumulate ? a.dacq[(long)c * a.d + lane] : 0.0) + (tq / (double)a.S) * a.scale;
  }
}

// best_so_far_kernel (acq.hip) over the training points that pass the HARD test c_k(mu(X_i)) <= 0 for every k: one workgroup per
// parameter l; best[l] = -inf when no point passes; workgroup 0 also writes the number of points that pass.
__global__ __launch_bounds__(256) void feasible_best_kernel(const double* __restrict__ mu_train, int N, int m, int util_kind,
                                                            const double* __restrict__ theta, int theta_dim, const double* __restrict__ params,
                                                            const double* __restrict__ tab, int K, double* __restrict__ best,
                                                            long long* __restrict__ nfeas) {
  const int l = blockIdx.x;
  const double* th = theta + (long)l * theta_dim;
  const double* b = tab + K * m;
  double mx = -INFINITY;
  int cnt = 0;
  for (int i = threadIdx.x; i < N; i += 256) {
    double y[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = j < m ? mu_train[(long)j * N + i] : 0.0;
    bool ok = true;
    for (int k = 0; k < K; ++k) {
      double c = 0.0;
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j)
        if (j < m) c += tab[k * m + j] * y[j];
      ok = ok && (c - b[k] <= 0.0);
    }
    if (ok) {
      ++cnt;
      mx = fmax(mx, utility_eval(util_kind, th, params, y, m));
    }
  }
  __shared__ double red[256];
  __shared__ int redn[256];
  red[threadIdx.x] = mx;
  redn[threadIdx.x] = cnt;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
      redn[threadIdx.x] += redn[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    best[l] = red[0];
    if (l == 0) nfeas[0] = redn[0];
  }
}

void launch_feasible_best(const double* mu_train, int N, int m, int util_kind, const double* theta, int theta_dim, int L, const double* util_params,
                          const double* tab, int K, double* best, long long* nfeas, hipStream_t s) {
  BOCF_LAUNCH(feasible_best_kernel, dim3((unsigned)L), dim3(256), 0, s, mu_train, N, m, util_kind, theta, theta_dim, util_params, tab, K, best, nfeas);
}

void launch_cacq(const CacqArgs& a, hipStream_t s) {
  if (a.C == 0) return;
  const dim3 grid((unsigned)((a.C + 3) / 4));
  switch (a.m >= 1 && a.m <= 8 ? a.m : 0) {
#define LM(M) case M: BOCF_LAUNCH((cacq_kernel<M>), grid, dim3(256), 0, s, a); break;
    LM(1) LM(2) LM(3) LM(4) LM(5) LM(6) LM(7) LM(8) default: LM(0)
#undef LM
  }
}

void launch_cacq_grad(const CacqArgs& a, hipStream_t s) {
  if (a.C == 0) return;
  const dim3 grid((unsigned)((a.C + 3) / 4));
  switch (a.m >= 1 && a.m <= 8 ? a.m : 0) {
#define LM(M) case M: BOCF_LAUNCH((cacq_grad_kernel<M>), grid, dim3(256), 0, s, a); break;
    LM(1) LM(2) LM(3) LM(4) LM(5) LM(6) LM(7) LM(8) default: LM(0)
#undef LM
  }
}
