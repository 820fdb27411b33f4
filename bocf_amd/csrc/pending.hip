// Monte-Carlo expected improvement of the composite utility at x, conditioned on r <= 15 pending points P (capi_pending.hip drives it).
// Per output j, with mu_j, sigma^2_j the posterior mean and the raw noiseless variance, Sigma_j(a, b) = k_j(a, b) - V_a^T V_b,
// Sigma~_j = Sigma_j(P, P) + tau_j I = L_j L_j^T, Q_j = Sigma~_j^-1 and the host-made joint samples F_sj = mu_j(P) + L_j z_sj, G_sj = L_j^-T z_sj:
//   c_j(x) = Sigma_j(P, x),  v_j(x) = max(sigma^2_j(x) - c_j^T Q_j c_j, 1e-10)
//   y_sj(x) = mu_j(x) + c_j(x)^T G_sj + sqrt(v_j(x)) W[s, j]
//   T_ls = max(best_l, max_i U(theta_l, F_s[:, i]))
//   alpha(x | P) = sum_l p_l (1/S) sum_s max(U(theta_l, y_s(x)) - T_ls, 0)
// (F, G, c, y) is the Cholesky factor of the bordered joint covariance of [f(P), f(x)]: alpha(x | P) = qEI(P u {x}) - qEI(P) for the same normals.
//   pending_pack_kernel       Sigma(P, P) and mu(P) of every output in one contiguous block for the host
//   pending_threshold_kernel  T_ls
//   pending_acq_kernel        alpha(x_c | P), one wave per candidate
//   pending_grad_kernel       d alpha / dx_c with P, Zp, W held fixed
// fp64 throughout.  Every sum has a fixed order; every kernel writes its own outputs only (no atomics).
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"
#include "utility_dev.h"

#define PEND_CLIP 1e-10          // the variance clip of predict_noiseless, as in kg.hip
#define PEND_MAX_R 15

__global__ __launch_bounds__(256) void pending_pack_kernel(const double* __restrict__ cov, long ldc, long strideC, const double* __restrict__ mu, long ldmu,
                                                           int r, double* __restrict__ out) {
  const int j = blockIdx.x, m = gridDim.x, rr = r * r;
  for (int e = threadIdx.x; e < rr + r; e += 256) {
    if (e < rr) {
      const int i = e / r, k = e - i * r;
      out[(long)j * rr + e] = cov[(long)j * strideC + (long)i * ldc + k];
    } else {
      out[(long)m * rr + (long)j * r + (e - rr)] = mu[(long)j * ldmu + (e - rr)];
    }
  }
}

void launch_pending_pack(const double* cov, long ldc, long strideC, const double* mu, long ldmu, int r, double* out, int m, hipStream_t s) {
  if (m <= 0 || r <= 0) return;
  BOCF_LAUNCH(pending_pack_kernel, dim3((unsigned)m), dim3(256), 0, s, cov, ldc, strideC, mu, ldmu, r, out);
}

// ---------------------------------------------------------------------------------------------
// One workgroup per parameter l, one thread per sample s: the pending points in index order.
__global__ __launch_bounds__(256) void pending_threshold_kernel(PendArgs g) {
  const int l = blockIdx.x, s = threadIdx.x;
  if (s >= g.S) return;
  const double* th = g.theta + (long)l * g.theta_dim;
  double t = g.best[l];
  for (int i = 0; i < g.r; ++i) {
    double y[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = j < g.m ? g.F[((long)j * g.r + i) * g.S + s] : 0.0;
    t = fmax(t, utility_eval(g.util_kind, th, g.util_params, y, g.m));
  }
  g.T[(long)l * g.S + s] = t;
}

void launch_pending_threshold(const PendArgs& a, hipStream_t s) {
  if (a.L <= 0 || a.S <= 0) return;
  BOCF_LAUNCH(pending_threshold_kernel, dim3((unsigned)a.L), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------------------------
// the tables a value launch reads: G, W, T, theta, prob, utility parameters -- in this order in LDS (TAB) or in memory.  G is [j][i][s],
// W [j][s], T [l][s]: consecutive lanes (samples) read consecutive words.
struct PendTables {
  const double* G; const double* Wt; const double* T; const double* theta; const double* prob; const double* params;
};

size_t pending_table_bytes(const PendArgs& a) {
  const size_t n = (size_t)a.m * a.r * a.S + (size_t)a.m * a.S + (size_t)a.L * a.S + (size_t)a.L * a.theta_dim + (size_t)a.L + BOCF_MAX_M;
  return n * sizeof(double);
}

template <bool TAB>
__device__ __forceinline__ PendTables pending_tables(const PendArgs& g, double* lds) {
  PendTables t;
  if constexpr (TAB) {
    const int nG = g.m * g.r * g.S, nW = g.m * g.S, nT = g.L * g.S, nth = g.L * g.theta_dim;
    double* G = lds;
    double* Wt = G + nG;
    double* T = Wt + nW;
    double* theta = T + nT;
    double* prob = theta + nth;
    double* params = prob + g.L;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < nG; e += nt) G[e] = g.G[e];
    for (int e = tid; e < nW; e += nt) Wt[e] = g.Wt[e];
    for (int e = tid; e < nT; e += nt) T[e] = g.T[e];
    for (int e = tid; e < nth; e += nt) theta[e] = g.theta[e];
    for (int e = tid; e < g.L; e += nt) prob[e] = g.prob[e];
    for (int e = tid; e < BOCF_MAX_M; e += nt) params[e] = g.util_params[e];
    __syncthreads();
    t.G = G; t.Wt = Wt; t.T = T; t.theta = theta; t.prob = prob; t.params = params;
  } else {
    t.G = g.G; t.Wt = g.Wt; t.T = g.T; t.theta = g.theta; t.prob = g.prob; t.params = g.util_params;
  }
  return t;
}

// sum over the wave in a fixed butterfly: every lane ends with the same bits
__device__ __forceinline__ double pending_wave_sum(double t) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  return t;
}

// c_j^T Q_j c_j of candidate c: lane i < r forms a_i = (Q_j c_j)_i (k increasing) and a_i c_ji, the wave adds them up.  Returns the raw
// conditioned variance sigma^2_j(x_c) - c^T Q c on every lane; `a` is this lane's a_i (0 from lane r on).
__device__ __forceinline__ double pending_raw_var(const PendArgs& g, int j, int c, int lane, double& a) {
  const double* __restrict__ cj = g.cov + (long)j * g.strideC + (long)c * g.ldc;
  a = 0.0;
  double t = 0.0;
  if (lane < g.r) {
    const double* __restrict__ q = g.Q + ((long)j * g.r + lane) * g.r;
    for (int k = 0; k < g.r; ++k) a = __builtin_fma(q[k], cj[k], a);
    t = a * cj[lane];
  }
  return g.s2c[(long)j * g.lds + c] - pending_wave_sum(t);
}

// y_sj of one sample for every output: mu_j + sqrt(v_j) W_sj + sum_i c_ji G_sji, i increasing
__device__ __forceinline__ void pending_sample(const PendArgs& g, const PendTables& t, int c, int s, int m, const double (&mu)[BOCF_MAX_M],
                                               const double (&sv)[BOCF_MAX_M], double (&y)[BOCF_MAX_M]) {
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    double acc = 0.0;
    if (j < m) {
      const double* __restrict__ cj = g.cov + (long)j * g.strideC + (long)c * g.ldc;
      const double* __restrict__ Gj = t.G + (long)j * g.r * g.S + s;
      acc = __builtin_fma(sv[j], t.Wt[(long)j * g.S + s], mu[j]);
      for (int i = 0; i < g.r; ++i) acc = __builtin_fma(cj[i], Gj[(long)i * g.S], acc);
    }
    y[j] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// One wave per candidate (four per workgroup, the layout of eu_kernel / kg_kernel).  The wave forms v_j once (wave-uniform); the lanes
// stride the samples s; y_s is formed once per sample and reused for the L parameters (l in index order); the lanes' sums meet in a fixed
// butterfly.  Nothing depends on the other candidates of the launch.
// (MC = the output count as a template argument, 1 ... 8, or 0 = read it from the arguments, as in kg_kernel)
template <bool TAB, int MC>
__global__ __launch_bounds__(256) void pending_acq_kernel(PendArgs g) {
  extern __shared__ double pend_lds[];
  const PendTables t = pending_tables<TAB>(g, pend_lds);
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (c >= g.C) return;                          // wave-uniform (behind the workgroup barrier of the table load)
  const int m = MC > 0 ? MC : g.m;
  double mu[BOCF_MAX_M], sv[BOCF_MAX_M];
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    mu[j] = 0.0;
    sv[j] = 0.0;
    if (j < m) {
      double a;
      mu[j] = g.muc[(long)j * g.lds + c];
      sv[j] = sqrt(fmax(pending_raw_var(g, j, c, lane, a), PEND_CLIP));
    }
  }
  double acc = 0.0;
  for (int s = lane; s < g.S; s += 64) {
    double y[BOCF_MAX_M];
    pending_sample(g, t, c, s, m, mu, sv, y);
    for (int l = 0; l < g.L; ++l) {
      const double u = utility_eval(g.util_kind, t.theta + (long)l * g.theta_dim, t.params, y, m);
      acc += t.prob[l] * fmax(u - t.T[(long)l * g.S + s], 0.0);
    }
  }
  acc = pending_wave_sum(acc);
  if (lane == 0) g.acq[c] = (g.accumulate ? g.acq[c] : 0.0) + acc * (1.0 / g.S) * g.scale;
}

template <bool TAB>
static void launch_pending_m(const PendArgs& a, dim3 grid, size_t shm, hipStream_t s) {
#define LM(M) case M: BOCF_LAUNCH((pending_acq_kernel<TAB, M>), grid, dim3(256), shm, s, a); return;
  switch (a.m) { LM(1) LM(2) LM(3) LM(4) LM(5) LM(6) LM(7) LM(8) default: break; }
#undef LM
  BOCF_LAUNCH((pending_acq_kernel<TAB, 0>), grid, dim3(256), shm, s, a);
}

void launch_pending_acq(const PendArgs& a, hipStream_t s) {
  if (a.C <= 0) return;
  const dim3 grid((unsigned)((a.C + 3) / 4));
  const size_t bytes = pending_table_bytes(a);
  if (bytes <= 65536) launch_pending_m<true>(a, grid, bytes, s);
  else launch_pending_m<false>(a, grid, 0, s);
}

// ---------------------------------------------------------------------------------------------
// d alpha / dx_c.  Same traversal: one wave per candidate, the lanes stride the samples.  With w_ls = p_l / S on the improving (l, s) and
// g_lsj = dU/dy_j there,  e_sj = sum_l w_ls g_lsj  and per output
//   A_j = sum_s e_sj,  B_j = sum_s e_sj W_sj,  D_ji = sum_s e_sj G_sji
//   d alpha / dx_q = sum_j [ A_j dmu_j/dx_q + sum_i D_ji dc_ji/dx_q + B_j / (2 sqrt(v_j)) dv_j/dx_q ],
//   dv_j/dx_q = dsigma^2_j/dx_q - 2 sum_i a_ji dc_ji/dx_q,  a_j = Q_j c_j;  zero where the 1e-10 clip is active.
// The m (2 + r) accumulators (272 at m = 16, r = 15) do not fit a lane's registers.  Pass 1 forms y_s and the utility gradients ONCE per
// sample and leaves e_sj in the scratch E (C, m, S); pass 2 walks the outputs one at a time with 2 + r accumulators, reading e_sj back -- every
// lane reads exactly the words it wrote itself (same lane-to-sample map), so no barrier and no LDS are involved.  The tables are read from
// memory (the gradient form serves the optimiser's small batches).  Lane q < d assembles coordinate q.
__global__ __launch_bounds__(256) void pending_grad_kernel(PendArgs g) {
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (c >= g.C) return;
  const int m = g.m, r = g.r, S = g.S;
  PendTables t;
  t.G = g.G; t.Wt = g.Wt; t.T = g.T; t.theta = g.theta; t.prob = g.prob; t.params = g.util_params;
  double* E = g.E + (long)c * m * S;
  {
    double mu[BOCF_MAX_M], sv[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) {
      mu[j] = 0.0;
      sv[j] = 0.0;
      if (j < m) {
        double a;
        mu[j] = g.muc[(long)j * g.lds + c];
        sv[j] = sqrt(fmax(pending_raw_var(g, j, c, lane, a), PEND_CLIP));
      }
    }
    const double invS = 1.0 / S;
    for (int s = lane; s < S; s += 64) {
      double y[BOCF_MAX_M], e[BOCF_MAX_M];
      pending_sample(g, t, c, s, m, mu, sv, y);
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j) e[j] = 0.0;
      for (int l = 0; l < g.L; ++l) {
        const double* th = t.theta + (long)l * g.theta_dim;
        if (utility_eval(g.util_kind, th, t.params, y, m) > t.T[(long)l * S + s]) {
          double du[BOCF_MAX_M];
          utility_grad(g.util_kind, th, t.params, y, m, du);
          const double w = t.prob[l] * invS;
#pragma unroll
          for (int j = 0; j < BOCF_MAX_M; ++j) e[j] = __builtin_fma(w, du[j], e[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j)
        if (j < m) E[(long)j * S + s] = e[j];
    }
  }
  const int q = lane < g.d ? lane : g.d - 1;       // (lanes from d on compute coordinate d - 1 again and do not store)
  double gq = 0.0;
  for (int j = 0; j < m; ++j) {
    double A = 0.0, B = 0.0, D[PEND_MAX_R];
#pragma unroll
    for (int i = 0; i < PEND_MAX_R; ++i) D[i] = 0.0;
    for (int s = lane; s < S; s += 64) {
      const double e = E[(long)j * S + s];
      A += e;
      B = __builtin_fma(e, t.Wt[(long)j * S + s], B);
#pragma unroll
      for (int i = 0; i < PEND_MAX_R; ++i)
        if (i < r) D[i] = __builtin_fma(e, t.G[((long)j * r + i) * S + s], D[i]);
    }
    A = pending_wave_sum(A);
    B = pending_wave_sum(B);
    double a;
    const double raw = pending_raw_var(g, j, c, lane, a);
    const double* __restrict__ dc = g.dcov + (((long)j * g.C + c) * r) * g.d + q;
    double acc = A * g.dmu[((long)j * g.ldg + c) * g.d + q];
    double adc = 0.0;
#pragma unroll
    for (int i = 0; i < PEND_MAX_R; ++i)
      if (i < r) {
        const double Di = pending_wave_sum(D[i]);
        const double ai = __shfl(a, i, 64);
        const double dci = dc[(long)i * g.d];
        acc = __builtin_fma(Di, dci, acc);
        adc = __builtin_fma(ai, dci, adc);
      }
    if (raw > PEND_CLIP) acc += B * (0.5 / sqrt(raw)) * (g.ds2[((long)j * g.ldg + c) * g.d + q] - 2.0 * adc);
    gq += acc;
  }
  if (lane < g.d) g.dacq[(long)c * g.d + lane] = (g.accumulate ? g.dacq[(long)c * g.d + lane] : 0.0) + gq * g.scale;
}

void launch_pending_grad(const PendArgs& a, hipStream_t s) {
  if (a.C <= 0 || a.d <= 0) return;
  BOCF_LAUNCH(pending_grad_kernel, dim3((unsigned)((a.C + 3) / 4)), dim3(256), 0, s, a);
}
