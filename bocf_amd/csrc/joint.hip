// Joint Monte-Carlo expected improvement of the composite utility at whole q-point batches, q <= 8 (capi_joint.hip drives it).
// Per output j of a batch X = (x_1 .. x_q): mu_j(X) (q), Sigma_j = k_j(X, X) - V_X^T V_X symmetrised (latent, noiseless),
// tau_j = 1e-8 max(mean diag Sigma_j, 1e-10), C_j = the floored row-wise Cholesky factor of Sigma_j + tau_j I (joint_chol.h), and with the
// host normals Z (S, m, q) common to all batches
//   y_sjk = mu_jk + sum_{i <= k} C_j[k][i] Z[s, j, i],   u_lsk = U(theta_l, y_s.k),   k* = the lowest index of max_k u_lsk
//   alpha(X) = sum_l p_l (1/S) sum_s max(u_lsk* - best_l, 0)
//   joint_acq_kernel    alpha of every batch and the number of floored pivots, one workgroup per batch, lanes = samples
//   joint_grad_kernel   the same value (same bits) and d alpha / dx_a by the envelope rule with Z, theta, best fixed:
//                       Ybar[s][j][k*] += p_l 1[u > best_l] dU/dy_j;  mubar_jk = sum_s Ybar[s][j][k];  Cbar_j[k][i] = sum_s Ybar[s][j][k] Z[s, j, i];
//                       Sigmabar_j = the reverse pass of the factorization;  d alpha / dx_a = sum_j [ mubar_ja dmu_j(x_a)/dx +
//                       Sigmabar_j[a][a] dsigma^2_j(x_a)/dx + 2 sum_{b != a} Sigmabar_j[a][b] d_1 Sigma_j(x_a, x_b) ]
// Z stays in memory (S m q doubles, up to 256 KiB: more than a workgroup's LDS; every batch reads the same words, so they come from L2),
// transposed to (m, q, S) so that consecutive lanes read consecutive words.  LDS holds the batch's factors, means and adjoints.
// fp64 throughout.  Every sum has a fixed order; every kernel writes its own outputs only (no atomics).
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"
#include "joint_chol.h"
#include "utility_dev.h"

#define JOINT_LC 4               // utility parameters per pass over the q points (their running maxima stay in registers)
#define JOINT_LDQ JOINT_MAX_Q    // row stride of a factor in LDS

struct JointLds {
  double C[BOCF_MAX_M][JOINT_MAX_Q * JOINT_LDQ];    // Sigma_j, then its factor (lower triangle)
  double G[BOCF_MAX_M][JOINT_MAX_Q * JOINT_LDQ];    // gradient form: Cbar_j, then d alpha / d Sigma_j (lower triangle)
  double mu[BOCF_MAX_M][JOINT_MAX_Q];
  double mub[BOCF_MAX_M][JOINT_MAX_Q];
  double wsum[4];
  unsigned floored[BOCF_MAX_M];
};

// thread j < m: Sigma_j of batch b symmetrised into LDS, factorized in place; mu_j(X)
__device__ __forceinline__ void joint_factor(const JointArgs& g, int b, JointLds& L) {
  const int j = threadIdx.x, q = g.q;
  if (j < g.m) {
    const double* __restrict__ cv = g.cov + (long)j * g.strideC;
    const long c0 = (long)b * q;
    for (int k = 0; k < q; ++k) {
      for (int i = 0; i <= k; ++i) L.C[j][k * JOINT_LDQ + i] = 0.5 * (cv[(c0 + k) * g.ldc + c0 + i] + cv[(c0 + i) * g.ldc + c0 + k]);
      L.mu[j][k] = g.mu[(long)j * g.ldm + c0 + k];
    }
    const double tau = joint_chol_tau(L.C[j], q, JOINT_LDQ);
    L.floored[j] = joint_chol_floor(L.C[j], JOINT_LDQ, q, tau, L.C[j], JOINT_LDQ);
  }
  __syncthreads();
}

// y_s.k of sample s at point k for every output: mu_jk + sum_{i <= k} C_j[k][i] Z[s, j, i], i increasing
__device__ __forceinline__ void joint_point(const JointArgs& g, const JointLds& L, int s, int k, double (&y)[BOCF_MAX_M]) {
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    double acc = 0.0;
    if (j < g.m) {
      const double* __restrict__ z = g.Zt + (long)j * g.q * g.S + s;
      const double* c = &L.C[j][k * JOINT_LDQ];
      acc = L.mu[j][k];
      for (int i = 0; i <= k; ++i) acc = __builtin_fma(c[i], z[(long)i * g.S], acc);
    }
    y[j] = acc;
  }
}

// the maximum over the q points and its lowest index for parameters l0 .. l0 + JOINT_LC - 1 of sample s: the points are walked once, y_s.k
// is formed once per point and reused for the parameters
__device__ __forceinline__ void joint_walk(const JointArgs& g, const JointLds& L, int s, int l0, double (&um)[JOINT_LC], int (&ks)[JOINT_LC]) {
#pragma unroll
  for (int t = 0; t < JOINT_LC; ++t) {
    um[t] = -__builtin_inf();
    ks[t] = 0;
  }
  for (int k = 0; k < g.q; ++k) {
    double y[BOCF_MAX_M];
    joint_point(g, L, s, k, y);
#pragma unroll
    for (int t = 0; t < JOINT_LC; ++t)
      if (l0 + t < g.L) {
        const double u = utility_eval(g.util_kind, g.theta + (long)(l0 + t) * g.theta_dim, g.util_params, y, g.m);
        if (u > um[t]) {
          um[t] = u;
          ks[t] = k;
        }
      }
  }
}

// sum over the workgroup in a fixed order: a butterfly inside every wave, then the waves in index order; thread 0 holds the result
__device__ __forceinline__ double joint_block_sum(double t, JointLds& L) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) L.wsum[w] = t;
  __syncthreads();
  double r = 0.0;
  for (int i = 0; i < nw; ++i) r += L.wsum[i];
  return r;
}

__device__ __forceinline__ void joint_store_value(const JointArgs& g, int b, double acc, JointLds& L) {
  const double total = joint_block_sum(acc, L);
  if (threadIdx.x == 0) {
    g.acq[b] = (g.accumulate ? g.acq[b] : 0.0) + total * (1.0 / g.S) * g.scale;
    if (g.floored) {
      int n = 0;
      for (int j = 0; j < g.m; ++j) n += __builtin_popcount(L.floored[j]);
      g.floored[b] = (g.accumulate ? g.floored[b] : 0) + n;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// One workgroup per batch, S rounded up to whole waves of threads; thread s is sample s.
__global__ __launch_bounds__(256) void joint_acq_kernel(JointArgs g) {
  __shared__ JointLds L;
  const int b = blockIdx.x, s = threadIdx.x;
  joint_factor(g, b, L);
  double acc = 0.0;
  if (s < g.S)
    for (int l0 = 0; l0 < g.L; l0 += JOINT_LC) {
      double um[JOINT_LC];
      int ks[JOINT_LC];
      joint_walk(g, L, s, l0, um, ks);
#pragma unroll
      for (int t = 0; t < JOINT_LC; ++t)
        if (l0 + t < g.L) acc += g.prob[l0 + t] * fmax(um[t] - g.best[l0 + t], 0.0);
    }
  joint_store_value(g, b, acc, L);
}

// ---------------------------------------------------------------------------------------------
// The value as above, then the reverse pass.  Phase 1: thread s zeroes its column of E (b, m, q, S) and adds p_l dU/dy at (j, k*) of every
// improving parameter, l increasing -- every thread touches the words of its own sample only.  Phase 2: one thread per entry of mubar (m q)
// and of the lower triangle of Cbar (m q (q + 1) / 2) sums over s in increasing order.  Phase 3: thread j runs the factorization's reverse
// pass of output j.  Phase 4: one thread per (point a, coordinate) gathers d alpha / dx_a over the outputs in increasing order.
__global__ __launch_bounds__(256) void joint_grad_kernel(JointArgs g) {
  __shared__ JointLds L;
  const int b = blockIdx.x, s = threadIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const int m = g.m, q = g.q, S = g.S, d = g.d;
  joint_factor(g, b, L);
  double* __restrict__ E = g.E + (long)b * m * q * S;
  double acc = 0.0;
  if (s < S) {
    for (int e = 0; e < m * q; ++e) E[(long)e * S + s] = 0.0;
    for (int l0 = 0; l0 < g.L; l0 += JOINT_LC) {
      double um[JOINT_LC];
      int ks[JOINT_LC];
      joint_walk(g, L, s, l0, um, ks);
#pragma unroll
      for (int t = 0; t < JOINT_LC; ++t)
        if (l0 + t < g.L) {
          const int l = l0 + t;
          acc += g.prob[l] * fmax(um[t] - g.best[l], 0.0);
          if (um[t] > g.best[l]) {
            double y[BOCF_MAX_M], du[BOCF_MAX_M];
            joint_point(g, L, s, ks[t], y);
            utility_grad(g.util_kind, g.theta + (long)l * g.theta_dim, g.util_params, y, m, du);
            const double w = g.prob[l];
            double* __restrict__ Ek = E + (long)ks[t] * S + s;
#pragma unroll
            for (int j = 0; j < BOCF_MAX_M; ++j)
              if (j < m) Ek[(long)j * q * S] = __builtin_fma(w, du[j], Ek[(long)j * q * S]);
          }
        }
    }
  }
  joint_store_value(g, b, acc, L);
  __syncthreads();                                 // E of every sample is written (workgroup scope)
  const int tri = q * (q + 1) / 2, nmu = m * q, nent = nmu + m * tri;
  for (int e = tid; e < nent; e += nt) {
    if (e < nmu) {
      const double* __restrict__ Ee = E + (long)e * S;
      double t = 0.0;
      for (int i = 0; i < S; ++i) t += Ee[i];
      L.mub[e / q][e % q] = t;
    } else {
      const int j = (e - nmu) / tri;
      int i = (e - nmu) - j * tri, k = 0;
      while (i > k) {
        i -= k + 1;
        ++k;
      }
      const double* __restrict__ Ee = E + ((long)j * q + k) * S;
      const double* __restrict__ z = g.Zt + ((long)j * q + i) * S;
      double t = 0.0;
      for (int ss = 0; ss < S; ++ss) t = __builtin_fma(Ee[ss], z[ss], t);
      L.G[j][k * JOINT_LDQ + i] = t;
    }
  }
  __syncthreads();
  if (tid < m) joint_chol_adjoint(L.C[tid], JOINT_LDQ, q, L.floored[tid], L.G[tid], JOINT_LDQ);
  __syncthreads();
  const double f = (1.0 / S) * g.scale;
  for (int e = tid; e < q * d; e += nt) {
    const int a = e / d, x = e - a * d;
    const long c = (long)b * q + a;
    double t = 0.0;
    for (int j = 0; j < m; ++j) {
      double tj = L.mub[j][a] * g.dmu[((long)j * g.ldg + c) * d + x];
      tj = __builtin_fma(L.G[j][a * JOINT_LDQ + a], g.ds2[((long)j * g.ldg + c) * d + x], tj);
      const double* __restrict__ dc = g.dcov + (((long)j * g.Cn + c) * g.Cn + (long)b * q) * d + x;
      for (int o = 0; o < q; ++o)
        if (o != a) tj = __builtin_fma(o > a ? L.G[j][o * JOINT_LDQ + a] : L.G[j][a * JOINT_LDQ + o], dc[(long)o * d], tj);
      t += tj;
    }
    g.dacq[c * d + x] = (g.accumulate ? g.dacq[c * d + x] : 0.0) + t * f;
  }
}

// acq[i] = -inf for B <= i < n: the acquisition vector holds one value per batch, the selection reads one per resident candidate
__global__ __launch_bounds__(256) void joint_tail_kernel(double* __restrict__ acq, int B, int n) {
  const int i = B + blockIdx.x * 256 + threadIdx.x;
  if (i < n) acq[i] = -__builtin_inf();
}

static dim3 joint_block(const JointArgs& a) { return dim3((unsigned)((a.S + 63) / 64 * 64)); }

void launch_joint_acq(const JointArgs& a, hipStream_t s) {
  if (a.B <= 0) return;
  BOCF_LAUNCH(joint_acq_kernel, dim3((unsigned)a.B), joint_block(a), 0, s, a);
}

void launch_joint_grad(const JointArgs& a, hipStream_t s) {
  if (a.B <= 0 || a.d <= 0) return;
  BOCF_LAUNCH(joint_grad_kernel, dim3((unsigned)a.B), joint_block(a), 0, s, a);
}

void launch_joint_tail(double* acq, int B, int n, hipStream_t s) {
  if (n <= B) return;
  BOCF_LAUNCH(joint_tail_kernel, dim3((unsigned)((n - B + 255) / 256)), dim3(256), 0, s, acq, B, n);
}
