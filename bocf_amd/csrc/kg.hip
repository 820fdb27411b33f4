// Look-ahead posterior and the discrete composite knowledge gradient (capi_kg.hip drives them).  Per output j, with the fit's own
// Ky_j = K_j + (noise_j + 1e-8 + jitter_j) I and Sigma_j(a, x) = k_j(a, x) - k_j(a, X) Ky_j^-1 k_j(X, x):
//   s2_j(x)       = max(sigma^2_j(x), 0) + noise_j + 1e-8 + jitter_j
//   beta_j(a; x)  = Sigma_j(a, x) / s_j(x)
//   mu_j(a | x, z) = mu_j(a) + beta_j z_j,   sigma^2_j(a | x) = sigma^2_j(a) - beta_j^2       (gp.py:514-544: the bordered factorization, by the
//                                                                                            Schur complement a rank-one downdate)
//   KG(x) = sum_l p_l [ (1/Sf) sum_s max_a v(a; x, z_s, theta_l) - max_a v0(a; theta_l) ],
//   v = E_w[ U(theta, mu(a | x, z) + sigma(a | x) o w) ] with sigma^2 clipped at 1e-10, v0 the same from the current mu(a), sigma^2(a).
//   kg_diag_kernel    raw sigma^2 from V = R^T K(X, .): variance - column sums of squares
//   cov_grad_kernel   d Sigma_j(a, x_c) / dx_c against the resident Wa = Ky^-1 K(X, A)
//   cond_var_kernel   the conditioned variance and its input gradient
//   kg_v0_kernel      max_a v0(a; theta_l)
//   kg_kernel         KG(x_c), one wave per candidate; with gradients also the maximiser a* of every (l, s)
//   kg_partials_kernel  dv/dmu, dv/dvar at a* per (candidate, l, s)
//   kg_grad_kernel    the envelope-rule gradient from those
// fp64 throughout.  Every sum and maximum has a fixed order; every kernel writes its own outputs only (no atomics).
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"
#include "kern_family.h"
#include "utility_dev.h"
#include "eu_dev.h"

#define KG_CLIP 1e-10            // predict_noiseless's variance clip (gpmodel_fixed_hyps.py:95)

// ---------------------------------------------------------------------------------------------
// One thread per column: the rows in increasing order (coalesced across the columns).
__global__ __launch_bounds__(256) void kg_diag_kernel(const double* __restrict__ V, long ldv, long strideV, int K, int n, const KernHyp* __restrict__ hyp,
                                                      double* __restrict__ out, long ldo) {
  const int j = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const double* __restrict__ v = V + (long)j * strideV + c;
  double acc = 0.0;
  for (int k = 0; k < K; ++k) {
    const double t = v[(long)k * ldv];
    acc = __builtin_fma(t, t, acc);
  }
  out[(long)j * ldo + c] = hyp[j].variance - acc;          // k_j(x, x) = variance_j for every family
}

void launch_kg_diag(const double* V, long ldv, long strideV, int K, int n, const KernHyp* hyp, double* out, long ldo, int m, hipStream_t s) {
  if (m <= 0 || n <= 0) return;
  BOCF_LAUNCH(kg_diag_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)m), dim3(256), 0, s, V, ldv, strideV, K, n, hyp, out, ldo);
}

// ---------------------------------------------------------------------------------------------
// One workgroup per (candidate, output).  g_i = f(r_i) (x_c - X_i) (scaled coordinates, kern_dfac of kern_family.h) of 64 training rows at a
// time goes through LDS; thread t owns reference point a0 + t (+ 256, ...) and adds g_i Wa[i][a] over the rows in increasing order.
#define CG_ROWS 64
template <int D>
__global__ __launch_bounds__(256) void cov_grad_kernel(const double* __restrict__ Xs, long strideXs, int N, int kernel_id, const KernHyp* __restrict__ hyp,
                                                       const double* __restrict__ Xc, int Cn, const double* __restrict__ XA, int a0, int an,
                                                       const double* __restrict__ Wa, long ldw, long strideW, double* __restrict__ out) {
  __shared__ double gl[CG_ROWS][D];
  const int c = blockIdx.x, j = blockIdx.y, tid = threadIdx.x;
  const KernHyp h = hyp[j];
  double xc[D];
#pragma unroll
  for (int q = 0; q < D; ++q) xc[q] = Xc[(long)c * D + q] / h.ls[q];
  const double* __restrict__ X = Xs + (long)j * strideXs;
  const double* __restrict__ W = Wa + (long)j * strideW;
  for (int ab = 0; ab < an; ab += 256) {
    const int a = ab + tid;
    const bool valid = a < an;
    double acc[D];
#pragma unroll
    for (int q = 0; q < D; ++q) acc[q] = 0.0;
    for (int i0 = 0; i0 < N; i0 += CG_ROWS) {
      __syncthreads();
      if (tid < CG_ROWS) {
        const int i = i0 + tid;
        double df[D];
        double r2 = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) {
          df[q] = i < N ? xc[q] - X[(long)i * D + q] : 0.0;
          r2 += df[q] * df[q];
        }
        const double f = kern_dfac(kernel_id, h.variance, r2);
#pragma unroll
        for (int q = 0; q < D; ++q) gl[tid][q] = f * df[q];
      }
      __syncthreads();
      const int rows = N - i0 < CG_ROWS ? N - i0 : CG_ROWS;
      if (valid)
        for (int ii = 0; ii < rows; ++ii) {
          const double w = W[(long)(i0 + ii) * ldw + a0 + a];
#pragma unroll
          for (int q = 0; q < D; ++q) acc[q] = __builtin_fma(gl[ii][q], w, acc[q]);
        }
    }
    if (valid) {
      double df[D];
      double r2 = 0.0;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        df[q] = xc[q] - XA[(long)(a0 + a) * D + q] / h.ls[q];
        r2 += df[q] * df[q];
      }
      const double f = kern_dfac(kernel_id, h.variance, r2);
      double* o = out + (((long)j * Cn + c) * an + a) * D;
#pragma unroll
      for (int q = 0; q < D; ++q) o[q] = (f * df[q] - acc[q]) / h.ls[q];      // (scaled coordinates: (x_q - y_q) / l_q^2 = df_q / l_q)
    }
  }
}

void launch_cov_grad(const double* Xs, long strideXs, int N, int d, int kernel_id, const int* kids, const KernHyp* hyp, const double* Xc, int Cn,
                     const double* XA, int a0, int an, const double* Wa, long ldw, long strideW, double* out, int m, hipStream_t s) {
  if (m <= 0 || Cn <= 0 || an <= 0) return;
  bocf_family_runs(kernel_id, kids, m, [&](int j0, int mr, int kid) {
    const dim3 grid((unsigned)Cn, (unsigned)mr);
    bocf_launch_by_d("cov_grad_kernel", d, [&](auto Dc) {
      constexpr int D = decltype(Dc)::value;
      BOCF_LAUNCH(cov_grad_kernel<D>, grid, dim3(256), 0, s, Xs + (long)j0 * strideXs, strideXs, N, kid, hyp + j0, Xc, Cn, XA, a0, an,
                  Wa + (long)j0 * strideW, ldw, strideW, out + (long)j0 * Cn * an * d);
    });
  });
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cond_var_kernel(const double* __restrict__ cov, long ldc, long strideC, int q, const double* __restrict__ s2c, long lds,
                                                       const double* __restrict__ s2A, long lda, const double* __restrict__ nug,
                                                       const double* __restrict__ ds2c, long ldg, const double* __restrict__ dcov, int C, int d,
                                                       double* __restrict__ var, double* __restrict__ dvar) {
  const int j = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const double s2q = fmax(s2A[(long)j * lda + q], 0.0) + nug[j];
  const double cv = cov[(long)j * strideC + (long)c * ldc + q];
  var[(long)j * C + c] = s2c[(long)j * lds + c] - cv * cv / s2q;
  if (dvar)
    for (int k = 0; k < d; ++k)
      dvar[((long)j * C + c) * d + k] = ds2c[((long)j * ldg + c) * d + k] - 2.0 * cv * dcov[((long)j * C + c) * d + k] / s2q;
}

void launch_cond_var(const double* cov, long ldc, long strideC, int q, const double* s2c, long lds, const double* s2A, long lda, const double* nug,
                     const double* ds2c, long ldg, const double* dcov, int C, int d, double* var, double* dvar, int m, hipStream_t s) {
  if (m <= 0 || C <= 0) return;
  BOCF_LAUNCH(cond_var_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)m), dim3(256), 0, s, cov, ldc, strideC, q, s2c, lds, s2A, lda, nug, ds2c, ldg,
              dcov, C, d, var, dvar);
}

// ---------------------------------------------------------------------------------------------
// v = E_w[ U(theta, mu + sigma o w) ] of one (reference point, fantasy, parameter) in the three modes of the expected-utility kernel, with
// GRAD its partials A = dv/dmu, B = dv/dvar.  MC: the MEAN over the S common random numbers Wt (m, S), samples in increasing order.
template <int MODE, bool GRAD>
__device__ __forceinline__ double kg_inner(int kind, const double* __restrict__ th, const double* __restrict__ params, const double (&mu)[BOCF_MAX_M],
                                           const double (&s2)[BOCF_MAX_M], int m, const double* __restrict__ Wt, int S, double (&A)[BOCF_MAX_M],
                                           double (&B)[BOCF_MAX_M]) {
  if constexpr (MODE == BOCF_EU_MEAN) {
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < m) {
        v += th[j] * mu[j];
        if (GRAD) A[j] = th[j];
      }
    return v;
  } else if constexpr (MODE == BOCF_EU_CLOSED) {
    return eu_closed(kind, th, mu, s2, m, A, B);
  } else {
    double sg[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) sg[j] = j < m ? sqrt(s2[j]) : 1.0;
    double acc = 0.0;
    for (int s = 0; s < S; ++s) {
      double y[BOCF_MAX_M], g[BOCF_MAX_M];
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = mu[j] + sg[j] * (j < m ? Wt[(long)j * S + s] : 0.0);
      acc += utility_eval(kind, th, params, y, m);
      if (GRAD) {
        utility_grad(kind, th, params, y, m, g);
#pragma unroll
        for (int j = 0; j < BOCF_MAX_M; ++j) {
          A[j] += g[j];
          B[j] += j < m ? g[j] * Wt[(long)j * S + s] : 0.0;
        }
      }
    }
    const double inv = 1.0 / S;
    if (GRAD) {
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j) {
        A[j] *= inv;
        B[j] *= inv * 0.5 / sg[j];                // d sigma / d var = 1 / (2 sigma)
      }
    }
    return acc * inv;
  }
}

// (value, index) maximum over the wave, ties to the lowest index: every lane ends with the same pair
__device__ __forceinline__ void kg_wave_argmax(double& best, int& bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
}

// the tables a launch reads: mu(A), sigma^2(A), Zf, theta, prob, v0, Wt, utility parameters -- in this order in LDS (TAB) or in memory
struct KgTables {
  const double* muA; const double* s2A; int lda;
  const double* Zf; const double* theta; const double* prob; const double* v0; const double* Wt; const double* params;
};

size_t kg_table_bytes(const KgArgs& a) {
  const size_t n = 2 * (size_t)a.m * a.na + (size_t)a.Sf * a.m + (size_t)a.L * a.theta_dim + 2 * (size_t)a.L +
                   (a.mode == BOCF_EU_MC ? (size_t)a.m * a.S : 0) + BOCF_MAX_M;
  return n * sizeof(double);
}

template <bool TAB>
__device__ __forceinline__ KgTables kg_tables(const KgArgs& g, double* lds) {
  KgTables t;
  if constexpr (TAB) {
    const int mS = g.mode == BOCF_EU_MC ? g.m * g.S : 0;
    double* muA = lds;
    double* s2A = muA + g.m * g.na;
    double* Zf = s2A + g.m * g.na;
    double* theta = Zf + g.Sf * g.m;
    double* prob = theta + g.L * g.theta_dim;
    double* v0 = prob + g.L;
    double* Wt = v0 + g.L;
    double* params = Wt + mS;
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < g.m * g.na; e += nt) {
      const int j = e / g.na, a = e - j * g.na;
      muA[e] = g.muA[(long)j * g.lda + a];
      s2A[e] = g.s2A[(long)j * g.lda + a];
    }
    for (int e = tid; e < g.Sf * g.m; e += nt) Zf[e] = g.Zf[e];
    for (int e = tid; e < g.L * g.theta_dim; e += nt) theta[e] = g.theta[e];
    for (int e = tid; e < g.L; e += nt) {
      prob[e] = g.prob[e];
      v0[e] = g.v0 ? g.v0[e] : 0.0;
    }
    for (int e = tid; e < mS; e += nt) Wt[e] = g.Wt[e];
    for (int e = tid; e < BOCF_MAX_M; e += nt) params[e] = g.util_params[e];
    __syncthreads();
    t.muA = muA; t.s2A = s2A; t.lda = g.na; t.Zf = Zf; t.theta = theta; t.prob = prob; t.v0 = v0; t.Wt = Wt; t.params = params;
  } else {
    t.muA = g.muA; t.s2A = g.s2A; t.lda = g.lda; t.Zf = g.Zf; t.theta = g.theta; t.prob = g.prob; t.v0 = g.v0; t.Wt = g.Wt; t.params = g.util_params;
  }
  return t;
}

// ---------------------------------------------------------------------------------------------
// max_a v0(a; theta_l): one wave per parameter, lanes stride a
template <int MODE>
__global__ __launch_bounds__(64) void kg_v0_kernel(KgArgs g, double* __restrict__ v0_out) {
  const int l = blockIdx.x, lane = threadIdx.x;
  const double* th = g.theta + (long)l * g.theta_dim;
  double best = -INFINITY;
  int bi = 0x7fffffff;
  for (int a = lane; a < g.na; a += 64) {
    double mu[BOCF_MAX_M], s2[BOCF_MAX_M], A[BOCF_MAX_M], B[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) {
      mu[j] = j < g.m ? g.muA[(long)j * g.lda + a] : 0.0;
      s2[j] = j < g.m ? fmax(g.s2A[(long)j * g.lda + a], KG_CLIP) : 0.0;
      A[j] = 0.0;
      B[j] = 0.0;
    }
    const double v = kg_inner<MODE, false>(g.util_kind, th, g.util_params, mu, s2, g.m, g.Wt, g.S, A, B);
    if (v > best) {
      best = v;
      bi = a;
    }
  }
  kg_wave_argmax(best, bi);
  if (lane == 0) v0_out[l] = best;
}

void launch_kg_v0(const KgArgs& a, double* v0_out, hipStream_t s) {
  if (a.L <= 0) return;
  const dim3 grid((unsigned)a.L);
  if (a.mode == BOCF_EU_MEAN) BOCF_LAUNCH((kg_v0_kernel<BOCF_EU_MEAN>), grid, dim3(64), 0, s, a, v0_out);
  else if (a.mode == BOCF_EU_CLOSED) BOCF_LAUNCH((kg_v0_kernel<BOCF_EU_CLOSED>), grid, dim3(64), 0, s, a, v0_out);
  else BOCF_LAUNCH((kg_v0_kernel<BOCF_EU_MC>), grid, dim3(64), 0, s, a, v0_out);
}

// ---------------------------------------------------------------------------------------------
// One wave per candidate (four per workgroup, the layout of eu_kernel).  The wave holds 1 / s_j(x_c) in registers; for every parameter l
// and fantasy s the lanes stride the reference points a -- beta from the candidate's own row of Sigma, the conditioned mean and variance,
// the inner value -- keep their running maximum (a increasing: ties to the lowest a), and meet in a fixed butterfly.  The sums over s and l
// run in index order on wave-uniform values.  Nothing depends on the other candidates of the launch.
// (MC = the output count as a template argument, 1 ... 8, or 0 = read it from the arguments, as in eu_kernel)
template <int MODE, bool TAB, int MC>
__global__ __launch_bounds__(256) void kg_kernel(KgArgs g) {
  extern __shared__ double kg_lds[];
  const KgTables t = kg_tables<TAB>(g, kg_lds);
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= g.C) return;                          // wave-uniform (behind the workgroup barrier of the table load)
  const int m = MC > 0 ? MC : g.m;
  double is[BOCF_MAX_M];                         // 1 / s_j(x_c)
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) is[j] = j < m ? 1.0 / sqrt(fmax(g.s2c[(long)j * g.lds + c], 0.0) + g.nug[j]) : 0.0;
  const double* __restrict__ row = g.cov + (long)c * g.ldc;
  const double invSf = 1.0 / g.Sf;
  double total = 0.0;
  for (int l = 0; l < g.L; ++l) {
    const double* th = t.theta + (long)l * g.theta_dim;
    double acc = 0.0;
    for (int s = 0; s < g.Sf; ++s) {
      const double* z = t.Zf + (long)s * m;
      double best = -INFINITY;
      int bi = 0x7fffffff;
      for (int a = lane; a < g.na; a += 64) {
        double mu[BOCF_MAX_M], s2[BOCF_MAX_M], A[BOCF_MAX_M], B[BOCF_MAX_M];
#pragma unroll
        for (int j = 0; j < BOCF_MAX_M; ++j) {
          const double b = j < m ? row[(long)j * g.strideC + a] * is[j] : 0.0;
          mu[j] = j < m ? t.muA[(long)j * t.lda + a] + b * z[j] : 0.0;
          s2[j] = j < m ? fmax(t.s2A[(long)j * t.lda + a] - b * b, KG_CLIP) : 0.0;
          A[j] = 0.0;
          B[j] = 0.0;
        }
        const double v = kg_inner<MODE, false>(g.util_kind, th, t.params, mu, s2, m, t.Wt, g.S, A, B);
        if (v > best) {
          best = v;
          bi = a;
        }
      }
      kg_wave_argmax(best, bi);
      acc += best;
      if (g.astar && lane == 0) g.astar[((long)c * g.L + l) * g.Sf + s] = bi < g.na ? bi : 0;      // (no finite value at all: a* = 0)
    }
    total += t.prob[l] * (acc * invSf - t.v0[l]);
  }
  if (lane == 0) g.acq[c] = (g.accumulate ? g.acq[c] : 0.0) + total * g.scale;
}

template <int MODE, bool TAB>
static void launch_kg_m(const KgArgs& a, dim3 grid, size_t shm, hipStream_t s) {
#define LM(M) case M: BOCF_LAUNCH((kg_kernel<MODE, TAB, M>), grid, dim3(256), shm, s, a); return;
  switch (a.m) { LM(1) LM(2) LM(3) LM(4) LM(5) LM(6) LM(7) LM(8) default: break; }
#undef LM
  BOCF_LAUNCH((kg_kernel<MODE, TAB, 0>), grid, dim3(256), shm, s, a);
}

void launch_kg(const KgArgs& a, hipStream_t s) {
  if (a.C <= 0) return;
  const dim3 grid((unsigned)((a.C + 3) / 4));
  const size_t bytes = kg_table_bytes(a);
  const bool tab = bytes <= 65536;
#define KG(MODE)                                               \
  if (tab) launch_kg_m<MODE, true>(a, grid, bytes, s);         \
  else launch_kg_m<MODE, false>(a, grid, 0, s)
  if (a.mode == BOCF_EU_MEAN) { KG(BOCF_EU_MEAN); }
  else if (a.mode == BOCF_EU_CLOSED) { KG(BOCF_EU_CLOSED); }
  else { KG(BOCF_EU_MC); }
#undef KG
}

// ---------------------------------------------------------------------------------------------
// The partials A = dv/dmu, B = dv/dvar at the maximiser a* of every (candidate, parameter, fantasy) the value kernel recorded: one thread each.
// B is zero where the 1e-10 clip of the conditioned variance is active (the clip's derivative).
template <int MODE>
__global__ __launch_bounds__(256) void kg_partials_kernel(KgArgs g) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)g.C * g.L * g.Sf) return;
  const int s = (int)(e % g.Sf), l = (int)((e / g.Sf) % g.L), c = (int)(e / ((long)g.Sf * g.L));
  const int m = g.m, a = g.astar[e];
  const double* th = g.theta + (long)l * g.theta_dim;
  const double* z = g.Zf + (long)s * m;
  double mu[BOCF_MAX_M], s2[BOCF_MAX_M], A[BOCF_MAX_M], B[BOCF_MAX_M];
  unsigned clipped = 0;
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    double b = 0.0, raw = 0.0;
    if (j < m) {
      b = g.cov[(long)j * g.strideC + (long)c * g.ldc + a] * (1.0 / sqrt(fmax(g.s2c[(long)j * g.lds + c], 0.0) + g.nug[j]));
      raw = g.s2A[(long)j * g.lda + a] - b * b;
    }
    mu[j] = j < m ? g.muA[(long)j * g.lda + a] + b * z[j] : 0.0;
    s2[j] = j < m ? fmax(raw, KG_CLIP) : 0.0;
    clipped |= (raw > KG_CLIP ? 0u : 1u) << j;
    A[j] = 0.0;
    B[j] = 0.0;
  }
  (void)kg_inner<MODE, true>(g.util_kind, th, g.util_params, mu, s2, m, g.Wt, g.S, A, B);
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j)
    if (j < m) {
      g.AB[e * 2 * m + j] = A[j];
      g.AB[e * 2 * m + m + j] = ((clipped >> j) & 1u) ? 0.0 : B[j];
    }
}

void launch_kg_partials(const KgArgs& a, hipStream_t s) {
  const long n = (long)a.C * a.L * a.Sf;
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (a.mode == BOCF_EU_MEAN) BOCF_LAUNCH((kg_partials_kernel<BOCF_EU_MEAN>), grid, dim3(256), 0, s, a);
  else if (a.mode == BOCF_EU_CLOSED) BOCF_LAUNCH((kg_partials_kernel<BOCF_EU_CLOSED>), grid, dim3(256), 0, s, a);
  else BOCF_LAUNCH((kg_partials_kernel<BOCF_EU_MC>), grid, dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------------------------
// dKG/dx_cq = sum_l p_l (1/Sf) sum_s sum_j (A_j z_sj - 2 B_j beta_j) d beta_j(a*; x_c)/dx_q   (envelope rule: a* held fixed; v0 does not depend
// on x),  d beta_j/dx = dSigma_j(a*, x)/dx / s_j - Sigma_j(a*, x) dsigma^2_j(x)/dx / (2 s_j^3)  (the second term is zero where max(sigma^2, 0)
// is at its floor).  One thread per (candidate, coordinate), l, s, j in index order.
__global__ __launch_bounds__(256) void kg_grad_kernel(KgGradArgs g) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)g.C * g.d) return;
  const int c = (int)(idx / g.d), q = (int)(idx - (long)c * g.d);
  const int m = g.m;
  const double invSf = 1.0 / g.Sf;
  double total = 0.0;
  for (int l = 0; l < g.L; ++l) {
    double acc = 0.0;
    for (int s = 0; s < g.Sf; ++s) {
      const long e = ((long)c * g.L + l) * g.Sf + s;
      const int a = g.astar[e];
      for (int j = 0; j < m; ++j) {
        const double raw = g.s2c[(long)j * g.lds + c];
        const double s2 = fmax(raw, 0.0) + g.nug[j];
        const double is = 1.0 / sqrt(s2);
        const double cv = g.cov[(long)j * g.strideC + (long)c * g.ldc + a];
        const double b = cv * is;
        const double ds = raw > 0.0 ? g.ds2c[((long)j * g.ldg + c) * g.d + q] : 0.0;
        const double db = g.dcov[((((long)j * g.C + c) * g.na) + a) * g.d + q] * is - cv * ds * 0.5 * is / s2;
        acc += (g.AB[e * 2 * m + j] * g.Zf[(long)s * m + j] - 2.0 * g.AB[e * 2 * m + m + j] * b) * db;
      }
    }
    total += g.prob[l] * (acc * invSf);
  }
  g.dacq[idx] = (g.accumulate ? g.dacq[idx] : 0.0) + total * g.scale;
}

void launch_kg_grad(const KgGradArgs& a, hipStream_t s) {
  if (a.C <= 0 || a.d <= 0) return;
  BOCF_LAUNCH(kg_grad_kernel, dim3((unsigned)(((long)a.C * a.d + 255) / 256)), dim3(256), 0, s, a);
}
