// Pathwise posterior samples (Matheron's rule with random Fourier features; capi_paths.hip drives them):
//   f_js(x) = ybar_j + sum_i k_j(x, X_i) v_js[i] + sum_f phi_jf(x) w_jfs,   phi_jf(x) = sqrt(2 s2_j / F) cos(omega_jf . x / l_j + b_jf)
//   path_values_kernel  the values of S paths per output at a batch of points: a matrix product whose left operand -- the covariance row,
//                       then the feature row, of every point -- is generated in registers and never stored
//   path_rhs_kernel     the right-hand side yc - g(X) - sqrt(nug) E of the staging solve
//   path_point_kernel   value and input gradient of ONE path per row (the few hundred rows of a refinement)
//   path_chain_kernel   the utility of a row's outputs and the chain rule (utility_dev.h)
// fp64 throughout; the device consumes no random numbers.
#include "bocf_internal.h"
#include "kern_family.h"
#include "utility_dev.h"

typedef double v4d __attribute__((ext_vector_type(4)));

// cos / sin of a feature's argument omega . x / l + b: the device library's (full-range argument reduction)
__device__ __forceinline__ double path_cos(double x) { return cos(x); }
__device__ __forceinline__ void path_sincos(double x, double* sn, double* cs) { *sn = sin(x); *cs = cos(x); }

#define PV_ROWS 64            // points per workgroup: four waves x one 16-row operand tile
#define PV_KB 32              // contraction rows (training points, then features) staged in LDS per step
#define PV_LDV 80             // LDS row of the right operand (doubles): 64 columns + 16, so the four rows of an instruction start 32 banks apart

// ---------------------------------------------------------------------------------------------
// out[j][c][s] = (ymean_j) + sum_{i < N} k_j(x_c, X_i) v[j][i][s] + sum_{f < F} phi_jf(x_c) w[j][f][s],  s < S <= 64.
// A wave owns 16 points and all S columns.  v_mfma_f64_16x16x4_f64 with the fragment layout of gemm_f64.hip: lane (l15, lq) supplies
// A[point l15][row lq] -- it FORMS that element, the covariance of its point (scaled coordinates in registers) with training row i0 + lq
// (coordinates out of LDS; the cross kernel's arithmetic: kern_of_r2_family), so the 64 lanes do 64 different
// exponentials per instruction and nothing is computed twice -- and B[row lq][column l15 + 16 t] out of the LDS copy of four rows of v.  One
// generated operand feeds nt = ceil(S / 16) <= 4 instructions.  The feature sum is the same loop with cos in place of the covariance value,
// omega in place of X and w in place of v, continuing the same accumulators.
// Per point the summation order is fixed: training rows ascending in groups of four (one instruction), then features likewise; rows and
// features past the end enter as exact zeros of the right operand.  It does not depend on the batch: a point's value is the same bits
// wherever it stands in whatever batch.  Workgroups are independent.
template <int D, int FAM>
__global__ __launch_bounds__(256) void path_values_kernel(PathValArgs g) {
  constexpr int XLD = D | 1;                                 // odd LDS row: the four rows an instruction reads fall into different banks
  __shared__ double xl[PV_KB][XLD];
  __shared__ double bl[PV_KB];
  __shared__ double vl[PV_KB][PV_LDV];
  const int j = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lq = lane >> 4;
  const int cbase = blockIdx.x * PV_ROWS + wave * 16;
  const KernHyp& h = g.hyp[j];
  const int nt = g.nt, ncol = 16 * nt;
  // this lane's point (clamped: lanes past the batch compute on the last point and store nothing)
  const long cme = cbase + l15 < g.C ? cbase + l15 : g.C - 1;
  double xc[D];
#pragma unroll
  for (int q = 0; q < D; ++q) xc[q] = g.prescaled ? g.Xc[(long)j * g.strideXc + cme * D + q] : g.Xc[cme * D + q] / h.ls[q];

  v4d acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (v4d){0.0, 0.0, 0.0, 0.0};

  const double variance = h.variance;
  // ---- sum_i k(x_c, X_i) v[i][s]
  {
    const double* __restrict__ X = g.Xs + (long)j * g.strideXs;
    const double* __restrict__ V = g.v + (long)j * g.strideV;
    for (int k0 = 0; k0 < g.N; k0 += PV_KB) {
      __syncthreads();
      for (int e = tid; e < PV_KB * D; e += 256) {
        const int r = e / D, q = e - r * D;
        xl[r][q] = k0 + r < g.N ? X[(long)(k0 + r) * D + q] : 0.0;
      }
      for (int e = tid; e < PV_KB * ncol; e += 256) {
        const int r = e / ncol, s = e - r * ncol;
        vl[r][s] = (k0 + r < g.N && s < g.S) ? V[(long)(k0 + r) * g.ldv + s] : 0.0;
      }
      __syncthreads();
      const int kn = g.N - k0 < PV_KB ? g.N - k0 : PV_KB;
      for (int kk = 0; kk < kn; kk += 4) {
        const int r = kk + lq;
        double r2 = 0.0;
#pragma unroll
        for (int q = 0; q < D; ++q) {
          const double dq = xl[r][q] - xc[q];
          r2 += dq * dq;
        }
        const double a = kern_of_r2_family<FAM>(variance, r2);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vl[r][16 * t + l15], acc[t], 0, 0, 0);
      }
    }
  }
  // ---- sum_f phi_f(x_c) w[f][s]
  {
    const double amp = sqrt(2.0 * variance / (double)(g.F > 0 ? g.F : 1));
    const double* __restrict__ Om = g.omega + (long)j * g.F * D;
    const double* __restrict__ Ph = g.phase + (long)j * g.F;
    const double* __restrict__ W = g.w + (long)j * g.F * g.S;
    for (int k0 = 0; k0 < g.F; k0 += PV_KB) {
      __syncthreads();
      for (int e = tid; e < PV_KB * D; e += 256) {
        const int r = e / D, q = e - r * D;
        xl[r][q] = k0 + r < g.F ? Om[(long)(k0 + r) * D + q] : 0.0;
      }
      if (tid < PV_KB) bl[tid] = k0 + tid < g.F ? Ph[k0 + tid] : 0.0;
      for (int e = tid; e < PV_KB * ncol; e += 256) {
        const int r = e / ncol, s = e - r * ncol;
        vl[r][s] = (k0 + r < g.F && s < g.S) ? W[(long)(k0 + r) * g.S + s] : 0.0;
      }
      __syncthreads();
      const int kn = g.F - k0 < PV_KB ? g.F - k0 : PV_KB;
      for (int kk = 0; kk < kn; kk += 4) {
        const int r = kk + lq;
        double arg = bl[r];
#pragma unroll
        for (int q = 0; q < D; ++q) arg = __builtin_fma(xl[r][q], xc[q], arg);
        const double a = amp * path_cos(arg);
#pragma unroll
        for (int t = 0; t < 4; ++t)
          if (t < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vl[r][16 * t + l15], acc[t], 0, 0, 0);
      }
    }
  }
  // accumulator layout: lane holds D[point = (lane >> 4) + 4 reg][column = lane & 15]
  const double add = g.add_mean ? h.ymean : 0.0;
  double* __restrict__ O = g.out + (long)j * g.strideOut;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (t < nt) {
      const int s = 16 * t + l15;
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        const long c = cbase + lq + 4 * rg;
        if (c < g.C && s < g.S) O[c * g.S + s] = acc[t][rg] + add;
      }
    }
}

void launch_path_values(const PathValArgs& a, int d, int kernel_id, const int* kids, int m, hipStream_t s) {
  if (m <= 0 || a.C <= 0 || a.S <= 0) return;
  bocf_family_runs(kernel_id, kids, m, [&](int j0, int mr, int kid) {
    PathValArgs g = a;
    g.Xs = a.Xs + (long)j0 * a.strideXs;
    g.v = a.v ? a.v + (long)j0 * a.strideV : nullptr;
    g.omega = a.omega + (long)j0 * a.F * d; g.phase = a.phase + (long)j0 * a.F; g.w = a.w + (long)j0 * a.F * a.S;
    g.hyp = a.hyp + j0;
    if (a.prescaled) g.Xc = a.Xc + (long)j0 * a.strideXc;
    g.out = a.out + (long)j0 * a.strideOut;
    g.nt = (a.S + 15) / 16;
    const dim3 grid((unsigned)((a.C + PV_ROWS - 1) / PV_ROWS), (unsigned)mr);
    bocf_launch_by_d("path_values_kernel", d, [&](auto Dc) {
      bocf_dispatch_family(kid, [&](auto Kc) {
        constexpr int D = decltype(Dc)::value, FAM = decltype(Kc)::value;
        BOCF_LAUNCH((path_values_kernel<D, FAM>), grid, dim3(256), 0, s, g);
      });
    });
  });
}

// ---------------------------------------------------------------------------------------------
// rhs[j][i][s] = yc[j][i] - g[j][i][s] - sqrt(nug_j) E[j][i][s]  (i < N, s < S), zero elsewhere: Np x ld per output, the right-hand sides
// of the staging solve in the layout launch_gemm_f64 takes for its B operand
__global__ __launch_bounds__(256) void path_rhs_kernel(const double* __restrict__ yc, const double* __restrict__ gX, const double* __restrict__ E,
                                                       const double* __restrict__ nug, int N, int Np, int S, int ld, double* __restrict__ rhs) {
  const int j = blockIdx.y;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)Np * ld) return;
  const int i = (int)(e / ld), s = (int)(e - (long)i * ld);
  double v = 0.0;
  if (i < N && s < S) v = yc[(long)j * Np + i] - gX[((long)j * N + i) * S + s] - sqrt(nug[j]) * E[((long)j * N + i) * S + s];
  rhs[(long)j * Np * ld + e] = v;
}

void launch_path_rhs(const double* yc, const double* gX, const double* E, const double* nug, int N, int Np, int S, int ld, double* rhs, int m, hipStream_t s) {
  if (m <= 0) return;
  const long n = (long)Np * ld;
  BOCF_LAUNCH(path_rhs_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)m), dim3(256), 0, s, yc, gX, E, nug, N, Np, S, ld, rhs);
}

// ---------------------------------------------------------------------------------------------
// Value and input gradient of one path per row: row c evaluates global path row_path[c] = (hyper-sample h, path s of it) and this
// workgroup its output jj of that hyper-sample.
//   val   = ymean + sum_i k(x, X_i) v_i + sum_f amp cos(a_f) w_f,               a_f = omega_f . x / l + b_f
//   d/dx_q = [ sum_i kern_dfac(r_i) (x_q - X_iq) / l_q v_i  -  sum_f amp sin(a_f) omega_fq w_f ] / l_q      (kern_dfac = -f, kern_family.h)
// Threads stride the training rows, then the features; the partial sums meet in the fixed butterfly and wave order of grad_kernel.
template <int D>
__global__ __launch_bounds__(256) void path_point_kernel(PathPointArgs g) {
  const int c = blockIdx.x, jj = blockIdx.y;
  const int p = g.row_path[c];
  int hi = 0;
  while (hi + 1 < g.nh && p >= g.tab[hi + 1].p0) ++hi;       // (tab is ordered by p0; the entry point checked 0 <= p < P)
  const PathHyper T = g.tab[hi];
  const int s = p - T.p0;
  const int j = T.h * g.per + jj;
  const KernHyp& h = g.hyp[j];
  const int kid = g.kids ? g.kids[j] : g.kernel_id;
  double xc[D], gr[D];
#pragma unroll
  for (int q = 0; q < D; ++q) {
    xc[q] = g.Xc[(long)c * D + q] / h.ls[q];
    gr[q] = 0.0;
  }
  double val = 0.0;
  const double* __restrict__ X = g.Xs + (long)j * g.strideXs;
  const double* __restrict__ V = T.v + (long)jj * g.Np * g.ldv;
  for (int i = threadIdx.x; i < g.N; i += 256) {
    double df[D];
    double r2 = 0.0;
#pragma unroll
    for (int q = 0; q < D; ++q) {
      df[q] = xc[q] - X[(long)i * D + q];
      r2 += df[q] * df[q];
    }
    const double vi = V[(long)i * g.ldv + s];
    val += kern_of_r2(kid, h.variance, r2) * vi;
    const double cf = kern_dfac(kid, h.variance, r2) * vi;
#pragma unroll
    for (int q = 0; q < D; ++q) gr[q] += cf * df[q];
  }
  const double amp = sqrt(2.0 * h.variance / (double)T.F);
  const double* __restrict__ Om = T.omega + (long)jj * T.F * D;
  const double* __restrict__ Ph = T.phase + (long)jj * T.F;
  const double* __restrict__ W = T.w + (long)jj * T.F * T.S;
  for (int f = threadIdx.x; f < T.F; f += 256) {
    double arg = Ph[f];
#pragma unroll
    for (int q = 0; q < D; ++q) arg = __builtin_fma(Om[(long)f * D + q], xc[q], arg);
    const double wf = amp * W[(long)f * T.S + s];
    double sn, cs;
    path_sincos(arg, &sn, &cs);
    val += cs * wf;
    const double sf = -sn * wf;
#pragma unroll
    for (int q = 0; q < D; ++q) gr[q] += sf * Om[(long)f * D + q];
  }
  __shared__ double red[4][D + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q <= D; ++q) {
    double a = q < D ? gr[q < D ? q : 0] : val;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) red[w][q] = a;
  }
  __syncthreads();
  if (threadIdx.x <= D) {
    const int q = threadIdx.x;
    const double t = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
    if (q < D) g.pg[((long)c * g.per + jj) * D + q] = t / h.ls[q];
    else g.pv[(long)c * g.per + jj] = t + h.ymean;
  }
}

void launch_path_point(const PathPointArgs& a, int d, int C, hipStream_t s) {
  if (C <= 0) return;
  bocf_launch_by_d("path_point_kernel", d, [&](auto Dc) {
    constexpr int D = decltype(Dc)::value;
    BOCF_LAUNCH(path_point_kernel<D>, dim3((unsigned)C, (unsigned)a.per), dim3(256), 0, s, a);
  });
}

// ---------------------------------------------------------------------------------------------
// u_c = U(theta_{p[c]}, y_c) and du_c/dx = sum_j dU/dy_j dy_cj/dx from the values pv (C, per) and gradients pg (C, per, d): a thread per row
__global__ __launch_bounds__(256) void path_chain_kernel(const double* __restrict__ pv, const double* __restrict__ pg, int per, int d, int C,
                                                         const int* __restrict__ row_path, int util_kind, const double* __restrict__ theta, int tw,
                                                         const double* __restrict__ params, double* __restrict__ val, double* __restrict__ grad) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double y[BOCF_MAX_M], gy[BOCF_MAX_M];
#pragma unroll
  for (int q = 0; q < BOCF_MAX_M; ++q) y[q] = q < per ? pv[(long)c * per + q] : 0.0;
  const double* th = theta + (long)row_path[c] * tw;
  val[c] = utility_eval(util_kind, th, params, y, per);
  if (!grad) return;
  utility_grad(util_kind, th, params, y, per, gy);
  for (int q = 0; q < d; ++q) {
    double t = 0.0;
#pragma unroll
    for (int jj = 0; jj < BOCF_MAX_M; ++jj)
      if (jj < per) t += gy[jj] * pg[((long)c * per + jj) * d + q];
    grad[(long)c * d + q] = t;
  }
}

void launch_path_chain(const double* pv, const double* pg, int per, int d, int C, const int* row_path, int util_kind, const double* theta, int tw,
                       const double* params, double* val, double* grad, hipStream_t s, const UtilProg* prog) {
  if (C <= 0) return;
  if (util_kind == BOCF_UTIL_PROGRAM) {
    launch_path_chain_prog(pv, pg, d, C, row_path, theta, tw, val, grad, *prog, s);
    return;
  }
  BOCF_LAUNCH(path_chain_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, pv, pg, per, d, C, row_path, util_kind, theta, tw, params, val, grad);
}
