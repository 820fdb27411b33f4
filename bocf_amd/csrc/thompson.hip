// Joint posterior over a candidate set and composite Thompson sampling (capi_thompson.hip drives them):
//   post_cov_f64_kernel   Sigma_j(X1, X2) = k_j(X1, X2) - V1^T V2 per output, V = R^T K(X, X.) (posterior.py:104-125)
//   post_diag_kernel      mean of diag(Sigma_j) over the valid candidates / jitter added to that diagonal
//   post_sample_kernel    F_j = mu_j + U_j^T Z_j, U_j the upper Cholesky factor of Sigma_j + jitter I
//   thompson_util_kernel  u(s, c) = U(theta_s, F[:, c, s]) with the acquisitions' utility_eval
// fp64 throughout.
#include "bocf_internal.h"
#include "kern_family.h"
#include "utility_dev.h"

typedef double v4d __attribute__((ext_vector_type(4)));
typedef double v2d __attribute__((ext_vector_type(2)));

#define TBM 128
#define TBK 16
#define TLDT 144   // padded LDS row (doubles): the bank property of gemm_f64.hip's LDT

// ---------------------------------------------------------------------------------------------
// Sigma tile (rt, ct) of output j: the tiling and register staging of gemm_tn_f64_kernel (128 x 128 tile per 4-wave workgroup, 64 x 64 per
// wave as 4 x 4 v_mfma_f64_16x16x4_f64 accumulators, BK = 16, tile t + 1 staged in VGPRs while tile t is multiplied out of LDS).  Both
// operands k-major: V1[kk][r] (ld1 columns), V2[kk][c] (ld2 columns), contraction over K rows.  The epilogue evaluates k_j(x1_r, x2_c) from
// the inputs divided by the lengthscales (the cross kernel's arithmetic) and stores k - acc: K(X1, X2) never reaches HBM.
// SYM: X1 = X2, only the tiles on / above the diagonal are launched (the ones the factorization reads), the padded diagonal is 1 and the
// rest of the padding 0 -- the layout launch_build_train_kernel gives S -- and jitter[j] (optional) is added to the valid diagonal.
// Not SYM: out-of-range entries are 0.
struct PostCovArgs {
  const double* V1; long ld1; long strideV1;
  const double* V2; long ld2; long strideV2;
  const double* X1; int n1;
  const double* X2; int n2;
  int d, K;
  const KernHyp* hyp;          // the launch's first output
  const double* jitter;        // SYM: per output, or nullptr
  double* out; long ldo; long strideO;
  int nrt, nct;
};

template <int KID, bool SYM>
__global__ __launch_bounds__(256, 2) void post_cov_f64_kernel(PostCovArgs g) {
  __shared__ double lds[2][2][TBK][TLDT];   // [buffer][A|B][k][m or n]   73,728 B
  int rt, ct;
  const int j = blockIdx.z;
  if constexpr (SYM) {
    int ut = blockIdx.x;                                     // tiles on / above the diagonal, row by row
    rt = 0;
    while (ut >= g.nct - rt) {
      ut -= g.nct - rt;
      ++rt;
    }
    ct = rt + ut;
  } else {
    rt = blockIdx.x / g.nct;
    ct = blockIdx.x - rt * g.nct;
  }
  const double* __restrict__ A = g.V1 + (long)j * g.strideV1 + (long)rt * TBM;
  const double* __restrict__ B = g.V2 + (long)j * g.strideV2 + (long)ct * TBM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, lq = lane >> 4;
  const int srow = tid >> 6, scol = (tid & 63) * 2;

  v4d acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[i][q] = (v4d){0.0, 0.0, 0.0, 0.0};

  v2d ra[4], rb[4];
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const v2d*>(A + (long)(kt + srow + 4 * i) * g.ld1 + scol);
      rb[i] = *reinterpret_cast<const v2d*>(B + (long)(kt + srow + 4 * i) * g.ld2 + scol);
    }
  };
  auto lstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<v2d*>(&lds[buf][0][srow + 4 * i][scol]) = ra[i];
      *reinterpret_cast<v2d*>(&lds[buf][1][srow + 4 * i][scol]) = rb[i];
    }
  };
  auto compute = [&](int cur) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int kq = ks * 4 + lq;
      double fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = lds[cur][0][kq][wr * 64 + i * 16 + l15];
#pragma unroll
      for (int q = 0; q < 4; ++q) fb[q] = lds[cur][1][kq][wc * 64 + q * 16 + l15];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[i][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[i], fb[q], acc[i][q], 0, 0, 0);
    }
  };
  if (g.K > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < g.K; kt += TBK) {
    const bool more = kt + TBK < g.K;
    if (more) gload(kt + TBK);
    compute(cur);
    if (more) lstore(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // epilogue: the tile's scaled inputs through the idle operand LDS, [coordinate][row] (a 16-lane group reads one row: broadcast; the
  // column side is lane-contiguous)
  const KernHyp& h = g.hyp[j];
  double* xs1 = &lds[0][0][0][0];                            // [d][128]
  double* xs2 = xs1 + BOCF_MAX_D * TBM;                      // [d][128]   (2 x 32 x 128 doubles = 64 KiB of the 72)
  for (int e = tid; e < g.d * TBM; e += 256) {
    const int q = e / TBM, r = e - q * TBM;
    const int r1 = rt * TBM + r, c2 = ct * TBM + r;
    xs1[q * TBM + r] = r1 < g.n1 ? g.X1[(long)r1 * g.d + q] / h.ls[q] : 0.0;
    xs2[q * TBM + r] = c2 < g.n2 ? g.X2[(long)c2 * g.d + q] / h.ls[q] : 0.0;
  }
  __syncthreads();
  double* O = g.out + (long)j * g.strideO;
  const double jit = SYM && g.jitter ? g.jitter[j] : 0.0;
  // accumulator layout of v_mfma_f64_16x16x4_f64: lane holds D[row = (lane >> 4) + 4 reg][col = lane & 15]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int rl = wr * 64 + i * 16 + lq + 4 * rg;
      const long r = (long)rt * TBM + rl;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int cl = wc * 64 + q * 16 + l15;
        const long c = (long)ct * TBM + cl;
        double v;
        if (r < g.n1 && c < g.n2) {
          double r2 = 0.0;
          for (int p = 0; p < g.d; ++p) {
            const double dq = xs1[p * TBM + rl] - xs2[p * TBM + cl];
            r2 += dq * dq;
          }
          v = kern_of_r2(KID, h.variance, r2) - acc[i][q][rg];
          if (SYM && r == c) v += jit;
        } else {
          v = SYM && r == c ? 1.0 : 0.0;
        }
        O[r * g.ldo + c] = v;
      }
    }
}

void launch_post_cov(const double* V1, long ld1, long strideV1, const double* V2, long ld2, long strideV2, const double* X1, int n1, const double* X2,
                     int n2, int d, int K, int kernel_id, const int* kids, const KernHyp* hyp, const double* jitter, int sym, double* out, long ldo,
                     long strideO, int m, hipStream_t s) {
  if (m <= 0 || n1 <= 0 || n2 <= 0) return;
  bocf_family_runs(kernel_id, kids, m, [&](int j0, int mr, int kid) {
    PostCovArgs g{};
    g.V1 = V1 + (long)j0 * strideV1; g.ld1 = ld1; g.strideV1 = strideV1;
    g.V2 = V2 + (long)j0 * strideV2; g.ld2 = ld2; g.strideV2 = strideV2;
    g.X1 = X1; g.n1 = n1; g.X2 = X2; g.n2 = n2; g.d = d; g.K = K;
    g.hyp = hyp + j0; g.jitter = jitter ? jitter + j0 : nullptr;
    g.out = out + (long)j0 * strideO; g.ldo = ldo; g.strideO = strideO;
    g.nrt = (n1 + TBM - 1) / TBM; g.nct = (n2 + TBM - 1) / TBM;
    const unsigned tiles = sym ? (unsigned)(g.nct * (g.nct + 1) / 2) : (unsigned)(g.nrt * g.nct);
    const dim3 grid(tiles, 1, (unsigned)mr);
    bocf_dispatch_family(kid, [&](auto Kc) {
      constexpr int KID = decltype(Kc)::value;
      if (sym) BOCF_LAUNCH((post_cov_f64_kernel<KID, true>), grid, dim3(256), 0, s, g);
      else BOCF_LAUNCH((post_cov_f64_kernel<KID, false>), grid, dim3(256), 0, s, g);
    });
  });
}

// ---------------------------------------------------------------------------------------------
// mode 0: mean[j] = mean of Sigma_j[i][i] over i < n (fixed order: per-thread strided sums, then a tree);  mode 1: Sigma_j[i][i] += jit[j]
__global__ __launch_bounds__(256) void post_diag_kernel(double* __restrict__ S, long ld, long strideS, int n, int mode, double* __restrict__ mean,
                                                        const double* __restrict__ jit) {
  const int j = blockIdx.x;
  double* Sj = S + (long)j * strideS;
  if (mode == 1) {
    const double a = jit[j];
    for (int i = threadIdx.x; i < n; i += 256) Sj[(long)i * ld + i] += a;
    return;
  }
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc += Sj[(long)i * ld + i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) mean[j] = red[0] / n;
}

void launch_post_diag(double* S, long ld, long strideS, int n, int mode, double* mean, const double* jit, int m, hipStream_t s) {
  if (m <= 0 || n <= 0) return;
  BOCF_LAUNCH(post_diag_kernel, dim3((unsigned)m), dim3(256), 0, s, S, ld, strideS, n, mode, mean, jit);
}

// ---------------------------------------------------------------------------------------------
// F_j[c][s] = mu_j[c] + sum_{k <= c} U_j[k][c] Z_j[k][s]   (U_j: upper factor, row-major ld; entries below the diagonal are never read)
// A workgroup owns 64 columns of U and ALL S sample columns: U is read from HBM once, whatever S is (the kernel is bound by that read:
// S <= 256 gives at most 512 flops per 8-byte element).  256 threads = 64 columns x 4 sample groups of SPT samples; 16 k-rows of U (the
// 64-column segment) and of Z (all S) are staged in LDS per step.  Per element the sum runs over k in increasing order.
#define SMP_COLS 64
#define SMP_K 16
template <int SPT>
__global__ __launch_bounds__(256) void post_sample_kernel(const double* __restrict__ U, long ldu, long strideU, const double* __restrict__ Z,
                                                          const double* __restrict__ mu, long ldmu, int C, int S, double* __restrict__ F) {
  __shared__ double zl[SMP_K][4 * SPT];
  __shared__ double ul[SMP_K][SMP_COLS];
  const int j = blockIdx.y;
  const int c0 = blockIdx.x * SMP_COLS;
  const int tid = threadIdx.x, cl = tid & 63, sg = tid >> 6;
  const int c = c0 + cl;
  const double* Uj = U + (long)j * strideU;
  const double* Zj = Z + (long)j * C * S;
  double acc[SPT];
#pragma unroll
  for (int t = 0; t < SPT; ++t) acc[t] = 0.0;
  int kend = c0 + SMP_COLS;
  if (kend > C) kend = C;
  for (int k0 = 0; k0 < kend; k0 += SMP_K) {
    for (int e = tid; e < SMP_K * SMP_COLS; e += 256) {
      const int kk = e / SMP_COLS, cc = e - kk * SMP_COLS;
      const int k = k0 + kk, col = c0 + cc;
      ul[kk][cc] = (k < C && col < C && k <= col) ? Uj[(long)k * ldu + col] : 0.0;
    }
    for (int e = tid; e < SMP_K * 4 * SPT; e += 256) {
      const int kk = e / (4 * SPT), ss = e - kk * (4 * SPT);
      const int k = k0 + kk;
      zl[kk][ss] = (k < C && ss < S) ? Zj[(long)k * S + ss] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SMP_K; ++kk) {
      const double u = ul[kk][cl];
#pragma unroll
      for (int t = 0; t < SPT; ++t) acc[t] = __builtin_fma(u, zl[kk][sg * SPT + t], acc[t]);
    }
    __syncthreads();
  }
  if (c >= C) return;
  const double m0 = mu[(long)j * ldmu + c];
  double* Fj = F + (long)j * C * S + (long)c * S;
#pragma unroll
  for (int t = 0; t < SPT; ++t) {
    const int s = sg * SPT + t;
    if (s < S) Fj[s] = m0 + acc[t];
  }
}

void launch_post_sample(const double* U, long ldu, long strideU, const double* Z, const double* mu, long ldmu, int C, int S, double* F, int m,
                        hipStream_t s) {
  if (m <= 0 || C <= 0 || S <= 0) return;
  const dim3 grid((unsigned)((C + SMP_COLS - 1) / SMP_COLS), (unsigned)m);
  const int spt = (S + 3) / 4;
#define PS(N) BOCF_LAUNCH((post_sample_kernel<N>), grid, dim3(256), 0, s, U, ldu, strideU, Z, mu, ldmu, C, S, F)
  if (spt <= 1) PS(1);
  else if (spt <= 2) PS(2);
  else if (spt <= 4) PS(4);
  else if (spt <= 8) PS(8);
  else if (spt <= 16) PS(16);
  else if (spt <= 32) PS(32);
  else PS(64);
#undef PS
}

// ---------------------------------------------------------------------------------------------
// u[s][c] = U(theta_s, F[:, c, s]) for the S paths of one sample block F (m, C, S); theta (S, theta_dim), u (S, ldu)
__global__ __launch_bounds__(256) void thompson_util_kernel(const double* __restrict__ F, int m, int C, int S, int util_kind,
                                                            const double* __restrict__ theta, int theta_dim, const double* __restrict__ params,
                                                            double* __restrict__ u, long ldu) {
  const int s = blockIdx.y;
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double y[BOCF_MAX_M];
#pragma unroll
  for (int q = 0; q < BOCF_MAX_M; ++q) y[q] = q < m ? F[((long)q * C + c) * S + s] : 0.0;
  u[(long)s * ldu + c] = utility_eval(util_kind, theta + (long)s * theta_dim, params, y, m);
}

void launch_thompson_util(const double* F, int m, int C, int S, int util_kind, const double* theta, int theta_dim, const double* params, double* u,
                          long ldu, hipStream_t s, const UtilProg* prog) {
  if (C <= 0 || S <= 0) return;
  if (util_kind == BOCF_UTIL_PROGRAM) {
    launch_thompson_util_prog(F, C, S, theta, theta_dim, u, ldu, *prog, s);
    return;
  }
  BOCF_LAUNCH(thompson_util_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)S), dim3(256), 0, s, F, m, C, S, util_kind, theta, theta_dim, params,
              u, ldu);
}
