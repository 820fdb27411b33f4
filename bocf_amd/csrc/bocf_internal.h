// Internal declarations shared by the HIP translation units of libbocf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kern_dispatch.h"     // BOCF_MAX_D (max input dimension), bocf_dispatch_d, bocf_dispatch_family, bocf_family_runs
#include "util_args.h"         // BOCF_MAX_M (max model outputs per hyper-sample), BOCF_MAX_L (max utility-parameter support size on device)

#define BOCF_TILE 128          // panel width NB == GEMM tile edge; every matrix is padded to it
#define BOCF_MAX_FITS 1024     // max independent factorizations in one fit (hyper-samples x outputs)

// Every kernel launch goes through BOCF_LAUNCH: the launch status (bad grid / block / shared-memory configuration) is read
// right behind the launch and the FIRST failure is remembered with the kernel's name; the C-ABI entry point that issued it
// reports it (bocf_last_error() names the kernel, not whichever call happened to synchronise next).
void bocf_note_launch(const char* kernel, hipError_t e);
#define BOCF_LAUNCH(kern, grid, block, shm, stream, ...)              \
  do {                                                                \
    hipLaunchKernelGGL(kern, grid, block, shm, stream, __VA_ARGS__);  \
    bocf_note_launch(#kern, hipGetLastError());                       \
  } while (0)
// bocf_dispatch_d behind a launcher: an input dimension that no instantiation covers is reported as a failed launch of `kernel`
template <typename F>
static inline void bocf_launch_by_d(const char* kernel, int d, F f) {
  if (!bocf_dispatch_d(d, f)) bocf_note_launch(kernel, hipErrorInvalidValue);
}

// s + c += a * b with the running sum carried as an unevaluated pair (s, c): TwoProd through fma, TwoSum (Knuth).  The posterior
// mean sum_k K(x*, X_k) alpha_k is a sum of N terms of size |alpha| ~ 1e6 (cond(Ky) ~ 4e9 at BASELINE configs[2]) that cancels to O(1):
// plain fp64 accumulation leaves 4e-8 absolute there, the pair 5e-9 (measured against oracle/truth_ld.c) -- below what the fp64
// rounding of K itself leaves.  (Contraction is switched off locally: fusing a * b into the following add would defeat TwoProd.)
__device__ __forceinline__ void dd_fma_acc(double& s, double& c, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  const double e = __builtin_fma(a, b, -p);
  const double t = s + p;
  const double z = t - s;
  c += ((s - (t - z)) + (p - z)) + e;
  s = t;
}
__device__ __forceinline__ void dd_add_acc(double& s, double& c, double hi, double lo) {
#pragma clang fp contract(off)
  const double t = s + hi;
  const double z = t - s;
  c += ((s - (t - z)) + (hi - z)) + lo;
  s = t;
}

// exp(x) for x <= 0 down to the underflow threshold: the operation sequence of the device library's double-precision exp (argument reduction
// by rint(x log2 e) with a two-part ln 2, degree-11 polynomial, ldexp) WITHOUT its two range selects (x > 1024 -> inf, x < -1075 -> 0):
// every covariance function of the path takes exp of -r^2/2, -sqrt(5) r or -sqrt(3) r.  Same operations on the same operands: the same bits
// as exp() on 2^30 arguments across [-745.2, 0] (tools/hbm_kernel_probe.hip) and 0 below -1075; 5 of the ~56 vector instructions per element
// of the K builds.  tests/test_gpu_extremes.py (test_ramp_train_kernel_through_the_subnormal_band) walks the K builds through the normal
// range, the subnormal band, true zero and the clamp against a long-double truth, entry by entry.
//
// bocf_exp_nonpos_times(x, a) = a exp(x) with ONE rounding into the subnormal range: the amplitude goes into the ldexp, a * ldexp(p, n)
// -> ldexp(a * p, n).  Wherever exp(x) is a normal number the two are the same bits (a power of two commutes with the rounding of the
// product); below, exp(x) alone keeps 52 - (-1022 - n) bits and a Matern amplitude (1 + u + 5/3 r2 ~ 1.9e5 at u = 745) multiplied that
// rounding error up: 9.1e4 subnormal ulps in K at l = 1e-3 (Matern52), 367 (Matern32), against <= 1 now.
__device__ __forceinline__ double bocf_exp_nonpos_times(double x, double a) {
  x = __builtin_fmax(x, -1100.0);                        // (far-apart points with tiny lengthscales: below -1075 the library returns 0, and so does ldexp here)
  const double dn = __builtin_rint(x * 0x1.71547652b82fep+0);
  const double t = __builtin_fma(-dn, 0x1.abc9e3b39803fp-56, __builtin_fma(-dn, 0x1.62e42fefa39efp-1, x));
  double p = __builtin_fma(t, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
  p = __builtin_fma(t, p, 0x1.71dee623fde64p-19);
  p = __builtin_fma(t, p, 0x1.a01997c89e6b0p-16);
  p = __builtin_fma(t, p, 0x1.a01a014761f6ep-13);
  p = __builtin_fma(t, p, 0x1.6c16c1852b7b0p-10);
  p = __builtin_fma(t, p, 0x1.1111111122322p-7);
  p = __builtin_fma(t, p, 0x1.55555555502a1p-5);
  p = __builtin_fma(t, p, 0x1.5555555555511p-3);
  p = __builtin_fma(t, p, 0x1.000000000000bp-1);
  p = __builtin_fma(t, p, 1.0);
  p = __builtin_fma(t, p, 1.0);
  return __builtin_ldexp(a * p, (int)dn);
}
__device__ __forceinline__ double bocf_exp_nonpos(double x) { return bocf_exp_nonpos_times(x, 1.0); }      // (1.0 * p is p: the same instructions as before)

// ---------------------------------------------------------------------------------------
// f64 MFMA GEMM (gemm_f64.hip):  C[r][c] = beta*Cin[r][c] + alpha * sum_kk A[kk][r] * B[kk][c]
// A and B are stored k-major (the contraction index is the slow one), C is row-major.
// Per-tile contraction length: kend = min(K, kb + krt*rt + kct*ct)  (rt/ct = tile row/col).
// ---------------------------------------------------------------------------------------
struct GemmArgs {
  const double* A;  long lda;  long strideA;   // batch stride (per blockIdx.z)
  const double* B;  long ldb;  long strideB;
  const double* Cin; double* Cout; long ldc; long strideC;
  int M, Ncols, K;             // multiples of 128 / 128 / 16
  int kb, krt, kct;            // per-tile contraction length rule
  int kbeg_rt, kbeg_ct;        // contraction starts at kbeg_rt * rt + kbeg_ct * ct (lower-triangular operands)
  int batch1;                  // blockIdx.z = z2 * batch1 + z1; second-level strides below (0 = unused)
  long strideA2, strideB2, strideC2;
  int upper_only;              // skip tiles with ct < rt (symmetric rank-k update)
  int rt_desc;                 // schedule heavy (large rt) tiles first
  int ct_desc;                 // idem for contraction lengths that grow with the column tile (kct > 0)
  int swizzle;                 // 0 plain order; 2 row-tile-major across the batch (heaviest rows first); 258 the 256-row variance kernel; probes build: 1, 100 + RT, 256, 257
  int batch;                   // set by the launcher
  int prefetch1;               // A/B switch: 1 = one-tile-deep staging in the sumsq variant
  int stagger;                 // probes build, two-buffer 256-row kernel: waves 4..7 store their operand share before the MFMAs
  int no_x3;                   // 1: never route a triangular store product to the three-buffer kernel (A/B, tests)
  int vprobe;                  // timing-only: the 256-row variance kernel also executes the VALU work of a fused K* tile build
  double alpha, beta;
  double* sumsq;               // epilogue 1: partial column sums of squares [batch][rt][Ncols]
  long strideSumsq;            // batch stride of sumsq
  int* tile_ctr;               // 256-row variance kernel: two zeroed device counters (next tile, workgroups done) -> one workgroup per compute unit
  int ncu;                     //   works through the tiles as a queue and leaves the counters zeroed; nullptr = one workgroup per tile
};
// epilogue 0: store C;  epilogue 1: write sumsq partials only (C is never stored)
void launch_gemm_f64(const GemmArgs& g, int batch, int epilogue, hipStream_t s);

// fp32 variance contraction (gemm_f32.hip): sum-of-squares epilogue only
struct GemmArgs32 {
  const float* A; long lda; long strideA;
  const float* B; long ldb; long strideB;
  int M, Ncols, K;
  double* sumsq; long strideSumsq;
  int tile128;                 // 1: always the 128-row kernel (option "swizzle" = 0: A/B, tests)
};
void launch_gemm_f32_sumsq(const GemmArgs32& g, int batch, hipStream_t s);
void launch_f64_to_f32(const double* src, float* dst, long n, hipStream_t s);

// ---------------------------------------------------------------------------------------
// fit kernels (fit.hip)
// ---------------------------------------------------------------------------------------
struct KernHyp {               // per-output hyper-parameters, device-resident array of these
  double variance;
  double noise;
  double ymean;
  double ls[BOCF_MAX_D];       // lengthscale_q (inputs are DIVIDED by it, as the reference does)
  double jitter;               // diagonal jitter of the current ladder attempt (read by the fused inference kernel only)
};

void launch_scale_inputs(const double* X, int n, int d, const KernHyp* hyp, int m, double* Xs, long strideXs, hipStream_t s);
// K(X,X) -> S (Np x Np per output, upper tiles), diag += noise + 1e-8 + jitter[j]; padding = identity
void launch_build_train_kernel(const double* Xs, long strideXs, int N, int Np, int d, int kernel_id, const KernHyp* hyp,
                               const double* jitter, int add_diag, double* S, long strideS, int m, hipStream_t s, const int* kids = nullptr);
// factor the p-th 128x128 diagonal block in place (upper, A = U^T U), write E = U^-1 and E^T
// one 128 x 128 tile per output, K = 128: C = beta C + alpha A^T B (A, B k-major), sixteen 32 x 32 pieces, a wave each
// (ntiles tiles side by side: B and C advance by 128 columns per tile, A is shared)
void launch_tile128(const double* A, long lda, long strideA, const double* B, long ldb, long strideB, double* C, long ldc, long strideC,
                    double alpha, double beta, int m, hipStream_t s, int ntiles = 1, int K = 128, int* done = nullptr);
#ifdef BOCF_PROBES
void dbg_tl_start();                     // debug timeline of the factorization's chain kernels (env BOCF_DBG_TL, probes build)
void dbg_tl_dump(const char* path);
#endif
void set_potrf_scalar(int on);   // 1: scalar diagonal-block kernel instead of the MFMA form (process-wide A/B switch)
// done (optional): device counter the kernel's workgroups add 1 to when their output is released (dependencies across streams)
void launch_potrf_diag(double* S, long strideS, int N, int Np, int p, double* E, double* ET, long strideE, int* info, int m, hipStream_t s,
                       int* done = nullptr);
// single-wave launch that polls up to two device counters until they reach n0 / n1 (bounded; *err = 1 on a timeout)
void launch_gate(const int* f0, int n0, const int* f1, int n1, int* err, hipStream_t s);
void launch_signal(int* f, int add, hipStream_t s);
// One-launch factorization + inverse of models with few panels (chol_team.hip): every output has a team of T resident workgroups
struct TeamArgs {
  double* S; double* RT; double* R; long strideS;   // upper factor (in: Ky, out: U), R^T (lower) and R (upper), Np x Np per output
  double* E; double* ET; long strideE;              // inverted diagonal blocks
  int N, Np, nb;
  int* info;                                        // per output: LAPACK-style info of the diagonal blocks
  int* F; int fstride;                              // per-output counters (chol_team_flag_words(nb) ints each, chol_plan.h), zeroed by the caller
  int* err;                                         // first wait that ran out of polls (0 = none)
  int T;                                            // workgroups per team (>= 2)
  int p0, p1;                                       // panels [p0, p1) of the factorization (the whole of it: 0, nb; do_inverse needs that)
  int do_inverse;
  double* KI; int do_kinv;                          // with do_inverse: also Ky^-1 = R R^T (upper tiles, Np x Np per output, stride strideS)
  int crit_load;                                    // the workgroups of the critical units carry nothing else while the others get by with <= this many units each
  int stream;                                       // a workgroup of the team streams the critical tiles underneath the diagonal blocks (team_crit_stream)
  unsigned long long* tl;                           // probes build: per-workgroup task timeline (nullptr = off)
};
void launch_chol_team(const TeamArgs& a, int m, hipStream_t s);
// whole inference (log-marginal + hyper-gradients) of a model with N <= 128, d <= 16 in one launch; yc has row stride 128
#define BOCF_INFER_MAX_D 16
// out: m rows of (2 + d gradients, log-marginal, info)
void launch_infer128(const double* X, int N, int d, int kernel_id, const KernHyp* hyp, const double* yc, double* out, int m, hipStream_t s,
                     const int* kids = nullptr);
// device-resident HMC chain of a small model (fit.hip hmc128_kernel): one workgroup per output runs the whole chain
struct HmcArgs {
  const double* X; int N, d; const double* yc;      // yc: (m, 128) centred targets
  double* theta; const int* fixed; int P, nls;      // theta (m, P) in/out: [variance, lengthscale (nls = 1 or d), noise]
  double prior_a, prior_b, prior_const;             // Gamma(a, b): lnpdf = const + (a - 1) log x - b x
  const double* mom; const double* uni;             // (m, ns, P) free entries packed in front; (m, ns)
  int ns, iters; double eps; int max_tries, raise_on_failure; double diag_shift;
  double* chains; int* accepted; int* diverged; int* status; long long* n_infer;
};
void launch_hmc128(const HmcArgs& a, int kernel_id, int m, hipStream_t s, const int* kids = nullptr);
// stream-resident HMC chain of larger models (hmc_stream.hip): the O(P) arithmetic between the inferences of the leapfrog steps
enum { HS_INIT = 0, HS_EVAL0 = 1, HS_PRE = 2, HS_POST = 3, HS_FINISH = 4 };
struct HmcStreamArgs {
  int m, P, nls, d, ns, iters;
  double eps, prior_a, prior_b, prior_const, diag_shift;
  const int* fixed;                                 // (m, P)
  const double* mom; const double* uni;             // (m, ns, P) free entries packed in front; (m, ns)
  double* state;                                    // hmc_stream_state_doubles(m)
  double* chains; int* accepted; int* diverged; long long* n_eval;
  int* abort_draw;                                  // -1, or the first draw the host has to run (jitter ladder / domain exit / schedule time-out)
  KernHyp* hyp;                                     // the hyper-parameters the inference's kernels read
  // the inference's own small launches folded into PRE / POST: inputs scaled by the lengthscales, zeroed schedule counters (PRE);
  // log-marginal from diag(U), alpha, yc and the reduction of the hyper-gradient partials (POST)
  const double* X; double* Xs; long strideXs; int N, Np;
  int* flags; int flag_words;                       // per-output counters of the team schedule (+ its time-out word behind them), or nullptr
  const double* S; long strideS; const double* alpha; const double* yc;
  const double* part; int nblk;                     // (m, nblk, 2 + d) partials of hypgrad_kernel: [dvariance, dnoise, dlengthscale ...]
  int* info; const int* sched_err;                  // per-output pivot status of the factorization; time-out word of its schedule (or nullptr)
  double* theta;                                    // (m, P) in / out
};
int hmc_stream_state_doubles(int m);
void launch_hmc_stream(const HmcStreamArgs& a, int mode, int i, int it, hipStream_t s);
// copy the diagonal 128x128 blocks [blk_lo, blk_hi) of E into the diagonal tiles of R
void launch_copy_diag_blocks(const double* E, long strideE, double* R, long strideR, int Np, int blk_lo, int blk_hi, int m, hipStream_t s);
// dst[(c0+c)][(r0+r)] = src[(r0+r)][(c0+c)] for a rows x cols block, `count` blocks spaced `step` along the diagonal
void launch_transpose_block(const double* src, double* dst, long stride, int Np, int r0, int c0, int rows, int cols, int count, int step,
                            int m, hipStream_t s);
// tiles on / above the diagonal of one Np x Np matrix <-> a contiguous buffer of nb (nb + 1) / 2 tiles (the exchange format of the sharded fit)
void launch_pack_upper_tiles(const double* R, int Np, double* packed, hipStream_t s);
void launch_unpack_upper_tiles(const double* packed, int Np, double* R, hipStream_t s);
// alpha = R t (t = R^T y comes from launch_gemv_small_t)
void launch_gemv_upper_n(const double* R, long strideR, int Np, const double* t, double* alpha, int m, hipStream_t s);
// loo.hip: leave-one-out mean / variance / log predictive density of every training point from R and alpha ((m, ld) each, first N columns;
// shift (m) = what the fit added to the diagonal besides the noise; flags = BOCF_ADD_NOISE / BOCF_CLIP as for a prediction), the sums of
// the densities over the points, and the parameter-index rows (L, N) of the expected-utility launches over those posteriors
void launch_loo(const double* R, long strideR, int N, int Np, const double* alpha, const double* yc, const KernHyp* hyp, const double* shift, int flags,
                double* mu, double* var, double* lpd, long ld, int m, hipStream_t s);
void launch_loo_sum(const double* lpd, long ld, int N, double* out, int m, hipStream_t s);
void launch_loo_rows(int* rows, int N, int L, hipStream_t s);
// Rank-1 append of one observation (row/column N of the padded factor; requires N < Np).  u = R^T k_new (Np),
// w = R u (Np), sumsq = ||u||^2 per output.  On a non-positive pivot fail[j] = 1 and nothing is written.
void launch_append_write(double* S, double* R, double* RT, long strideS, double* E, double* ET, long strideE, int Np, int N,
                         const double* u, const double* w, const double* sumsq, long ldsumsq, const KernHyp* hyp, int* fail, int m,
                         hipStream_t s);
// Removal of observation k (remove.hip): U' -> S (both halves), R' -> R, R^T, E, E^T through the T scratch (Np x Np per output), row / column
// N-1 back to identity padding.  coef: 2 Np doubles per output, part: 2 (Np / 128) Np doubles per output.
void launch_remove_factor(double* S, double* R, double* RT, double* T, long strideS, double* E, double* ET, long strideE, int Np, int N, int k,
                          double* coef, double* part, int m, hipStream_t s);
// rows k+1 .. N-1 of nblk row-major (rows, d) blocks (stride apart) move up by one; tmp: nblk (N - 1 - k) d doubles
void launch_remove_rows(double* buf, long stride, int nblk, int N, int k, int d, double* tmp, hipStream_t s);

// d lml / d (variance, lengthscale_q, noise) per output from alpha and Kinv (upper tiles valid):
// part: (m, nblocks, 2 + d) scratch; out: (m, 2 + d) = [dvariance, dnoise, dls_0 ... dls_{d-1}]
int hypgrad_num_blocks(int Np);
void launch_hypgrad(const double* Xs, long strideXs, int N, int Np, int d, int kernel_id, const KernHyp* hyp, const double* alpha,
                    const double* Kinv, long strideK, double* part, double* out, int m, hipStream_t s, const int* kids = nullptr, bool reduce = true);
void launch_lml(const double* S, long strideS, int N, int Np, const double* alpha, const double* yc, double* lml, int m, hipStream_t s);
// One step of iterative refinement of alpha = Ky^-1 yc with the residual in double-double (exact_gaussian_inference.py:51 solves once
// with dpotrs; at cond(Ky) ~ 4e9 that -- like R (R^T yc) here -- leaves ~4e-8 relative in alpha, the refined alpha 2e-9):
//   launch_kalpha_dd:   part[j][blk][0/1][i] = the pair (hi, lo) of sum_{k in 128-block blk} Ky[i][k] alpha[k], Ky rebuilt on the fly
//                       exactly as build_train_kernel stores it (diagonal = variance + (noise + 1e-8 + jitter))
//   launch_refine_rhs:  r[j][i] = yc[i] - sum_blk pairs      (rows >= N: 0)
//   (the caller solves delta = R (R^T r) with the GEMV kernels)
//   launch_refine_apply: alpha += delta;  mu_train[j][i] = yc[i] + ymean - dg alpha[i]   (K alpha = yc - dg alpha for the solution of
//                       (K + dg I) alpha = yc: the posterior mean at the training inputs, multi_outputGP.py:176-180, without another
//                       pass over K and without the cancellation of the direct sum)
void launch_kalpha_dd(const double* Xs, long strideXs, int N, int Np, int d, int kernel_id, const KernHyp* hyp, const double* jitter,
                      const double* alpha, double* part, int m, hipStream_t s, const int* kids = nullptr);
// int8 (Ozaki) form of the variance contraction (gemm_i8.hip, option "predict_i8"): digit fragments of R (per fit) and of K* (per chunk),
// exact int8 products, fp64 recombination, the per-128-row sums of squares of the fp64 kernels' layout
#define BOCF_I8_SLICES 6            // (the digit buffers are sized by i8_operand_bytes, predict_plan.h)
void launch_col_exponents(const double* R, long strideR, int Np, int* expo, int m, hipStream_t s);
// X[k][col] (k-major, leading dimension ld) -> fragments F; expo: per column (expo_stride = columns per matrix) or one per matrix (0)
void launch_slice_operand(const double* X, long ld, long strideX, int krows, int Np, int ncols, const int* expo, int expo_stride, void* F, int m,
                          hipStream_t s);
void launch_var_i8(const void* Af, const void* Bf, int Np, int ncols, const int* eA, const int* eB, double* sumsq, long strideSumsq, int m,
                   hipStream_t s, int group = 0);
int kalpha_block(int Np);                              // columns per partial sum of launch_kalpha_dd (part holds Np / that many pairs per row)
void launch_refine_rhs(const double* part, int N, int Np, const double* yc, double* r, int m, hipStream_t s);
void launch_refine_apply(const double* delta, int N, int Np, const KernHyp* hyp, const double* jitter, const double* yc, double* alpha,
                         double* mu_train, long ldmu, int m, hipStream_t s);

// ---------------------------------------------------------------------------------------
// predict kernels (predict.hip)
// ---------------------------------------------------------------------------------------
// cross kernel K*[j][kk][c] (Np x ldk per output; rows >= N zero) + partial means
void launch_cross_kernel(const double* Xs, long strideXs, int N, int Np, int d, int kernel_id, const KernHyp* hyp,
                         const double* Xc, int c0, int Cn, int Cpad, const double* alpha, double* Kstar, long ldk, long strideK,
                         double* meanpart, double* meanlo, int nsplit, int m, int store_k, hipStream_t s, const int* kids = nullptr);
// (meanpart / meanlo: the partial means per 128-row block as unevaluated pairs hi + lo, same layout each)
// store_k: 0 = mean only, 1 = K* as fp64, 2 = K* as fp32 (Kstar then points to float storage; ldk/strideK in elements)
void launch_finalize_mean(const double* meanpart, const double* meanlo, int nsplit, int Cpad, const KernHyp* hyp, double* mean, long ldmean, int c0,
                          int Cn, int m, hipStream_t s);
// (meanpart != nullptr: the same launch finishes the means too -- mean and var share ldvar)
void launch_finalize_var(const double* sumsq, int nrt, int Cpad, const KernHyp* hyp, int flags, double* var, long ldvar, int c0, int Cn, int m, hipStream_t s,
                         const double* meanpart = nullptr, const double* meanlo = nullptr, int nsplit = 0, double* mean = nullptr);
// column 0 of the predictive covariance from the mean-shaped pass t (see cov_column_kernel)
void launch_cov_column(const double* Xc, int C, int d, int kernel_id, const KernHyp* hyp, const double* t, long ldt, int flags, double* cov,
                       long ldcov, int m, hipStream_t s, const int* kids = nullptr);

// Low-latency path for n <= BOCF_SMALL_N candidates (single-point L-BFGS calls): GEMV-shaped, R read once.
#define BOCF_SMALL_N 16
// V[j][r][c] = sum_{kk<=r} R[kk][r] K*[kk][c]   (V: Np x nc per output, nc in {1,2,4,8,16}; K*: ldk columns)
void launch_gemv_small_t(const double* R, long strideR, int Np, const double* Kstar, long ldk, long strideK, double* V, int nc, int m, hipStream_t s);
// sumsq[j][c] = sum_r V[r][c]^2   (written as a single row-tile partial: nrt = 1, row length ldo)
void launch_sumsq_small(const double* V, int Np, double* sumsq, long ldo, int nc, int m, hipStream_t s);
// W[j][r][c] = sum_{kk>=r} R[r][kk] V[kk][c]   (W: Np x 16 per output)
void launch_gemv_small_n(const double* R, long strideR, int Np, const double* V, double* W, int nc, int m, hipStream_t s);
// the same three steps on the matrix pipe (predict.hip): K* + mean partials of <= 16 candidates; V = R^T K* with the column sums of squares per
// 16-row tile (sumsq[j][Np / 16][ldss]); W = R V from R^T
void launch_cross_small(const double* Xs, long strideXs, int N, int Np, int d, int kernel_id, const KernHyp* hyp, const double* Xc, int c0, int Cn, int nc,
                        const double* alpha, double* Kstar, long ldk, long strideK, double* meanpart, double* meanlo, int Cpad, int m, hipStream_t s,
                        const int* kids = nullptr);
void launch_gemv_small_t_mfma(const double* R, long strideR, int Np, const double* Kstar, long ldk, long strideK, double* V, double* sumsq, long ldss,
                              int nc, int m, hipStream_t s);
void launch_gemv_small_n_mfma(const double* RT, long strideR, int Np, const double* V, double* W, int nc, int m, hipStream_t s);

// d mean / dx and d var / dx of every candidate: (m, ldg, d) each.  W = Ky^-1 K(X, X*) (Np x ldw per output).
void launch_grad_kernel(const double* Xs, long strideXs, int N, int Np, int d, int kernel_id, const KernHyp* hyp, const double* Xc, int c0,
                        int Cn, const double* alpha, const double* W, long ldw, long strideW, double* dmean, double* dvar, long ldg,
                        int m, hipStream_t s, const int* kids = nullptr);

// ---------------------------------------------------------------------------------------
// utility programs (util_prog.hip; layout and limits: include/bocf_hip.h)
// ---------------------------------------------------------------------------------------
// The program resident on a context as the HOST sees it: the numbers of its validated header and the device copy of the blob.  The
// launchers below take it when the utility kind is BOCF_UTIL_PROGRAM and dispatch to the interpreter kernels.
struct UtilProg {
  const unsigned* dev = nullptr;     // device copy of the whole blob (nullptr: no program resident)
  int m = 0, theta_dim = 0, n_slots = 0, n_val = 0, n_grad = 0, n_const = 0;
  int val_out = 0;
  int grad_out[1 + BOCF_MAX_M] = {0};
};
// 0 when the blob is a valid program for m outputs and theta_dim parameters (m, theta_dim < 0: whatever its header states), else -1 with
// the offending field in bocf_last_error(); *out (optional) receives the header numbers (dev stays nullptr)
int util_prog_check(const char* who, const void* blob, long nbytes, int m, int theta_dim, UtilProg* out);
// threads per workgroup (64, 128 or 256) and bytes of dynamic LDS of a program launch: (m + slots) x threads x 8 bytes
void util_prog_geometry(const UtilProg& p, int* threads, size_t* lds_bytes);

// ---------------------------------------------------------------------------------------
// acquisition + selection kernels (acq.hip)
// ---------------------------------------------------------------------------------------
struct AcqArgs {
  const double* mean; const double* var; long ld;   // (m, ld), first C columns valid
  int m, C, L;
  int kind;                // BOCF_ACQ_*
  int util_kind;           // BOCF_UTIL_*
  int theta_dim;
  const double* theta;     // device (L, theta_dim)
  const double* prob;      // device (L) weights (already 1/L when the reference takes a plain mean)
  const double* best;      // device (L)
  const double* util_params; int n_util_params;
  const double* Wt; int S; // device (m, S) transposed normals
  double* acq;             // device (C)
  const double* dmean; const double* dvar; long ldg; int d;   // gradient variants: (m, ldg, d)
  double* dacq;            // device (C, d)
  int accumulate;          // 0: acq/dacq are written; 1: added to (hyper-sample h > 0 of the h-loop, maEI.py:85-97)
  double scale;            // 1 / H
  const UtilProg* prog;    // HOST pointer, read by the launchers only: the resident program when util_kind is BOCF_UTIL_PROGRAM
};
void launch_best_so_far(const double* mu_train, int N, int m, int linear, int util_kind, const double* theta, int theta_dim, int L,
                        const double* util_params, double* best, hipStream_t s, const UtilProg* prog = nullptr);
void launch_acq_linear(const AcqArgs& a, hipStream_t s);
void launch_acq_mc(const AcqArgs& a, hipStream_t s);
void launch_acq_linear_grad(const AcqArgs& a, hipStream_t s);
void launch_acq_mc_grad(const AcqArgs& a, hipStream_t s);
// ---------------------------------------------------------------------------------------
// expected utility of the recommendation step (eu.hip)
// ---------------------------------------------------------------------------------------
struct EuArgs {
  const double* mean; const double* var; long ld;   // (m, ld) rows of one hyper-sample, first C columns valid (var unused in MEAN mode)
  const double* dmean; const double* dvar; long ldg; int d;   // (m, ldg, d); read only when grad != nullptr
  int m, C;
  int mode;                // BOCF_EU_*
  int util_kind;           // BOCF_UTIL_*
  int theta_dim;
  const double* theta;     // device (L, theta_dim)
  const int* rows;         // device (C): parameter index of every candidate, in [0, L)
  const double* util_params;
  const double* Zt; int S; // device (L, m, S): transposed normals of every parameter (MC mode)
  double* val;             // device (C)
  double* grad;            // device (C, d) or nullptr (value only)
  int accumulate;          // 0: val/grad are written; 1: added to (hyper-sample h > 0)
  double scale;            // n_hyps with one resident hyper-sample, else 1
  const UtilProg* prog;    // HOST pointer, read by the launcher only: the resident program when util_kind is BOCF_UTIL_PROGRAM
};
void launch_eu(const EuArgs& a, hipStream_t s);
// the interpreter kernels behind the launchers above and launch_thompson_util (util_prog.hip): same geometry, same reduction order
void launch_best_so_far_prog(const double* mu_train, int N, const double* theta, int theta_dim, int L, double* best, const UtilProg& p, hipStream_t s);
void launch_acq_mc_prog(const AcqArgs& a, hipStream_t s);
void launch_acq_mc_grad_prog(const AcqArgs& a, hipStream_t s);
void launch_eu_prog(const EuArgs& a, hipStream_t s);
void launch_thompson_util_prog(const double* F, int C, int S, const double* theta, int theta_dim, double* u, long ldu, const UtilProg& p, hipStream_t s);
// two-stage top-k (value desc, index asc); out: idx (k) int64, val (k)
void launch_topk(const double* acq, int C, int k, long long* blk_idx, double* blk_val, long long* out_idx, double* out_val, hipStream_t s);
int topk_num_blocks(int C);
// device-resident anchor refinement (refine.hip; the step itself is refine_step.h).  init: fresh rows from the clamped resident candidates
// Xc (A, d) into zeroed state blocks, running = A.  advance: every running row consumes -acq / -dacq at its trial point and writes its next
// one (a stopped row its final x) into Xc; running is decremented once per row that stops.  d <= REFINE_MAX_D, one workgroup per row.
struct RefineSettings;
void launch_refine_init(double* Xc, double* dbl, int* ints, int* running, int A, const RefineSettings& s, hipStream_t st);
void launch_refine_advance(const double* acq, const double* dacq, double* Xc, double* dbl, int* ints, int* running, int A, const RefineSettings& s,
                           const double* lo, const double* hi, hipStream_t st, const double* acq2 = nullptr, const double* dacq2 = nullptr,
                           const int* map = nullptr, const int* small = nullptr);
// A > BOCF_SMALL_N: the first BOCF_SMALL_N running rows of Xc gathered in row order into x2 (BOCF_SMALL_N, d), map[row] = its column there
// (-1: stopped), *small = no more than BOCF_SMALL_N rows run; launch_refine_advance then reads acq2 / dacq2 (of x2) when *small
void launch_refine_compact(const double* Xc, const int* ints, int A, int d, double* x2, int* map, int* small, hipStream_t st);
#ifdef BOCF_PROBES
void launch_refine_poly(const double* Xc, int A, int d, double* acq, double* dacq, hipStream_t st);   // -f, -g of refine_poly.h at the rows
#endif
// multi-GPU selection: pack the k local winners (+ lo) into a 2 * world * k buffer of doubles; merge the gathered buffer
void launch_pack_topk(const long long* idx, const double* val, int k, long long lo, int world, int rank, double* pack, hipStream_t s);
void launch_merge_packed(const double* pack, int k, int world, long long* gidx, double* gval, long long* out_idx, double* out_val, hipStream_t s);

// ---------------------------------------------------------------------------------------
// joint posterior and composite Thompson sampling (thompson.hip)
// ---------------------------------------------------------------------------------------
// out[j][r][c] = k_j(x1_r, x2_c) - sum_{kk < K} V1[j][kk][r] V2[j][kk][c]  (V k-major, K a multiple of 16, ld1 / ld2 / ldo multiples of 128 covering
// n1 / n2).  sym: X1 = X2, tiles on / above the diagonal only, padded diagonal 1, jitter[j] (optional) added to the valid diagonal.
void launch_post_cov(const double* V1, long ld1, long strideV1, const double* V2, long ld2, long strideV2, const double* X1, int n1, const double* X2,
                     int n2, int d, int K, int kernel_id, const int* kids, const KernHyp* hyp, const double* jitter, int sym, double* out, long ldo,
                     long strideO, int m, hipStream_t s);
// mode 0: mean[j] = mean of the first n diagonal entries of S_j; mode 1: those entries += jit[j]
void launch_post_diag(double* S, long ld, long strideS, int n, int mode, double* mean, const double* jit, int m, hipStream_t s);
// F[j][c][s] = mu[j][c] + sum_{k <= c} U[j][k][c] Z[j][k][s]   (Z, F: (m, C, S) contiguous, S <= 256)
void launch_post_sample(const double* U, long ldu, long strideU, const double* Z, const double* mu, long ldmu, int C, int S, double* F, int m,
                        hipStream_t s);
// u[s][c] = U(theta_s, F[:, c, s]) (utility_dev.h) for one sample block F (m, C, S)
void launch_thompson_util(const double* F, int m, int C, int S, int util_kind, const double* theta, int theta_dim, const double* params, double* u,
                          long ldu, hipStream_t s, const UtilProg* prog = nullptr);

// ---------------------------------------------------------------------------------------
// pathwise posterior samples (paths.hip)
// ---------------------------------------------------------------------------------------
// out[j][c][s] = (add_mean ? ymean_j : 0) + sum_{i < N} k_j(x_c, X_i) v[j][i][s] + sum_{f < F} sqrt(2 s2_j / F) cos(omega_jf . x_c / l_j + b_jf) w[j][f][s]
// for the launch's m outputs, C points and S <= 64 paths; per point the sum runs over i ascending, then f ascending, whatever the batch.
struct PathValArgs {
  const double* Xs; long strideXs; int N;           // scaled training inputs (N, d) per output; N = 0: the feature part alone
  const double* v; long ldv; long strideV;          // (rows, ldv) per output, the first S columns read (nullptr with N = 0)
  const double* omega; const double* phase; const double* w; int F;   // (m, F, d), (m, F), (m, F, S) contiguous
  int S, nt;                                        // nt = ceil(S / 16): set by the launcher
  const KernHyp* hyp;
  const double* Xc; long strideXc; int prescaled;   // points (C, d): shared and divided by the lengthscales here, or (prescaled) per output and used as they are
  int C;
  double* out; long strideOut;                      // (C, S) per output
  int add_mean;
};
void launch_path_values(const PathValArgs& a, int d, int kernel_id, const int* kids, int m, hipStream_t s);
// rhs[j][i][s] = yc[j][i] - gX[j][i][s] - sqrt(nug_j) E[j][i][s] for i < N, s < S, zero elsewhere (Np x ld per output); gX, E: (m, N, S)
void launch_path_rhs(const double* yc, const double* gX, const double* E, const double* nug, int N, int Np, int S, int ld, double* rhs, int m, hipStream_t s);
// the resident paths of one hyper-sample as the small kernels see them (device pointers to its first output)
struct PathHyper {
  const double* omega; const double* phase; const double* w; const double* v;
  int F, S, p0, h;                                  // p0: global index of its first path
};
struct PathPointArgs {
  const double* Xs; long strideXs; int N, Np;       // of ALL outputs of the model
  const KernHyp* hyp; const int* kids; int kernel_id;   // kids: device array of the m kernel ids, or nullptr = kernel_id
  const PathHyper* tab; int nh;                     // device table of the hyper-samples with paths, p0 ascending
  int per; long ldv;
  const double* Xc; const int* row_path;            // (C, d) rows and their global path
  double* pv; double* pg;                           // (C, per) values (target mean included) and (C, per, d) input gradients
};
void launch_path_point(const PathPointArgs& a, int d, int C, hipStream_t s);
// val[c] = U(theta_{row_path[c]}, pv[c]) and (grad != nullptr) grad[c][q] = sum_j dU/dy_j pg[c][j][q]; theta rows tw wide
void launch_path_chain(const double* pv, const double* pg, int per, int d, int C, const int* row_path, int util_kind, const double* theta, int tw,
                       const double* params, double* val, double* grad, hipStream_t s, const UtilProg* prog = nullptr);
void launch_path_chain_prog(const double* pv, const double* pg, int d, int C, const int* row_path, const double* theta, int theta_dim, double* val,
                            double* grad, const UtilProg& p, hipStream_t s);

// ---------------------------------------------------------------------------------------
// look-ahead posterior and discrete composite knowledge gradient (kg.hip)
// ---------------------------------------------------------------------------------------
// out[j][c] = variance_j - sum_{kk < K} V[j][kk][c]^2 for c < n: the raw (noiseless, unclipped) posterior variance from V = R^T K(X, x_c)
void launch_kg_diag(const double* V, long ldv, long strideV, int K, int n, const KernHyp* hyp, double* out, long ldo, int m, hipStream_t s);
// out[j][c][a - a0][q] = d Sigma_j(a, x_c) / d x_cq for the Cn candidates Xc and the reference points a0 <= a < a0 + an of XA:
//   dk_j(x_c, a)/dx - sum_i dk_j(x_c, X_i)/dx Wa[j][i][a]   (gp.py:602-610), Wa = Ky^-1 K(X, A) (Np x ldw per output); i in increasing order
void launch_cov_grad(const double* Xs, long strideXs, int N, int d, int kernel_id, const int* kids, const KernHyp* hyp, const double* Xc, int Cn,
                     const double* XA, int a0, int an, const double* Wa, long ldw, long strideW, double* out, int m, hipStream_t s);
// conditioned on reference point q:  var[j][c] = s2c[j][c] - cov[j][c][q]^2 / s2(q),  s2(q) = max(s2A[j][q], 0) + nug[j]   (gp.py:543, raw);
// dvar[j][c][:] = ds2c[j][c][:] - 2 cov[j][c][q] dcov[j][c][:] / s2(q)  (dvar = nullptr: values only).  var (m, C), dvar (m, C, d) contiguous.
void launch_cond_var(const double* cov, long ldc, long strideC, int q, const double* s2c, long lds, const double* s2A, long lda, const double* nug,
                     const double* ds2c, long ldg, const double* dcov, int C, int d, double* var, double* dvar, int m, hipStream_t s);
struct KgArgs {
  const double* cov; int ldc; long strideC;         // Sigma_j(x_c, a): (m, rows, ldc) of one hyper-sample, C x na valid
  const double* s2c; int lds;                       // raw sigma^2_j(x_c): (m, lds)
  const double* nug;                                // (m): noise_j + 1e-8 + jitter_j
  const double* muA; const double* s2A; int lda;    // (m, lda): mu_j(a) and the raw sigma^2_j(a)
  const double* v0;                                 // (L): max_a v0(a; theta_l) of this hyper-sample (launch_kg_v0)
  const double* Zf; int Sf;                         // (Sf, m) fantasy normals
  const double* theta; int theta_dim; const double* prob; int L;
  const double* util_params;                        // (BOCF_MAX_M)
  const double* Wt; int S;                          // (m, S) transposed common random numbers (MC mode)
  int m, na, C, mode, util_kind;
  double* acq; int accumulate; double scale;        // (C): written, or added to (hyper-sample h > 0)
  int* astar; double* AB;                           // gradient form: the maximiser (C, L, Sf) and dv/dmu | dv/dvar at it (C, L, Sf, 2 m); else nullptr
};                                                  // (launch_kg writes astar, launch_kg_partials reads it and writes AB)
// bytes of LDS the tables of a launch need; the launcher keeps them in LDS when they fit in 64 KiB, else the kernel reads them from memory
size_t kg_table_bytes(const KgArgs& a);
void launch_kg(const KgArgs& a, hipStream_t s);
void launch_kg_v0(const KgArgs& a, double* v0_out, hipStream_t s);
void launch_kg_partials(const KgArgs& a, hipStream_t s);
struct KgGradArgs {
  const double* cov; long ldc; long strideC;        // as KgArgs
  const double* dcov;                               // (m, C, na, d)
  const double* s2c; long lds; const double* ds2c; long ldg;   // raw sigma^2_j(x_c) and its input gradient (m, ldg, d)
  const double* nug; const double* Zf; int Sf; const double* prob; int L;
  int m, na, C, d;
  const int* astar; const double* AB;
  double* dacq; int accumulate; double scale;       // (C, d)
};
void launch_kg_grad(const KgGradArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Monte-Carlo improvement of the composite utility conditioned on pending points (pending.hip)
// ---------------------------------------------------------------------------------------
// out = Sigma_j(P, P) of every output (m, r, r; from the padded tiles, row stride ldc) followed by mu_j(P) (m, r): one block for the one host copy
void launch_pending_pack(const double* cov, long ldc, long strideC, const double* mu, long ldmu, int r, double* out, int m, hipStream_t s);
struct PendArgs {
  const double* cov; int ldc; long strideC;         // Sigma_j(x_c, p_i): (m, rows, ldc) of one hyper-sample, C x r valid
  const double* s2c; const double* muc; int lds;    // raw sigma^2_j(x_c) and mu_j(x_c): (m, lds)
  const double* Q;                                  // (m, r, r): Sigma~_j^-1
  const double* F; const double* G;                 // (m, r, S): joint samples at the pending points and L^-T z, s fastest
  const double* Wt;                                 // (m, S) transposed common random numbers
  const double* best;                               // (L) best-so-far of this hyper-sample
  double* T;                                        // (L, S) thresholds of this hyper-sample (launch_pending_threshold writes, the others read)
  const double* theta; int theta_dim; const double* prob; int L;
  const double* util_params;                        // (BOCF_MAX_M)
  int m, r, S, C, util_kind;
  double* acq; int accumulate; double scale;        // (C): written, or added to (hyper-sample h > 0)
  // gradient form
  const double* dmu; const double* ds2; int ldg;    // d mu_j / dx, d sigma^2_j / dx: (m, ldg, d)
  const double* dcov;                               // d Sigma_j(x_c, p_i) / dx_c: (m, C, r, d)
  double* E;                                        // (C, m, S) scratch: every lane reads back what it wrote itself
  int d; double* dacq;                              // (C, d)
};
// bytes of LDS the tables of a value launch need (G, W, T, theta, prob, utility parameters); in LDS up to 64 KiB, else read from memory
size_t pending_table_bytes(const PendArgs& a);
void launch_pending_threshold(const PendArgs& a, hipStream_t s);
void launch_pending_acq(const PendArgs& a, hipStream_t s);
void launch_pending_grad(const PendArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------
// joint Monte-Carlo expected improvement of the composite utility at q-point batches (joint.hip; the factor is joint_chol.h)
// ---------------------------------------------------------------------------------------
struct JointArgs {
  const double* cov; int ldc; long strideC;         // Sigma_j between the points of the launch: (m, rows, ldc) of one hyper-sample; batch b is rows / columns b q .. b q + q - 1
  const double* mu; int ldm;                        // mu_j of the points: (m, ldm)
  const double* Zt;                                 // (m, q, S) transposed host normals, s fastest
  const double* best;                               // (L) incumbent of this hyper-sample
  const double* theta; int theta_dim; const double* prob; int L;
  const double* util_params;                        // (BOCF_MAX_M)
  int m, q, S, B, util_kind;
  double* acq; int* floored; int accumulate; double scale;   // (B) each (floored may be nullptr): written, or added to (hyper-sample h > 0)
  // gradient form
  const double* dmu; const double* ds2; int ldg;    // d mu_j / dx, d sigma^2_j / dx: (m, ldg, d)
  const double* dcov; int Cn;                       // d Sigma_j(x_c, x_a) / dx_c of all Cn = B q points: (m, Cn, Cn, d)
  double* E;                                        // (B, m, q, S) scratch: written and read inside one workgroup
  int d; double* dacq;                              // (B q, d)
};
void launch_joint_acq(const JointArgs& a, hipStream_t s);
void launch_joint_grad(const JointArgs& a, hipStream_t s);
void launch_joint_tail(double* acq, int B, int n, hipStream_t s);   // acq[B .. n) = -inf

// ---------------------------------------------------------------------------------------
// constrained Monte-Carlo expected improvement: linear output constraints inside the sample sum (cacq.hip)
// ---------------------------------------------------------------------------------------
#define BOCF_MAX_CONSTRAINTS 8
struct CacqArgs {
  const double* mean; const double* var; long ld;   // (m, ld) rows of one hyper-sample, first C columns valid
  const double* dmean; const double* dvar; long ldg; int d;   // gradient form: (m, ldg, d)
  int m, C, L, S, K;
  int util_kind, theta_dim;
  const double* theta; const double* prob;          // device (L, theta_dim), (L)
  const double* best; const long long* nfeas;       // device (L) feasible incumbent and |F| of this hyper-sample (launch_feasible_best)
  const double* util_params;                        // (BOCF_MAX_M)
  const double* Wt;                                 // (m, S) transposed common random numbers
  const double* tab;                                // A (K, m) | b (K) | 1 / eta (K)
  double* acq; double* dacq;                        // (C), (C, d)
  int accumulate; double scale;                     // written, or added to (hyper-sample h > 0); 1 / H
};
// best[l] = max over the training points with A mu - b <= 0 (every row) of U(theta_l, mu), -inf when there is none; nfeas[0] = their number
void launch_feasible_best(const double* mu_train, int N, int m, int util_kind, const double* theta, int theta_dim, int L, const double* util_params,
                          const double* tab, int K, double* best, long long* nfeas, hipStream_t s);
void launch_cacq(const CacqArgs& a, hipStream_t s);
void launch_cacq_grad(const CacqArgs& a, hipStream_t s);

// ---------------------------------------------------------------------------------------
// constrained expected utility of the recommendation step (ceu.hip): eu_kernel's Monte-Carlo form with every sample
// weighed by phi and an infeasible outcome worth u0 -- G = sum_s [u0 + phi (U - u0)], P = mean_s phi
// ---------------------------------------------------------------------------------------
struct CeuArgs {
  double* val; double* pof; double* grad;           // (C), (C), (C, d).  (First: with the outputs behind the inputs the compiler reserves a
                                                    // 36-byte stack frame it never touches for ceu_kernel<2, true> and <3, true>)
  const double* mean; const double* var; long ld;   // (m, ld) rows of one hyper-sample, first C columns valid
  const double* dmean; const double* dvar; long ldg; int d;   // gradient form: (m, ldg, d)
  int m, C, S, K;
  int util_kind, theta_dim;
  const double* theta; const double* u0;            // device (L, theta_dim), (L): the worth of an infeasible outcome per parameter
  const int* rows;                                  // device (C): parameter index of every candidate, in [0, L)
  const double* util_params;                        // (BOCF_MAX_M)
  const double* Zt;                                 // (L, m, S) transposed normals of every parameter (bocf_set_eu_samples)
  const double* tab;                                // A (K, m) | b (K) | 1 / eta (K)
  int accumulate;                                   // written, or added to (hyper-sample h > 0)
  double scale, pscale;                             // of G: n_hyps with one resident hyper-sample, else 1; of P: 1 / (n_h S)
};
void launch_ceu(const CeuArgs& a, bool grad, hipStream_t s);

// ---------------------------------------------------------------------------------------
// quantile / tail-mean acquisitions of the composite utility and the closed-form confidence bound (risk.hip)
// ---------------------------------------------------------------------------------------
struct RiskArgs {
  const double* mean; const double* var; long ld;   // (m, ld) rows of one hyper-sample, first C columns valid
  const double* dmean; const double* dvar; long ldg; int d;   // gradient form: (m, ldg, d)
  int m, C, L, S;
  int kind, rank;                                   // BOCF_RISK_*, the integer rank k in [0, S - 1]
  int util_kind, theta_dim;
  const double* theta; const double* prob;          // device (L, theta_dim), (L)
  const double* util_params;                        // (BOCF_MAX_M)
  const double* Wt;                                 // (m, S) transposed common random numbers
  double kappa;                                     // the closed form's exploration weight (launch_linear_ucb only)
  double* acq; double* dacq;                        // (C), (C, d)
  int accumulate; double scale;                     // written, or added to (hyper-sample h > 0); 1 / H
};
void launch_risk(const RiskArgs& a, bool grad, hipStream_t s);
void launch_linear_ucb(const RiskArgs& a, bool grad, hipStream_t s);
// min_out[l], max_out[l] = min / max over the N training points of U(theta_l, mu(X_i)): one workgroup per parameter, fixed order
void launch_train_utility_range(const double* mu_train, int N, int m, int util_kind, const double* theta, int theta_dim, int L, const double* util_params,
                                double* min_out, double* max_out, hipStream_t s);
