/*
 * bocf_hip.h -- C ABI of libbocf_hip.so: MI355X (gfx950) implementation of BOCF's
 * GP-posterior + composite-acquisition hot path.
 *
 * The reference (RaulAstudillo06/BOCF) has NO native boundary on this path: it is pure
 * Python over SciPy LAPACK.  This header is the FFI a maintainer binds with ctypes
 * underneath the reference's two plug-in surfaces (multi_outputGP.py:9-349 and
 * GPyOpt/acquisitions/base.py:5-74); INTEGRATION.md shows that binding.  Every entry
 * point names the reference code it replaces (paths relative to the reference root).
 *
 * Conventions: plain C, caller-owned HOST buffers unless a name says "device", row-major
 * float64, no alignment requirement.  Return 0 = ok; >0 = LAPACK-style info (1-based index
 * of the first non-positive Cholesky pivot); <0 = HIP/runtime/argument error (text via
 * bocf_last_error()).  A context owns its device memory and one HIP stream, is bound to one
 * GPU, is NOT thread-safe, and every call is synchronous on return unless stated otherwise.
 */
#ifndef BOCF_HIP_H
#define BOCF_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bocf_ctx bocf_ctx;

/* kernel ids: GPy/kern/src/rbf.py:42-43 (RBF) and GPy/kern/src/se.py:44-62 (SE, the GPModel
 * default, gpmodel.py:58) share sigma^2 exp(-r^2/2); Matern52 stationary.py:529-530;
 * Matern32 stationary.py:440-441.  Distances use direct differences of the inputs divided
 * by the lengthscale (se.py:65-93 convention). */
enum { BOCF_KERN_RBF = 0, BOCF_KERN_SE = 1, BOCF_KERN_MATERN52 = 2, BOCF_KERN_MATERN32 = 3 };

/* predict flags */
enum { BOCF_ADD_NOISE = 1,   /* + sigma_n^2: GP.predict gp.py:316-320 / posterior_variance gp.py:416-417 */
       BOCF_CLIP = 2 };      /* clip variance to [1e-10, inf): GPyOpt/models/gpmodel.py:147,174,183 */

/* acquisition kinds */
enum { BOCF_ACQ_EI = 0,      /* maEI.py:96 / uEI_noiseless.py:80 */
       BOCF_ACQ_PI = 1 };    /* maPI.py:91-92 / uPI.py:83 (jitter 1e-6) */

/* device utility functions U(theta, y), y in R^m -- the closed set the reference's experiment
 * scripts use, compiled in (any other straight-line callable runs as a utility PROGRAM, below):
 *   LINEAR       theta . y                              test_1b.py:89-90     theta_dim = m
 *   NEG_SQ_DIST  -sum_j (y_j - theta_j)^2               test_1a.py:89-92     theta_dim = m
 *   NEG_SUM_EXP  -sum_j exp(y_j)                        test_2a.py:60-62     theta unused
 *   NEG_EXP_COS  -sum_j c_j e^{-y_j/pi} cos(pi y_j)     test_3a.py:52-57     util_params = c (m)
 *   ROSENBROCK   -sum_{j<m/2} (a-y_j)^2 + 100 y_{j+m/2}^2   test_5a.py:48-52  a = theta[0] */
enum { BOCF_UTIL_LINEAR = 0, BOCF_UTIL_NEG_SQ_DIST = 1, BOCF_UTIL_NEG_SUM_EXP = 2,
       BOCF_UTIL_NEG_EXP_COS = 3, BOCF_UTIL_ROSENBROCK = 4,
       BOCF_UTIL_PROGRAM = 5 };  /* the utility program resident on the context, see below */

/* ---- utility programs: a user's own U(theta, y) on the device without recompiling.  The host traces the user's callable into a
 * STRAIGHT-LINE program (bocf_amd/utility_program.py: no branches, no loops; dU/dy is derived at trace time and is ordinary program
 * output), the device interprets it inside the Monte-Carlo kernels (util_prog.hip).  With util_kind = BOCF_UTIL_PROGRAM the Monte-Carlo
 * acquisitions, the Monte-Carlo expected utility and the Thompson selection evaluate the program staged on the context; n_util_params
 * must be 0 and theta_dim and the outputs per hyper-sample must be those the program was built for.  The closed-form expected utility and
 * the knowledge gradient do not take it.  Non-finite utility values are the caller's responsibility: the program computes what its
 * arithmetic gives (log of a negative number, a division by zero ...), nothing is trapped or replaced.
 *
 * The blob (little endian, 8-byte units):
 *   header  32 x uint32:  [0] magic BOCF_PROG_MAGIC  [1] version BOCF_PROG_VERSION  [2] m  [3] theta_dim  [4] slots  [5] instructions of the
 *           value section  [6] instructions of the value+gradient section  [7] constants  [8] slot of U after the value section
 *           [9] slot of U and [10 + j] slot of dU/dy_j (j < m) after the value+gradient section; the remaining words are 0
 *   value section, then value+gradient section: one instruction = 2 x uint32
 *           word 0 = opcode | destination slot << 8,   word 1 = operand a | operand b << 16   (a unary operation repeats a as b)
 *           operand = kind << 14 | index:  kind 0 slot, 1 input y_index, 2 parameter theta_index, 3 constant-pool entry
 *   constant pool: float64 each
 * total 128 + 8 (instructions + constants) bytes.  Each section starts with every slot unwritten, runs its instructions in order and leaves
 * its outputs in the slots the header names.  The arithmetic is IEEE double without contraction, one operation per instruction. */
#define BOCF_PROG_MAGIC 0x47505542u
#define BOCF_PROG_VERSION 1
#define BOCF_PROG_HEADER_WORDS 32
#define BOCF_PROG_MAX_INSTR 1024   /* instructions per section */
#define BOCF_PROG_MAX_SLOTS 64     /* per-sample value slots (the device keeps them in LDS) */
#define BOCF_PROG_MAX_CONSTS 256   /* constant-pool entries */
enum { BOCF_OP_ADD = 0, BOCF_OP_SUB, BOCF_OP_MUL, BOCF_OP_DIV, BOCF_OP_NEG, BOCF_OP_ABS, BOCF_OP_SIGN, BOCF_OP_SQRT, BOCF_OP_EXP, BOCF_OP_LOG,
       BOCF_OP_SIN, BOCF_OP_COS, BOCF_OP_TANH, BOCF_OP_POW, BOCF_OP_MIN, BOCF_OP_MAX,
       BOCF_OP_GE,               /* a >= b ? 1.0 : 0.0 */
       BOCF_OP_COUNT };
enum { BOCF_OPERAND_SLOT = 0, BOCF_OPERAND_INPUT = 1, BOCF_OPERAND_PARAM = 2, BOCF_OPERAND_CONST = 3 };

int bocf_version(void);
const char* bocf_last_error(void);

/* Create / destroy a context on HIP device `device`. */
int bocf_create(int device, bocf_ctx** out);
void bocf_destroy(bocf_ctx* ctx);

/* Options (bocf_option_info enumerates the table: name, range, kind; kind 0 = speed only, kind 1 = semantics the caller asks for).
 * Sizes / plumbing:
 *   "chunk" = max candidates per pass (multiple of 128; default 65536), "workspace_mb" = cap of the per-pass K* workspace (default
 *   24576; the chunk is lowered to fit), "profile" = 1 records HIP events around the dominant (variance-GEMM) kernel and the named phases,
 *   "small_path" = 0 disables the GEMV-shaped path for <= 16 candidates, "prefetch1".
 * Semantics (kind 1):
 *   "predict_f32" = 1 runs the O(N^2 C) variance contraction in fp32 (K* and the inverse factor rounded to fp32, fp32 MFMA; fit, mean and
 *     gradients stay fp64) -- the arithmetic BASELINE configs[4] names,
 *   "reuse_data" = 1: the following bocf_fit calls use the X / Y of the previous fit (same N, d, m; the pointers are ignored) and upload
 *     only the hyper-parameters; "skip_mu_train" = 1: bocf_fit does not refresh the posterior mean at the training inputs -- both for
 *     the thousands of inferences of a hyper-parameter update (optimise + HMC), which read only the log-marginal and its gradients;
 *     reset both to 0 before the fit that serves predictions,
 *   "hyper_samples" = H (default 1): the m outputs given to bocf_fit are H hyper-samples x m/H model outputs, hyper-sample-major -- the
 *     model_instances of GPModel (gpmodel.py:80-96, one kernel/noise setting per HMC draw).  The acquisition entry points then run the
 *     reference's h-loop (maEI.py:85-97, uEI_noiseless.py:71-82) on the device: theta/W refer to the m/H model outputs, every
 *     hyper-sample adds 1/H of its marginal,
 *   "acq_hyper_samples" = n (default 0 = all): the acquisitions average over the first n hyper-samples only (n_hyps_samples =
 *     min(10, number_of_hyps_samples()), maEI.py:35),
 *   "best_group" = -1 (default): hyper-sample h uses its own best-so-far (maEI.py:88); g >= 0: every h uses hyper-sample g's
 *     (uEI_noiseless.py:66 evaluates it once, with whichever hyper-sample was current).
 * Factorization schedules (speed only: every one computes the same factor up to rounding; tests/test_gpu_parity.py pins it):
 *   "team_fit" = -1 (default: by size) / 0 (never) / 1: resident workgroup TEAMS that hand tiles to each other through device-side
 *     counters (chol_team.hip).  Up to "team_whole_max" (default 24) panels of 128 rows ONE launch does the Cholesky AND the inverse;
 *     beyond, "team_hybrid" = 2 (default): the first block rows as team launches of "team_panels" (default 6) panels, each followed by one
 *     trailing update with K = 128 x that, then ONE team launch (Cholesky + inverse) for the remaining corner on "team_tail_share"
 *     eighths of the compute units while the inverse of the first block rows runs underneath; 1: the first block rows by the launched
 *     schedule; 0: no hybrid (team_fit = 1 then means panel groups throughout).  "team_stream" = 1 (default): a workgroup of every team
 *     forms U[p][p+1] and the last row of A[p+1][p+1] sixteen rows at a time UNDERNEATH the diagonal block p (same sums in the same
 *     order: bit-identical to 0 up to 8 panels); "team_crit_load": the workgroups of the critical tiles carry nothing else while the
 *     others get by with at most this many tiles each,
 *   "predict_i8" = 1: the variance contraction v = L^-1 K*, sum v^2 (posterior.py:308-313) in EXACT int8 products (gemm_i8.hip): every
 *     column of R and of K* gets one power-of-two scale and is cut into six signed digits of radix 254 (|d| <= 127: 47.9 bits), the 21 digit
 *     products with i + j <= 5 run on v_mfma_i32_16x16x64_i8 into int32 sums, fp64 recombination, squares and the per-128-row partial sums of
 *     the fp64 kernels.  From 17 candidates per call up, N <= 16384, variances only (gradients keep the fp64 path); the posterior mean does not
 *     go through it.  Accuracy at cond(Ky) = 4e9 (config 3): |d var| <= 1.1e-11 sigma_f^2, 3.4e-6 relative at variances of 1e-6 sigma_f^2 (the fp64
 *     contraction: 1e-14 / 1e-8) -- inside every parity gate of tests/test_gpu_round3.py.  Speed at N = 4096: 38-40 against 62.2 ms per
 *     65 536-candidate step.  An option like predict_f32: the default stays the fp64 contraction.  "i8_group" (speed only): 0 = the
 *     workgroups an XCD runs together are a block of 4 row-tile pairs x 8 column tiles, g >= 1 = bands of g pairs x all column tiles.
 *   "lookahead" = -1 (by size) / 0 (single stream) / 2 (reserved-CU chain with device-side counters: one output, or two outputs up to
 *     12 panels), "aggregate" = G panels per trailing update of the single-stream schedule (default 0 = by size: 1 below 16 panels,
 *     2 from 16, 3 from 32), "overlap_inverse" (early part of the inverse underneath the factorization), "trsm_wave", "merge_x3" = 0 /
 *     1 / 2 (second product of an inverse merge in the three-buffer triangular kernel: never / from 4096 rows / whenever the shape allows).
 *     Every schedule that waits on device-side counters has a 0.2 s cut-off; when it fires the attempt is redone on the single-stream
 *     schedule (bocf_get_stat "sched_timeouts"), twice and those schedules stay off for the context.
 *   "swizzle" = variance-GEMM tiling: -1 (default) by size (258 from 2048 candidates per pass when the padded N is a multiple of 256,
 *     else 0); 258 = 256-row tiles in the three-buffer kernel, 0 = 128-row tiles; both give bit-identical sums.
 * Multi-GPU:
 *   "shard_fit" = 1 (with a communicator, bocf_comm_init): bocf_fit factorizes only this rank's contiguous share of the m independent
 *     outputs (multi_outputGP.py:64-102 fits them one after the other) and the ranks exchange what prediction needs -- the inverse
 *     factors by one RCCL broadcast per output (one group), alpha / train mean / log-marginal / jitter / status by ONE all-reduce.  The
 *     helper context takes the caller's schedule options and history and chooses by the global output count, so a share is factorized
 *     by the kernel sequence the replicated fit would run for it (bit-identical results); where the schedules still differ the results
 *     agree up to rounding.  bocf_get_factor (L), bocf_append, bocf_update_targets and bocf_lml_gradients are not served by such a
 *     fit (they need the upper factor, which stays on its owner).
 * NOT in this library: the timing-only kernel variants, slower tilings / tile orders kept for the tools, and the test hooks (diagonal
 * shift that forces the jitter ladder, single-process stand-in for the ranks of a sharded fit, forced schedule time-out / device size)
 * exist only in libbocf_hip_probes.so (the same sources with -DBOCF_PROBES), which tools/ and the tests that need a hook load; the
 * product library rejects those names. */
int bocf_set_option(bocf_ctx* ctx, const char* name, long long value);

/* FIT, one exact-GP inference per output with fixed hyper-parameters.  Replaces
 * multi_outputGP.updateModel (multi_outputGP.py:97-102) -> GPModelFixedHyps.updateModel
 * (gpmodel_fixed_hyps.py:61-69) -> GP.parameters_changed (GPy/core/gp.py:247-256) ->
 * ExactGaussianInference.inference (exact_gaussian_inference.py:29-65):
 *   Y is mean-centred per output (Standardize, normalizer.py:57-63, std == 1);
 *   Ky = K(X,X) + (noise + 1e-8) I (:46-47); L = chol(Ky) with the jitchol ladder
 *   (GPy/util/linalg.py:52-71: jitter = mean(diag) 1e-6, x10 per retry, <= max_tries);
 *   alpha = Ky^-1 (Y - mean) (:51); log-marginal (:53).
 * X (N,d); Y (m,N); variance (m); lengthscale (m,d) (an isotropic kernel repeats its value);
 * noise (m).  jitter_out (m) / lml_out (m) may be NULL.  Returns 0, or info>0 if some output
 * is not positive definite even with jitter (scipy.linalg.LinAlgError in the reference). */
int bocf_fit(bocf_ctx* ctx, const double* X, const double* Y, int N, int d, int m, int kernel_id,
             const double* variance, const double* lengthscale, const double* noise,
             int max_jitter_tries, double* jitter_out, double* lml_out);

/* Outputs with DIFFERENT kernel families: the reference's multi_outputGP takes a kernel list, one GPy kernel per output
 * (multi_outputGP.py:44-47 -> GPModel(kernel=...) gpmodel.py:50-61).  ids (m) are taken by the NEXT bocf_fit / bocf_infer / bocf_hmc
 * call with m outputs (hyper-sample-major like every per-output array) and override its kernel_id argument; the list is consumed by
 * that call (m = 0 clears a pending one).  The kernels that evaluate a covariance function are specialised per family at compile time:
 * the library issues one launch per run of equal ids. */
int bocf_set_kernel_ids(bocf_ctx* ctx, const int* ids, int m);

/* Same inputs, new targets Y (m,N): recomputes the mean-centring, alpha, the log-marginal and the cached
 * posterior mean at the training inputs (two GEMVs) -- what GP.set_XY(Y=...) costs the reference a full
 * inference for (GPy/core/gp.py:191-227). */
int bocf_update_targets(bocf_ctx* ctx, const double* Y, double* lml_out);

/* Rank-1 append of ONE observation x_new (d) with the complete new targets Y (m,N+1): borders the resident
 * factor U and its inverse R in O(N^2) instead of refitting in O(N^3) (the reference refits: cbo.py:363,419 ->
 * GP.set_XY).  Returns 0 on success; 1 when the caller must run bocf_fit instead (padding exhausted, i.e. N is
 * a multiple of 128; a jittered factor; an output-sharded fit; or a non-positive new pivot, in which case the
 * context is marked unfitted).  On success everything derived from the old factor is dropped: the candidate
 * batch and its acquisition vector, the reference / pending / Thompson sets, the reduced-precision copies of R
 * and the inverse of Ky an inference left for bocf_lml_gradients (which is then formed anew). */
int bocf_append(bocf_ctx* ctx, const double* x_new, const double* Y, double* lml_out);

/* Removal of ONE observation, row `index` of the resident inputs, with the complete new targets Y (m,N-1): the
 * plane rotations that row `index` of R fixes take U and R to the factor of the remaining N-1 points in O(N^2)
 * (orthogonal transformations only; no pivot can fail).  The inputs behind `index` move up by one and row N-1
 * becomes identity padding again, so a bocf_append can follow at every N.  Returns 0 on success; 1 when the
 * caller must run bocf_fit instead and nothing has been touched (a jittered factor; an output-sharded fit);
 * < 0 with bocf_last_error (not fitted, null Y, index outside [0,N), N = 1).  On success everything derived from
 * the old factor is dropped, exactly as after bocf_append.  One host synchronisation. */
int bocf_remove(bocf_ctx* ctx, int index, const double* Y, double* lml_out);

/* Gradients of the log marginal likelihood of the CURRENT fit w.r.t. the raw hyper-parameters: kernel variance
 * (m), lengthscales (m,d) (an isotropic kernel's single gradient is the sum over d), noise variance (m).  The
 * numerical core of hyper-parameter learning (GP.parameters_changed, GPy/core/gp.py:256-258): dL_dK and
 * dL_dthetaL of exact_gaussian_inference.py:61-63 + kern.update_gradients_full (stationary.py:191-214,
 * se.py:169-188).  Ky^-1 = R R^T replaces pdinv's dpotri.  Priors / transformations stay on the host. */
int bocf_lml_gradients(bocf_ctx* ctx, double* dvariance_out, double* dlengthscale_out, double* dnoise_out);

/* One hyper-parameter INFERENCE = bocf_fit's log-marginal + bocf_lml_gradients, in one call: what every step of
 * GPModel.updateModel's optimiser (gpmodel.py:115 -> paramz Model._objective_grads) and every leapfrog step of its HMC
 * (GPy/inference/mcmc/hmc.py:62-66) costs.  Arguments as bocf_fit; returns 0, the LAPACK-style info of a failed
 * factorization (> 0), or < 0.  Models with N <= 128 and d <= 16 run as ONE fused launch per jitter attempt (kernel
 * build, Cholesky, inverse, alpha, log-marginal, Ky^-1 and the gradient sums in one workgroup per output) and leave
 * no factor behind -- call bocf_fit before predicting; larger models run bocf_fit + bocf_lml_gradients.  Option
 * "fused_infer" = 0 forces the two-call path. */
int bocf_infer(bocf_ctx* ctx, const double* X, const double* Y, int N, int d, int m, int kernel_id, const double* variance,
               const double* lengthscale, const double* noise, int max_jitter_tries, double* jitter_out, double* lml_out,
               double* dvariance_out, double* dlengthscale_out, double* dnoise_out);

/* The HMC chain of GPModel.updateModel (gpmodel.py:117-118: HMC(model, stepsize).sample(num_samples, hmc_iters) ->
 * GPy/inference/mcmc/hmc.py:30-69 with M = I; 200 draws x 20 leapfrog steps = 4000 inferences per output and model update in the
 * reference) as ONE device launch, for the models the fused inference serves (N <= 128, d <= 16).  One workgroup per output runs its
 * whole chain: per leapfrog step the in-kernel inference (kernel matrix, jitchol ladder linalg.py:52-71, alpha, log-marginal,
 * hyper-gradients: exact_gaussian_inference.py:46-63, stationary.py:191-214), the objective -(log-marginal + log-prior) and its
 * gradient w.r.t. the optimizer array (paramz Model._objective_grads; Gamma priors priors.py:264-330, Logexp transform of paramz 0.9.1
 * as restated in bocf_amd/hyper.py), the momentum / position updates (hmc.py:62-66), and per draw the Hamiltonian and the
 * Metropolis test (hmc.py:45-59).  The HOST draws momenta and uniforms in the reference's RNG order and hands them in.
 *   theta (m, P) in/out, P = 2 + nls: [kern.variance, kern.lengthscale (nls = 1 isotropic | d ARD), Gaussian_noise.variance];
 *   fixed (m, P): 1 = constrain_fixed (not sampled);  prior Gamma(a, b) on every parameter;
 *   momenta (m, num_samples, P) / chains_out (m, num_samples, P): the free entries of a draw packed in front;  uniforms (m, num_samples);
 *   chains_out[i] = the state draw i started from, overwritten by the proposal when accepted (hmc.py:45-59);
 *   raise_on_failure = 1: a factorization that fails even with jitter (or parameters leaving the positive domain) stops that output's
 *   chain with status_out[j] = draw + 1 and the call returns 1 (hmc.py lets jitchol's LinAlgError propagate); 0: the proposal is
 *   rejected and the chain goes on.  A non-finite objective is rejected in both modes, as hmc.py:51-58 does.
 *   inferences_out: leapfrog-step inferences of the longest chain.  Leaves no factor behind (bocf_fit before predicting). */
int bocf_hmc(bocf_ctx* ctx, const double* X, const double* Y, int N, int d, int m, int kernel_id, double* theta, int nls, const int* fixed,
             double prior_a, double prior_b, const double* momenta, const double* uniforms, int num_samples, int hmc_iters, double stepsize,
             int max_jitter_tries, int raise_on_failure, double* chains_out, int* accepted_out, int* diverged_out, int* status_out,
             long long* inferences_out);

/* The same chain for models beyond the fused kernel (N > 128 or d > 16), STREAM-RESIDENT: GPy/inference/mcmc/hmc.py:30-69 as
 * GPModel.updateModel runs it (gpmodel.py:117-118).  Every leapfrog step (hmc.py:62-66) is the launch sequence of one inference
 * (bocf_fit's factorization + bocf_lml_gradients: exact_gaussian_inference.py:46-63, stationary.py:191-214) between two launches of a
 * small kernel that does what the host loop did per step -- momentum / position update, Logexp transform, Gamma priors (priors.py:264-330),
 * objective and gradient w.r.t. the optimizer array, and per draw the Hamiltonian and the Metropolis test (hmc.py:45-59); the host
 * enqueues and looks at one word every few draws.  Arguments as bocf_hmc.  jitchol's ladder (linalg.py:52-71) needs the host: when a
 * factorization meets a non-positive pivot (or parameters leave the positive domain) the chain stops with *draws_done_out = that draw
 * (< num_samples) and every output back at the draw's start; the caller runs that ONE draw with bocf_infer per step (ladder included) and
 * calls again for the remaining draws.  accepted_out / diverged_out / chains_out cover the completed draws.  Returns 0 or < 0.  Leaves no
 * usable factor behind (bocf_fit before predicting). */
int bocf_hmc_streamed(bocf_ctx* ctx, const double* X, const double* Y, int N, int d, int m, int kernel_id, double* theta, int nls,
                      const int* fixed, double prior_a, double prior_b, const double* momenta, const double* uniforms, int num_samples,
                      int hmc_iters, double stepsize, double* chains_out, int* accepted_out, int* diverged_out, int* draws_done_out,
                      long long* inferences_out);

/* Per-output status of the LAST bocf_fit / bocf_infer: info_out[j] = 0 when output j factorized (possibly on a jitter
 * rung), else the 1-based index of its first non-positive pivot on the last rung tried -- which outputs made jitchol give
 * up (GPy/util/linalg.py:56-71 raises for ONE matrix; here m are factorized together, so the caller needs to know which).
 * n must equal the m of that call. */
int bocf_last_fit_info(bocf_ctx* ctx, int* info_out, int n);

/* Test/inspection hooks: lower Cholesky factor L (N,N row-major) and alpha (N) of output j --
 * Posterior.woodbury_chol / woodbury_vector (posterior.py:132-170, 193-205). */
int bocf_get_factor(bocf_ctx* ctx, int j, double* L_out, double* alpha_out);
/* K(X,X) of output j as built on the device (N,N), without the diagonal noise: kern.K(X). */
int bocf_get_train_kernel(bocf_ctx* ctx, int j, double* K_out);

/* Test/inspection hook for the acquisition kernels alone: hand the context a posterior -- mean (m,C), var (m,C) exactly as
 * model.predict / posterior_variance would return it, and the posterior mean at N evaluated points mu_train (m,N) -- so
 * that bocf_acq_linear / bocf_set_mc_samples + bocf_acq_mc / bocf_select_topk run on it (the duck-typed Mock-model pattern
 * of the reference's own acquisition tests, GPyOpt/testing/acquisitions_tests/test_ei_acquisition.py:11-26).  Everything
 * that needs a factorization fails until the next bocf_fit. */
int bocf_set_posterior(bocf_ctx* ctx, int m, int C, int N, const double* mean, const double* var, const double* mu_train);

/* Upload the candidate batch X* (C,d); it stays resident in HBM until replaced. */
int bocf_set_candidates(bocf_ctx* ctx, const double* Xc, int C);

/* PREDICT on the resident candidates.  Replaces multi_outputGP.predict / posterior_mean /
 * posterior_variance[_noiseless] (multi_outputGP.py:138-200) -> PosteriorExact._raw_predict /
 * raw_posterior_mean / raw_posterior_variance (posterior.py:268-320):
 *   mean = K(X*,X) alpha + ymean;  var = sigma_f^2 - ||L^-1 K(X,X*)||^2 [+ noise] [clipped].
 * mean_out / var_out are (m,C) or NULL. */
int bocf_predict(bocf_ctx* ctx, int flags, double* mean_out, double* var_out);

/* The `full_cov=True` form of multi_outputGP.predict (multi_outputGP.py:138-149): every output's model returns its n x n predictive
 * covariance (PosteriorExact._raw_predict with full_cov, posterior.py:274-283: Kxx - tmp^T tmp; + noise on the diagonal,
 * gaussian.py:95-97; every ENTRY clipped at 1e-10, gpmodel_fixed_hyps.py:84-86 / gpmodel.py:145-147) and the wrapper keeps column 0
 * (cov[j,:] = tmp2[:,0], multi_outputGP.py:146-148).  cov0_out (m,C): cov0[j][i] = k_j(x_i, x_0) - k_j(x_i,X) Ky_j^-1 k_j(X, x_0)
 * [+ noise_j if i == 0 and BOCF_ADD_NOISE] [clipped at 1e-10 if BOCF_CLIP] for the resident candidates x_0 ... x_{C-1}; the n x n
 * matrix is never formed (one extra solve w = R (R^T k(X, x_0)) and a mean-shaped pass over the candidates). */
int bocf_predict_cov_column(bocf_ctx* ctx, int flags, double* cov0_out);

/* Joint posterior over point sets and composite Thompson sampling.  All three are local to the context: they issue no collective (a
 * multi-rank run calls them on one rank's context; sampling across candidate shards would need the cross-shard covariance).  They work on
 * a fitted model (bocf_fit / bocf_infer; not a bocf_set_posterior one) and leave the predict and acquisition state as it was.
 * `group` = h selects hyper-sample h's outputs [h m, (h + 1) m) of the m = outputs / hyper_samples per sample, -1 all of them; M_g is
 * the number of outputs selected.  The covariance of M_g padded C x C matrices (M_g Cp^2 8 bytes, Cp = C rounded up to 128) must fit in
 * option "workspace_mb", else the call fails.  Every failure returns < 0 with bocf_last_error() set; the context stays usable.
 *
 * bocf_posterior_cov: the noiseless, unclipped posterior covariance (posterior.py:104-125, gp.py:576-583)
 *   cov_out[j][a][b] = k_j(x1_a, x2_b) - k_j(x1_a, X) Ky_j^-1 k_j(X, x2_b),   (M_g, n1, n2), X1 (n1, d), X2 (n2, d).
 * bocf_posterior_samples: joint samples of the latent outputs at the resident candidates (bocf_set_candidates, C of them):
 *   F_j = mu_j + L_j Z_j, L_j L_j^T = Sigma_j + jitter_j I, Sigma_j the candidates' covariance above and mu_j the posterior mean
 *   (target mean included).  Z (M_g, C, S) standard normals from the host, 1 <= S <= 256; samples_out (M_g, C, S) or NULL (they stay on
 *   the device for bocf_thompson_select); jitter_out (M_g) the jitter used.  Jitter ladder per output: rung 0 = 1e-8 max(mean(diag
 *   Sigma_j), 1e-10), ten times the last per further rung, at most max(1, max_jitter_tries) rungs.  Returns 0, or j + 1 > 0 for the first
 *   output j that stayed indefinite (the samples of that call are then not kept).  The samples replace the resident ones of the
 *   hyper-samples selected (group -1: all of them); a fit, a data change or a new candidate set drops them all.
 * bocf_thompson_select: for every resident sample path p -- hyper-samples in increasing order, then the path index within that
 *   hyper-sample's block -- the k best candidates of u(p, c) = U(theta_p, F[:, c, p]) (the device utility util_kind with util_params, as
 *   the acquisitions evaluate it): value descending, ties to the lowest index.  theta (P, theta_dim), one row per path; idx_out and
 *   val_out (P, k); 1 <= k <= min(C, 64). */
int bocf_posterior_cov(bocf_ctx* ctx, const double* X1, int n1, const double* X2, int n2, int group, double* cov_out);
int bocf_posterior_samples(bocf_ctx* ctx, int group, const double* Z, int S, int max_jitter_tries, double* samples_out, double* jitter_out);
int bocf_thompson_select(bocf_ctx* ctx, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim, int k,
                         long long* idx_out, double* val_out);

/* Pathwise posterior samples: Thompson paths as FUNCTIONS of x (Matheron's rule with random Fourier features; Wilson et al. 2020,
 * "Efficiently sampling functions from Gaussian process posteriors").  Local to the context and for a fitted model only, like the joint
 * posterior above; `group` has the meaning it has in bocf_posterior_samples.  Per output j (of hyper-sample h) and path s, with the
 * inputs divided by the lengthscales, x~ = x / l_j:
 *   phi_jf(x) = sqrt(2 s2_j / F) cos(omega_jf . x~ + b_jf)                       f < F
 *   g_js(x)   = sum_f phi_jf(x) w_jfs                                            a draw of the (feature-approximated) prior
 *   v_js      = Ky_j^-1 (yc_j - g_js(X) - sqrt(nug_j) E_j[:, s]),                nug_j = noise_j + 1e-8 + jitter_j, the fit's diagonal
 *   f_js(x)   = ybar_j + g_js(x) + sum_i k_j(x, X_i) v_js[i]
 * The device consumes no random numbers: omega (M_g, F, d), phase b (M_g, F), weights w (M_g, F, S) and eps E (M_g, N, S) come from the
 * host.  For the RBF / SE ids omega ~ N(0, I); for Matern-nu omega = z / sqrt(chi2_{2 nu} / (2 nu)), z ~ N(0, I) (nu = 5/2, 3/2);
 * b ~ U[0, 2 pi); w, E ~ N(0, 1).
 * EXACT given (omega, b): E_{w,E}[f] is the posterior mean, and at the training inputs f_s(X_i) = Y_i - sqrt(nug) E_is - nug v_is.
 * APPROXIMATE: the variance of a path is that of the feature approximation of the prior (the method's error, not the device's; F = 2048
 * on Matern-5/2 gave pointwise ratios between 0.73 and 2.07 to the exact posterior variance near data).
 *
 * bocf_set_paths: stages S paths (1 <= S <= 64) of F features (1 <= F <= 16384) for the hyper-samples of `group`, replacing theirs; S = 0
 *   drops them.  The solve is v = R (R^T rhs) with the fit's R = U^-1 through the fp64 GEMM: a PLAIN fp64 solve, no double-double
 *   refinement (the posterior mean's alpha is refined; v is not).  Paths belong to one posterior INCLUDING its targets: bocf_fit,
 *   bocf_infer, bocf_append and bocf_update_targets drop them; bocf_set_candidates does NOT -- a path is a function.
 * bocf_path_values: evaluates every resident path of the group at the resident candidates; values_out (M_g, C, S) or NULL.  The values
 *   stay on the device as the group's resident Thompson samples, so bocf_thompson_select ranks them unchanged (and a new candidate set
 *   drops the VALUES, as it drops any samples).  Per candidate the sum runs over the training rows in increasing order, then the
 *   features: a candidate's value does not depend on the batch it came in.  The predict and acquisition state is left as it was.
 * bocf_path_utility: for row c of the resident candidates, u_c = U(theta_p, f_{., p}(x_c)) of the ONE path p = row_path[c] -- paths
 *   numbered as bocf_thompson_select numbers them -- and (grad_out (C, d) != NULL) du_c/dx = sum_j dU/dy_j df_{j,p}/dx.  theta
 *   (P, theta_dim) with P the number of resident paths; val_out (C).  Meant for the few hundred rows of a refinement step.
 * Every failure returns < 0 with bocf_last_error() naming the entry point; the context stays usable. */
int bocf_set_paths(bocf_ctx* ctx, int group, const double* omega, const double* phase, const double* weights, const double* eps, int F, int S);
int bocf_path_values(bocf_ctx* ctx, int group, double* values_out);
int bocf_path_utility(bocf_ctx* ctx, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim, int P,
                      const int* row_path, double* val_out, double* grad_out);

/* Input gradients of the posterior at the resident candidates, (m,C,d) each.  Replaces
 * multi_outputGP.posterior_mean_gradient / posterior_variance_gradient (multi_outputGP.py:284-306) ->
 * GP.posterior_mean_gradient / posterior_variance_gradient (GPy/core/gp.py:438-490) -> kern.gradients_X
 * (stationary.py:312-331, se.py:135-148); uses w = Ky^-1 k(X,x*) = R (R^T k*) instead of dpotri. */
int bocf_predict_gradients(bocf_ctx* ctx, double* dmean_out, double* dvar_out);

/* Posterior mean at the training inputs, (m,N): multi_outputGP.posterior_mean_at_evaluated_points
 * (multi_outputGP.py:176-180). */
int bocf_mean_at_train(bocf_ctx* ctx, double* out);

/* Closed-form acquisition of a LINEAR utility over the resident candidates.  Replaces
 * maEI._compute_acq/_marginal_acq/_marginal_best_so_far (maEI.py:38-54,81-98,129-136) and the
 * maPI / EI / PI twins.  theta (L,m), prob (L) or NULL (= plain mean over L sampled thetas,
 * maEI.py:52).  acq_out (C) or NULL (result stays on the device for bocf_select_topk). */
int bocf_acq_linear(bocf_ctx* ctx, int kind, const double* theta, const double* prob, int L, double* acq_out);

/* As bocf_acq_linear, plus d acq / dx (C,d): maEI._compute_acq_withGradients / _marginal_acq_with_gradient
 * (maEI.py:57-78,101-126; EI = (mu-best) Phi + sigma phi with scipy's norm.pdf/cdf) and the maPI twin
 * (maPI.py:56-76,96-121). */
int bocf_acq_linear_grad(bocf_ctx* ctx, int kind, const double* theta, const double* prob, int L, double* acq_out, double* dacq_out);

/* Upload the common-random-number normals W (S,m): uEI_noiseless.W_samples (uEI_noiseless.py:31). */
int bocf_set_mc_samples(bocf_ctx* ctx, const double* W, int S);

/* Monte-Carlo acquisition of a composite utility over the resident candidates.  Replaces
 * uEI_noiseless._compute_acq/_marginal_acq (uEI_noiseless.py:40-83) and uPI (uPI.py:43-86):
 *   acq(x) = sum_l p_l (1/S) sum_s hinge_or_indicator( U(theta_l, mu(x) + sigma(x) o W_s) - best_l ),
 *   best_l = max_i U(theta_l, mu(X_i)), sigma = sqrt(clipped posterior variance incl. noise).
 * theta (L,theta_dim) (may be NULL when theta_dim == 0). */
int bocf_acq_mc(bocf_ctx* ctx, int kind, int util_kind, const double* util_params, int n_util_params,
                const double* theta, int theta_dim, const double* prob, int L, double* acq_out);

/* Monte-Carlo EI with d acq / dx (C,d): uEI_noiseless._compute_acq_withGradients /
 * _marginal_acq_with_gradient (uEI_noiseless.py:118-170); dU/dy is the analytic derivative of the
 * device utility (the dfunc of the experiment scripts). */
int bocf_acq_mc_grad(bocf_ctx* ctx, int util_kind, const double* util_params, int n_util_params, const double* theta,
                     int theta_dim, const double* prob, int L, double* acq_out, double* dacq_out);

/* Utility programs (layout above).  bocf_check_utility_program is host-only and takes no context: it accepts the blob only if its size, magic
 * and version are right, m and theta_dim are the ones given, both section lengths, the slot count and the constant count are within the
 * limits, every opcode is known, every destination and every slot operand is below the slot count, a slot is read only after the section
 * wrote it, every input index is below m, every parameter index below theta_dim, every constant index below the constant count, every
 * constant is finite and every output slot was written by its section -- so an accepted program cannot address outside its slot file or
 * its argument arrays and its interpreter loop runs a validated number of steps.  Returns 0, or < 0 with the offending field named in the
 * error text.  bocf_set_utility_program runs the same check (for the m and theta_dim the header states) and stages the blob on the
 * context, where it stays until it is replaced (like the samples of bocf_set_mc_samples); it invalidates the best-so-far cache.  A rejected
 * blob leaves the resident program as it was and never reaches a launch. */
int bocf_check_utility_program(const void* blob, long nbytes, int m, int theta_dim);
int bocf_set_utility_program(bocf_ctx* ctx, const void* blob, long nbytes);

/* Selection on the last acquisition vector: indices of the k largest values, ties to the lowest
 * index -- np.argsort(-acq)[:k] of AnchorPointsGenerator.get (anchor_points_generator.py:59-61)
 * applied to AcquisitionBase.acquisition_function's -acq (GPyOpt/acquisitions/base.py:33-40).
 * idx_out (k) int64, val_out (k) or NULL. */
int bocf_select_topk(bocf_ctx* ctx, int k, long long* idx_out, double* val_out);

/* ---- expected utility of the recommendation step (cbo.py:121-235, CBO._current_marginal_argmax).  The reference maximises, for
 * every utility parameter theta_l of _current_max_value (cbo.py:61-84), the posterior expected utility
 *   v(x) = sum_{h < n_hyps} E_h[ U(theta_l, f(x)) ]          (a SUM over hyper-samples and samples, cbo.py:160 "not normalized")
 * with the posterior of predict_noiseless (no likelihood noise, variance clipped at 1e-10).  Modes:
 *   BOCF_EU_MEAN    theta . mu                    utility.linear (cbo.py:124-157); util_kind ignored, theta_dim = m
 *   BOCF_EU_CLOSED  psi(theta, mu, var)           expectation_utility given (cbo.py:159-188); closed forms of
 *                   NEG_SQ_DIST  -||mu - theta||^2 - sum var
 *                   NEG_SUM_EXP  -sum exp(mu_j + var_j / 2)
 *                   ROSENBROCK   -sum_{j<m/2} (a - mu_j)^2 + 100 mu_{j+m/2}^2 + var_j + 100 var_{j+m/2}
 *                   (LINEAR and NEG_EXP_COS have none here: an error)
 *   BOCF_EU_MC      sum_{s<S} U(theta, mu + sigma o Z_s)   otherwise (cbo.py:190-231); Z of bocf_set_eu_samples, per parameter
 * Hyper-samples: with several resident (option hyper_samples = H > 1) the first n_hyps <= H are summed; with one (fixed
 * hyper-parameters, where the reference makes n_hyps identical passes) the value is multiplied by n_hyps. */
enum { BOCF_EU_MEAN = 0, BOCF_EU_CLOSED = 1, BOCF_EU_MC = 2 };

/* Upload the Monte-Carlo normals of the recommendation step: Z (L,S,m), block l = the np.random.normal(size=(S, m)) drawn for
 * parameter l (cbo.py:200).  Independent of bocf_set_mc_samples. */
int bocf_set_eu_samples(bocf_ctx* ctx, const double* Z, int L, int S);

/* Expected utility (and its input gradient) over the resident candidates, candidate c taking parameter row_param[c] in [0, L) of
 * theta (L,theta_dim): all L argmax problems in one call.  val_out (C); grad_out (C,d) or NULL (value only: no gradient pass).
 * Leaves the acquisition state (the last acquisition vector for bocf_select_topk, the Monte-Carlo samples of bocf_set_mc_samples,
 * the best-so-far cache) untouched. */
int bocf_expected_utility(bocf_ctx* ctx, int mode, int util_kind, const double* util_params, int n_util_params, const double* theta,
                          int theta_dim, int L, const int* row_param, int n_hyps, double* val_out, double* grad_out);

/* ---- look-ahead posterior and the discrete composite knowledge gradient.  The reference's multi_outputGP carries look-ahead helpers
 * (multi_outputGP.py:203-281,309-330 -> GPy/core/gp.py:493-627) for the knowledge-gradient acquisitions its experiment scripts import
 * (test_1a.py:7-8).  Per output j, with the fit's own Ky_j = K_j + (noise_j + 1e-8 + jitter_j) I, mu_j and sigma^2_j the posterior mean and
 * the noiseless, unclipped variance, Sigma_j(a, x) = k_j(a, x) - k_j(a, X) Ky_j^-1 k_j(X, x):
 *   s2_j(x)         = max(sigma^2_j(x), 0) + noise_j + 1e-8 + jitter_j
 *   sigma^2_j(a | x) = sigma^2_j(a) - Sigma_j(a, x)^2 / s2_j(x)       raw: no clip, no noise (gp.py:514-544 factorizes the bordered Ky with
 *                                                                    N + 1 rows; by the Schur complement that is this rank-one downdate)
 *   beta_j(a; x)    = Sigma_j(a, x) / s_j(x),   mu_j(a | x, z) = mu_j(a) + beta_j(a; x) z_j     (fantasy with a standard normal z_j)
 * These entry points work on a fitted model (not a host-given posterior), are local to the context, use fp64 throughout (options
 * predict_f32 / predict_i8 are not read) and leave the predict, acquisition-parameter, Monte-Carlo-sample, expected-utility, best-so-far
 * and Thompson state as it was; only the acquisition call overwrites the acquisition vector, as every acquisition does.  Every failure
 * returns < 0 with the entry point's name in the error text; the context stays usable.  M = all fitted outputs, `group` and M_g as for
 * the joint posterior above.
 *
 * bocf_set_ref_points: stages the reference set A = Xa (na, d), 1 <= na <= 1024, for all M outputs: V_A = R^T K(X, A), Wa = Ky^-1 K(X, A),
 *   mu(A) and sigma^2(A) (multi_outputGP.partial_precomputation_for_covariance, multi_outputGP.py:245-254 -> gp.py:547-561).  It stays
 *   resident until it is replaced; a fit, an appended observation, new targets or a host-given posterior drop it, a new candidate set does
 *   not.  2 M Np nap 8 bytes (nap = na rounded up to 128) must fit in option "workspace_mb".
 * bocf_cov_to_ref: cov_out[j][c][a] = Sigma_j(x_c, a) for the resident candidates, (M_g, C, na), as V_c^T V_A subtracted from k
 *   (posterior_covariance_between_points_partially_precomputed, multi_outputGP.py:269-281 -> gp.py:564-573); dcov_out (M_g, C, na, d) or
 *   NULL: d Sigma_j(x_c, a) / d x_c = dk_j(x_c, a)/dx - sum_i dk_j(x_c, X_i)/dx Wa[i][a] (posterior_covariance_gradient and its
 *   precomputed twin, multi_outputGP.py:309-330 -> gp.py:586-627), for every kernel family.  The candidates are worked off in chunks whose V
 *   fits in "workspace_mb"; the gradient form needs M_g C na d 8 bytes there.
 * bocf_conditioned_variance: var_out[j][c] = sigma^2_j(x_c | a_q), the variance at the resident candidates conditioned on reference
 *   point q, (M_g, C) (posterior_variance_conditioned_on_next_point, multi_outputGP.py:215-228 -> gp.py:514-544); dvar_out (M_g, C, d) or
 *   NULL: its gradient in x_c, d sigma^2_j(x_c)/dx - 2 Sigma d Sigma/dx / s2_j(a_q) (multi_outputGP.py:231-242).
 * bocf_acq_kg: the one-step look-ahead value of every resident candidate against the discretisation A,
 *     KG(x) = sum_l p_l [ (1/Sf) sum_s max_a v(a; x, z_s, theta_l) - max_a v0(a; theta_l) ],
 *     v(a; x, z, theta) = E_w[ U(theta, mu(a | x, z) + sigma(a | x) o w) ]  with sigma^2(a | x) clipped at 1e-10, v0 the same with the
 *     current mu(a), sigma^2(a); ties in max_a go to the lowest a.  `mode` is the inner expectation, as for the expected utility:
 *     BOCF_EU_MEAN theta . mu, BOCF_EU_CLOSED the closed forms (an error for LINEAR and NEG_EXP_COS), BOCF_EU_MC the MEAN over the S <= 256
 *     common random numbers of the Monte-Carlo samples set for the acquisitions.  theta (L, theta_dim), prob (L) or NULL (= 1 / L),
 *     Zf (Sf, m) fantasy normals, 1 <= Sf <= 256.  With a finite Sf the value can be slightly negative; it is not clamped.  acq_out (C) or
 *     NULL; the values stay in the acquisition vector for the top-k selection (larger is better).  With option hyper_samples = H the
 *     first acq_hyper_samples are averaged.  dacq_out (C, d) or NULL: the envelope-rule gradient (the maximiser a* of every (s, l) held
 *     fixed); this form holds d Sigma / dx of every (output, candidate, reference point) at once -- averaged outputs x C na d 8 bytes
 *     within "workspace_mb" -- and is meant for the optimiser's small batches.
 *     (The reference's own knowledge-gradient acquisitions, uKG_SGA / uKG_cf of test_1a.py:7-8, are not in its tree; this is the
 *     discrete form over its look-ahead helpers gp.py:493-627.) */
int bocf_set_ref_points(bocf_ctx* ctx, const double* Xa, int na);
int bocf_cov_to_ref(bocf_ctx* ctx, int group, double* cov_out, double* dcov_out);
int bocf_conditioned_variance(bocf_ctx* ctx, int group, int q, double* var_out, double* dvar_out);
int bocf_acq_kg(bocf_ctx* ctx, int mode, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                const double* prob, int L, const double* Zf, int Sf, double* acq_out, double* dacq_out);

/* ---- greedy q-point batches: the Monte-Carlo expected improvement of the composite utility conditioned on pending points.  A batch
 * is filled one point at a time with the earlier points pending (the way the method of cbo.py:274-281 is run with an evaluator of batch
 * size q; the joint samples come from the look-ahead covariances of multi_outputGP.py:257-266 -> gp.py:576-583).  Per output j of
 * hyper-sample h, with mu_j, sigma^2_j and Sigma_j as above and the pending points P = (p_1 .. p_r), 1 <= r <= 15:
 *   Sigma~_j = Sigma_j(P, P) + tau_j I = L_j L_j^T (lower),  Q_j = Sigma~_j^-1          tau_j from the jitter ladder of the joint samples:
 *                                                                                      1e-8 max(mean diag, 1e-10), x 10 per rung
 *   F_sj = mu_j(P) + L_j Zp[s, j, :],  G_sj = L_j^-T Zp[s, j, :]                        Zp (S, m, r): host normals
 *   c_j(x) = Sigma_j(P, x),  v_j(x) = max(sigma^2_j(x) - c_j^T Q_j c_j, 1e-10)
 *   y_sj(x) = mu_j(x) + c_j(x)^T G_sj + sqrt(v_j(x)) W[s, j]                            W (S, m): the resident Monte-Carlo samples, S <= 256
 *   T_ls = max(best_l, max_i U(theta_l, F_s[:, i]))                                     best_l: the best-so-far of the Monte-Carlo acquisitions
 *   alpha(x | P) = (1/Ha) sum_h sum_l p_l (1/S) sum_s max(U(theta_l, y_s(x)) - T_ls, 0)
 * (F, G, c, y) is the Cholesky factor of the bordered joint covariance of [f(P), f(x)], so alpha(x | P) = qEI(P u {x}) - qEI(P) for the same
 * normals.  The latent, noiseless variance is used on purpose.  fp64 only, local to the context, state left as for the look-ahead entry
 * points above (the resident reference set included); every failure returns < 0 with the entry point's name in the error text.
 *
 * bocf_set_pending_points: stages P = Xp (r, d) for all M outputs in buffers of its own (as the reference set is staged), forms
 *   Sigma_j(P, P), factorizes it on the host with at most max_jitter_tries rungs and uploads Q, F, G.  Needs resident Monte-Carlo samples
 *   with S equal to theirs.  jitter_out (M) or NULL receives tau.  Returns 0, or j + 1 for the first output that stays indefinite.  The
 *   pending set stays resident until it is replaced; it is dropped by whatever drops the reference set.
 * bocf_get_pending_samples: F_out (M, r, S) = the joint samples F at the pending points, as the device holds them.
 * bocf_acq_pending: alpha(x | P) of every resident candidate into acq_out (C) or NULL (the values stay in the acquisition vector for the
 *   top-k selection); dacq_out (C, d) or NULL: d alpha / dx with P, Zp, W fixed --
 *   dy_sj/dx = dmu_j/dx + G_sj^T dc_j/dx + W[s, j] dv_j/dx / (2 sqrt(v_j)),  dv_j/dx = dsigma^2_j/dx - 2 (Q_j c_j)^T dc_j/dx (zero where the
 *   clip is active).  theta (L, theta_dim), prob (L) or NULL (= 1 / L); BOCF_UTIL_PROGRAM is refused.  With option hyper_samples = H the
 *   first acq_hyper_samples are averaged.  The candidates are worked off in chunks whose V fits in "workspace_mb"; the gradient form holds
 *   d Sigma / dx of every (output, candidate, pending point) at once, in one chunk. */
int bocf_set_pending_points(bocf_ctx* ctx, const double* Xp, int r, const double* Zp, int S, int max_jitter_tries, double* jitter_out);
int bocf_get_pending_samples(bocf_ctx* ctx, double* F_out);
int bocf_acq_pending(bocf_ctx* ctx, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                     const double* prob, int L, double* acq_out, double* dacq_out);

/* ---- joint q-point expected improvement of the composite utility (q-uEI): the quantity the greedy and the Thompson
 * batches approximate, at whole batches.  The resident candidates are read as B = C / q batches, batch b = rows b q .. b q + q - 1,
 * 1 <= q <= 8.  Per output j of hyper-sample h and batch X = (x_1 .. x_q):
 *   Sigma_j = k_j(X, X) - V_X^T V_X, symmetrised                       the latent, noiseless posterior covariance, as for the pending points
 *   tau_j   = 1e-8 max(mean diag Sigma_j, 1e-10)                        rung 0 of the pending points' ladder; there are no further rungs
 *   C_j     = row-wise Cholesky factor of Sigma_j + tau_j I with a pivot floor: p_k = a_kk - sum_{i<k} C_ki^2, and where !(p_k > 1e-10)
 *             p_k := 1e-10 and the pivot counts as floored -- no batch can fail
 *   y_sjk   = mu_jk + sum_{i <= k} C_j[k][i] Z[s, j, i]                 Z (S, m, q): host normals, common to all batches and hyper-samples
 *   alpha(X) = (1/Ha) sum_h sum_l p_l (1/S) sum_s max(max_k U(theta_l, y_s.k) - best_hl, 0)
 * best: (Ha, L) incumbents, or NULL = the best-so-far of the Monte-Carlo acquisitions per hyper-sample (option "best_group" honoured as in
 * bocf_acq_pending).  Argument conventions of bocf_acq_pending otherwise: theta (L, theta_dim), prob (L) or NULL (= 1 / L), the first
 * acq_hyper_samples hyper-samples are averaged, BOCF_UTIL_PROGRAM is refused.  acq_out (B) or NULL: the values also stay in the acquisition
 * vector (entries B .. C - 1 are -inf) for the top-k selection, which then ranks batches.  floored_out (B) or NULL: floored pivots per
 * batch, summed over outputs and hyper-samples.  dacq_out (B, q, d) or NULL: d alpha / dx of every point by the envelope rule with Z,
 * theta, best and tau fixed, the maximising point k* being the lowest index of the maximum; a floored pivot is a constant --
 *   dalpha/dx_a = sum_j [ mubar_ja dmu_j(x_a)/dx + Sigmabar_j[a][a] dsigma^2_j(x_a)/dx + 2 sum_{b != a} Sigmabar_j[a][b] d_1 Sigma_j(x_a, x_b) ],
 * Sigmabar_j the reverse pass of the factorization applied to Cbar_j[k][i] = sum_s Ybar[s][j][k] Z[s, j, i].  The value form takes any B and
 * works in chunks of whole batches (at most 512 points; V and Sigma of a chunk fit in "workspace_mb"); the gradient form takes C <= 128 in
 * one chunk.  S <= 256, m <= 16 outputs per hyper-sample.  fp64 only, buffers of its own: the Monte-Carlo samples, the reference set, the
 * pending points, the paths and the utility program stay resident; one stream synchronisation per call; every failure returns < 0 with the
 * entry point's name in the error text. */
int bocf_acq_joint(bocf_ctx* ctx, int q, const double* Z, int S, int util_kind, const double* util_params, int n_util_params, const double* theta,
                   int theta_dim, const double* prob, int L, const double* best, double* acq_out, double* dacq_out, int* floored_out);

/* ---- constrained uEI: linear constraints on the outputs inside the Monte-Carlo sum.  The simulator's outputs also
 * decide whether a design is admissible; the constraints are functions of the same m' outputs per hyper-sample the utility reads, so they
 * are applied sample by sample (the reference's AcquisitionBase has its constraint weighting commented out, base.py:5-74):
 *   A (K, m'), b (K), eta (K), 1 <= K <= 8, eta_k > 0, every entry finite
 *   c_k(y)  = sum_j A_kj y_j - b_k                   feasible <=> c_k(y) <= 0 for every k
 *   s(t)    = 1 / (1 + exp(-t))                      evaluated as exp of a non-positive argument on both branches
 *   phi(y)  = prod_k s(-c_k(y) / eta_k)              k in index order
 *   y_s(x)  = mu(x) + sigma(x) o W_s                 mu, sigma exactly the posterior bocf_acq_mc uses (variance with noise, clipped at 1e-10)
 *   F       = { i : c_k(mu_g(X_i)) <= 0 for every k }    HARD test on the train mean of the hyper-sample option best_group selects
 *   best_l  = max_{i in F} U(theta_l, mu_g(X_i))     only when F is not empty
 *   I_ls(x) = max(U(theta_l, y_s) - best_l, 0) if F is not empty;  1 if it is (the acquisition is then the smoothed probability of feasibility)
 *   alpha(x) = (1/Ha) sum_h sum_l p_l (1/S) sum_s I_ls(x) phi(y_s(x))
 * and, with T_ls = I_ls phi and s_k = s(-c_k / eta_k),
 *   dT/dy_j = [F not empty] 1{U > best_l} dU/dy_j phi - T_ls sum_k (1 - s_k) A_kj / eta_k
 *   A_j = sum_l p_l (1/S) sum_s dT/dy_j,  B_j = sum_l p_l (1/S) sum_s dT/dy_j W_sj / (2 sigma_j)
 *   d alpha / dx_q = (1/Ha) sum_h sum_j A_j dmu_j/dx_q + B_j dsigma^2_j/dx_q.
 * The smoothing is in the value as well as in the gradient; eta -> 0 recovers the indicator; a vacuous constraint (b_k huge) gives s = 1
 * exactly and alpha is then the uEI of bocf_acq_mc.  fp64; every failure returns < 0 with the entry point's name in the error text.
 *
 * bocf_set_output_constraints: the constraints stay resident until they are replaced (K = 0 drops them), like the samples of
 *   bocf_set_mc_samples; they do not depend on the factor, so no fit, append, target update or candidate upload forgets them.  m must be the
 *   outputs per hyper-sample (checked here when a model is fitted, and by the evaluating calls).
 * bocf_feasible_best: best_out (L) = best_l (-inf when F is empty) and *n_feasible_out = |F| for the hyper-sample of option best_group
 *   (-1: hyper-sample 0); either may be NULL.
 * bocf_acq_mc_constrained: alpha of every resident candidate into acq_out (C) or NULL -- the values are left as the context's acquisition
 *   vector, so bocf_select_topk, bocf_global_topk and the packed multi-rank merge work on them unchanged; dacq_out (C, d) or NULL = value
 *   only.  Needs resident constraints and Monte-Carlo samples; theta (L, theta_dim), prob (L) or NULL (= 1 / L); BOCF_UTIL_PROGRAM is
 *   refused, and so is the gradient form on a bocf_set_posterior context.  The hyper-sample loop runs inside the call under options
 *   acq_hyper_samples and best_group exactly as in bocf_acq_mc (-1: every hyper-sample's own feasible incumbent); candidate batches of any
 *   size go through the predict pass's chunking.  The incumbent is computed per call in buffers of this path: the parameter and
 *   best-so-far caches of the other acquisitions, the pending, reference and path sets are left as they were.  One synchronisation. */
int bocf_set_output_constraints(bocf_ctx* ctx, const double* A, const double* b, const double* eta, int K, int m);
int bocf_feasible_best(bocf_ctx* ctx, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                       int L, double* best_out, long long* n_feasible_out);
int bocf_acq_mc_constrained(bocf_ctx* ctx, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                            const double* prob, int L, double* acq_out, double* dacq_out);

/* ---- feasibility-aware recommendation: the constrained expected utility.  bocf_expected_utility in its Monte-Carlo
 * form with every sample weighed by the phi above (the resident set of bocf_set_output_constraints) and an infeasible outcome worth a
 * constant u0_l per utility parameter.  Per hyper-sample, with the posterior of bocf_expected_utility (predict_noiseless: NO likelihood
 * noise, variance clipped at 1e-10 -- not the noisy one of bocf_acq_mc) and Z the parameter's own normals of bocf_set_eu_samples:
 *   y_s(x)  = mu(x) + sigma(x) o Z_s                     Z block row_param[c]
 *   T_s     = phi(y_s) (U(theta_l, y_s) - u0_l)
 *   G_l(x)  = sum_{h < n_hyps} sum_{s < S} [ u0_l + T_s ]        a SUM, as bocf_expected_utility's; one resident hyper-sample counts n_hyps times
 *   P(x)    = (1 / (n_h S)) sum_h sum_s phi(y_s)                 smoothed probability of feasibility, a MEAN (n_h = hyper-samples visited)
 *   dT/dy_j = phi (dU/dy_j - (U - u0_l) q_j),   q_j = sum_k (1 - s_k) A_kj / eta_k     (1 - s_k from the same e as s_k, never a difference)
 *   A_j = sum_s dT/dy_j,  B_j = sum_s dT/dy_j Z_sj / (2 sigma_j),  dG/dx_q = sum_h sum_j A_j dmu_j/dx_q + B_j dsigma^2_j/dx_q.
 * Vacuous constraints give phi = 1 exactly: G is then bocf_expected_utility's BOCF_EU_MC value (up to the order of the sums) and P = 1.  u0
 * enters through U - u0 only: G is affine in u0 with slope sum (1 - phi).  Once phi multiplies the utility there is no mean or closed
 * form: every branch of the recommendation step takes this Monte-Carlo form with the utility's compiled-in kind (BOCF_UTIL_LINEAR for the
 * linear branch); BOCF_UTIL_PROGRAM is refused.  P is value-only.  fp64; every failure returns < 0 with the entry point's name in the
 * error text; the argument checks need no device and run before the context is touched.
 *
 * bocf_train_utility_range: min_out (L), max_out (L) = the range of U(theta_l, mu_g(X_i)) over all N training points, g the hyper-sample of
 *   option best_group (-1: hyper-sample 0) -- the default u0 is the min.  Needs no constraints.
 * bocf_expected_utility_constrained: candidate c takes parameter row_param[c] in [0, L) of theta (L, theta_dim) and u_infeasible (L, every
 *   entry finite); val_out (C) = G, pof_out (C) = P or NULL, grad_out (C, d) = dG/dx or NULL (value only).  The hyper-sample rules are
 *   bocf_expected_utility's (the first n_hyps of H are summed; H = 1 is scaled by n_hyps; more than are resident is refused).  The value
 *   form also runs on a bocf_set_posterior context; the gradient form refuses it, and d > 64.  Writes buffers of its own: the acquisition
 *   vector, the samples of bocf_set_mc_samples, the parameter and best-so-far caches, the incumbent buffers of bocf_acq_mc_constrained
 *   and bocf_expected_utility's buffers are left as they were.  One stream, one synchronisation. */
int bocf_train_utility_range(bocf_ctx* ctx, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                             int L, double* min_out, double* max_out);
int bocf_expected_utility_constrained(bocf_ctx* ctx, int util_kind, const double* util_params, int n_util_params, const double* theta,
                                      int theta_dim, int L, const double* u_infeasible, const int* row_param, int n_hyps, double* val_out,
                                      double* pof_out, double* grad_out);

/* ---- multi-GPU: candidate shards, ONE collective.  One process per GPU, one context per process.  The
 * reference's own candidate parallelism is a pathos process pool over single candidates (uEI_noiseless.py:85-97); here rank
 * r scores the contiguous slice [lo_r, hi_r) of the batch against its resident fit and the ranks exchange only their k
 * local winners.  RCCL is bound at run time (dlopen librccl.so.1); errors come back as < 0 with the RCCL text in
 * bocf_last_error().
 *
 * bocf_comm_unique_id: rank 0 creates the 128-byte rendezvous id (ncclGetUniqueId); the host passes it to the other ranks by
 *   whatever channel launched them (torch.distributed broadcast, MPI, a file).
 * bocf_comm_init: collective over all ranks (ncclCommInitRank); the communicator is owned by the context.
 * bocf_comm_info: returns 1 if the context holds a communicator (and its world / rank), 0 if not. */
#define BOCF_COMM_ID_BYTES 128
int bocf_comm_unique_id(char* id_out);
int bocf_comm_init(bocf_ctx* ctx, const char* id_bytes, int world, int rank);
int bocf_comm_destroy(bocf_ctx* ctx);
int bocf_comm_info(bocf_ctx* ctx, int* world_out, int* rank_out);

/* Global selection over the sharded batch: local top-k of the last acquisition vector (device), packed with the global
 * indices lo + i into a 2 * world * k buffer of doubles (values | indices, -inf elsewhere: RCCL has no MAXLOC), ONE
 * ncclAllReduce(max) on the context's stream, merged on the device (value descending, index ascending) -- the
 * np.argsort(scores)[:num_anchor] of AnchorPointsGenerator.get (anchor_points_generator.py:59-61) on the WHOLE batch,
 * identical on every rank.  Without a communicator it is the single-rank selection with lo added.  Empty slots (fewer than
 * k candidates in total) come back as index -1, value -inf. */
int bocf_global_topk(bocf_ctx* ctx, int k, long long lo, long long* idx_out, double* val_out);

/* The same selection for a host that owns the collective (torch.distributed): bocf_topk_packed writes the packed buffer of
 * this rank into caller-provided DEVICE memory (2 * world * k doubles) and returns when it is complete; after the caller's
 * all-reduce(MAX) over that buffer bocf_merge_packed merges it on the device. */
int bocf_topk_packed(bocf_ctx* ctx, int k, long long lo, int world, int rank, void* device_buf);
int bocf_merge_packed(bocf_ctx* ctx, int k, int world, const void* device_buf, long long* idx_out, double* val_out);

/* Profiling of the dominant kernel (needs option "profile"=1): accumulated HIP-event time in
 * ms and launch count since the last reset; algorithmic flops of those launches. */
int bocf_profile_read(bocf_ctx* ctx, double* ms_out, long long* launches_out, double* flops_out, int reset);

/* Named phases (option "profile" = 1): accumulated HIP-event time on the context's stream and number of brackets since the
 * last reset.  Names: "kbuild" (K(X,X) build), "cholesky", "inverse" (mirror + triangular inverse), "alpha" (alpha,
 * log-marginal, train mean) of bocf_fit; "cross" (K(X,X*) + mean), "acq", "topk" of the acquisition call. */
int bocf_profile_phase(bocf_ctx* ctx, const char* name, double* ms_out, long long* count_out, int reset);

/* Counters and facts about the context (diagnostics; none of them changes a result).  Names: "sched_timeouts" = how often a
 * multi-stream factorization schedule ran into its 0.2 s dependency time-out and the attempt was redone on the single-stream
 * schedule (then "gated_schedules_off" = 1 for the rest of the context's life); "last_schedule" = schedule of the last
 * factorization (0 single stream, 2 reserved CUs, 3 one team launch, 4 team launches of panel groups, 5 hybrid: the first block rows
 * launched or by team groups, one team launch for the rest);
 * "early_inverse";
 * "cu_masks_ok"; "comm_world" = ranks of the context's RCCL communicator (0 = none); "kstar_workspace_bytes". */
int bocf_get_stat(bocf_ctx* ctx, const char* name, long long* value_out);

/* The option table of bocf_set_option, readable without a GPU: bocf_option_count() entries; bocf_option_info gives name, accepted
 * range, kind (0 = speed only: same result up to rounding; 1 = documented semantics; 2 = probe / test hook -- present ONLY in the
 * -DBOCF_PROBES build libbocf_hip_probes.so that tools/ and some tests load, never in libbocf_hip.so) and a one-line description;
 * bocf_option_check(name, value) = 0 if bocf_set_option would accept the pair, else < 0 (text in bocf_last_error()). */
int bocf_option_count(void);
int bocf_option_info(int index, const char** name_out, long long* lo_out, long long* hi_out, int* kind_out, const char** what_out);
int bocf_option_check(const char* name, long long value);

/* Block until the context's stream is idle. */
int bocf_sync(bocf_ctx* ctx);

/* The acquisition optimiser's inner loop (host arithmetic, no context): replaces the 16 sequential scipy.optimize.fmin_l_bfgs_b runs of
 * GPyOpt/optimization/optimizer.py:283-354 (OptLbfgs: maxiter 500, factr 1e6; OptLbfgs2: maxiter 50, factr 1e5, pgtol 1e-15) behind
 * acquisition_optimizer.py:66-78 (one run per anchor point) by ONE batched run: all A starts advance together, f_df is called once per
 * trial step on the rows still running -- with the device acquisitions that is one device pass per step for all anchors.  L-BFGS-B's
 * stopping tests (max |projected gradient| <= pgtol, (f_k - f_k+1) / max(|f_k|, |f_k+1|, 1) <= factr * eps, maxiter iterations, maxfun >= 0
 * trial points per row), its first move and its curvature test; m curvature pairs per row, Armijo constant c1 and at most max_ls trial
 * steps per iteration along the projection arc.  f_df(user, Z (n x d), rows (n: which start each row of Z belongs to), n, d, f_out (n),
 * g_out (n x d)) returns 0, or non-zero to abort (the call then returns 2).  X0, X_out: A x d; lo, hi: d (infinite allowed);
 * F_out: A; calls_out[2] = callbacks, points evaluated; iters_out[A] = iterations per start.  Returns 0, 1 (bad argument) or 2. */
typedef int (*bocf_fdf_callback)(void* user, const double* Z, const int* rows, int n, int d, double* f_out, double* g_out);
int bocf_lbfgsb_batched(bocf_fdf_callback f_df, void* user, const double* X0, int A, int d, const double* lo, const double* hi, int maxiter,
                        int m, double factr, double pgtol, int max_ls, double c1, int maxfun, double* X_out, double* F_out,
                        long long* calls_out, int* iters_out);

/* ---- the same refinement with the loop on the device.  The rows of X0 (A, d), 1 <= A <= 64, are clamped into the
 * box lo, hi (d; infinite allowed, lo <= hi) and become the resident candidate batch; every pass enqueues the posterior with its input
 * gradients and the acquisition of the resident rows -- what bocf_acq_linear_grad (form BOCF_REFINE_LINEAR, `kind` = BOCF_ACQ_EI / _PI;
 * theta (L, m), the utility arguments before it are ignored) or bocf_acq_mc_grad (form BOCF_REFINE_MC; `kind` ignored; the utility block as
 * there, a resident utility program included) enqueue -- and one launch that advances every running row by one evaluation of the state
 * machine of csrc/refine_step.h (minimising -acq: the algorithm, settings and stopping tests of bocf_lbfgsb_batched, maxfun < 0 = none)
 * and writes its next trial point into the resident rows.  No callback, no per-pass copy: after every poll_every >= 1 passes the host
 * reads one word (rows still running) and stops enqueueing at zero or when the pass budget min(1 + maxiter max_ls, maxfun + max_ls) is
 * spent; rows are frozen once stopped, so the results do not depend on poll_every.  A batch of more than 16 rows is predicted twice per
 * pass (the whole batch, and its first 16 running rows, read once no more run; the whole batch is dropped once a poll shows that no more
 * run), so that every point goes through the kernels the host loop would use for it: about 0.7 ms instead of 0.13 ms per pass at N = 1024
 * until then (DESIGN.md section 19 has the figures).  X_out (A, d), F_out (A) = -acq there; iters_out,
 * nfun_out (evaluations), reason_out (A each, or NULL): per row, reason one of RefineReason of csrc/refine_step.h (1 pgtol, 2 relative
 * decrease, 3 arc search failed, 4 maxiter, 5 maxfun, 6 non-finite start, 7 NaN gradient); counters_out[2] (or NULL) = passes enqueued,
 * host synchronisations.  Afterwards the resident candidates are the final points and the context serves no acquisition vector.  Every
 * refusal of an argument names bocf_refine_acq and happens before the context is touched (the resident batch is replaced last of the
 * steps that can fail before the first launch). */
enum { BOCF_REFINE_LINEAR = 0, BOCF_REFINE_MC = 1 };
#define BOCF_REFINE_MAX_ROWS 64
int bocf_refine_acq(bocf_ctx* ctx, int form, int kind, int util_kind, const double* util_params, int n_util_params, const double* theta,
                    int theta_dim, const double* prob, int L, const double* X0, int A, const double* lo, const double* hi, int maxiter, int m,
                    double factr, double pgtol, int max_ls, double c1, int maxfun, int poll_every, double* X_out, double* F_out,
                    int* iters_out, int* nfun_out, int* reason_out, long long* counters_out);

/* ---- leave-one-out cross-validation of the resident model (ExactGaussianInference.LOO,
 * GPy/inference/latent_function_inference/exact_gaussian_inference.py:67-79).  For factorization j with the fit's own
 * Ky = K + (noise_j + 1e-8 + jitter_j) I, yc = y - ymean_j (the centre and the hyper-parameters are held when a point is left out, as
 * GPy's LOO holds them), alpha = Ky^-1 yc, c_i = (Ky^-1)_ii = sum_{k >= i} R[i][k]^2 from the resident inverse factor, shift = 1e-8 + jitter_j:
 *   mu_loo[i]  = y_i - alpha_i / c_i
 *   var_loo[i] = 1 / c_i - shift              with BOCF_ADD_NOISE (the likelihood noise stays in), - noise_j more without;
 *                                             clipped at 1e-10 under BOCF_CLIP: the flags mean what they mean for a prediction
 *   lpd[i]     = -0.5 log 2 pi + 0.5 log c_i - 0.5 alpha_i^2 / c_i      (:73-79 to the letter: nothing removed from 1 / c_i)
 *   lpd_sum[j] = sum_{i < N} lpd[i]           (summed in a fixed order)
 * for all M = H m resident factorizations, hyper-sample-major: mean_out, var_out, lpd_out (M,N), lpd_sum_out (M), each or all NULL.  One
 * pass over the upper triangles of R instead of N refits; two calls give the same bits.
 *
 * bocf_loo_utility: val_out (L,N), entry (l, i) = E[U(theta_l, y)], y ~ N(mu_loo[:, i], diag var_loo[:, i]) over the outputs of hyper-sample
 * `group` (0 .. H - 1) -- the cross-validated prediction of the composite objective at training point i.  `mode` as for the expected
 * utility of the recommendation step (BOCF_EU_MEAN / _CLOSED / _MC); the Monte-Carlo mode reads the normals of the eu-sample upload and
 * returns the MEAN over its S samples (not that entry point's sum); utility kind BOCF_UTIL_PROGRAM evaluates the resident program
 * (Monte-Carlo mode).  L <= 32.  The Monte-Carlo mode takes square roots of the variances: pass BOCF_CLIP.
 *
 * Both work on a fitted model -- also after an append, after new targets, on a jittered and on an output-sharded fit --, are local to the
 * context, recompute what they read from R and alpha in every call, keep their results in buffers of their own (the predict, candidate,
 * acquisition, sample, best-so-far, reference, pending, Thompson and path state is left as it was) and synchronise once.  < 0 with the
 * entry point's name in the error text, the context still usable: null or unfitted context (a fused inference leaves none), a host-given
 * posterior, unknown flags, a bad group, a bad utility block. */
int bocf_loo(bocf_ctx* ctx, int flags, double* mean_out, double* var_out, double* lpd_out, double* lpd_sum_out);
int bocf_loo_utility(bocf_ctx* ctx, int group, int flags, int mode, int util_kind, const double* util_params, int n_util_params,
                     const double* theta, int theta_dim, int L, double* val_out);

/* ---- quantile and tail-mean acquisitions of the composite utility.  U o f is not Gaussian, so a confidence bound or a
 * risk measure of U(theta, f(x)) has no closed form; the estimator is an order statistic of the Monte-Carlo samples uEI already draws.
 * Per candidate x, hyper-sample and utility parameter theta_l:
 *   u_s      = U(theta_l, mu(x) + sigma(x) o W_s),  s = 0 .. S - 1      mu, sigma exactly the posterior bocf_acq_mc reads (variance with noise,
 *                                                                      clipped at 1e-10), W the resident samples of bocf_set_mc_samples
 *   order    : by value ascending, then by sample index ascending; a NaN utility ranks -- and counts -- as -inf (the convention of the
 *              top-k kernels), and -0.0 is +0.0 (equal as numbers: the index decides between them)
 *   u_(k)    = the sample with exactly k samples before it in that order, s*(k) its index, k an integer rank in [0, S - 1]
 *   rho      = u_(k)                                   BOCF_RISK_QUANTILE
 *            = mean of u_(k) .. u_(S-1), S - k terms    BOCF_RISK_UPPER_TAIL
 *            = mean of u_(0) .. u_(k),   k + 1 terms    BOCF_RISK_LOWER_TAIL   (the conditional value at risk)
 *   alpha(x) = (1/Ha) sum_h sum_l p_l rho_hl(x)         hyper-sample loop of bocf_acq_mc (options acq_hyper_samples); prob NULL = 1 / L
 * The caller turns a level beta into the rank; the ABI takes the integer only, so no floating floor is computed twice.  The gradient is
 * pathwise over the selected set T ({s*(k)} for the quantile, the tail's index set for the tail kinds):
 *   d rho / dx_q = (1/|T|) sum_{s in T} sum_j dU/dy_j(y_s) (dmu_j/dx_q + W_sj / (2 sigma_j) dsigma^2_j/dx_q)
 * -- the per-sample term bocf_acq_mc_grad accumulates for improving samples.  There is no incumbent: option best_group is not read and the
 * best-so-far cache of the improvement acquisitions is left as it was.  The selection is exact (no interpolation between order statistics)
 * and independent of how the samples are spread over the hardware.  S <= 4096.
 *
 * bocf_acq_risk: alpha of every resident candidate into acq_out (C) or NULL -- the values are left as the context's acquisition vector, so
 *   bocf_select_topk and bocf_global_topk work on them; dacq_out (C, d) or NULL = value only.  BOCF_UTIL_PROGRAM is refused; the gradient
 *   form is refused on a bocf_set_posterior context and for d > 64.
 * bocf_acq_linear_ucb: the closed form for the linear utility theta^T f (GP-UCB; GPyOpt's AcquisitionLCB with the sign of a maximiser),
 *   alpha(x) = (1/Ha) sum_h sum_l p_l [ theta_l^T mu + kappa sqrt(sum_j theta_lj^2 var_j) ],
 *   d alpha / dx_q: theta^T dmu/dx_q + kappa (sum_j theta_j^2 dvar_j/dx_q) / (2 sqrt(sum_j theta_j^2 var_j));
 *   theta (L, m'), m' the outputs per hyper-sample; kappa finite (kappa = 0 is theta^T mu, negative kappa the lower bound).
 * fp64.  One stream, one synchronisation per call.  Every failure returns < 0 with the entry point's name in the error text: unfitted model,
 * no resident samples, rank outside [0, S - 1], unknown kind, S > 4096, a utility program, a bad utility block, d > 64 with gradients, a
 * non-finite kappa; the checks that need no context run before it is touched. */
enum { BOCF_RISK_QUANTILE = 0, BOCF_RISK_UPPER_TAIL = 1, BOCF_RISK_LOWER_TAIL = 2 };
#define BOCF_RISK_MAX_SAMPLES 4096
int bocf_acq_risk(bocf_ctx* ctx, int kind, int rank, int util_kind, const double* util_params, int n_util_params, const double* theta,
                  int theta_dim, const double* prob, int L, double* acq_out, double* dacq_out);
int bocf_acq_linear_ucb(bocf_ctx* ctx, double kappa, const double* theta, const double* prob, int L, double* acq_out, double* dacq_out);

/* ---- log-space expected improvement (Ament et al. 2023, "Unexpected Improvements to Expected Improvement").  Where the
 * incumbent is hard to beat, EI and its gradient are exactly zero in floating point and a selection or a refinement works on a plateau;
 * these forms have EI's maximisers but are finite with a useful gradient everywhere.  The incumbents best_l, the posterior (variance with
 * noise, clipped at 1e-10), the hyper-sample loop (options acq_hyper_samples, best_group) and the weights p_l (1 / L when prob is NULL) are
 * exactly those of bocf_acq_linear / bocf_acq_mc; H is the number of hyper-samples the loop walks.
 *
 * bocf_acq_log_linear: the closed form for the linear utility theta^T f, theta (L, m'), m' the outputs per hyper-sample.  Per (h, l):
 *   mu = theta_l^T mu_h,  sigma = sqrt(sum_j theta_lj^2 var_hj),  z = (mu - best_l) / sigma   (no floor on sigma, in value and gradient alike)
 *   l_lh = log sigma + log h(z),  h(z) = phi(z) + z Phi(z)
 *   log alpha(x) = LSE_(h, l) [ log p_l - log H + l_lh ]
 *   d log alpha  = sum_(h, l) w_lh (dsigma / sigma + r(z) (dmu - z dsigma) / sigma),  r = Phi / h, w_lh the softmax weights
 *   log h and r are accurate for every finite z: for z <= -1 through erfcx, from |z| = 30 on through the asymptotic series of 1 - |z| Phi / phi.
 *   A term with p_l = 0 or sigma = 0 is -inf and carries no weight; if every term is -inf the value is -inf and the gradient 0, never NaN.
 *
 * bocf_acq_log_mc: the Monte-Carlo form for a composite utility (compiled-in kinds and BOCF_UTIL_PROGRAM), samples y_hs = mu_h + sigma_h o W_s
 *   of the resident normals (bocf_set_mc_samples), temperature tau > 0 in the units of the utility:
 *   t = (U(theta_l, y_hs) - best_l) / tau,  psi(t) = softplus(t) + 0.1 / (1 + t^2)
 *   log alpha_tau(x) = LSE_(h, l, s) [ log p_l - log(H S) + log tau + log psi(t) ]
 *   psi is monotone and its logarithm finite for every finite t; 0 < psi(t) - max(t, 0) <= ln 2 + 0.1, so
 *   0 < exp(log alpha_tau) - alpha_EI <= tau (ln 2 + 0.1) with alpha_EI what bocf_acq_mc returns.  The gradient is pathwise through y, the
 *   per-sample weight being the softmax weight times psi'(t) / (tau psi(t)) times dU/dy_j.  A sample whose utility is NaN or infinite
 *   carries no weight.
 *
 * Both: log alpha of every resident candidate into acq_out (C) or NULL -- the values are left as the context's acquisition vector, so
 * bocf_select_topk and bocf_global_topk work on them; dacq_out (C, d) or NULL = value only.  The sums run in a fixed order: a candidate's bits
 * do not depend on its batch.  Parameters and incumbents live in buffers of their own: a bocf_acq_linear / bocf_acq_mc call after one of
 * these returns the bits it returns without it.  fp64.  One stream, one synchronisation per call.  Every failure returns < 0 with the
 * entry point's name in the error text: unfitted model, tau not finite or <= 0, unknown utility kind, no resident samples, L outside
 * 1 .. 32, a bad utility block, no or a mismatching resident program, no candidates, a gradient on a bocf_set_posterior context or for
 * d > 64; the checks that need no context run before it is touched. */
int bocf_acq_log_linear(bocf_ctx* ctx, const double* theta, const double* prob, int L, double* acq_out, double* dacq_out);
int bocf_acq_log_mc(bocf_ctx* ctx, double tau, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                    const double* prob, int L, double* acq_out, double* dacq_out);

#ifdef __cplusplus
}
#endif
#endif
