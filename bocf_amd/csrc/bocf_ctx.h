// Context of one GPU (opaque bocf_ctx of include/bocf_hip.h) and the error plumbing shared by capi.hip and comm.hip.
#pragma once
#include "bocf_internal.h"
#include "call_args.h"
#include "chol_plan.h"
#include "predict_plan.h"
#include "../../include/bocf_hip.h"

#include <map>
#include <string>
#include <utility>
#include <vector>

void bocf_set_error(const char* text);                    // records bocf_last_error() verbatim (positive LAPACK-style returns)
int bocf_launch_status();
int bocf_plan_cholesky(bocf_ctx* c, bool kinv, CholPlan* out);   // capi_chol.hip: the schedule of the next factorization (kinv: Ky^-1 wanted), its streams and counters
int bocf_run_cholesky(bocf_ctx* c, const CholPlan& plan, bool counters_zeroed = false);   // blocked Cholesky of all outputs (counters_zeroed: by the caller's kernels)
int bocf_run_trtri(bocf_ctx* c, bool early_done);         // capi_chol.hip: R = U^-1 (the part the factorization did not already start)
int bocf_comm_broadcast(bocf_ctx* c, double* buf, size_t count, int root);   // comm.hip: ncclBroadcast on the context's stream
int bocf_comm_group(bool start);                                             // ncclGroupStart / ncclGroupEnd
int bocf_comm_abort(bocf_ctx* c);                                            // ncclCommAbort: peers fail instead of blocking
int bocf_comm_allreduce_sum(bocf_ctx* c, double* buf, size_t count);        // in place, on the context's stream
#define fail bocf_fail
#define HIPCHK(expr)                                                         \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) return fail(#expr, hipGetErrorString(e_));         \
  } while (0)
#define LAUNCHCHK()                       \
  do {                                    \
    if (bocf_launch_status()) return -1;  \
  } while (0)

// host array of the per-output kernel ids of the resident model, or nullptr when every output uses c->kernel_id
#define BOCF_KIDS(c) ((int)(c)->kernel_ids.size() == (c)->m && (c)->m > 0 ? (c)->kernel_ids.data() : nullptr)
static inline int round_up(int x, int q) { return (x + q - 1) / q * q; }
static inline int nsplit_for(int Np, int Cpad, int m) {
  const int blocks = ((Cpad + 511) / 512) * m;        // cross_kernel: 256 threads x 2 columns per workgroup
  int ns = 2048 / (blocks > 0 ? blocks : 1);
  if (ns < 1) ns = 1;
  const int maxs = Np / BOCF_TILE;
  if (ns > maxs) ns = maxs;
  return ns;
}

static_assert(PLAN_TILE == BOCF_TILE && PLAN_SMALL_N == BOCF_SMALL_N && PLAN_I8_SLICES == BOCF_I8_SLICES, "predict_plan.h mirrors bocf_internal.h");

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return fail("hipMalloc", hipGetErrorString(e));
    cap = bytes;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct bocf_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // small batches (the single points and 16-point groups of the acquisition optimiser): candidates go up and results come back through pinned
  // staging buffers -- asynchronous copies, ONE stream synchronisation per call instead of one per pageable copy
  void* pin_in = nullptr; void* pin_out = nullptr;
  size_t pin_in_cap = 0, pin_out_cap = 0;
  hipEvent_t ev_pin = nullptr;     // the upload out of pin_in has completed
  void* fit_pin = nullptr; size_t fit_pin_cap = 0;     // status words + log-marginal of a fit
  void* up_pin = nullptr; size_t up_pin_cap = 0, arena_used = 0;   // pinned arena of a fit's host-to-device copies (X, hyper-parameters, targets, jitter)
  std::vector<hipEvent_t> ev_chol;  // lookahead Cholesky: events per panel
  // Reserved-CU lookahead (run_cholesky): the serial chain of diagonal-block factorizations runs on a stream whose CU mask
  // holds `res_cus` compute units that NO other stream of the factorization may use (the trailing updates run on streams
  // masked to the complement), so a diagonal block never waits for a CU to drain and never shares one.
  hipStream_t s_res = nullptr, s_hi = nullptr, s_bulk = nullptr;
  DevBuf chol_flags;         // device-side dependency counters of the gated schedules (+ the timeout word)
  int chol_flags_used = 0;
  int chol_err_off = 0;      // index of the time-out word inside chol_flags (from the plan of the last factorization)
  CholOptions chol;          // the factorization-schedule options (chol_plan.h)
  int kinv_done = 0;         // the factorization schedule left Ky^-1 in the T scratch (an inference asked for it, bocf_plan_cholesky)
  int inverse_done = 0;      // the factorization schedule already produced R and R^T (team schedule)
  int ncu = 0;               // compute units of the device (read once, by bocf_create)
  int* tile_ctr = nullptr;   // tile-queue counters of the variance contraction (two ints, zeroed by bocf_create; every launch leaves them zeroed)
  unsigned long long* team_tl = nullptr;   // probes build: task timeline of the team kernel (tools/team_timeline.py)
  int res_cus = 0;           // CUs currently reserved by s_res (0 = streams not created)
  int cu_masks_ok = 1;       // cleared when hipExtStreamCreateWithCUMask is refused: the single-stream schedules are used
  hipStream_t s_inv = nullptr;
  hipEvent_t ev_half = nullptr, ev_inv_early = nullptr;
  int early_inverse_started = 0;
  void* zeroed_R = nullptr; void* zeroed_RT = nullptr; int zeroed_Np = 0, zeroed_m = 0;
  int gated_off = 0;         // latched by bocf_fit when a device-side dependency timed out: single-stream schedules from then on
  long long sched_timeouts = 0;   // how often that happened (bocf_get_stat "sched_timeouts")
  int sched_retry = 0;       // the next factorization attempt is the redo of one that timed out: single-stream
  long long fits_done = 0;   // successful bocf_fit calls of this context
  int last_schedule = 0;     // schedule of the last factorization (CholSchedule): 0 launched, 2 reserved CUs, 3 one team launch, 4 team panel groups, 5 hybrid
  int sched_m = 0;           // > 0: choose the schedule as for this many outputs (the helper context of an output-sharded fit)
  int force_sched_timeout = 0;   // test hook (BOCF_PROBES builds only)
  int data_N = 0, data_d = 0, data_m = 0;   // shape of the X / Y resident on the device
  int fused_infer = 1;       // bocf_infer: one fused launch for N <= 128, d <= 16
  int reuse_data = 0;        // next bocf_fit calls: X, Y (and N, d, m) are those of the previous fit -- only the hyper-parameters change
  int skip_mu_train = 0;     // do not refresh the posterior mean at the training inputs (HMC / optimiser inferences never read it)
  DevBuf gpart, gout;        // bocf_lml_gradients scratch
  DevBuf hmc_buf;            // bocf_hmc: parameters, momenta, uniforms, chains, counters
  double* infer_out = nullptr;    // host-mapped result block of the fused inference (the kernel writes it over PCIe: no D2H copy)
  size_t infer_out_cap = 0;
  // ---- fit state
  bool fitted = false;
  bool canned = false;       // bocf_set_posterior: mean / var / train mean were given by the host (acquisition kernels only)
  int N = 0, Np = 0, d = 0, m = 0, kernel_id = 0;
  long xs_stride = 0;        // per-output stride of Xs (capacity Np rows so that observations can be appended)
  std::vector<int> kernel_ids;   // per-output kernel family of the resident model when the outputs differ (else empty: all kernel_id)
  std::vector<int> pending_ids;  // bocf_set_kernel_ids: taken by the next bocf_fit / bocf_infer / bocf_hmc with as many outputs
  std::vector<KernHyp> hyp;
  std::vector<double> jitter;
  std::vector<int> last_info;  // per-output LAPACK-style info of the last bocf_fit / bocf_infer attempt (0 = factorized)
  DevBuf R32;                // fp32 copy of R for the fp32 variance contraction (option predict_f32)
  bool r32_valid = false;
  int predict_f32 = 0;
  // int8 (Ozaki) variance contraction (option predict_i8): digit fragments of R and their column exponents (per fit), of K* (per chunk), the
  // kernels' variance exponents
  DevBuf Ri8, Ri8e, Ki8, Ki8e;
  bool ri8_valid = false;
  int predict_i8 = 0, i8_group = 0;    // i8_group: 0 = XCD blocks of 4 row-tile pairs x 8 column tiles, g >= 1 = bands of g pairs (speed only)
  DevBuf X, Xs, S, R, RT, E, ET, T, yc, tvec, rvec, dvec, alpha, lml, jit, hypd, info, mu_train;
  // ---- candidates
  int C = 0;
  DevBuf Xc;
  // ---- workspace
  long chunk = 65536;
  long workspace_mb = 24576; // cap of the per-pass K* / V workspace
  DevBuf Kstar, meanpart, sumsq, mean, var, acq, Vbuf, dmean, dvar, dacq, Vs, Ws;
  int pred_cap = 0;          // columns allocated in mean/var/acq
  // ---- acquisition parameters
  DevBuf theta, prob, best, params, Wt;
  std::vector<double> last_params;   // host copy of what theta/prob/params hold (skip identical re-uploads)
  long long mu_epoch = 0;            // bumped whenever mu_train changes (fit, target refresh, append, canned posterior)
  long long best_epoch = -1; int best_sig = -1;   // what c->best was computed from: mu_epoch and (linear, utility kind, group); reset when the parameters are re-uploaded
  int S_mc = 0;
  bool have_acq = false;
  // ---- the resident utility program (bocf_set_utility_program; util_prog.hip): stays until it is replaced
  DevBuf prog_buf;
  UtilProg prog;
  DevBuf blk_idx, blk_val, out_idx, out_val;
  // ---- expected utility of the recommendation step (bocf_set_eu_samples / bocf_expected_utility): buffers of its own, so the
  // acquisition state above (acq, dacq, theta / prob / params, Wt, the best-so-far cache) is left as it was
  DevBuf eu_theta, eu_rows, eu_Z, eu_val, eu_grad;
  int eu_S = 0, eu_L = 0, eu_m = 0;  // samples per parameter, parameters and outputs per hyper-sample of eu_Z (eu_S = 0: none set)
  void* eu_pin = nullptr;            // pinned staging of theta | params | rows
  size_t eu_pin_cap = 0;
  hipEvent_t ev_eu_pin = nullptr;    // the upload out of eu_pin
  // ---- profiling of the dominant kernel
  bool profile = false;
  double test_diag_shift = 0.0;
  int prefetch1 = 0;
  int kstar_valu_probe = 0;  // timing-only experiment (gemm_f64.hip, VPROBE)
  int small_path = 1;        // GEMV-shaped path for <= 16 candidates
  int hyper_samples = 1;     // H: the m outputs are H groups (hyper-samples, group-major) of m / H model outputs
  int acq_hyper_samples = 0; // hyper-samples the acquisitions average over (0 = all; the reference uses min(10, H), maEI.py:35)
  int best_group = -1;       // -1: each hyper-sample's own best-so-far (maEI.py:88); >= 0: that group's for every h (uEI_noiseless.py:66)
  int swizzle = -1;          // variance GEMM tiling: -1 = by size (256-row three-buffer kernel from 2048 candidates per pass), 0 = 128-row tiles,
                             // 258 = 256-row tiles; probes build also 1 / 100+RT (tile orders measured slower), 256 / 257 (two-buffer kernel)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  double prof_flops = 0.0;
  std::map<std::string, std::vector<std::pair<hipEvent_t, hipEvent_t>>> phases;   // named phases (bocf_profile_phase)
  // ---- multi-GPU (comm.hip): RCCL communicator of this rank, buffers of the one collective of the path
  int shard_fit = 0;         // option: bocf_fit factorizes only this rank's share of the outputs and exchanges the inverse factors
  int shard_fit_simulate = 0;   // test hook: G > 0 = one process plays all G ranks in turn (no collectives)
  bool sharded = false;      // the current fit holds R / R^T / alpha only (no upper factor)
  bocf_ctx* shard_helper = nullptr;
  DevBuf shard_meta;
  void* comm = nullptr;      // ncclComm_t
  int world = 1, rank = 0;
  DevBuf pack, gidx, gval;
  // ---- joint posterior / composite Thompson sampling (capi_thompson.hip): buffers of their own, the predict and acquisition state is left
  // as it was.  The factorization of Sigma runs on a helper context (its S, E, ET, info, schedule state), created on first use.
  bocf_ctx* ts_helper = nullptr;
  DevBuf ts_X, ts_K, ts_V, ts_mp, ts_mu, ts_Z, ts_jit, ts_u, ts_theta, ts_params, ts_out;
  std::vector<DevBuf> ts_F;  // resident samples of hyper-sample h: (m / H, C, ts_S[h]) -- ts_S[h] = 0: none
  std::vector<int> ts_S;
  // ---- look-ahead posterior and knowledge gradient (capi_kg.hip): the resident reference set A of all m outputs -- V_A = R^T K(X, A) and
  // Wa = Ky^-1 K(X, A) (Np x nap each, nap = na rounded up to 128), mu(A), the raw sigma^2(A) (m x nap each), the conditioning nugget
  // noise + 1e-8 + jitter per output -- and the per-chunk workspaces.  Buffers of their own: the predict, acquisition, expected-utility and
  // Thompson state is left as it was (scratch shared with the joint posterior: ts_K, ts_mp)
  int kg_na = 0;             // reference points resident (0 = none)
  DevBuf kg_XA, kg_VA, kg_Wa, kg_muA, kg_s2A, kg_nug;
  DevBuf kg_V, kg_W, kg_cov, kg_s2c, kg_dcov, kg_dmean, kg_dvar, kg_par, kg_v0, kg_astar, kg_AB, kg_out, kg_dout;
  // ---- pending points of a greedy batch (capi_pending.hip): the r <= 15 points P staged like a reference set in buffers of their own
  // (the uKG reference set survives), Q = (Sigma(P, P) + tau I)^-1 (m, r, r) and the joint samples F, G (m, r, S) made on the host
  // (pending_host.h).  The per-chunk workspaces are the look-ahead's (kg_V, kg_cov, kg_s2c, kg_W, kg_dmean, kg_dvar, kg_dcov, kg_dout).
  int pd_r = 0, pd_S = 0;    // pending points resident (0 = none) and the samples F, G were made for
  DevBuf pd_XP, pd_VP, pd_Wp, pd_muP, pd_cov, pd_pack, pd_QFG, pd_par, pd_best, pd_T, pd_muc, pd_E;
  std::vector<double> pd_host, pd_up;   // Sigma(P, P) | mu(P) as copied back; Q | F | G as uploaded (kept: the upload is asynchronous)
  // ---- joint q-point acquisition (capi_joint.hip): V, Ky^-1 K*, mu, Sigma and the gradients of the chunk's points, the utility block with
  // the transposed normals behind it, the incumbents (Ha, L), the per-batch pivot counts and the gradient kernel's scratch in buffers of
  // its own.  Nothing in them outlives a call: no fit, append or candidate upload has anything to invalidate here.
  DevBuf jt_V, jt_W, jt_mu, jt_cov, jt_dmean, jt_dvar, jt_dcov, jt_par, jt_best, jt_fl, jt_E, jt_dout;
  std::vector<double> jt_tail;          // Z transposed (and the caller's incumbents) as the tail of util_up's block (kept: its capacity is reused)
  // ---- pathwise posterior samples (capi_paths.hip): per hyper-sample h one block omega (m', F, d) | phase (m', F) | w (m', F, S) |
  // v (m', Np, BOCF_TILE) with pt_S[h] paths of pt_F[h] features (pt_S[h] = 0: none); staging and per-call scratch of their own
  std::vector<DevBuf> pt_buf;
  std::vector<int> pt_S, pt_F;
  DevBuf pt_E, pt_g, pt_rhs, pt_tmp, pt_nug, pt_par, pt_rows, pt_tab, pt_pv, pt_pg, pt_val, pt_grad;
  // ---- linear output constraints of the constrained acquisition (capi_constrained.hip): the table A (K, m') | b (K) | 1 / eta (K), resident
  // until it is replaced (they do not depend on the factor: no fit, data change or candidate upload drops them); parameters, feasible
  // incumbents (Ha, L) and feasible counts (Ha) of a call in buffers of their own -- the acquisitions' parameter and best-so-far caches
  // are left as they were
  int cq_K = 0, cq_m = 0;    // constraints resident (0 = none) and the outputs per hyper-sample they were given for
  DevBuf cq_tab, cq_par, cq_best, cq_nf;
  // ---- constrained expected utility of the recommendation step (bocf_expected_utility_constrained, bocf_train_utility_range;
  // capi_constrained.hip): parameters | u0 | rows of a call, its outputs and the utility range in buffers of their own -- the acquisition
  // state, the incumbent buffers above and bocf_expected_utility's buffers are left as they were
  DevBuf cu_par, cu_val, cu_pof, cu_grad, cu_rng;
  std::vector<double> cu_tail;   // u0 (L) | row_param (C ints) as the tail of util_up's block (kept: its capacity is reused)
  // ---- device-resident anchor refinement (capi_refine.hip): the rows' state blocks of refine_step.h (doubles; ints with the running-rows
  // word, the small flag and the column map behind them); for batches above the small path the gathered running rows (rf_x2) and the
  // whole batch's acquisition and gradient kept across the second predict (rf_acq).  Nothing in them outlives a call.
  DevBuf rf_dbl, rf_int, rf_x2, rf_acq;
  // ---- leave-one-out cross-validation (capi_loo.hip): mean | variance | log density (m, Np each) and their sums (m), the per-output
  // diagonal shift, and the parameters, rows and values of bocf_loo_utility in buffers of their own.  Every call recomputes what it reads
  // from R and alpha, so no fit, append or target update has anything to invalidate here.
  DevBuf loo_out, loo_sum, loo_shift, loo_par, loo_rows, loo_val;
  std::vector<double> loo_shift_host;   // source of the shift's upload (kept: the copy is asynchronous)
  // ---- quantile / tail-mean and confidence-bound acquisitions (capi_risk.hip): theta | prob | utility parameters of a call in a buffer of
  // its own -- the parameter and best-so-far caches of the improvement acquisitions are left as they were.  Nothing in it outlives a call.
  DevBuf rk_par;
  // ---- log-space expected improvement (capi_logei.hip): theta | prob | utility parameters of a call and the incumbents (hyper-samples
  // averaged, L) in buffers of their own -- the parameter and best-so-far caches of the improvement acquisitions are left as they were.
  // Nothing in them outlives a call.
  DevBuf lg_par, lg_best;
  UtilPack util_up;         // host source of the utility block's upload (util_args.h says why it lives here); kg_par, pd_par, cq_par are its device copies
};

// hyper-samples the acquisitions average over: option acq_hyper_samples, or (0, or more than are resident) all of option hyper_samples (1 .. 64)
static inline int bocf_acq_hyper_count(const bocf_ctx* c) {
  return (c->acq_hyper_samples > 0 && c->acq_hyper_samples < c->hyper_samples) ? c->acq_hyper_samples : c->hyper_samples;
}
// whose best-so-far hyper-sample h improves on: that of option best_group for all, or (-1) its own
static inline int bocf_best_group_of(const bocf_ctx* c, int h) { return c->best_group >= 0 ? c->best_group : h; }

// util_prog.hip: what every entry point checks before it evaluates the resident program (utility kind BOCF_UTIL_PROGRAM): one is resident,
// no util_params, and it was built for these m outputs per hyper-sample and this theta_dim.  Errors name `who`.
int bocf_check_resident_program(bocf_ctx* c, const char* who, int m, int theta_dim, int n_util_params);
// the resident Thompson samples belong to one posterior and one candidate set: dropped by every fit, data change and candidate upload
void bocf_thompson_drop(bocf_ctx* c);
// the resident reference set belongs to one posterior: dropped by every fit and data change (NOT by a candidate upload)
void bocf_kg_drop(bocf_ctx* c);
// the resident pending points belong to one posterior, like the reference set: dropped wherever it is
void bocf_pending_drop(bocf_ctx* c);
// the resident paths belong to one posterior INCLUDING its targets: dropped by every fit and data change (NOT by a candidate upload)
void bocf_paths_drop(bocf_ctx* c);
// capi_kg.hip, shared with capi_pending.hip.  A staged point set of the look-ahead paths: the uKG reference set or the pending points.
struct KgRefSet { const DevBuf* XA; const DevBuf* VA; const DevBuf* Wa; int na; };
int bocf_kg_stage(bocf_ctx* c, const double* Xdev, int na, int nap, double* VA, double* Wa, double* muA, double* s2A);
int bocf_kg_chunk_size(const bocf_ctx* c, int mg);      // candidates per chunk under option workspace_mb; below 128: refuse
int bocf_kg_chunk(bocf_ctx* c, const KgRefSet& ref, int j0, int mg, int c0, int cn, int cnp, bool with_grad, double* mu);
int bocf_kg_chunk_dcov(bocf_ctx* c, const KgRefSet& ref, int j0, int mg, int c0, int cn, int a0, int an);
// capi_thompson.hip, shared with capi_kg.hip: V = R^T K(X, Xq) for the mg outputs from j0 (Np x npad per output, k-major) with, for
// mu != nullptr, the posterior mean at Xq (mg x npad)
int bocf_enqueue_V(bocf_ctx* c, int j0, int mg, const double* Xq, int n, int npad, double* V, double* mu);
// capi.hip: the posterior the Monte-Carlo acquisitions read (variance with noise, clipped at 1e-10; with grad its input gradients) of every
// resident candidate, through the predict pass's plan and chunking
int bocf_acq_posterior(bocf_ctx* c, bool grad);
// ... and the one bocf_expected_utility reads (predict_noiseless: no likelihood noise, clipped at 1e-10)
int bocf_eu_posterior(bocf_ctx* c, bool grad);
// two device vectors to the host with ONE synchronisation (either may be empty)
int bocf_copy_pair_out(bocf_ctx* c, const void* src0, double* out0, size_t b0, const void* src1, double* out1, size_t b1);
// what ends an acquisition over the resident candidates: c->acq stands for the selections, and the values (C) and gradients (C, d; either
// may be null) go to the host with ONE synchronisation
int bocf_acq_finish(bocf_ctx* c, double* acq_out, double* dacq_out);
// capi.hip, shared with capi_refine.hip: the parameter upload of bocf_acq_linear[_grad] / bocf_acq_mc[_grad] (it checks L, theta and the
// parameter count; skipped when nothing changed; *uploaded, when given, is set when it ran: one synchronisation), the part of them that
// only enqueues -- the posterior (with grad: and its gradients) and one acquisition launch per hyper-sample, into c->acq / c->dacq; the
// Monte-Carlo gradient form is BOCF_ACQ_EI -- and one device word to the host with ONE synchronisation
int bocf_acq_upload_params(bocf_ctx* c, const double* theta, int theta_dim, const double* prob, int L, const double* params, int nparams,
                           bool* uploaded = nullptr);
int bocf_acq_enqueue(bocf_ctx* c, int m, bool linear, bool grad, int kind, int util_kind, int n_util_params, int theta_dim, int L);
int bocf_copy_word_out(bocf_ctx* c, const int* dev, int* out);

// ---- what the entry points that evaluate a utility over the posterior share (call_args.h has their checks) ----------------------------------
// the plain record the checks read, on the caller's stack; a null context is all zeros: not fitted
static inline CallState bocf_call_state(const bocf_ctx* c) {
  if (!c) return CallState{};
  return CallState{c->fitted, c->canned, c->N, c->d, c->m, c->hyper_samples, c->best_group, c->C, c->S_mc, c->eu_S, c->eu_L, c->eu_m,
                   c->cq_K, c->cq_m, c->kg_na, c->pd_r, c->pd_S};
}
// The reference's h-loop (maEI.py:85-97, uEI_noiseless.py:71-82): hyper-sample h reads rows [h m, (h + 1) m) of the posterior of the resident
// candidates -- a->mean / a->var, leading dimension pred_cap, and with grad a->dmean / a->dvar (d values per column)
template <typename Args> static inline void bocf_posterior_rows(const bocf_ctx* c, int h, int m, bool grad, Args* a) {
  const size_t off = (size_t)h * m * c->pred_cap;
  a->mean = c->mean.as<double>() + off; a->var = c->var.as<double>() + off;
  if (grad) { a->dmean = c->dmean.as<double>() + off * c->d; a->dvar = c->dvar.as<double>() + off * c->d; }
}
// A packed utility block (util_args.h; its host source is c->util_up) into the calling path's OWN parameter buffer, asynchronously: the
// parameter and best-so-far caches of the improvement acquisitions are left as they were
static inline int bocf_upload_util(bocf_ctx* c, const UtilPack& pk, DevBuf* par) {
  if (par->ensure(pk.bytes())) return -1;
  HIPCHK(hipMemcpyAsync(par->p, pk.host.data(), pk.bytes(), hipMemcpyHostToDevice, c->stream));
  return 0;
}

// HIP-event bracket of a named phase on the context's stream (only with option "profile" = 1; otherwise free)
struct PhaseTimer {
  bocf_ctx* c;
  const char* name;
  hipEvent_t e0 = nullptr;
  PhaseTimer(bocf_ctx* ctx, const char* n) : c(ctx), name(n) {
    if (!c->profile) return;
    if (hipEventCreate(&e0) != hipSuccess) { e0 = nullptr; return; }
    (void)hipEventRecord(e0, c->stream);
  }
  void stop() {
    if (!e0) return;
    hipEvent_t e1 = nullptr;
    if (hipEventCreate(&e1) == hipSuccess) {
      (void)hipEventRecord(e1, c->stream);
      c->phases[name].emplace_back(e0, e1);
    } else {
      (void)hipEventDestroy(e0);
    }
    e0 = nullptr;
  }
  ~PhaseTimer() { stop(); }
};

// HIP-event bracket of the dominant kernel of a predict pass (option "profile" = 1; otherwise free): bocf_profile_read sums its time,
// counts it and adds the pass's m N^2 n flops
struct KernelTimer {
  bocf_ctx* c;
  double flops;
  hipEvent_t e0 = nullptr;
  KernelTimer(bocf_ctx* ctx, int ncols) : c(ctx), flops((double)ctx->m * (double)ctx->N * (double)ctx->N * (double)ncols) {
    if (!c->profile) return;
    if (hipEventCreate(&e0) != hipSuccess) { e0 = nullptr; return; }
    (void)hipEventRecord(e0, c->stream);
  }
  ~KernelTimer() {
    if (!e0) return;
    hipEvent_t e1 = nullptr;
    if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); return; }
    (void)hipEventRecord(e1, c->stream);
    c->events.emplace_back(e0, e1);
    c->prof_flops += flops;
  }
};
