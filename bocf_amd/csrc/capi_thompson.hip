// Joint posterior and composite Thompson sampling entry points of the C ABI (include/bocf_hip.h): bocf_posterior_cov,
// bocf_posterior_samples, bocf_thompson_select.  The kernels are thompson.hip; V = R^T K(X, X.) comes from the predict path's cross kernel
// and fp64 GEMM, the factorization of Sigma from the fit's planned Cholesky schedules (capi_chol.hip) run on a helper context.
#include "bocf_ctx.h"

#include <cstring>
#include <vector>

void bocf_thompson_drop(bocf_ctx* c) {
  for (int& s : c->ts_S) s = 0;
}

static int check_workspace(bocf_ctx* c, const char* who, int mg, long rows, long cols) {
  const double bytes = (double)mg * (double)rows * (double)cols * sizeof(double);
  if (bytes > (double)c->workspace_mb * 1048576.0) return fail(who, "the covariance matrices exceed option workspace_mb: fewer candidates or a larger cap");
  return 0;
}

// V = R^T K(X, Xq) for the mg outputs from j0 (Np x npad per output, k-major) and, with mu != nullptr, the posterior mean at Xq (mg x npad)
int bocf_enqueue_V(bocf_ctx* c, int j0, int mg, const double* Xq, int n, int npad, double* V, double* mu) {
  const int N = c->N, Np = c->Np, nrt = Np / BOCF_TILE;
  const long strideS = (long)Np * Np;
  const size_t plane = (size_t)mg * nrt * npad;
  if (c->ts_K.ensure(sizeof(double) * (size_t)mg * Np * npad) || c->ts_mp.ensure(sizeof(double) * 2 * plane)) return -1;
  const int* kids = BOCF_KIDS(c);
  launch_cross_kernel(c->Xs.as<double>() + (long)j0 * c->xs_stride, c->xs_stride, N, Np, c->d, c->kernel_id, c->hypd.as<KernHyp>() + j0, Xq, 0, n, npad,
                      c->alpha.as<double>() + (long)j0 * Np, c->ts_K.as<double>(), npad, (long)Np * npad, c->ts_mp.as<double>(), c->ts_mp.as<double>() + plane,
                      nsplit_for(Np, npad, mg), mg, 1, c->stream, kids ? kids + j0 : nullptr);
  if (mu)
    launch_finalize_mean(c->ts_mp.as<double>(), c->ts_mp.as<double>() + plane, nrt, npad, c->hypd.as<KernHyp>() + j0, mu, npad, 0, n, mg, c->stream);
  GemmArgs v{};
  v.A = c->R.as<double>() + (long)j0 * strideS; v.lda = Np; v.strideA = strideS;
  v.B = c->ts_K.as<double>(); v.ldb = npad; v.strideB = (long)Np * npad;
  v.Cin = nullptr; v.Cout = V; v.ldc = npad; v.strideC = (long)Np * npad;
  v.M = Np; v.Ncols = npad; v.K = Np; v.kb = BOCF_TILE; v.krt = BOCF_TILE; v.rt_desc = 1; v.alpha = 1.0;
  launch_gemm_f64(v, mg, 0, c->stream);
  return 0;
}

extern "C" int bocf_posterior_cov(bocf_ctx* c, const double* X1, int n1, const double* X2, int n2, int group, double* cov_out) {
  static const char* who = "bocf_posterior_cov";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  if (!X1 || !X2 || !cov_out) return fail(who, "null argument");
  if (n1 < 1 || n2 < 1) return fail(who, "n1 and n2 must be >= 1");
  int j0, mg, per;
  if (bocf_group_range(who, bocf_call_state(c), group, &j0, &mg, &per)) return -1;
  const int d = c->d, Np = c->Np;
  const int n1p = round_up(n1, BOCF_TILE), n2p = round_up(n2, BOCF_TILE);
  if (check_workspace(c, who, mg, n1p, n2p)) return -1;
  HIPCHK(hipSetDevice(c->device));
  if (c->ts_X.ensure(sizeof(double) * (size_t)(n1 + n2) * d) || c->ts_V.ensure(sizeof(double) * (size_t)mg * Np * (n1p + n2p)) ||
      c->ts_out.ensure(sizeof(double) * (size_t)mg * n1p * n2p))
    return -1;
  double* x1 = c->ts_X.as<double>();
  double* x2 = x1 + (size_t)n1 * d;
  double* V1 = c->ts_V.as<double>();
  double* V2 = V1 + (size_t)mg * Np * n1p;
  HIPCHK(hipMemcpyAsync(x1, X1, sizeof(double) * (size_t)n1 * d, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(x2, X2, sizeof(double) * (size_t)n2 * d, hipMemcpyHostToDevice, c->stream));
  {
    PhaseTimer t(c, "post_cov");
    if (bocf_enqueue_V(c, j0, mg, x1, n1, n1p, V1, nullptr) || bocf_enqueue_V(c, j0, mg, x2, n2, n2p, V2, nullptr)) return -1;
    const int* kids = BOCF_KIDS(c);
    launch_post_cov(V1, n1p, (long)Np * n1p, V2, n2p, (long)Np * n2p, x1, n1, x2, n2, d, Np, c->kernel_id, kids ? kids + j0 : nullptr,
                    c->hypd.as<KernHyp>() + j0, nullptr, 0, c->ts_out.as<double>(), n2p, (long)n1p * n2p, mg, c->stream);
  }
  for (int j = 0; j < mg; ++j)
    HIPCHK(hipMemcpy2DAsync(cov_out + (size_t)j * n1 * n2, sizeof(double) * n2, c->ts_out.as<double>() + (size_t)j * n1p * n2p, sizeof(double) * n2p,
                            sizeof(double) * n2, n1, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  return 0;
}

// The helper context that factorizes Sigma: the fit's schedules on its own S / E / ET / info and schedule history, created on first use.
// It factorizes only -- no inverse is wanted: the one-launch team schedules (which invert as they factor), the hybrid schedule and the
// early inverse are switched off, so the launched or reserved-CU schedules run.
static bocf_ctx* thompson_helper(bocf_ctx* c) {
  if (!c->ts_helper) {
    if (bocf_create(c->device, &c->ts_helper)) return nullptr;
    c->ts_helper->chol.team_hybrid = 0;
    c->ts_helper->chol.overlap_inverse = 0;
    c->ts_helper->chol.team_fit = 0;
  }
  return c->ts_helper;
}

// the helper's work is enqueued on the caller's stream (one order for everything, phases timed on the caller's events)
struct BorrowStream {
  bocf_ctx* h;
  hipStream_t own;
  BorrowStream(bocf_ctx* helper, hipStream_t s) : h(helper), own(helper->stream) { h->stream = s; }
  ~BorrowStream() { h->stream = own; }
};

extern "C" int bocf_posterior_samples(bocf_ctx* c, int group, const double* Z, int S, int max_jitter_tries, double* samples_out, double* jitter_out) {
  static const char* who = "bocf_posterior_samples";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  if (!Z) return fail(who, "null Z");
  if (S < 1 || S > 256) return fail(who, "S out of range (1 .. 256)");
  const int C = c->C;
  if (C < 1) return fail(who, "no resident candidates (bocf_set_candidates)");
  int j0, mg, per;
  if (bocf_group_range(who, bocf_call_state(c), group, &j0, &mg, &per)) return -1;
  const int H = c->m / per, h0 = group < 0 ? 0 : group, h1 = group < 0 ? H : group + 1;
  const int d = c->d, Np = c->Np, Cp = round_up(C, BOCF_TILE), nbc = Cp / BOCF_TILE;
  const long strideS = (long)Cp * Cp;
  if (check_workspace(c, who, mg, Cp, Cp)) return -1;
  HIPCHK(hipSetDevice(c->device));
  if ((int)c->ts_S.size() != H) {                          // (another hyper-sample count than the last call's)
    for (DevBuf& b : c->ts_F) b.release();
    c->ts_S.assign(H, 0);
    c->ts_F.assign(H, DevBuf{});
  }
  for (int h = h0; h < h1; ++h) c->ts_S[h] = 0;            // (replaced below, or gone if this call fails)
  bocf_ctx* hc = thompson_helper(c);
  if (!hc) return -1;
  HIPCHK(hipSetDevice(c->device));
  if (c->ts_V.ensure(sizeof(double) * (size_t)mg * Np * Cp) || c->ts_mu.ensure(sizeof(double) * (size_t)mg * Cp) ||
      c->ts_Z.ensure(sizeof(double) * (size_t)mg * C * S) || c->ts_jit.ensure(sizeof(double) * 2 * mg) ||
      hc->S.ensure(sizeof(double) * strideS * mg) || hc->E.ensure(sizeof(double) * (size_t)mg * nbc * BOCF_TILE * BOCF_TILE) ||
      hc->ET.ensure(sizeof(double) * (size_t)mg * nbc * BOCF_TILE * BOCF_TILE) || hc->info.ensure(sizeof(int) * (mg + 1)))
    return -1;
  for (int h = h0; h < h1; ++h)
    if (c->ts_F[h].ensure(sizeof(double) * (size_t)per * C * S)) return -1;
  HIPCHK(hipMemcpyAsync(c->ts_Z.p, Z, sizeof(double) * (size_t)mg * C * S, hipMemcpyHostToDevice, c->stream));
  hc->N = C; hc->Np = Cp; hc->m = mg; hc->d = d; hc->sched_m = 0;
  BorrowStream borrow(hc, c->stream);
  const int* kids = BOCF_KIDS(c);
  double* jd = c->ts_jit.as<double>();
  auto build = [&](bool with_jitter) {
    PhaseTimer t(c, "post_cov");
    launch_post_cov(c->ts_V.as<double>(), Cp, (long)Np * Cp, c->ts_V.as<double>(), Cp, (long)Np * Cp, c->Xc.as<double>(), C, c->Xc.as<double>(), C, d, Np,
                    c->kernel_id, kids ? kids + j0 : nullptr, c->hypd.as<KernHyp>() + j0, with_jitter ? jd : nullptr, 1, hc->S.as<double>(), Cp, strideS, mg,
                    c->stream);
  };
  {
    PhaseTimer t(c, "post_cov");
    if (bocf_enqueue_V(c, j0, mg, c->Xc.as<double>(), C, Cp, c->ts_V.as<double>(), c->ts_mu.as<double>())) return -1;
  }
  build(false);
  // rung 0 from the mean of each Sigma_j's diagonal
  std::vector<double> jit(mg), dmean(mg);
  launch_post_diag(hc->S.as<double>(), Cp, strideS, C, 0, jd + mg, nullptr, mg, c->stream);
  HIPCHK(hipMemcpyAsync(dmean.data(), jd + mg, sizeof(double) * mg, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int j = 0; j < mg; ++j) jit[j] = 1e-8 * (dmean[j] > 1e-10 ? dmean[j] : 1e-10);
  const int rungs = max_jitter_tries > 1 ? max_jitter_tries : 1;
  std::vector<int> info(mg + 1, 0);
  bool rebuild = false;
  for (int attempt = 0;;) {
    HIPCHK(hipMemcpyAsync(jd, jit.data(), sizeof(double) * mg, hipMemcpyHostToDevice, c->stream));
    if (rebuild) build(true);
    else launch_post_diag(hc->S.as<double>(), Cp, strideS, C, 1, nullptr, jd, mg, c->stream);
    HIPCHK(hipMemsetAsync(hc->info.p, 0, sizeof(int) * mg, c->stream));
    {
      PhaseTimer t(c, "post_chol");
      CholPlan plan;
      if (bocf_plan_cholesky(hc, false, &plan) || bocf_run_cholesky(hc, plan)) return -1;
    }
    HIPCHK(hipMemcpyAsync(info.data(), hc->info.p, sizeof(int) * mg, hipMemcpyDeviceToHost, c->stream));
    info[mg] = 0;
    if (hc->chol_flags_used) HIPCHK(hipMemcpyAsync(&info[mg], hc->chol_flags.as<int>() + hc->chol_err_off, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    hc->chol_flags_used = 0;
    LAUNCHCHK();
    rebuild = true;
    if (info[mg]) {
      // a dependency of a multi-stream schedule timed out (fit_replicated's handling): redo this attempt single-stream
      hc->sched_timeouts++;
      if (hc->sched_timeouts >= 2) hc->gated_off = 1;
      if (hc->sched_timeouts > 8) return fail(who, "the factorization schedule keeps timing out waiting for device-side dependencies");
      hc->sched_retry = 1;
      continue;
    }
    bool bad = false;
    for (int j = 0; j < mg; ++j) bad = bad || info[j] != 0;
    if (!bad || ++attempt >= rungs) break;
    for (int j = 0; j < mg; ++j)
      if (info[j] != 0) jit[j] *= 10.0;
  }
  if (jitter_out) memcpy(jitter_out, jit.data(), sizeof(double) * mg);
  for (int j = 0; j < mg; ++j)
    if (info[j] != 0) {
      bocf_set_error("not positive definite, even with jitter.");
      return j + 1;
    }
  hc->fits_done++;
  {
    PhaseTimer t(c, "post_samples");
    for (int h = h0; h < h1; ++h) {
      const int jl = (h - h0) * per;                         // first output of hyper-sample h inside this call's mg
      launch_post_sample(hc->S.as<double>() + (long)jl * strideS, Cp, strideS, c->ts_Z.as<double>() + (size_t)jl * C * S, c->ts_mu.as<double>() + (size_t)jl * Cp,
                         Cp, C, S, c->ts_F[h].as<double>(), per, c->stream);
    }
  }
  if (samples_out)
    for (int h = h0; h < h1; ++h)
      HIPCHK(hipMemcpyAsync(samples_out + (size_t)(h - h0) * per * C * S, c->ts_F[h].p, sizeof(double) * (size_t)per * C * S, hipMemcpyDeviceToHost,
                            c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  for (int h = h0; h < h1; ++h) c->ts_S[h] = S;
  return 0;
}

extern "C" int bocf_thompson_select(bocf_ctx* c, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim, int k,
                                    long long* idx_out, double* val_out) {
  static const char* who = "bocf_thompson_select";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  int P = 0;
  for (int s : c->ts_S) P += s;
  if (P == 0) return fail(who, "no resident samples: call bocf_posterior_samples first");
  const int C = c->C, H = (int)c->ts_S.size(), per = c->m / H;
  if (k < 1 || k > 64 || k > C) return fail(who, "k out of range (1 .. min(C, 64))");
  if (!idx_out || (theta_dim > 0 && !theta) || theta_dim < 0) return fail(who, "null argument / bad theta_dim");
  if (util_kind < BOCF_UTIL_LINEAR || util_kind > BOCF_UTIL_PROGRAM) return fail(who, "unknown utility kind");
  if (n_util_params < 0 || n_util_params > BOCF_MAX_M || (n_util_params > 0 && !util_params)) return fail(who, "too many utility parameters / null");
  if (bocf_check_group_fits(who, per)) return -1;
  if (util_kind == BOCF_UTIL_PROGRAM && bocf_check_resident_program(c, who, per, theta_dim, n_util_params)) return -1;
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> par;                                   // the widened theta rows | the parameters (util_args.h)
  const int tw = bocf_util_pack_rows(theta, theta_dim, P, per, util_params, n_util_params, &par);
  const int nb = topk_num_blocks(C);
  if (c->ts_theta.ensure(sizeof(double) * (size_t)P * tw) || c->ts_params.ensure(sizeof(double) * BOCF_MAX_M) || c->ts_u.ensure(sizeof(double) * (size_t)P * C) ||
      c->ts_mp.ensure(16 * (size_t)nb * k) || c->ts_out.ensure(16 * (size_t)P * k))
    return -1;
  HIPCHK(hipMemcpyAsync(c->ts_theta.p, par.data(), sizeof(double) * (size_t)P * tw, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->ts_params.p, par.data() + (size_t)P * tw, sizeof(double) * BOCF_MAX_M, hipMemcpyHostToDevice, c->stream));
  long long* oi = c->ts_out.as<long long>();
  double* ov = reinterpret_cast<double*>(oi + (size_t)P * k);
  long long* bi = c->ts_mp.as<long long>();
  double* bv = reinterpret_cast<double*>(bi + (size_t)nb * k);
  {
    PhaseTimer t(c, "thompson_select");
    int p0 = 0;
    for (int h = 0; h < H; ++h) {
      if (c->ts_S[h] == 0) continue;
      launch_thompson_util(c->ts_F[h].as<double>(), per, C, c->ts_S[h], util_kind, c->ts_theta.as<double>() + (size_t)p0 * tw, tw, c->ts_params.as<double>(),
                           c->ts_u.as<double>() + (size_t)p0 * C, C, c->stream, &c->prog);
      p0 += c->ts_S[h];
    }
    for (int p = 0; p < P; ++p)
      launch_topk(c->ts_u.as<double>() + (size_t)p * C, C, k, bi, bv, oi + (size_t)p * k, ov + (size_t)p * k, c->stream);
  }
  HIPCHK(hipMemcpyAsync(idx_out, oi, sizeof(long long) * (size_t)P * k, hipMemcpyDeviceToHost, c->stream));
  if (val_out) HIPCHK(hipMemcpyAsync(val_out, ov, sizeof(double) * (size_t)P * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  return 0;
}
