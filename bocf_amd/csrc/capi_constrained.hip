// Constrained-acquisition entry points of the C ABI (include/bocf_hip.h): bocf_set_output_constraints, bocf_feasible_best,
// bocf_acq_mc_constrained -- the Monte-Carlo expected improvement of the composite utility with K <= 8 linear constraints on the outputs
// weighing every sample (kernels: cacq.hip).  The posterior is the one bocf_acq_mc reads (the predict pass's plan and chunking, variance
// with noise, clipped), the hyper-sample loop runs here under options acq_hyper_samples / best_group, the value is left as the context's
// acquisition vector for the selections.  The constraints do not depend on the factor: nothing here calls a drop function, and no fit,
// data change or candidate upload forgets them.  The feasible incumbent is computed per call into buffers of this path (the
// acquisitions' parameter and best-so-far caches are left as they were).  One stream, one synchronisation per call.
// Below them the feasibility-aware recommendation step (kernels: ceu.hip): bocf_train_utility_range and
// bocf_expected_utility_constrained -- bocf_expected_utility's Monte-Carlo form, posterior (no likelihood noise, clipped) and hyper-sample
// rules with every sample weighed by the same phi; their argument checks are ceu_args.h's and run before the context is touched.
#include "bocf_ctx.h"
#include "ceu_args.h"

#include <cmath>
#include <cstring>
#include <vector>

extern "C" int bocf_set_output_constraints(bocf_ctx* c, const double* A, const double* b, const double* eta, int K, int m) {
  static const char* who = "bocf_set_output_constraints";
  // (the argument checks come first: they need no context, so no GPU)
  if (K == 0) {                                              // drop them
    if (!c) return fail(who, "null context");
    c->cq_K = 0;
    return 0;
  }
  if (K < 1 || K > BOCF_MAX_CONSTRAINTS) return fail(who, "K out of range (1 .. 8; 0 drops the constraints)");
  if (m < 1 || m > BOCF_MAX_M) return fail(who, "m out of range (1 .. 16)");
  if (!A || !b || !eta) return fail(who, "null A, b or eta");
  for (int i = 0; i < K * m; ++i)
    if (!std::isfinite(A[i])) return fail(who, "A has a non-finite entry");
  for (int k = 0; k < K; ++k) {
    if (!std::isfinite(b[k])) return fail(who, "b has a non-finite entry");
    if (!std::isfinite(eta[k]) || !(eta[k] > 0.0)) return fail(who, "eta must be finite and > 0");
  }
  if (!c) return fail(who, "null context");
  if (c->fitted) {
    const int H = c->hyper_samples > 0 ? c->hyper_samples : 1;
    if (c->m % H == 0 && c->m / H != m) return fail(who, "m differs from the outputs per hyper-sample of the fitted model");
  }
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> tab((size_t)K * m + 2 * (size_t)K);
  memcpy(tab.data(), A, sizeof(double) * (size_t)K * m);
  for (int k = 0; k < K; ++k) {
    tab[(size_t)K * m + k] = b[k];
    tab[(size_t)K * m + K + k] = 1.0 / eta[k];
  }
  if (c->cq_tab.ensure(sizeof(double) * ((size_t)BOCF_MAX_CONSTRAINTS * BOCF_MAX_M + 2 * BOCF_MAX_CONSTRAINTS))) return -1;
  c->cq_K = 0;                                               // (replaced below, or gone if this call fails)
  HIPCHK(hipMemcpyAsync(c->cq_tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->cq_K = K;
  c->cq_m = m;
  return 0;
}

// theta | prob | utility parameters in one upload; the incumbent buffers
static int constrained_upload(bocf_ctx* c, const UtilArgs& u, int Ha) {
  if (c->cq_best.ensure(sizeof(double) * (size_t)Ha * u.L) || c->cq_nf.ensure(sizeof(long long) * (size_t)Ha)) return -1;
  return bocf_upload_util(c, bocf_util_pack(u, nullptr, 0, &c->util_up), &c->cq_par);
}

extern "C" int bocf_feasible_best(bocf_ctx* c, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim, int L,
                                  double* best_out, long long* n_feasible_out) {
  static const char* who = "bocf_feasible_best";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, nullptr, L};
  const int m = bocf_constrained_utility(who, bocf_call_state(c), u, true, BOCF_CACQ_NO_PROGRAM);
  if (m < 0) return -1;
  HIPCHK(hipSetDevice(c->device));
  if (constrained_upload(c, u, 1)) return -1;
  const double* par = c->cq_par.as<double>();
  const int gb = bocf_best_group_of(c, 0);
  launch_feasible_best(c->mu_train.as<double>() + (size_t)gb * m * c->N, c->N, m, util_kind, par + c->util_up.theta, theta_dim, L, par + c->util_up.params,
                       c->cq_tab.as<double>(), c->cq_K, c->cq_best.as<double>(), c->cq_nf.as<long long>(), c->stream);
  long long nf = 0;
  std::vector<double> best(L);
  HIPCHK(hipMemcpyAsync(best.data(), c->cq_best.p, sizeof(double) * L, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&nf, c->cq_nf.p, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  if (best_out) memcpy(best_out, best.data(), sizeof(double) * L);
  if (n_feasible_out) *n_feasible_out = nf;
  return 0;
}

extern "C" int bocf_acq_mc_constrained(bocf_ctx* c, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                                       const double* prob, int L, double* acq_out, double* dacq_out) {
  static const char* who = "bocf_acq_mc_constrained";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, prob, L};
  const bool grad = dacq_out != nullptr;
  const int m = bocf_cacq_check(who, bocf_call_state(c), u, grad);
  if (m < 0) return -1;
  const int Ha = bocf_acq_hyper_count(c);
  HIPCHK(hipSetDevice(c->device));
  if (constrained_upload(c, u, Ha)) return -1;
  c->have_acq = false;
  if (bocf_acq_posterior(c, grad)) return -1;
  const double* par = c->cq_par.as<double>();
  CacqArgs a{};
  a.ld = c->pred_cap; a.m = m; a.C = c->C; a.L = L; a.S = c->S_mc; a.K = c->cq_K; a.util_kind = util_kind; a.theta_dim = theta_dim;
  a.theta = par + c->util_up.theta; a.prob = par + c->util_up.prob; a.util_params = par + c->util_up.params;
  a.Wt = c->Wt.as<double>(); a.tab = c->cq_tab.as<double>(); a.acq = c->acq.as<double>(); a.scale = 1.0 / Ha;
  if (grad) { a.ldg = c->pred_cap; a.d = c->d; a.dacq = c->dacq.as<double>(); }
  // the hyper-sample loop of bocf_acq_mc: hyper-sample h reads rows [h m, (h + 1) m) of the posterior and adds its share; the incumbent
  // is each hyper-sample's own, or that of option best_group for all
  for (int h = 0; h < Ha; ++h) {
    const int slot = c->best_group >= 0 ? 0 : h;
    double* best = c->cq_best.as<double>() + (size_t)slot * L;
    long long* nf = c->cq_nf.as<long long>() + slot;
    PhaseTimer t(c, "acq");
    if (h == 0 || c->best_group < 0) {
      const int gb = bocf_best_group_of(c, h);
      launch_feasible_best(c->mu_train.as<double>() + (size_t)gb * m * c->N, c->N, m, util_kind, a.theta, theta_dim, L, a.util_params, a.tab, a.K, best, nf,
                           c->stream);
    }
    a.best = best; a.nfeas = nf;
    bocf_posterior_rows(c, h, m, grad, &a);
    a.accumulate = h > 0;
    if (grad) launch_cacq_grad(a, c->stream);
    else launch_cacq(a, c->stream);
  }
  return bocf_acq_finish(c, acq_out, dacq_out);
}

// ---- the feasibility-aware recommendation step ------------------------------------------------------------------------------------------
extern "C" int bocf_train_utility_range(bocf_ctx* c, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim, int L,
                                        double* min_out, double* max_out) {
  static const char* who = "bocf_train_utility_range";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, nullptr, L};
  const int m = bocf_constrained_utility(who, bocf_call_state(c), u, false, BOCF_CEU_NO_PROGRAM);
  if (m < 0) return -1;
  if (!min_out || !max_out) return fail(who, "null min_out / max_out");
  HIPCHK(hipSetDevice(c->device));
  const UtilPack& pk = bocf_util_pack(u, nullptr, 0, &c->util_up);
  if (c->cu_rng.ensure(sizeof(double) * 2 * (size_t)L) || bocf_upload_util(c, pk, &c->cu_par)) return -1;
  const double* par = c->cu_par.as<double>();
  double* rng = c->cu_rng.as<double>();
  const int gb = bocf_best_group_of(c, 0);
  launch_train_utility_range(c->mu_train.as<double>() + (size_t)gb * m * c->N, c->N, m, util_kind, par + pk.theta, theta_dim, L, par + pk.params, rng, rng + L,
                             c->stream);
  return bocf_copy_pair_out(c, rng, min_out, sizeof(double) * L, rng + L, max_out, sizeof(double) * L);
}

extern "C" int bocf_expected_utility_constrained(bocf_ctx* c, int util_kind, const double* util_params, int n_util_params, const double* theta,
                                                 int theta_dim, int L, const double* u_infeasible, const int* row_param, int n_hyps, double* val_out,
                                                 double* pof_out, double* grad_out) {
  static const char* who = "bocf_expected_utility_constrained";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, nullptr, L};
  const CallState st = bocf_call_state(c);
  const int m = bocf_constrained_utility(who, st, u, true, BOCF_CEU_NO_PROGRAM);
  if (m < 0) return -1;
  const bool grad = grad_out != nullptr;
  const int rc = bocf_ceu_check_call(who, st, u, m, u_infeasible, row_param, n_hyps, val_out, grad);
  if (rc) return rc < 0 ? -1 : 0;
  HIPCHK(hipSetDevice(c->device));
  const int C = c->C, d = c->d;
  // theta | prob | utility parameters | u0 (L) | rows (C ints) in one block, one upload
  const size_t nrow = ((size_t)C + 1) / 2;
  c->cu_tail.assign((size_t)L + nrow, 0.0);
  memcpy(c->cu_tail.data(), u_infeasible, sizeof(double) * L);
  memcpy(c->cu_tail.data() + L, row_param, sizeof(int) * (size_t)C);
  const UtilPack& pk = bocf_util_pack(u, c->cu_tail.data(), c->cu_tail.size(), &c->util_up);
  if (c->cu_val.ensure(sizeof(double) * (size_t)C) || c->cu_pof.ensure(sizeof(double) * (size_t)C) ||
      (grad && c->cu_grad.ensure(sizeof(double) * (size_t)C * d)) || bocf_upload_util(c, pk, &c->cu_par))
    return -1;
  if (bocf_eu_posterior(c, grad)) return -1;
  const double* par = c->cu_par.as<double>();
  const int H = c->hyper_samples;
  const int nh = H == 1 ? 1 : n_hyps;             // the hyper-sample rules of bocf_expected_utility
  CeuArgs a{};
  a.val = c->cu_val.as<double>(); a.pof = c->cu_pof.as<double>(); a.grad = grad ? c->cu_grad.as<double>() : nullptr;
  a.ld = c->pred_cap; a.ldg = c->pred_cap; a.d = d;
  a.m = m; a.C = C; a.S = c->eu_S; a.K = c->cq_K; a.util_kind = util_kind; a.theta_dim = theta_dim;
  a.theta = par + pk.theta; a.util_params = par + pk.params; a.u0 = par + pk.tail;
  a.rows = reinterpret_cast<const int*>(par + pk.tail + L);
  a.Zt = c->eu_Z.as<double>(); a.tab = c->cq_tab.as<double>();
  a.scale = H == 1 ? (double)n_hyps : 1.0;
  a.pscale = 1.0 / ((double)nh * (double)c->eu_S);
  for (int h = 0; h < nh; ++h) {
    bocf_posterior_rows(c, h, m, grad, &a);
    a.accumulate = h > 0;
    PhaseTimer t(c, "ceu");
    launch_ceu(a, grad, c->stream);
  }
  // the feasibility is enqueued behind the kernels; the pair's one synchronisation covers it
  if (pof_out) HIPCHK(hipMemcpyAsync(pof_out, c->cu_pof.p, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, c->stream));
  return bocf_copy_pair_out(c, c->cu_val.p, val_out, sizeof(double) * (size_t)C, c->cu_grad.p, grad_out, grad ? sizeof(double) * (size_t)C * d : 0);
}
