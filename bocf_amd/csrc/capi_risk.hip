// Quantile / tail-mean and confidence-bound entry points of the C ABI (include/bocf_hip.h): bocf_acq_risk -- an exact
// order statistic, or the mean of a tail, of the Monte-Carlo samples of the composite utility -- and bocf_acq_linear_ucb, the closed form
// for a linear utility (kernels: risk.hip).  The posterior is the one bocf_acq_mc reads (the predict pass's plan and chunking, variance
// with noise, clipped), the samples are the resident ones of bocf_set_mc_samples, the hyper-sample loop runs here under option
// acq_hyper_samples, the value is left as the context's acquisition vector for the selections.  There is no incumbent: option best_group
// is not read, and the parameters go up into a buffer of this path, so the parameter and best-so-far caches of the improvement
// acquisitions are left as they were.  The checks that need no context run before it is touched.  One stream, one synchronisation per call.
#include "bocf_ctx.h"
#include "risk_args.h"

// theta | prob | utility parameters in one upload, the posterior, one launch per hyper-sample, the pair to the host
static int risk_run(bocf_ctx* c, const UtilArgs& u, int m, RiskArgs a, bool closed, double* acq_out, double* dacq_out) {
  const bool grad = dacq_out != nullptr;
  const int Ha = bocf_acq_hyper_count(c);
  HIPCHK(hipSetDevice(c->device));
  const UtilPack& pk = bocf_util_pack(u, nullptr, 0, &c->util_up);
  if (bocf_upload_util(c, pk, &c->rk_par)) return -1;
  c->have_acq = false;
  if (bocf_acq_posterior(c, grad)) return -1;
  const double* par = c->rk_par.as<double>();
  a.ld = c->pred_cap; a.m = m; a.C = c->C; a.L = u.L; a.util_kind = u.kind; a.theta_dim = u.theta_dim;
  a.theta = par + pk.theta; a.prob = par + pk.prob; a.util_params = par + pk.params;
  a.acq = c->acq.as<double>(); a.scale = 1.0 / Ha;
  if (grad) { a.ldg = c->pred_cap; a.d = c->d; a.dacq = c->dacq.as<double>(); }
  // the hyper-sample loop of bocf_acq_mc: hyper-sample h reads rows [h m, (h + 1) m) of the posterior and adds its share
  for (int h = 0; h < Ha; ++h) {
    PhaseTimer t(c, "acq");
    bocf_posterior_rows(c, h, m, grad, &a);
    a.accumulate = h > 0;
    if (closed) launch_linear_ucb(a, grad, c->stream);
    else launch_risk(a, grad, c->stream);
  }
  return bocf_acq_finish(c, acq_out, dacq_out);
}

extern "C" int bocf_acq_risk(bocf_ctx* c, int kind, int rank, int util_kind, const double* util_params, int n_util_params, const double* theta,
                             int theta_dim, const double* prob, int L, double* acq_out, double* dacq_out) {
  static const char* who = "bocf_acq_risk";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, prob, L};
  const int m = bocf_risk_check(who, bocf_call_state(c), kind, rank, u, dacq_out != nullptr);
  if (m < 0) return -1;
  RiskArgs a{};
  a.kind = kind; a.rank = rank; a.S = c->S_mc; a.Wt = c->Wt.as<double>();
  return risk_run(c, u, m, a, false, acq_out, dacq_out);
}

extern "C" int bocf_acq_linear_ucb(bocf_ctx* c, double kappa, const double* theta, const double* prob, int L, double* acq_out, double* dacq_out) {
  static const char* who = "bocf_acq_linear_ucb";
  const int m = bocf_ucb_check(who, bocf_call_state(c), kappa, theta, prob, L, dacq_out != nullptr);
  if (m < 0) return -1;
  const UtilArgs u{BOCF_UTIL_LINEAR, nullptr, 0, theta, m, prob, L};           // theta is (L, m)
  RiskArgs a{};
  a.kappa = kappa;
  return risk_run(c, u, m, a, true, acq_out, dacq_out);
}
