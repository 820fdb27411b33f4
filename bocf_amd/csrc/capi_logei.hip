// Log-space expected-improvement entry points of the C ABI (include/bocf_hip.h): bocf_acq_log_linear -- log EI of a
// linear utility in closed form -- and bocf_acq_log_mc -- the log of the smooth surrogate of the Monte-Carlo EI of a composite utility
// (kernels: logei.hip).  The posterior is the one bocf_acq_linear / bocf_acq_mc read (the predict pass's plan and chunking, variance with
// noise, clipped), the samples are the resident ones of bocf_set_mc_samples, the incumbents are theirs too (each hyper-sample's own, or that
// of option best_group for all), the hyper-samples of option acq_hyper_samples are closed inside ONE launch, the value is left as the
// context's acquisition vector for the selections.  Parameters and incumbents live in buffers of this path: the parameter and best-so-far
// caches of the improvement acquisitions are left as they were, so a bocf_acq_mc / bocf_acq_linear call after one of these returns the
// bits it returns without it.  The checks that need no context run before it is touched.  One stream, one synchronisation per call.
#include "bocf_ctx.h"
#include "logei.h"
#include "logei_args.h"

// theta | prob | utility parameters in one upload, the posterior, the incumbents of every hyper-sample, one launch, the pair to the host
static int logei_run(bocf_ctx* c, UtilArgs u, int m, bool closed, double tau, double* acq_out, double* dacq_out) {
  static const double no_theta[BOCF_MAX_L] = {0.0};         // a program without parameters: one unread column
  const bool grad = dacq_out != nullptr;
  const int Ha = bocf_acq_hyper_count(c);
  if (u.theta_dim == 0) { u.theta = no_theta; u.theta_dim = 1; }
  HIPCHK(hipSetDevice(c->device));
  const UtilPack& pk = bocf_util_pack(u, nullptr, 0, &c->util_up);
  if (c->lg_best.ensure(sizeof(double) * (size_t)Ha * u.L) || bocf_upload_util(c, pk, &c->lg_par)) return -1;
  c->have_acq = false;
  if (bocf_acq_posterior(c, grad)) return -1;
  const double* par = c->lg_par.as<double>();
  LogEiArgs a{};
  a.mean = c->mean.as<double>(); a.var = c->var.as<double>(); a.ld = c->pred_cap;
  a.m = m; a.C = c->C; a.L = u.L; a.H = Ha; a.util_kind = u.kind; a.theta_dim = u.theta_dim;
  a.theta = par + pk.theta; a.prob = par + pk.prob; a.util_params = par + pk.params;
  a.best = c->lg_best.as<double>(); a.best_stride = c->best_group >= 0 ? 0 : u.L;
  a.acq = c->acq.as<double>(); a.tau = tau; a.prog = &c->prog;
  if (!closed) { a.Wt = c->Wt.as<double>(); a.S = c->S_mc; }
  if (grad) { a.dmean = c->dmean.as<double>(); a.dvar = c->dvar.as<double>(); a.ldg = c->pred_cap; a.d = c->d; a.dacq = c->dacq.as<double>(); }
  PhaseTimer t(c, "acq");
  // the incumbents of the improvement acquisitions: each hyper-sample's own, or that of option best_group for all
  for (int h = 0; h < (c->best_group >= 0 ? 1 : Ha); ++h)
    launch_best_so_far(c->mu_train.as<double>() + (size_t)bocf_best_group_of(c, h) * m * c->N, c->N, m, closed ? 1 : 0, u.kind, a.theta, u.theta_dim, u.L,
                       a.util_params, c->lg_best.as<double>() + (size_t)h * u.L, c->stream, &c->prog);
  if (closed) launch_logei_linear(a, grad, c->stream);
  else launch_logei_mc(a, grad, c->stream);
  t.stop();
  return bocf_acq_finish(c, acq_out, dacq_out);
}

extern "C" int bocf_acq_log_linear(bocf_ctx* c, const double* theta, const double* prob, int L, double* acq_out, double* dacq_out) {
  static const char* who = "bocf_acq_log_linear";
  const int m = bocf_log_linear_check(who, bocf_call_state(c), theta, L, dacq_out != nullptr);
  if (m < 0) return -1;
  return logei_run(c, UtilArgs{BOCF_UTIL_LINEAR, nullptr, 0, theta, m, prob, L}, m, true, 1.0, acq_out, dacq_out);   // theta is (L, m)
}

extern "C" int bocf_acq_log_mc(bocf_ctx* c, double tau, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                               const double* prob, int L, double* acq_out, double* dacq_out) {
  static const char* who = "bocf_acq_log_mc";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, prob, L};
  bool program;
  const int m = bocf_log_mc_check(who, bocf_call_state(c), tau, u, dacq_out != nullptr, &program);
  if (m < 0) return -1;
  if (program && bocf_check_resident_program(c, who, m, theta_dim, n_util_params)) return -1;
  return logei_run(c, u, m, false, tau, acq_out, dacq_out);
}
