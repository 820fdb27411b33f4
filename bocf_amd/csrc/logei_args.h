// The argument checks of the log-space expected-improvement entry points (bocf_acq_log_linear, bocf_acq_log_mc; capi_logei.hip), in their
// order, over a plain record of what they read from the context.  Host-only and pure like util_args.h and risk_args.h (no HIP include,
// nothing allocated): none of them needs a device, so the entry points run them before the context is touched, and the CPU suite drives
// them through tests/logei_args_driver.cpp -- including the branches no fitted context can reach today (a fit refuses d > 32, the gradient
// kernels hold d <= 64 lanes' worth).  The checks are those of bocf_acq_linear[_grad] / bocf_acq_mc[_grad]; a utility program is accepted
// (the caller checks the resident one with bocf_check_resident_program).  Errors name `who`.
#pragma once
#include "util_args.h"
#include <cmath>

// what the checks read from the context (bocf_ctx.h has the meaning of every field); a null context is fitted = 0
struct LogEiState {
  int fitted, canned, m, hyper_samples, best_group;   // m: all fitted outputs = hyper_samples groups
  int S_mc;                                           // resident samples of bocf_set_mc_samples
  int d, C;
};

// outputs per hyper-sample of a fitted context, or -1
static inline int bocf_logei_group_size(const char* who, const LogEiState& s) {
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  const int H = s.hyper_samples;
  if (H < 1 || s.m % H) return bocf_fail(who, "the fitted outputs are not a whole number of hyper-samples (option hyper_samples)");
  if (s.best_group >= H) return bocf_fail(who, "option best_group is not a valid hyper-sample index");
  if (s.m / H > BOCF_MAX_M) return bocf_fail(who, "more outputs per hyper-sample than the device utilities take (16)");
  return s.m / H;
}

// what both entry points check last
static inline int bocf_logei_check_call(const char* who, const LogEiState& s, bool grad) {
  if (s.C < 1) return bocf_fail(who, "no resident candidates (bocf_set_candidates)");
  if (grad && s.canned) return bocf_fail(who, "the context holds a host-given posterior (bocf_set_posterior): it carries no gradients; fit first");
  if (grad && s.d > 64) return bocf_fail(who, "input dimension too large (gradients: d <= 64)");
  return 0;
}

// bocf_acq_log_linear: theta is (L, m).  Returns m per hyper-sample, or -1.
static inline int bocf_log_linear_check(const char* who, const LogEiState& s, const double* theta, int L, bool grad) {
  const int m = bocf_logei_group_size(who, s);
  if (m < 0) return -1;
  if (L < 1 || L > BOCF_MAX_L) return bocf_fail(who, "L out of range (1 .. 32)");
  if (!theta) return bocf_fail(who, "theta is null");
  if (bocf_logei_check_call(who, s, grad)) return -1;
  return m;
}

// bocf_acq_log_mc: tau and the utility's kind need no context at all and come first.  Returns m per hyper-sample, or -1.  For
// BOCF_UTIL_PROGRAM the block is checked against the resident program by the caller (*program is set).
static inline int bocf_log_mc_check(const char* who, const LogEiState& s, double tau, const UtilArgs& u, bool grad, bool* program) {
  *program = false;
  if (!(std::isfinite(tau) && tau > 0.0)) return bocf_fail(who, "tau must be finite and > 0");
  if (u.kind < BOCF_UTIL_LINEAR || u.kind > BOCF_UTIL_PROGRAM) return bocf_fail(who, "unknown utility kind");
  const int m = bocf_logei_group_size(who, s);
  if (m < 0) return -1;
  if (s.S_mc < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  if (u.L < 1 || u.L > BOCF_MAX_L) return bocf_fail(who, "L out of range (1 .. 32)");
  if (u.kind == BOCF_UTIL_PROGRAM) {
    if (u.theta_dim < 0 || (u.theta_dim > 0 && !u.theta)) return bocf_fail(who, "theta is null");
    *program = true;
  } else if (bocf_util_check(who, u, m, BOCF_EU_MC)) {
    return -1;
  }
  if (bocf_logei_check_call(who, s, grad)) return -1;
  return m;
}
