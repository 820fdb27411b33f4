// The argument checks of the log-space expected-improvement entry points (bocf_acq_log_linear, bocf_acq_log_mc; capi_logei.hip), in their
// order, built on the shared record and pieces of call_args.h.  Host-only and pure like it (no HIP include, nothing allocated): none of
// them needs a device, so the entry points run them before the context is touched, and the CPU suite drives them through
// tests/logei_args_driver.cpp.  The checks are those of bocf_acq_linear[_grad] / bocf_acq_mc[_grad]; a utility program is accepted (the
// caller checks the resident one with bocf_check_resident_program).  Errors name `who`.
#pragma once
#include "call_args.h"

// bocf_acq_log_linear: theta is (L, m).  Returns m per hyper-sample, or -1.
static inline int bocf_log_linear_check(const char* who, const CallState& s, const double* theta, int L, bool grad) {
  const int m = bocf_check_groups(who, s, true);
  if (m < 0) return -1;
  if (L < 1 || L > BOCF_MAX_L) return bocf_fail(who, "L out of range (1 .. 32)");
  if (!theta) return bocf_fail(who, "theta is null");
  if (bocf_check_call(who, s, grad)) return -1;
  return m;
}

// bocf_acq_log_mc: tau and the utility's kind need no context at all and come first.  Returns m per hyper-sample, or -1.  For
// BOCF_UTIL_PROGRAM the block is checked against the resident program by the caller (*program is set).
static inline int bocf_log_mc_check(const char* who, const CallState& s, double tau, const UtilArgs& u, bool grad, bool* program) {
  *program = false;
  if (!(std::isfinite(tau) && tau > 0.0)) return bocf_fail(who, "tau must be finite and > 0");
  if (u.kind < BOCF_UTIL_LINEAR || u.kind > BOCF_UTIL_PROGRAM) return bocf_fail(who, "unknown utility kind");
  const int m = bocf_check_groups(who, s, true);
  if (m < 0) return -1;
  if (s.S_mc < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  if (u.L < 1 || u.L > BOCF_MAX_L) return bocf_fail(who, "L out of range (1 .. 32)");
  if (u.kind == BOCF_UTIL_PROGRAM) {
    if (u.theta_dim < 0 || (u.theta_dim > 0 && !u.theta)) return bocf_fail(who, "theta is null");
    *program = true;
  } else if (bocf_util_check(who, u, m, BOCF_EU_MC)) {
    return -1;
  }
  if (bocf_check_call(who, s, grad)) return -1;
  return m;
}
