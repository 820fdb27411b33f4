// The argument checks of the quantile / tail-mean and confidence-bound entry points (bocf_acq_risk, bocf_acq_linear_ucb; capi_risk.hip), in
// their order, built on the shared record and pieces of call_args.h.  Host-only and pure like it (no HIP include, nothing allocated): none
// of them needs a device, so the entry points run them before the context is touched, and the CPU suite drives them through
// tests/risk_args_driver.cpp.  There is no incumbent, so option best_group is not looked at.  Errors name `who`.
#pragma once
#include "call_args.h"

#define BOCF_RISK_NO_PROGRAM "the risk acquisition does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities"

// bocf_acq_risk: kind, rank and the utility's kind need no context at all and come first.  Returns m per hyper-sample, or -1.
static inline int bocf_risk_check(const char* who, const CallState& s, int kind, int rank, const UtilArgs& u, bool grad) {
  if (kind != BOCF_RISK_QUANTILE && kind != BOCF_RISK_UPPER_TAIL && kind != BOCF_RISK_LOWER_TAIL)
    return bocf_fail(who, "unknown risk kind (BOCF_RISK_QUANTILE, BOCF_RISK_UPPER_TAIL, BOCF_RISK_LOWER_TAIL)");
  if (rank < 0) return bocf_fail(who, "rank out of range (0 .. S - 1)");
  const int m = bocf_compiled_utility(who, s, u, BOCF_EU_MC, BOCF_RISK_NO_PROGRAM);
  if (m < 0) return -1;
  if (s.S_mc < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  if (s.S_mc > BOCF_RISK_MAX_SAMPLES) return bocf_fail(who, "too many Monte-Carlo samples resident for an exact selection (S <= 4096)");
  if (rank >= s.S_mc) return bocf_fail(who, "rank out of range (0 .. S - 1)");
  if (bocf_check_call(who, s, grad)) return -1;
  return m;
}

// bocf_acq_linear_ucb: theta is (L, m).  Returns m per hyper-sample, or -1.
static inline int bocf_ucb_check(const char* who, const CallState& s, double kappa, const double* theta, const double* prob, int L, bool grad) {
  if (!std::isfinite(kappa)) return bocf_fail(who, "kappa must be finite");
  const int m = bocf_check_groups(who, s, false);
  if (m < 0) return -1;
  const UtilArgs u{BOCF_UTIL_LINEAR, nullptr, 0, theta, m, prob, L};
  if (bocf_util_check(who, u, m, BOCF_EU_MC) || bocf_check_call(who, s, grad)) return -1;
  return m;
}
