// The argument checks of the quantile / tail-mean and confidence-bound entry points (bocf_acq_risk, bocf_acq_linear_ucb; capi_risk.hip), in
// their order, over a plain record of what they read from the context.  Host-only and pure like util_args.h and ceu_args.h (no HIP
// include, nothing allocated): none of them needs a device, so the entry points run them before the context is touched, and the CPU suite
// drives them through tests/risk_args_driver.cpp -- including the branches no fitted context can reach today (a fit refuses d > 32, the
// gradient kernels hold d <= 64 lanes' worth).  Errors name `who`.
#pragma once
#include "util_args.h"
#include <cmath>

#define BOCF_RISK_NO_PROGRAM "the risk acquisition does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities"

// what the checks read from the context (bocf_ctx.h has the meaning of every field); a null context is fitted = 0
struct RiskState {
  int fitted, canned, m, hyper_samples;   // m: all fitted outputs = hyper_samples groups
  int S_mc;                               // resident samples of bocf_set_mc_samples
  int d, C;
};

// outputs per hyper-sample of a fitted context, or -1
static inline int bocf_risk_group_size(const char* who, const RiskState& s) {
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  const int H = s.hyper_samples;
  if (H < 1 || s.m % H) return bocf_fail(who, "the fitted outputs are not a whole number of hyper-samples (option hyper_samples)");
  if (s.m / H > BOCF_MAX_M) return bocf_fail(who, "more outputs per hyper-sample than the device utilities take (16)");
  return s.m / H;
}

// what both entry points check once the utility block is known to fit
static inline int bocf_risk_check_call(const char* who, const RiskState& s, bool grad) {
  if (s.C < 1) return bocf_fail(who, "no resident candidates (bocf_set_candidates)");
  if (grad && s.canned) return bocf_fail(who, "the context holds a host-given posterior (bocf_set_posterior): it carries no gradients; fit first");
  if (grad && s.d > 64) return bocf_fail(who, "input dimension too large (gradients: d <= 64)");
  return 0;
}

// bocf_acq_risk: kind, rank and the utility's kind need no context at all and come first.  Returns m per hyper-sample, or -1.
static inline int bocf_risk_check(const char* who, const RiskState& s, int kind, int rank, const UtilArgs& u, bool grad) {
  if (kind != BOCF_RISK_QUANTILE && kind != BOCF_RISK_UPPER_TAIL && kind != BOCF_RISK_LOWER_TAIL)
    return bocf_fail(who, "unknown risk kind (BOCF_RISK_QUANTILE, BOCF_RISK_UPPER_TAIL, BOCF_RISK_LOWER_TAIL)");
  if (rank < 0) return bocf_fail(who, "rank out of range (0 .. S - 1)");
  if (bocf_util_check_kind(who, u, BOCF_RISK_NO_PROGRAM)) return -1;
  const int m = bocf_risk_group_size(who, s);
  if (m < 0) return -1;
  if (bocf_util_check(who, u, m, BOCF_EU_MC)) return -1;
  if (s.S_mc < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  if (s.S_mc > BOCF_RISK_MAX_SAMPLES) return bocf_fail(who, "too many Monte-Carlo samples resident for an exact selection (S <= 4096)");
  if (rank >= s.S_mc) return bocf_fail(who, "rank out of range (0 .. S - 1)");
  if (bocf_risk_check_call(who, s, grad)) return -1;
  return m;
}

// bocf_acq_linear_ucb: theta is (L, m).  Returns m per hyper-sample, or -1.
static inline int bocf_ucb_check(const char* who, const RiskState& s, double kappa, const double* theta, const double* prob, int L, bool grad) {
  if (!std::isfinite(kappa)) return bocf_fail(who, "kappa must be finite");
  const int m = bocf_risk_group_size(who, s);
  if (m < 0) return -1;
  const UtilArgs u{BOCF_UTIL_LINEAR, nullptr, 0, theta, m, prob, L};
  if (bocf_util_check(who, u, m, BOCF_EU_MC)) return -1;
  if (bocf_risk_check_call(who, s, grad)) return -1;
  return m;
}
