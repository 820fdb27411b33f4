// The argument checks of the constrained expected-utility entry points (bocf_train_utility_range, bocf_expected_utility_constrained;
// capi_constrained.hip), in their order, over a plain record of what they read from the context.  Host-only and pure like util_args.h (no
// HIP include, nothing allocated): none of them needs a device, so the entry points run them before the context is touched, and the CPU
// suite drives them through tests/ceu_args_driver.cpp.  Errors name `who`.
#pragma once
#include "util_args.h"
#include <cmath>

#define BOCF_CEU_NO_PROGRAM \
  "the constrained expected utility does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities"

// what the checks read from the context (bocf_ctx.h has the meaning of every field)
struct CeuState {
  int fitted, canned, m, hyper_samples, best_group;   // m: all fitted outputs = hyper_samples groups
  int cq_K, cq_m;                                      // resident constraints
  int eu_S, eu_L, eu_m;                                // resident normals of bocf_set_eu_samples
  int d, C;
};

// The utility block: the kind alone (this path's own text for BOCF_UTIL_PROGRAM), then the outputs per hyper-sample, then the block against
// them in the Monte-Carlo form.  need_constraints: bocf_train_utility_range reads no constraint.  Returns m per hyper-sample, or -1.
static inline int bocf_ceu_check_utility(const char* who, const CeuState& s, const UtilArgs& u, bool need_constraints) {
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  if (bocf_util_check_kind(who, u, BOCF_CEU_NO_PROGRAM)) return -1;
  if (need_constraints && s.cq_K < 1) return bocf_fail(who, "no output constraints resident (bocf_set_output_constraints)");
  const int H = s.hyper_samples;
  if (H < 1 || s.m % H) return bocf_fail(who, "the fitted outputs are not a whole number of hyper-samples (option hyper_samples)");
  const int m = s.m / H;
  if (m > BOCF_MAX_M) return bocf_fail(who, "more outputs per hyper-sample than the device utilities take (16)");
  if (need_constraints && s.cq_m != m) return bocf_fail(who, "the resident output constraints were given for another m than the outputs per hyper-sample");
  if (s.best_group >= H) return bocf_fail(who, "option best_group is not a valid hyper-sample index");
  if (bocf_util_check(who, u, m, BOCF_EU_MC)) return -1;
  return m;
}

// What bocf_expected_utility_constrained checks after its utility block.  Returns 0, 1 when there is no resident candidate (nothing to
// do, as in bocf_expected_utility), or -1.
static inline int bocf_ceu_check_call(const char* who, const CeuState& s, const UtilArgs& u, int m, const double* u_infeasible, const int* row_param,
                                      int n_hyps, const double* val_out, bool grad) {
  if (s.eu_S < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_eu_samples)");
  if (s.eu_L < u.L) return bocf_fail(who, "fewer Monte-Carlo sample blocks than parameters (bocf_set_eu_samples)");
  if (s.eu_m != m) return bocf_fail(who, "the Monte-Carlo samples were set for another output count (bocf_set_eu_samples)");
  if (!u_infeasible) return bocf_fail(who, "u_infeasible is null");
  for (int l = 0; l < u.L; ++l)
    if (!std::isfinite(u_infeasible[l])) return bocf_fail(who, "u_infeasible has a non-finite entry");
  if (n_hyps < 1) return bocf_fail(who, "n_hyps must be >= 1");
  if (s.hyper_samples > 1 && n_hyps > s.hyper_samples) return bocf_fail(who, "n_hyps exceeds the resident hyper-samples");
  if (grad && s.canned) return bocf_fail(who, "the context holds a host-given posterior (bocf_set_posterior): it carries no gradients; fit first");
  if (grad && s.d > 64) return bocf_fail(who, "input dimension too large (gradients: d <= 64)");
  if (s.C == 0) return 1;
  if (!val_out || !row_param) return bocf_fail(who, "null output / row_param");
  for (int i = 0; i < s.C; ++i)
    if (row_param[i] < 0 || row_param[i] >= u.L) return bocf_fail(who, "row_param out of range [0, L)");
  return 0;
}
