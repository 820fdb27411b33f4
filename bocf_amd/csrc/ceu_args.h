// The argument checks of the constrained expected-utility entry points (bocf_train_utility_range, bocf_expected_utility_constrained;
// capi_constrained.hip), in their order, built on the shared record and pieces of call_args.h.  Host-only and pure like it (no HIP
// include, nothing allocated): none of them needs a device, so the entry points run them before the context is touched, and the CPU
// suite drives them through tests/ceu_args_driver.cpp.  Errors name `who`.
#pragma once
#include "call_args.h"

// The utility block is bocf_constrained_utility's (call_args.h) with this path's own text for BOCF_UTIL_PROGRAM; bocf_train_utility_range
// reads no constraint.
#define BOCF_CEU_NO_PROGRAM \
  "the constrained expected utility does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities"

// What bocf_expected_utility_constrained checks after its utility block.  Returns 0, 1 when there is no resident candidate (nothing to
// do, as in bocf_expected_utility), or -1.
static inline int bocf_ceu_check_call(const char* who, const CallState& s, const UtilArgs& u, int m, const double* u_infeasible, const int* row_param,
                                      int n_hyps, const double* val_out, bool grad) {
  if (bocf_check_eu_samples(who, s, u.L, m)) return -1;
  if (!u_infeasible) return bocf_fail(who, "u_infeasible is null");
  for (int l = 0; l < u.L; ++l)
    if (!std::isfinite(u_infeasible[l])) return bocf_fail(who, "u_infeasible has a non-finite entry");
  if (bocf_check_n_hyps(who, s, n_hyps) || bocf_check_grad(who, s, grad)) return -1;
  return bocf_check_rows(who, s, u.L, row_param, val_out);
}
