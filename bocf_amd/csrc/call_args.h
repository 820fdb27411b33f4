// The argument checks of the entry points that evaluate a utility over the posterior, in their order, over ONE plain record of what any of
// them reads from the context (CallState; bocf_call_state of bocf_ctx.h fills it).  Host-only and pure like util_args.h (no HIP include,
// nothing allocated): the entry points run them before the context is touched, and the CPU suite drives them through
// tests/call_args_driver.cpp -- also the branches no fitted context reaches today (a fit refuses d > 32).  Errors name `who`.  First the
// pieces every family shares, each refusal spelled out once (`old`: the wording the first entry points keep), then one sequence per entry
// point or pair.  What reads more than the record (the resident program, the workspace cap, the parameter upload) stays with the entry
// point, at its place in the sequence: a check that stands behind one of those is a function of its own here.
#pragma once
#include "joint_chol.h"        // JOINT_MAX_Q
#include "kern_dispatch.h"     // BOCF_MAX_D
#include "util_args.h"
#include <cmath>

// a null context is all zeros: not fitted
struct CallState {
  int fitted, canned, N, d, m, hyper_samples, best_group, C, S_mc;   // m: all fitted outputs = hyper_samples groups
  int eu_S, eu_L, eu_m;                                               // resident normals of bocf_set_eu_samples
  int cq_K, cq_m;                                                     // resident constraints
  int kg_na, pd_r, pd_S;                                              // resident reference points; pending points and the samples they were made for
};

// ---- the shared pieces ----------------------------------------------------------------------------------------------------------------------
static inline int bocf_check_posterior(const char* who, const CallState& s) {
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  if (s.canned) return bocf_fail(who, "the context holds a host-given posterior (bocf_set_posterior): it has no factor to sample from; fit first");
  return 0;
}
// outputs per hyper-sample when the fit holds whole groups, or -1
static inline int bocf_whole_groups(const char* who, const CallState& s, bool old = false) {
  if (s.hyper_samples < 1 || s.m % s.hyper_samples)
    return bocf_fail(who, old ? "the fitted outputs are not a multiple of option hyper_samples"
                              : "the fitted outputs are not a whole number of hyper-samples (option hyper_samples)");
  return s.m / s.hyper_samples;
}
static inline int bocf_check_best_group(const char* who, const CallState& s) {
  if (s.best_group >= s.hyper_samples) return bocf_fail(who, "option best_group is not a valid hyper-sample index");
  return 0;
}
static inline int bocf_check_group_fits(const char* who, int m, bool old = false) {
  if (m > BOCF_MAX_M) return bocf_fail(who, old ? "too many outputs per hyper-sample" : "more outputs per hyper-sample than the device utilities take (16)");
  return 0;
}
// outputs per hyper-sample of a fitted context that the device utilities take (best_group: and option best_group names one of them), or -1
static inline int bocf_check_groups(const char* who, const CallState& s, bool best_group, bool old = false) {
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  const int m = bocf_whole_groups(who, s, old);
  if (m < 0 || (best_group && bocf_check_best_group(who, s)) || bocf_check_group_fits(who, m, old)) return -1;
  return m;
}
// the outputs `group` selects: hyper-sample h's [h m', (h + 1) m') (m' = outputs per hyper-sample), or all of them for -1
static inline int bocf_group_range(const char* who, const CallState& s, int group, int* j0, int* mg, int* per) {
  if ((*per = bocf_whole_groups(who, s)) < 0) return -1;
  if (group < -1 || group >= s.hyper_samples) return bocf_fail(who, "group out of range (-1 or 0 .. hyper_samples - 1)");
  *j0 = group < 0 ? 0 : group * *per;
  *mg = group < 0 ? s.m : *per;
  return 0;
}
// the gradient forms: a host-given posterior has none, and lane q < d of the gradient kernels owns d / dx_q
static inline int bocf_check_grad_dim(const char* who, const CallState& s, bool grad, bool old = false) {
  if (grad && s.d > 64) return bocf_fail(who, old ? "input dimension too large" : "input dimension too large (gradients: d <= 64)");
  return 0;
}
static inline int bocf_check_grad(const char* who, const CallState& s, bool grad, bool old = false) {
  if (grad && s.canned) return bocf_fail(who, "the context holds a host-given posterior (bocf_set_posterior): it carries no gradients; fit first");
  return bocf_check_grad_dim(who, s, grad, old);
}
// what the acquisitions over the resident candidates check last
static inline int bocf_check_call(const char* who, const CallState& s, bool grad, bool old = false) {
  if (s.C < 1) return bocf_fail(who, "no resident candidates (bocf_set_candidates)");
  return bocf_check_grad(who, s, grad, old);
}
// the resident normals of bocf_set_eu_samples against L parameters and m outputs per hyper-sample
static inline int bocf_check_eu_samples(const char* who, const CallState& s, int L, int m, bool old = false) {
  if (s.eu_S < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_eu_samples)");
  if (s.eu_L < L)
    return bocf_fail(who, old ? "fewer Monte-Carlo sample blocks than parameters" : "fewer Monte-Carlo sample blocks than parameters (bocf_set_eu_samples)");
  if (s.eu_m != m)
    return bocf_fail(who, old ? "the Monte-Carlo samples were set for another output count"
                              : "the Monte-Carlo samples were set for another output count (bocf_set_eu_samples)");
  return 0;
}
// the expected utilities: the hyper-samples asked for; and, last, the rows -- 0, 1 when there is no resident candidate (nothing to do), or -1
static inline int bocf_check_n_hyps(const char* who, const CallState& s, int n_hyps) {
  if (n_hyps < 1) return bocf_fail(who, "n_hyps must be >= 1");
  if (s.hyper_samples > 1 && n_hyps > s.hyper_samples) return bocf_fail(who, "n_hyps exceeds the resident hyper-samples");
  return 0;
}
static inline int bocf_check_rows(const char* who, const CallState& s, int L, const int* row_param, const double* val_out) {
  if (s.C == 0) return 1;
  if (!val_out || !row_param) return bocf_fail(who, "null output / row_param");
  for (int i = 0; i < s.C; ++i)
    if (row_param[i] < 0 || row_param[i] >= L) return bocf_fail(who, "row_param out of range [0, L)");
  return 0;
}
// A compiled-in utility against a fitted context: the kind alone (`no_program`: the caller's text for BOCF_UTIL_PROGRAM), the outputs per
// hyper-sample, the block against them in the BOCF_EU_* form `mode`.  Returns m per hyper-sample, or -1.
static inline int bocf_compiled_utility(const char* who, const CallState& s, const UtilArgs& u, int mode, const char* no_program) {
  if (bocf_util_check_kind(who, u, no_program)) return -1;
  const int m = bocf_check_groups(who, s, false);
  if (m < 0 || bocf_util_check(who, u, m, mode)) return -1;
  return m;
}
// ... and against the resident output constraints (need_constraints: bocf_train_utility_range reads none).  Returns m per hyper-sample, or -1.
static inline int bocf_constrained_utility(const char* who, const CallState& s, const UtilArgs& u, bool need_constraints, const char* no_program) {
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  if (bocf_util_check_kind(who, u, no_program)) return -1;
  if (need_constraints && s.cq_K < 1) return bocf_fail(who, "no output constraints resident (bocf_set_output_constraints)");
  const int m = bocf_check_groups(who, s, false);
  if (m < 0) return -1;
  if (need_constraints && s.cq_m != m) return bocf_fail(who, "the resident output constraints were given for another m than the outputs per hyper-sample");
  if (bocf_check_best_group(who, s) || bocf_util_check(who, u, m, BOCF_EU_MC)) return -1;
  return m;
}

// ---- the improvement acquisitions (capi.hip; bocf_refine_acq borrows the group and utility checks) -----------------------------------------
// bocf_acq_linear, bocf_acq_linear_grad.  L and theta are checked by the parameter upload, behind "no candidate: nothing to do".
static inline int bocf_acq_linear_check(const char* who, const CallState& s, int kind) {
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  if (kind != BOCF_ACQ_EI && kind != BOCF_ACQ_PI) return bocf_fail(who, "unknown acquisition kind");
  return bocf_check_groups(who, s, true, true);
}
// The utility checks of bocf_acq_mc and bocf_acq_mc_grad.  For BOCF_UTIL_PROGRAM the block is checked against the resident program by the
// caller (*program is set).
static inline int bocf_mc_utility_check(const char* who, const CallState& s, const UtilArgs& u, bool* program) {
  *program = false;
  if (u.kind < 0 || u.kind > BOCF_UTIL_PROGRAM) return bocf_fail(who, "unknown utility kind");
  if (s.S_mc < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  const int m = bocf_check_groups(who, s, true, true);
  if (m < 0) return -1;
  if ((*program = u.kind == BOCF_UTIL_PROGRAM)) return m;
  if ((u.kind == BOCF_UTIL_LINEAR || u.kind == BOCF_UTIL_NEG_SQ_DIST) && u.theta_dim != m) return bocf_fail(who, "theta_dim must equal m");
  if (u.kind == BOCF_UTIL_ROSENBROCK && (u.theta_dim < 1 || (m & 1))) return bocf_fail(who, "rosenbrock utility needs theta_dim >= 1 and even m");
  if (u.kind == BOCF_UTIL_NEG_EXP_COS && u.n_params != m) return bocf_fail(who, "neg_exp_cos needs m weights");
  if (u.n_params > 0 && !u.params) return bocf_fail(who, "util_params is null");
  return m;
}
// bocf_acq_mc (grad = false: the kind is the caller's) and bocf_acq_mc_grad; behind the resident program's check the gradient form goes on
// with bocf_check_grad_dim(who, s, true, true)
static inline int bocf_acq_mc_check(const char* who, const CallState& s, bool grad, int kind, const UtilArgs& u, bool* program) {
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  if (!grad && kind != BOCF_ACQ_EI && kind != BOCF_ACQ_PI) return bocf_fail(who, "unknown acquisition kind");
  return bocf_mc_utility_check(who, s, u, program);
}
// bocf_set_mc_samples, bocf_set_eu_samples (args_ok: the samples are given and every count is >= 1)
static inline int bocf_set_samples_check(const char* who, const CallState& s, bool args_ok) {
  if (!s.fitted || !args_ok) return bocf_fail(who, "model not fitted / bad samples");
  return bocf_check_groups(who, s, true, true);
}
// bocf_expected_utility, up to the resident program's check (*program: the caller makes it) ...
static inline int bocf_eu_check_utility(const char* who, const CallState& s, int mode, const UtilArgs& u, bool* program) {
  *program = false;
  if (!s.fitted) return bocf_fail(who, "model not fitted");
  if (s.canned) return bocf_fail(who, "the context holds a host-given posterior (bocf_set_posterior): fit first");
  if (mode < BOCF_EU_MEAN || mode > BOCF_EU_MC) return bocf_fail(who, "unknown mode");
  if (u.kind < 0 || u.kind > BOCF_UTIL_PROGRAM) return bocf_fail(who, "unknown utility kind");
  const int m = bocf_check_groups(who, s, true, true);
  if (m < 0) return -1;
  if (u.L < 1 || u.theta_dim < 1 || !u.theta) return bocf_fail(who, "theta must be (L >= 1, theta_dim >= 1)");
  if (mode == BOCF_EU_CLOSED && u.kind == BOCF_UTIL_PROGRAM)
    return bocf_fail(who, "a utility program has no closed-form expectation (BOCF_EU_CLOSED): use the Monte-Carlo mode");
  *program = mode == BOCF_EU_MC && u.kind == BOCF_UTIL_PROGRAM;
  return m;
}
// ... and behind it.  Returns 0, 1 when there is no resident candidate (nothing to do), or -1.
static inline int bocf_eu_check_call(const char* who, const CallState& s, int mode, const UtilArgs& u, int m, const int* row_param, int n_hyps,
                                     const double* val_out, bool grad) {
  if ((mode == BOCF_EU_MEAN || u.kind == BOCF_UTIL_LINEAR || u.kind == BOCF_UTIL_NEG_SQ_DIST) && u.theta_dim != m)
    return bocf_fail(who, "theta_dim must equal m");
  if (mode != BOCF_EU_MEAN && u.kind == BOCF_UTIL_ROSENBROCK && (m & 1)) return bocf_fail(who, "rosenbrock utility needs even m");
  if (mode == BOCF_EU_CLOSED && (u.kind == BOCF_UTIL_LINEAR || u.kind == BOCF_UTIL_NEG_EXP_COS))
    return bocf_fail(who, "no closed-form expectation for this utility (use the Monte-Carlo mode)");
  if (mode == BOCF_EU_MC && u.kind == BOCF_UTIL_NEG_EXP_COS && u.n_params != m) return bocf_fail(who, "neg_exp_cos needs m weights");
  if (u.n_params < 0 || u.n_params > BOCF_MAX_M || (u.n_params > 0 && !u.params)) return bocf_fail(who, "bad utility parameters");
  if (mode == BOCF_EU_MC && bocf_check_eu_samples(who, s, u.L, m, true)) return -1;
  if (bocf_check_grad_dim(who, s, grad, true) || bocf_check_n_hyps(who, s, n_hyps)) return -1;
  return bocf_check_rows(who, s, u.L, row_param, val_out);
}

// ---- the look-ahead family: the workspace and chunk refusals follow in the entry point -----------------------------------------------------
// what reads the resident reference set needs it, candidates and d <= 32 (bocf_cov_to_ref, bocf_conditioned_variance, bocf_acq_kg)
static inline int bocf_kg_ready(const char* who, const CallState& s) {
  if (bocf_check_posterior(who, s)) return -1;
  if (s.kg_na < 1) return bocf_fail(who, "no reference points: call bocf_set_ref_points after the fit");
  if (s.C < 1) return bocf_fail(who, "no resident candidates (bocf_set_candidates)");
  if (s.d > BOCF_MAX_D) return bocf_fail(who, "input dimension too large");
  return 0;
}
// bocf_acq_kg
static inline int bocf_kg_check(const char* who, const CallState& s, int mode, const UtilArgs& u, const double* Zf, int Sf) {
  if (bocf_check_posterior(who, s)) return -1;
  if (mode < BOCF_EU_MEAN || mode > BOCF_EU_MC) return bocf_fail(who, "unknown mode");
  const int m = bocf_compiled_utility(who, s, u, mode, "the knowledge gradient does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities");
  if (m < 0) return -1;
  if (!Zf) return bocf_fail(who, "null Zf");
  if (Sf < 1 || Sf > 256) return bocf_fail(who, "Sf out of range (1 .. 256)");
  if (mode == BOCF_EU_MC && s.S_mc < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  if (mode == BOCF_EU_MC && s.S_mc > 256) return bocf_fail(who, "more than 256 Monte-Carlo samples");
  return bocf_kg_ready(who, s) ? -1 : m;
}
// bocf_acq_pending
static inline int bocf_pending_check(const char* who, const CallState& s, const UtilArgs& u) {
  if (bocf_check_posterior(who, s)) return -1;
  const int m = bocf_compiled_utility(who, s, u, BOCF_EU_MC,
                                      "the pending-point acquisition does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities");
  if (m < 0) return -1;
  if (s.S_mc < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  if (s.S_mc > 256) return bocf_fail(who, "more than 256 Monte-Carlo samples");
  if (s.pd_r < 1) return bocf_fail(who, "no pending points: call bocf_set_pending_points after the fit");
  if (s.pd_S != s.S_mc) return bocf_fail(who, "the number of Monte-Carlo samples changed since bocf_set_pending_points");
  if (s.C < 1) return bocf_fail(who, "no resident candidates (bocf_set_candidates)");
  if (s.d > BOCF_MAX_D) return bocf_fail(who, "input dimension too large");
  if (bocf_check_best_group(who, s)) return -1;
  return m;
}
// bocf_acq_joint
static inline int bocf_joint_check(const char* who, const CallState& s, const UtilArgs& u, int q, const double* Z, int S) {
  if (bocf_check_posterior(who, s)) return -1;
  const int m = bocf_compiled_utility(who, s, u, BOCF_EU_MC,
                                      "the joint acquisition does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities");
  if (m < 0) return -1;
  if (q < 1 || q > JOINT_MAX_Q) return bocf_fail(who, "q out of range (1 .. 8)");
  if (!Z) return bocf_fail(who, "null Z");
  if (S < 1 || S > 256) return bocf_fail(who, "S out of range (1 .. 256)");
  if (s.C < 1) return bocf_fail(who, "no resident candidates (bocf_set_candidates)");
  if (s.C % q) return bocf_fail(who, "the number of resident candidates is not a multiple of q");
  if (s.d > BOCF_MAX_D) return bocf_fail(who, "input dimension too large");
  if (bocf_check_best_group(who, s)) return -1;
  return m;
}

// ---- the constrained acquisition (capi_constrained.hip): bocf_feasible_best is bocf_constrained_utility with this text -----------------------
#define BOCF_CACQ_NO_PROGRAM "the constrained acquisition does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities"
// bocf_acq_mc_constrained
static inline int bocf_cacq_check(const char* who, const CallState& s, const UtilArgs& u, bool grad) {
  const int m = bocf_constrained_utility(who, s, u, true, BOCF_CACQ_NO_PROGRAM);
  if (m < 0) return -1;
  if (s.S_mc < 1) return bocf_fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  if (bocf_check_call(who, s, grad, true)) return -1;
  return m;
}

// ---- bocf_loo_utility (capi_loo.hip) --------------------------------------------------------------------------------------------------------
// up to the resident program's check (*program: the caller makes it) ...
static inline int bocf_loo_utility_check(const char* who, const CallState& s, int group, int flags, int mode, const UtilArgs& u, bool* program) {
  *program = false;
  if (bocf_check_posterior(who, s)) return -1;
  if (flags & ~(BOCF_ADD_NOISE | BOCF_CLIP)) return bocf_fail(who, "unknown flags (BOCF_ADD_NOISE | BOCF_CLIP)");
  if (mode < BOCF_EU_MEAN || mode > BOCF_EU_MC) return bocf_fail(who, "unknown mode");
  if (group < 0) return bocf_fail(who, "group out of range (0 .. hyper_samples - 1)");
  int j0, mg, m;
  if (bocf_group_range(who, s, group, &j0, &mg, &m) || bocf_check_group_fits(who, m)) return -1;
  if (u.kind == BOCF_UTIL_PROGRAM && mode != BOCF_EU_MEAN) {
    if (mode == BOCF_EU_CLOSED) return bocf_fail(who, "a utility program has no closed-form expectation (BOCF_EU_CLOSED): use the Monte-Carlo mode");
    if (u.L < 1 || u.L > BOCF_MAX_L) return bocf_fail(who, "L out of range (1 .. 32)");
    if (u.theta_dim < 1 || u.theta_dim > BOCF_MAX_M || !u.theta) return bocf_fail(who, "theta must be (L, 1 <= theta_dim <= 16)");
    *program = true;
    return m;
  }
  if (u.kind < BOCF_UTIL_LINEAR || u.kind > BOCF_UTIL_PROGRAM) return bocf_fail(who, "unknown utility kind");
  UtilArgs k = u;
  if (mode == BOCF_EU_MEAN) k.kind = BOCF_UTIL_LINEAR;     // (the mean form ignores the kind)
  if (bocf_util_check(who, k, m, mode)) return -1;
  return m;
}
// ... and behind it
static inline int bocf_loo_utility_check_call(const char* who, const CallState& s, int mode, int L, int m, const double* val_out) {
  if (mode == BOCF_EU_MC && bocf_check_eu_samples(who, s, L, m)) return -1;
  if (!val_out) return bocf_fail(who, "null val_out");
  return 0;
}
