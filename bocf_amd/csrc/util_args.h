// The utility block of the C ABI's argument lists (include/bocf_hip.h): util_kind, util_params, n_util_params, theta, theta_dim, prob, L --
// checked and packed for upload in one place; a new entry point takes its block from here.  Host-only and pure (no HIP include): the CPU
// suite drives it through tests/util_args_driver.cpp.  The checks allocate nothing, the packers only inside the vector they are given.
#pragma once
#include "../../include/bocf_hip.h"
#include <cstring>
#include <vector>

#define BOCF_MAX_M 16         // max model outputs (per hyper-sample)
#define BOCF_MAX_L 32          // max utility-parameter support size on device

int bocf_fail(const char* what, const char* detail);      // records bocf_last_error(), returns -1

struct UtilArgs { int kind; const double* params; int n_params; const double* theta; int theta_dim; const double* prob; int L; };

// The checks of the entry points that take a compiled-in utility only (bocf_acq_kg, bocf_acq_pending, bocf_acq_mc_constrained,
// bocf_feasible_best), in two parts because each looks up m, the outputs per hyper-sample, between them.  Errors name `who`.  First the
// kind alone (`no_program`: the caller's text for BOCF_UTIL_PROGRAM), then the block against m and the BOCF_EU_* form of the expectation
// (the improvement acquisitions are the BOCF_EU_MC case).
static inline int bocf_util_check_kind(const char* who, const UtilArgs& u, const char* no_program) {
  if (u.kind == BOCF_UTIL_PROGRAM) return bocf_fail(who, no_program);
  if (u.kind < BOCF_UTIL_LINEAR || u.kind > BOCF_UTIL_ROSENBROCK) return bocf_fail(who, "unknown utility kind");
  return 0;
}
static inline int bocf_util_check(const char* who, const UtilArgs& u, int m, int mode) {
  if (u.L < 1 || u.L > BOCF_MAX_L) return bocf_fail(who, "L out of range (1 .. 32)");
  if (u.theta_dim < 1 || u.theta_dim > BOCF_MAX_M || !u.theta) return bocf_fail(who, "theta must be (L, 1 <= theta_dim <= 16)");
  if ((mode == BOCF_EU_MEAN || u.kind == BOCF_UTIL_LINEAR || u.kind == BOCF_UTIL_NEG_SQ_DIST) && u.theta_dim != m)
    return bocf_fail(who, "theta_dim must equal m");
  if (mode != BOCF_EU_MEAN && u.kind == BOCF_UTIL_ROSENBROCK && (m & 1)) return bocf_fail(who, "rosenbrock utility needs even m");
  if (mode == BOCF_EU_CLOSED && (u.kind == BOCF_UTIL_LINEAR || u.kind == BOCF_UTIL_NEG_EXP_COS))
    return bocf_fail(who, "no closed-form expectation for this utility (use the Monte-Carlo mode)");
  if (u.n_params < 0 || u.n_params > BOCF_MAX_M || (u.n_params > 0 && !u.params)) return bocf_fail(who, "bad utility parameters");
  if (mode == BOCF_EU_MC && u.kind == BOCF_UTIL_NEG_EXP_COS && u.n_params != m) return bocf_fail(who, "neg_exp_cos needs m weights");
  return 0;
}

// theta (L, theta_dim) | prob (L; 1 / L each when null) | params (zero-padded to BOCF_MAX_M) | tail (n_tail doubles of the caller's, e.g. the
// fantasy normals): one host block for ONE upload; the members are offsets into `host` and so into the device copy.
// Where `host` lives: in the context (bocf_ctx::util_up), never on the stack.  The upload out of it is asynchronous and a helper that
// enqueues it returns before the entry point's one stream synchronisation, so the source must outlive every frame; every entry point that
// packs synchronises the context's stream before it returns, so the next pack never overwrites a block whose copy is in flight; and
// assign() reuses the capacity, so a run of calls does not allocate.
struct UtilPack {
  std::vector<double> host;
  size_t theta = 0, prob = 0, params = 0, tail = 0;
  size_t bytes() const { return sizeof(double) * host.size(); }
};
static inline const UtilPack& bocf_util_pack(const UtilArgs& u, const double* tail, size_t n_tail, UtilPack* pk) {
  const size_t nth = (size_t)u.L * u.theta_dim;
  pk->theta = 0; pk->prob = nth; pk->params = nth + u.L; pk->tail = pk->params + BOCF_MAX_M;
  pk->host.assign(pk->tail + n_tail, 0.0);
  double* h = pk->host.data();
  memcpy(h, u.theta, sizeof(double) * nth);
  for (int l = 0; l < u.L; ++l) h[pk->prob + l] = u.prob ? u.prob[l] : 1.0 / u.L;
  for (int i = 0; i < u.n_params; ++i) h[pk->params + i] = u.params[i];
  if (n_tail) memcpy(h + pk->tail, tail, sizeof(double) * n_tail);
  return *pk;
}

// One theta row per path for the selections over sample paths (bocf_thompson_select, bocf_path_utility): the P rows widened to
// tw = max(theta_dim, per, 1) columns (the utilities read theta[j] for j < per, the outputs per hyper-sample), zeros behind, then the
// parameters zero-padded to BOCF_MAX_M at P * tw.  Returns tw.
static inline int bocf_util_pack_rows(const double* theta, int theta_dim, int P, int per, const double* params, int n_params, std::vector<double>* host) {
  const int tw = theta_dim > per ? theta_dim : (per > 1 ? per : 1);
  host->assign((size_t)P * tw + BOCF_MAX_M, 0.0);
  for (int p = 0; p < P; ++p)
    for (int q = 0; q < theta_dim; ++q) (*host)[(size_t)p * tw + q] = theta[(size_t)p * theta_dim + q];
  for (int q = 0; q < n_params; ++q) (*host)[(size_t)P * tw + q] = params[q];
  return tw;
}
