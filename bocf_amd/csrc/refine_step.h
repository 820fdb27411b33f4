// One step of the anchor refinement, stated once for the host and the device: the algorithm of bocf_lbfgsb_batched
// (optimizer_host.hip) / lbfgsb_batched_numpy, turned inside out into a per-row state machine.  refine_advance() consumes the value and the
// gradient at the row's current trial point and leaves the row's next trial point; whoever drives it only evaluates: refine_advance_kernel
// (refine.hip) between two acquisition passes on the stream, tests/refine_step_driver.cpp on analytic objectives.
//
// Plain C++, no HIP include: __host__ __device__ under hipcc, plain under a host compiler (the pattern of chol_plan.h / util_args.h).
//
// Why a row needs nothing from the others.  In the host loop `head` advances once per outer iteration for every running row, and a running
// row completes exactly one iteration per outer iteration, so the slot a row writes is iterations[row] % m.  A row that accepts a step
// starts its next iteration in the same call (stop tests, direction, t = 1, trial point): one call is one evaluation per running row.
//
// Same bits on x86 and gfx950.  Every sum runs in the host routine's order (ascending k; the two-loop recursion newest -> oldest, then
// oldest -> newest), every function body opens with REFINE_FP_STRICT -- `#pragma clang fp contract(off)`, which both hipcc (whose default is
// -ffp-contract=fast-honor-pragmas) and a host clang obey, so a * b + c stays a rounded product and a rounded sum; under GCC the functions
// sit between `#pragma GCC optimize("fp-contract=off")` brackets (REFINE_FP_BEGIN / REFINE_FP_END) -- and only + - * / sqrt fabs fmin fmax are used, which IEEE-754 fixes.
//
// Every loop is bounded by d, m or max_ls (max_ls bounds the CALLS of one arc search: a call never loops over trial points).
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define REFINE_HD __host__ __device__
#else
#define REFINE_HD
#endif
// REFINE_FP_STRICT opens every function body; REFINE_FP_BEGIN / REFINE_FP_END bracket the functions of a header (this one and
// refine_poly.h) for GCC, which has no statement-level pragma
#if defined(__clang__)
#define REFINE_FP_STRICT _Pragma("clang fp contract(off)")
#define REFINE_FP_BEGIN
#define REFINE_FP_END
#elif defined(__GNUC__)
#define REFINE_FP_STRICT
#define REFINE_FP_BEGIN _Pragma("GCC push_options") _Pragma("GCC optimize(\"fp-contract=off\")")
#define REFINE_FP_END _Pragma("GCC pop_options")
#else
#define REFINE_FP_STRICT
#define REFINE_FP_BEGIN
#define REFINE_FP_END
#endif
REFINE_FP_BEGIN

#define REFINE_MAX_D 64        // input dimensions the device entry accepts (the Monte-Carlo gradient kernel's bound)
#define REFINE_MAX_M 64        // curvature pairs kept per row

// why a row stopped (0: it has not)
enum RefineReason {
  REFINE_RUNNING = 0,
  REFINE_PGTOL = 1,            // max |projected gradient| <= pgtol
  REFINE_FACTR = 2,            // relative decrease <= factr * eps
  REFINE_ARC_FAILED = 3,       // max_ls trial points along the projection arc, none accepted: the row keeps its point
  REFINE_MAXITER = 4,
  REFINE_MAXFUN = 5,           // (tested where an iteration starts, as the host loop does: an arc search is never cut short)
  REFINE_NONFINITE_START = 6,  // f at the clamped start is not finite: the start is left in place
  REFINE_NAN_GRADIENT = 7
};

struct RefineSettings {
  int d, m, maxiter, max_ls, maxfun;   // maxfun < 0: none
  double factr, pgtol, c1;
  int boxed;                           // every bound finite (refine_boxed)
};

// Per-row state: one block of doubles and one of ints, so a driver can keep rows in two flat arrays (and compare a frozen row's bytes).
//   doubles: x (d) | g (d) | dir (d) | xt (d) | q (d) | z (d) | S (m, d) | Y (m, d) | rho (m) | alphas (m) | f | gamma | t
//   ints:    iterations | evaluations | reason | trial points of the current arc search | started
#define REFINE_ROW_INTS 8
REFINE_HD static inline size_t refine_row_doubles(int d, int m) { return (size_t)6 * d + (size_t)2 * m * d + (size_t)2 * m + 3; }

struct RefineRow {
  double *x, *g, *dir, *xt, *q, *z, *S, *Y, *rho, *alphas, *f, *gamma, *t;
  int *iters, *nfun, *reason, *ls, *started;
};

REFINE_HD static inline RefineRow refine_row_view(double* dbl, int* ints, int d, int m) {
  RefineRow r;
  r.x = dbl; r.g = r.x + d; r.dir = r.g + d; r.xt = r.dir + d; r.q = r.xt + d; r.z = r.q + d;
  r.S = r.z + d; r.Y = r.S + (size_t)m * d; r.rho = r.Y + (size_t)m * d; r.alphas = r.rho + m;
  r.f = r.alphas + m; r.gamma = r.f + 1; r.t = r.gamma + 1;
  r.iters = ints; r.nfun = ints + 1; r.reason = ints + 2; r.ls = ints + 3; r.started = ints + 4;
  return r;
}

REFINE_HD static inline int refine_boxed(const double* lo, const double* hi, int d) {
  int boxed = 1;
  for (int k = 0; k < d; ++k) boxed = boxed && std::isfinite(lo[k]) && std::isfinite(hi[k]);
  return boxed;
}

// a fresh row: x = xt = the start clamped into the box (the first call evaluates it there), everything else zero
REFINE_HD static inline void refine_init(const RefineRow& r, const double* x0, const double* lo, const double* hi, const RefineSettings& s) {
  REFINE_FP_STRICT
  const size_t n = refine_row_doubles(s.d, s.m);
  for (size_t i = 0; i < n; ++i) r.x[i] = 0.0;
  for (int i = 0; i < REFINE_ROW_INTS; ++i) r.iters[i] = 0;
  for (int k = 0; k < s.d; ++k) r.x[k] = r.xt[k] = std::fmin(std::fmax(x0[k], lo[k]), hi[k]);
}

// the point the driver evaluates next (a stopped row: its final x)
REFINE_HD static inline const double* refine_point(const RefineRow& r) { return *r.reason == REFINE_RUNNING ? r.xt : r.x; }

REFINE_HD static inline void refine_trial_point(const RefineRow& r, const double* lo, const double* hi, int d) {
  REFINE_FP_STRICT
  const double t = *r.t;
  for (int k = 0; k < d; ++k) r.xt[k] = std::fmin(std::fmax(r.x[k] + t * r.dir[k], lo[k]), hi[k]);
}

// Where an iteration starts: the stop tests at the current point, then the direction, t = 1 and the first trial point of the arc search.
REFINE_HD static inline void refine_begin_iteration(const RefineRow& r, const double* lo, const double* hi, const RefineSettings& s) {
  REFINE_FP_STRICT
  const int d = s.d, m = s.m;
  if (*r.iters >= s.maxiter) { *r.reason = REFINE_MAXITER; return; }
  // projected gradient (components pushing out of the box are not free) into q
  double pgmax = 0.0;
  bool nan = false;
  for (int k = 0; k < d; ++k) {
    const bool out = (r.x[k] <= lo[k] && r.g[k] > 0.0) || (r.x[k] >= hi[k] && r.g[k] < 0.0);
    r.q[k] = out ? 0.0 : r.g[k];
    const double v = std::fabs(r.q[k]);
    nan = nan || v != v;
    if (v > pgmax) pgmax = v;
  }
  if (nan) { *r.reason = REFINE_NAN_GRADIENT; return; }
  if (!(pgmax > s.pgtol)) { *r.reason = REFINE_PGTOL; return; }
  if (s.maxfun >= 0 && !(*r.nfun < s.maxfun)) { *r.reason = REFINE_MAXFUN; return; }
  // r.dir holds the projected gradient while the recursion runs on q (free[k] <=> dir[k] != 0)
  for (int k = 0; k < d; ++k) r.dir[k] = r.q[k];
  const int head = *r.iters % m;
  for (int jj = 0; jj < m; ++jj) {                         // newest -> oldest
    const int j = ((head - 1 - jj) % m + m) % m;
    const double* sv = r.S + (size_t)j * d;
    const double* yv = r.Y + (size_t)j * d;
    double dot = 0.0;
    for (int k = 0; k < d; ++k) dot += (r.dir[k] != 0.0 ? sv[k] : 0.0) * r.q[k];
    r.alphas[j] = r.rho[j] * dot;
    for (int k = 0; k < d; ++k) r.q[k] -= r.alphas[j] * (r.dir[k] != 0.0 ? yv[k] : 0.0);
  }
  // no curvature pair yet: L-BFGS-B's first move -- a unit step along the projected steepest descent on a fully boxed problem, a step of
  // length 1 when some variable is unbounded
  double g0;
  if (*r.gamma > 0.0) g0 = *r.gamma;
  else if (s.boxed) g0 = 1.0;
  else {
    double qq = 0.0;
    for (int k = 0; k < d; ++k) qq += r.q[k] * r.q[k];
    g0 = 1.0 / std::fmax(std::sqrt(qq), 1e-300);
  }
  for (int k = 0; k < d; ++k) r.z[k] = r.q[k] * g0;
  for (int jj = m - 1; jj >= 0; --jj) {                    // oldest -> newest
    const int j = ((head - 1 - jj) % m + m) % m;
    const double* sv = r.S + (size_t)j * d;
    const double* yv = r.Y + (size_t)j * d;
    double dot = 0.0;
    for (int k = 0; k < d; ++k) dot += (r.dir[k] != 0.0 ? yv[k] : 0.0) * r.z[k];
    const double beta = r.rho[j] * dot;
    for (int k = 0; k < d; ++k) r.z[k] += (r.dir[k] != 0.0 ? sv[k] : 0.0) * (r.alphas[j] - beta);
  }
  double slope = 0.0;
  for (int k = 0; k < d; ++k) {
    r.q[k] = r.dir[k];                                     // (the projected gradient, kept for the restart below)
    r.dir[k] = r.dir[k] != 0.0 ? -r.z[k] : 0.0;
    slope += r.dir[k] * r.g[k];
  }
  if (!(slope < 0.0)) {                                    // not a descent direction: steepest descent, drop the history
    double nrm = 1.0;
    if (!s.boxed) {
      double pp = 0.0;
      for (int k = 0; k < d; ++k) pp += r.q[k] * r.q[k];
      nrm = std::fmax(std::sqrt(pp), 1e-300);
    }
    for (int k = 0; k < d; ++k) r.dir[k] = -r.q[k] / nrm;
    for (int j = 0; j < m; ++j) r.rho[j] = 0.0;
    *r.gamma = 0.0;
  }
  *r.t = 1.0;
  *r.ls = 0;
  refine_trial_point(r, lo, hi, d);
}

// f, g: the objective and its gradient at refine_point(r).  A stopped row is frozen: nothing of it is written.
REFINE_HD static inline void refine_advance(const RefineRow& r, double f, const double* g, const double* lo, const double* hi, const RefineSettings& s) {
  REFINE_FP_STRICT
  if (*r.reason != REFINE_RUNNING) return;
  const int d = s.d, m = s.m;
  const double eps = 2.220446049250313e-16;
  ++*r.nfun;
  if (!*r.started) {                                       // the value at the clamped start
    *r.started = 1;
    *r.f = f;
    for (int k = 0; k < d; ++k) r.g[k] = g[k];
    if (!std::isfinite(f)) { *r.reason = REFINE_NONFINITE_START; return; }
    refine_begin_iteration(r, lo, hi, s);
    return;
  }
  // a trial point of the Armijo search along the projection arc x(t) = P(x + t dir)
  double decrease = 0.0;
  for (int k = 0; k < d; ++k) decrease += r.g[k] * (r.xt[k] - r.x[k]);
  if (std::isfinite(f) && f <= *r.f + s.c1 * decrease) {
    const int head = *r.iters % m;
    double* sv = r.S + (size_t)head * d;
    double* yv = r.Y + (size_t)head * d;
    double sy = 0.0, yy = 0.0;
    for (int k = 0; k < d; ++k) {
      sv[k] = r.xt[k] - r.x[k];
      yv[k] = g[k] - r.g[k];
      sy += sv[k] * yv[k];
      yy += yv[k] * yv[k];
    }
    if (sy > eps * yy) {                                   // L-BFGS-B's curvature test (the slot stays empty otherwise)
      r.rho[head] = 1.0 / sy;
      *r.gamma = sy / yy;
    } else {
      for (int k = 0; k < d; ++k) sv[k] = yv[k] = 0.0;
      r.rho[head] = 0.0;
    }
    const double rel = (*r.f - f) / std::fmax(std::fmax(std::fabs(*r.f), std::fabs(f)), 1.0);
    for (int k = 0; k < d; ++k) {
      r.x[k] = r.xt[k];
      r.g[k] = g[k];
    }
    *r.f = f;
    ++*r.iters;
    if (rel <= s.factr * eps) { *r.reason = REFINE_FACTR; return; }
    refine_begin_iteration(r, lo, hi, s);
    return;
  }
  // rejected: safeguarded quadratic interpolation of f along the arc
  const double t = *r.t;
  const double num = -decrease * t, den = 2.0 * (f - *r.f - decrease);
  const double tq = (std::isfinite(den) && den > 0.0) ? num / den : 0.5 * t;
  *r.t = std::fmin(std::fmax(tq, 0.1 * t), 0.5 * t);
  if (++*r.ls >= s.max_ls) { *r.reason = REFINE_ARC_FAILED; return; }
  refine_trial_point(r, lo, hi, d);
}

// evaluations a row can take at most: the start, then max_ls trial points per iteration (maxfun is tested where an iteration starts, so it
// cuts at the end of the arc search in which it was reached); the pass budget of a driver that evaluates every running row once per pass
REFINE_HD static inline long long refine_pass_budget(const RefineSettings& s) {
  long long b = 1 + (long long)s.maxiter * s.max_ls;
  if (s.maxfun >= 0) {
    const long long c = (long long)(s.maxfun > 1 ? s.maxfun : 1) + s.max_ls;
    if (c < b) b = c;
  }
  return b;
}

REFINE_FP_END
