// How a runtime (input dimension, kernel id) reaches a <D, family> instantiation, and how a list of per-output kernel ids becomes one launch
// per run of equal ids.  Host only, no HIP include: tests/kern_dispatch_driver.cpp compiles it with a plain C++ compiler.
//
// A launcher has one shape -- the runs, the run's pointer offsets, then the dispatch with a generic lambda:
//   bocf_family_runs(kernel_id, kids, m, [&](int j0, int mr, int kid) {
//     bocf_launch_by_d("some_kernel", d, [&](auto Dc) {                 // (bocf_internal.h: bocf_dispatch_d + the failure report)
//       bocf_dispatch_family(kid, [&](auto Kc) {
//         constexpr int D = decltype(Dc)::value, KID = decltype(Kc)::value;
//         BOCF_LAUNCH((some_kernel<D, KID>), grid, block, 0, s, Xs + (long)j0 * strideXs, ...);
//       });
//     });
//   });
// The instantiations are the 32 x 3 the kernels always had: every lambda body is instantiated once per constant it is called with.
#pragma once
#include <type_traits>
#include <utility>

#define BOCF_MAX_D 32          // max input dimension

// f(std::integral_constant<int, d>) for 1 <= d <= BOCF_MAX_D; returns whether it called f.  A launcher that gets false launches nothing and
// must say so (bocf_launch_by_d records hipErrorInvalidValue under the kernel's name, so the entry point fails at its launch check and does
// not hand back stale buffers).  Not reachable through the C API: a fit refuses d < 1 and d > BOCF_MAX_D, and every later entry point works
// on a fitted context.
template <typename F, int... I>
static inline bool bocf_dispatch_d_seq(int d, F& f, std::integer_sequence<int, I...>) {
  return ((d == I + 1 ? (f(std::integral_constant<int, I + 1>{}), true) : false) || ...);
}
template <typename F>
static inline bool bocf_dispatch_d(int d, F f) {
  return bocf_dispatch_d_seq(d, f, std::make_integer_sequence<int, BOCF_MAX_D>{});
}

// f(std::integral_constant<int, family>), family in {0, 2, 3}: kernel ids 0 (RBF) and 1 (SE) are the same function and share family 0,
// 2 is Matern52, everything else Matern32.  The one place on the host that maps an id to the family the kernels are specialised for.
template <typename F>
static inline void bocf_dispatch_family(int kernel_id, F f) {
  if (kernel_id <= 1) f(std::integral_constant<int, 0>{});
  else if (kernel_id == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 3>{});
}

// Outputs may use different kernel FAMILIES (the reference's multi_outputGP takes a kernel list, multi_outputGP.py:44-47).  The kernels
// that evaluate a covariance function are specialised per family at compile time, so a launcher that is given `kids` (host array of m
// kernel ids, or nullptr = every output uses `kernel_id`) issues one launch per RUN of equal ids, with its pointers advanced to the
// run's first output: f(j0, m_run, kernel_id_of_the_run).
template <typename F>
static inline void bocf_family_runs(int kernel_id, const int* kids, int m, F f) {
  if (!kids) {
    f(0, m, kernel_id);
    return;
  }
  for (int j0 = 0; j0 < m;) {
    int j1 = j0 + 1;
    while (j1 < m && kids[j1] == kids[j0]) ++j1;
    f(j0, j1 - j0, kids[j0]);
    j0 = j1;
  }
}
