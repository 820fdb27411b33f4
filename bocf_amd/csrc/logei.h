// Log-space expected improvement (definitions: include/bocf_hip.h): what capi_logei.hip hands to the kernels of
// logei.hip.  One launch covers every hyper-sample: all H m rows of the posterior are resident, so the log-sum-exp over (h, l[, s]) is
// closed inside the kernel and nothing is combined across launches.
#pragma once
#include "bocf_internal.h"

struct LogEiArgs {
  const double* mean; const double* var; long ld;   // (H m, ld): rows [h m, (h + 1) m) are hyper-sample h; first C columns valid
  const double* dmean; const double* dvar; long ldg; int d;   // gradient forms: (H m, ldg, d)
  int m, C, L, H;
  int util_kind, theta_dim;
  const double* theta; const double* prob;          // device (L, theta_dim), (L)
  const double* best; int best_stride;              // device incumbents: hyper-sample h reads best + h * best_stride (0: one row for all)
  const double* util_params;                        // (BOCF_MAX_M)
  const double* Wt; int S;                          // device (m, S) transposed normals (Monte-Carlo form)
  double tau;                                       // temperature of the Monte-Carlo form, in utility units
  double* acq; double* dacq;                        // device (C), (C, d)
  const UtilProg* prog;                             // HOST pointer, read by the launcher only: the resident program when util_kind is BOCF_UTIL_PROGRAM
};
void launch_logei_linear(const LogEiArgs& a, bool grad, hipStream_t s);
void launch_logei_mc(const LogEiArgs& a, bool grad, hipStream_t s);
