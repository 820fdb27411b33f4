// bocf_refine_acq (include/bocf_hip.h): the acquisition optimiser's anchor refinement with the loop on the device.  What
// bocf_lbfgsb_batched does between two callbacks -- each a candidate upload, an acquisition pass, a copy back and a synchronisation -- is one
// more launch on the stream here (refine_advance_kernel, refine.hip): a pass is the posterior with its gradients and the acquisition of the
// resident rows, exactly as bocf_acq_linear_grad / bocf_acq_mc_grad enqueue them (bocf_acq_enqueue, capi.hip), then the step, which
// writes every row's next trial point into the resident candidate rows.  The host only enqueues, and every poll_every passes reads ONE word.
#include "bocf_ctx.h"
#include "refine_step.h"

#include <cmath>
#include <utility>

extern "C" int bocf_refine_acq(bocf_ctx* c, int form, int kind, int util_kind, const double* util_params, int n_util_params, const double* theta,
                               int theta_dim, const double* prob, int L, const double* X0, int A, const double* lo, const double* hi, int maxiter, int m,
                               double factr, double pgtol, int max_ls, double c1, int maxfun, int poll_every, double* X_out, double* F_out,
                               int* iters_out, int* nfun_out, int* reason_out, long long* counters_out) {
  const char* me = "bocf_refine_acq";
  if (!c || !c->fitted) return fail(me, "model not fitted");
  if (c->canned) return fail(me, "the context holds a host-given posterior (bocf_set_posterior): fit first");
  if (form != BOCF_REFINE_LINEAR && form != BOCF_REFINE_MC) return fail(me, "unknown form (BOCF_REFINE_LINEAR or BOCF_REFINE_MC)");
  if (A < 1 || A > BOCF_REFINE_MAX_ROWS) return fail(me, "A out of range (1 .. 64)");
  if (!X0 || !lo || !hi || !X_out || !F_out) return fail(me, "null X0, lo, hi, X_out or F_out");
  const int d = c->d;
  if (d < 1 || d > REFINE_MAX_D) return fail(me, "input dimension too large");
  for (int k = 0; k < d; ++k)
    if (!(lo[k] <= hi[k])) return fail(me, "lo > hi (or a NaN bound)");
  if (poll_every < 1) return fail(me, "poll_every must be >= 1");
  if (m < 1 || m > REFINE_MAX_M || max_ls < 1 || maxiter < 0) return fail(me, "need 1 <= m <= 64, max_ls >= 1 and maxiter >= 0");
  if (L < 1 || L > BOCF_MAX_L) return fail(me, "L out of range (1 .. 32)");
  const bool linear = form == BOCF_REFINE_LINEAR;
  int per;
  if (linear) {
    if (kind != BOCF_ACQ_EI && kind != BOCF_ACQ_PI) return fail(me, "unknown acquisition kind");
    if (!theta) return fail(me, "theta is null");
    per = bocf_check_groups(me, bocf_call_state(c), true, true);
    if (per < 0) return -1;
    util_kind = BOCF_UTIL_LINEAR; util_params = nullptr; n_util_params = 0; theta_dim = per;
  } else {
    bool program;                                            // (a resident program is accepted: checked here)
    per = bocf_mc_utility_check(me, bocf_call_state(c), UtilArgs{util_kind, util_params, n_util_params, theta, theta_dim, prob, L}, &program);
    if (per < 0 || (program && bocf_check_resident_program(c, me, per, theta_dim, n_util_params))) return -1;
    if (theta_dim > 0 && !theta) return fail(me, "theta is null");
    if (n_util_params < 0 || n_util_params > BOCF_MAX_M) return fail(me, "bad utility parameters");
    kind = BOCF_ACQ_EI;                                      // (the Monte-Carlo gradient form has no other)
  }
  HIPCHK(hipSetDevice(c->device));
  RefineSettings s;
  s.d = d; s.m = m; s.maxiter = maxiter; s.max_ls = max_ls; s.maxfun = maxfun < 0 ? -1 : maxfun;
  s.factr = factr; s.pgtol = pgtol; s.c1 = c1; s.boxed = refine_boxed(lo, hi, d);
  long long syncs = 0, passes = 0;
  bool uploaded = false;
  if (bocf_acq_upload_params(c, theta, theta_dim, prob, L, util_params, n_util_params, &uploaded)) return -1;
  if (uploaded) ++syncs;
  // ints: the rows' blocks | running rows | small flag | column map (A)
  const size_t nd = (size_t)A * refine_row_doubles(d, m), ni = (size_t)A * REFINE_ROW_INTS + 2 + A;
  // Above the small path of the predict pass the host loop's posterior changes kernels once BOCF_SMALL_N or fewer rows run; to evaluate
  // every point through the kernels the host loop would use, such a batch is predicted twice per pass (refine.hip: refine_compact_kernel)
  const bool two = A > BOCF_SMALL_N;
  if (c->rf_dbl.ensure(sizeof(double) * nd) || c->rf_int.ensure(sizeof(int) * ni)) return -1;
  if (two && (c->rf_x2.ensure(sizeof(double) * BOCF_SMALL_N * d) || c->rf_acq.ensure(sizeof(double) * (size_t)A * (d + 1)))) return -1;
  double* dbl = c->rf_dbl.as<double>();
  int* ints = c->rf_int.as<int>();
  int* running = ints + (size_t)A * REFINE_ROW_INTS;
  int* small = running + 1;
  int* map = running + 2;
  double* acq_all = two ? c->rf_acq.as<double>() : nullptr;
  double* dacq_all = two ? acq_all + A : nullptr;
  // Last of the steps that can fail before anything is enqueued, so that a failed allocation above leaves the resident batch alone: the
  // clamped starts become the resident candidate batch (through the pinned buffer: no synchronisation)
  std::vector<double> Xcl((size_t)A * d);
  for (int a = 0; a < A; ++a)
    for (int k = 0; k < d; ++k) Xcl[(size_t)a * d + k] = std::fmin(std::fmax(X0[(size_t)a * d + k], lo[k]), hi[k]);
  if (bocf_set_candidates(c, Xcl.data(), A)) return -1;
  HIPCHK(hipMemsetAsync(dbl, 0, sizeof(double) * nd, c->stream));
  HIPCHK(hipMemsetAsync(ints, 0, sizeof(int) * ni, c->stream));
  launch_refine_init(c->Xc.as<double>(), dbl, ints, running, A, s, c->stream);
  // No row can take more evaluations than the budget, so the loop ends with every row stopped even if it never polls.  The last, partial
  // group of passes is not polled: the row results say the same.
  const long long budget = refine_pass_budget(s);
  int rc = 0;
  // A poll has shown that no more than BOCF_SMALL_N rows run.  The count only falls, so from then on the gathered rows are all there is
  // to evaluate and the whole-batch posterior is no longer enqueued; the device-side flag was set before the host could know, so the
  // results do not depend on when (or whether) a poll says so.
  bool few = false;
  while (rc == 0 && passes < budget) {
    const long long n = budget - passes < poll_every ? budget - passes : poll_every;
    for (long long i = 0; i < n && rc == 0; ++i) {
      if (!few) rc = bocf_acq_enqueue(c, per, linear, true, kind, util_kind, n_util_params, theta_dim, L);
      // (the buffers are read after the enqueue: the first pass may have grown them)
      if (rc == 0 && !two) launch_refine_advance(c->acq.as<double>(), c->dacq.as<double>(), c->Xc.as<double>(), dbl, ints, running, A, s, lo, hi, c->stream);
      if (rc || !two) continue;
      // the whole batch's values aside, then the first BOCF_SMALL_N running rows as a batch of their own: the gathered rows stand in
      // for the resident candidates while that pass is enqueued
      if (!few && (hipMemcpyAsync(acq_all, c->acq.p, sizeof(double) * A, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
                   hipMemcpyAsync(dacq_all, c->dacq.p, sizeof(double) * (size_t)A * d, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)) {
        rc = fail(me, "device copy of the acquisition vector failed");
        break;
      }
      launch_refine_compact(c->Xc.as<double>(), ints, A, d, c->rf_x2.as<double>(), map, small, c->stream);
      // (run_predict reads the candidates through c->Xc and c->C alone and keeps nothing keyed to them between two calls; state that a
      // later change keys to the candidate batch must be dropped here as bocf_set_candidates drops it)
      std::swap(c->Xc, c->rf_x2);
      c->C = BOCF_SMALL_N;
      rc = bocf_acq_enqueue(c, per, linear, true, kind, util_kind, n_util_params, theta_dim, L);
      std::swap(c->Xc, c->rf_x2);
      c->C = A;
      if (rc == 0)
        launch_refine_advance(acq_all, dacq_all, c->Xc.as<double>(), dbl, ints, running, A, s, lo, hi, c->stream, c->acq.as<double>(), c->dacq.as<double>(),
                              map, small);
    }
    c->have_acq = false;                                   // c->acq belongs to trial points that have moved on
    if (rc) break;
    passes += n;
    if (passes >= budget) break;
    int left = 0;
    rc = bocf_copy_word_out(c, running, &left);
    ++syncs;
    if (left == 0) break;
    few = two && left <= BOCF_SMALL_N;
  }
  if (rc) {
    (void)hipStreamSynchronize(c->stream);
    return -1;
  }
  std::vector<double> hd(nd);
  std::vector<int> hi_((size_t)A * REFINE_ROW_INTS);
  if (bocf_copy_pair_out(c, dbl, hd.data(), sizeof(double) * nd, ints, reinterpret_cast<double*>(hi_.data()), sizeof(int) * hi_.size())) return -1;
  ++syncs;
  for (int a = 0; a < A; ++a) {
    const RefineRow r = refine_row_view(hd.data() + (size_t)a * refine_row_doubles(d, m), hi_.data() + (size_t)a * REFINE_ROW_INTS, d, m);
    for (int k = 0; k < d; ++k) X_out[(size_t)a * d + k] = r.x[k];
    F_out[a] = *r.f;
    if (iters_out) iters_out[a] = *r.iters;
    if (nfun_out) nfun_out[a] = *r.nfun;
    if (reason_out) reason_out[a] = *r.reason;
  }
  if (counters_out) {
    counters_out[0] = passes;
    counters_out[1] = syncs;
  }
  return 0;
}
