// Leave-one-out entry points of the C ABI (include/bocf_hip.h): bocf_loo, bocf_loo_utility.  The kernels are loo.hip; the expected
// utility over the leave-one-out posteriors is launch_eu (eu.hip / util_prog.hip) pointed at them with C = N.  Both work on a fitted
// model, read R, alpha, the centred targets and the hyper-parameters only, keep their results in buffers of their own (the predict,
// candidate, acquisition, sample, best-so-far, reference, pending, Thompson and path state is left as it was) and recompute what they
// read on every call: after bocf_append, bocf_update_targets or a refit there is nothing stale to serve.  One stream, one
// synchronisation per call.
#include "bocf_ctx.h"

// mean | variance | log density of the outputs [j0, j0 + mg) into their rows of loo_out (three planes of m x Np)
static int loo_enqueue(bocf_ctx* c, const char* who, int flags, int j0, int mg) {
  const int N = c->N, Np = c->Np, m = c->m;
  if ((int)c->jitter.size() != m || (int)c->hyp.size() != m) return fail(who, "the fit left no per-output jitter / hyper-parameters");
  const size_t plane = (size_t)m * Np;
  if (c->loo_out.ensure(sizeof(double) * 3 * plane) || c->loo_sum.ensure(sizeof(double) * m) || c->loo_shift.ensure(sizeof(double) * m)) return -1;
  // what the fit added to the diagonal besides the noise: 1e-8 + the jitter of the rung it stopped at (build_train_kernel, fit.hip)
  c->loo_shift_host.resize(m);
  for (int j = 0; j < m; ++j) c->loo_shift_host[j] = 1e-8 + (c->jitter[j] - c->test_diag_shift);
  HIPCHK(hipMemcpyAsync(c->loo_shift.p, c->loo_shift_host.data(), sizeof(double) * m, hipMemcpyHostToDevice, c->stream));
  double* out = c->loo_out.as<double>();
  PhaseTimer t(c, "loo");
  launch_loo(c->R.as<double>() + (size_t)j0 * Np * Np, (long)Np * Np, N, Np, c->alpha.as<double>() + (size_t)j0 * Np, c->yc.as<double>() + (size_t)j0 * Np,
             c->hypd.as<KernHyp>() + j0, c->loo_shift.as<double>() + j0, flags, out + (size_t)j0 * Np, out + plane + (size_t)j0 * Np,
             out + 2 * plane + (size_t)j0 * Np, Np, mg, c->stream);
  return 0;
}

extern "C" int bocf_loo(bocf_ctx* c, int flags, double* mean_out, double* var_out, double* lpd_out, double* lpd_sum_out) {
  static const char* who = "bocf_loo";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  if (flags & ~(BOCF_ADD_NOISE | BOCF_CLIP)) return fail(who, "unknown flags (BOCF_ADD_NOISE | BOCF_CLIP)");
  HIPCHK(hipSetDevice(c->device));
  const int N = c->N, Np = c->Np, m = c->m;
  if (loo_enqueue(c, who, flags, 0, m)) return -1;
  const size_t plane = (size_t)m * Np;
  const double* out = c->loo_out.as<double>();
  launch_loo_sum(out + 2 * plane, Np, N, c->loo_sum.as<double>(), m, c->stream);
  double* host[3] = {mean_out, var_out, lpd_out};
  for (int k = 0; k < 3; ++k)
    if (host[k])
      HIPCHK(hipMemcpy2DAsync(host[k], sizeof(double) * N, out + k * plane, sizeof(double) * Np, sizeof(double) * N, (size_t)m, hipMemcpyDeviceToHost, c->stream));
  if (lpd_sum_out) HIPCHK(hipMemcpyAsync(lpd_sum_out, c->loo_sum.p, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  return 0;
}

extern "C" int bocf_loo_utility(bocf_ctx* c, int group, int flags, int mode, int util_kind, const double* util_params, int n_util_params,
                                const double* theta, int theta_dim, int L, double* val_out) {
  static const char* who = "bocf_loo_utility";
  const CallState st = bocf_call_state(c);
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, nullptr, L};
  bool program;
  const int m = bocf_loo_utility_check(who, st, group, flags, mode, u, &program);
  if (m < 0 || (program && bocf_check_resident_program(c, who, m, theta_dim, n_util_params))) return -1;
  if (bocf_loo_utility_check_call(who, st, mode, L, m, val_out)) return -1;
  HIPCHK(hipSetDevice(c->device));
  const int N = c->N, Np = c->Np, j0 = group * m;            // hyper-sample `group` is outputs [j0, j0 + m)
  const UtilPack& pk = bocf_util_pack(u, nullptr, 0, &c->util_up);
  if (c->loo_rows.ensure(sizeof(int) * (size_t)L * N) || c->loo_val.ensure(sizeof(double) * (size_t)L * N)) return -1;
  if (loo_enqueue(c, who, flags, j0, m)) return -1;
  if (bocf_upload_util(c, pk, &c->loo_par)) return -1;
  launch_loo_rows(c->loo_rows.as<int>(), N, L, c->stream);
  const size_t plane = (size_t)c->m * Np;
  EuArgs a{};
  a.mean = c->loo_out.as<double>() + (size_t)j0 * Np; a.var = c->loo_out.as<double>() + plane + (size_t)j0 * Np; a.ld = Np;
  a.m = m; a.C = N; a.mode = mode; a.util_kind = util_kind; a.theta_dim = theta_dim; a.d = c->d;
  a.theta = c->loo_par.as<double>() + pk.theta; a.util_params = c->loo_par.as<double>() + pk.params;
  a.Zt = c->eu_Z.as<double>(); a.S = c->eu_S;
  a.grad = nullptr; a.accumulate = 0;
  a.scale = mode == BOCF_EU_MC ? 1.0 / c->eu_S : 1.0;        // the MEAN over the S normals (not bocf_expected_utility's sum)
  a.prog = &c->prog;
  for (int l = 0; l < L; ++l) {
    a.rows = c->loo_rows.as<int>() + (size_t)l * N;
    a.val = c->loo_val.as<double>() + (size_t)l * N;
    PhaseTimer t(c, "loo_eu");
    launch_eu(a, c->stream);
  }
  HIPCHK(hipMemcpyAsync(val_out, c->loo_val.p, sizeof(double) * (size_t)L * N, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  return 0;
}
