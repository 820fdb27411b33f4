// Pending-point entry points of the C ABI (include/bocf_hip.h): bocf_set_pending_points, bocf_get_pending_samples, bocf_acq_pending -- the
// Monte-Carlo improvement of the composite utility at the resident candidates, conditioned on joint samples at r <= 15 pending points (the
// greedy fill of a q-point batch).  The kernels are pending.hip; the pending points are staged like a reference set (bocf_kg_stage) in
// buffers of their own, Sigma(P, P) comes from launch_post_cov, its small factorizations from the host (pending_host.h), the per-chunk
// V / Sigma(candidates, P) / gradients from the look-ahead's chunk helpers (capi_kg.hip).  fp64 only: options predict_f32 / predict_i8 are
// not read here.  One stream, one synchronisation per call.
#include "bocf_ctx.h"
#include "pending_host.h"

#include <cstring>
#include <vector>

void bocf_pending_drop(bocf_ctx* c) { c->pd_r = 0; }

static const char* kWorkspace = "the look-ahead workspace exceeds option workspace_mb: fewer candidates or a larger cap";

extern "C" int bocf_set_pending_points(bocf_ctx* c, const double* Xp, int r, const double* Zp, int S, int max_jitter_tries, double* jitter_out) {
  static const char* who = "bocf_set_pending_points";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  if (!Xp) return fail(who, "null Xp");
  if (r < 1 || r > PENDING_MAX_R) return fail(who, "r out of range (1 .. 15)");
  if (!Zp) return fail(who, "null Zp");
  if (S < 1 || S > 256) return fail(who, "S out of range (1 .. 256)");
  if (c->S_mc < 1) return fail(who, "no Monte-Carlo samples set (bocf_set_mc_samples)");
  if (S != c->S_mc) return fail(who, "S must equal the number of resident Monte-Carlo samples (bocf_set_mc_samples)");
  if (c->d > BOCF_MAX_D) return fail(who, "input dimension too large");
  int j0, M, m;
  if (bocf_group_range(who, bocf_call_state(c), -1, &j0, &M, &m) || bocf_check_group_fits(who, m)) return -1;
  const int Np = c->Np, d = c->d, rp = BOCF_TILE;
  if (2.0 * M * (double)Np * rp * sizeof(double) > (double)c->workspace_mb * 1048576.0) return fail(who, kWorkspace);
  HIPCHK(hipSetDevice(c->device));
  c->pd_r = 0;                                               // (replaced below, or gone if this call fails)
  const size_t rr = (size_t)r * r, npack = (size_t)M * (rr + r), nQ = (size_t)M * rr, nF = (size_t)M * r * S;
  if (c->pd_XP.ensure(sizeof(double) * (size_t)r * d) || c->pd_VP.ensure(sizeof(double) * (size_t)M * Np * rp) ||
      c->pd_Wp.ensure(sizeof(double) * (size_t)M * Np * rp) || c->pd_muP.ensure(sizeof(double) * (size_t)M * rp) ||
      c->pd_cov.ensure(sizeof(double) * (size_t)M * rp * rp) || c->pd_pack.ensure(sizeof(double) * npack) || c->pd_QFG.ensure(sizeof(double) * (nQ + 2 * nF)))
    return -1;
  HIPCHK(hipMemcpyAsync(c->pd_XP.p, Xp, sizeof(double) * (size_t)r * d, hipMemcpyHostToDevice, c->stream));
  if (bocf_kg_stage(c, c->pd_XP.as<double>(), r, rp, c->pd_VP.as<double>(), c->pd_Wp.as<double>(), c->pd_muP.as<double>(), nullptr)) return -1;
  {
    PhaseTimer t(c, "kg_cov");
    launch_post_cov(c->pd_VP.as<double>(), rp, (long)Np * rp, c->pd_VP.as<double>(), rp, (long)Np * rp, c->pd_XP.as<double>(), r, c->pd_XP.as<double>(), r, d, Np,
                    c->kernel_id, BOCF_KIDS(c), c->hypd.as<KernHyp>(), nullptr, 0, c->pd_cov.as<double>(), rp, (long)rp * rp, M, c->stream);
    launch_pending_pack(c->pd_cov.as<double>(), rp, (long)rp * rp, c->pd_muP.as<double>(), rp, r, c->pd_pack.as<double>(), M, c->stream);
  }
  c->pd_host.resize(npack);
  HIPCHK(hipMemcpyAsync(c->pd_host.data(), c->pd_pack.p, sizeof(double) * npack, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  c->pd_up.assign(nQ + 2 * nF, 0.0);
  std::vector<double> tau(M, 0.0);
  const int bad = pending_prepare(c->pd_host.data(), c->pd_host.data() + nQ, M, m, r, Zp, S, max_jitter_tries, tau.data(), nullptr, c->pd_up.data(),
                                  c->pd_up.data() + nQ, c->pd_up.data() + nQ + nF);
  if (jitter_out) memcpy(jitter_out, tau.data(), sizeof(double) * M);
  if (bad) {
    bocf_set_error("bocf_set_pending_points: the covariance of the pending points is not positive definite, even with jitter.");
    return bad;
  }
  // (the upload reads pd_up, which lives in the context: the stream orders it before the first bocf_acq_pending)
  HIPCHK(hipMemcpyAsync(c->pd_QFG.p, c->pd_up.data(), sizeof(double) * (nQ + 2 * nF), hipMemcpyHostToDevice, c->stream));
  c->pd_r = r;
  c->pd_S = S;
  return 0;
}

extern "C" int bocf_get_pending_samples(bocf_ctx* c, double* F_out) {
  static const char* who = "bocf_get_pending_samples";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  if (c->pd_r < 1) return fail(who, "no pending points: call bocf_set_pending_points after the fit");
  if (!F_out) return fail(who, "null F_out");
  const size_t nQ = (size_t)c->m * c->pd_r * c->pd_r, nF = (size_t)c->m * c->pd_r * c->pd_S;
  memcpy(F_out, c->pd_up.data() + nQ, sizeof(double) * nF);
  return 0;
}

extern "C" int bocf_acq_pending(bocf_ctx* c, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                                const double* prob, int L, double* acq_out, double* dacq_out) {
  static const char* who = "bocf_acq_pending";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, prob, L};
  const int m = bocf_pending_check(who, bocf_call_state(c), u);
  if (m < 0) return -1;
  const int Ha = bocf_acq_hyper_count(c);
  const int mg = Ha * m;
  const int C = c->C, d = c->d, N = c->N, r = c->pd_r, S = c->pd_S, rp = BOCF_TILE;
  const bool grad = dacq_out != nullptr;
  const int chunk = bocf_kg_chunk_size(c, mg);
  if (chunk < BOCF_TILE) return fail(who, kWorkspace);
  if (grad) {
    // one chunk: d Sigma / dx of every (candidate, pending point) is held at once (the optimiser's small batches)
    if ((double)mg * C * (double)r * d * sizeof(double) > (double)c->workspace_mb * 1048576.0 || round_up(C, BOCF_TILE) > chunk) return fail(who, kWorkspace);
  }
  HIPCHK(hipSetDevice(c->device));
  // theta | prob | utility parameters in one upload
  const UtilPack& pk = bocf_util_pack(u, nullptr, 0, &c->util_up);
  const int cap = round_up(C < chunk ? C : chunk, BOCF_TILE);
  if (c->pd_best.ensure(sizeof(double) * (size_t)Ha * L) || c->pd_T.ensure(sizeof(double) * (size_t)Ha * L * S) ||
      c->pd_muc.ensure(sizeof(double) * (size_t)mg * cap) || c->acq.ensure(sizeof(double) * (size_t)round_up(C, BOCF_TILE)))
    return -1;
  if (grad && (c->kg_dout.ensure(sizeof(double) * (size_t)C * d) || c->pd_E.ensure(sizeof(double) * (size_t)C * m * S))) return -1;
  c->have_acq = false;
  if (bocf_upload_util(c, pk, &c->pd_par)) return -1;
  const size_t nQ = (size_t)c->m * r * r, nF = (size_t)c->m * r * S;
  const double* Qd = c->pd_QFG.as<double>();
  PendArgs a{};
  a.ldc = rp; a.theta = c->pd_par.as<double>() + pk.theta; a.theta_dim = theta_dim; a.prob = c->pd_par.as<double>() + pk.prob; a.L = L;
  a.util_params = c->pd_par.as<double>() + pk.params;
  a.Wt = c->Wt.as<double>(); a.m = m; a.r = r; a.S = S; a.util_kind = util_kind; a.scale = 1.0 / Ha; a.d = d;
  // thresholds: each hyper-sample's own best-so-far, or that of option best_group for all (the rule of the Monte-Carlo acquisitions),
  // into buffers of this path -- the acquisitions' best-so-far cache is left as it was
  for (int h = 0; h < Ha; ++h) {
    const int gb = bocf_best_group_of(c, h);
    PendArgs t = a;
    t.F = Qd + nQ + (size_t)h * m * r * S;
    double* best = c->pd_best.as<double>() + (size_t)h * L;
    t.best = best; t.T = c->pd_T.as<double>() + (size_t)h * L * S;
    PhaseTimer pt(c, "pending_kernel");
    launch_best_so_far(c->mu_train.as<double>() + (size_t)gb * m * N, N, m, 0, util_kind, a.theta, theta_dim, L, a.util_params, best, c->stream, nullptr);
    launch_pending_threshold(t, c->stream);
  }
  const KgRefSet ref{&c->pd_XP, &c->pd_VP, &c->pd_Wp, r};
  for (int c0 = 0; c0 < C; c0 += chunk) {
    const int cn = C - c0 < chunk ? C - c0 : chunk, cnp = round_up(cn, BOCF_TILE);
    if (bocf_kg_chunk(c, ref, 0, mg, c0, cn, cnp, grad, c->pd_muc.as<double>())) return -1;
    if (grad && bocf_kg_chunk_dcov(c, ref, 0, mg, c0, cn, 0, r)) return -1;
    for (int h = 0; h < Ha; ++h) {
      PendArgs k = a;
      k.cov = c->kg_cov.as<double>() + (size_t)h * m * cnp * rp; k.strideC = (long)cnp * rp;
      k.s2c = c->kg_s2c.as<double>() + (size_t)h * m * cnp; k.muc = c->pd_muc.as<double>() + (size_t)h * m * cnp; k.lds = cnp;
      k.Q = Qd + (size_t)h * m * r * r; k.F = Qd + nQ + (size_t)h * m * r * S; k.G = Qd + nQ + nF + (size_t)h * m * r * S;
      k.T = c->pd_T.as<double>() + (size_t)h * L * S;
      k.C = cn; k.acq = c->acq.as<double>() + c0; k.accumulate = h > 0;
      PhaseTimer pt(c, "pending_kernel");
      launch_pending_acq(k, c->stream);
      if (grad) {
        k.dmu = c->kg_dmean.as<double>() + (size_t)h * m * cnp * d; k.ds2 = c->kg_dvar.as<double>() + (size_t)h * m * cnp * d; k.ldg = cnp;
        k.dcov = c->kg_dcov.as<double>() + (size_t)h * m * cn * r * d;
        k.E = c->pd_E.as<double>(); k.dacq = c->kg_dout.as<double>();
        launch_pending_grad(k, c->stream);
      }
    }
  }
  if (acq_out) HIPCHK(hipMemcpyAsync(acq_out, c->acq.p, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, c->stream));
  if (grad) HIPCHK(hipMemcpyAsync(dacq_out, c->kg_dout.p, sizeof(double) * (size_t)C * d, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  c->have_acq = true;
  return 0;
}
