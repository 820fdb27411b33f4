// Joint q-point entry point of the C ABI (include/bocf_hip.h): bocf_acq_joint -- the Monte-Carlo expected improvement of the composite
// utility at whole batches of q <= 8 points, the resident candidates read as B = C / q batches.  The kernels are joint.hip; V = R^T K(X, .)
// and the mean come from bocf_enqueue_V, Sigma between the points of a chunk from launch_post_cov, the gradient form's Ky^-1 K*, d mu / dx,
// d sigma^2 / dx and d Sigma / dx from the look-ahead's kernels -- all into buffers of this path (jt_*): the Monte-Carlo samples, the
// reference set, the pending points, the paths and the utility program stay resident and valid.  fp64 only: options predict_f32 /
// predict_i8 are not read here.  One stream, one synchronisation per call.
#include "bocf_ctx.h"
#include "joint_chol.h"

#define JOINT_MAX_CHUNK 512      // points per chunk of the value form: Sigma of a chunk is formed whole (chunk^2 entries per output)
#define JOINT_MAX_GRAD_POINTS 128

static const char* kWorkspace = "the joint workspace exceeds option workspace_mb: fewer candidates or a larger cap";

extern "C" int bocf_acq_joint(bocf_ctx* c, int q, const double* Z, int S, int util_kind, const double* util_params, int n_util_params, const double* theta,
                              int theta_dim, const double* prob, int L, const double* best, double* acq_out, double* dacq_out, int* floored_out) {
  static const char* who = "bocf_acq_joint";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, prob, L};
  const int m = bocf_joint_check(who, bocf_call_state(c), u, q, Z, S);
  if (m < 0) return -1;
  const int Ha = bocf_acq_hyper_count(c);
  const int mg = Ha * m;
  const int C = c->C, d = c->d, N = c->N, Np = c->Np, B = C / q;
  const bool grad = dacq_out != nullptr;
  const double cap = (double)c->workspace_mb * 1048576.0;
  // points per chunk: V (Np x chunk) and Sigma (chunk x chunk) of every output under the cap, whole batches only
  int chunk = bocf_kg_chunk_size(c, mg);
  if (chunk > JOINT_MAX_CHUNK) chunk = JOINT_MAX_CHUNK;
  while (chunk >= BOCF_TILE && (double)mg * chunk * ((double)Np + chunk) * sizeof(double) > cap) chunk -= BOCF_TILE;
  if (chunk < BOCF_TILE) return fail(who, kWorkspace);
  if (grad) {
    // one chunk: Ky^-1 K* and d Sigma / dx between all points are held at once (the optimiser's batch: 16 anchors of q = 8)
    if (C > JOINT_MAX_GRAD_POINTS) return fail(who, "the gradient form takes at most 128 points (B q <= 128)");
    if ((double)mg * BOCF_TILE * (2.0 * Np + BOCF_TILE + (double)C * d) * sizeof(double) > cap) return fail(who, kWorkspace);
  }
  const int pts = chunk / q * q, cap_p = round_up(C < pts ? C : pts, BOCF_TILE);
  HIPCHK(hipSetDevice(c->device));
  // theta | prob | utility parameters | Z transposed to (m, q, S) | the caller's incumbents (Ha, L) in one upload
  const size_t nZ = (size_t)m * q * S, nbest = best ? (size_t)Ha * L : 0;
  c->jt_tail.assign(nZ + nbest, 0.0);
  for (int s = 0; s < S; ++s)
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < q; ++i) c->jt_tail[((size_t)j * q + i) * S + s] = Z[((size_t)s * m + j) * q + i];
  for (size_t i = 0; i < nbest; ++i) c->jt_tail[nZ + i] = best[i];
  const UtilPack& pk = bocf_util_pack(u, c->jt_tail.data(), c->jt_tail.size(), &c->util_up);
  if (c->jt_best.ensure(sizeof(double) * (size_t)Ha * L) || c->jt_fl.ensure(sizeof(int) * (size_t)B) ||
      c->jt_V.ensure(sizeof(double) * (size_t)mg * Np * cap_p) || c->jt_mu.ensure(sizeof(double) * (size_t)mg * cap_p) ||
      c->jt_cov.ensure(sizeof(double) * (size_t)mg * cap_p * cap_p) || c->acq.ensure(sizeof(double) * (size_t)round_up(C, BOCF_TILE)))
    return -1;
  if (grad && (c->jt_W.ensure(sizeof(double) * (size_t)mg * Np * cap_p) || c->jt_dmean.ensure(sizeof(double) * (size_t)mg * cap_p * d) ||
               c->jt_dvar.ensure(sizeof(double) * (size_t)mg * cap_p * d) || c->jt_dcov.ensure(sizeof(double) * (size_t)mg * C * C * d) ||
               c->jt_E.ensure(sizeof(double) * (size_t)C * m * S) || c->jt_dout.ensure(sizeof(double) * (size_t)C * d)))
    return -1;
  c->have_acq = false;
  if (bocf_upload_util(c, pk, &c->jt_par)) return -1;
  const double* par = c->jt_par.as<double>();
  JointArgs a{};
  a.theta = par + pk.theta; a.theta_dim = theta_dim; a.prob = par + pk.prob; a.L = L; a.util_params = par + pk.params; a.Zt = par + pk.tail;
  a.m = m; a.q = q; a.S = S; a.util_kind = util_kind; a.scale = 1.0 / Ha; a.d = d;
  // incumbents: the caller's, or each hyper-sample's own best-so-far / that of option best_group for all (the rule of the Monte-Carlo
  // acquisitions) into a buffer of this path -- the acquisitions' best-so-far cache is left as it was
  const double* bests = best ? par + pk.tail + nZ : c->jt_best.as<double>();
  if (!best)
    for (int h = 0; h < Ha; ++h) {
      const int gb = bocf_best_group_of(c, h);
      PhaseTimer pt(c, "joint_kernel");
      launch_best_so_far(c->mu_train.as<double>() + (size_t)gb * m * N, N, m, 0, util_kind, a.theta, theta_dim, L, a.util_params,
                         c->jt_best.as<double>() + (size_t)h * L, c->stream, nullptr);
    }
  const int* kids = BOCF_KIDS(c);
  for (int p0 = 0; p0 < C; p0 += pts) {
    const int cn = C - p0 < pts ? C - p0 : pts, cnp = round_up(cn, BOCF_TILE);
    const double* Xq = c->Xc.as<double>() + (size_t)p0 * d;
    {
      PhaseTimer t(c, "joint_V");
      if (bocf_enqueue_V(c, 0, mg, Xq, cn, cnp, c->jt_V.as<double>(), c->jt_mu.as<double>())) return -1;
    }
    {
      PhaseTimer t(c, "joint_cov");
      launch_post_cov(c->jt_V.as<double>(), cnp, (long)Np * cnp, c->jt_V.as<double>(), cnp, (long)Np * cnp, Xq, cn, Xq, cn, d, Np, c->kernel_id, kids,
                      c->hypd.as<KernHyp>(), nullptr, 0, c->jt_cov.as<double>(), cnp, (long)cnp * cnp, mg, c->stream);
    }
    if (grad) {
      PhaseTimer t(c, "joint_grad");
      GemmArgs w{};                                          // W = R V (R k-major = RT; the contraction of row tile rt starts at its diagonal block)
      w.A = c->RT.as<double>(); w.lda = Np; w.strideA = (long)Np * Np;
      w.B = c->jt_V.as<double>(); w.ldb = cnp; w.strideB = (long)Np * cnp;
      w.Cin = nullptr; w.Cout = c->jt_W.as<double>(); w.ldc = cnp; w.strideC = (long)Np * cnp;
      w.M = Np; w.Ncols = cnp; w.K = Np; w.kb = Np; w.kbeg_rt = BOCF_TILE; w.alpha = 1.0;
      launch_gemm_f64(w, mg, 0, c->stream);
      launch_grad_kernel(c->Xs.as<double>(), c->xs_stride, N, Np, d, c->kernel_id, c->hypd.as<KernHyp>(), Xq, 0, cn, c->alpha.as<double>(),
                         c->jt_W.as<double>(), cnp, (long)Np * cnp, c->jt_dmean.as<double>(), c->jt_dvar.as<double>(), cnp, mg, c->stream, kids);
      launch_cov_grad(c->Xs.as<double>(), c->xs_stride, N, d, c->kernel_id, kids, c->hypd.as<KernHyp>(), Xq, cn, Xq, 0, cn, c->jt_W.as<double>(), cnp,
                      (long)Np * cnp, c->jt_dcov.as<double>(), mg, c->stream);
    }
    for (int h = 0; h < Ha; ++h) {
      JointArgs k = a;
      k.cov = c->jt_cov.as<double>() + (size_t)h * m * cnp * cnp; k.ldc = cnp; k.strideC = (long)cnp * cnp;
      k.mu = c->jt_mu.as<double>() + (size_t)h * m * cnp; k.ldm = cnp;
      k.best = bests + (size_t)h * L;
      k.B = cn / q; k.acq = c->acq.as<double>() + p0 / q; k.floored = c->jt_fl.as<int>() + p0 / q; k.accumulate = h > 0;
      PhaseTimer pt(c, "joint_kernel");
      if (grad) {
        k.dmu = c->jt_dmean.as<double>() + (size_t)h * m * cnp * d; k.ds2 = c->jt_dvar.as<double>() + (size_t)h * m * cnp * d; k.ldg = cnp;
        k.dcov = c->jt_dcov.as<double>() + (size_t)h * m * cn * cn * d; k.Cn = cn;
        k.E = c->jt_E.as<double>(); k.dacq = c->jt_dout.as<double>();
        launch_joint_grad(k, c->stream);
      } else {
        launch_joint_acq(k, c->stream);
      }
    }
  }
  launch_joint_tail(c->acq.as<double>(), B, C, c->stream);
  if (acq_out) HIPCHK(hipMemcpyAsync(acq_out, c->acq.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
  if (grad) HIPCHK(hipMemcpyAsync(dacq_out, c->jt_dout.p, sizeof(double) * (size_t)C * d, hipMemcpyDeviceToHost, c->stream));
  if (floored_out) HIPCHK(hipMemcpyAsync(floored_out, c->jt_fl.p, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  c->have_acq = true;
  return 0;
}
