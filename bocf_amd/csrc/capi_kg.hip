// Look-ahead posterior and knowledge-gradient entry points of the C ABI (include/bocf_hip.h): bocf_set_ref_points, bocf_cov_to_ref,
// bocf_conditioned_variance, bocf_acq_kg.  The kernels are kg.hip; V = R^T K(X, .) comes from the predict path's cross kernel and fp64 GEMM
// (bocf_enqueue_V), the covariances Sigma(candidates, A) = k - V_c^T V_A from the joint posterior's rectangular kernel (launch_post_cov),
// d sigma^2 / dx from grad_kernel.  fp64 only: options predict_f32 / predict_i8 are not read here.  One stream, one synchronisation per call.
#include "bocf_ctx.h"

#include <vector>

#define KG_MAX_REF 1024
#define KG_MAX_CHUNK 8192

void bocf_kg_drop(bocf_ctx* c) { c->kg_na = 0; }

static KgRefSet kg_ref(bocf_ctx* c) { return KgRefSet{&c->kg_XA, &c->kg_VA, &c->kg_Wa, c->kg_na}; }

static const char* kWorkspace = "the look-ahead workspace exceeds option workspace_mb: fewer candidates or a larger cap";

// candidates per chunk: V of a chunk (mg x Np x chunk doubles) stays under the cap; 0 when not even 128 fit
int bocf_kg_chunk_size(const bocf_ctx* c, int mg) {
  const double cap = (double)c->workspace_mb * 1048576.0;
  const double per_col = (double)mg * (double)c->Np * sizeof(double);
  long cols = (long)(cap / per_col) / BOCF_TILE * BOCF_TILE;
  if (cols > KG_MAX_CHUNK) cols = KG_MAX_CHUNK;
  const int Cp = round_up(c->C, BOCF_TILE);
  if (cols > Cp) cols = Cp;
  return (int)cols;
}

// W = R V for the mg outputs from j0 (R k-major = RT; the contraction of row tile rt starts at its diagonal block)
static void kg_enqueue_W(bocf_ctx* c, int j0, int mg, const double* V, int npad, double* W) {
  const int Np = c->Np;
  GemmArgs w{};
  w.A = c->RT.as<double>() + (long)j0 * Np * Np; w.lda = Np; w.strideA = (long)Np * Np;
  w.B = V; w.ldb = npad; w.strideB = (long)Np * npad;
  w.Cin = nullptr; w.Cout = W; w.ldc = npad; w.strideC = (long)Np * npad;
  w.M = Np; w.Ncols = npad; w.K = Np; w.kb = Np; w.kbeg_rt = BOCF_TILE; w.alpha = 1.0;
  launch_gemm_f64(w, mg, 0, c->stream);
}

// What staging a point set A (na points resident at Xdev, nap = na rounded up to 128) enqueues for all M outputs: V_A = R^T K(X, A), Wa = Ky^-1 K(X, A),
// mu(A) and (s2A != nullptr) the raw sigma^2(A).  Shared by bocf_set_ref_points and bocf_set_pending_points, each with buffers of its own.
int bocf_kg_stage(bocf_ctx* c, const double* Xdev, int na, int nap, double* VA, double* Wa, double* muA, double* s2A) {
  const int M = c->m, Np = c->Np;
  PhaseTimer t(c, "kg_ref");
  if (bocf_enqueue_V(c, 0, M, Xdev, na, nap, VA, muA)) return -1;
  kg_enqueue_W(c, 0, M, VA, nap, Wa);
  if (s2A) launch_kg_diag(VA, nap, (long)Np * nap, Np, na, c->hypd.as<KernHyp>(), s2A, nap, M, c->stream);
  return 0;
}

// V, Sigma(., A) and the raw sigma^2 of candidates [c0, c0 + cn) for the mg outputs from j0 into kg_V (Np x cnp), kg_cov (cnp x nap), kg_s2c (cnp),
// against the staged set `ref`; with_grad: also W = Ky^-1 k(X, x_c) and d mu / dx, d sigma^2 / dx into kg_dmean / kg_dvar (cnp x d);
// mu != nullptr: also the posterior mean of the candidates (mg x cnp)
int bocf_kg_chunk(bocf_ctx* c, const KgRefSet& ref, int j0, int mg, int c0, int cn, int cnp, bool with_grad, double* mu) {
  const int Np = c->Np, d = c->d, na = ref.na, nap = round_up(na, BOCF_TILE);
  const double* Xq = c->Xc.as<double>() + (size_t)c0 * d;
  const int* kids = BOCF_KIDS(c);
  if (c->kg_V.ensure(sizeof(double) * (size_t)mg * Np * cnp) || c->kg_cov.ensure(sizeof(double) * (size_t)mg * cnp * nap) ||
      c->kg_s2c.ensure(sizeof(double) * (size_t)mg * cnp))
    return -1;
  {
    PhaseTimer t(c, "kg_V");
    if (bocf_enqueue_V(c, j0, mg, Xq, cn, cnp, c->kg_V.as<double>(), mu)) return -1;
  }
  {
    PhaseTimer t(c, "kg_cov");
    launch_post_cov(c->kg_V.as<double>(), cnp, (long)Np * cnp, ref.VA->as<double>() + (size_t)j0 * Np * nap, nap, (long)Np * nap, Xq, cn, ref.XA->as<double>(),
                    na, d, Np, c->kernel_id, kids ? kids + j0 : nullptr, c->hypd.as<KernHyp>() + j0, nullptr, 0, c->kg_cov.as<double>(), nap,
                    (long)cnp * nap, mg, c->stream);
    launch_kg_diag(c->kg_V.as<double>(), cnp, (long)Np * cnp, Np, cn, c->hypd.as<KernHyp>() + j0, c->kg_s2c.as<double>(), cnp, mg, c->stream);
  }
  if (with_grad) {
    if (c->kg_W.ensure(sizeof(double) * (size_t)mg * Np * cnp) || c->kg_dmean.ensure(sizeof(double) * (size_t)mg * cnp * d) ||
        c->kg_dvar.ensure(sizeof(double) * (size_t)mg * cnp * d))
      return -1;
    PhaseTimer t(c, "kg_grad");
    kg_enqueue_W(c, j0, mg, c->kg_V.as<double>(), cnp, c->kg_W.as<double>());
    launch_grad_kernel(c->Xs.as<double>() + (long)j0 * c->xs_stride, c->xs_stride, c->N, Np, d, c->kernel_id, c->hypd.as<KernHyp>() + j0, Xq, 0, cn,
                       c->alpha.as<double>() + (long)j0 * Np, c->kg_W.as<double>(), cnp, (long)Np * cnp, c->kg_dmean.as<double>(), c->kg_dvar.as<double>(),
                       cnp, mg, c->stream, kids ? kids + j0 : nullptr);
  }
  return 0;
}

// d Sigma(x_c, a) / dx_c of the chunk's cn candidates against reference points [a0, a0 + an) into kg_dcov (mg, cn, an, d)
int bocf_kg_chunk_dcov(bocf_ctx* c, const KgRefSet& ref, int j0, int mg, int c0, int cn, int a0, int an) {
  const int Np = c->Np, d = c->d, nap = round_up(ref.na, BOCF_TILE);
  if (c->kg_dcov.ensure(sizeof(double) * (size_t)mg * cn * an * d)) return -1;
  const int* kids = BOCF_KIDS(c);
  PhaseTimer t(c, "kg_grad");
  launch_cov_grad(c->Xs.as<double>() + (long)j0 * c->xs_stride, c->xs_stride, c->N, d, c->kernel_id, kids ? kids + j0 : nullptr, c->hypd.as<KernHyp>() + j0,
                  c->Xc.as<double>() + (size_t)c0 * d, cn, ref.XA->as<double>(), a0, an, ref.Wa->as<double>() + (size_t)j0 * Np * nap, nap, (long)Np * nap,
                  c->kg_dcov.as<double>(), mg, c->stream);
  return 0;
}

extern "C" int bocf_set_ref_points(bocf_ctx* c, const double* Xa, int na) {
  static const char* who = "bocf_set_ref_points";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  if (!Xa) return fail(who, "null Xa");
  if (na < 1 || na > KG_MAX_REF) return fail(who, "na out of range (1 .. 1024)");
  if (c->d > BOCF_MAX_D) return fail(who, "input dimension too large");
  const int M = c->m, Np = c->Np, d = c->d, nap = round_up(na, BOCF_TILE);
  if (2.0 * M * (double)Np * nap * sizeof(double) > (double)c->workspace_mb * 1048576.0) return fail(who, kWorkspace);
  HIPCHK(hipSetDevice(c->device));
  c->kg_na = 0;                                              // (replaced below, or gone if this call fails)
  if (c->kg_XA.ensure(sizeof(double) * (size_t)na * d) || c->kg_VA.ensure(sizeof(double) * (size_t)M * Np * nap) ||
      c->kg_Wa.ensure(sizeof(double) * (size_t)M * Np * nap) || c->kg_muA.ensure(sizeof(double) * (size_t)M * nap) ||
      c->kg_s2A.ensure(sizeof(double) * (size_t)M * nap) || c->kg_nug.ensure(sizeof(double) * (size_t)M))
    return -1;
  std::vector<double> nug(M);
  for (int j = 0; j < M; ++j) nug[j] = c->hyp[j].noise + 1e-8 + (j < (int)c->jitter.size() ? c->jitter[j] : 0.0);
  HIPCHK(hipMemcpyAsync(c->kg_XA.p, Xa, sizeof(double) * (size_t)na * d, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->kg_nug.p, nug.data(), sizeof(double) * (size_t)M, hipMemcpyHostToDevice, c->stream));
  if (bocf_kg_stage(c, c->kg_XA.as<double>(), na, nap, c->kg_VA.as<double>(), c->kg_Wa.as<double>(), c->kg_muA.as<double>(), c->kg_s2A.as<double>())) return -1;
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  c->kg_na = na;
  return 0;
}

extern "C" int bocf_cov_to_ref(bocf_ctx* c, int group, double* cov_out, double* dcov_out) {
  static const char* who = "bocf_cov_to_ref";
  if (bocf_kg_ready(who, bocf_call_state(c))) return -1;
  if (!cov_out) return fail(who, "null cov_out");
  int j0, mg, per;
  if (bocf_group_range(who, bocf_call_state(c), group, &j0, &mg, &per)) return -1;
  const int C = c->C, d = c->d, na = c->kg_na, nap = round_up(na, BOCF_TILE);
  const int chunk = bocf_kg_chunk_size(c, mg);
  if (chunk < BOCF_TILE) return fail(who, kWorkspace);
  if (dcov_out && (double)mg * C * (double)na * d * sizeof(double) > (double)c->workspace_mb * 1048576.0) return fail(who, kWorkspace);
  HIPCHK(hipSetDevice(c->device));
  for (int c0 = 0; c0 < C; c0 += chunk) {
    const int cn = C - c0 < chunk ? C - c0 : chunk, cnp = round_up(cn, BOCF_TILE);
    if (bocf_kg_chunk(c, kg_ref(c), j0, mg, c0, cn, cnp, false, nullptr)) return -1;
    for (int j = 0; j < mg; ++j)
      HIPCHK(hipMemcpy2DAsync(cov_out + ((size_t)j * C + c0) * na, sizeof(double) * na, c->kg_cov.as<double>() + (size_t)j * cnp * nap, sizeof(double) * nap,
                              sizeof(double) * na, cn, hipMemcpyDeviceToHost, c->stream));
    if (dcov_out) {
      if (bocf_kg_chunk_dcov(c, kg_ref(c), j0, mg, c0, cn, 0, na)) return -1;
      for (int j = 0; j < mg; ++j)
        HIPCHK(hipMemcpyAsync(dcov_out + ((size_t)j * C + c0) * na * d, c->kg_dcov.as<double>() + (size_t)j * cn * na * d, sizeof(double) * (size_t)cn * na * d,
                              hipMemcpyDeviceToHost, c->stream));
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  return 0;
}

extern "C" int bocf_conditioned_variance(bocf_ctx* c, int group, int q, double* var_out, double* dvar_out) {
  static const char* who = "bocf_conditioned_variance";
  if (bocf_kg_ready(who, bocf_call_state(c))) return -1;
  if (!var_out) return fail(who, "null var_out");
  if (q < 0 || q >= c->kg_na) return fail(who, "q out of range (0 .. na - 1)");
  int j0, mg, per;
  if (bocf_group_range(who, bocf_call_state(c), group, &j0, &mg, &per)) return -1;
  const int C = c->C, d = c->d, nap = round_up(c->kg_na, BOCF_TILE);
  const int chunk = bocf_kg_chunk_size(c, mg);
  if (chunk < BOCF_TILE) return fail(who, kWorkspace);
  HIPCHK(hipSetDevice(c->device));
  const bool grad = dvar_out != nullptr;
  for (int c0 = 0; c0 < C; c0 += chunk) {
    const int cn = C - c0 < chunk ? C - c0 : chunk, cnp = round_up(cn, BOCF_TILE);
    if (bocf_kg_chunk(c, kg_ref(c), j0, mg, c0, cn, cnp, grad, nullptr)) return -1;
    if (grad && bocf_kg_chunk_dcov(c, kg_ref(c), j0, mg, c0, cn, q, 1)) return -1;
    if (c->kg_out.ensure(sizeof(double) * (size_t)mg * cn) || (grad && c->kg_dout.ensure(sizeof(double) * (size_t)mg * cn * d))) return -1;
    launch_cond_var(c->kg_cov.as<double>(), nap, (long)cnp * nap, q, c->kg_s2c.as<double>(), cnp, c->kg_s2A.as<double>() + (size_t)j0 * nap, nap,
                    c->kg_nug.as<double>() + j0, grad ? c->kg_dvar.as<double>() : nullptr, cnp, grad ? c->kg_dcov.as<double>() : nullptr, cn, d,
                    c->kg_out.as<double>(), grad ? c->kg_dout.as<double>() : nullptr, mg, c->stream);
    for (int j = 0; j < mg; ++j) {
      HIPCHK(hipMemcpyAsync(var_out + (size_t)j * C + c0, c->kg_out.as<double>() + (size_t)j * cn, sizeof(double) * cn, hipMemcpyDeviceToHost, c->stream));
      if (grad)
        HIPCHK(hipMemcpyAsync(dvar_out + ((size_t)j * C + c0) * d, c->kg_dout.as<double>() + (size_t)j * cn * d, sizeof(double) * (size_t)cn * d,
                              hipMemcpyDeviceToHost, c->stream));
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  return 0;
}

extern "C" int bocf_acq_kg(bocf_ctx* c, int mode, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim,
                           const double* prob, int L, const double* Zf, int Sf, double* acq_out, double* dacq_out) {
  static const char* who = "bocf_acq_kg";
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, prob, L};
  const int m = bocf_kg_check(who, bocf_call_state(c), mode, u, Zf, Sf);
  if (m < 0) return -1;
  const int Ha = bocf_acq_hyper_count(c);                   // the convention of the other acquisitions
  const int mg = Ha * m;
  const int C = c->C, d = c->d, na = c->kg_na, nap = round_up(na, BOCF_TILE);
  const bool grad = dacq_out != nullptr;
  int chunk = bocf_kg_chunk_size(c, mg);
  if (chunk < BOCF_TILE) return fail(who, kWorkspace);
  if (grad) {
    // one chunk: d Sigma / dx of every (candidate, reference point) is held at once (the optimiser's small batches)
    if ((double)mg * C * (double)na * d * sizeof(double) > (double)c->workspace_mb * 1048576.0 || round_up(C, BOCF_TILE) > chunk) return fail(who, kWorkspace);
  }
  HIPCHK(hipSetDevice(c->device));
  // theta | prob | utility parameters | Zf in one upload
  const UtilPack& pk = bocf_util_pack(u, Zf, (size_t)Sf * m, &c->util_up);
  if (c->kg_v0.ensure(sizeof(double) * (size_t)Ha * L) || c->acq.ensure(sizeof(double) * (size_t)round_up(C, BOCF_TILE))) return -1;
  if (grad && (c->kg_dout.ensure(sizeof(double) * (size_t)C * d) || c->kg_astar.ensure(sizeof(int) * (size_t)C * L * Sf) ||
               c->kg_AB.ensure(sizeof(double) * (size_t)C * L * Sf * 2 * m)))
    return -1;
  c->have_acq = false;
  if (bocf_upload_util(c, pk, &c->kg_par)) return -1;
  KgArgs a{};
  a.ldc = nap; a.lda = nap; a.nug = c->kg_nug.as<double>();
  a.theta = c->kg_par.as<double>() + pk.theta; a.theta_dim = theta_dim; a.prob = c->kg_par.as<double>() + pk.prob; a.L = L;
  a.util_params = c->kg_par.as<double>() + pk.params; a.Zf = c->kg_par.as<double>() + pk.tail; a.Sf = Sf;
  a.Wt = mode == BOCF_EU_MC ? c->Wt.as<double>() : nullptr; a.S = mode == BOCF_EU_MC ? c->S_mc : 0;
  a.m = m; a.na = na; a.mode = mode; a.util_kind = util_kind; a.scale = 1.0 / Ha;
  for (int h = 0; h < Ha; ++h) {
    KgArgs v = a;
    v.muA = c->kg_muA.as<double>() + (size_t)h * m * nap; v.s2A = c->kg_s2A.as<double>() + (size_t)h * m * nap;
    PhaseTimer t(c, "kg_kernel");
    launch_kg_v0(v, c->kg_v0.as<double>() + (size_t)h * L, c->stream);
  }
  for (int c0 = 0; c0 < C; c0 += chunk) {
    const int cn = C - c0 < chunk ? C - c0 : chunk, cnp = round_up(cn, BOCF_TILE);
    if (bocf_kg_chunk(c, kg_ref(c), 0, mg, c0, cn, cnp, grad, nullptr)) return -1;
    if (grad && bocf_kg_chunk_dcov(c, kg_ref(c), 0, mg, c0, cn, 0, na)) return -1;
    for (int h = 0; h < Ha; ++h) {
      KgArgs k = a;
      k.cov = c->kg_cov.as<double>() + (size_t)h * m * cnp * nap; k.strideC = (long)cnp * nap;
      k.s2c = c->kg_s2c.as<double>() + (size_t)h * m * cnp; k.lds = cnp;
      k.nug = a.nug + (size_t)h * m;
      k.muA = c->kg_muA.as<double>() + (size_t)h * m * nap; k.s2A = c->kg_s2A.as<double>() + (size_t)h * m * nap;
      k.v0 = c->kg_v0.as<double>() + (size_t)h * L;
      k.C = cn; k.acq = c->acq.as<double>() + c0; k.accumulate = h > 0;
      if (grad) { k.astar = c->kg_astar.as<int>(); k.AB = c->kg_AB.as<double>(); }
      {
        PhaseTimer t(c, "kg_kernel");
        launch_kg(k, c->stream);
        if (grad) launch_kg_partials(k, c->stream);
      }
      if (grad) {
        KgGradArgs g{};
        g.cov = k.cov; g.ldc = nap; g.strideC = k.strideC;
        g.dcov = c->kg_dcov.as<double>() + (size_t)h * m * cn * na * d;
        g.s2c = k.s2c; g.lds = cnp; g.ds2c = c->kg_dvar.as<double>() + (size_t)h * m * cnp * d; g.ldg = cnp;
        g.nug = k.nug; g.Zf = a.Zf; g.Sf = Sf; g.prob = a.prob; g.L = L; g.m = m; g.na = na; g.C = cn; g.d = d;
        g.astar = k.astar; g.AB = k.AB; g.dacq = c->kg_dout.as<double>(); g.accumulate = h > 0; g.scale = a.scale;
        PhaseTimer t(c, "kg_grad");
        launch_kg_grad(g, c->stream);
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
