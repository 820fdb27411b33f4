// Pathwise posterior samples, the entry points of the C ABI (include/bocf_hip.h): bocf_set_paths, bocf_path_values, bocf_path_utility.
// The kernels are paths.hip.  Staging solves Ky v = rhs for S right-hand sides per output with the fit's R = U^-1 through the fp64 GEMM,
// exactly as bocf_kg_stage forms Wa (V = R^T rhs, v = R V): a plain fp64 solve, no double-double refinement.  Local to one context, like
// the joint-posterior entry points; one stream, one synchronisation per call.
#include "bocf_ctx.h"

#include <cstring>
#include <vector>

#define PATHS_MAX_S 64
#define PATHS_MAX_F 16384
#define PATHS_LDV BOCF_TILE     // row length of rhs / v: the GEMM's column tile (S <= 64 of it used)

void bocf_paths_drop(bocf_ctx* c) {
  for (int& s : c->pt_S) s = 0;
}

static const char* kNoPaths = "no paths are resident (bocf_set_paths after the fit; a fit, an appended observation and new targets drop them)";

// doubles of hyper-sample h's block and the offsets of its parts (each part starts on a 128-byte boundary: v is a GEMM output)
struct PathBlock {
  size_t omega, phase, w, v, total;
  static size_t up(size_t n) { return (n + 15) / 16 * 16; }
  PathBlock(int per, int F, int S, int d, int Np) {
    omega = 0;
    phase = up(omega + (size_t)per * F * d);
    w = up(phase + (size_t)per * F);
    v = up(w + (size_t)per * F * S);
    total = v + (size_t)per * Np * PATHS_LDV;
  }
};

extern "C" int bocf_set_paths(bocf_ctx* c, int group, const double* omega, const double* phase, const double* weights, const double* eps, int F, int S) {
  static const char* who = "bocf_set_paths";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  int j0, mg, per;
  if (bocf_group_range(who, bocf_call_state(c), group, &j0, &mg, &per)) return -1;
  const int H = c->m / per, h0 = group < 0 ? 0 : group, h1 = group < 0 ? H : group + 1;
  if (S == 0) {                                              // drop the group's paths
    if ((int)c->pt_S.size() == H)
      for (int h = h0; h < h1; ++h) c->pt_S[h] = 0;
    else bocf_paths_drop(c);
    return 0;
  }
  if (S < 1 || S > PATHS_MAX_S) return fail(who, "S out of range (0 .. 64)");
  if (F < 1 || F > PATHS_MAX_F) return fail(who, "F out of range (1 .. 16384)");
  if (!omega || !phase || !weights || !eps) return fail(who, "null argument");
  if (c->d > BOCF_MAX_D) return fail(who, "input dimension too large");
  const int N = c->N, Np = c->Np, d = c->d;
  HIPCHK(hipSetDevice(c->device));
  if ((int)c->pt_S.size() != H) {                            // (another hyper-sample count than the last call's)
    for (DevBuf& b : c->pt_buf) b.release();
    c->pt_S.assign(H, 0);
    c->pt_F.assign(H, 0);
    c->pt_buf.assign(H, DevBuf{});
  }
  for (int h = h0; h < h1; ++h) c->pt_S[h] = 0;              // (replaced below, or gone if this call fails)
  const PathBlock blk(per, F, S, d, Np);
  for (int h = h0; h < h1; ++h)
    if (c->pt_buf[h].ensure(sizeof(double) * blk.total)) return -1;
  const size_t nE = (size_t)mg * N * S, nR = (size_t)mg * Np * PATHS_LDV;
  if (c->pt_E.ensure(sizeof(double) * nE) || c->pt_g.ensure(sizeof(double) * nE) || c->pt_rhs.ensure(sizeof(double) * nR) ||
      c->pt_tmp.ensure(sizeof(double) * nR) || c->pt_nug.ensure(sizeof(double) * (size_t)mg))
    return -1;
  std::vector<double> nug(mg);
  for (int j = 0; j < mg; ++j) nug[j] = c->hyp[j0 + j].noise + 1e-8 + (j0 + j < (int)c->jitter.size() ? c->jitter[j0 + j] : 0.0);
  for (int h = h0; h < h1; ++h) {
    double* b = c->pt_buf[h].as<double>();
    const size_t jl = (size_t)(h - h0) * per;
    HIPCHK(hipMemcpyAsync(b + blk.omega, omega + jl * F * d, sizeof(double) * (size_t)per * F * d, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + blk.phase, phase + jl * F, sizeof(double) * (size_t)per * F, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b + blk.w, weights + jl * F * S, sizeof(double) * (size_t)per * F * S, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemcpyAsync(c->pt_E.p, eps, sizeof(double) * nE, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->pt_nug.p, nug.data(), sizeof(double) * (size_t)mg, hipMemcpyHostToDevice, c->stream));
  const int* kids = BOCF_KIDS(c);
  const long strideS = (long)Np * Np, strideV = (long)Np * PATHS_LDV;
  {
    PhaseTimer t(c, "paths_stage");
    // 1. g(X): the feature part of the value kernel at the training inputs (already divided by the lengthscales: Xs)
    for (int h = h0; h < h1; ++h) {
      const int jh = h * per;
      const double* b = c->pt_buf[h].as<double>();
      PathValArgs a{};
      a.Xs = c->Xs.as<double>() + (long)jh * c->xs_stride; a.strideXs = c->xs_stride; a.N = 0;
      a.omega = b + blk.omega; a.phase = b + blk.phase; a.w = b + blk.w; a.F = F; a.S = S;
      a.hyp = c->hypd.as<KernHyp>() + jh;
      a.Xc = c->Xs.as<double>() + (long)jh * c->xs_stride; a.strideXc = c->xs_stride; a.prescaled = 1; a.C = N;
      a.out = c->pt_g.as<double>() + (size_t)(jh - j0) * N * S; a.strideOut = (long)N * S; a.add_mean = 0;
      launch_path_values(a, d, c->kernel_id, kids ? kids + jh : nullptr, per, c->stream);
    }
    // 2. rhs = yc - g(X) - sqrt(nug) E
    launch_path_rhs(c->yc.as<double>() + (long)j0 * Np, c->pt_g.as<double>(), c->pt_E.as<double>(), c->pt_nug.as<double>(), N, Np, S, PATHS_LDV,
                    c->pt_rhs.as<double>(), mg, c->stream);
    // 3. V = R^T rhs, then v = R V (bocf_enqueue_V's and kg_enqueue_W's GEMMs)
    GemmArgs v{};
    v.A = c->R.as<double>() + (long)j0 * strideS; v.lda = Np; v.strideA = strideS;
    v.B = c->pt_rhs.as<double>(); v.ldb = PATHS_LDV; v.strideB = strideV;
    v.Cin = nullptr; v.Cout = c->pt_tmp.as<double>(); v.ldc = PATHS_LDV; v.strideC = strideV;
    v.M = Np; v.Ncols = PATHS_LDV; v.K = Np; v.kb = BOCF_TILE; v.krt = BOCF_TILE; v.rt_desc = 1; v.alpha = 1.0;
    launch_gemm_f64(v, mg, 0, c->stream);
    for (int h = h0; h < h1; ++h) {
      const int jh = h * per;
      GemmArgs w{};
      w.A = c->RT.as<double>() + (long)jh * strideS; w.lda = Np; w.strideA = strideS;
      w.B = c->pt_tmp.as<double>() + (long)(jh - j0) * strideV; w.ldb = PATHS_LDV; w.strideB = strideV;
      w.Cin = nullptr; w.Cout = c->pt_buf[h].as<double>() + blk.v; w.ldc = PATHS_LDV; w.strideC = strideV;
      w.M = Np; w.Ncols = PATHS_LDV; w.K = Np; w.kb = Np; w.kbeg_rt = BOCF_TILE; w.alpha = 1.0;
      launch_gemm_f64(w, per, 0, c->stream);
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  for (int h = h0; h < h1; ++h) {
    c->pt_S[h] = S;
    c->pt_F[h] = F;
  }
  return 0;
}

extern "C" int bocf_path_values(bocf_ctx* c, int group, double* values_out) {
  static const char* who = "bocf_path_values";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  int j0, mg, per;
  if (bocf_group_range(who, bocf_call_state(c), group, &j0, &mg, &per)) return -1;
  const int H = c->m / per, h0 = group < 0 ? 0 : group, h1 = group < 0 ? H : group + 1;
  if ((int)c->pt_S.size() != H) return fail(who, kNoPaths);
  for (int h = h0; h < h1; ++h)
    if (c->pt_S[h] < 1) return fail(who, kNoPaths);
  const int C = c->C;
  if (C < 1) return fail(who, "no resident candidates (bocf_set_candidates)");
  const int N = c->N, Np = c->Np, d = c->d;
  HIPCHK(hipSetDevice(c->device));
  if ((int)c->ts_S.size() != H) {
    for (DevBuf& b : c->ts_F) b.release();
    c->ts_S.assign(H, 0);
    c->ts_F.assign(H, DevBuf{});
  }
  for (int h = h0; h < h1; ++h) c->ts_S[h] = 0;              // (replaced below, or gone if this call fails)
  for (int h = h0; h < h1; ++h)
    if (c->ts_F[h].ensure(sizeof(double) * (size_t)per * C * c->pt_S[h])) return -1;
  const int* kids = BOCF_KIDS(c);
  {
    PhaseTimer t(c, "path_values");
    for (int h = h0; h < h1; ++h) {
      const int jh = h * per, S = c->pt_S[h], F = c->pt_F[h];
      const PathBlock blk(per, F, S, d, Np);
      const double* b = c->pt_buf[h].as<double>();
      PathValArgs a{};
      a.Xs = c->Xs.as<double>() + (long)jh * c->xs_stride; a.strideXs = c->xs_stride; a.N = N;
      a.v = b + blk.v; a.ldv = PATHS_LDV; a.strideV = (long)Np * PATHS_LDV;
      a.omega = b + blk.omega; a.phase = b + blk.phase; a.w = b + blk.w; a.F = F; a.S = S;
      a.hyp = c->hypd.as<KernHyp>() + jh;
      a.Xc = c->Xc.as<double>(); a.strideXc = 0; a.prescaled = 0; a.C = C;
      a.out = c->ts_F[h].as<double>(); a.strideOut = (long)C * S; a.add_mean = 1;
      launch_path_values(a, d, c->kernel_id, kids ? kids + jh : nullptr, per, c->stream);
    }
  }
  if (values_out) {
    size_t off = 0;
    for (int h = h0; h < h1; ++h) {
      const size_t n = (size_t)per * C * c->pt_S[h];
      HIPCHK(hipMemcpyAsync(values_out + off, c->ts_F[h].p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
      off += n;
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  for (int h = h0; h < h1; ++h) c->ts_S[h] = c->pt_S[h];
  return 0;
}

extern "C" int bocf_path_utility(bocf_ctx* c, int util_kind, const double* util_params, int n_util_params, const double* theta, int theta_dim, int P,
                                 const int* row_path, double* val_out, double* grad_out) {
  static const char* who = "bocf_path_utility";
  if (bocf_check_posterior(who, bocf_call_state(c))) return -1;
  int j0, mg, per;
  if (bocf_group_range(who, bocf_call_state(c), -1, &j0, &mg, &per)) return -1;
  const int H = c->m / per;
  int Pres = 0;
  if ((int)c->pt_S.size() == H)
    for (int s : c->pt_S) Pres += s;
  if (Pres == 0) return fail(who, kNoPaths);
  if (P != Pres) return fail(who, "P does not match the resident paths (the sum over the hyper-samples of the S of bocf_set_paths)");
  const int C = c->C, d = c->d, N = c->N, Np = c->Np;
  if (C < 1) return fail(who, "no resident candidates (bocf_set_candidates)");
  if (!row_path || !val_out || (theta_dim > 0 && !theta) || theta_dim < 0) return fail(who, "null argument / bad theta_dim");
  for (int r = 0; r < C; ++r)
    if (row_path[r] < 0 || row_path[r] >= P) return fail(who, "row_path out of range (0 .. P - 1)");
  if (util_kind < BOCF_UTIL_LINEAR || util_kind > BOCF_UTIL_PROGRAM) return fail(who, "unknown utility kind");
  if (n_util_params < 0 || n_util_params > BOCF_MAX_M || (n_util_params > 0 && !util_params)) return fail(who, "too many utility parameters / null");
  if (bocf_check_group_fits(who, per)) return -1;
  if (util_kind == BOCF_UTIL_PROGRAM && bocf_check_resident_program(c, who, per, theta_dim, n_util_params)) return -1;
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> par;                                   // the widened theta rows | the parameters (util_args.h)
  const int tw = bocf_util_pack_rows(theta, theta_dim, P, per, util_params, n_util_params, &par);
  const int* kids = BOCF_KIDS(c);
  std::vector<int> rows((size_t)C + c->m, 0);
  memcpy(rows.data(), row_path, sizeof(int) * (size_t)C);
  for (int j = 0; j < c->m; ++j) rows[(size_t)C + j] = kids ? kids[j] : c->kernel_id;
  std::vector<PathHyper> tab;
  for (int h = 0, p0 = 0; h < H; ++h) {
    if (c->pt_S[h] == 0) continue;
    const PathBlock blk(per, c->pt_F[h], c->pt_S[h], d, Np);
    const double* b = c->pt_buf[h].as<double>();
    tab.push_back(PathHyper{b + blk.omega, b + blk.phase, b + blk.w, b + blk.v, c->pt_F[h], c->pt_S[h], p0, h});
    p0 += c->pt_S[h];
  }
  if (c->pt_par.ensure(sizeof(double) * par.size()) || c->pt_rows.ensure(sizeof(int) * rows.size()) || c->pt_tab.ensure(sizeof(PathHyper) * tab.size()) ||
      c->pt_pv.ensure(sizeof(double) * (size_t)C * per) || c->pt_pg.ensure(sizeof(double) * (size_t)C * per * d) ||
      c->pt_val.ensure(sizeof(double) * (size_t)C) || c->pt_grad.ensure(sizeof(double) * (size_t)C * d))
    return -1;
  HIPCHK(hipMemcpyAsync(c->pt_par.p, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->pt_rows.p, rows.data(), sizeof(int) * rows.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->pt_tab.p, tab.data(), sizeof(PathHyper) * tab.size(), hipMemcpyHostToDevice, c->stream));
  {
    PhaseTimer t(c, "path_utility");
    PathPointArgs a{};
    a.Xs = c->Xs.as<double>(); a.strideXs = c->xs_stride; a.N = N; a.Np = Np;
    a.hyp = c->hypd.as<KernHyp>(); a.kids = c->pt_rows.as<int>() + C; a.kernel_id = c->kernel_id;
    a.tab = c->pt_tab.as<PathHyper>(); a.nh = (int)tab.size();
    a.per = per; a.ldv = PATHS_LDV;
    a.Xc = c->Xc.as<double>(); a.row_path = c->pt_rows.as<int>();
    a.pv = c->pt_pv.as<double>(); a.pg = c->pt_pg.as<double>();
    launch_path_point(a, d, C, c->stream);
    launch_path_chain(a.pv, a.pg, per, d, C, a.row_path, util_kind, c->pt_par.as<double>(), tw, c->pt_par.as<double>() + (size_t)P * tw,
                      c->pt_val.as<double>(), grad_out ? c->pt_grad.as<double>() : nullptr, c->stream, &c->prog);
  }
  HIPCHK(hipMemcpyAsync(val_out, c->pt_val.p, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, c->stream));
  if (grad_out) HIPCHK(hipMemcpyAsync(grad_out, c->pt_grad.p, sizeof(double) * (size_t)C * d, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  return 0;
}
