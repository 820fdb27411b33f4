// Factorization schedules of libbocf_hip.so: the blocked Cholesky of all outputs -- resident workgroup teams (one launch, 2..8 panels;
// chol_team.hip), single stream with panel aggregation, reserved-CU chain with device-side counters -- and the triangular inverse by
// recursive doubling, early part underneath the factorization.  Called by bocf_fit (capi_fit.hip) through bocf_run_cholesky / bocf_run_trtri.
#include "bocf_ctx.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// (accessors of the factorization's buffers: one place for the casts)
static inline int wm(bocf_ctx* c) { return c->m; }
static inline double* wS(bocf_ctx* c) { return c->S.as<double>(); }
static inline double* wR(bocf_ctx* c) { return c->R.as<double>(); }
static inline double* wRT(bocf_ctx* c) { return c->RT.as<double>(); }
static inline double* wT(bocf_ctx* c) { return c->T.as<double>(); }
static inline double* wE(bocf_ctx* c) { return c->E.as<double>(); }
static inline double* wET(bocf_ctx* c) { return c->ET.as<double>(); }
static inline int* winfo(bocf_ctx* c) { return c->info.as<int>(); }

// ---------------------------------------------------------------------------------------------
// Cholesky (upper form, right-looking, NB = 128) of all m outputs at once.
//
// Per panel p the chain  diagonal block (one workgroup per output, ~41 us) -> row solve (one tile row) -> trailing
// update  is a dependency chain of short, latency-bound launches.  Schedules (option "lookahead"): 0 = everything on one stream, G panels
// per trailing update (option "aggregate"); 2 = the chain on reserved compute units with device-side counters (run_cholesky_reserved,
// one output, or two up to 12 panels).  (Round 3 built and measured three more -- a persistent chain on reserved CUs, output groups staggered
// on streams of their own, the next pair's diagonal block underneath the trailing update: slower, a tie, a tie -- and removed them again:
// DESIGN.md 10, profiles/r03.)
static GemmArgs trsm_args(bocf_ctx* c, int p, int W) {
  const int Np = c->Np;
  const long strideS = (long)Np * Np, strideE = (long)(Np / BOCF_TILE) * BOCF_TILE * BOCF_TILE;
  double* panel = wS(c) + (long)p * BOCF_TILE * Np + (long)(p + 1) * BOCF_TILE;
  GemmArgs g{};
  // U_p,> = E_p^T A_p,>   (in place)
  g.A = wE(c) + (long)p * BOCF_TILE * BOCF_TILE; g.lda = BOCF_TILE; g.strideA = strideE;
  g.B = panel; g.ldb = Np; g.strideB = strideS;
  g.Cin = nullptr; g.Cout = panel; g.ldc = Np; g.strideC = strideS;
  g.M = BOCF_TILE; g.Ncols = W; g.K = BOCF_TILE; g.kb = BOCF_TILE; g.alpha = 1.0; g.beta = 0.0;
  return g;
}

// the row solve of panel p over W columns: wave-level single-tile kernel (K = 128: latency, not throughput, decides) unless the
// option says otherwise
static void launch_trsm(bocf_ctx* c, int p, int W, hipStream_t st) {
  if (W <= 0) return;
  if (c->chol.trsm_wave) {
    const int Np = c->Np;
    const long strideS = (long)Np * Np, strideE = (long)(Np / BOCF_TILE) * BOCF_TILE * BOCF_TILE;
    double* panel = wS(c) + (long)p * BOCF_TILE * Np + (long)(p + 1) * BOCF_TILE;
    launch_tile128(wE(c) + (long)p * BOCF_TILE * BOCF_TILE, BOCF_TILE, strideE, panel, Np, strideS, panel, Np, strideS, 1.0, 0.0, wm(c), st,
                   W / BOCF_TILE);
  } else {
    launch_gemm_f64(trsm_args(c, p, W), wm(c), 0, st);
  }
}

// A_>,> -= U_p,>^T U_p,> restricted to block rows [first, first + rows) of the trailing matrix (tiles on/above the diagonal)
static GemmArgs syrk_args(bocf_ctx* c, int p, int first, int rows, int W) {
  const int Np = c->Np;
  const long strideS = (long)Np * Np;
  double* panel = wS(c) + (long)p * BOCF_TILE * Np + (long)(p + 1) * BOCF_TILE;
  const long off = (long)first * BOCF_TILE;
  GemmArgs t{};
  t.A = panel + off; t.lda = Np; t.strideA = strideS;
  t.B = panel + off; t.ldb = Np; t.strideB = strideS;
  double* trail = wS(c) + ((long)(p + 1) * BOCF_TILE + off) * Np + (long)(p + 1) * BOCF_TILE + off;
  t.Cin = trail; t.Cout = trail; t.ldc = Np; t.strideC = strideS;
  t.M = rows * BOCF_TILE; t.Ncols = W - (int)off; t.K = BOCF_TILE; t.kb = BOCF_TILE; t.upper_only = 1; t.alpha = -1.0; t.beta = 1.0;
  return t;
}

// (Re)create the three masked streams for `want` of `ncu` compute units reserved.  Mask bit i selects CU (i / 8) of XCD (i % 8) on
// MI355X (tools/cumask_probe.hip), so 8 k reserved bits take k CUs from every XCD.
// Returns 0 = streams ready; 1 = the runtime refuses CU masks (cu_masks_ok is cleared); -1 = a HIP error (recorded).
static int ensure_reserved_streams(bocf_ctx* c, int want, int ncu) {
  if (c->res_cus == want && c->s_res) return 0;
  for (hipStream_t* st : {&c->s_res, &c->s_hi, &c->s_bulk})
    if (*st) {
      (void)hipStreamDestroy(*st);
      *st = nullptr;
    }
  c->res_cus = 0;
  const int words = (ncu + 31) / 32;
  std::vector<uint32_t> res(words, 0u), rest(words, 0u);
  for (int i = 0; i < ncu; ++i) (i < want ? res : rest)[i / 32] |= 1u << (i % 32);
  int lo_prio = 0, hi_prio = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
  hipError_t e = hipExtStreamCreateWithCUMask(&c->s_res, (uint32_t)words, res.data());
  if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&c->s_hi, (uint32_t)words, rest.data());
  if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&c->s_bulk, (uint32_t)words, rest.data());
  if (e != hipSuccess) {
    (void)hipGetLastError();
    for (hipStream_t* st : {&c->s_res, &c->s_hi, &c->s_bulk})
      if (*st) {
        (void)hipStreamDestroy(*st);
        *st = nullptr;
      }
    c->cu_masks_ok = 0;      // this runtime / box refuses CU masks: keep to the single-stream schedules
    return 1;
  }
  c->res_cus = want;
  return 0;
}

static void trtri_early(bocf_ctx* c, int h, hipStream_t st);
enum { MERGE_FIRST = 1, MERGE_SECOND = 2 };
static void merge_level(bocf_ctx* c, int lo, int w, int w2, int count, int which, hipStream_t st);

// Right-looking blocked Cholesky whose serial chain runs alone on reserved compute units, with DEVICE-SIDE dependencies
// between its three streams (counters in memory, fit.hip: dep_signal / gate_kernel; stream events cost 10-25 us each here):
//
//   s_res  (reserved CUs)   potrf(p)  T1(p) S1(p)  potrf(p+1)  T1(p+1) S1(p+1)  potrf(p+2) ...
//   s_hi   (other CUs)              T2(p)   S2(p)          T2(p+1)   S2(p+1) ...
//   s_bulk (other CUs)                  bulkA(p) bulkB(p) ......... bulkA(p+1) bulkB(p+1) ...
//
//   potrf(p)  diagonal block p -> U_pp, E_p = U_pp^-1                    (one workgroup per output)        signals P(p)
//   T1(p)     U[p][p+1] = E_p^T A[p][p+1]                                 (ONE tile per output)             signals T1(p)
//   S1(p)     A[p+1][p+1] -= U[p][p+1]^T U[p][p+1]                        (all the next potrf needs)
//   T2(p)     U[p][c] = E_p^T A[p][c], c >= p+2                           (the rest of the row solve)       signals T2(p)
//   S2(p)     A[p+1][c] -= U[p][p+1]^T U[p][c], c >= p+2                  (the rest of block row p+1)       signals R(p)
//   bulkA(p)  block row p+2 of panel p's trailing update                  (then signal_kernel)             signals BA(p)
//   bulkB(p)  the rows below it
//
// Every tile receives its updates from different panels in whatever order the streams reach them (sums commute); what is
// enforced is mutual exclusion on a tile and completion before a tile is consumed -- by a gate in front of the consumer:
//   T1(p), S1(p): gate R(p-1), BA(p-1)      T2(p): gate P(p)      S2(p): gate T1(p), BA(p-1)      bulkA(p): gate T2(p)
// (bulkA(p-1) follows every older bulk on its in-order stream, so BA(p-1) stands for all of them.)  The chain per panel is
// potrf + two single-tile products + three kernel boundaries on CUs nobody else may use; a trailing update has two chain
// steps to finish before anything waits for it.
static int run_cholesky_reserved(bocf_ctx* c, const CholPlan& plan) {
  const int Np = c->Np, m = c->m, nb = Np / BOCF_TILE;
  const long strideS = (long)Np * Np, strideE = (long)nb * BOCF_TILE * BOCF_TILE;
  double* S = wS(c);
  while ((int)c->ev_chol.size() < 4) {
    hipEvent_t ev;
    HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    c->ev_chol.push_back(ev);
  }
  const auto t_host0 = std::chrono::steady_clock::now();
  // counters: 5 per panel + the timeout word (plan.flag_ints, zeroed by run_cholesky_impl)
  int* F = c->chol_flags.as<int>();
  auto fP = [&](int p) { return F + 5 * p; };
  auto fT1 = [&](int p) { return F + 5 * p + 1; };
  auto fT2 = [&](int p) { return F + 5 * p + 2; };
  auto fR = [&](int p) { return F + 5 * p + 3; };
  auto fBA = [&](int p) { return F + 5 * p + 4; };
  int* ferr = F + plan.err_off;
  hipEvent_t ev0 = c->ev_chol[0], evE1 = c->ev_chol[1], evE2 = c->ev_chol[2], evE3 = c->ev_chol[3];
  HIPCHK(hipEventRecord(ev0, c->stream));
  for (hipStream_t st : {c->s_res, c->s_hi, c->s_bulk}) HIPCHK(hipStreamWaitEvent(st, ev0, 0));
  launch_potrf_diag(S, strideS, c->N, Np, 0, wE(c), wET(c), strideE, winfo(c), m, c->s_res, fP(0));
  for (int p = 0; p + 1 < nb; ++p) {
    const int W = Np - (p + 1) * BOCF_TILE;                // trailing width after panel p (>= 128)
    const int nrest = W / BOCF_TILE - 1;                   // tiles right of column block p+1
    double* panel = S + (long)p * BOCF_TILE * Np + (long)(p + 1) * BOCF_TILE;              // U[p][p+1 ...]
    double* trail = S + (long)(p + 1) * BOCF_TILE * Np + (long)(p + 1) * BOCF_TILE;        // A[p+1][p+1 ...]
    const double* Ep = wE(c) + (long)p * BOCF_TILE * BOCF_TILE;
    const int prev_rest = nrest + 1;                       // nrest of panel p-1
    // ---- chain: T1(p), S1(p), potrf(p+1)
    if (p > 0) launch_gate(fR(p - 1), 4 * prev_rest * m, fBA(p - 1), prev_rest * m, ferr, c->s_res);
    launch_tile128(Ep, BOCF_TILE, strideE, panel, Np, strideS, panel, Np, strideS, 1.0, 0.0, m, c->s_res, 1, BOCF_TILE, fT1(p));     // T1(p)
    launch_tile128(panel, Np, strideS, panel, Np, strideS, trail, Np, strideS, -1.0, 1.0, m, c->s_res, 1, BOCF_TILE, nullptr);      // S1(p)
    launch_potrf_diag(S, strideS, c->N, Np, p + 1, wE(c), wET(c), strideE, winfo(c), m, c->s_res, fP(p + 1));
    if (nrest <= 0) continue;                              // last panel pair: nothing right of column block p+1
    // ---- row work: T2(p), S2(p)
    launch_gate(fP(p), m, nullptr, 0, ferr, c->s_hi);
    launch_tile128(Ep, BOCF_TILE, strideE, panel + BOCF_TILE, Np, strideS, panel + BOCF_TILE, Np, strideS, 1.0, 0.0, m, c->s_hi, nrest, BOCF_TILE,
                   fT2(p));                                                                                                          // T2(p)
    launch_gate(fT1(p), 4 * m, p > 0 ? fBA(p - 1) : nullptr, prev_rest * m, ferr, c->s_hi);
    launch_tile128(panel, Np, strideS, panel + BOCF_TILE, Np, strideS, trail + BOCF_TILE, Np, strideS, -1.0, 1.0, m, c->s_hi, nrest, BOCF_TILE,
                   fR(p));                                                                                                           // S2(p)
    // ---- the part of the inverse that needs only block rows [0, h) of U starts as soon as row h-1 is solved, on its own stream
    //      (complement CUs): from here on the chain sets the pace and the chip is mostly idle
    if (p == plan.inv_after) {
      HIPCHK(hipStreamWaitEvent(c->s_inv, ev0, 0));
      launch_gate(fT2(p), 4 * nrest * m, fT1(p), 4 * m, ferr, c->s_inv);
      trtri_early(c, plan.h, c->s_inv);
      HIPCHK(hipEventRecord(c->ev_inv_early, c->s_inv));
      c->early_inverse_started = 1;
    }
    // ---- trailing update below block row p+1
    launch_gate(fT2(p), 4 * nrest * m, nullptr, 0, ferr, c->s_bulk);
    launch_gemm_f64(syrk_args(c, p, 1, 1, W), m, 0, c->s_bulk);                                   // bulkA(p): block row p+2
    launch_signal(fBA(p), nrest * m, c->s_bulk);           // (the GEMM kernel is not instrumented: the kernel boundary is its release)
    if (nrest - 1 > 0) launch_gemm_f64(syrk_args(c, p, 2, nrest - 1, W), m, 0, c->s_bulk);        // bulkB(p)
  }
  HIPCHK(hipEventRecord(evE1, c->s_res));
  HIPCHK(hipEventRecord(evE2, c->s_hi));
  HIPCHK(hipEventRecord(evE3, c->s_bulk));
  for (hipEvent_t ev : {evE1, evE2, evE3}) HIPCHK(hipStreamWaitEvent(c->stream, ev, 0));
#ifdef BOCF_PROBES
  if (getenv("BOCF_DBG")) {
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "run_cholesky_reserved: host enqueue %.1f us for %d panels\n", std::chrono::duration<double, std::micro>(t1 - t_host0).count(), nb);
  }
#else
  (void)t_host0;
#endif
  return 0;
}

// The part of the inverse that needs only block rows [0, h) of U starts on the second stream once they are final, underneath the rest of
// the factorization (whose second half is a chain of short launches that leaves most of the chip idle).
static int start_early_inverse(bocf_ctx* c, int h) {
  HIPCHK(hipEventRecord(c->ev_half, c->stream));
  HIPCHK(hipStreamWaitEvent(c->s_inv, c->ev_half, 0));
  trtri_early(c, h, c->s_inv);
  HIPCHK(hipEventRecord(c->ev_inv_early, c->s_inv));
  return 0;
}

// Called by the single-stream Cholesky schedules right after the row solve of panel p.
static int maybe_start_early_inverse(bocf_ctx* c, const CholPlan& plan, int p) {
  if (p != plan.inv_after) return 0;
  if (start_early_inverse(c, plan.h)) return -1;
  c->early_inverse_started = 1;
  // (a second stage -- the merges inside block rows [h, 3h/2) started when row 3h/2 - 1 is solved -- was measured in round 3: visible
  //  inverse 1.22 -> 1.21 ms, Cholesky 4.62 -> 4.69 ms at config 3: neutral, not kept)
  return 0;
}

// A[pe ...][pe ...] -= U[p0 .. pe)[pe ...]^T U[p0 .. pe)[pe ...], pe = p0 + g: the trailing update behind a group of g solved block rows (K = 128 g)
static void launch_trailing_update(bocf_ctx* c, int p0, int g, hipStream_t st) {
  const int Np = c->Np, m = wm(c);
  const long strideS = (long)Np * Np;
  double* S = wS(c);
  const int pe = p0 + g;                            // first block row after the group
  const int W = Np - pe * BOCF_TILE;
  if (W <= 0) return;
  GemmArgs t{};
  double* rows = S + (long)p0 * BOCF_TILE * Np + (long)pe * BOCF_TILE;
  t.A = rows; t.lda = Np; t.strideA = strideS;
  t.B = rows; t.ldb = Np; t.strideB = strideS;
  double* trail = S + (long)pe * BOCF_TILE * Np + (long)pe * BOCF_TILE;
  t.Cin = trail; t.Cout = trail; t.ldc = Np; t.strideC = strideS;
  t.M = W; t.Ncols = W; t.K = g * BOCF_TILE; t.kb = g * BOCF_TILE; t.upper_only = 1; t.alpha = -1.0; t.beta = 1.0;
  // (epilogue 3 = the store epilogue on a grid of the upper tiles only.  A split-K treatment of the tiles of the last, partial round of a
  //  launch -- several workgroups per tile, partial sums combined by the tile's owner -- was built and measured in round 4: 4.19 ms against
  //  4.03 for this form at N = 4096, m = 4: tiles do not run in lockstep rounds, the tail packs by throughput; profiles/r04/split_tail.txt)
  launch_gemm_f64(t, m, 3, st);
}

// One panel group [p0, p0 + G) of the single-stream schedule for the current output window, on `st`.
// G panels per trailing update: the trailing matrix is read-modify-written once per G panels (its HBM traffic, not flops, is what the
// K = 128 updates cost); inside a group each new block row first receives the group's finished rows as ONE thin update with
// K = 128 * (rows so far).  G = 1: diagonal block, row solve, K = 128 trailing update.
static void chol_group_step(bocf_ctx* c, int p0, int G, hipStream_t st) {
  const int Np = c->Np, m = wm(c), nb = Np / BOCF_TILE;
  const long strideS = (long)Np * Np, strideE = (long)nb * BOCF_TILE * BOCF_TILE;
  double* S = wS(c);
  const int g = (nb - p0) < G ? (nb - p0) : G;
  for (int q = 0; q < g; ++q) {
    const int p = p0 + q;
    const int W = Np - (p + 1) * BOCF_TILE;
    if (q > 0) {
      // block row p -= U_{p0..p-1, p}^T U_{p0..p-1, p..}   (K = 128 q)
      GemmArgs t{};
      double* rows = S + (long)p0 * BOCF_TILE * Np + (long)p * BOCF_TILE;
      t.A = rows; t.lda = Np; t.strideA = strideS;
      t.B = rows; t.ldb = Np; t.strideB = strideS;
      double* row = S + (long)p * BOCF_TILE * Np + (long)p * BOCF_TILE;
      t.Cin = row; t.Cout = row; t.ldc = Np; t.strideC = strideS;
      t.M = BOCF_TILE; t.Ncols = W + BOCF_TILE; t.K = q * BOCF_TILE; t.kb = q * BOCF_TILE; t.alpha = -1.0; t.beta = 1.0;
      if (c->chol.trsm_wave)   // one block row, short K: the wave-level kernel (latency-bound either way, half the time)
        launch_tile128(rows, Np, strideS, rows, Np, strideS, row, Np, strideS, -1.0, 1.0, m, st, (W + BOCF_TILE) / BOCF_TILE, q * BOCF_TILE);
      else
        launch_gemm_f64(t, m, 0, st);
    }
    launch_potrf_diag(S, strideS, c->N, Np, p, wE(c), wET(c), strideE, winfo(c), m, st);
    launch_trsm(c, p, W, st);
  }
  launch_trailing_update(c, p0, g, st);
}


// Factorization AND inverse in one launch by resident workgroup teams (chol_team.hip), for models with few panels: the launched
// schedules below are then a chain of ~10 short dependent launches per panel with the chip idle underneath.  Panels [pfirst, pend) in
// teams of T workgroups: G = 0 ONE launch (factorization and inverse of the block from pfirst on, pend = nb), else launches of G panels,
// each followed by a trailing update.  Returns 0, or -1 on a HIP error.
static int run_cholesky_team(bocf_ctx* c, const CholPlan& plan, int pfirst, int pend, int G, int T) {
  const int Np = c->Np, m = c->m, nb = Np / BOCF_TILE, mb = plan.mb;
  const bool whole = G <= 0;
  const int g_max = whole ? nb - pfirst : G;
  const bool kinv = whole && plan.kinv;
  const long strideS = (long)Np * Np, strideE = (long)nb * BOCF_TILE * BOCF_TILE;
  const int words = chol_team_flag_words(nb);            // (the counters of output j, then the time-out word at plan.err_off)
  int* F = c->chol_flags.as<int>();
#ifdef BOCF_PROBES
  const char* tl_path = getenv("BOCF_TEAM_TL");            // probes build: per-task stamps of every workgroup of the LAST launch (tools/team_timeline.py)
  const size_t tl_words = (size_t)plan.ncu * 512 * 4;
  if (tl_path && !c->team_tl) HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->team_tl), sizeof(unsigned long long) * tl_words));
#endif
  for (int p0 = pfirst; p0 < pend; p0 += g_max) {
    const int g = pend - p0 < g_max ? pend - p0 : g_max;
#ifdef BOCF_PROBES
    const char* tl_grp = getenv("BOCF_TEAM_TL_GROUP");     // which panel group's launch the timeline keeps (default: the last)
    const bool tl_this = tl_path && (!tl_grp || atoi(tl_grp) == p0 / g_max);
    if (tl_this) HIPCHK(hipMemsetAsync(c->team_tl, 0, sizeof(unsigned long long) * tl_words, c->stream));
#endif
    for (int j0 = 0; j0 < m; j0 += mb) {
      const int mr = m - j0 < mb ? m - j0 : mb;
      TeamArgs a{};
      a.S = wS(c) + (long)j0 * strideS; a.RT = wRT(c) + (long)j0 * strideS; a.R = wR(c) + (long)j0 * strideS; a.strideS = strideS;
      a.E = wE(c) + (long)j0 * strideE; a.ET = wET(c) + (long)j0 * strideE; a.strideE = strideE;
      a.N = c->N; a.Np = Np; a.nb = nb;
      a.info = winfo(c) + j0;
      a.F = F + (size_t)j0 * words; a.fstride = words;
      a.err = F + plan.err_off;
      a.T = T; a.p0 = p0; a.p1 = p0 + g; a.do_inverse = whole ? 1 : 0; a.tl = nullptr;
      a.KI = wT(c) + (long)j0 * strideS; a.do_kinv = kinv ? 1 : 0;
      // (streaming the critical tiles pays while the chain of diagonal blocks sets the pace: measured m = 4, 16 panels 1.11 -> 0.99 ms, 20: a tie, 24: 2.52 -> 2.63)
      a.crit_load = c->chol.team_crit_load; a.stream = c->chol.team_stream && g <= 20 ? 1 : 0;
#ifdef BOCF_PROBES
      a.tl = tl_this ? c->team_tl : nullptr;
#endif
      launch_chol_team(a, mr, c->stream);
    }
    if (!whole) {
      launch_trailing_update(c, p0, g, c->stream);
      for (int p = p0; p < p0 + g && pend == nb; ++p)      // (the hybrid, which stops at pend, starts the inverse itself)
        if (maybe_start_early_inverse(c, plan, p)) return -1;
    }
  }
#ifdef BOCF_PROBES
  if (tl_path) {
    std::vector<unsigned long long> h(tl_words);
    HIPCHK(hipMemcpyAsync(h.data(), c->team_tl, sizeof(unsigned long long) * tl_words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (FILE* f = fopen(tl_path, "w")) {
      fprintf(f, "# T %d nb %d m %d\n", T, nb, m);
      for (size_t b = 0; b < (size_t)plan.ncu; ++b)
        for (size_t k = 0; k < 512; ++k) {
          const unsigned long long* r = h.data() + (b * 512 + k) * 4;
          if (r[0]) fprintf(f, "%zu %llu %llu %llu %llu\n", b, r[0], r[1], r[2], r[3]);
        }
      fclose(f);
    }
  }
#endif
  if (whole && pfirst == 0) {
    // (the teams write R^T (lower) and, transposed, R (upper): the strictly lower half of R / upper half of R^T is the zero half no fit ever writes)
    c->inverse_done = 1;
    c->kinv_done = kinv ? 1 : 0;
  }
  return 0;
}


// More than 24 panels: the launched schedule for the first h panels -- that is where the big trailing updates are, which the GEMM kernel does at
// 2-3x the rate of the teams' unit products -- and ONE team launch for the rest (Cholesky AND inverse of the trailing block: a problem of
// nb - h <= 24 panels, where the chain of diagonal blocks is what matters and the teams win).  h = the inverse's own split (largest power of
// two below nb): the inverse of the first h block rows and the first product of the top-level merge run on the second stream underneath,
// as in the launched schedule; after the team launch only R22 = (R22^T)^T and the merge's second product  R12 = -(R11 U12) R22  are left.
// The two parts share one zeroing of the counter block: a team launch over panels [p0, p1) touches only the counters of panels and block
// rows >= p0 -- P, D, ST, RD of its own panels, TR / IR rows from p0 on -- and reads the next panel's P only while that is still unwritten, so
// the first part's counters (rows < h) and the tail's (rows >= h) are disjoint, as those of the first part's successive launches are.  The
// time-out word is shared: one that fires in the first part reaches bocf_fit.
static int run_cholesky_hybrid(bocf_ctx* c, const CholPlan& plan) {
  const int nb = c->Np / BOCF_TILE, h = plan.h;
  if (plan.panels > 0) {                                   // (A/B: the first block rows by team launches of team_panels panels + trailing updates)
    if (run_cholesky_team(c, plan, 0, h, plan.panels, plan.T)) return -1;
  } else {
    for (int p0 = 0; p0 < h; p0 += plan.G) chol_group_step(c, p0, h - p0 < plan.G ? h - p0 : plan.G, c->stream);
  }
  // the first h block rows of U are final: their inverse, and the first product of the top-level merge, underneath the team launch
  if (start_early_inverse(c, h)) return -1;
  if (run_cholesky_team(c, plan, h, nb, 0, plan.T_tail)) return -1;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_inv_early, 0));
  merge_level(c, 0, h, nb - h, 1, MERGE_SECOND, c->stream);
  c->inverse_done = 1;
  return 0;
}

// The launched schedule: everything on the context's stream, G panels per trailing update.
static int run_cholesky_launched(bocf_ctx* c, const CholPlan& plan) {
  const int nb = c->Np / BOCF_TILE;
  for (int p0 = 0; p0 < nb; p0 += plan.G) {
    chol_group_step(c, p0, plan.G, c->stream);
    for (int p = p0; p < p0 + plan.G && p < nb; ++p)
      if (maybe_start_early_inverse(c, plan, p)) return -1;
  }
  return 0;
}

// The schedule of the next factorization of c (chol_plan.h) and what it needs: the reserved-CU streams, the counter block.  The one
// refusal the runtime may still make -- CU masks (hipExtStreamCreateWithCUMask) -- comes before anything is enqueued and is planned round.
// kinv: the caller is an inference (bocf_lml_gradients follows), a schedule that can, leaves Ky^-1 in the T scratch.
int bocf_plan_cholesky(bocf_ctx* c, bool kinv, CholPlan* out) {
  CholPlanInput in;
  in.nb = c->Np / BOCF_TILE; in.m = c->m; in.sched_m = c->sched_m; in.ncu = c->ncu;
  in.inv_stream = c->s_inv != nullptr; in.cu_masks_ok = c->cu_masks_ok; in.gated_off = c->gated_off; in.sched_retry = c->sched_retry;
  in.refit = c->fits_done > 0; in.want_kinv = kinv;
  c->sched_retry = 0;
  CholPlan plan = plan_cholesky(in, c->chol);
  if (plan.schedule == CHOL_RESERVED) {
    const int rs = ensure_reserved_streams(c, plan.reserved_cus, plan.ncu);
    if (rs < 0) return -1;
    if (rs > 0) {                                          // (cu_masks_ok is cleared for the context's later fits too)
      in.cu_masks_ok = false;
      plan = plan_cholesky(in, c->chol);
    }
  }
  if (plan.flag_ints > 0 && c->chol_flags.ensure(sizeof(int) * plan.flag_ints)) return -1;
  *out = plan;
  return 0;
}

static int run_cholesky_impl(bocf_ctx* c, const CholPlan& plan, bool counters_zeroed) {
  c->early_inverse_started = 0;
  c->inverse_done = 0;
  c->kinv_done = 0;
  c->last_schedule = plan.schedule;
  c->chol_flags_used = plan.flag_ints > 0 ? 1 : 0;
  c->chol_err_off = plan.err_off;
  set_potrf_scalar(c->chol.potrf_scalar);                // (probes build: timing-only variants of the diagonal-block kernel)
  // the counters and the time-out word, zeroed ONCE per factorization (unless the caller's kernels do it: the team schedule of a
  // stream-resident HMC chain)
  if (plan.flag_ints > 0 && !counters_zeroed) HIPCHK(hipMemsetAsync(c->chol_flags.p, 0, sizeof(int) * plan.flag_ints, c->stream));
  const int nb = c->Np / BOCF_TILE;
  switch (plan.schedule) {
    case CHOL_TEAM_WHOLE: return run_cholesky_team(c, plan, 0, nb, 0, plan.T);
    case CHOL_TEAM_GROUPS: return run_cholesky_team(c, plan, 0, nb, plan.panels, plan.T);
    case CHOL_RESERVED: return run_cholesky_reserved(c, plan);
    case CHOL_HYBRID: return run_cholesky_hybrid(c, plan);
    case CHOL_LAUNCHED: break;
  }
  return run_cholesky_launched(c, plan);
}

int bocf_run_cholesky(bocf_ctx* c, const CholPlan& plan, bool counters_zeroed) {
#ifdef BOCF_PROBES
  const char* tl = getenv("BOCF_DBG_TL");                // plain-run timeline of the chain kernels (tools/dbg_timeline.py)
  if (tl) {
    HIPCHK(hipStreamSynchronize(c->stream));
    dbg_tl_start();
  }
  const int rc = run_cholesky_impl(c, plan, counters_zeroed);
  if (tl && rc == 0) dbg_tl_dump(tl);
  return rc;
#else
  return run_cholesky_impl(c, plan, counters_zeroed);
#endif
}

// R = U^-1 (upper) by recursive doubling over the 128-blocks: the diagonal tiles are the E_p of the
// diagonal-block kernel; two neighbouring inverted blocks [lo,mid), [mid,hi) merge with
//     R12 = -(R11 * U12) * R22
// as two GEMMs.  All merges of one level are independent and run as ONE batched launch, so the whole inverse is
// ~log2(nb) levels of large GEMMs instead of nb dependent thin ones.  RT holds R^T (lower): the first product needs R11
// k-major.  The association (R11 U12) first matters twice: U12 enters as rows of the upper factor (no mirrored copy of U is
// needed), and the first product of a merge depends only on the LEFT half -- so everything that involves only the first h
// block rows (all their merges and the first product of the top-level merge) can run while the Cholesky is still busy
// with the block rows below (run_cholesky starts it on a second stream as soon as panel h-1 is solved).
//   first :  T'[r][c']   = sum_{kk >= r} R11[r][kk] U12[kk][c']        A = RT11, B = rows of U; then T'^T by a transpose
//   second:  RT21[c][r]  = -sum_{kk <= c} R22[kk][c] T'^T[kk][r]        A = rows of R22, B = T'^T; then R12 by a transpose
static void merge_level(bocf_ctx* c, int lo, int w, int w2, int count, int which, hipStream_t st) {
  const int Np = c->Np, m = wm(c);
  const long strideS = (long)Np * Np;
  const long dstep = (long)2 * w * BOCF_TILE * (Np + 1);            // next pair along the diagonal
  const long oLo = (long)lo * BOCF_TILE, oMid = (long)(lo + w) * BOCF_TILE;
  const int b1 = w * BOCF_TILE, b2 = w2 * BOCF_TILE;
  double* S = wS(c);
  double* R = wR(c);
  double* RT = wRT(c);
  double* T = wT(c);
  // Both products are arranged so that the contraction length depends on the ROW tile (whole rows of equal-length
  // workgroups, heaviest rows first): measured 0.85 ms against 1.03-1.09 ms for the same product with the length varying
  // along a row (top level of N = 4096).  The price is one extra transpose per level.
  if (which & MERGE_FIRST) {
    // T'[r][c'] = sum_{kk >= r} R11[r][kk] U12[kk][c']      A = RT11 (k-major R11), B = rows of U;  into T at (lo, mid)
    GemmArgs g{};
    g.A = RT + oLo * Np + oLo; g.lda = Np; g.strideA = strideS; g.strideA2 = dstep;
    g.B = S + oLo * Np + oMid; g.ldb = Np; g.strideB = strideS; g.strideB2 = dstep;
    g.Cin = nullptr; g.Cout = T + oLo * Np + oMid; g.ldc = Np; g.strideC = strideS; g.strideC2 = dstep;
    g.M = b1; g.Ncols = b2; g.K = b1; g.kb = b1; g.kbeg_rt = BOCF_TILE; g.alpha = 1.0; g.batch1 = m;
    g.swizzle = 2;      // row-tile-major across the whole batch (all outputs' heaviest row tiles first): inverse 2.55 -> 2.03 ms at config 3
    launch_gemm_f64(g, m * count, 0, st);
    // T'^T into T at (mid, lo): the k-major operand of the second product
    launch_transpose_block(T, T, strideS, Np, (int)oLo, (int)oMid, b1, b2, count, 2 * w * BOCF_TILE, m, st);
  }
  if (which & MERGE_SECOND) {
    // RT21[c][r] = R12[r][c] = -sum_{kk <= c} R22[kk][c] T'^T[kk][r]      A = rows of R22, B = T'^T;  straight into R^T
    GemmArgs h{};
    h.A = R + oMid * Np + oMid; h.lda = Np; h.strideA = strideS; h.strideA2 = dstep;
    h.B = T + oMid * Np + oLo; h.ldb = Np; h.strideB = strideS; h.strideB2 = dstep;
    h.Cin = nullptr; h.Cout = RT + oMid * Np + oLo; h.ldc = Np; h.strideC = strideS; h.strideC2 = dstep;
    h.M = b2; h.Ncols = b1; h.K = b2; h.kb = BOCF_TILE; h.krt = BOCF_TILE; h.rt_desc = 1; h.alpha = -1.0; h.batch1 = m;
    // the three-buffer triangular kernel with its store epilogue (the product has the variance's shape) from 4096 rows: measured inverse 6.80 -> 6.53 ms
    // at N = 8192, but 1.47 -> 1.55 at N = 4096 (2048-row products: 512 workgroups of very unequal length on 256 CUs suit the smaller tiles better)
    h.no_x3 = c->chol.merge_x3 <= 0 || (c->chol.merge_x3 == 1 && b2 < 4096);
    h.swizzle = 2;
    launch_gemm_f64(h, m * count, 0, st);
    // R12 = RT21^T
    launch_transpose_block(RT, R, strideS, Np, (int)oMid, (int)oLo, b2, b1, count, 2 * w * BOCF_TILE, m, st);
  }
}

static void copy_diag_range(bocf_ctx* c, int blk_lo, int blk_hi, hipStream_t st) {
  const int Np = c->Np, m = wm(c), nb = Np / BOCF_TILE;
  const long strideS = (long)Np * Np, strideE = (long)nb * BOCF_TILE * BOCF_TILE;
  launch_copy_diag_blocks(wE(c), strideE, wR(c), strideS, Np, blk_lo, blk_hi, m, st);
  launch_copy_diag_blocks(wET(c), strideE, wRT(c), strideS, Np, blk_lo, blk_hi, m, st);
}

// everything of the inverse that needs only block rows [0, h) of U: runs on `st` as soon as those rows are final
static void trtri_early(bocf_ctx* c, int h, hipStream_t st) {
  const int nb = c->Np / BOCF_TILE;
  copy_diag_range(c, 0, h, st);
  for (int w = 1; w < h; w *= 2) merge_level(c, 0, w, w, h / (2 * w), MERGE_FIRST | MERGE_SECOND, st);
  merge_level(c, 0, h, nb - h, 1, MERGE_FIRST, st);
}

// the rest: the merges among block rows [h, nb) and the second product of the top-level merge
static void trtri_late(bocf_ctx* c, int h, hipStream_t st) {
  const int nb = c->Np / BOCF_TILE;
  copy_diag_range(c, h, nb, st);
  for (int w = 1; w < h; w *= 2) {
    const int full = nb / (2 * w);                       // pairs with two complete halves
    const int first = h / (2 * w);                       // pairs that lie inside [0, h): done early
    if (full > first) merge_level(c, h, w, w, full - first, MERGE_FIRST | MERGE_SECOND, st);
    const int g = full * 2 * w;                          // a trailing incomplete pair, if any
    if (g + w < nb && g >= h) merge_level(c, g, w, nb - (g + w), 1, MERGE_FIRST | MERGE_SECOND, st);
  }
  merge_level(c, 0, h, nb - h, 1, MERGE_SECOND, st);
}

// levels [level_lo, level_hi) of the whole inverse of the current window on `st` (level -1 = the copy of the inverted diagonal blocks,
// level l = the merges of width 2^l)
static void trtri_all(bocf_ctx* c, hipStream_t st, int level_lo, int level_hi) {
  const int nb = c->Np / BOCF_TILE;
  if (level_lo < 0) copy_diag_range(c, 0, nb, st);
  int lv = 0;
  for (int w = 1; w < nb; w *= 2, ++lv) {
    if (lv < level_lo || lv >= level_hi) continue;
    const int full = nb / (2 * w);                       // pairs with two complete halves
    if (full > 0) merge_level(c, 0, w, w, full, MERGE_FIRST | MERGE_SECOND, st);
    const int g = full * 2 * w;                          // a trailing incomplete pair, if any
    if (g + w < nb) merge_level(c, g, w, nb - (g + w), 1, MERGE_FIRST | MERGE_SECOND, st);
  }
}

int bocf_run_trtri(bocf_ctx* c, bool early_done) {
  if (c->inverse_done) return 0;                         // the team schedule produced R and R^T with the factorization
  const int nb = c->Np / BOCF_TILE;
  if (early_done) {                                      // the first h block rows were inverted underneath the factorization
    trtri_late(c, trtri_split(nb), c->stream);
    return 0;
  }
  // everything here: every level is ONE batched launch over all its pairs (the early / late split would double the
  // launch count, which is what the small sizes are made of)
  trtri_all(c, c->stream, -1, 64);
  return 0;
}

