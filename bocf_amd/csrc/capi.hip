// C ABI of libbocf_hip.so (declared in include/bocf_hip.h): context, memory, and the launch
// sequences of fit / predict / acquisition / selection.  No torch types, no CPU fallback.
#include "bocf_ctx.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static thread_local std::string g_err;
int bocf_fail(const char* what, const char* detail) {
  g_err = std::string(what) + ": " + (detail ? detail : "");
  return -1;
}
void bocf_set_error(const char* text) { g_err = text ? text : ""; }

// first failed kernel launch since the last report (BOCF_LAUNCH, bocf_internal.h)
static thread_local std::string g_launch_err;
void bocf_note_launch(const char* kernel, hipError_t e) {
  if (e != hipSuccess && g_launch_err.empty()) g_launch_err = std::string("launch of ") + kernel + ": " + hipGetErrorString(e);
}
int bocf_launch_status() {
  const hipError_t e = hipGetLastError();
  if (!g_launch_err.empty()) {
    g_err = g_launch_err;
    g_launch_err.clear();
    return -1;
  }
  if (e != hipSuccess) return fail("hipGetLastError", hipGetErrorString(e));
  return 0;
}

extern "C" int bocf_version(void) { return 100; }
extern "C" const char* bocf_last_error(void) { return g_err.c_str(); }

extern "C" int bocf_create(int device, bocf_ctx** out) {
  if (!out) return fail("bocf_create", "null out");
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail("bocf_create", "no such HIP device");
  HIPCHK(hipSetDevice(device));
  bocf_ctx* c = new bocf_ctx();
  c->device = device;
  hipError_t e = hipStreamCreate(&c->stream);
  if (e != hipSuccess) {
    delete c;
    return fail("hipStreamCreate", hipGetErrorString(e));
  }
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) {
    delete c;
    return fail("hipGetDeviceProperties", hipGetErrorString(e));
  }
  c->ncu = prop.multiProcessorCount;
  e = hipMalloc((void**)&c->tile_ctr, 2 * sizeof(int));
  if (e == hipSuccess) e = hipMemset(c->tile_ctr, 0, 2 * sizeof(int));
  if (e != hipSuccess) {
    if (c->tile_ctr) (void)hipFree(c->tile_ctr);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return fail("bocf_create: tile counters", hipGetErrorString(e));
  }
  *out = c;
  return 0;
}

static void drop_events(bocf_ctx* c) {
  for (auto& pr : c->events) {
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  c->events.clear();
}

static void drop_phases(bocf_ctx* c) {
  for (auto& kv : c->phases)
    for (auto& pr : kv.second) {
      (void)hipEventDestroy(pr.first);
      (void)hipEventDestroy(pr.second);
    }
  c->phases.clear();
}

extern "C" void bocf_destroy(bocf_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)bocf_comm_destroy(c);
  if (c->shard_helper) bocf_destroy(c->shard_helper);
  c->shard_helper = nullptr;
  if (c->ts_helper) bocf_destroy(c->ts_helper);
  c->ts_helper = nullptr;
  for (DevBuf& b : c->ts_F) b.release();
  for (DevBuf& b : c->pt_buf) b.release();
  drop_events(c);
  drop_phases(c);
  if (c->pin_in) (void)hipHostFree(c->pin_in);
  if (c->pin_out) (void)hipHostFree(c->pin_out);
  if (c->fit_pin) (void)hipHostFree(c->fit_pin);
  if (c->up_pin) (void)hipHostFree(c->up_pin);
  if (c->ev_pin) (void)hipEventDestroy(c->ev_pin);
  if (c->eu_pin) (void)hipHostFree(c->eu_pin);
  if (c->ev_eu_pin) (void)hipEventDestroy(c->ev_eu_pin);
  DevBuf* bufs[] = {&c->R32, &c->Ri8, &c->Ri8e, &c->Ki8, &c->Ki8e, &c->X, &c->Xs, &c->S, &c->R, &c->RT, &c->E, &c->ET, &c->T, &c->yc, &c->tvec, &c->alpha, &c->lml, &c->jit, &c->hypd,
                    &c->info, &c->mu_train, &c->rvec, &c->dvec, &c->hmc_buf, &c->Xc, &c->Kstar, &c->meanpart, &c->sumsq, &c->mean, &c->var, &c->acq, &c->Vbuf, &c->dmean, &c->dvar, &c->dacq, &c->Vs, &c->Ws, &c->theta,
                    &c->prob, &c->best, &c->params, &c->Wt, &c->blk_idx, &c->blk_val, &c->out_idx, &c->out_val, &c->gpart, &c->gout, &c->pack, &c->gidx,
                    &c->gval, &c->shard_meta, &c->chol_flags, &c->eu_theta, &c->eu_rows, &c->eu_Z, &c->eu_val, &c->eu_grad,
                    &c->ts_X, &c->ts_K, &c->ts_V, &c->ts_mp, &c->ts_mu, &c->ts_Z, &c->ts_jit, &c->ts_u, &c->ts_theta, &c->ts_params, &c->ts_out,
                    &c->kg_XA, &c->kg_VA, &c->kg_Wa, &c->kg_muA, &c->kg_s2A, &c->kg_nug, &c->kg_V, &c->kg_W, &c->kg_cov, &c->kg_s2c, &c->kg_dcov, &c->kg_dmean, &c->kg_dvar,
                    &c->kg_par, &c->kg_v0, &c->kg_astar, &c->kg_AB, &c->kg_out, &c->kg_dout, &c->prog_buf,
                    &c->pd_XP, &c->pd_VP, &c->pd_Wp, &c->pd_muP, &c->pd_cov, &c->pd_pack, &c->pd_QFG, &c->pd_par, &c->pd_best, &c->pd_T, &c->pd_muc, &c->pd_E,
                    &c->pt_E, &c->pt_g, &c->pt_rhs, &c->pt_tmp, &c->pt_nug, &c->pt_par, &c->pt_rows, &c->pt_tab, &c->pt_pv, &c->pt_pg, &c->pt_val, &c->pt_grad,
                    &c->cq_tab, &c->cq_par, &c->cq_best, &c->cq_nf, &c->cu_par, &c->cu_val, &c->cu_pof, &c->cu_grad, &c->cu_rng, &c->rf_dbl, &c->rf_int, &c->rf_x2, &c->rf_acq,
                    &c->loo_out, &c->loo_sum, &c->loo_shift, &c->loo_par, &c->loo_rows, &c->loo_val,
                    &c->jt_V, &c->jt_W, &c->jt_mu, &c->jt_cov, &c->jt_dmean, &c->jt_dvar, &c->jt_dcov, &c->jt_par, &c->jt_best, &c->jt_fl, &c->jt_E, &c->jt_dout,
                    &c->rk_par, &c->lg_par, &c->lg_best};
  for (DevBuf* b : bufs) b->release();
  if (c->infer_out) (void)hipHostFree(c->infer_out);
  if (c->tile_ctr) (void)hipFree(c->tile_ctr);
  for (hipEvent_t ev : c->ev_chol) (void)hipEventDestroy(ev);
  for (hipStream_t st : {c->s_res, c->s_hi, c->s_bulk, c->s_inv})
    if (st) (void)hipStreamDestroy(st);
  if (c->ev_half) (void)hipEventDestroy(c->ev_half);
  if (c->ev_inv_early) (void)hipEventDestroy(c->ev_inv_early);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

// ---------------------------------------------------------------------------------------------
// Options.  ONE table: name, accepted range, kind.  Kind 0 = speed only (schedules, tilings, workspace sizes: every setting
// computes the same result up to rounding, the tests pin that); kind 1 = documented semantics (fp32 contraction, the hyper-sample
// layout of the fitted outputs, data re-use between inferences: what the caller ASKS for); kind 2 = probes and test hooks
// (timing-only kernel variants whose results are wrong, the diagonal shift that forces the jitter ladder, the single-process
// stand-in for the ranks of a sharded fit) -- compiled only with -DBOCF_PROBES into libbocf_hip_probes.so, which tools/ and the
// tests that need a hook load; the product library has no such entry and rejects the names.  bocf_option_info / bocf_option_check
// need no GPU: the CPU suite enumerates the table (tests/test_host_cpu.py).
struct OptDesc {
  const char* name;
  long long lo, hi;
  int kind;
  void (*set)(bocf_ctx*, long long);
  bool (*extra)(long long);          // further constraint inside [lo, hi] (nullptr = none)
  const char* what;
};
static bool opt_lookahead_ok(long long v) { return v == -1 || v == 0 || v == 2; }
#ifdef BOCF_PROBES
static bool opt_swizzle_ok(long long v) { return v == -1 || v == 0 || v == 1 || (v >= 100 && v < 164) || (v >= 256 && v <= 258); }
static bool opt_potrf_ok(long long v) { return v == 0 || (v >= 11 && v <= 14); }
#else
static bool opt_swizzle_ok(long long v) { return v == -1 || v == 0 || v == 258; }
#endif
static const OptDesc g_options[] = {
    {"chunk", 128, 1 << 24, 0, [](bocf_ctx* c, long long v) { c->chunk = (long)round_up((int)v, 128); }, nullptr, "candidates per pass (rounded up to 128)"},
    {"workspace_mb", 1, 1 << 20, 0, [](bocf_ctx* c, long long v) { c->workspace_mb = (long)v; }, nullptr, "cap of the per-pass K* workspace"},
    {"profile", 0, 1, 0, [](bocf_ctx* c, long long v) { c->profile = v != 0; }, nullptr, "HIP events around the dominant kernel and the named phases"},
    {"predict_f32", 0, 1, 1, [](bocf_ctx* c, long long v) { c->predict_f32 = v != 0; }, nullptr, "fp32 variance contraction (BASELINE configs[4])"},
    {"i8_group", 0, 64, 0, [](bocf_ctx* c, long long v) { c->i8_group = (int)v; }, nullptr, "predict_i8: 0 = workgroups in blocks of 4 row-tile pairs x 8 column tiles per XCD; g >= 1 = bands of g pairs x all column tiles"},
    {"predict_i8", 0, 1, 1, [](bocf_ctx* c, long long v) { c->predict_i8 = v != 0; }, nullptr, "variance contraction in exact int8 products (six radix-254 digits per operand column, fp64 recombination)"},
    {"fused_infer", 0, 1, 0, [](bocf_ctx* c, long long v) { c->fused_infer = v != 0; }, nullptr, "one fused launch per inference for N <= 128"},
    {"reuse_data", 0, 1, 1, [](bocf_ctx* c, long long v) { c->reuse_data = v != 0; }, nullptr, "next fits reuse the resident X / Y"},
    {"skip_mu_train", 0, 1, 1, [](bocf_ctx* c, long long v) { c->skip_mu_train = v != 0; }, nullptr, "do not refresh the mean at the training inputs"},
    {"aggregate", 0, 8, 0, [](bocf_ctx* c, long long v) { c->chol.aggregate = (int)v; }, nullptr, "panels per trailing update (0 = by size)"},
    {"lookahead", -1, 2, 0, [](bocf_ctx* c, long long v) { c->chol.lookahead = (int)v; }, opt_lookahead_ok,
     "factorization schedule: -1 by size, 0 single stream, 2 reserved-CU chain"},
    {"team_fit", -1, 1, 0, [](bocf_ctx* c, long long v) { c->chol.team_fit = (int)v; }, nullptr, "factorization + inverse in one launch by resident workgroup teams (-1 = by size)"},
    {"team_panels", 1, 32, 0, [](bocf_ctx* c, long long v) { c->chol.team_panels = (int)v; }, nullptr, "team schedule above 8 panels: panels per team launch (one trailing update each)"},
    {"team_hybrid", 0, 2, 0, [](bocf_ctx* c, long long v) { c->chol.team_hybrid = (int)v; }, nullptr, "more than 24 panels: launched schedule for the first block rows, one team launch for the rest"},
    {"team_tail_share", 1, 8, 0, [](bocf_ctx* c, long long v) { c->chol.team_tail_share = (int)v; }, nullptr, "hybrid schedule: eighths of the compute units the tail's teams take"},
    {"team_whole_max", 2, 32, 0, [](bocf_ctx* c, long long v) { c->chol.team_whole_max = (int)v; }, nullptr, "panels up to which one team launch does the whole factorization and inverse"},
    {"team_stream", 0, 1, 0, [](bocf_ctx* c, long long v) { c->chol.team_stream = (int)v; }, nullptr, "teams: the critical tiles are formed underneath the diagonal blocks, 16 rows at a time"},
    {"team_crit_load", 0, 4096, 0, [](bocf_ctx* c, long long v) { c->chol.team_crit_load = (int)v; }, nullptr, "teams: critical-chain workgroups carry nothing else while the others get by with <= this many units each"},
    {"lookahead_min_nb", 2, 1 << 20, 0, [](bocf_ctx* c, long long v) { c->chol.lookahead_min_nb = (int)v; }, nullptr, "reserved-CU schedule from this many panels"},
    {"merge_x3", 0, 2, 0, [](bocf_ctx* c, long long v) { c->chol.merge_x3 = (int)v; }, nullptr, "second product of an inverse merge in the three-buffer kernel"},
    {"shard_fit", 0, 1, 0, [](bocf_ctx* c, long long v) { c->shard_fit = v != 0; }, nullptr, "output-sharded fit over the communicator"},
    {"trsm_wave", 0, 1, 0, [](bocf_ctx* c, long long v) { c->chol.trsm_wave = v != 0; }, nullptr, "row solves through the wave-level single-tile kernel"},
    {"overlap_inverse", -1, 1, 0, [](bocf_ctx* c, long long v) { c->chol.overlap_inverse = (int)v; }, nullptr, "early part of the inverse underneath the factorization (-1 = by size)"},
    {"small_path", 0, 1, 0, [](bocf_ctx* c, long long v) { c->small_path = v != 0; }, nullptr, "GEMV-shaped path for <= 16 candidates"},
    {"prefetch1", 0, 1, 0, [](bocf_ctx* c, long long v) { c->prefetch1 = v != 0; }, nullptr, "one-tile-deep staging in the 128-row variance kernel"},
    {"swizzle", -1, 258, 0, [](bocf_ctx* c, long long v) { c->swizzle = (int)v; }, opt_swizzle_ok, "variance-GEMM tiling: -1 by size, 0 128-row tiles, 258 256-row tiles (probes build: also 1, 100..163, 256, 257)"},
    {"hyper_samples", 1, 64, 1,
     [](bocf_ctx* c, long long v) {
       if ((int)v != c->hyper_samples) c->S_mc = c->eu_S = 0;   // the transposed normals are laid out per group size
       c->hyper_samples = (int)v;
     },
     nullptr, "the fitted outputs are H hyper-samples x m / H model outputs"},
    {"acq_hyper_samples", 0, 64, 1, [](bocf_ctx* c, long long v) { c->acq_hyper_samples = (int)v; }, nullptr, "hyper-samples the acquisitions average over (0 = all)"},
    {"best_group", -1, 63, 1, [](bocf_ctx* c, long long v) { c->best_group = (int)v; }, nullptr, "whose best-so-far every hyper-sample uses (-1 = its own)"},
#ifdef BOCF_PROBES
    {"potrf_scalar", 0, 14, 2, [](bocf_ctx* c, long long v) { c->chol.potrf_scalar = (int)v; }, opt_potrf_ok, "TIMING-ONLY variants of the diagonal-block kernel: 11..14 (wrong results)"},
    {"shard_fit_simulate", 0, 64, 2, [](bocf_ctx* c, long long v) { c->shard_fit_simulate = (int)v; }, nullptr, "TEST HOOK: one process plays all G ranks of a sharded fit"},
    {"kstar_valu_probe", 0, 4, 2, [](bocf_ctx* c, long long v) { c->kstar_valu_probe = (int)v; }, nullptr, "TIMING-ONLY variants of the two-buffer 256-row variance kernel (wrong results)"},
    {"test_diag_shift_1e12", -1000000000000000LL, 1000000000000000LL, 2, [](bocf_ctx* c, long long v) { c->test_diag_shift = (double)v * 1e-12; }, nullptr,
     "TEST HOOK: Ky diagonal -= value * 1e-12 (forces the jitter ladder)"},
    {"force_sched_timeout", 0, 1, 2, [](bocf_ctx* c, long long v) { c->force_sched_timeout = (int)v; }, nullptr, "TEST HOOK: the next gated schedule reports a dependency time-out"},
    {"force_cu_count", 0, 4096, 2, [](bocf_ctx* c, long long v) { c->chol.force_cu_count = (int)v; }, nullptr, "TEST HOOK: pretend the device has this many compute units (schedule selection)"},
#endif
};
static const int g_noptions = (int)(sizeof(g_options) / sizeof(g_options[0]));

static const OptDesc* find_option(const char* name) {
  for (int i = 0; i < g_noptions; ++i)
    if (!strcmp(name, g_options[i].name)) return &g_options[i];
  return nullptr;
}

extern "C" int bocf_option_count(void) { return g_noptions; }

extern "C" int bocf_option_info(int index, const char** name_out, long long* lo_out, long long* hi_out, int* kind_out, const char** what_out) {
  if (index < 0 || index >= g_noptions) return fail("bocf_option_info", "index out of range");
  const OptDesc& o = g_options[index];
  if (name_out) *name_out = o.name;
  if (lo_out) *lo_out = o.lo;
  if (hi_out) *hi_out = o.hi;
  if (kind_out) *kind_out = o.kind;
  if (what_out) *what_out = o.what;
  return 0;
}

extern "C" int bocf_option_check(const char* name, long long value) {
  if (!name) return fail("bocf_set_option", "null argument");
  const OptDesc* o = find_option(name);
  if (!o) return fail("bocf_set_option", (std::string("unknown option '") + name + "'").c_str());
  if (value < o->lo || value > o->hi || (o->extra && !o->extra(value)))
    return fail("bocf_set_option", (std::string(name) + " = " + std::to_string(value) + " is out of range: " + o->what).c_str());
  return 0;
}

extern "C" int bocf_set_option(bocf_ctx* c, const char* name, long long value) {
  if (!c || !name) return fail("bocf_set_option", "null argument");
  if (bocf_option_check(name, value)) return -1;
  find_option(name)->set(c, value);
  return 0;
}

extern "C" int bocf_sync(bocf_ctx* c) {
  if (!c) return fail("bocf_sync", "null ctx");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// Test / inspection hook: a posterior handed over by the host instead of computed by fit + predict.
extern "C" int bocf_set_posterior(bocf_ctx* c, int m, int C, int N, const double* mean, const double* var, const double* mu_train) {
  if (!c || !mean || !var || !mu_train) return fail("bocf_set_posterior", "null argument");
  if (m < 1 || m > BOCF_MAX_FITS || C < 1 || N < 1) return fail("bocf_set_posterior", "m, C or N out of range");
  HIPCHK(hipSetDevice(c->device));
  const int cap = round_up(C, BOCF_TILE);
  if (c->mean.ensure(sizeof(double) * (size_t)m * cap) || c->var.ensure(sizeof(double) * (size_t)m * cap) || c->acq.ensure(sizeof(double) * cap) ||
      c->mu_train.ensure(sizeof(double) * (size_t)m * N))
    return -1;
  for (int j = 0; j < m; ++j) {
    HIPCHK(hipMemcpyAsync(c->mean.as<double>() + (size_t)j * cap, mean + (size_t)j * C, sizeof(double) * C, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->var.as<double>() + (size_t)j * cap, var + (size_t)j * C, sizeof(double) * C, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemcpyAsync(c->mu_train.p, mu_train, sizeof(double) * (size_t)m * N, hipMemcpyHostToDevice, c->stream));
  c->mu_epoch++;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->m = m; c->N = N; c->Np = round_up(N, BOCF_TILE); c->d = 1; c->C = C; c->pred_cap = cap;
  bocf_thompson_drop(c);
  bocf_kg_drop(c);
  bocf_pending_drop(c);
  bocf_paths_drop(c);
  c->fitted = true;
  c->canned = true;
  c->have_acq = false;
  c->S_mc = 0;
  c->eu_S = 0;
  return 0;
}

#define BOCF_PIN_BYTES ((size_t)1 << 18)
static int pin_ensure(void** p, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return 0;
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  *cap = 0;
  const size_t want = bytes < 4096 ? 4096 : bytes;
  if (hipHostMalloc(p, want, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return 1;                                              // (the caller takes the pageable path)
  }
  *cap = want;
  return 0;
}

extern "C" int bocf_set_candidates(bocf_ctx* c, const double* Xc, int C) {
  if (!c || !c->fitted) return fail("bocf_set_candidates", "model not fitted");
  if (c->canned) return fail("bocf_set_candidates", "the context holds a host-given posterior (bocf_set_posterior): fit first");
  if (C < 0 || (C > 0 && !Xc)) return fail("bocf_set_candidates", "bad candidate batch");
  HIPCHK(hipSetDevice(c->device));
  c->have_acq = false;
  bocf_thompson_drop(c);
  c->C = C;
  if (C == 0) return 0;
  if (c->Xc.ensure(sizeof(double) * (size_t)C * c->d)) return -1;
  const size_t bytes = sizeof(double) * (size_t)C * c->d;
  if (bytes <= BOCF_PIN_BYTES && pin_ensure(&c->pin_in, &c->pin_in_cap, bytes) == 0) {
    // small batch: through the pinned buffer, no synchronisation here (whatever reads the candidates is ordered behind the copy on the stream)
    if (!c->ev_pin) HIPCHK(hipEventCreateWithFlags(&c->ev_pin, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(c->ev_pin));          // (an upload still reading the buffer: only when nothing synchronised in between)
    memcpy(c->pin_in, Xc, bytes);
    HIPCHK(hipMemcpyAsync(c->Xc.p, c->pin_in, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_pin, c->stream));
    return 0;
  }
  HIPCHK(hipMemcpyAsync(c->Xc.p, Xc, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// One pass of run_predict: candidates [c0, c0 + Cn) of the resident batch, their K* and partial sums in the first Cpad columns of the workspace
struct PredictPass {
  const PredictPlan& p;
  const double* w;           // mean weights: alpha, or those bocf_predict_cov_column hands over
  int flags;                 // BOCF_ADD_NOISE / BOCF_CLIP of the variances
  bool need_grad;
  int c0, Cn, Cpad;
};

static int small_width(int Cn) {                             // the small path's columns: the next power of two
  int nc = 1;
  while (nc < Cn) nc *= 2;
  return nc;
}

// K* of the pass (not for means only) and the partial means per 128-row block (hi and lo planes); for means only, the means themselves
static void predict_cross(bocf_ctx* c, const PredictPass& s) {
  const PredictPlan& p = s.p;
  double* mp = c->meanpart.as<double>();
  PhaseTimer t(c, "cross");
  if (p.kind == PRED_SMALL)                                   // (the matrix-pipe form of the small path)
    launch_cross_small(c->Xs.as<double>(), c->xs_stride, c->N, c->Np, c->d, c->kernel_id, c->hypd.as<KernHyp>(), c->Xc.as<double>(), s.c0, s.Cn,
                       small_width(s.Cn), s.w, c->Kstar.as<double>(), s.Cpad, (long)c->Np * s.Cpad, mp, mp + p.mean_plane, s.Cpad, c->m, c->stream,
                       BOCF_KIDS(c));
  else
    launch_cross_kernel(c->Xs.as<double>(), c->xs_stride, c->N, c->Np, c->d, c->kernel_id, c->hypd.as<KernHyp>(), c->Xc.as<double>(), s.c0, s.Cn,
                        s.Cpad, s.w, c->Kstar.as<double>(), s.Cpad, (long)c->Np * s.Cpad, mp, mp + p.mean_plane, nsplit_for(c->Np, s.Cpad, c->m), c->m,
                        p.kind == PRED_MEAN ? 0 : (p.kind == PRED_F32 ? 2 : 1), c->stream, BOCF_KIDS(c));
  if (!p.mean_with_var)
    launch_finalize_mean(mp, mp + p.mean_plane, p.nrt, s.Cpad, c->hypd.as<KernHyp>(), c->mean.as<double>(), p.ld, s.c0, s.Cn, c->m, c->stream);
}

// variances of the pass from `rows` partial sums of squares per column, and its means from their partials, in one launch
static void predict_finalize(bocf_ctx* c, const PredictPass& s, int rows) {
  double* mp = c->meanpart.as<double>();
  launch_finalize_var(c->sumsq.as<double>(), rows, s.Cpad, c->hypd.as<KernHyp>(), s.flags, c->var.as<double>(), s.p.ld, s.c0, s.Cn, c->m, c->stream, mp,
                      mp + s.p.mean_plane, s.p.nrt, c->mean.as<double>());
}

// n <= 16: GEMV-shaped, R streamed once per product (single-point L-BFGS calls); gradients: W = R V from R^T, then dk/dx
static void contract_small(bocf_ctx* c, const PredictPass& s) {
  const int Np = c->Np, nc = small_width(s.Cn);
  const long strideS = (long)Np * Np;
  launch_gemv_small_t_mfma(c->R.as<double>(), strideS, Np, c->Kstar.as<double>(), s.Cpad, (long)Np * s.Cpad, c->Vs.as<double>(), c->sumsq.as<double>(),
                           s.Cpad, nc, c->m, c->stream);
  predict_finalize(c, s, Np / 16);
  if (!s.need_grad) return;
  launch_gemv_small_n_mfma(c->RT.as<double>(), strideS, Np, c->Vs.as<double>(), c->Ws.as<double>(), nc, c->m, c->stream);
  launch_grad_kernel(c->Xs.as<double>(), c->xs_stride, c->N, Np, c->d, c->kernel_id, c->hypd.as<KernHyp>(), c->Xc.as<double>(), s.c0, s.Cn, s.w,
                     c->Ws.as<double>(), nc, (long)Np * nc, c->dmean.as<double>(), c->dvar.as<double>(), s.p.ld, c->m, c->stream, BOCF_KIDS(c));
}

// gradients need w = Ky^-1 k* = R (R^T k*): V = R^T K* stored this time, then W = R V (R k-major = RT);
// W overwrites the K* buffer (no longer needed: the gradient kernel recomputes dk/dx from the inputs)
static void predict_gradients(bocf_ctx* c, const PredictPass& s) {
  const int Np = c->Np;
  GemmArgs v{};
  v.A = c->R.as<double>(); v.lda = Np; v.strideA = (long)Np * Np;
  v.B = c->Kstar.as<double>(); v.ldb = s.Cpad; v.strideB = (long)Np * s.Cpad;
  v.Cin = nullptr; v.Cout = c->Vbuf.as<double>(); v.ldc = s.Cpad; v.strideC = (long)Np * s.Cpad;
  v.M = Np; v.Ncols = s.Cpad; v.K = Np; v.kb = BOCF_TILE; v.krt = BOCF_TILE; v.rt_desc = 1; v.alpha = 1.0;
  launch_gemm_f64(v, c->m, 0, c->stream);
  GemmArgs w{};
  w.A = c->RT.as<double>(); w.lda = Np; w.strideA = (long)Np * Np;
  w.B = c->Vbuf.as<double>(); w.ldb = s.Cpad; w.strideB = (long)Np * s.Cpad;
  w.Cin = nullptr; w.Cout = c->Kstar.as<double>(); w.ldc = s.Cpad; w.strideC = (long)Np * s.Cpad;
  w.M = Np; w.Ncols = s.Cpad; w.K = Np; w.kb = Np; w.kbeg_rt = BOCF_TILE; w.alpha = 1.0;
  launch_gemm_f64(w, c->m, 0, c->stream);
  launch_grad_kernel(c->Xs.as<double>(), c->xs_stride, c->N, Np, c->d, c->kernel_id, c->hypd.as<KernHyp>(), c->Xc.as<double>(), s.c0, s.Cn, s.w,
                     c->Kstar.as<double>(), s.Cpad, (long)Np * s.Cpad, c->dmean.as<double>(), c->dvar.as<double>(), s.p.ld, c->m, c->stream, BOCF_KIDS(c));
}

// V = R^T K*, only its column sums of squares leave the chip: the three-buffer kernel, whose loop keeps the vector ALU free and skips the zero
// blocks of R's diagonal range (gemm_f64.hip), in the plan's tiling; then the gradients
static void contract_f64(bocf_ctx* c, const PredictPass& s) {
  const int Np = c->Np;
  GemmArgs g{};
  g.A = c->R.as<double>(); g.lda = Np; g.strideA = (long)Np * Np;
  g.B = c->Kstar.as<double>(); g.ldb = s.Cpad; g.strideB = (long)Np * s.Cpad;
  g.M = Np; g.Ncols = s.Cpad; g.K = Np; g.kb = BOCF_TILE; g.krt = BOCF_TILE; g.rt_desc = 1;
  g.swizzle = s.p.tiling(s.Cpad);
  g.vprobe = c->kstar_valu_probe;
  g.prefetch1 = c->prefetch1;
  g.sumsq = c->sumsq.as<double>(); g.strideSumsq = (long)s.p.nrt * s.Cpad;
  g.tile_ctr = c->tile_ctr; g.ncu = c->ncu;
  {
    KernelTimer t(c, s.Cn);
    launch_gemm_f64(g, c->m, 1, c->stream);
  }
  predict_finalize(c, s, s.p.nrt);
  if (s.need_grad) predict_gradients(c, s);
}

// fp32 variance contraction (BASELINE configs[4]): K* stored as fp32 by the cross kernel, R32 = (float) R
static void contract_f32(bocf_ctx* c, const PredictPass& s) {
  const int Np = c->Np;
  GemmArgs32 g{};
  g.A = c->R32.as<float>(); g.lda = Np; g.strideA = (long)Np * Np;
  g.B = c->Kstar.as<float>(); g.ldb = s.Cpad; g.strideB = (long)Np * s.Cpad;
  g.M = Np; g.Ncols = s.Cpad; g.K = Np;
  g.sumsq = c->sumsq.as<double>(); g.strideSumsq = (long)s.p.nrt * s.Cpad;
  g.tile128 = s.p.swizzle == 0;
  {
    KernelTimer t(c, s.Cn);
    launch_gemm_f32_sumsq(g, c->m, c->stream);
  }
  predict_finalize(c, s, s.p.nrt);
}

// int8 (Ozaki): the pass's K* -> digit fragments, then the exact int8 contraction; same partial sums' layout, same finalisation
static void contract_i8(bocf_ctx* c, const PredictPass& s) {
  const int Np = c->Np;
  {
    KernelTimer t(c, s.Cn);
    launch_slice_operand(c->Kstar.as<double>(), s.Cpad, (long)Np * s.Cpad, Np, Np, s.Cpad, c->Ki8e.as<int>(), 0, c->Ki8.p, c->m, c->stream);
    launch_var_i8(c->Ri8.p, c->Ki8.p, Np, s.Cpad, c->Ri8e.as<int>(), c->Ki8e.as<int>(), c->sumsq.as<double>(), (long)s.p.nrt * s.Cpad, c->m, c->stream,
                  c->i8_group);
  }
  predict_finalize(c, s, s.p.nrt);
}

// the int8 operands that last as long as the fit: R's digit fragments and column exponents, and ONE scale per output for every column of K*
// (a stationary kernel never exceeds its variance)
static int prepare_i8(bocf_ctx* c) {
  const int Np = c->Np, m = c->m;
  HIPCHK(hipMemsetAsync(c->Ri8e.p, 0x80, sizeof(int) * (size_t)m * Np, c->stream));      // (below any exponent: the kernel takes maxima)
  launch_col_exponents(c->R.as<double>(), (long)Np * Np, Np, c->Ri8e.as<int>(), m, c->stream);
  launch_slice_operand(c->R.as<double>(), Np, (long)Np * Np, Np, Np, Np, c->Ri8e.as<int>(), Np, c->Ri8.p, m, c->stream);
  std::vector<int> eb(m);
  for (int j = 0; j < m; ++j) eb[j] = c->hyp[j].variance > 0.0 ? ilogb(c->hyp[j].variance) + 1 : 0;
  HIPCHK(hipMemcpyAsync(c->Ki8e.p, eb.data(), sizeof(int) * m, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));             // (eb goes out of scope)
  c->ri8_valid = true;
  return 0;
}

// mean / var of all resident candidates into c->mean / c->var (m, pred_cap); w: the mean weights (nullptr: alpha)
static int run_predict(bocf_ctx* c, int flags, bool need_var, bool need_grad = false, const double* w = nullptr) {
  const int C = c->C;
  if (C == 0) return 0;
  if (c->canned) {           // mean / var were given by the host (bocf_set_posterior): nothing to predict
    if (need_grad) return fail("predict", "a host-given posterior carries no gradients");
    return 0;
  }
  PredictPlanInput in;
  in.C = C; in.N = c->N; in.Np = c->Np; in.m = c->m; in.d = c->d; in.pred_cap = c->pred_cap;
  in.need_var = need_var; in.need_grad = need_grad;
  in.chunk = c->chunk; in.workspace_mb = c->workspace_mb;
  in.small_path = c->small_path; in.predict_f32 = c->predict_f32; in.predict_i8 = c->predict_i8; in.swizzle = c->swizzle;
  const PredictPlan p = plan_predict(in);
  // grow the workspace (R's fp32 copy and int8 operands only where the fit has none yet), then the operands that last for the fit
  DevBuf* bufs[] = {&c->mean, &c->var, &c->acq, &c->Kstar, &c->sumsq, &c->R32, &c->Ki8, &c->Ki8e, &c->Ri8, &c->Ri8e,
                    &c->Vs, &c->Ws, &c->Vbuf, &c->dmean, &c->dvar, &c->dacq, &c->meanpart};
  const size_t bytes[] = {p.mean_bytes, p.var_bytes, p.acq_bytes, p.kstar_bytes, p.sumsq_bytes, c->r32_valid ? 0 : p.r32_bytes, p.ki8_bytes, p.ki8e_bytes,
                          c->ri8_valid ? 0 : p.ri8_bytes, c->ri8_valid ? 0 : p.ri8e_bytes, p.vs_bytes, p.ws_bytes, p.vbuf_bytes, p.dmean_bytes,
                          p.dvar_bytes, p.dacq_bytes, p.meanpart_bytes};
  for (size_t i = 0; i < sizeof(bytes) / sizeof(bytes[0]); ++i)
    if (bufs[i]->ensure(bytes[i])) return -1;
  c->pred_cap = p.ld;
  if (p.kind == PRED_F32 && !c->r32_valid) {
    launch_f64_to_f32(c->R.as<double>(), c->R32.as<float>(), (long)c->m * c->Np * c->Np, c->stream);
    c->r32_valid = true;
  }
  if (p.kind == PRED_I8 && !c->ri8_valid && prepare_i8(c)) return -1;
  // per pass: K* and the mean partials, the contraction, the finalisation
  for (long c0 = 0; c0 < C; c0 += p.chunk) {
    const int Cn = (int)((C - c0) < p.chunk ? (C - c0) : p.chunk);
    const PredictPass s{p, w ? w : c->alpha.as<double>(), flags, need_grad, (int)c0, Cn, round_up(Cn, BOCF_TILE)};
    predict_cross(c, s);
    switch (p.kind) {
      case PRED_MEAN: break;
      case PRED_SMALL: contract_small(c, s); break;
      case PRED_F64: contract_f64(c, s); break;
      case PRED_F32: contract_f32(c, s); break;
      case PRED_I8: contract_i8(c, s); break;
    }
  }
  LAUNCHCHK();
  return 0;
}

// `rows` rows of `len` doubles (device row stride ld) to contiguous host rows, for up to four arrays, then ONE stream synchronisation; small
// totals go through the pinned buffer (a copy into pageable memory is staged and waited for one by one)
struct RowsOut { const double* dev; long ld; int rows; size_t len; double* out; };
static int copy_rows_out_sync(bocf_ctx* c, const RowsOut* v, int n) {
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += v[i].out ? sizeof(double) * v[i].rows * v[i].len : 0;
  const bool pinned = total > 0 && total <= BOCF_PIN_BYTES && pin_ensure(&c->pin_out, &c->pin_out_cap, total) == 0;
  char* pin = static_cast<char*>(c->pin_out);
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    if (!v[i].out) continue;
    for (int j = 0; j < v[i].rows; ++j) {
      void* dst = pinned ? static_cast<void*>(pin + off) : static_cast<void*>(v[i].out + (size_t)j * v[i].len);
      HIPCHK(hipMemcpyAsync(dst, v[i].dev + (size_t)j * v[i].ld, sizeof(double) * v[i].len, hipMemcpyDeviceToHost, c->stream));
      off += sizeof(double) * v[i].len;
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (pinned) {
    off = 0;
    for (int i = 0; i < n; ++i) {
      if (!v[i].out) continue;
      const size_t b = sizeof(double) * v[i].rows * v[i].len;
      memcpy(v[i].out, pin + off, b);
      off += b;
    }
  }
  return 0;
}

extern "C" int bocf_predict(bocf_ctx* c, int flags, double* mean_out, double* var_out) {
  if (!c || !c->fitted || c->canned) return fail("bocf_predict", "model not fitted");
  HIPCHK(hipSetDevice(c->device));
  if (c->C == 0) return 0;
  if (run_predict(c, flags, var_out != nullptr)) return -1;
  const RowsOut v[2] = {{c->mean.as<double>(), c->pred_cap, c->m, (size_t)c->C, mean_out}, {c->var.as<double>(), c->pred_cap, c->m, (size_t)c->C, var_out}};
  return copy_rows_out_sync(c, v, 2);
}

// multi_outputGP.predict(X, full_cov=True): see include/bocf_hip.h.  Three steps on kernels the mean path already has: k0 = K(X, x_0) (the
// cross kernel on the one candidate, stored), w = R (R^T k0) (the two GEMVs of the alpha solve), then the ordinary mean pass over all the
// candidates with w in the place of alpha, and one finalisation kernel.
extern "C" int bocf_predict_cov_column(bocf_ctx* c, int flags, double* cov_out) {
  if (!c || !c->fitted || c->canned) return fail("bocf_predict_cov_column", "model not fitted");
  if (!cov_out) return fail("bocf_predict_cov_column", "null output");
  HIPCHK(hipSetDevice(c->device));
  if (c->C == 0) return 0;
  const int N = c->N, Np = c->Np, m = c->m, d = c->d, nrt = Np / BOCF_TILE;
  const long strideS = (long)Np * Np;
  const size_t plane = (size_t)m * nrt * (Np > BOCF_TILE ? Np : BOCF_TILE);
  if (c->Kstar.ensure(sizeof(double) * (size_t)m * Np * BOCF_TILE) || c->meanpart.ensure(sizeof(double) * 2 * plane) ||
      c->tvec.ensure(sizeof(double) * (size_t)m * Np) || c->dvec.ensure(sizeof(double) * (size_t)m * Np))
    return -1;
  launch_cross_kernel(c->Xs.as<double>(), c->xs_stride, N, Np, d, c->kernel_id, c->hypd.as<KernHyp>(), c->Xc.as<double>(), 0, 1, BOCF_TILE,
                      c->alpha.as<double>(), c->Kstar.as<double>(), BOCF_TILE, (long)Np * BOCF_TILE, c->meanpart.as<double>(),
                      c->meanpart.as<double>() + plane, 1, m, 1, c->stream, BOCF_KIDS(c));
  launch_gemv_small_t(c->R.as<double>(), strideS, Np, c->Kstar.as<double>(), BOCF_TILE, (long)Np * BOCF_TILE, c->tvec.as<double>(), 1, m, c->stream);
  launch_gemv_upper_n(c->R.as<double>(), strideS, Np, c->tvec.as<double>(), c->dvec.as<double>(), m, c->stream);
  if (run_predict(c, 0, false, false, c->dvec.as<double>())) return -1;   // (c->mean then holds K(x_i, X) w + ymean)
  if (c->var.ensure(sizeof(double) * (size_t)m * c->pred_cap)) return -1;
  launch_cov_column(c->Xc.as<double>(), c->C, d, c->kernel_id, c->hypd.as<KernHyp>(), c->mean.as<double>(), c->pred_cap, flags, c->var.as<double>(),
                    c->pred_cap, m, c->stream, BOCF_KIDS(c));
  const RowsOut v[1] = {{c->var.as<double>(), c->pred_cap, m, (size_t)c->C, cov_out}};
  if (copy_rows_out_sync(c, v, 1)) return -1;
  LAUNCHCHK();
  c->have_acq = false;                                       // c->mean / c->var no longer hold the posterior the acquisition kernels read
  return 0;
}

extern "C" int bocf_predict_gradients(bocf_ctx* c, double* dmean_out, double* dvar_out) {
  if (!c || !c->fitted || c->canned) return fail("bocf_predict_gradients", "model not fitted");
  HIPCHK(hipSetDevice(c->device));
  if (c->C == 0) return 0;
  if (run_predict(c, BOCF_ADD_NOISE | BOCF_CLIP, true, true)) return -1;
  const RowsOut v[2] = {{c->dmean.as<double>(), (long)c->pred_cap * c->d, c->m, (size_t)c->C * c->d, dmean_out},
                        {c->dvar.as<double>(), (long)c->pred_cap * c->d, c->m, (size_t)c->C * c->d, dvar_out}};
  if (copy_rows_out_sync(c, v, 2)) return -1;
  LAUNCHCHK();
  return 0;
}

extern "C" int bocf_mean_at_train(bocf_ctx* c, double* out) {
  if (!c || !c->fitted || !out) return fail("bocf_mean_at_train", "model not fitted / null out");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpyAsync(out, c->mu_train.p, sizeof(double) * (size_t)c->m * c->N, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// (uploaded, when given: set when the parameters went up, which costs one stream synchronisation)
int bocf_acq_upload_params(bocf_ctx* c, const double* theta, int theta_dim, const double* prob, int L, const double* params, int nparams,
                           bool* uploaded) {
  if (L < 1 || L > BOCF_MAX_L) return fail("acquisition", "L out of range (1..32)");
  std::vector<double> th((size_t)L * (theta_dim > 0 ? theta_dim : 1), 0.0), pr(L), pa(BOCF_MAX_M, 0.0);
  if (theta_dim > 0) {
    if (!theta) return fail("acquisition", "theta is null");
    memcpy(th.data(), theta, sizeof(double) * (size_t)L * theta_dim);
  }
  for (int l = 0; l < L; ++l) pr[l] = prob ? prob[l] : 1.0 / L;   // maEI.py:50 vs :52
  if (nparams > BOCF_MAX_M) return fail("acquisition", "too many utility parameters");
  for (int i = 0; i < nparams; ++i) pa[i] = params[i];
  // L-BFGS refinement calls the acquisition hundreds of times with the same parameters: upload only on change
  std::vector<double> key;
  key.reserve(th.size() + pr.size() + pa.size() + 2);
  key.push_back((double)L);
  key.push_back((double)theta_dim);
  key.insert(key.end(), th.begin(), th.end());
  key.insert(key.end(), pr.begin(), pr.end());
  key.insert(key.end(), pa.begin(), pa.end());
  if (key.size() == c->last_params.size() && !memcmp(key.data(), c->last_params.data(), sizeof(double) * key.size())) return 0;
  if (c->theta.ensure(sizeof(double) * th.size()) || c->prob.ensure(sizeof(double) * L) || c->best.ensure(sizeof(double) * L) ||
      c->params.ensure(sizeof(double) * BOCF_MAX_M))
    return -1;
  HIPCHK(hipMemcpyAsync(c->theta.p, th.data(), sizeof(double) * th.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->prob.p, pr.data(), sizeof(double) * L, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->params.p, pa.data(), sizeof(double) * BOCF_MAX_M, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->last_params.swap(key);
  c->best_epoch = -1;                                    // the best-so-far values belong to the old parameters
  if (uploaded) *uploaded = true;
  return 0;
}

// two device vectors to the host: small totals through the pinned buffer -- both copies asynchronous, one synchronisation
int bocf_copy_pair_out(bocf_ctx* c, const void* src0, double* out0, size_t b0, const void* src1, double* out1, size_t b1) {
  if (b0 + b1 > 0 && b0 + b1 <= BOCF_PIN_BYTES && pin_ensure(&c->pin_out, &c->pin_out_cap, b0 + b1) == 0) {
    char* pin = static_cast<char*>(c->pin_out);
    if (b0) HIPCHK(hipMemcpyAsync(pin, src0, b0, hipMemcpyDeviceToHost, c->stream));
    if (b1) HIPCHK(hipMemcpyAsync(pin + b0, src1, b1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (b0) memcpy(out0, pin, b0);
    if (b1) memcpy(out1, pin + b0, b1);
    LAUNCHCHK();
    return 0;
  }
  if (out1) HIPCHK(hipMemcpyAsync(out1, src1, b1, hipMemcpyDeviceToHost, c->stream));
  if (out0) HIPCHK(hipMemcpyAsync(out0, src0, b0, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  LAUNCHCHK();
  return 0;
}

int bocf_acq_posterior(bocf_ctx* c, bool grad) { return run_predict(c, BOCF_ADD_NOISE | BOCF_CLIP, true, grad); }
int bocf_eu_posterior(bocf_ctx* c, bool grad) { return run_predict(c, BOCF_CLIP, true, grad); }
int bocf_acq_finish(bocf_ctx* c, double* acq_out, double* dacq_out) {
  c->have_acq = true;
  const size_t b0 = acq_out ? sizeof(double) * (size_t)c->C : 0, b1 = dacq_out ? sizeof(double) * (size_t)c->C * c->d : 0;
  return bocf_copy_pair_out(c, c->acq.p, acq_out, b0, c->dacq.p, dacq_out, b1);
}

typedef void (*AcqLaunch)(const AcqArgs& a, hipStream_t s);

// The reference's h-loop (maEI.py:85-97, uEI_noiseless.py:71-82) runs here: hyper-sample h reads its rows of the posterior
// (bocf_posterior_rows) and adds its share (1/H) to acq (and dacq).
static void acq_over_hyper_samples(bocf_ctx* c, AcqArgs a, int m, int linear, bool grad, AcqLaunch launch) {
  const int H = bocf_acq_hyper_count(c);
  for (int h = 0; h < H; ++h) {
    if (h == 0 || c->best_group < 0) {
      const int gb = bocf_best_group_of(c, h);
      // one hyper-sample: best-so-far depends on the train mean and the parameters only -- the hundreds of acquisition calls of one
      // BO step (batch call + L-BFGS refinements) share it
      const int sig = (linear ? 1 : 0) | (a.util_kind << 1) | (gb << 8);
      const bool cached = H == 1 && c->best_epoch == c->mu_epoch && c->best_sig == sig;
      c->best_epoch = H == 1 ? c->mu_epoch : -1;
      c->best_sig = sig;
      if (!cached)
      launch_best_so_far(c->mu_train.as<double>() + (size_t)gb * m * c->N, c->N, m, linear, a.util_kind, a.theta, a.theta_dim, a.L,
                         a.util_params, c->best.as<double>(), c->stream, a.prog);
    }
    bocf_posterior_rows(c, h, m, grad, &a);
    a.accumulate = h > 0;
    a.scale = 1.0 / H;
    PhaseTimer t(c, "acq");
    launch(a, c->stream);
  }
}

// The part of an acquisition that only enqueues, with the parameters already on the device: the posterior -- with its input gradients
// for the _grad forms -- of every resident candidate and one launch per hyper-sample; c->acq (and c->dacq) hold the result once the stream
// gets there.  Shared by run_acq and, once per pass, by the device-resident refinement (capi_refine.hip; declared in bocf_ctx.h).
int bocf_acq_enqueue(bocf_ctx* c, int m, bool linear, bool grad, int kind, int util_kind, int n_util_params, int theta_dim, int L) {
  const AcqLaunch launch = linear ? (grad ? launch_acq_linear_grad : launch_acq_linear) : (grad ? launch_acq_mc_grad : launch_acq_mc);
  // model.predict (maEI.py:87) / posterior_mean + posterior_variance (uEI_noiseless.py:73-74)
  if (run_predict(c, BOCF_ADD_NOISE | BOCF_CLIP, true, grad)) return -1;
  AcqArgs a{};
  a.ld = c->pred_cap;
  a.m = m; a.C = c->C; a.L = L; a.kind = kind; a.util_kind = util_kind; a.theta_dim = theta_dim > 0 ? theta_dim : 1;
  a.theta = c->theta.as<double>(); a.prob = c->prob.as<double>(); a.best = c->best.as<double>();
  a.util_params = c->params.as<double>(); a.n_util_params = n_util_params; a.acq = c->acq.as<double>();
  a.prog = &c->prog;
  if (!linear) { a.Wt = c->Wt.as<double>(); a.S = c->S_mc; }
  if (grad) { a.ldg = c->pred_cap; a.d = c->d; a.dacq = c->dacq.as<double>(); }
  acq_over_hyper_samples(c, a, m, linear ? 1 : 0, grad, launch);
  c->have_acq = true;
  return 0;
}

// What the four acquisitions share once their arguments are checked: the parameters go up (only when they changed), the enqueue part above,
// values (and gradients) to the host.
// linear: the linear-utility forms (EI / PI of theta^T f); theta_dim as the caller gave it; the Monte-Carlo forms read the resident samples.
static int run_acq(bocf_ctx* c, int m, bool linear, bool grad, int kind, int util_kind, const double* util_params, int n_util_params,
                   const double* theta, int theta_dim, const double* prob, int L, double* acq_out, double* dacq_out) {
  HIPCHK(hipSetDevice(c->device));
  if (c->C == 0) return 0;
  if (bocf_acq_upload_params(c, theta, theta_dim, prob, L, util_params, n_util_params)) return -1;
  if (bocf_acq_enqueue(c, m, linear, grad, kind, util_kind, n_util_params, theta_dim, L)) return -1;
  return bocf_acq_finish(c, acq_out, dacq_out);
}

extern "C" int bocf_acq_linear(bocf_ctx* c, int kind, const double* theta, const double* prob, int L, double* acq_out) {
  const int m = bocf_acq_linear_check("bocf_acq_linear", bocf_call_state(c), kind);
  if (m < 0) return -1;
  return run_acq(c, m, true, false, kind, BOCF_UTIL_LINEAR, nullptr, 0, theta, m, prob, L, acq_out, nullptr);
}

extern "C" int bocf_acq_linear_grad(bocf_ctx* c, int kind, const double* theta, const double* prob, int L, double* acq_out,
                                    double* dacq_out) {
  const int m = bocf_acq_linear_check("bocf_acq_linear_grad", bocf_call_state(c), kind);
  if (m < 0) return -1;
  return run_acq(c, m, true, true, kind, BOCF_UTIL_LINEAR, nullptr, 0, theta, m, prob, L, acq_out, dacq_out);
}

extern "C" int bocf_set_mc_samples(bocf_ctx* c, const double* W, int S) {
  const int m = bocf_set_samples_check("bocf_set_mc_samples", bocf_call_state(c), W && S >= 1);     // W is (S, outputs per hyper-sample)
  if (m < 0) return -1;
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> wt((size_t)m * S);
  for (int s = 0; s < S; ++s)
    for (int j = 0; j < m; ++j) wt[(long)j * S + s] = W[(long)s * m + j];
  if (c->Wt.ensure(sizeof(double) * wt.size())) return -1;
  HIPCHK(hipMemcpyAsync(c->Wt.p, wt.data(), sizeof(double) * wt.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->S_mc = S;
  return 0;
}

extern "C" int bocf_acq_mc(bocf_ctx* c, int kind, int util_kind, const double* util_params, int n_util_params, const double* theta,
                           int theta_dim, const double* prob, int L, double* acq_out) {
  static const char* who = "bocf_acq_mc";
  bool program;
  const int m = bocf_acq_mc_check(who, bocf_call_state(c), false, kind, UtilArgs{util_kind, util_params, n_util_params, theta, theta_dim, prob, L}, &program);
  if (m < 0 || (program && bocf_check_resident_program(c, who, m, theta_dim, n_util_params))) return -1;
  return run_acq(c, m, false, false, kind, util_kind, util_params, n_util_params, theta, theta_dim, prob, L, acq_out, nullptr);
}

extern "C" int bocf_acq_mc_grad(bocf_ctx* c, int util_kind, const double* util_params, int n_util_params, const double* theta,
                                int theta_dim, const double* prob, int L, double* acq_out, double* dacq_out) {
  static const char* who = "bocf_acq_mc_grad";
  const CallState st = bocf_call_state(c);
  bool program;
  const int m = bocf_acq_mc_check(who, st, true, BOCF_ACQ_EI, UtilArgs{util_kind, util_params, n_util_params, theta, theta_dim, prob, L}, &program);
  if (m < 0 || (program && bocf_check_resident_program(c, who, m, theta_dim, n_util_params)) || bocf_check_grad_dim(who, st, true, true)) return -1;
  return run_acq(c, m, false, true, BOCF_ACQ_EI, util_kind, util_params, n_util_params, theta, theta_dim, prob, L, acq_out, dacq_out);
}

// one device word to the host through the pinned buffer: ONE stream synchronisation
int bocf_copy_word_out(bocf_ctx* c, const int* dev, int* out) {
  if (pin_ensure(&c->pin_out, &c->pin_out_cap, sizeof(int)) == 0) {
    HIPCHK(hipMemcpyAsync(c->pin_out, dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = *static_cast<const int*>(c->pin_out);
    return 0;
  }
  HIPCHK(hipMemcpyAsync(out, dev, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int bocf_set_eu_samples(bocf_ctx* c, const double* Z, int L, int S) {
  const int m = bocf_set_samples_check("bocf_set_eu_samples", bocf_call_state(c), Z && L >= 1 && S >= 1);     // Z is (L, S, outputs per hyper-sample)
  if (m < 0) return -1;
  HIPCHK(hipSetDevice(c->device));
  std::vector<double> zt((size_t)L * m * S);               // -> (L, m, S): lanes of a wave read consecutive samples
  for (int l = 0; l < L; ++l)
    for (int s = 0; s < S; ++s)
      for (int j = 0; j < m; ++j) zt[((size_t)l * m + j) * S + s] = Z[((size_t)l * S + s) * m + j];
  if (c->eu_Z.ensure(sizeof(double) * zt.size())) return -1;
  HIPCHK(hipMemcpyAsync(c->eu_Z.p, zt.data(), sizeof(double) * zt.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->eu_L = L;
  c->eu_S = S;
  c->eu_m = m;
  return 0;
}

extern "C" int bocf_expected_utility(bocf_ctx* c, int mode, int util_kind, const double* util_params, int n_util_params, const double* theta,
                                     int theta_dim, int L, const int* row_param, int n_hyps, double* val_out, double* grad_out) {
  const char* me = "bocf_expected_utility";
  const CallState st = bocf_call_state(c);
  const UtilArgs u{util_kind, util_params, n_util_params, theta, theta_dim, nullptr, L};
  bool program;
  const int m = bocf_eu_check_utility(me, st, mode, u, &program);
  if (m < 0 || (program && bocf_check_resident_program(c, me, m, theta_dim, n_util_params))) return -1;
  const int rc = bocf_eu_check_call(me, st, mode, u, m, row_param, n_hyps, val_out, grad_out != nullptr);
  if (rc) return rc < 0 ? -1 : 0;
  HIPCHK(hipSetDevice(c->device));
  const int C = c->C, d = c->d;
  // theta | params | rows in one pinned staging buffer (free again once the previous call's copy is done)
  const size_t bt = sizeof(double) * (size_t)L * theta_dim, bp = sizeof(double) * BOCF_MAX_M, br = sizeof(int) * (size_t)C;
  if (c->eu_theta.ensure(bt + bp) || c->eu_rows.ensure(br) || c->eu_val.ensure(sizeof(double) * (size_t)C) ||
      (grad_out && c->eu_grad.ensure(sizeof(double) * (size_t)C * d)))
    return -1;
  if (c->ev_eu_pin) HIPCHK(hipEventSynchronize(c->ev_eu_pin));       // (only pending when an earlier call failed before its synchronisation)
  else HIPCHK(hipEventCreateWithFlags(&c->ev_eu_pin, hipEventDisableTiming));
  const bool pinned = pin_ensure(&c->eu_pin, &c->eu_pin_cap, bt + bp + br) == 0;
  std::vector<char> pageable;
  char* stage;
  if (pinned) {
    stage = static_cast<char*>(c->eu_pin);
  } else {
    pageable.resize(bt + bp + br);
    stage = pageable.data();
  }
  memcpy(stage, theta, bt);
  memset(stage + bt, 0, bp);
  if (n_util_params > 0) memcpy(stage + bt, util_params, sizeof(double) * n_util_params);
  memcpy(stage + bt + bp, row_param, br);
  HIPCHK(hipMemcpyAsync(c->eu_theta.p, stage, bt + bp, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->eu_rows.p, stage + bt + bp, br, hipMemcpyHostToDevice, c->stream));
  if (pinned) HIPCHK(hipEventRecord(c->ev_eu_pin, c->stream));
  else HIPCHK(hipStreamSynchronize(c->stream));
  // predict_noiseless (gpmodel.py:151-159): no likelihood noise, clipped; the mean form needs no variance unless gradients are asked for
  const bool need_grad = grad_out != nullptr;
  if (run_predict(c, BOCF_CLIP, mode != BOCF_EU_MEAN || need_grad, need_grad)) return -1;
  const int H = c->hyper_samples;
  const int nh = H == 1 ? 1 : n_hyps;
  EuArgs a{};
  a.ld = c->pred_cap; a.ldg = c->pred_cap; a.d = d;
  a.m = m; a.C = C; a.mode = mode; a.util_kind = util_kind; a.theta_dim = theta_dim;
  a.theta = c->eu_theta.as<double>(); a.util_params = c->eu_theta.as<double>() + (size_t)L * theta_dim;
  a.rows = c->eu_rows.as<int>(); a.Zt = c->eu_Z.as<double>(); a.S = c->eu_S;
  a.val = c->eu_val.as<double>(); a.grad = need_grad ? c->eu_grad.as<double>() : nullptr;
  a.scale = H == 1 ? (double)n_hyps : 1.0;
  a.prog = &c->prog;
  for (int h = 0; h < nh; ++h) {
    bocf_posterior_rows(c, h, m, need_grad, &a);
    a.accumulate = h > 0;
    PhaseTimer t(c, "eu");
    launch_eu(a, c->stream);
  }
  return bocf_copy_pair_out(c, c->eu_val.p, val_out, sizeof(double) * (size_t)C, c->eu_grad.p, grad_out, need_grad ? sizeof(double) * (size_t)C * d : 0);
}

extern "C" int bocf_select_topk(bocf_ctx* c, int k, long long* idx_out, double* val_out) {
  if (!c || !c->have_acq) return fail("bocf_select_topk", "no acquisition vector on the device");
  if (k < 1 || k > 64 || !idx_out) return fail("bocf_select_topk", "k out of range (1..64) / null out");
  HIPCHK(hipSetDevice(c->device));
  const int nb = topk_num_blocks(c->C);
  if (c->blk_idx.ensure(sizeof(long long) * (size_t)nb * k) || c->blk_val.ensure(sizeof(double) * (size_t)nb * k) ||
      c->out_idx.ensure(8 * (size_t)128))                  // [0, k): indices, [k, 2k): values (k <= 64)
    return -1;
  {
    PhaseTimer t(c, "topk");
    launch_topk(c->acq.as<double>(), c->C, k, c->blk_idx.as<long long>(), c->blk_val.as<double>(), c->out_idx.as<long long>(),
                reinterpret_cast<double*>(c->out_idx.as<long long>() + k), c->stream);
  }
  // (indices and values sit next to each other in one allocation: ONE device-to-host copy)
  long long host[128];
  HIPCHK(hipMemcpyAsync(host, c->out_idx.p, 8 * (size_t)(val_out ? 2 * k : k), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  memcpy(idx_out, host, sizeof(long long) * k);
  if (val_out) memcpy(val_out, host + k, sizeof(double) * k);
  LAUNCHCHK();
  return 0;
}

extern "C" int bocf_profile_read(bocf_ctx* c, double* ms_out, long long* launches_out, double* flops_out, int reset) {
  if (!c) return fail("bocf_profile_read", "null ctx");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  double ms = 0.0;
  for (auto& pr : c->events) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, pr.first, pr.second));
    ms += t;
  }
  if (ms_out) *ms_out = ms;
  if (launches_out) *launches_out = (long long)c->events.size();
  if (flops_out) *flops_out = c->prof_flops;
  if (reset) {
    drop_events(c);
    c->prof_flops = 0.0;
  }
  return 0;
}

extern "C" int bocf_get_stat(bocf_ctx* c, const char* name, long long* value_out) {
  if (!c || !name || !value_out) return fail("bocf_get_stat", "null argument");
  if (!strcmp(name, "sched_timeouts")) *value_out = c->sched_timeouts;
  else if (!strcmp(name, "gated_schedules_off")) *value_out = c->gated_off;
  else if (!strcmp(name, "last_schedule")) *value_out = c->last_schedule;
  else if (!strcmp(name, "early_inverse")) *value_out = c->early_inverse_started;
  else if (!strcmp(name, "cu_masks_ok")) *value_out = c->cu_masks_ok;
  else if (!strcmp(name, "comm_world")) *value_out = c->comm ? c->world : 0;
  else if (!strcmp(name, "kstar_workspace_bytes")) *value_out = (long long)c->Kstar.cap;
  else return fail("bocf_get_stat", "unknown statistic");
  return 0;
}

extern "C" int bocf_profile_phase(bocf_ctx* c, const char* name, double* ms_out, long long* count_out, int reset) {
  if (!c || !name) return fail("bocf_profile_phase", "null argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  double ms = 0.0;
  long long n = 0;
  auto it = c->phases.find(name);
  if (it != c->phases.end()) {
    for (auto& pr : it->second) {
      float t = 0.f;
      HIPCHK(hipEventElapsedTime(&t, pr.first, pr.second));
      ms += t;
      ++n;
    }
    if (reset) {
      for (auto& pr : it->second) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
      }
      c->phases.erase(it);
    }
  }
  if (ms_out) *ms_out = ms;
  if (count_out) *count_out = n;
  return 0;
}
