// How one predict pass runs (capi.hip: run_predict), decided before anything is enqueued: plan_predict reads the model's shape, what the
// caller asks for and the options, and returns the contraction kind, the chunking, the variance-GEMM tiling and the bytes of every workspace
// buffer the pass grows.  Host-only and pure (no HIP): the CPU suite drives it (tests/test_predict_plan_cpu.py).
#pragma once

#include <cstddef>

#define PLAN_TILE 128              // == BOCF_TILE: panel width, every operand is padded to it
#define PLAN_SMALL_N 16            // == BOCF_SMALL_N: candidates of the GEMV-shaped path
#define PLAN_I8_SLICES 6           // == BOCF_I8_SLICES: radix-254 digits per operand column

// digit fragments of an Np x ncols operand (ncols a multiple of 16), m matrices (gemm_i8.hip's layout)
inline size_t i8_operand_bytes(int Np, int ncols, int m) { return (size_t)m * PLAN_I8_SLICES * (size_t)(Np / 64) * (size_t)(ncols / 16) * 1024; }

// what the decision reads: the resident model and candidates, the request, the options (bocf_set_option)
struct PredictPlanInput {
  int C = 0, N = 0, Np = 0, m = 0, d = 0;   // candidates, observations (padded), fitted outputs, input dimension
  int pred_cap = 0;                  // columns already allocated in mean / var / acq
  bool need_var = false, need_grad = false;   // (gradients imply variances)
  long chunk = 65536;                // option "chunk": candidates per pass
  long workspace_mb = 24576;         // option "workspace_mb": cap of the per-pass K* (and, for gradients, V) workspace
  bool small_path = true, predict_f32 = false, predict_i8 = false;
  int swizzle = -1;                  // option "swizzle": variance-GEMM tiling, -1 = by size
};

enum PredictKind {
  PRED_MEAN = 0,   // means only: the cross kernel's partial sums, one finalisation
  PRED_SMALL = 1,  // <= 16 candidates: GEMV-shaped products on the matrix pipe
  PRED_F64 = 2,    // V = R^T K* in fp64, only its column sums of squares leave the chip (and the gradient tail)
  PRED_F32 = 3,    // the same contraction in fp32 (option predict_f32)
  PRED_I8 = 4,     // the same contraction in exact int8 digit products (option predict_i8)
};

struct PredictPlan {
  PredictKind kind = PRED_MEAN;
  long chunk = 0;                    // candidates per pass, after the workspace cap
  int chunkpad = 0;                  // columns of the per-pass workspace
  int ld = 0;                        // columns of mean / var / acq (>= pred_cap)
  int nrt = 0;                       // 128-row tiles of R
  bool mean_with_var = false;        // the variance finalisation also finishes the means
  int swizzle = -1;
  size_t mean_plane = 0;             // doubles per plane (hi, lo) of the partial means
  // bytes each buffer is grown to (0: the pass does not touch it); R32 and Ri8 / Ri8e only when no valid copy of R's operand exists
  size_t mean_bytes = 0, var_bytes = 0, acq_bytes = 0, meanpart_bytes = 0;
  size_t kstar_bytes = 0, sumsq_bytes = 0, vs_bytes = 0, ws_bytes = 0, vbuf_bytes = 0;
  size_t dmean_bytes = 0, dvar_bytes = 0, dacq_bytes = 0;
  size_t r32_bytes = 0, ri8_bytes = 0, ri8e_bytes = 0, ki8_bytes = 0, ki8e_bytes = 0;

  // variance-GEMM tiling of a pass of n columns: 256-row tiles (the three-buffer kernel, gemm_f64.hip) from 2048 candidates per pass --
  // 0.93 of the fp64 MFMA peak against 0.83 for the 128-row kernel at N = 4096, 0.81 against 0.77 at config 2 (N = 1024, 8192 candidates);
  // below that its fewer, larger workgroups leave CUs idle (N = 1024, C = 1024: 0.49 against 0.40 ms for the 128-row kernel).  Padded sizes
  // that are not a multiple of 256 fall back in the launcher.  Option "swizzle" = 0 / 256 / 257 / 258 forces a tiling.
  int tiling(int n) const { return swizzle < 0 ? (n >= 2048 ? 258 : 0) : swizzle; }
};

inline PredictPlan plan_predict(const PredictPlanInput& in) {
  const int Np = in.Np, m = in.m, C = in.C;
  const auto rup = [](int x) { return (x + PLAN_TILE - 1) / PLAN_TILE * PLAN_TILE; };
  PredictPlan p;
  p.nrt = Np / PLAN_TILE;
  p.swizzle = in.swizzle;
  // candidates per pass: option "chunk", lowered so that the K* (and, for gradients, V) workspace of ALL fitted outputs (hyper-samples x
  // outputs) stays inside option "workspace_mb"; results do not depend on the chunking
  const double per_col = (double)m * Np * sizeof(double) * (in.need_grad ? 2.0 : 1.0);
  long fit_cols = (long)((double)in.workspace_mb * 1048576.0 / per_col);
  fit_cols = fit_cols / PLAN_TILE * PLAN_TILE;
  if (fit_cols < PLAN_TILE) fit_cols = PLAN_TILE;
  p.chunk = in.chunk > fit_cols ? fit_cols : in.chunk;
  p.chunkpad = (int)(C < p.chunk ? rup(C) : p.chunk);
  p.ld = in.pred_cap < C ? rup(C) : in.pred_cap;
  // the contraction: the small path from 16 candidates down; fp32 (BASELINE configs[4]) and int8 for variances only -- the mean (whose
  // alpha-weighted sum cancels catastrophically in fp32) and the gradient path (which needs V itself) stay in fp64; int8 up to
  // Np = 16384 (int32 group sums: 6 x 127^2 x N < 2^31)
  const bool small = C <= PLAN_SMALL_N && in.small_path;
  const bool f32 = in.predict_f32 && in.need_var && !in.need_grad && !small;
  const bool i8 = in.predict_i8 && in.need_var && !in.need_grad && !small && !f32 && Np <= 16384;
  p.kind = !in.need_var ? PRED_MEAN : small ? PRED_SMALL : f32 ? PRED_F32 : i8 ? PRED_I8 : PRED_F64;
  p.mean_with_var = in.need_var;
  // workspace
  p.mean_bytes = p.var_bytes = sizeof(double) * (size_t)m * p.ld;
  p.acq_bytes = sizeof(double) * (size_t)p.ld;
  p.mean_plane = (size_t)m * p.nrt * (p.chunkpad > Np ? p.chunkpad : Np);
  p.meanpart_bytes = sizeof(double) * 2 * p.mean_plane;
  if (in.need_var) {
    p.kstar_bytes = sizeof(double) * (size_t)m * Np * p.chunkpad;   // (fp32: the same bytes)
    // (<= 16 candidates keep one partial per 16-row tile, whichever path runs)
    p.sumsq_bytes = sizeof(double) * (size_t)m * (C <= PLAN_SMALL_N ? Np / 16 : p.nrt) * p.chunkpad;
  }
  if (p.kind == PRED_SMALL) p.vs_bytes = p.ws_bytes = sizeof(double) * (size_t)m * Np * PLAN_SMALL_N;
  if (in.need_grad) {
    if (!small) p.vbuf_bytes = sizeof(double) * (size_t)m * Np * p.chunkpad;
    p.dmean_bytes = p.dvar_bytes = sizeof(double) * (size_t)m * p.ld * in.d;
    p.dacq_bytes = sizeof(double) * (size_t)p.ld * in.d;
  }
  if (f32) p.r32_bytes = sizeof(float) * (size_t)m * Np * Np;
  if (i8) {
    p.ki8_bytes = i8_operand_bytes(Np, p.chunkpad, m);
    p.ki8e_bytes = sizeof(int) * (size_t)m;
    p.ri8_bytes = i8_operand_bytes(Np, Np, m);
    p.ri8e_bytes = sizeof(int) * (size_t)m * Np;
  }
  return p;
}
