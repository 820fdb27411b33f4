// Probes-only entries that run ONE launcher of the matrix-product kernels on operands a test supplies from the host (compiled only with
// -DBOCF_PROBES: the product library gets an empty object and exports none of these names).  One entry per launcher -- launch_gemm_f64,
// launch_gemm_f32_sumsq, launch_var_i8 (with launch_col_exponents / launch_slice_operand), launch_tile128 -- each taking a plain C
// descriptor: host buffers with their lengths, the origin of the operand inside each buffer (a sub-matrix of a larger allocation, as the
// factorization addresses its panels), and every scalar the launcher reads.  An entry creates its own stream on device 0, copies the
// buffers up, launches `repeat` times (every launch starts from the host's C / sums; only the tile-queue counters carry over), synchronises
// and copies everything back.  Before anything is launched the descriptor is checked on the host: every address a kernel of that launcher
// can touch (full K rows of each operand, as the callers allocate them) lies inside the buffers, or the entry fails without a launch.
// tests/gemm_ref.py states the same contract in NumPy; tests/test_gpu_gemm_kernels.py compares the two.
#ifdef BOCF_PROBES
#include "bocf_ctx.h"
#include "refine_step.h"

#include <cmath>
#include <cstdio>

namespace {

struct ProbeScope {                                      // the entry's stream and device buffers, released on every return path
  hipStream_t s = nullptr;
  std::vector<void*> bufs;
  ~ProbeScope() {
    for (void* p : bufs) (void)hipFree(p);
    if (s) (void)hipStreamDestroy(s);
  }
  int open() {
    HIPCHK(hipSetDevice(0));
    HIPCHK(hipStreamCreate(&s));
    return 0;
  }
  template <typename T>
  int alloc(T** p, size_t count) {
    void* q = nullptr;
    HIPCHK(hipMalloc(&q, sizeof(T) * (count ? count : 1)));
    bufs.push_back(q);
    *p = static_cast<T*>(q);
    return 0;
  }
  template <typename T>
  int up(T* dev, const T* host, size_t count) {
    if (count) HIPCHK(hipMemcpyAsync(dev, host, sizeof(T) * count, hipMemcpyHostToDevice, s));
    return 0;
  }
  template <typename T>
  int down(T* host, const T* dev, size_t count) {
    if (count) HIPCHK(hipMemcpyAsync(host, dev, sizeof(T) * count, hipMemcpyDeviceToHost, s));
    return 0;
  }
  int finish() {
    HIPCHK(hipStreamSynchronize(s));
    return bocf_launch_status() ? -1 : 0;
  }
};

int probe_fail(const char* who, const char* fmt, long a = 0, long b = 0, long c = 0) {
  char text[256];
  snprintf(text, sizeof(text), fmt, a, b, c);
  return bocf_fail(who, text);
}

// largest batch offset of a one- or two-level batch (z = z2 * batch1 + z1)
long batch_span(int batch, int batch1, long s1, long s2) {
  if (batch1 > 0) {
    const int z1 = (batch < batch1 ? batch : batch1) - 1, z2 = (batch - 1) / batch1;
    return (long)z1 * s1 + (long)z2 * s2;
  }
  return (long)(batch - 1) * s1;
}

// rows x width elements with leading dimension ld at origin off (+ up to span) inside a buffer of len elements; `align`: elements per vector access
int check_extent(const char* who, const char* name, const void* host, long len, long off, long span, long rows, long ld, long width, long align) {
  if (!host || len <= 0) return probe_fail(who, (std::string(name) + ": null buffer").c_str());
  if (off < 0 || span < 0 || ld < width || rows <= 0 || width <= 0) return probe_fail(who, (std::string(name) + ": bad origin, stride or leading dimension").c_str());
  if (off % align || ld % align || span % align) return probe_fail(who, (std::string(name) + ": origin, leading dimension and strides must be multiples of %ld elements").c_str(), align);
  const long last = off + span + (rows - 1) * ld + width;
  if (last > len) return probe_fail(who, (std::string(name) + ": the operand ends at element %ld of a buffer of %ld").c_str(), last, len);
  return 0;
}

}  // namespace

extern "C" {

struct bocf_probe_gemm_f64_desc {
  double* A; long lenA, offA;
  double* B; long lenB, offB;                            // (b_alias_c: B is ignored, offB is an origin inside C)
  double* C; long lenC, offC;                            // in and out
  double* sumsq; long lenS, offS;                        // in and out
  long lda, strideA, strideA2;
  long ldb, strideB, strideB2;
  long ldc, strideC, strideC2;
  long strideSumsq;
  double alpha, beta;
  int M, Ncols, K, kb, krt, kct, kbeg_rt, kbeg_ct, batch1, upper_only, rt_desc, ct_desc, swizzle, prefetch1, stagger, no_x3, vprobe;
  int batch, epilogue;
  int has_cin;                                           // Cin = Cout (read-modify-write) or nullptr
  int b_alias_c;                                         // the in-place panel solve: B is a sub-matrix of Cout's buffer
  int use_queue, ncu;                                    // tile queue of the 256-row variance kernel: the entry owns the two counters
  int repeat;
  int ctr[2];                                            // out: the counters after the last launch
};

int bocf_probe_gemm_f64(bocf_probe_gemm_f64_desc* d) {
  const char* who = "bocf_probe_gemm_f64";
  if (!d) return probe_fail(who, "null descriptor");
  if (d->M <= 0 || d->Ncols <= 0 || d->K <= 0 || d->M % 128 || d->Ncols % 128 || d->K % 16) return probe_fail(who, "M, Ncols must be multiples of 128 and K of 16");
  if (d->kb < 0 || d->krt < 0 || d->kct < 0 || d->kbeg_rt < 0 || d->kbeg_ct < 0 || d->kb % 16 || d->krt % 16 || d->kct % 16 || d->kbeg_rt % 16 || d->kbeg_ct % 16)
    return probe_fail(who, "the contraction-range fields must be non-negative multiples of 16");
  if (d->batch <= 0 || d->batch1 < 0 || d->repeat <= 0) return probe_fail(who, "batch and repeat must be positive");
  if (d->epilogue != 0 && d->epilogue != 1 && d->epilogue != 3) return probe_fail(who, "epilogue is 0, 1 or 3");
  if (d->epilogue == 3 && d->M != d->Ncols) return probe_fail(who, "epilogue 3 is the square upper-only grid");
  if (d->use_queue && d->ncu <= 0) return probe_fail(who, "the tile queue needs ncu > 0");
  if (d->strideA < 0 || d->strideB < 0 || d->strideC < 0 || d->strideA2 < 0 || d->strideB2 < 0 || d->strideC2 < 0 || d->strideSumsq < 0) return probe_fail(who, "negative stride");
  const long spanA = batch_span(d->batch, d->batch1, d->strideA, d->strideA2), spanB = batch_span(d->batch, d->batch1, d->strideB, d->strideB2);
  const long spanC = batch_span(d->batch, d->batch1, d->strideC, d->strideC2);
  const bool store = d->epilogue != 1;
  if (check_extent(who, "A", d->A, d->lenA, d->offA, spanA, d->K, d->lda, d->M, 2)) return -1;
  if (d->b_alias_c) {
    if (!store) return probe_fail(who, "B can alias Cout only with a store epilogue");
    if (check_extent(who, "B (in C)", d->C, d->lenC, d->offB, spanB, d->K, d->ldb, d->Ncols, 2)) return -1;
  } else if (check_extent(who, "B", d->B, d->lenB, d->offB, spanB, d->K, d->ldb, d->Ncols, 2)) {
    return -1;
  }
  if (store && check_extent(who, "C", d->C, d->lenC, d->offC, spanC, d->M, d->ldc, d->Ncols, 2)) return -1;
  if (!store && check_extent(who, "sumsq", d->sumsq, d->lenS, d->offS, (long)(d->batch - 1) * d->strideSumsq, d->M / 128, d->Ncols, d->Ncols, 1)) return -1;

  ProbeScope sc;
  if (sc.open()) return -1;
  double *dA = nullptr, *dB = nullptr, *dC = nullptr, *dS = nullptr;
  int* dctr = nullptr;
  const size_t nA = (size_t)d->lenA, nB = d->b_alias_c ? 0 : (size_t)d->lenB, nC = d->C ? (size_t)d->lenC : 0, nS = d->sumsq ? (size_t)d->lenS : 0;
  if (sc.alloc(&dA, nA) || sc.alloc(&dB, nB) || sc.alloc(&dC, nC) || sc.alloc(&dS, nS) || sc.alloc(&dctr, 2)) return -1;
  if (sc.up(dA, d->A, nA) || sc.up(dB, d->B, nB)) return -1;
  HIPCHK(hipMemsetAsync(dctr, 0, 2 * sizeof(int), sc.s));                  // once: a launch must leave the counters as the next one needs them
  GemmArgs g{};
  g.A = dA + d->offA; g.lda = d->lda; g.strideA = d->strideA; g.strideA2 = d->strideA2;
  g.B = (d->b_alias_c ? dC : dB) + d->offB; g.ldb = d->ldb; g.strideB = d->strideB; g.strideB2 = d->strideB2;
  g.Cout = store ? dC + d->offC : nullptr; g.Cin = store && d->has_cin ? dC + d->offC : nullptr;
  g.ldc = d->ldc; g.strideC = d->strideC; g.strideC2 = d->strideC2;
  g.M = d->M; g.Ncols = d->Ncols; g.K = d->K; g.kb = d->kb; g.krt = d->krt; g.kct = d->kct; g.kbeg_rt = d->kbeg_rt; g.kbeg_ct = d->kbeg_ct;
  g.batch1 = d->batch1; g.upper_only = d->upper_only; g.rt_desc = d->rt_desc; g.ct_desc = d->ct_desc; g.swizzle = d->swizzle;
  g.prefetch1 = d->prefetch1; g.stagger = d->stagger; g.no_x3 = d->no_x3; g.vprobe = d->vprobe;
  g.alpha = d->alpha; g.beta = d->beta;
  g.sumsq = store ? nullptr : dS + d->offS; g.strideSumsq = d->strideSumsq;
  g.tile_ctr = d->use_queue ? dctr : nullptr; g.ncu = d->use_queue ? d->ncu : 0;
  for (int it = 0; it < d->repeat; ++it) {
    if (sc.up(dC, d->C, nC) || sc.up(dS, d->sumsq, nS)) return -1;
    launch_gemm_f64(g, d->batch, d->epilogue, sc.s);
  }
  if (sc.down(d->A, dA, nA) || sc.down(d->B, dB, nB) || sc.down(d->C, dC, nC) || sc.down(d->sumsq, dS, nS) || sc.down(d->ctr, dctr, 2)) return -1;
  return sc.finish();
}

struct bocf_probe_gemm_f32_desc {
  double* A; long lenA, offA;                            // host doubles: the entry converts whole buffers with launch_f64_to_f32
  double* B; long lenB, offB;
  double* sumsq; long lenS, offS;                        // in and out
  long lda, strideA, ldb, strideB, strideSumsq;
  int M, Ncols, K, tile128, batch, repeat;
};

int bocf_probe_gemm_f32(bocf_probe_gemm_f32_desc* d) {
  const char* who = "bocf_probe_gemm_f32";
  if (!d) return probe_fail(who, "null descriptor");
  if (d->M <= 0 || d->Ncols <= 0 || d->K <= 0 || d->M % 128 || d->Ncols % 128 || d->K % 32) return probe_fail(who, "M, Ncols must be multiples of 128 and K of 32");
  if (d->batch <= 0 || d->repeat <= 0) return probe_fail(who, "batch and repeat must be positive");
  if (d->strideA < 0 || d->strideB < 0 || d->strideSumsq < 0) return probe_fail(who, "negative stride");
  if (check_extent(who, "A", d->A, d->lenA, d->offA, (long)(d->batch - 1) * d->strideA, d->K, d->lda, d->M, 4)) return -1;
  if (check_extent(who, "B", d->B, d->lenB, d->offB, (long)(d->batch - 1) * d->strideB, d->K, d->ldb, d->Ncols, 4)) return -1;
  if (check_extent(who, "sumsq", d->sumsq, d->lenS, d->offS, (long)(d->batch - 1) * d->strideSumsq, d->M / 128, d->Ncols, d->Ncols, 1)) return -1;
  ProbeScope sc;
  if (sc.open()) return -1;
  double *dA = nullptr, *dB = nullptr, *dS = nullptr;
  float *fA = nullptr, *fB = nullptr;
  const size_t nA = (size_t)d->lenA, nB = (size_t)d->lenB, nS = (size_t)d->lenS;
  if (sc.alloc(&dA, nA) || sc.alloc(&dB, nB) || sc.alloc(&dS, nS) || sc.alloc(&fA, nA) || sc.alloc(&fB, nB)) return -1;
  if (sc.up(dA, d->A, nA) || sc.up(dB, d->B, nB)) return -1;
  launch_f64_to_f32(dA, fA, (long)nA, sc.s);
  launch_f64_to_f32(dB, fB, (long)nB, sc.s);
  GemmArgs32 g{};
  g.A = fA + d->offA; g.lda = d->lda; g.strideA = d->strideA;
  g.B = fB + d->offB; g.ldb = d->ldb; g.strideB = d->strideB;
  g.M = d->M; g.Ncols = d->Ncols; g.K = d->K;
  g.sumsq = dS + d->offS; g.strideSumsq = d->strideSumsq;
  g.tile128 = d->tile128;
  for (int it = 0; it < d->repeat; ++it) {
    if (sc.up(dS, d->sumsq, nS)) return -1;
    launch_gemm_f32_sumsq(g, d->batch, sc.s);
  }
  if (sc.down(d->sumsq, dS, nS)) return -1;
  return sc.finish();
}

struct bocf_probe_var_i8_desc {
  double* A; long lenA;                                  // m matrices Np x Np (k-major, leading dimension Np), strideA apart
  double* B; long lenB, offB;                            // m matrices Np x ncols, leading dimension ldb
  double* sumsq; long lenS, offS;                        // in and out: [m][Np / 128][ncols]
  int* eA;                                               // out: (m, Np) column exponents of A as launch_col_exponents left them
  int* eB;                                               // in: (m) one exponent per matrix of B
  long strideA, ldb, strideB, strideSumsq;
  int Np, ncols, m, i8_group, repeat;
};

int bocf_probe_var_i8(bocf_probe_var_i8_desc* d) {
  const char* who = "bocf_probe_var_i8";
  if (!d || !d->eA || !d->eB) return probe_fail(who, "null descriptor or exponent array");
  if (d->Np <= 0 || d->ncols <= 0 || d->Np % 128 || d->ncols % 64) return probe_fail(who, "Np must be a multiple of 128 and ncols of 64");
  if (d->m <= 0 || d->repeat <= 0) return probe_fail(who, "m and repeat must be positive");
  if (d->strideA < 0 || d->strideB < 0 || d->strideSumsq < 0) return probe_fail(who, "negative stride");
  if (check_extent(who, "A", d->A, d->lenA, 0, (long)(d->m - 1) * d->strideA, d->Np, d->Np, d->Np, 1)) return -1;
  if (check_extent(who, "B", d->B, d->lenB, d->offB, (long)(d->m - 1) * d->strideB, d->Np, d->ldb, d->ncols, 1)) return -1;
  if (check_extent(who, "sumsq", d->sumsq, d->lenS, d->offS, (long)(d->m - 1) * d->strideSumsq, d->Np / 128, d->ncols, d->ncols, 1)) return -1;
  ProbeScope sc;
  if (sc.open()) return -1;
  double *dA = nullptr, *dB = nullptr, *dS = nullptr;
  int *deA = nullptr, *deB = nullptr;
  char *fA = nullptr, *fB = nullptr;
  const size_t nA = (size_t)d->lenA, nB = (size_t)d->lenB, nS = (size_t)d->lenS, nE = (size_t)d->m * d->Np;
  if (sc.alloc(&dA, nA) || sc.alloc(&dB, nB) || sc.alloc(&dS, nS) || sc.alloc(&deA, nE) || sc.alloc(&deB, (size_t)d->m) ||
      sc.alloc(&fA, i8_operand_bytes(d->Np, d->Np, d->m)) || sc.alloc(&fB, i8_operand_bytes(d->Np, d->ncols, d->m)))
    return -1;
  if (sc.up(dA, d->A, nA) || sc.up(dB, d->B, nB) || sc.up(deB, d->eB, (size_t)d->m)) return -1;
  HIPCHK(hipMemsetAsync(deA, 0x80, sizeof(int) * nE, sc.s));               // (below any exponent: the kernel takes maxima)
  launch_col_exponents(dA, d->strideA, d->Np, deA, d->m, sc.s);
  launch_slice_operand(dA, d->Np, d->strideA, d->Np, d->Np, d->Np, deA, d->Np, fA, d->m, sc.s);
  launch_slice_operand(dB + d->offB, d->ldb, d->strideB, d->Np, d->Np, d->ncols, deB, 0, fB, d->m, sc.s);
  for (int it = 0; it < d->repeat; ++it) {
    if (sc.up(dS, d->sumsq, nS)) return -1;
    launch_var_i8(fA, fB, d->Np, d->ncols, deA, deB, dS + d->offS, d->strideSumsq, d->m, sc.s, d->i8_group);
  }
  if (sc.down(d->sumsq, dS, nS) || sc.down(d->eA, deA, nE)) return -1;
  return sc.finish();
}

struct bocf_probe_tile128_desc {
  double* A; long lenA, offA;
  double* B; long lenB, offB;                            // (b_alias_c: B is ignored, offB is an origin inside C)
  double* C; long lenC, offC;                            // in and out
  long lda, strideA, ldb, strideB, ldc, strideC;
  double alpha, beta;
  int ntiles, K, m, b_alias_c, repeat;
};

int bocf_probe_tile128(bocf_probe_tile128_desc* d) {
  const char* who = "bocf_probe_tile128";
  if (!d) return probe_fail(who, "null descriptor");
  if (d->ntiles <= 0 || d->K <= 0 || d->K % 128 || d->m <= 0 || d->repeat <= 0) return probe_fail(who, "ntiles, m, repeat must be positive and K a multiple of 128");
  if (d->strideA < 0 || d->strideB < 0 || d->strideC < 0) return probe_fail(who, "negative stride");
  const long W = 128L * d->ntiles;
  if (check_extent(who, "A", d->A, d->lenA, d->offA, (long)(d->m - 1) * d->strideA, d->K, d->lda, 128, 2)) return -1;
  if (d->b_alias_c) {
    if (check_extent(who, "B (in C)", d->C, d->lenC, d->offB, (long)(d->m - 1) * d->strideB, d->K, d->ldb, W, 2)) return -1;
  } else if (check_extent(who, "B", d->B, d->lenB, d->offB, (long)(d->m - 1) * d->strideB, d->K, d->ldb, W, 2)) {
    return -1;
  }
  if (check_extent(who, "C", d->C, d->lenC, d->offC, (long)(d->m - 1) * d->strideC, 128, d->ldc, W, 2)) return -1;
  ProbeScope sc;
  if (sc.open()) return -1;
  double *dA = nullptr, *dB = nullptr, *dC = nullptr;
  const size_t nA = (size_t)d->lenA, nB = d->b_alias_c ? 0 : (size_t)d->lenB, nC = (size_t)d->lenC;
  if (sc.alloc(&dA, nA) || sc.alloc(&dB, nB) || sc.alloc(&dC, nC)) return -1;
  if (sc.up(dA, d->A, nA) || sc.up(dB, d->B, nB)) return -1;
  for (int it = 0; it < d->repeat; ++it) {
    if (sc.up(dC, d->C, nC)) return -1;
    launch_tile128(dA + d->offA, d->lda, d->strideA, (d->b_alias_c ? dC : dB) + d->offB, d->ldb, d->strideB, dC + d->offC, d->ldc, d->strideC, d->alpha,
                   d->beta, d->m, sc.s, d->ntiles, d->K);
  }
  if (sc.down(d->A, dA, nA) || sc.down(d->B, dB, nB) || sc.down(d->C, dC, nC)) return -1;
  return sc.finish();
}

// (Not one of the launcher probes above, hence not named like them.)  The refinement's state machine on the device alone: refine_advance_kernel on the polynomial of refine_poly.h in the place of the
// acquisition pass, `passes` times, from the clamped rows of X0 (A, d).  Outputs as bocf_refine_acq's (F_out = the polynomial).
int bocf_refine_probe_poly(const double* X0, int A, int d, const double* lo, const double* hi, int maxiter, int m, double factr, double pgtol, int max_ls,
                           double c1, int maxfun, int passes, double* X_out, double* F_out, int* iters_out, int* nfun_out, int* reason_out) {
  const char* who = "bocf_refine_probe_poly";
  if (!X0 || !lo || !hi || !X_out || !F_out || !iters_out || !nfun_out || !reason_out) return probe_fail(who, "null argument");
  if (A < 1 || A > 64 || d < 1 || d > REFINE_MAX_D || m < 1 || m > REFINE_MAX_M || max_ls < 1 || maxiter < 0 || passes < 0)
    return probe_fail(who, "need 1 <= A <= 64, 1 <= d <= 64, 1 <= m <= 64, max_ls >= 1, maxiter >= 0, passes >= 0");
  for (int k = 0; k < d; ++k)
    if (!(lo[k] <= hi[k])) return probe_fail(who, "lo > hi");
  RefineSettings s;
  s.d = d; s.m = m; s.maxiter = maxiter; s.max_ls = max_ls; s.maxfun = maxfun < 0 ? -1 : maxfun;
  s.factr = factr; s.pgtol = pgtol; s.c1 = c1; s.boxed = refine_boxed(lo, hi, d);
  std::vector<double> Xcl((size_t)A * d);
  for (int a = 0; a < A; ++a)
    for (int k = 0; k < d; ++k) Xcl[(size_t)a * d + k] = std::fmin(std::fmax(X0[(size_t)a * d + k], lo[k]), hi[k]);
  ProbeScope sc;
  if (sc.open()) return -1;
  const size_t nd = (size_t)A * refine_row_doubles(d, m), ni = (size_t)A * REFINE_ROW_INTS + 1;
  double *Xc = nullptr, *acq = nullptr, *dacq = nullptr, *dbl = nullptr;
  int* ints = nullptr;
  if (sc.alloc(&Xc, (size_t)A * d) || sc.alloc(&acq, (size_t)A) || sc.alloc(&dacq, (size_t)A * d) || sc.alloc(&dbl, nd) || sc.alloc(&ints, ni)) return -1;
  if (sc.up(Xc, Xcl.data(), (size_t)A * d)) return -1;
  HIPCHK(hipMemsetAsync(dbl, 0, sizeof(double) * nd, sc.s));
  HIPCHK(hipMemsetAsync(ints, 0, sizeof(int) * ni, sc.s));
  int* running = ints + (size_t)A * REFINE_ROW_INTS;
  launch_refine_init(Xc, dbl, ints, running, A, s, sc.s);
  for (int p = 0; p < passes; ++p) {
    launch_refine_poly(Xc, A, d, acq, dacq, sc.s);
    launch_refine_advance(acq, dacq, Xc, dbl, ints, running, A, s, lo, hi, sc.s);
  }
  std::vector<double> hd(nd);
  std::vector<int> hints(ni);
  if (sc.down(hd.data(), dbl, nd) || sc.down(hints.data(), ints, ni)) return -1;
  if (sc.finish()) return -1;
  for (int a = 0; a < A; ++a) {
    const RefineRow r = refine_row_view(hd.data() + (size_t)a * refine_row_doubles(d, m), hints.data() + (size_t)a * REFINE_ROW_INTS, d, m);
    for (int k = 0; k < d; ++k) X_out[(size_t)a * d + k] = r.x[k];
    F_out[a] = *r.f;
    iters_out[a] = *r.iters;
    nfun_out[a] = *r.nfun;
    reason_out[a] = *r.reason;
  }
  return 0;
}

}  // extern "C"
#endif
