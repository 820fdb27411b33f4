// Device side of the resident anchor refinement: between two acquisition passes one launch of refine_advance_kernel
// moves every row of the batch one evaluation further -- the step of refine_step.h, the same text the host driver of the CPU suite runs.
//
// One workgroup (one wave) per row.  The step is a serial recurrence of a few hundred flops whose sums must run in the host routine's
// order, so lane 0 runs it; the lanes share the loads of the gradient and the stores of the next trial point.  No workgroup waits for,
// polls or reads anything another workgroup writes; the only shared word is the count of running rows, decremented (one atomic per row,
// once) when a row stops and read by the host alone.  All stores are ordinary vector stores.
#include "bocf_internal.h"
#include "refine_poly.h"
#include "../../include/bocf_hip.h"

static_assert(REFINE_MAX_D == 64, "refine_advance_kernel stages the box with one lane per dimension");

// bounds of the box by value in the kernel arguments (2 x 64 doubles): nothing to upload, nothing to keep alive
struct RefineBox { double lo[REFINE_MAX_D], hi[REFINE_MAX_D]; };

struct RefineKernelArgs {
  const double* acq;         // (A) the acquisition at the resident candidates (maximised: the optimiser minimises its negative)
  const double* dacq;        // (A, d)
  double* Xc;                // (A, d) resident candidate rows: the next trial point of every row goes here
  double* dbl; int* ints;    // the rows' state blocks (refine_row_doubles each / REFINE_ROW_INTS each)
  int* running;              // rows still running
  // batches above the small path (refine_compact_kernel): when *small, row r reads column map[r] of acq2 / dacq2 instead
  const double* acq2; const double* dacq2; const int* map; const int* small;
  int A;
  RefineSettings s;
};

// fresh rows from the (already clamped) resident candidates; the state blocks were zeroed by the caller
__global__ __launch_bounds__(64) void refine_init_kernel(RefineKernelArgs a) {
  const int row = blockIdx.x;
  if (row >= a.A) return;
  const RefineRow r = refine_row_view(a.dbl + (size_t)row * refine_row_doubles(a.s.d, a.s.m), a.ints + (size_t)row * REFINE_ROW_INTS, a.s.d, a.s.m);
  for (int k = threadIdx.x; k < a.s.d; k += 64) r.x[k] = r.xt[k] = a.Xc[(size_t)row * a.s.d + k];
  if (row == 0 && threadIdx.x == 0) *a.running = a.A;
}

__global__ __launch_bounds__(64) void refine_advance_kernel(RefineKernelArgs a, RefineBox box) {
  __shared__ double g[REFINE_MAX_D], lo[REFINE_MAX_D], hi[REFINE_MAX_D];
  const int row = blockIdx.x, d = a.s.d;
  if (row >= a.A) return;
  lo[threadIdx.x] = box.lo[threadIdx.x];                   // (REFINE_MAX_D = the 64 lanes)
  hi[threadIdx.x] = box.hi[threadIdx.x];
  const RefineRow r = refine_row_view(a.dbl + (size_t)row * refine_row_doubles(d, a.s.m), a.ints + (size_t)row * REFINE_ROW_INTS, d, a.s.m);
  const double* acq = a.acq;
  const double* dacq = a.dacq;
  int col = row;
  if (a.map && *a.small) {
    acq = a.acq2; dacq = a.dacq2;
    col = a.map[row] < 0 ? 0 : a.map[row];                 // (a stopped row reads nothing it uses)
  }
  for (int k = threadIdx.x; k < d; k += 64) g[k] = -dacq[(size_t)col * d + k];
  __syncthreads();
  if (threadIdx.x == 0 && *r.reason == REFINE_RUNNING) {
    refine_advance(r, -acq[col], g, lo, hi, a.s);
    if (*r.reason != REFINE_RUNNING) atomicSub(a.running, 1);
  }
  __syncthreads();                                         // (lane 0's stores to the row's block are visible to the workgroup behind it)
  const double* p = refine_point(r);
  for (int k = threadIdx.x; k < d; k += 64) a.Xc[(size_t)row * d + k] = p[k];
}

// Batches above the small path of the predict pass (A > BOCF_SMALL_N).  The host loop evaluates the running rows only, so once
// BOCF_SMALL_N or fewer are left its posterior comes from the small path, whose last digits differ from the GEMM path's.  To evaluate every
// point as the host loop does, without asking the host how many rows run, a pass of such a batch predicts twice -- the whole batch, and
// the first BOCF_SMALL_N running rows gathered here in row order (x2; short lists repeat their last row) -- and the step reads the
// gathered columns when *small says that no more are running.  One workgroup; nothing waits.
__global__ __launch_bounds__(64) void refine_compact_kernel(const double* Xc, const int* ints, int A, int d, double* x2, int* map, int* small) {
  __shared__ int list[BOCF_REFINE_MAX_ROWS];
  __shared__ int count;
  if (threadIdx.x == 0) {
    int n = 0;
    for (int a = 0; a < A; ++a) {
      const bool running = ints[(size_t)a * REFINE_ROW_INTS + 2] == REFINE_RUNNING;
      map[a] = running ? n : -1;
      if (running) list[n++] = a;
    }
    count = n;
    *small = n <= BOCF_SMALL_N;
  }
  __syncthreads();
  const int n = count;
  for (int i = threadIdx.x; i < BOCF_SMALL_N * d; i += 64) {
    const int j = i / d, k = i - j * d;
    const int src = n ? list[j < n ? j : n - 1] : 0;
    x2[i] = Xc[(size_t)src * d + k];
  }
}

#ifdef BOCF_PROBES
// probes build: -f and -g of the polynomial of refine_poly.h at the resident rows, in the place of the acquisition pass
__global__ __launch_bounds__(64) void refine_poly_kernel(const double* Xc, int A, int d, double* acq, double* dacq) {
  __shared__ double g[REFINE_MAX_D];
  const int row = blockIdx.x;
  if (row >= A) return;
  if (threadIdx.x == 0) acq[row] = -refine_poly(Xc + (size_t)row * d, d, g);
  __syncthreads();
  for (int k = threadIdx.x; k < d; k += 64) dacq[(size_t)row * d + k] = -g[k];
}
#endif

static RefineKernelArgs refine_args(const double* acq, const double* dacq, double* Xc, double* dbl, int* ints, int* running, int A, const RefineSettings& s) {
  RefineKernelArgs a;
  a.acq = acq; a.dacq = dacq; a.Xc = Xc; a.dbl = dbl; a.ints = ints; a.running = running; a.A = A; a.s = s;
  a.acq2 = a.dacq2 = nullptr; a.map = a.small = nullptr;
  return a;
}

static RefineBox refine_box(const double* lo, const double* hi, int d) {
  RefineBox b;
  for (int k = 0; k < REFINE_MAX_D; ++k) {
    b.lo[k] = k < d ? lo[k] : 0.0;
    b.hi[k] = k < d ? hi[k] : 0.0;
  }
  return b;
}

void launch_refine_init(double* Xc, double* dbl, int* ints, int* running, int A, const RefineSettings& s, hipStream_t st) {
  BOCF_LAUNCH(refine_init_kernel, dim3((unsigned)A), dim3(64), 0, st, refine_args(nullptr, nullptr, Xc, dbl, ints, running, A, s));
}

void launch_refine_advance(const double* acq, const double* dacq, double* Xc, double* dbl, int* ints, int* running, int A, const RefineSettings& s,
                           const double* lo, const double* hi, hipStream_t st, const double* acq2, const double* dacq2, const int* map, const int* small) {
  RefineKernelArgs a = refine_args(acq, dacq, Xc, dbl, ints, running, A, s);
  a.acq2 = acq2; a.dacq2 = dacq2; a.map = map; a.small = small;
  BOCF_LAUNCH(refine_advance_kernel, dim3((unsigned)A), dim3(64), 0, st, a, refine_box(lo, hi, s.d));
}

void launch_refine_compact(const double* Xc, const int* ints, int A, int d, double* x2, int* map, int* small, hipStream_t st) {
  BOCF_LAUNCH(refine_compact_kernel, dim3(1), dim3(64), 0, st, Xc, ints, A, d, x2, map, small);
}

#ifdef BOCF_PROBES
void launch_refine_poly(const double* Xc, int A, int d, double* acq, double* dacq, hipStream_t st) {
  BOCF_LAUNCH(refine_poly_kernel, dim3((unsigned)A), dim3(64), 0, st, Xc, A, d, acq, dacq);
}
#endif
