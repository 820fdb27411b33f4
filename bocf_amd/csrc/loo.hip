// Leave-one-out cross-validation of the resident model (ExactGaussianInference.LOO, exact_gaussian_inference.py:67-79, plus the
// leave-one-out predictive moments the log densities are made of).  The fit leaves R = U^-1 (upper, row-major, Ky^-1 = R R^T) and alpha
// = Ky^-1 yc resident, so for training point i of factorization j
//   c_i      = (Ky^-1)_ii = sum_{k >= i} R[i][k]^2            (a sum of squares over a contiguous row: no cancellation)
//   mu_loo   = y_i - alpha_i / c_i
//   var_loo  = 1 / c_i - shift [- noise],  shift = what the fit added to the diagonal besides the noise (1e-8 + jitter)
//   lpd      = -0.5 log 2 pi + 0.5 log c_i - 0.5 alpha_i^2 / c_i   (:73-79 to the letter)
// One bandwidth-bound pass over the upper triangle of R instead of N refits.  Geometry of gemv_upper_n_kernel (fit.hip): one wave per
// training row, four per workgroup, grid (Np / 4, M); a lane takes the column pairs 2 lane + 128 t from the 64-aligned start of the row's
// upper part, the 64 partial sums meet in the fixed __shfl_xor butterfly, lane 0 writes the row's three results.  No atomics, plain
// stores; what a row gets depends on that row alone (not on N's padding, the other outputs or the launch's grid).
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"

#include <cstdint>

// VEC: the pair is one 16-byte load (the row start r Np + (r & ~63) is a multiple of 64 doubles, so only the base and the per-output
// stride decide); otherwise two 8-byte loads.  Both forms add the same squares in the same order: the bits do not depend on the choice.
template <int VEC>
__global__ __launch_bounds__(256) void loo_kernel(const double* __restrict__ R, long strideR, int N, int Np, const double* __restrict__ alpha,
                                                  const double* __restrict__ yc, const KernHyp* __restrict__ hyp, const double* __restrict__ shift,
                                                  int flags, double* __restrict__ mu, double* __restrict__ var, double* __restrict__ lpd, long ld) {
  const int j = blockIdx.y;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = blockIdx.x * 4 + w;
  if (r >= N) return;                                      // wave-uniform (padding rows have no observation)
  const double* __restrict__ Rr = R + (long)j * strideR + (long)r * Np;
  typedef double v2 __attribute__((ext_vector_type(2)));
  double acc = 0.0;
  // (kk is even and < N <= Np, Np even: kk + 1 is inside the row)
  for (int kk = (r & ~63) + 2 * lane; kk < N; kk += 128) {
    double a, b;
    if (VEC) {
      const v2 p = *reinterpret_cast<const v2*>(Rr + kk);
      a = p.x;
      b = p.y;
    } else {
      a = Rr[kk];
      b = Rr[kk + 1];
    }
    if (kk < r) a = 0.0;                                   // below the diagonal, and ...
    if (kk + 1 < r || kk + 1 >= N) b = 0.0;                // ... columns of the padding: not part of Ky^-1
    acc = __builtin_fma(a, a, acc);
    acc = __builtin_fma(b, b, acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) {
    const double c = acc, a = alpha[(long)j * Np + r];
    const double q = a / c;
    double v = 1.0 / c - shift[j];
    if (!(flags & BOCF_ADD_NOISE)) v -= hyp[j].noise;
    if ((flags & BOCF_CLIP) && !(v >= 1e-10)) v = 1e-10;
    mu[(long)j * ld + r] = (yc[(long)j * Np + r] + hyp[j].ymean) - q;
    var[(long)j * ld + r] = v;
    lpd[(long)j * ld + r] = -0.91893853320467274178 + 0.5 * log(c) - 0.5 * (a * q);
  }
}

void launch_loo(const double* R, long strideR, int N, int Np, const double* alpha, const double* yc, const KernHyp* hyp, const double* shift, int flags,
                double* mu, double* var, double* lpd, long ld, int m, hipStream_t s) {
  const dim3 grid((unsigned)(Np / 4), (unsigned)m);
  if ((reinterpret_cast<uintptr_t>(R) & 15) == 0 && (strideR & 1) == 0 && (Np & 1) == 0)
    BOCF_LAUNCH((loo_kernel<1>), grid, dim3(256), 0, s, R, strideR, N, Np, alpha, yc, hyp, shift, flags, mu, var, lpd, ld);
  else
    BOCF_LAUNCH((loo_kernel<0>), grid, dim3(256), 0, s, R, strideR, N, Np, alpha, yc, hyp, shift, flags, mu, var, lpd, ld);
}

// lpd_sum[j] = sum_{i < N} lpd[j][i]: one workgroup per factorization, strided partial sums and the LDS tree of lml_kernel (fit.hip) --
// a fixed order
__global__ __launch_bounds__(256) void loo_sum_kernel(const double* __restrict__ lpd, long ld, int N, double* __restrict__ out) {
  const int j = blockIdx.x;
  double s = 0.0;
  for (int i = threadIdx.x; i < N; i += 256) s += lpd[(long)j * ld + i];
  __shared__ double red[256];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[j] = red[0];
}

void launch_loo_sum(const double* lpd, long ld, int N, double* out, int m, hipStream_t s) {
  BOCF_LAUNCH(loo_sum_kernel, dim3((unsigned)m), dim3(256), 0, s, lpd, ld, N, out);
}

// rows[l][i] = l: the parameter index of every "candidate" of the l-th expected-utility launch over the N leave-one-out posteriors
__global__ __launch_bounds__(256) void loo_rows_kernel(int* __restrict__ rows, int N, int L) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N && (int)blockIdx.y < L) rows[(long)blockIdx.y * N + i] = blockIdx.y;
}

void launch_loo_rows(int* rows, int N, int L, hipStream_t s) {
  BOCF_LAUNCH(loo_rows_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)L), dim3(256), 0, s, rows, N, L);
}
