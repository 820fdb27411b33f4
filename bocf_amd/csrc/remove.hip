// Removal of one observation from the resident factor: U' and R' = U'^-1 of the N - 1 remaining points in O(N^2).
//
// Row k of R, r, fixes every plane rotation: t_q = ||r[k .. q]||, s_j = t_j / t_{j+1}, c_j = r[j+1] / t_{j+1} (j = k .. N-2).  The chain
// of reflections in the planes (j, j+1) is linear in its carry, and with these coefficients the carry in front of step j telescopes to
//   p_j = (1 / t_j) sum_{q = k .. j} r[q] x[q]
// for x a column of U (indexed by its row) or a row of R (indexed by its column) -- a prefix dot product with r, no product of s_j.  So
//   out[j] = x[j]                                   j <  k
//   out[j] = s_j x[j+1] - (c_j / t_j) sum_{q<=j} r[q] x[q]      k <= j <= N-2
// and a 128-row block needs from the blocks above it only their partial dot products.  Four launches, all outputs in each:
//   remove_scan_kernel     s_j and g_j = c_j / t_j from the prefix sums of r^2
//   remove_partial_kernel  the partial dot products of every 128-row block with r, for the columns of U and of R^T
//   remove_rotate_kernel   out[j] per 128 x 128 tile into the T scratch: U' in its upper triangle (diagonal included), R'^T strictly below
//                          (the diagonal of R' is 1 / diag U').  Out of place: out[j] reads rows j and j+1 and the columns shift left by
//                          one, so a tile reads what its neighbours would overwrite.
//   remove_store_kernel    T back into S (both halves), R, R^T and the diagonal tiles E, E^T through an LDS tile: every store is a
//                          coalesced row.  Inside the diagonal 64-tiles of S, R, R^T and everywhere in E, E^T the entries that are zero by
//                          construction are written as zeros; the off-diagonal tiles of the other triangle of R / R^T are left alone (zeros
//                          since the buffers were cleared: no kernel writes them).  Row / column N-1 becomes identity padding.
// remove_shift_kernel moves the input rows behind k up by one (X and every output's scaled copy) through a scratch.
#include "bocf_internal.h"
#include "fit_device.h"

#define RM_ST 64               // tile edge of the store kernel (one 64 x 65 LDS tile: 33 KB)

// one workgroup per output.  coef: s (Np) | g (Np); entries outside k .. N-2 are not read.
__global__ __launch_bounds__(256) void remove_scan_kernel(const double* __restrict__ R, long strideS, int Np, int N, int k,
                                                          double* __restrict__ coef) {
  const int o = blockIdx.x, tid = threadIdx.x;
  const double* __restrict__ r = R + (long)o * strideS + (long)k * Np;
  double* __restrict__ sc = coef + (long)o * 2 * Np;
  double* __restrict__ gc = sc + Np;
  const int len = N - k, chunk = (len + 255) / 256;
  const int q0 = k + tid * chunk, q1 = min(q0 + chunk, N);
  __shared__ double part[256];
  double s = 0.0;
  for (int q = q0; q < q1; ++q) s += r[q] * r[q];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {                                        // exclusive prefix over the 256 chunk sums, in order
    double run = 0.0;
    for (int i = 0; i < 256; ++i) {
      const double v = part[i];
      part[i] = run;
      run += v;
    }
  }
  __syncthreads();
  if (q0 >= q1) return;
  double run = part[tid] + r[q0] * r[q0];
  double tcur = sqrt(run);
  for (int j = q0; j < q1 && j < N - 1; ++j) {
    const double rn = r[j + 1];
    run += rn * rn;
    const double tnext = sqrt(run);
    sc[j] = tcur / tnext;
    gc[j] = rn / (tnext * tcur);
    tcur = tnext;
  }
}

// x[q] of column `col`: U from S (rows <= col; the lower half of S mirrors it) or R^T (rows >= col); zero outside the N-point factor
__device__ __forceinline__ double rm_entry(const double* __restrict__ M, int mat, int Np, int N, int q, int col) {
  const bool in = mat == 0 ? (q <= col && col < N) : (q >= col && q < N);
  return in ? M[(long)q * Np + col] : 0.0;
}

// grid (Np / 128, nb, 2 m): part[((o * 2 + mat) * nb + I) * Np + col] = sum over the rows q of block I, k <= q < N, of r[q] x[q] -- for the
// tiles that can hold a non-zero of U (I <= column block) or R^T (I >= column block) from the block of k on; the others are not written
__global__ __launch_bounds__(NB) void remove_partial_kernel(const double* __restrict__ S, const double* __restrict__ RT,
                                                            const double* __restrict__ R, long strideS, int Np, int N, int k,
                                                            double* __restrict__ part) {
  const int I = blockIdx.y, mat = blockIdx.z & 1, o = blockIdx.z >> 1, nb = Np / NB;
  if (I * NB + NB - 1 < k) return;                       // (never read: the sums start at the block that holds k)
  if (mat == 0 ? I > (int)blockIdx.x : I < (int)blockIdx.x) return;   // zero by construction (U below, R^T above the diagonal tiles): the rotate kernel's sums skip them
  const int col = blockIdx.x * NB + threadIdx.x;
  const double* __restrict__ M = (mat == 0 ? S : RT) + (long)o * strideS;
  __shared__ double rs[NB];
  {
    const int q = I * NB + threadIdx.x;
    rs[threadIdx.x] = (q >= k && q < N) ? R[(long)o * strideS + (long)k * Np + q] : 0.0;
  }
  __syncthreads();
  int lo = max(k, I * NB), hi = min(I * NB + NB - 1, N - 1);
  if (mat == 0) hi = col < N ? min(hi, col) : -1;
  else lo = max(lo, col);
  double acc = 0.0;
#pragma unroll 4
  for (int q = lo; q <= hi; ++q) acc += rs[q - I * NB] * M[(long)q * Np + col];
  part[((long)(o * 2 + mat) * nb + I) * Np + col] = acc;
}

// grid (Np / 128, nb, 2 m): tile (I, J) of T -- rows j of block I, new columns c' of block J.  mat 0 (U': I <= J, J >= k / 128) writes
// j <= c', mat 1 (R'^T: I >= J, I >= k / 128) writes j > c'.
__global__ __launch_bounds__(NB) void remove_rotate_kernel(const double* __restrict__ S, const double* __restrict__ RT,
                                                           const double* __restrict__ R, long strideS, int Np, int N, int k,
                                                           const double* __restrict__ coef, const double* __restrict__ part,
                                                           double* __restrict__ T) {
  const int J = blockIdx.x, I = blockIdx.y, mat = blockIdx.z & 1, o = blockIdx.z >> 1, nb = Np / NB, kb = k / NB;
  if (mat == 0 ? (I > J || J < kb) : (I < J || I < kb)) return;
  const int tid = threadIdx.x, j0 = I * NB;
  __shared__ double rs[NB], ss[NB], gs[NB];
  {
    const int q = j0 + tid;
    rs[tid] = (q >= k && q < N) ? R[(long)o * strideS + (long)k * Np + q] : 0.0;
    const bool step = q >= k && q < N - 1;
    ss[tid] = step ? coef[(long)o * 2 * Np + q] : 0.0;
    gs[tid] = step ? coef[(long)o * 2 * Np + Np + q] : 0.0;
  }
  __syncthreads();
  const int cn = J * NB + tid;                           // new column
  const int c = cn + (cn >= k ? 1 : 0);                  // the column it comes from (Np: none, reads as zero)
  const bool have = c < N;
  const double* __restrict__ M = (mat == 0 ? S : RT) + (long)o * strideS;
  double* __restrict__ Tj = T + (long)o * strideS;
  double acc = 0.0;
  if (have)                                              // (R^T is zero above the row block of its column: those partial sums are not even written)
    for (int b = mat == 0 ? kb : max(kb, c / NB); b < I; ++b) acc += part[((long)(o * 2 + mat) * nb + b) * Np + c];
  double xj = have ? rm_entry(M, mat, Np, N, j0, c) : 0.0;
#pragma unroll 8
  for (int l = 0; l < NB; ++l) {
    const int j = j0 + l;
    const double xn = (have && j + 1 < N) ? rm_entry(M, mat, Np, N, j + 1, c) : 0.0;
    acc += rs[l] * xj;
    double out = j < k ? xj : ss[l] * xn - gs[l] * acc;
    if (j >= N - 1 || cn >= N - 1) out = j == cn ? 1.0 : 0.0;          // identity padding from row / column N-1 on
    if (mat == 0 ? j <= cn : j > cn) Tj[(long)j * Np + cn] = out;
    xj = xn;
  }
}

// grid (Np / 64, Np / 64, m): the pair of 64 x 64 tiles (I, J) and (J, I) of T, I <= J, J >= k / 64 (columns in front of k keep their
// values in all five arrays).  R and R^T keep the zeros of their other triangle outside the diagonal 64-tiles: nothing ever writes them.
__global__ __launch_bounds__(256) void remove_store_kernel(const double* __restrict__ T, double* __restrict__ S, double* __restrict__ R,
                                                          double* __restrict__ RT, long strideS, double* __restrict__ E,
                                                          double* __restrict__ ET, long strideE, int Np, int k) {
  const int J = blockIdx.x, I = blockIdx.y, o = blockIdx.z;
  if (I > J || J < k / RM_ST) return;
  const int tid = threadIdx.x, b = tid & (RM_ST - 1), a0 = tid / RM_ST;
  const bool diag = I == J;
  const double* __restrict__ Tj = T + (long)o * strideS;
  double* __restrict__ Sj = S + (long)o * strideS;
  double* __restrict__ Rj = R + (long)o * strideS;
  double* __restrict__ RTj = RT + (long)o * strideS;
  const int gi0 = I * RM_ST, gj0 = J * RM_ST;
  __shared__ double tile[RM_ST][RM_ST + 1];
  __shared__ double dinv[RM_ST];
  // ---- U': tile (I, J) of T
  for (int a = a0; a < RM_ST; a += 4) tile[a][b] = Tj[(long)(gi0 + a) * Np + gj0 + b];
  __syncthreads();
  if (tid < RM_ST) dinv[tid] = diag ? 1.0 / tile[tid][tid] : 0.0;
  for (int a = a0; a < RM_ST; a += 4) {
    Sj[(long)(gi0 + a) * Np + gj0 + b] = (!diag || a <= b) ? tile[a][b] : tile[b][a];
    if (!diag) Sj[(long)(gj0 + a) * Np + gi0 + b] = tile[b][a];       // the mirrored lower half
  }
  __syncthreads();
  // ---- R'^T: tile (J, I) of T (the diagonal tile is already here)
  if (!diag) {
    for (int a = a0; a < RM_ST; a += 4) tile[a][b] = Tj[(long)(gj0 + a) * Np + gi0 + b];
    __syncthreads();
  }
  const int p = I / 2;                                   // the 128-tile of row block I
  const bool in_e = p == J / 2;                          // (I, J) lies inside a diagonal 128-tile: E and E^T hold it too
  double* __restrict__ Ej = E + (long)o * strideE + (long)p * NB * NB;
  double* __restrict__ ETj = ET + (long)o * strideE + (long)p * NB * NB;
  const int ei0 = gi0 - p * NB, ej0 = gj0 - p * NB;
  for (int a = a0; a < RM_ST; a += 4) {
    // R^T rows of block J, columns of block I: tile[a][b] = R'[gi0 + b][gj0 + a]
    const double vt = !diag ? tile[a][b] : (a > b ? tile[a][b] : (a == b ? dinv[a] : 0.0));
    // R rows of block I, columns of block J: R'[gi0 + a][gj0 + b] = tile[b][a]
    const double vr = !diag ? tile[b][a] : (a < b ? tile[b][a] : (a == b ? dinv[a] : 0.0));
    RTj[(long)(gj0 + a) * Np + gi0 + b] = vt;
    Rj[(long)(gi0 + a) * Np + gj0 + b] = vr;
    if (in_e) {
      Ej[(ei0 + a) * NB + ej0 + b] = vr;
      ETj[(ej0 + a) * NB + ei0 + b] = vt;
      if (!diag) {                                       // the quarter of the diagonal 128-tile below / above it: zeros
        Ej[(ej0 + a) * NB + ei0 + b] = 0.0;
        ETj[(ei0 + a) * NB + ej0 + b] = 0.0;
      }
    }
  }
}

// rows k+1 .. N-1 of `nblk` row-major (rows, d) blocks move up by one, through tmp (nblk x cnt): phase 0 copies them out, phase 1 back
__global__ __launch_bounds__(256) void remove_shift_kernel(double* __restrict__ buf, long stride, int k, int d, long cnt,
                                                          double* __restrict__ tmp, int phase) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= cnt) return;
  double* __restrict__ blk = buf + (long)blockIdx.y * stride;
  double* __restrict__ t = tmp + (long)blockIdx.y * cnt;
  if (phase == 0) t[e] = blk[(long)(k + 1) * d + e];
  else blk[(long)k * d + e] = t[e];
}

void launch_remove_factor(double* S, double* R, double* RT, double* T, long strideS, double* E, double* ET, long strideE, int Np, int N, int k,
                          double* coef, double* part, int m, hipStream_t s) {
  const unsigned nb = (unsigned)(Np / NB), nt = (unsigned)(Np / RM_ST);
  BOCF_LAUNCH(remove_scan_kernel, dim3((unsigned)m), dim3(256), 0, s, R, strideS, Np, N, k, coef);
  BOCF_LAUNCH(remove_partial_kernel, dim3(nb, nb, (unsigned)(2 * m)), dim3(NB), 0, s, S, RT, R, strideS, Np, N, k, part);
  BOCF_LAUNCH(remove_rotate_kernel, dim3(nb, nb, (unsigned)(2 * m)), dim3(NB), 0, s, S, RT, R, strideS, Np, N, k, coef, part, T);
  BOCF_LAUNCH(remove_store_kernel, dim3(nt, nt, (unsigned)m), dim3(256), 0, s, T, S, R, RT, strideS, E, ET, strideE, Np, k);
}

void launch_remove_rows(double* buf, long stride, int nblk, int N, int k, int d, double* tmp, hipStream_t s) {
  const long cnt = (long)(N - 1 - k) * d;
  if (cnt <= 0) return;
  const dim3 grid((unsigned)((cnt + 255) / 256), (unsigned)nblk);
  BOCF_LAUNCH(remove_shift_kernel, grid, dim3(256), 0, s, buf, stride, k, d, cnt, tmp, 0);
  BOCF_LAUNCH(remove_shift_kernel, grid, dim3(256), 0, s, buf, stride, k, d, cnt, tmp, 1);
}
