// Utility programs (include/bocf_hip.h): the host-side validator and the Monte-Carlo kernels that evaluate the user's traced utility
// through the interpreter of util_prog_dev.h.  The launchers of acq.hip / eu.hip / thompson.hip dispatch here when the utility kind is
// BOCF_UTIL_PROGRAM; the kernels of the closed set are untouched.
// Geometry and arithmetic order are those of the closed-set kernels: one wave per candidate, lanes stride the samples, partial sums meet in
// the fixed __shfl_xor butterfly, sums over the parameters l in index order -- a candidate's result does not depend on the batch it came
// in, and runs are bit-reproducible.  The sample loop is wave-uniform (lanes past the last sample compute on the last sample and are
// masked out of the sums), so every branch of the interpreter is scalar.
#include "bocf_ctx.h"
#include "util_prog_dev.h"

#include <cmath>
#include <cstdio>
#include <cstring>

// ---------------------------------------------------------------------------------------------
// validator (host only)
static int prog_fail(const char* who, const char* fmt, long a = 0, long b = 0, long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  return fail(who, buf);
}

static int check_section(const char* who, const char* name, const unsigned* w, int n, int n_slots, int m, int theta_dim, int n_const, const int* outs,
                         int n_outs) {
  bool written[BOCF_PROG_MAX_SLOTS] = {false};
  for (int i = 0; i < n; ++i) {
    const unsigned op = w[2 * i] & 0xffu, dst = w[2 * i] >> 8;
    if (op >= BOCF_OP_COUNT) return prog_fail(who, (std::string(name) + " section, instruction %ld: opcode %ld out of range").c_str(), i, op);
    const unsigned ops[2] = {w[2 * i + 1] & 0xffffu, w[2 * i + 1] >> 16};
    for (unsigned o : ops) {
      const unsigned kind = o >> 14, idx = o & 0x3fffu;
      if (kind == BOCF_OPERAND_SLOT) {
        if ((int)idx >= n_slots) return prog_fail(who, (std::string(name) + " section, instruction %ld: slot index %ld >= slot count %ld").c_str(), i, idx, n_slots);
        if (!written[idx]) return prog_fail(who, (std::string(name) + " section, instruction %ld: slot %ld is read before it is written").c_str(), i, idx);
      } else if (kind == BOCF_OPERAND_INPUT) {
        if ((int)idx >= m) return prog_fail(who, (std::string(name) + " section, instruction %ld: input index %ld >= m = %ld").c_str(), i, idx, m);
      } else if (kind == BOCF_OPERAND_PARAM) {
        if ((int)idx >= theta_dim) return prog_fail(who, (std::string(name) + " section, instruction %ld: parameter index %ld >= theta_dim = %ld").c_str(), i, idx, theta_dim);
      } else if ((int)idx >= n_const) {
        return prog_fail(who, (std::string(name) + " section, instruction %ld: constant index %ld >= constant count %ld").c_str(), i, idx, n_const);
      }
    }
    if ((int)dst >= n_slots) return prog_fail(who, (std::string(name) + " section, instruction %ld: destination slot index %ld >= slot count %ld").c_str(), i, dst, n_slots);
    written[dst] = true;
  }
  for (int q = 0; q < n_outs; ++q) {
    if (outs[q] < 0 || outs[q] >= n_slots) return prog_fail(who, (std::string(name) + " section: output %ld names slot %ld >= slot count %ld").c_str(), q, outs[q], n_slots);
    if (!written[outs[q]]) return prog_fail(who, (std::string(name) + " section: output slot %ld (output %ld) is never written").c_str(), outs[q], q);
  }
  return 0;
}

int util_prog_check(const char* who, const void* blob, long nbytes, int m, int theta_dim, UtilProg* out) {
  if (!blob) return fail(who, "null blob");
  const long hb = 4L * BOCF_PROG_HEADER_WORDS;
  if (nbytes < hb) return prog_fail(who, "truncated blob: %ld bytes, the header alone has %ld", nbytes, hb);
  unsigned h[BOCF_PROG_HEADER_WORDS];
  memcpy(h, blob, hb);
  if (h[0] != BOCF_PROG_MAGIC) return fail(who, "bad magic: not a utility program");
  if (h[1] != BOCF_PROG_VERSION) return prog_fail(who, "unsupported version %ld (this library reads version %ld)", h[1], BOCF_PROG_VERSION);
  if (h[2] < 1 || h[2] > BOCF_MAX_M) return prog_fail(who, "m = %ld out of range (1 .. %ld)", h[2], BOCF_MAX_M);
  if (h[3] >= (1u << 14)) return prog_fail(who, "theta_dim = %ld out of range", h[3]);
  if (m >= 0 && (int)h[2] != m) return prog_fail(who, "the program was built for m = %ld outputs, the call has m = %ld", h[2], m);
  if (theta_dim >= 0 && (int)h[3] != theta_dim) return prog_fail(who, "the program was built for theta_dim = %ld, the call has theta_dim = %ld", h[3], theta_dim);
  if (h[4] < 1 || h[4] > BOCF_PROG_MAX_SLOTS) return prog_fail(who, "slot count %ld out of range (1 .. BOCF_PROG_MAX_SLOTS = %ld)", h[4], BOCF_PROG_MAX_SLOTS);
  if (h[5] < 1 || h[5] > BOCF_PROG_MAX_INSTR) return prog_fail(who, "value section length %ld out of range (1 .. BOCF_PROG_MAX_INSTR = %ld)", h[5], BOCF_PROG_MAX_INSTR);
  if (h[6] < 1 || h[6] > BOCF_PROG_MAX_INSTR)
    return prog_fail(who, "value+gradient section length %ld out of range (1 .. BOCF_PROG_MAX_INSTR = %ld)", h[6], BOCF_PROG_MAX_INSTR);
  if (h[7] > BOCF_PROG_MAX_CONSTS) return prog_fail(who, "constant count %ld exceeds BOCF_PROG_MAX_CONSTS = %ld", h[7], BOCF_PROG_MAX_CONSTS);
  const long want = hb + 8L * ((long)h[5] + h[6] + h[7]);
  if (nbytes != want) return prog_fail(who, nbytes < want ? "truncated blob: %ld bytes, the header describes %ld" : "blob size %ld does not match the %ld bytes the header describes", nbytes, want);
  UtilProg p;
  p.m = (int)h[2]; p.theta_dim = (int)h[3]; p.n_slots = (int)h[4]; p.n_val = (int)h[5]; p.n_grad = (int)h[6]; p.n_const = (int)h[7];
  p.val_out = (int)h[8];
  for (int q = 0; q <= p.m; ++q) p.grad_out[q] = (int)h[9 + q];
  std::vector<unsigned> code(2 * (size_t)(p.n_val + p.n_grad));
  memcpy(code.data(), static_cast<const char*>(blob) + hb, 4 * code.size());
  std::vector<double> consts(p.n_const);
  memcpy(consts.data(), static_cast<const char*>(blob) + hb + 4 * code.size(), 8 * consts.size());
  for (int q = 0; q < p.n_const; ++q)
    if (!std::isfinite(consts[q])) return prog_fail(who, "constant %ld is not finite", q);
  if (check_section(who, "value", code.data(), p.n_val, p.n_slots, p.m, p.theta_dim, p.n_const, &p.val_out, 1)) return -1;
  if (check_section(who, "value+gradient", code.data() + 2 * (size_t)p.n_val, p.n_grad, p.n_slots, p.m, p.theta_dim, p.n_const, p.grad_out, 1 + p.m)) return -1;
  if (out) *out = p;
  return 0;
}

extern "C" int bocf_check_utility_program(const void* blob, long nbytes, int m, int theta_dim) {
  if (m < 0 || theta_dim < 0) return fail("bocf_check_utility_program", "m and theta_dim must be >= 0");
  return util_prog_check("bocf_check_utility_program", blob, nbytes, m, theta_dim, nullptr);
}

extern "C" int bocf_set_utility_program(bocf_ctx* c, const void* blob, long nbytes) {
  static const char* who = "bocf_set_utility_program";
  if (!c) return fail(who, "null context");
  UtilProg p;
  if (util_prog_check(who, blob, nbytes, -1, -1, &p)) return -1;      // a rejected blob leaves the resident program as it was
  HIPCHK(hipSetDevice(c->device));
  c->prog.dev = nullptr;                                   // (every call is synchronous on return: no kernel is reading the old copy)
  c->best_epoch = -1;                                      // the best-so-far values belong to the old program
  if (c->prog_buf.ensure((size_t)nbytes)) return -1;
  HIPCHK(hipMemcpyAsync(c->prog_buf.p, blob, (size_t)nbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  p.dev = c->prog_buf.as<unsigned>();
  c->prog = p;
  return 0;
}

int bocf_check_resident_program(bocf_ctx* c, const char* who, int m, int theta_dim, int n_util_params) {
  if (!c->prog.dev) return fail(who, "utility kind BOCF_UTIL_PROGRAM but no utility program is resident (bocf_set_utility_program)");
  if (n_util_params != 0) return fail(who, "a utility program takes no util_params (n_util_params must be 0)");
  if (m != c->prog.m) return prog_fail(who, "the resident utility program was built for m = %ld outputs, the model has %ld per hyper-sample", c->prog.m, m);
  if (theta_dim != c->prog.theta_dim) return prog_fail(who, "the resident utility program was built for theta_dim = %ld, the call has %ld", c->prog.theta_dim, theta_dim);
  return 0;
}

// entries <= 16: 256 threads, <= 32: 128, else 64 -- at most 32 KiB (40 KiB for the largest file) per workgroup, so that several
// workgroups share the 160 KiB of a compute unit (DESIGN section 14 has the occupancy table)
void util_prog_geometry(const UtilProg& p, int* threads, size_t* lds_bytes) {
  const int entries = p.m + p.n_slots;
  const int nt = entries <= 16 ? 256 : (entries <= 32 ? 128 : 64);
  *threads = nt;
  *lds_bytes = sizeof(double) * (size_t)entries * nt;
}

static UtilProgDev dev_view(const UtilProg& p) {
  UtilProgDev v{};
  const unsigned* code = p.dev + BOCF_PROG_HEADER_WORDS;
  v.val_code = reinterpret_cast<const uint2*>(code);
  v.grad_code = reinterpret_cast<const uint2*>(code + 2 * (size_t)p.n_val);
  v.consts = reinterpret_cast<const double*>(code + 2 * (size_t)(p.n_val + p.n_grad));
  v.m = p.m; v.n_slots = p.n_slots; v.n_val = p.n_val; v.n_grad = p.n_grad; v.val_out = p.val_out;
  for (int q = 0; q <= BOCF_MAX_M; ++q) v.grad_out[q] = p.grad_out[q];
  return v;
}

extern __shared__ __attribute__((aligned(16))) double prog_file[];   // (m + slots) x blockDim.x, entry-major

// ---------------------------------------------------------------------------------------------
// best_l = max_i U(theta_l, mu(X_i)): one workgroup per parameter, threads stride the evaluated points (best_so_far_kernel)
__global__ __launch_bounds__(256) void best_so_far_prog_kernel(const double* __restrict__ mu_train, int N, const double* __restrict__ theta, int theta_dim,
                                                               double* __restrict__ best, UtilProgDev p) {
  const int l = blockIdx.x, nt = blockDim.x, tid = threadIdx.x;
  const double* th = theta + (long)l * theta_dim;
  double* file = prog_file + tid;
  double mx = -INFINITY;
  for (int i0 = 0; i0 < N; i0 += nt) {                     // workgroup-uniform trip count
    const int i = min(i0 + tid, N - 1);
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < p.m) file[(long)j * nt] = mu_train[(long)j * N + i];
    prog_run(p.val_code, p.n_val, file, nt, p.m, th, p.consts);
    const double v = file[(long)(p.m + p.val_out) * nt];
    if (i0 + tid < N) mx = fmax(mx, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  __syncthreads();                                         // every thread is done with its column: the file is free
  if ((tid & 63) == 0) prog_file[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    double r = prog_file[0];
    for (int w = 1; w < nt / 64; ++w) r = fmax(r, prog_file[w]);
    best[l] = r;
  }
}

void launch_best_so_far_prog(const double* mu_train, int N, const double* theta, int theta_dim, int L, double* best, const UtilProg& p, hipStream_t s) {
  int nt;
  size_t lds;
  util_prog_geometry(p, &nt, &lds);
  BOCF_LAUNCH(best_so_far_prog_kernel, dim3((unsigned)L), dim3((unsigned)nt), lds, s, mu_train, N, theta, theta_dim, best, dev_view(p));
}

// ---------------------------------------------------------------------------------------------
// Monte-Carlo EI / PI (acq_mc_kernel): one wave per candidate, blockDim.x / 64 candidates per workgroup
__global__ __launch_bounds__(256) void acq_mc_prog_kernel(AcqArgs a, UtilProgDev p) {
  const int lane = threadIdx.x & 63, nt = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.x * (nt >> 6) + wave;
  if (c >= a.C) return;                                    // wave-uniform
  double* file = prog_file + threadIdx.x;
  double mu[BOCF_MAX_M], sg[BOCF_MAX_M];
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    mu[j] = j < p.m ? a.mean[(long)j * a.ld + c] : 0.0;
    sg[j] = j < p.m ? sqrt(a.var[(long)j * a.ld + c]) : 0.0;
  }
  double acq = 0.0;
  for (int l = 0; l < a.L; ++l) {
    const double* th = a.theta + (long)l * a.theta_dim;
    const double best = a.kind == BOCF_ACQ_EI ? a.best[l] : a.best[l] + 1e-6;
    double part = 0.0;
    for (int s0 = 0; s0 < a.S; s0 += 64) {
      const int s = min(s0 + lane, a.S - 1);
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j)
        if (j < p.m) file[(long)j * nt] = mu[j] + sg[j] * a.Wt[(long)j * a.S + s];
      prog_run(p.val_code, p.n_val, file, nt, p.m, th, p.consts);
      const double v = file[(long)(p.m + p.val_out) * nt];
      if (s0 + lane < a.S) {
        if (a.kind == BOCF_ACQ_EI) part += fmax(v - best, 0.0);
        else part += (v - best) > 0.0 ? 1.0 : 0.0;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    acq += (part / (double)a.S) * a.prob[l];
  }
  if (lane == 0) a.acq[c] = (a.accumulate ? a.acq[c] : 0.0) + acq * a.scale;
}

void launch_acq_mc_prog(const AcqArgs& a, hipStream_t s) {
  int nt;
  size_t lds;
  util_prog_geometry(*a.prog, &nt, &lds);
  const int per = nt / 64;
  BOCF_LAUNCH(acq_mc_prog_kernel, dim3((unsigned)((a.C + per - 1) / per)), dim3((unsigned)nt), lds, s, a, dev_view(*a.prog));
}

// Monte-Carlo EI with input gradients (acq_mc_grad_kernel).  The value section runs for every sample; the value+gradient section only in
// the sample rounds in which some lane improves (a wave-uniform vote), and only improving lanes accumulate.
__global__ __launch_bounds__(256) void acq_mc_grad_prog_kernel(AcqArgs a, UtilProgDev p) {
  const int lane = threadIdx.x & 63, nt = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.x * (nt >> 6) + wave;
  if (c >= a.C) return;
  double* file = prog_file + threadIdx.x;
  double mu[BOCF_MAX_M], sg[BOCF_MAX_M];
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    mu[j] = j < p.m ? a.mean[(long)j * a.ld + c] : 0.0;
    sg[j] = j < p.m ? sqrt(a.var[(long)j * a.ld + c]) : 1.0;
  }
  double acq = 0.0;
  double dq = 0.0;                                         // lane q < d accumulates d acq / dx_q
  for (int l = 0; l < a.L; ++l) {
    const double* th = a.theta + (long)l * a.theta_dim;
    const double best = a.best[l];
    double part = 0.0;
    double A[BOCF_MAX_M], Bc[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) { A[j] = 0.0; Bc[j] = 0.0; }
    for (int s0 = 0; s0 < a.S; s0 += 64) {
      const int s = min(s0 + lane, a.S - 1);
      const bool live = s0 + lane < a.S;
      double w[BOCF_MAX_M];
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j) {
        w[j] = j < p.m ? a.Wt[(long)j * a.S + s] : 0.0;
        if (j < p.m) file[(long)j * nt] = mu[j] + sg[j] * w[j];
      }
      prog_run(p.val_code, p.n_val, file, nt, p.m, th, p.consts);
      const double v = file[(long)(p.m + p.val_out) * nt];
      const bool imp = live && v > best;
      if (live) part += fmax(v - best, 0.0);
      if (__any(imp)) {                                    // wave-uniform
        prog_run(p.grad_code, p.n_grad, file, nt, p.m, th, p.consts);
        if (imp) {
#pragma unroll
          for (int j = 0; j < BOCF_MAX_M; ++j)
            if (j < p.m) {
              const double g = file[(long)(p.m + p.grad_out[1 + j]) * nt];
              A[j] += g;
              Bc[j] += g * (0.5 * w[j] / sg[j]);
            }
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) {
      if (j < p.m) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          A[j] += __shfl_xor(A[j], o, 64);
          Bc[j] += __shfl_xor(Bc[j], o, 64);
        }
      }
    }
    const double wgt = a.prob[l] / (double)a.S;
    acq += part * wgt;
    if (lane < a.d) {
      double t = 0.0;
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j)
        if (j < p.m) t += A[j] * a.dmean[((long)j * a.ldg + c) * a.d + lane] + Bc[j] * a.dvar[((long)j * a.ldg + c) * a.d + lane];
      dq += t * wgt;
    }
  }
  if (lane == 0) a.acq[c] = (a.accumulate ? a.acq[c] : 0.0) + acq * a.scale;
  if (lane < a.d) a.dacq[(long)c * a.d + lane] = (a.accumulate ? a.dacq[(long)c * a.d + lane] : 0.0) + dq * a.scale;
}

void launch_acq_mc_grad_prog(const AcqArgs& a, hipStream_t s) {
  int nt;
  size_t lds;
  util_prog_geometry(*a.prog, &nt, &lds);
  const int per = nt / 64;
  BOCF_LAUNCH(acq_mc_grad_prog_kernel, dim3((unsigned)((a.C + per - 1) / per)), dim3((unsigned)nt), lds, s, a, dev_view(*a.prog));
}

// ---------------------------------------------------------------------------------------------
// Monte-Carlo expected utility of the recommendation step (eu_kernel, mode BOCF_EU_MC): value, and gradient when a.grad is given
__global__ __launch_bounds__(256) void eu_prog_kernel(EuArgs a, UtilProgDev p) {
  const int lane = threadIdx.x & 63, nt = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.x * (nt >> 6) + wave;
  if (c >= a.C) return;                                    // wave-uniform
  double* file = prog_file + threadIdx.x;
  const int row = a.rows[c];
  const double* th = a.theta + (long)row * a.theta_dim;
  const bool grad = a.grad != nullptr;
  double mu[BOCF_MAX_M], sg[BOCF_MAX_M], A[BOCF_MAX_M], B[BOCF_MAX_M];
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    mu[j] = j < p.m ? a.mean[(long)j * a.ld + c] : 0.0;
    sg[j] = j < p.m ? sqrt(a.var[(long)j * a.ld + c]) : 1.0;
    A[j] = 0.0;
    B[j] = 0.0;
  }
  const double* Z = a.Zt + (long)row * p.m * a.S;         // (m, S) normals of this candidate's parameter
  double part = 0.0;
  for (int s0 = 0; s0 < a.S; s0 += 64) {
    const int s = min(s0 + lane, a.S - 1);
    const bool live = s0 + lane < a.S;
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < p.m) file[(long)j * nt] = mu[j] + sg[j] * Z[(long)j * a.S + s];
    if (grad) {                                            // the value+gradient section also leaves U
      prog_run(p.grad_code, p.n_grad, file, nt, p.m, th, p.consts);
      if (live) {
        part += file[(long)(p.m + p.grad_out[0]) * nt];
#pragma unroll
        for (int j = 0; j < BOCF_MAX_M; ++j)
          if (j < p.m) {
            const double g = file[(long)(p.m + p.grad_out[1 + j]) * nt];
            A[j] += g;
            B[j] += g * Z[(long)j * a.S + s];
          }
      }
    } else {
      prog_run(p.val_code, p.n_val, file, nt, p.m, th, p.consts);
      if (live) part += file[(long)(p.m + p.val_out) * nt];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
  if (grad) {
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) {
      if (j < p.m) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          A[j] += __shfl_xor(A[j], o, 64);
          B[j] += __shfl_xor(B[j], o, 64);
        }
        B[j] *= 0.5 / sg[j];                               // d sigma / dx = (d var / dx) / (2 sigma)  (cbo.py:218-219)
      }
    }
  }
  if (lane == 0) a.val[c] = (a.accumulate ? a.val[c] : 0.0) + part * a.scale;
  if (grad && lane < a.d) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < p.m) t += A[j] * a.dmean[((long)j * a.ldg + c) * a.d + lane] + B[j] * a.dvar[((long)j * a.ldg + c) * a.d + lane];
    a.grad[(long)c * a.d + lane] = (a.accumulate ? a.grad[(long)c * a.d + lane] : 0.0) + t * a.scale;
  }
}

void launch_eu_prog(const EuArgs& a, hipStream_t s) {
  int nt;
  size_t lds;
  util_prog_geometry(*a.prog, &nt, &lds);
  const int per = nt / 64;
  BOCF_LAUNCH(eu_prog_kernel, dim3((unsigned)((a.C + per - 1) / per)), dim3((unsigned)nt), lds, s, a, dev_view(*a.prog));
}

// ---------------------------------------------------------------------------------------------
// u[s][c] = U(theta_s, F[:, c, s]) for the S paths of one sample block F (m, C, S): a thread per candidate (thompson_util_kernel)
__global__ __launch_bounds__(256) void thompson_util_prog_kernel(const double* __restrict__ F, int C, int S, const double* __restrict__ theta, int theta_dim,
                                                                 double* __restrict__ u, long ldu, UtilProgDev p) {
  const int s = blockIdx.y, nt = blockDim.x;
  const int c = blockIdx.x * nt + threadIdx.x;
  const int cc = min(c, C - 1);                            // every thread runs the program: the branches stay uniform
  double* file = prog_file + threadIdx.x;
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j)
    if (j < p.m) file[(long)j * nt] = F[((long)j * C + cc) * S + s];
  prog_run(p.val_code, p.n_val, file, nt, p.m, theta + (long)s * theta_dim, p.consts);
  if (c < C) u[(long)s * ldu + c] = file[(long)(p.m + p.val_out) * nt];
}

void launch_thompson_util_prog(const double* F, int C, int S, const double* theta, int theta_dim, double* u, long ldu, const UtilProg& p, hipStream_t s) {
  int nt;
  size_t lds;
  util_prog_geometry(p, &nt, &lds);
  BOCF_LAUNCH(thompson_util_prog_kernel, dim3((unsigned)((C + nt - 1) / nt), (unsigned)S), dim3((unsigned)nt), lds, s, F, C, S, theta, theta_dim, u, ldu,
              dev_view(p));
}

// ---------------------------------------------------------------------------------------------
// Utility of a row's path values and the chain rule (path_chain_kernel): a thread per row, the value+gradient section when a gradient is
// wanted (it also leaves U), else the value section
__global__ __launch_bounds__(256) void path_chain_prog_kernel(const double* __restrict__ pv, const double* __restrict__ pg, int d, int C,
                                                              const int* __restrict__ row_path, const double* __restrict__ theta, int theta_dim,
                                                              double* __restrict__ val, double* __restrict__ grad, UtilProgDev p) {
  const int nt = blockDim.x;
  const int c = blockIdx.x * nt + threadIdx.x;
  const int cc = min(c, C - 1);                            // every thread runs the program: the branches stay uniform
  double* file = prog_file + threadIdx.x;
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j)
    if (j < p.m) file[(long)j * nt] = pv[(long)cc * p.m + j];
  const double* th = theta + (long)row_path[cc] * theta_dim;
  if (!grad) {
    prog_run(p.val_code, p.n_val, file, nt, p.m, th, p.consts);
    if (c < C) val[c] = file[(long)(p.m + p.val_out) * nt];
    return;
  }
  prog_run(p.grad_code, p.n_grad, file, nt, p.m, th, p.consts);
  if (c >= C) return;
  val[c] = file[(long)(p.m + p.grad_out[0]) * nt];
  for (int q = 0; q < d; ++q) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < p.m) t += file[(long)(p.m + p.grad_out[1 + j]) * nt] * pg[((long)c * p.m + j) * d + q];
    grad[(long)c * d + q] = t;
  }
}

void launch_path_chain_prog(const double* pv, const double* pg, int d, int C, const int* row_path, const double* theta, int theta_dim, double* val,
                            double* grad, const UtilProg& p, hipStream_t s) {
  int nt;
  size_t lds;
  util_prog_geometry(p, &nt, &lds);
  BOCF_LAUNCH(path_chain_prog_kernel, dim3((unsigned)((C + nt - 1) / nt)), dim3((unsigned)nt), lds, s, pv, pg, d, C, row_path, theta, theta_dim, val, grad,
              dev_view(p));
}
