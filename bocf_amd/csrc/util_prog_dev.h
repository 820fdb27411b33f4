// Device interpreter of a utility program (include/bocf_hip.h, "utility programs"): the forward evaluator of one straight-line section,
// used by the kernels of util_prog.hip.  The program is the same for every lane of a launch: instruction words, parameters and constants
// are read through uniform (scalar) loads and the opcode switch is a uniform branch, so the lanes never diverge.  What differs per lane --
// the inputs y_j and the value slots -- lives in LDS, entry e of thread t at file[e * threads + t]: a runtime-indexed private array would
// go to scratch, and with this layout consecutive lanes touch consecutive 8-byte words (conflict-free 64-bit LDS accesses).  Entries
// [0, m) are the inputs, [m, m + slots) the value slots.
// Only programs that bocf_check_utility_program accepted reach a launch: every index below is within the file / the argument arrays and
// the loop count is the validated one.
#pragma once
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"

// what a kernel needs of the resident program, by value (host-validated numbers, device pointers)
struct UtilProgDev {
  const uint2* val_code;      // value section
  const uint2* grad_code;     // value+gradient section
  const double* consts;
  int m, n_slots, n_val, n_grad;
  int val_out;                // slot of U after the value section
  int grad_out[1 + BOCF_MAX_M];   // slot of U, then of dU/dy_j, after the value+gradient section
};

__device__ __forceinline__ double prog_operand(unsigned o, const double* file, int stride, int m, const double* __restrict__ theta,
                                               const double* __restrict__ consts) {
  const unsigned kind = o >> 14, idx = o & 0x3fffu;
  if (kind == BOCF_OPERAND_PARAM) return theta[idx];
  if (kind == BOCF_OPERAND_CONST) return consts[idx];
  return file[(long)(kind == BOCF_OPERAND_SLOT ? m + idx : idx) * stride];
}

// runs n instructions of `code` on this thread's column of the file (file = base + thread index, stride = threads per workgroup)
__device__ __forceinline__ void prog_run(const uint2* __restrict__ code, int n, double* file, int stride, int m, const double* __restrict__ theta,
                                         const double* __restrict__ consts) {
#pragma clang fp contract(off)
  for (int i = 0; i < n; ++i) {
    const uint2 w = code[i];
    const unsigned op = w.x & 0xffu, dst = w.x >> 8;
    const double a = prog_operand(w.y & 0xffffu, file, stride, m, theta, consts);
    const double b = prog_operand(w.y >> 16, file, stride, m, theta, consts);
    double r;
    switch (op) {
      case BOCF_OP_ADD: r = a + b; break;
      case BOCF_OP_SUB: r = a - b; break;
      case BOCF_OP_MUL: r = a * b; break;
      case BOCF_OP_DIV: r = a / b; break;
      case BOCF_OP_NEG: r = -a; break;
      case BOCF_OP_ABS: r = fabs(a); break;
      case BOCF_OP_SIGN: r = a > 0.0 ? 1.0 : (a < 0.0 ? -1.0 : (a == 0.0 ? 0.0 : a)); break;
      case BOCF_OP_SQRT: r = sqrt(a); break;
      case BOCF_OP_EXP: r = exp(a); break;
      case BOCF_OP_LOG: r = log(a); break;
      case BOCF_OP_SIN: r = sin(a); break;
      case BOCF_OP_COS: r = cos(a); break;
      case BOCF_OP_TANH: r = tanh(a); break;
      case BOCF_OP_POW: r = pow(a, b); break;
      case BOCF_OP_MIN: r = fmin(a, b); break;
      case BOCF_OP_MAX: r = fmax(a, b); break;
      default: r = a >= b ? 1.0 : 0.0; break;          // BOCF_OP_GE
    }
    file[(long)(m + dst) * stride] = r;
  }
}
