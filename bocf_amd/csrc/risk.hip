// Quantile and tail-mean acquisitions of a composite utility (definitions: include/bocf_hip.h): an exact order
// statistic of the S Monte-Carlo samples u_s = U(theta_l, mu + sigma o W_s) of one candidate, and below it the closed-form confidence
// bound of a linear utility.
// Geometry of acq_mc_m_kernel (acq.hip): one wave per candidate, four per workgroup, lanes stride the S samples, no atomics and no
// barrier -- a candidate's bits do not depend on its batch.
// Where the samples live: in LDS, as their monotone 64-bit keys.  Every utility is evaluated ONCE per theta_l; lane t writes the keys of the
// samples s = t, t + 64, ... into its wave's S-word strip of the dynamic LDS (4 S words per workgroup, 128 KiB at the limit S = 4096) and
// only ever reads those words back, so the strip is lane-private storage: no cross-lane hand-off through LDS and consecutive lanes on
// consecutive banks.  (Registers would need a compile-time slot count: 64 guarded slots for every S, or an instantiation per count.)  One
// slot is also kept in a register: the last, partial one -- the only one in which a lane may have no sample -- so the selection reads the
// full slots unguarded, and for S <= 64 it runs out of that register alone.  Occupancy at large S is the strip's: 32 S bytes of LDS per
// workgroup against 160 KiB per compute unit leave 2 workgroups (8 waves) per unit at S = 2048 and 1 (4 waves) at S = 4096; up to
// S = 640 the LDS admits the 8 workgroups a unit's 32 wave slots hold, and the registers decide.
// Selection: a radix descent over the key, most significant bit first.  The key maps doubles to unsigned integers in the total order (-0.0
// is +0.0, a NaN is -inf).  Round b counts the samples that agree with the prefix found so far and have bit b clear: a compare per sample
// whose wave-wide result IS the ballot, one population count and one add per slot, all scalar -- no shuffle and no LDS reduction.  After 64
// rounds the prefix is the key of u_(k) and the remaining rank r says that s*(k) is the r-th sample with that key in index order, found
// by one more pass of ballots (slot-major, lane-minor = index order).  The count per round is a property of the multiset of keys: the
// result does not depend on how the samples are spread over the lanes, and nothing is compared across an unsorted boundary.
// Tail kinds: one more pass with the threshold (key of u_(k), s*(k)) known; the members are summed with an error-free transformation
// (two-sum) per lane and across the butterfly -- the rounding errors of the partial sums are carried along and added back once at the
// end -- so the mean of a tail whose members cancel is as good as that of one whose members do not.
// The gradient form recomputes y_s and dU/dy only for the members of the selected set.
#include "bocf_internal.h"
#include "../../include/bocf_hip.h"
#include "utility_dev.h"
#include "cacq_dev.h"   // wave_uniform
#include <atomic>

// doubles -> unsigned integers, monotone in the total order of the header: NaN -> the key of -inf, -0.0 -> the key of +0.0
__device__ __forceinline__ unsigned long long risk_key(double u) {
  if (u != u) u = -INFINITY;
  if (u == 0.0) u = 0.0;
  const unsigned long long b = (unsigned long long)__double_as_longlong(u);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double risk_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
// s + e = a + b exactly (for finite s)
__device__ __forceinline__ void risk_two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// (MC = the output count as a template argument, 1 ... 8, or 0 = read it from the arguments, m <= 16)
template <int MC, bool GRAD>
__global__ __launch_bounds__(256) void risk_kernel(RiskArgs a) {
  extern __shared__ unsigned long long risk_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.x * 4 + wave;
  if (c >= a.C) return;                         // wave-uniform
  const int m_ = MC > 0 ? MC : a.m;
  constexpr int MM = MC > 0 ? MC : BOCF_MAX_M;
  const int S = a.S, k = a.rank;
  const int nslot = (S + 63) >> 6, nfull = S >> 6;     // slots in all, and those in which every lane has a sample
  const bool vtail = lane + 64 * nfull < S;            // this lane has a sample in the last, partial slot
  unsigned long long* __restrict__ keys = risk_lds + (size_t)wave * S;       // this wave's strip: words [0, S)
  double mu[MM], sg[MM];
#pragma unroll
  for (int j = 0; j < MM; ++j) {
    const bool on = MC > 0 || j < m_;
    mu[j] = on ? wave_uniform(a.mean[(long)j * a.ld + c]) : 0.0;
    sg[j] = on ? wave_uniform(sqrt(a.var[(long)j * a.ld + c])) : 1.0;
  }
  const int nT = a.kind == BOCF_RISK_QUANTILE ? 1 : (a.kind == BOCF_RISK_UPPER_TAIL ? S - k : k + 1);
  double acq = 0.0;
  double dq = 0.0;                              // lane q < d accumulates d alpha / dx_q
  for (int l = 0; l < a.L; ++l) {
    const double* th = a.theta + (long)l * a.theta_dim;
    // 1. the S utilities, once.  The last, partial slot (all of them for S < 64) also stays in a register: only there a lane may have no
    // sample, so the rounds below read the full slots without a guard, and for S <= 64 they read no LDS at all
    unsigned long long ktail = 0;
    for (int i = 0; i < nslot; ++i) {
      const int s = lane + 64 * i;
      if (s < S) {
        double y[BOCF_MAX_M];
#pragma unroll
        for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = 0.0;
#pragma unroll
        for (int j = 0; j < MM; ++j)
          if (MC > 0 || j < m_) y[j] = mu[j] + sg[j] * a.Wt[(long)j * S + s];
        const unsigned long long key = risk_key(utility_eval(a.util_kind, th, a.util_params, y, m_));
        keys[s] = key;
        if (i == nfull) ktail = key;
      }
    }
    // 2. the key of u_(k): r = rank among the samples that agree with the prefix
    unsigned long long prefix = 0;
    int r = k;
    for (int b = 63; b >= 0; --b) {
      int c0 = __popcll(__builtin_amdgcn_ballot_w64(vtail && ((ktail ^ prefix) >> b) == 0));
      // (four reads in flight: unrolled by hand, the compiler does not unroll a loop with a ballot in it by a run-time count)
      int i = 0;
      for (; i + 4 <= nfull; i += 4) {
        const unsigned long long k0 = keys[lane + 64 * i], k1 = keys[lane + 64 * (i + 1)], k2 = keys[lane + 64 * (i + 2)], k3 = keys[lane + 64 * (i + 3)];
        c0 += __popcll(__builtin_amdgcn_ballot_w64(((k0 ^ prefix) >> b) == 0)) + __popcll(__builtin_amdgcn_ballot_w64(((k1 ^ prefix) >> b) == 0)) +
              __popcll(__builtin_amdgcn_ballot_w64(((k2 ^ prefix) >> b) == 0)) + __popcll(__builtin_amdgcn_ballot_w64(((k3 ^ prefix) >> b) == 0));
      }
      for (; i < nfull; ++i) c0 += __popcll(__builtin_amdgcn_ballot_w64(((keys[lane + 64 * i] ^ prefix) >> b) == 0));
      if (r >= c0) {
        r -= c0;
        prefix |= 1ull << b;
      }
    }
    // 3. s*(k): the r-th sample with that key, in index order
    int sstar = -1;
    for (int i = 0; i < nslot && sstar < 0; ++i) {
      const bool eq = i < nfull ? keys[lane + 64 * i] == prefix : (vtail && ktail == prefix);
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(eq);
      const int cnt = __popcll(mask);
      if (r < cnt) {
        const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(eq && before == r);
        sstar = 64 * i + (__ffsll((unsigned long long)hit) - 1);
      } else {
        r -= cnt;
      }
    }
    // 4. the value, and the pathwise gradient over the selected set
    double rho = risk_unkey(prefix);
    if (GRAD || a.kind != BOCF_RISK_QUANTILE) {
      double hs = 0.0, he = 0.0;
      double Aj[MM], Bj[MM];
#pragma unroll
      for (int j = 0; j < MM; ++j) { Aj[j] = 0.0; Bj[j] = 0.0; }
      for (int i = 0; i < nslot; ++i) {
        const int s = lane + 64 * i;
        if (s >= S) continue;
        const unsigned long long key = keys[s];
        bool in;
        if (a.kind == BOCF_RISK_QUANTILE) in = s == sstar;
        else if (a.kind == BOCF_RISK_UPPER_TAIL) in = key > prefix || (key == prefix && s >= sstar);
        else in = key < prefix || (key == prefix && s <= sstar);
        if (!in) continue;
        double e;
        risk_two_sum(hs, risk_unkey(key), hs, e);
        he += e;
        if (GRAD) {
          double y[BOCF_MAX_M], g[BOCF_MAX_M], w[MM];
#pragma unroll
          for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = 0.0;
#pragma unroll
          for (int j = 0; j < MM; ++j) {
            w[j] = (MC > 0 || j < m_) ? a.Wt[(long)j * S + s] : 0.0;
            if (MC > 0 || j < m_) y[j] = mu[j] + sg[j] * w[j];
          }
          utility_grad(a.util_kind, th, a.util_params, y, m_, g);
#pragma unroll
          for (int j = 0; j < MM; ++j) {
            Aj[j] += g[j];
            Bj[j] += g[j] * (0.5 * w[j] / sg[j]);
          }
        }
      }
      if (a.kind != BOCF_RISK_QUANTILE) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const double os = __shfl_xor(hs, o, 64), oe = __shfl_xor(he, o, 64);
          double e;
          risk_two_sum(hs, os, hs, e);
          he = (he + oe) + e;
        }
        // (an infinite member makes the error terms NaN: the plain sum is the answer then)
        rho = (isfinite(hs) ? hs + he : hs) / (double)nT;
      }
      if (GRAD) {
        double tq = 0.0;
#pragma unroll
        for (int j = 0; j < MM; ++j)
          if (MC > 0 || j < m_) {
            double As = Aj[j], Bs = Bj[j];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
              As += __shfl_xor(As, o, 64);
              Bs += __shfl_xor(Bs, o, 64);
            }
            if (lane < a.d) tq += As * a.dmean[((long)j * a.ldg + c) * a.d + lane] + Bs * a.dvar[((long)j * a.ldg + c) * a.d + lane];
          }
        dq += (tq / (double)nT) * a.prob[l];
      }
    }
    acq += rho * a.prob[l];
  }
  if (lane == 0) a.acq[c] = (a.accumulate ? a.acq[c] : 0.0) + acq * a.scale;
  if (GRAD && lane < a.d) a.dacq[(long)c * a.d + lane] = (a.accumulate ? a.dacq[(long)c * a.d + lane] : 0.0) + dq * a.scale;
}

// Closed-form confidence bound of theta . f(x): thread per candidate, as acq_linear_grad_kernel (acq.hip).
//   value: theta^T mu + kappa sqrt(sum_j theta_j^2 var_j);  gradient: theta^T dmu + kappa (sum_j theta_j^2 dvar_j) / (2 sqrt(sum_j theta_j^2 var_j))
template <bool GRAD>
__global__ __launch_bounds__(256) void linear_ucb_kernel(RiskArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.C) return;
  double mean[BOCF_MAX_M], var[BOCF_MAX_M];
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j) {
    mean[j] = j < a.m ? a.mean[(long)j * a.ld + c] : 0.0;
    var[j] = j < a.m ? a.var[(long)j * a.ld + c] : 0.0;
  }
  double acq = 0.0;
  if (GRAD && !a.accumulate)
    for (int q = 0; q < a.d; ++q) a.dacq[(long)c * a.d + q] = 0.0;
  for (int l = 0; l < a.L; ++l) {
    const double* th = a.theta + (long)l * a.theta_dim;
    double mu = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j)
      if (j < a.m) {
        mu += th[j] * mean[j];
        s2 += (th[j] * th[j]) * var[j];
      }
    const double sigma = sqrt(s2);
    acq += (mu + a.kappa * sigma) * a.prob[l];
    if (GRAD)
      for (int q = 0; q < a.d; ++q) {
        double dmu = 0.0, dv = 0.0;
#pragma unroll
        for (int j = 0; j < BOCF_MAX_M; ++j)
          if (j < a.m) {
            dmu += th[j] * a.dmean[((long)j * a.ldg + c) * a.d + q];
            dv += (th[j] * th[j]) * a.dvar[((long)j * a.ldg + c) * a.d + q];
          }
        const double dsig = sigma > 0.0 ? 0.5 * dv / sigma : 0.0;       // (theta = 0: the bound is flat)
        a.dacq[(long)c * a.d + q] += ((dmu + a.kappa * dsig) * a.prob[l]) * a.scale;
      }
  }
  a.acq[c] = (a.accumulate ? a.acq[c] : 0.0) + acq * a.scale;
}

// One launch of risk_kernel<M, G>.  A strip set above the default dynamic-LDS limit has to be asked for: once per instantiation and
// device, for the largest set there is (S = BOCF_RISK_MAX_SAMPLES), not per launch -- the acquisition is called hundreds of times per
// refinement.  `asked` holds one bit per device; two threads that both find it clear both ask, which is harmless.
template <int M, bool G>
static void risk_launch(const RiskArgs& a, hipStream_t s) {
  static std::atomic<unsigned long long> asked{0};
  const dim3 grid((unsigned)((a.C + 3) / 4));
  const size_t lds = sizeof(unsigned long long) * 4 * (size_t)a.S;
  if (lds > 48 * 1024) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (e == hipSuccess && (dev > 63 || !(asked.load() & bit))) {
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(&risk_kernel<M, G>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(sizeof(unsigned long long) * 4 * BOCF_RISK_MAX_SAMPLES));
      if (e == hipSuccess && dev <= 63) asked.fetch_or(bit);
    }
    if (e != hipSuccess) {
      bocf_note_launch("risk_kernel (dynamic LDS)", e);
      return;
    }
  }
  BOCF_LAUNCH((risk_kernel<M, G>), grid, dim3(256), lds, s, a);
}

void launch_risk(const RiskArgs& a, bool grad, hipStream_t s) {
  if (a.C == 0) return;
  if (a.S < 1 || a.S > BOCF_RISK_MAX_SAMPLES || a.rank < 0 || a.rank >= a.S) {      // (the entry point refuses these by name)
    bocf_note_launch("risk_kernel", hipErrorInvalidValue);
    return;
  }
  switch (a.m >= 1 && a.m <= 8 ? a.m : 0) {
#define LM(M) case M: if (grad) risk_launch<M, true>(a, s); else risk_launch<M, false>(a, s); break;
    LM(1) LM(2) LM(3) LM(4) LM(5) LM(6) LM(7) LM(8) default: LM(0)
#undef LM
  }
}

void launch_linear_ucb(const RiskArgs& a, bool grad, hipStream_t s) {
  if (a.C == 0) return;
  const dim3 grid((unsigned)((a.C + 255) / 256));
  if (grad) BOCF_LAUNCH((linear_ucb_kernel<true>), grid, dim3(256), 0, s, a);
  else BOCF_LAUNCH((linear_ucb_kernel<false>), grid, dim3(256), 0, s, a);
}
