// Log-space expected improvement (definitions: include/bocf_hip.h): log EI of a linear utility in closed form, and the
// log of a smooth fat-tailed surrogate of the Monte-Carlo EI of a composite utility.  Both are finite and have a useful gradient where EI
// itself underflows to an exact zero.
// Every kernel closes the whole mixture -- hyper-samples h, parameters l and (Monte-Carlo) samples s -- in ONE launch as a log-sum-exp in a
// fixed order: all H m rows of the posterior are resident, so nothing is combined across launches.
//   closed form: thread per candidate (acq_linear_kernel); one pass over (h, l) in index order for the maximum, one for the sums.
//   Monte-Carlo: one wave per candidate, four per workgroup, lanes stride the samples (acq_mc_m_kernel).  Per hyper-sample every lane keeps a
//     running (max, sum, A_j, B_j) that it rescales whenever its maximum grows; the wave's maximum meets in the fixed __shfl_xor
//     butterfly, every lane rescales to it, the sums meet in the same butterfly, and the wave folds the hyper-sample into the mixture so
//     far.  No atomics, no barrier, no LDS: a candidate's bits do not depend on its batch.
//   utility programs: the same with the user's traced utility run through the interpreter of util_prog_dev.h (inputs and slots in LDS,
//     entry-major; util_prog_geometry for threads and LDS; a uniform trip count with masked lanes); the value+gradient section runs only in
//     the gradient form, where every live sample carries weight (it also leaves U), the value section otherwise.
#include "logei.h"
#include "../../include/bocf_hip.h"
#include "utility_dev.h"
#include "util_prog_dev.h"
#include "cacq_dev.h"   // wave_uniform

#define LG_INV_SQRT2 0.70710678118654752440
#define LG_INV_SQRT_2PI 0.39894228040143267794
#define LG_HALF_LOG_2PI 0.91893853320467274178
#define LG_SQRT_HALF_PI 1.25331413731550025121
#define LG_LOG_0_1 (-2.30258509299404568402)
#define LG_LOG_0_2 (-1.60943791243410037460)
#define LG_SERIES_FROM 30.0

// log h(z) and r(z) = Phi(z) / h(z) for h(z) = phi(z) + z Phi(z), accurate for every finite z.  For z <= -1: h = phi(z) g(z) with
// g = 1 - |z| R(z), R = Phi / phi = sqrt(pi / 2) erfcx(|z| / sqrt 2).  The direct difference loses a relative eps z^2, so from |z| = 30 on
// g comes from its asymptotic series sum_{k >= 1} (-1)^(k+1) (2k - 1)!! / z^(2k), 12 terms (the 12th is below 1e-21 of the first there).
__device__ __forceinline__ void logei_log_h(double z, double& logh, double& r) {
  if (z > -1.0) {
    const double Phi = 0.5 * erfc(-z * LG_INV_SQRT2);
    const double h = exp(-0.5 * z * z) * LG_INV_SQRT_2PI + z * Phi;
    logh = log(h);
    r = Phi / h;
    return;
  }
  const double az = -z;
  const double R = LG_SQRT_HALF_PI * erfcx(az * LG_INV_SQRT2);
  double g;
  if (az < LG_SERIES_FROM) {
    g = 1.0 - az * R;
  } else {
    const double x = 1.0 / (z * z);
    g = x * (1.0 + x * (-3.0 + x * (15.0 + x * (-105.0 + x * (945.0 + x * (-10395.0 + x * (135135.0 + x * (-2027025.0 + x * (34459425.0 +
        x * (-654729075.0 + x * (13749310575.0 + x * -316234143225.0)))))))))));
  }
  logh = -0.5 * z * z - LG_HALF_LOG_2PI + log(g);
  r = R / g;
}

// log psi(t) and psi'(t) / psi(t) for psi(t) = softplus(t) + 0.1 / (1 + t^2), finite for every finite t: log softplus(t) -> t for t << 0,
// log(1 + t^2) = 2 log |t| for huge |t|, and the ratio assembled from logarithms so that neither psi nor psi' has to be representable.
template <bool RATIO>
__device__ __forceinline__ void logei_log_psi(double t, double& lpsi, double& ratio) {
  const double at = fabs(t);
  const double l1p = log1p(exp(-at));
  double lsp;                                              // log softplus(t)
  if (t > 0.0) lsp = log(t + l1p);
  else if (t > -37.0) lsp = log(l1p);
  else lsp = t;                                            // log(e^t - e^2t / 2 + ...) = t - e^t / 2 ...: below 5e-17 from t here
  const double lq = at < 1e10 ? log1p(t * t) : 2.0 * log(at);
  const double lc = LG_LOG_0_1 - lq;
  const double hi = fmax(lsp, lc), lo = fmin(lsp, lc);
  lpsi = hi + log1p(exp(lo - hi));
  if (RATIO) {
    // psi' = sigmoid(t) - 0.2 t / (1 + t^2)^2, log sigmoid(t) = min(t, 0) - log1p(e^-|t|)
    const double tail = at > 0.0 ? exp(LG_LOG_0_2 + log(at) - 2.0 * lq - lpsi) : 0.0;
    ratio = exp(fmin(t, 0.0) - l1p - lpsi) + (t > 0.0 ? -tail : tail);
  }
}

// one more term e of a running log-sum-exp (mx, sum): sc rescales what was accumulated so far, wgt is the term's weight
__device__ __forceinline__ void logei_push(double e, double& mx, double& sum, double& sc, double& wgt) {
  const double nm = fmax(mx, e);
  sc = exp(mx - nm);
  wgt = exp(e - nm);
  sum = sum * sc + wgt;
  mx = nm;
}
__device__ __forceinline__ double logei_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double logei_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------
// closed form: l_lh = log sigma + log h(z), z = (mu - best_l) / sigma with no floor on sigma; log alpha = LSE_(h, l) [log p_l - log H + l_lh];
// the gradient is sum_(h, l) w_lh (dsigma / sigma + r(z) (dmu - z dsigma) / sigma) with the softmax weights w_lh -- the exact derivative of
// the value.  A term with p_l = 0 or sigma = 0 is -inf and carries no weight; all of them -inf: value -inf, gradient 0.
struct LogEiTerm { double e, sigma, z, r; };

__device__ __forceinline__ LogEiTerm logei_linear_term(const LogEiArgs& a, const double (&mean)[BOCF_MAX_M], const double (&var)[BOCF_MAX_M], int h, int l,
                                                       double logH) {
  LogEiTerm t{-INFINITY, 0.0, 0.0, 0.0};
  const double pl = a.prob[l];
  if (!(pl > 0.0)) return t;
  const double* th = a.theta + (long)l * a.theta_dim;
  double mu = 0.0, s2 = 0.0;
#pragma unroll
  for (int j = 0; j < BOCF_MAX_M; ++j)
    if (j < a.m) {
      mu += th[j] * mean[j];
      s2 += (th[j] * th[j]) * var[j];
    }
  t.sigma = sqrt(s2);
  if (!(t.sigma > 0.0)) return t;
  t.z = (mu - a.best[(long)h * a.best_stride + l]) / t.sigma;
  double lh;
  logei_log_h(t.z, lh, t.r);
  t.e = (log(pl) - logH) + (log(t.sigma) + lh);
  return t;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void logei_linear_kernel(LogEiArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.C) return;
  const double logH = log((double)a.H);
  double mean[BOCF_MAX_M], var[BOCF_MAX_M];
  double M = -INFINITY;
  for (int h = 0; h < a.H; ++h) {
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) {
      mean[j] = j < a.m ? a.mean[((long)h * a.m + j) * a.ld + c] : 0.0;
      var[j] = j < a.m ? a.var[((long)h * a.m + j) * a.ld + c] : 0.0;
    }
    for (int l = 0; l < a.L; ++l) M = fmax(M, logei_linear_term(a, mean, var, h, l, logH).e);
  }
  if (GRAD)
    for (int q = 0; q < a.d; ++q) a.dacq[(long)c * a.d + q] = 0.0;
  if (!(M > -INFINITY)) {
    a.acq[c] = -INFINITY;
    return;
  }
  double sum = 0.0;
  for (int h = 0; h < a.H; ++h) {
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) {
      mean[j] = j < a.m ? a.mean[((long)h * a.m + j) * a.ld + c] : 0.0;
      var[j] = j < a.m ? a.var[((long)h * a.m + j) * a.ld + c] : 0.0;
    }
    for (int l = 0; l < a.L; ++l) {
      const LogEiTerm t = logei_linear_term(a, mean, var, h, l, logH);
      if (!(t.e > -INFINITY)) continue;
      const double w = exp(t.e - M);
      sum += w;
      if (GRAD) {
        const double* th = a.theta + (long)l * a.theta_dim;
        for (int q = 0; q < a.d; ++q) {
          double dmu = 0.0, dv = 0.0;
#pragma unroll
          for (int j = 0; j < BOCF_MAX_M; ++j)
            if (j < a.m) {
              dmu += th[j] * a.dmean[(((long)h * a.m + j) * a.ldg + c) * a.d + q];
              dv += (th[j] * th[j]) * a.dvar[(((long)h * a.m + j) * a.ldg + c) * a.d + q];
            }
          const double dsig = 0.5 * dv / t.sigma;
          a.dacq[(long)c * a.d + q] += w * ((dsig + t.r * (dmu - t.z * dsig)) / t.sigma);
        }
      }
    }
  }
  a.acq[c] = M + log(sum);
  if (GRAD)
    for (int q = 0; q < a.d; ++q) a.dacq[(long)c * a.d + q] /= sum;
}

void launch_logei_linear(const LogEiArgs& a, bool grad, hipStream_t s) {
  if (a.C == 0) return;
  const dim3 grid((unsigned)((a.C + 255) / 256));
  if (grad) BOCF_LAUNCH((logei_linear_kernel<true>), grid, dim3(256), 0, s, a);
  else BOCF_LAUNCH((logei_linear_kernel<false>), grid, dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------------------------
// Monte-Carlo: log alpha_tau = LSE_(h, l, s) [log p_l - log(H S) + log tau + log psi(t)], t = (U(theta_l, mu_h + sigma_h o W_s) - best_l) / tau.
// The gradient is pathwise through y as acq_mc_grad_kernel assembles it: per output A_j = sum w rho dU/dy_j and B_j = sum w rho dU/dy_j
// W_sj / (2 sigma_j) with w the softmax weight and rho = psi'(t) / (tau psi(t)); lane q < d owns coordinate q.  A sample whose term is not
// finite (a NaN or infinite utility) carries no weight.
// What the wave does with one hyper-sample once its lanes hold (mx, sum[, A, B]): see the head of the file.
struct LogEiMix { double M, S, dq; };                      // the mixture so far: maximum, sum relative to it, lane q's gradient sum relative to it

__device__ __forceinline__ double logei_lane_scale(double mx, double Mh) { return mx > -INFINITY ? exp(mx - Mh) : 0.0; }

// (MC = the output count as a template argument, 1 ... 8, or 0 = read it from the arguments, m <= 16)
template <int MC, bool GRAD>
__global__ __launch_bounds__(256) void logei_mc_kernel(LogEiArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.x * 4 + wave;
  if (c >= a.C) return;                         // wave-uniform
  const int m_ = MC > 0 ? MC : a.m;
  constexpr int MM = MC > 0 ? MC : BOCF_MAX_M;
  const double lnorm = log(a.tau) - log((double)a.H * (double)a.S);
  LogEiMix mix{-INFINITY, 0.0, 0.0};
  for (int h = 0; h < a.H; ++h) {
    double mu[MM], sg[MM];
#pragma unroll
    for (int j = 0; j < MM; ++j) {
      const bool on = MC > 0 || j < m_;
      mu[j] = on ? wave_uniform(a.mean[((long)h * m_ + j) * a.ld + c]) : 0.0;
      sg[j] = on ? wave_uniform(sqrt(a.var[((long)h * m_ + j) * a.ld + c])) : 1.0;
    }
    double mx = -INFINITY, sum = 0.0;
    double A[MM], B[MM];
#pragma unroll
    for (int j = 0; j < MM; ++j) { A[j] = 0.0; B[j] = 0.0; }
    for (int l = 0; l < a.L; ++l) {
      const double pl = a.prob[l];
      if (!(pl > 0.0)) continue;                // wave-uniform: the term is -inf
      const double* th = a.theta + (long)l * a.theta_dim;
      const double lw = log(pl) + lnorm, best = a.best[(long)h * a.best_stride + l];
      for (int s = lane; s < a.S; s += 64) {
        double y[BOCF_MAX_M], w[MM];
#pragma unroll
        for (int j = 0; j < BOCF_MAX_M; ++j) y[j] = 0.0;
#pragma unroll
        for (int j = 0; j < MM; ++j) {
          w[j] = (MC > 0 || j < m_) ? a.Wt[(long)j * a.S + s] : 0.0;
          if (MC > 0 || j < m_) y[j] = mu[j] + sg[j] * w[j];
        }
        const double t = (utility_eval(a.util_kind, th, a.util_params, y, m_) - best) / a.tau;
        double lpsi, ratio = 0.0;
        logei_log_psi<GRAD>(t, lpsi, ratio);
        const double e = lw + lpsi;
        if (e > -INFINITY && e < INFINITY) {
          double sc, wgt;
          logei_push(e, mx, sum, sc, wgt);
          if (GRAD) {
            double g[BOCF_MAX_M];
            utility_grad(a.util_kind, th, a.util_params, y, m_, g);
            const double coef = wgt * (ratio / a.tau);
#pragma unroll
            for (int j = 0; j < MM; ++j) {
              A[j] = A[j] * sc + coef * g[j];
              B[j] = B[j] * sc + coef * (g[j] * (0.5 * w[j] / sg[j]));
            }
          }
        }
      }
    }
    const double Mh = logei_wave_max(mx);
    if (!(Mh > -INFINITY)) continue;            // wave-uniform: every term of this hyper-sample is -inf
    const double sc = logei_lane_scale(mx, Mh);
    const double Sh = logei_wave_sum(sum * sc);
    const double nM = fmax(mix.M, Mh);
    const double s0 = exp(mix.M - nM), s1 = exp(Mh - nM);
    mix.S = mix.S * s0 + Sh * s1;
    mix.M = nM;
    if (GRAD) {
      double tq = 0.0;
#pragma unroll
      for (int j = 0; j < MM; ++j)
        if (MC > 0 || j < m_) {
          const double As = logei_wave_sum(A[j] * sc), Bs = logei_wave_sum(B[j] * sc);
          if (lane < a.d)
            tq += As * a.dmean[(((long)h * m_ + j) * a.ldg + c) * a.d + lane] + Bs * a.dvar[(((long)h * m_ + j) * a.ldg + c) * a.d + lane];
        }
      mix.dq = mix.dq * s0 + tq * s1;
    }
  }
  const bool any = mix.M > -INFINITY;
  if (lane == 0) a.acq[c] = any ? mix.M + log(mix.S) : -INFINITY;
  if (GRAD && lane < a.d) a.dacq[(long)c * a.d + lane] = any ? mix.dq / mix.S : 0.0;
}

// the same over a utility program (acq_mc_prog_kernel / acq_mc_grad_prog_kernel): blockDim.x / 64 candidates per workgroup
extern __shared__ __attribute__((aligned(16))) double logei_prog_file[];   // (m + slots) x blockDim.x, entry-major

template <bool GRAD>
__global__ __launch_bounds__(256) void logei_mc_prog_kernel(LogEiArgs a, UtilProgDev p) {
  const int lane = threadIdx.x & 63, nt = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.x * (nt >> 6) + wave;
  if (c >= a.C) return;                         // wave-uniform
  double* file = logei_prog_file + threadIdx.x;
  const double lnorm = log(a.tau) - log((double)a.H * (double)a.S);
  const int u_slot = p.m + (GRAD ? p.grad_out[0] : p.val_out);
  LogEiMix mix{-INFINITY, 0.0, 0.0};
  for (int h = 0; h < a.H; ++h) {
    double mu[BOCF_MAX_M], sg[BOCF_MAX_M], A[BOCF_MAX_M], B[BOCF_MAX_M];
#pragma unroll
    for (int j = 0; j < BOCF_MAX_M; ++j) {
      mu[j] = j < p.m ? wave_uniform(a.mean[((long)h * p.m + j) * a.ld + c]) : 0.0;
      sg[j] = j < p.m ? wave_uniform(sqrt(a.var[((long)h * p.m + j) * a.ld + c])) : 1.0;
      A[j] = 0.0;
      B[j] = 0.0;
    }
    double mx = -INFINITY, sum = 0.0;
    for (int l = 0; l < a.L; ++l) {
      const double pl = a.prob[l];
      if (!(pl > 0.0)) continue;                // wave-uniform
      const double* th = a.theta + (long)l * a.theta_dim;
      const double lw = log(pl) + lnorm, best = a.best[(long)h * a.best_stride + l];
      for (int s0 = 0; s0 < a.S; s0 += 64) {     // wave-uniform trip count; lanes past the last sample are masked out of the sums
        const int s = min(s0 + lane, a.S - 1);
        const bool live = s0 + lane < a.S;
        double w[BOCF_MAX_M];
#pragma unroll
        for (int j = 0; j < BOCF_MAX_M; ++j) {
          w[j] = j < p.m ? a.Wt[(long)j * a.S + s] : 0.0;
          if (j < p.m) file[(long)j * nt] = mu[j] + sg[j] * w[j];
        }
        if (GRAD) prog_run(p.grad_code, p.n_grad, file, nt, p.m, th, p.consts);
        else prog_run(p.val_code, p.n_val, file, nt, p.m, th, p.consts);
        const double t = (file[(long)u_slot * nt] - best) / a.tau;
        double lpsi, ratio = 0.0;
        logei_log_psi<GRAD>(t, lpsi, ratio);
        const double e = lw + lpsi;
        if (live && e > -INFINITY && e < INFINITY) {
          double sc, wgt;
          logei_push(e, mx, sum, sc, wgt);
          if (GRAD) {
            const double coef = wgt * (ratio / a.tau);
#pragma unroll
            for (int j = 0; j < BOCF_MAX_M; ++j)
              if (j < p.m) {
                const double g = file[(long)(p.m + p.grad_out[1 + j]) * nt];
                A[j] = A[j] * sc + coef * g;
                B[j] = B[j] * sc + coef * (g * (0.5 * w[j] / sg[j]));
              }
          }
        }
      }
    }
    const double Mh = logei_wave_max(mx);
    if (!(Mh > -INFINITY)) continue;            // wave-uniform
    const double sc = logei_lane_scale(mx, Mh);
    const double Sh = logei_wave_sum(sum * sc);
    const double nM = fmax(mix.M, Mh);
    const double s0 = exp(mix.M - nM), s1 = exp(Mh - nM);
    mix.S = mix.S * s0 + Sh * s1;
    mix.M = nM;
    if (GRAD) {
      double tq = 0.0;
#pragma unroll
      for (int j = 0; j < BOCF_MAX_M; ++j)
        if (j < p.m) {
          const double As = logei_wave_sum(A[j] * sc), Bs = logei_wave_sum(B[j] * sc);
          if (lane < a.d)
            tq += As * a.dmean[(((long)h * p.m + j) * a.ldg + c) * a.d + lane] + Bs * a.dvar[(((long)h * p.m + j) * a.ldg + c) * a.d + lane];
        }
      mix.dq = mix.dq * s0 + tq * s1;
    }
  }
  const bool any = mix.M > -INFINITY;
  if (lane == 0) a.acq[c] = any ? mix.M + log(mix.S) : -INFINITY;
  if (GRAD && lane < a.d) a.dacq[(long)c * a.d + lane] = any ? mix.dq / mix.S : 0.0;
}

// what the kernel needs of the resident program, by value (dev_view of util_prog.hip)
static UtilProgDev logei_prog_view(const UtilProg& p) {
  UtilProgDev v{};
  const unsigned* code = p.dev + BOCF_PROG_HEADER_WORDS;
  v.val_code = reinterpret_cast<const uint2*>(code);
  v.grad_code = reinterpret_cast<const uint2*>(code + 2 * (size_t)p.n_val);
  v.consts = reinterpret_cast<const double*>(code + 2 * (size_t)(p.n_val + p.n_grad));
  v.m = p.m; v.n_slots = p.n_slots; v.n_val = p.n_val; v.n_grad = p.n_grad; v.val_out = p.val_out;
  for (int q = 0; q <= BOCF_MAX_M; ++q) v.grad_out[q] = p.grad_out[q];
  return v;
}

void launch_logei_mc(const LogEiArgs& a, bool grad, hipStream_t s) {
  if (a.C == 0) return;
  if (a.util_kind == BOCF_UTIL_PROGRAM) {
    if (!a.prog || !a.prog->dev) {                         // (the entry point refuses this by name)
      bocf_note_launch("logei_mc_prog_kernel", hipErrorInvalidValue);
      return;
    }
    int nt;
    size_t lds;
    util_prog_geometry(*a.prog, &nt, &lds);
    const int per = nt / 64;
    const dim3 grid((unsigned)((a.C + per - 1) / per));
    if (grad) BOCF_LAUNCH((logei_mc_prog_kernel<true>), grid, dim3((unsigned)nt), lds, s, a, logei_prog_view(*a.prog));
    else BOCF_LAUNCH((logei_mc_prog_kernel<false>), grid, dim3((unsigned)nt), lds, s, a, logei_prog_view(*a.prog));
    return;
  }
  const dim3 grid((unsigned)((a.C + 3) / 4));
  switch (a.m >= 1 && a.m <= 8 ? a.m : 0) {
#define LM(M) case M: if (grad) BOCF_LAUNCH((logei_mc_kernel<M, true>), grid, dim3(256), 0, s, a); else BOCF_LAUNCH((logei_mc_kernel<M, false>), grid, dim3(256), 0, s, a); break;
    LM(1) LM(2) LM(3) LM(4) LM(5) LM(6) LM(7) LM(8) default: LM(0)
#undef LM
  }
}
