// Host arithmetic of the pending-point acquisition (capi_pending.hip): from Sigma_j(P, P) of the r <= 15 pending points and the host normals
// Zp it produces, per output j, the jitter tau_j, the lower Cholesky factor L_j of Sigma~_j = Sigma_j + tau_j I, Q_j = Sigma~_j^-1 and the
// joint samples F_sj = mu_j(P) + L_j Zp[s, j, :], G_sj = L_j^-T Zp[s, j, :].  The jitter ladder is that of the joint posterior samples
// (DESIGN section 12): rung 0 = 1e-8 max(mean diag, 1e-10), x 10 per rung, at most max_tries rungs; rung 0 is always added.
// Host-only and pure (no HIP): the CPU suite drives it through tests/pending_host_driver.cpp.
#pragma once

#include <cmath>
#include <cstddef>

#define PENDING_MAX_R 15

// lower Cholesky of the r x r row-major A + tau I into L (r x r row-major, strict upper part zero); false on a pivot that is not a positive
// finite number.  Only the lower triangle of A is read.
static inline bool pending_cholesky(const double* A, int r, double tau, double* L) {
  for (int i = 0; i < r; ++i)
    for (int k = 0; k < r; ++k) L[i * r + k] = 0.0;
  for (int i = 0; i < r; ++i) {
    for (int k = 0; k <= i; ++k) {
      double s = A[i * r + k] + (i == k ? tau : 0.0);
      for (int t = 0; t < k; ++t) s -= L[i * r + t] * L[k * r + t];
      if (i == k) {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        L[i * r + i] = std::sqrt(s);
      } else {
        L[i * r + k] = s / L[k * r + k];
      }
    }
  }
  return true;
}

// the ladder for one output: tau and L on success (true); on failure tau holds the last rung tried
static inline bool pending_factor(const double* Sigma, int r, int max_tries, double* tau, double* L) {
  double mean = 0.0;
  for (int i = 0; i < r; ++i) mean += Sigma[i * r + i];
  mean /= r;
  double t = 1e-8 * (mean > 1e-10 ? mean : 1e-10);
  const int rungs = max_tries > 1 ? max_tries : 1;
  for (int attempt = 0;; t *= 10.0) {
    *tau = t;
    if (pending_cholesky(Sigma, r, t, L)) return true;
    if (++attempt >= rungs) return false;
  }
}

// Q = (L L^T)^-1 = L^-T L^-1 (r x r row-major, symmetric): column by column, forward then backward substitution
static inline void pending_inverse(const double* L, int r, double* Q) {
  double y[PENDING_MAX_R];
  for (int c = 0; c < r; ++c) {
    for (int i = 0; i < r; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int t = 0; t < i; ++t) s -= L[i * r + t] * y[t];
      y[i] = s / L[i * r + i];
    }
    for (int i = r - 1; i >= 0; --i) {
      double s = y[i];
      for (int t = i + 1; t < r; ++t) s -= L[t * r + i] * Q[t * r + c];
      Q[i * r + c] = s / L[i * r + i];
    }
  }
  for (int i = 0; i < r; ++i)                      // the two halves as one number
    for (int k = 0; k < i; ++k) Q[i * r + k] = Q[k * r + i] = 0.5 * (Q[i * r + k] + Q[k * r + i]);
}

// All M = H m outputs (hyper-sample-major; output h m + j reads the normals of model output j).
//   Sigma (M, r, r), mu (M, r), Zp (S, m, r)  ->  tau (M), Lout (M, r, r) or null, Q (M, r, r), F and G (M, r, S): [j][i][s], s fastest.
// Returns 0, or j + 1 for the first output that stays indefinite on the last rung (tau is filled for every output all the same).
static inline int pending_prepare(const double* Sigma, const double* mu, int M, int m, int r, const double* Zp, int S, int max_tries, double* tau,
                                  double* Lout, double* Q, double* F, double* G) {
  int bad = 0;
  double L[PENDING_MAX_R * PENDING_MAX_R], g[PENDING_MAX_R];
  for (int j = 0; j < M; ++j) {
    const size_t rr = (size_t)r * r;
    if (!pending_factor(Sigma + j * rr, r, max_tries, tau + j, L)) {
      if (!bad) bad = j + 1;
      continue;
    }
    if (Lout)
      for (size_t e = 0; e < rr; ++e) Lout[j * rr + e] = L[e];
    pending_inverse(L, r, Q + j * rr);
    double* Fj = F + (size_t)j * r * S;
    double* Gj = G + (size_t)j * r * S;
    for (int s = 0; s < S; ++s) {
      const double* z = Zp + ((size_t)s * m + j % m) * r;
      for (int i = 0; i < r; ++i) {
        double f = mu[(size_t)j * r + i];
        for (int t = 0; t <= i; ++t) f += L[i * r + t] * z[t];
        Fj[(size_t)i * S + s] = f;
      }
      for (int i = r - 1; i >= 0; --i) {             // L^T g = z
        double v = z[i];
        for (int t = i + 1; t < r; ++t) v -= L[t * r + i] * g[t];
        g[i] = v / L[i * r + i];
      }
      for (int i = 0; i < r; ++i) Gj[(size_t)i * S + s] = g[i];
    }
  }
  return bad;
}
