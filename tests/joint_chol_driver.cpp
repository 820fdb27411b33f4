// Stand-alone host driver of bocf_amd/csrc/joint_chol.h for tests/test_joint_cpu.py: the floored q x q Cholesky factor and its reverse
// pass exactly as the device kernels compile them, run by the host compiler (under -fsanitize=address,undefined in the suite).
// stdin:  n, then n records of: q, use_tau, A (q x q, row-major), Cbar (q x q, row-major; lower triangle read)
// stdout: per record: tau, the mask of floored pivots, C (q x q, upper triangle zero), G (q x q, upper triangle zero) = d alpha / dA of
//         the lower-triangle entries the factorization read.  The matrices live in heap blocks of exactly q * q doubles, so an access
//         outside them is caught.
#include <cstdio>
#include <vector>

#include "../bocf_amd/csrc/joint_chol.h"

int main() {
  int n = 0;
  if (scanf("%d", &n) != 1 || n < 0) return 2;
  for (int r = 0; r < n; ++r) {
    int q = 0, use_tau = 0;
    if (scanf("%d %d", &q, &use_tau) != 2 || q < 1 || q > JOINT_MAX_Q) return 2;
    std::vector<double> A((size_t)q * q), G((size_t)q * q), C((size_t)q * q, 0.0);
    for (double& v : A)
      if (scanf("%lf", &v) != 1) return 2;
    for (double& v : G)
      if (scanf("%lf", &v) != 1) return 2;
    for (int k = 0; k < q; ++k)
      for (int i = k + 1; i < q; ++i) G[(size_t)k * q + i] = 0.0;
    const double tau = use_tau ? joint_chol_tau(A.data(), q, q) : 0.0;
    const unsigned floored = joint_chol_floor(A.data(), q, q, tau, C.data(), q);
    joint_chol_adjoint(C.data(), q, q, floored, G.data(), q);
    printf("%.17g %u\n", tau, floored);
    for (double v : C) printf("%.17g\n", v);
    for (double v : G) printf("%.17g\n", v);
  }
  return 0;
}
