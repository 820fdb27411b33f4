// Stand-alone driver of bocf_amd/csrc/pending_host.h for tests/test_pending_cpu.py (built there with -fsanitize=address,undefined).
// stdin:  M m r S max_tries, then Sigma (M, r, r), mu (M, r), Zp (S, m, r) as text.
// stdout: the return value, then tau (M), L (M, r, r), Q (M, r, r), F (M, r, S), G (M, r, S), one number per line (%.17g).
#include "../bocf_amd/csrc/pending_host.h"

#include <cstdio>
#include <vector>

static bool read_all(std::vector<double>& v) {
  for (double& x : v)
    if (std::scanf("%lf", &x) != 1) return false;
  return true;
}

static void print_all(const std::vector<double>& v) {
  for (double x : v) std::printf("%.17g\n", x);
}

int main() {
  int M, m, r, S, tries;
  if (std::scanf("%d %d %d %d %d", &M, &m, &r, &S, &tries) != 5 || M < 1 || m < 1 || M % m || r < 1 || r > PENDING_MAX_R || S < 1) {
    std::fprintf(stderr, "bad header\n");
    return 2;
  }
  const size_t rr = (size_t)r * r;
  std::vector<double> Sigma(M * rr), mu((size_t)M * r), Zp((size_t)S * m * r);
  if (!read_all(Sigma) || !read_all(mu) || !read_all(Zp)) {
    std::fprintf(stderr, "short input\n");
    return 2;
  }
  std::vector<double> tau(M, 0.0), L(M * rr, 0.0), Q(M * rr, 0.0), F((size_t)M * r * S, 0.0), G((size_t)M * r * S, 0.0);
  const int rc = pending_prepare(Sigma.data(), mu.data(), M, m, r, Zp.data(), S, tries, tau.data(), L.data(), Q.data(), F.data(), G.data());
  std::printf("%d\n", rc);
  print_all(tau);
  print_all(L);
  print_all(Q);
  print_all(F);
  print_all(G);
  return 0;
}
