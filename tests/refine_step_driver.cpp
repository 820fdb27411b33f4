// Stand-alone driver of bocf_amd/csrc/refine_step.h for tests/test_refine_step_cpu.py: runs the per-row state machine on an analytic
// objective, one evaluation per running row and pass, exactly as refine_advance_kernel is driven on the device.
//
// stdin:  objective d m A maxiter max_ls maxfun factr pgtol c1 extra
//         lo (d) hi (d) X0 (A d) then the objective's numbers:  qsin: Q (d d) c (d);  sq, sqinf, sqnan: c0;  poly: none
// stdout: per row "x_0 .. x_{d-1} | f | iterations evaluations reason" (doubles as %a: bit-exact), then "passes P", then "frozen 0/1":
//         `extra` further calls on the stopped rows (with a value and gradient that would move a running row) left every state byte alone.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../bocf_amd/csrc/refine_poly.h"

static double next_double() {
  char tok[128];
  if (scanf("%127s", tok) != 1) {
    fprintf(stderr, "refine_step_driver: input ended early\n");
    exit(2);
  }
  return strtod(tok, nullptr);
}

struct Objective {
  std::string name;
  int d;
  std::vector<double> Q, c;
  double eval(const double* x, double* g) const {
    if (name == "poly") return refine_poly(x, d, g);
    if (name == "qsin") {                                  // 0.5 z'Qz - c'z + 0.05 sum sin(3 z), z = x - 0.3
      std::vector<double> z(d);
      for (int k = 0; k < d; ++k) z[k] = x[k] - 0.3;
      double f = 0.0;
      for (int k = 0; k < d; ++k) {
        double qz = 0.0;
        for (int e = 0; e < d; ++e) qz += Q[(size_t)k * d + e] * z[e];
        f += 0.5 * z[k] * qz - c[k] * z[k] + 0.05 * std::sin(3.0 * z[k]);
        g[k] = qz - c[k] + 0.15 * std::cos(3.0 * z[k]);
      }
      return f;
    }
    double f = 0.0;                                        // sq: sum (x - c0)^2; sqinf: inf beyond the plane x_0 = 0.5; sqnan: NaN gradient below x_0 = 0.3
    for (int k = 0; k < d; ++k) {
      f += (x[k] - c[0]) * (x[k] - c[0]);
      g[k] = 2.0 * (x[k] - c[0]);
    }
    if (name == "sqinf" && x[0] > 0.5) f = INFINITY;
    if (name == "sqnan" && x[0] < 0.3) g[0] = NAN;
    return f;
  }
};

int main() {
  char name[32];
  if (scanf("%31s", name) != 1) return 2;
  Objective ob;
  ob.name = name;
  RefineSettings s;
  s.d = (int)next_double(); s.m = (int)next_double();
  const int A = (int)next_double();
  s.maxiter = (int)next_double(); s.max_ls = (int)next_double(); s.maxfun = (int)next_double();
  s.factr = next_double(); s.pgtol = next_double(); s.c1 = next_double();
  const int extra = (int)next_double();
  const int d = s.d, m = s.m;
  if (d < 1 || m < 1 || A < 1 || s.max_ls < 1 || s.maxiter < 0) return 2;
  ob.d = d;
  std::vector<double> lo(d), hi(d), X0((size_t)A * d);
  for (double& v : lo) v = next_double();
  for (double& v : hi) v = next_double();
  for (double& v : X0) v = next_double();
  if (ob.name == "qsin") {
    ob.Q.resize((size_t)d * d);
    ob.c.resize(d);
    for (double& v : ob.Q) v = next_double();
    for (double& v : ob.c) v = next_double();
  } else if (ob.name != "poly") {
    ob.c.assign(1, next_double());
  }
  s.boxed = refine_boxed(lo.data(), hi.data(), d);

  const size_t nd = refine_row_doubles(d, m);
  std::vector<double> dbl((size_t)A * nd), g(d);
  std::vector<int> ints((size_t)A * REFINE_ROW_INTS);
  std::vector<RefineRow> rows;
  for (int a = 0; a < A; ++a) {
    rows.push_back(refine_row_view(dbl.data() + (size_t)a * nd, ints.data() + (size_t)a * REFINE_ROW_INTS, d, m));
    refine_init(rows[a], X0.data() + (size_t)a * d, lo.data(), hi.data(), s);
  }
  const long long budget = refine_pass_budget(s);
  long long passes = 0;
  for (; passes < budget; ++passes) {
    int running = 0;
    for (int a = 0; a < A; ++a) {
      if (*rows[a].reason != REFINE_RUNNING) continue;
      ++running;
      const double f = ob.eval(refine_point(rows[a]), g.data());
      refine_advance(rows[a], f, g.data(), lo.data(), hi.data(), s);
    }
    if (!running) break;
  }
  int still = 0;
  for (int a = 0; a < A; ++a) still += *rows[a].reason == REFINE_RUNNING;
  if (still) {
    fprintf(stderr, "refine_step_driver: %d rows still running after the pass budget\n", still);
    return 3;
  }
  const std::vector<double> dbl0 = dbl;
  const std::vector<int> ints0 = ints;
  for (int e = 0; e < extra; ++e)
    for (int a = 0; a < A; ++a) {
      for (int k = 0; k < d; ++k) g[k] = 1.0 + k;
      refine_advance(rows[a], -1e30, g.data(), lo.data(), hi.data(), s);
    }
  const int frozen = !memcmp(dbl0.data(), dbl.data(), sizeof(double) * dbl.size()) && !memcmp(ints0.data(), ints.data(), sizeof(int) * ints.size());
  for (int a = 0; a < A; ++a) {
    for (int k = 0; k < d; ++k) printf("%a ", rows[a].x[k]);
    printf("| %a | %d %d %d\n", *rows[a].f, *rows[a].iters, *rows[a].nfun, *rows[a].reason);
  }
  printf("passes %lld\nfrozen %d\n", passes, frozen);
  return 0;
}
