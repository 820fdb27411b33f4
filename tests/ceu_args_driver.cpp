// Host driver of the argument checks of the constrained expected-utility entry points (bocf_amd/csrc/ceu_args.h: the callers of
// util_args.h that bocf_train_utility_range and bocf_expected_utility_constrained are) for tests/test_ceu_cpu.py.  One case per line of
// standard input, one line of output per case:
//   who|fitted canned m H best_group cq_K cq_m eu_S eu_L eu_m d C need_constraints|kind n_params params_null theta_null theta_dim L|u0 rows n_hyps val_null grad
//     u0:   0 = null, 1 = L finite values, 2 = the last one NaN, 3 = the last one infinite
//     rows: 0 = null, 1 = C valid indices (i mod L), 2 = the last one L, 3 = the last one -1
//   -> "who: message" as bocf_fail got it; "ok m" (m = outputs per hyper-sample) when both parts accept; "nothing m" when there is no
//      resident candidate.  With need_constraints = 0 only the utility part runs (bocf_train_utility_range).
// u0 and rows are heap blocks of exactly L and C entries (none for size 0), so a sanitizer build sees any read past them.
#include "../bocf_amd/csrc/ceu_args.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

static int g_failed = 0;
int bocf_fail(const char* what, const char* detail) {
  if (!g_failed++) printf("%s: %s\n", what, detail);          // (a checker reports once: a second report would show as a second line)
  else printf("AGAIN %s: %s\n", what, detail);
  return -1;
}

int main() {
  char line[1 << 12];
  while (fgets(line, sizeof line, stdin)) {
    char* bar1 = strchr(line, '|');
    char* bar2 = bar1 ? strchr(bar1 + 1, '|') : nullptr;
    char* bar3 = bar2 ? strchr(bar2 + 1, '|') : nullptr;
    if (!bar3) return fprintf(stderr, "bad line: %s", line), 2;
    *bar1 = *bar2 = *bar3 = 0;
    CallState s{};
    int need_constraints, kind, n_params, params_null, theta_null, theta_dim, L, u0_mode, rows_mode, n_hyps, val_null, grad;
    if (sscanf(bar1 + 1, "%d %d %d %d %d %d %d %d %d %d %d %d %d", &s.fitted, &s.canned, &s.m, &s.hyper_samples, &s.best_group, &s.cq_K, &s.cq_m, &s.eu_S,
               &s.eu_L, &s.eu_m, &s.d, &s.C, &need_constraints) != 13)
      return fprintf(stderr, "bad state: %s", bar1 + 1), 2;
    if (sscanf(bar2 + 1, "%d %d %d %d %d %d", &kind, &n_params, &params_null, &theta_null, &theta_dim, &L) != 6)
      return fprintf(stderr, "bad utility block: %s", bar2 + 1), 2;
    if (sscanf(bar3 + 1, "%d %d %d %d %d", &u0_mode, &rows_mode, &n_hyps, &val_null, &grad) != 5) return fprintf(stderr, "bad call: %s", bar3 + 1), 2;
    const double one = 1.0;                                    // (the utility checks look at the pointers, never through them)
    const UtilArgs u{kind, params_null ? nullptr : &one, n_params, theta_null ? nullptr : &one, theta_dim, nullptr, L};
    std::vector<double> u0(L > 0 ? (size_t)L : 0, -0.5);
    if (u0_mode == 2 && !u0.empty()) u0.back() = std::nan("");
    if (u0_mode == 3 && !u0.empty()) u0.back() = std::numeric_limits<double>::infinity();
    std::vector<int> rows(s.C > 0 ? (size_t)s.C : 0);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = L > 0 ? (int)(i % (size_t)L) : 0;
    if (rows_mode == 2 && !rows.empty()) rows.back() = L;
    if (rows_mode == 3 && !rows.empty()) rows.back() = -1;
    double val = 0.0;
    g_failed = 0;
    const int m = bocf_constrained_utility(line, s, u, need_constraints != 0, BOCF_CEU_NO_PROGRAM);
    int rc = m < 0 ? -1 : 0;
    if (rc == 0 && need_constraints)
      rc = bocf_ceu_check_call(line, s, u, m, u0_mode && !u0.empty() ? u0.data() : nullptr, rows_mode && !rows.empty() ? rows.data() : nullptr, n_hyps,
                               val_null ? nullptr : &val, grad != 0);
    if ((rc < 0) != (g_failed == 1) || g_failed > 1) return fprintf(stderr, "status %d with %d reports\n", rc, g_failed), 1;
    if (rc == 0) printf("ok %d\n", m);
    if (rc == 1) printf("nothing %d\n", m);
  }
  return 0;
}
