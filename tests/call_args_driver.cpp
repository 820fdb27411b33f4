// Host driver of the argument checks of the entry points that evaluate a utility over the posterior (bocf_amd/csrc/call_args.h: what
// bocf_acq_linear[_grad], bocf_acq_mc[_grad], bocf_set_mc_samples, bocf_set_eu_samples, bocf_expected_utility, bocf_acq_kg,
// bocf_acq_pending, bocf_acq_joint, bocf_feasible_best, bocf_acq_mc_constrained and bocf_loo_utility run before they touch the context)
// for tests/test_call_args_cpu.py.  One case per line of standard input, one line of output per case; `who` names the entry point and
// selects its sequence:
//   who|fitted canned N d m H best_group C S_mc eu_S eu_L eu_m cq_K cq_m kg_na pd_r pd_S|kind n_params params_null theta_null theta_dim L|
//       acq_kind mode grad group flags n_hyps rows val_null z_null S q
//     rows:   0 = null, 1 = C valid indices (i mod L), 2 = the last one L, 3 = the last one -1
//     z_null: the samples of the call (W, Z, Zf) are null; S: their count (S, Sf); q: points per joint batch
//   -> "who: message" as bocf_fail got it; "ok m" (m = outputs per hyper-sample; "ok m program" when the resident program is still to be
//      checked, which the driver takes as passed, as the entry point goes on behind it); "nothing m" when there is no resident candidate.
// rows is a heap block of exactly C entries (none for C = 0), so a sanitizer build sees any read past it.
#include "../bocf_amd/csrc/call_args.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    int kind, n_params, params_null, theta_null, theta_dim, L, acq_kind, mode, grad, group, flags, n_hyps, rows_mode, val_null, z_null, S, q;
    if (sscanf(bar1 + 1, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &s.fitted, &s.canned, &s.N, &s.d, &s.m, &s.hyper_samples, &s.best_group, &s.C,
               &s.S_mc, &s.eu_S, &s.eu_L, &s.eu_m, &s.cq_K, &s.cq_m, &s.kg_na, &s.pd_r, &s.pd_S) != 17)
      return fprintf(stderr, "bad state: %s", bar1 + 1), 2;
    if (sscanf(bar2 + 1, "%d %d %d %d %d %d", &kind, &n_params, &params_null, &theta_null, &theta_dim, &L) != 6)
      return fprintf(stderr, "bad utility block: %s", bar2 + 1), 2;
    if (sscanf(bar3 + 1, "%d %d %d %d %d %d %d %d %d %d %d", &acq_kind, &mode, &grad, &group, &flags, &n_hyps, &rows_mode, &val_null, &z_null, &S, &q) != 11)
      return fprintf(stderr, "bad call: %s", bar3 + 1), 2;
    const double one = 1.0;                                    // (the checks look at the pointers, never through them)
    const UtilArgs u{kind, params_null ? nullptr : &one, n_params, theta_null ? nullptr : &one, theta_dim, nullptr, L};
    const double* Z = z_null ? nullptr : &one;
    std::vector<int> rows(s.C > 0 ? (size_t)s.C : 0);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = L > 0 ? (int)(i % (size_t)L) : 0;
    if (rows_mode == 2 && !rows.empty()) rows.back() = L;
    if (rows_mode == 3 && !rows.empty()) rows.back() = -1;
    const int* rp = rows_mode && !rows.empty() ? rows.data() : nullptr;
    const double* val = val_null ? nullptr : &one;
    const char* who = line;
    g_failed = 0;
    bool program = false;
    int m, rc = 0;                                             // rc: of the part behind the resident program's check
    if (!strcmp(who, "bocf_acq_linear") || !strcmp(who, "bocf_acq_linear_grad")) {
      m = bocf_acq_linear_check(who, s, acq_kind);
    } else if (!strcmp(who, "bocf_acq_mc")) {
      m = bocf_acq_mc_check(who, s, false, acq_kind, u, &program);
    } else if (!strcmp(who, "bocf_acq_mc_grad")) {
      m = bocf_acq_mc_check(who, s, true, acq_kind, u, &program);
      if (m >= 0) rc = bocf_check_grad_dim(who, s, true, true);
    } else if (!strcmp(who, "bocf_set_mc_samples")) {
      m = bocf_set_samples_check(who, s, Z && S >= 1);
    } else if (!strcmp(who, "bocf_set_eu_samples")) {
      m = bocf_set_samples_check(who, s, Z && L >= 1 && S >= 1);
    } else if (!strcmp(who, "bocf_expected_utility")) {
      m = bocf_eu_check_utility(who, s, mode, u, &program);
      if (m >= 0) rc = bocf_eu_check_call(who, s, mode, u, m, rp, n_hyps, val, grad != 0);
    } else if (!strcmp(who, "bocf_acq_kg")) {
      m = bocf_kg_check(who, s, mode, u, Z, S);
    } else if (!strcmp(who, "bocf_acq_pending")) {
      m = bocf_pending_check(who, s, u);
    } else if (!strcmp(who, "bocf_acq_joint")) {
      m = bocf_joint_check(who, s, u, q, Z, S);
    } else if (!strcmp(who, "bocf_feasible_best")) {
      m = bocf_constrained_utility(who, s, u, true, BOCF_CACQ_NO_PROGRAM);
    } else if (!strcmp(who, "bocf_acq_mc_constrained")) {
      m = bocf_cacq_check(who, s, u, grad != 0);
    } else if (!strcmp(who, "bocf_loo_utility")) {
      m = bocf_loo_utility_check(who, s, group, flags, mode, u, &program);
      if (m >= 0) rc = bocf_loo_utility_check_call(who, s, mode, L, m, val);
    } else {
      return fprintf(stderr, "unknown entry point: %s\n", who), 2;
    }
    const bool refused = m < 0 || rc < 0;
    if (refused != (g_failed == 1) || g_failed > 1) return fprintf(stderr, "status %d / %d with %d reports\n", m, rc, g_failed), 1;
    if (!refused) printf(rc == 1 ? "nothing %d%s\n" : "ok %d%s\n", m, program ? " program" : "");
  }
  return 0;
}
