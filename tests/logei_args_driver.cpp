// Host driver of the argument checks of the log-space expected-improvement entry points (bocf_amd/csrc/logei_args.h: what
// bocf_acq_log_linear and bocf_acq_log_mc run before they touch the context) for tests/test_logei_cpu.py.  One case per line of standard
// input, one line of output per case:
//   who|fitted canned m H best_group S_mc d C|kind n_params params_null theta_null theta_dim L grad|tau
//     tau: "none" = the line is a bocf_acq_log_linear call (theta, L and grad of the block); a number, "inf" or "nan" = a bocf_acq_log_mc call
//   -> "who: message" as bocf_fail got it, or "ok m" (m = outputs per hyper-sample; "ok m program" when the resident program is still to be checked).
#include "../bocf_amd/csrc/logei_args.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

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
    int kind, n_params, params_null, theta_null, theta_dim, L, grad;
    char tau_text[64];
    if (sscanf(bar1 + 1, "%d %d %d %d %d %d %d %d", &s.fitted, &s.canned, &s.m, &s.hyper_samples, &s.best_group, &s.S_mc, &s.d, &s.C) != 8)
      return fprintf(stderr, "bad state: %s", bar1 + 1), 2;
    if (sscanf(bar2 + 1, "%d %d %d %d %d %d %d", &kind, &n_params, &params_null, &theta_null, &theta_dim, &L, &grad) != 7)
      return fprintf(stderr, "bad call: %s", bar2 + 1), 2;
    if (sscanf(bar3 + 1, "%63s", tau_text) != 1) return fprintf(stderr, "bad tau: %s", bar3 + 1), 2;
    const double one = 1.0;                                    // (the checks look at the pointers, never through them)
    g_failed = 0;
    bool program = false;
    int m;
    if (!strcmp(tau_text, "none")) {
      m = bocf_log_linear_check(line, s, theta_null ? nullptr : &one, L, grad != 0);
    } else {
      const UtilArgs u{kind, params_null ? nullptr : &one, n_params, theta_null ? nullptr : &one, theta_dim, nullptr, L};
      m = bocf_log_mc_check(line, s, strtod(tau_text, nullptr), u, grad != 0, &program);
    }
    if ((m < 0) != (g_failed == 1) || g_failed > 1) return fprintf(stderr, "status %d with %d reports\n", m, g_failed), 1;
    if (m >= 0) printf(program ? "ok %d program\n" : "ok %d\n", m);
  }
  return 0;
}
