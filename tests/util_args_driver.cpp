// Host driver of the utility-argument block (bocf_amd/csrc/util_args.h) for tests/test_util_args_cpu.py.  One case per line of standard
// input, one line of output per case; numbers are written with %.17g, so they read back exactly.
//   util_args_driver check   line: who|program refusal|kind n_params params_null theta_null theta_dim L m mode
//                            bocf_util_check_kind, then bocf_util_check: "who: message" as bocf_fail got it, or "ok"
//   util_args_driver pack    line: L theta_dim n_params prob_given n_tail, then the values of theta, prob (if given), params, tail
//                            the offsets theta prob params tail, the size, then the packed doubles
//   util_args_driver rows    line: theta_dim P per n_params, then the values of theta (P, theta_dim) and params
//                            tw, the size, then the packed doubles
// Every array is a heap block of exactly the size the caller would pass (none for size 0), so a sanitizer build sees any read past it.
#include "../bocf_amd/csrc/util_args.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int g_failed = 0;
int bocf_fail(const char* what, const char* detail) {
  if (!g_failed++) printf("%s: %s\n", what, detail);          // (a checker reports once: a second report would show as a second line)
  else printf("AGAIN %s: %s\n", what, detail);
  return -1;
}

static std::vector<double> take(char** cursor, size_t n) {
  std::vector<double> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = strtod(*cursor, cursor);
  return v;
}
static const double* ptr(const std::vector<double>& v) { return v.empty() ? nullptr : v.data(); }
static void print(const std::vector<double>& v) {
  for (double x : v) printf(" %.17g", x);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return fprintf(stderr, "usage: util_args_driver check | pack | rows  (cases on standard input)\n"), 2;
  const std::string what = argv[1];
  char line[1 << 16];
  while (fgets(line, sizeof line, stdin)) {
    if (what == "check") {
      char* bar1 = strchr(line, '|');
      char* bar2 = bar1 ? strchr(bar1 + 1, '|') : nullptr;
      if (!bar2) return fprintf(stderr, "bad line: %s", line), 2;
      *bar1 = *bar2 = 0;
      int kind, n_params, params_null, theta_null, theta_dim, L, m, mode;
      if (sscanf(bar2 + 1, "%d %d %d %d %d %d %d %d", &kind, &n_params, &params_null, &theta_null, &theta_dim, &L, &m, &mode) != 8)
        return fprintf(stderr, "bad numbers: %s", bar2 + 1), 2;
      const double one = 1.0;                                  // (the checks look at the pointers, never through them)
      const UtilArgs u{kind, params_null ? nullptr : &one, n_params, theta_null ? nullptr : &one, theta_dim, nullptr, L};
      g_failed = 0;
      int rc = bocf_util_check_kind(line, u, bar1 + 1);
      if (rc == 0) rc = bocf_util_check(line, u, m, mode);
      if (rc != (g_failed ? -1 : 0)) return fprintf(stderr, "status %d with %d reports\n", rc, g_failed), 1;
      if (rc == 0) printf("ok\n");
    } else if (what == "pack") {
      char* cur = line;
      const int L = (int)strtol(cur, &cur, 10), theta_dim = (int)strtol(cur, &cur, 10), n_params = (int)strtol(cur, &cur, 10);
      const int prob_given = (int)strtol(cur, &cur, 10);
      const size_t n_tail = (size_t)strtol(cur, &cur, 10);
      const std::vector<double> theta = take(&cur, (size_t)L * theta_dim), prob = take(&cur, prob_given ? L : 0), params = take(&cur, n_params),
                                tail = take(&cur, n_tail);
      UtilPack pk;
      pk.host.assign(3, -1.0);                                 // (stale content of an earlier call must not survive)
      bocf_util_pack(UtilArgs{0, ptr(params), n_params, ptr(theta), theta_dim, ptr(prob), L}, ptr(tail), n_tail, &pk);
      printf("%zu %zu %zu %zu %zu", pk.theta, pk.prob, pk.params, pk.tail, pk.host.size());
      if (pk.bytes() != sizeof(double) * pk.host.size()) return fprintf(stderr, "bytes() is off\n"), 1;
      print(pk.host);
    } else if (what == "rows") {
      char* cur = line;
      const int theta_dim = (int)strtol(cur, &cur, 10), P = (int)strtol(cur, &cur, 10), per = (int)strtol(cur, &cur, 10);
      const int n_params = (int)strtol(cur, &cur, 10);
      const std::vector<double> theta = take(&cur, (size_t)P * theta_dim), params = take(&cur, n_params);
      std::vector<double> host(5, -1.0);
      const int tw = bocf_util_pack_rows(ptr(theta), theta_dim, P, per, ptr(params), n_params, &host);
      printf("%d %zu", tw, host.size());
      print(host);
    } else {
      return fprintf(stderr, "unknown command %s\n", argv[1]), 2;
    }
  }
  return 0;
}
