// Host driver of the factorization planner (bocf_amd/csrc/chol_plan.h) for tests/test_chol_plan_cpu.py.
//   chol_plan_driver            one plan per line of stdin: "key=value ..." (inputs and options by name) -> "key=value ..." of the plan
//   chol_plan_driver --sweep    the plan's invariants over nb 1..64, m 1..130, a range of CU counts and every option value; prints the
//                               number of plans checked and of violations, and the first few violations
#include "../bocf_amd/csrc/chol_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool set_field(CholPlanInput& in, CholOptions& o, const char* k, int v) {
  struct { const char* name; int* field; } ints[] = {
      {"nb", &in.nb}, {"m", &in.m}, {"sched_m", &in.sched_m}, {"ncu", &in.ncu},
      {"aggregate", &o.aggregate}, {"lookahead", &o.lookahead}, {"lookahead_min_nb", &o.lookahead_min_nb}, {"overlap_inverse", &o.overlap_inverse},
      {"team_fit", &o.team_fit}, {"team_panels", &o.team_panels}, {"team_hybrid", &o.team_hybrid}, {"team_tail_share", &o.team_tail_share},
      {"team_whole_max", &o.team_whole_max}, {"team_crit_load", &o.team_crit_load}, {"team_stream", &o.team_stream}, {"trsm_wave", &o.trsm_wave},
      {"merge_x3", &o.merge_x3}, {"potrf_scalar", &o.potrf_scalar}, {"force_cu_count", &o.force_cu_count}};
  struct { const char* name; bool* field; } flags[] = {
      {"inv_stream", &in.inv_stream}, {"cu_masks_ok", &in.cu_masks_ok}, {"gated_off", &in.gated_off}, {"sched_retry", &in.sched_retry},
      {"refit", &in.refit}, {"want_kinv", &in.want_kinv}};
  for (auto& f : ints)
    if (!strcmp(k, f.name)) return *f.field = v, true;
  for (auto& f : flags)
    if (!strcmp(k, f.name)) return *f.field = v != 0, true;
  return false;
}

// what every plan must satisfy; returns the first broken rule, or nullptr
static const char* violation(const CholPlanInput& in, const CholPlan& p) {
  const int nb = in.nb;
  const bool team = p.schedule == CHOL_TEAM_WHOLE || p.schedule == CHOL_TEAM_GROUPS || p.schedule == CHOL_HYBRID;
  if (team) {
    if (p.mb < 1 || p.mb > in.m) return "outputs per team launch";
    if ((p.schedule != CHOL_HYBRID || p.panels > 0) && (p.T < 2 || p.mb * p.T > p.ncu)) return "team launch: T >= 2, every workgroup resident";
    if (p.schedule == CHOL_TEAM_WHOLE && nb > TEAM_MAX_NB) return "one team launch beyond TEAM_MAX_NB panels";
    if (p.schedule == CHOL_TEAM_GROUPS && (p.panels < 1 || p.panels >= nb)) return "team groups";
  }
  if (p.schedule == CHOL_HYBRID) {
    if (p.T_tail < 2 || p.mb * p.T_tail > p.ncu) return "hybrid tail: T >= 2, every workgroup resident";
    if (nb - p.h < 2 || nb - p.h > 24 || nb - p.h > TEAM_MAX_NB) return "hybrid tail size";
    if (!in.inv_stream || p.inv_after != p.h - 1) return "hybrid: the early inverse behind the first part";
    if (p.panels == 0 && p.G < 1) return "hybrid first part";
  }
  if (p.schedule == CHOL_RESERVED && (p.reserved_cus < 8 || p.reserved_cus >= p.ncu / 2 || !in.cu_masks_ok || !in.refit)) return "reserved CUs";
  if (p.schedule == CHOL_LAUNCHED && (p.G < 1 || p.G > nb)) return "launched G";
  if (p.inv_after < -1 || p.inv_after >= nb || (p.inv_after >= 0 && !in.inv_stream)) return "early inverse";
  if (p.schedule == CHOL_LAUNCHED ? p.flag_ints != 0 : (p.err_off < 0 || p.err_off + 1 > p.flag_ints)) return "time-out word inside the counter block";
  if (team && (p.err_off != in.m * chol_team_flag_words(nb) || p.err_off + 4 > p.flag_ints)) return "team counter layout";
  if ((in.gated_off || in.sched_retry) && p.schedule != CHOL_LAUNCHED) return "gated schedule after a time-out";
  return nullptr;
}

static int sweep() {
  std::vector<CholOptions> sets;
  const CholOptions d;
  sets.push_back(d);
  auto each = [&](int CholOptions::*f, std::vector<int> vals) {
    for (int v : vals) {
      CholOptions o = d;
      o.*f = v;
      sets.push_back(o);
    }
  };
  each(&CholOptions::aggregate, {1, 2, 3, 4, 5, 6, 7, 8});
  each(&CholOptions::lookahead, {0, 2});
  each(&CholOptions::lookahead_min_nb, {2, 16});
  each(&CholOptions::overlap_inverse, {0, 1});
  each(&CholOptions::team_fit, {0, 1});
  each(&CholOptions::team_panels, {1, 2, 3, 4, 8, 16, 32});
  each(&CholOptions::team_hybrid, {0, 1});
  each(&CholOptions::team_tail_share, {1, 2, 3, 4, 6, 7, 8});
  each(&CholOptions::team_whole_max, {2, 8, 12, 16, 32});
  each(&CholOptions::force_cu_count, {4, 6});
  for (int th : {0, 1, 2}) {                               // team_fit = 1 with every hybrid mode and a small whole-launch limit
    CholOptions o = d;
    o.team_fit = 1; o.team_hybrid = th; o.team_whole_max = 8;
    sets.push_back(o);
  }
  const int cus[] = {4, 5, 6, 7, 8, 16, 80, 256};
  long plans = 0, bad = 0;
  for (const CholOptions& o : sets)
    for (int nb = 1; nb <= 64; ++nb)
      for (int m = 1; m <= 130; ++m)
        for (int ncu : cus)
          for (int bits = 0; bits < 32; ++bits) {
            CholPlanInput in;
            in.nb = nb; in.m = m; in.ncu = ncu;
            in.inv_stream = bits & 1; in.cu_masks_ok = bits & 2; in.refit = bits & 4; in.want_kinv = bits & 8; in.sched_retry = bits & 16;
            const CholPlan p = plan_cholesky(in, o);
            ++plans;
            if (const char* why = violation(in, p))
              if (++bad <= 5) printf("violation: %s (nb %d m %d ncu %d bits %d -> schedule %d)\n", why, nb, m, ncu, bits, (int)p.schedule);
          }
  printf("plans %ld violations %ld\n", plans, bad);
  return bad != 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--sweep")) return sweep();
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    CholPlanInput in;
    CholOptions o;
    for (char* tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) {
      char* eq = strchr(tok, '=');
      if (!eq) return fprintf(stderr, "bad token %s\n", tok), 2;
      *eq = 0;
      if (!set_field(in, o, tok, atoi(eq + 1))) return fprintf(stderr, "unknown key %s\n", tok), 2;
    }
    const CholPlan p = plan_cholesky(in, o);
    printf("schedule=%d G=%d h=%d panels=%d mb=%d T=%d T_tail=%d kinv=%d reserved_cus=%d inv_after=%d flag_ints=%d err_off=%d\n", (int)p.schedule, p.G,
           p.h, p.panels, p.mb, p.T, p.T_tail, p.kinv ? 1 : 0, p.reserved_cus, p.inv_after, p.flag_ints, p.err_off);
    fflush(stdout);
  }
  return 0;
}
