// Host driver of the predict planner (bocf_amd/csrc/predict_plan.h) for tests/test_predict_plan_cpu.py.
//   predict_plan_driver    one plan per line of stdin: "key=value ..." (inputs and options by name) -> "key=value ..." of the plan; "tiling" is
//                          that of the first pass, "passes" the number of passes
#include "../bocf_amd/csrc/predict_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static bool set_field(PredictPlanInput& in, const char* k, long v) {
  struct { const char* name; int* field; } ints[] = {{"C", &in.C}, {"N", &in.N}, {"Np", &in.Np}, {"m", &in.m}, {"d", &in.d}, {"pred_cap", &in.pred_cap},
                                                     {"swizzle", &in.swizzle}};
  struct { const char* name; bool* field; } flags[] = {{"need_var", &in.need_var}, {"need_grad", &in.need_grad}, {"small_path", &in.small_path},
                                                       {"predict_f32", &in.predict_f32}, {"predict_i8", &in.predict_i8}};
  if (!strcmp(k, "chunk")) return in.chunk = v, true;
  if (!strcmp(k, "workspace_mb")) return in.workspace_mb = v, true;
  for (auto& f : ints)
    if (!strcmp(k, f.name)) return *f.field = (int)v, true;
  for (auto& f : flags)
    if (!strcmp(k, f.name)) return *f.field = v != 0, true;
  return false;
}

int main() {
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    PredictPlanInput in;
    for (char* tok = strtok(line, " \t\n"); tok; tok = strtok(nullptr, " \t\n")) {
      char* eq = strchr(tok, '=');
      if (!eq) return fprintf(stderr, "bad token %s\n", tok), 2;
      *eq = 0;
      if (!set_field(in, tok, atol(eq + 1))) return fprintf(stderr, "unknown key %s\n", tok), 2;
    }
    const PredictPlan p = plan_predict(in);
    const long first = in.C < p.chunk ? in.C : p.chunk;
    const int first_pad = (int)((first + PLAN_TILE - 1) / PLAN_TILE * PLAN_TILE);
    printf("kind=%d chunk=%ld chunkpad=%d passes=%ld ld=%d nrt=%d mean_with_var=%d tiling=%d mean_plane=%zu mean=%zu var=%zu acq=%zu meanpart=%zu "
           "kstar=%zu sumsq=%zu vs=%zu ws=%zu vbuf=%zu dmean=%zu dvar=%zu dacq=%zu r32=%zu ri8=%zu ri8e=%zu ki8=%zu ki8e=%zu\n",
           (int)p.kind, p.chunk, p.chunkpad, (in.C + p.chunk - 1) / p.chunk, p.ld, p.nrt, p.mean_with_var ? 1 : 0, p.tiling(first_pad), p.mean_plane,
           p.mean_bytes, p.var_bytes, p.acq_bytes, p.meanpart_bytes, p.kstar_bytes, p.sumsq_bytes, p.vs_bytes, p.ws_bytes, p.vbuf_bytes, p.dmean_bytes,
           p.dvar_bytes, p.dacq_bytes, p.r32_bytes, p.ri8_bytes, p.ri8e_bytes, p.ki8_bytes, p.ki8e_bytes);
    fflush(stdout);
  }
  return 0;
}
