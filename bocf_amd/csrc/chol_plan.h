// The factorization schedule of one Cholesky (capi_chol.hip), decided before anything is enqueued: plan_cholesky reads the context's
// options and history and returns everything the executors need -- which schedule, its panel groups, the team sizes, the reserved
// compute units, where the early inverse starts, the layout of the counter block.  Host-only and pure (no HIP): the CPU suite drives it
// (tests/test_chol_plan_cpu.py).
#pragma once

#define TEAM_MAX_NB 32             // panels one team launch can factor (chol_team.hip: TEAM_MAXU units per workgroup at a team of two)

// every factorization-schedule option of the context (bocf_set_option; descriptions in include/bocf_hip.h)
struct CholOptions {
  int aggregate = 0;         // panels per trailing update of the blocked Cholesky (0 = by size, 1 = classic right-looking)
  int lookahead = -1;        // -1: by size; 0: single stream; 2: reserved-CU schedule
  int lookahead_min_nb = 8;  // reserved-CU lookahead from this many 128-panels on
  // inverse overlapped with the factorization: the part that needs only the first h block rows runs on s_inv
  int overlap_inverse = -1;  // -1 = by size (from N = 4096 with at least two outputs: -4 % at 4096, -6 % at 6144, -2.5 % at 8192; neutral below), 0 / 1 = off / on
  int team_fit = -1;         // one-launch factorization + inverse by resident workgroup teams (chol_team.hip): -1 = by size (2..24 panels), 0 / 1 = never / whenever it applies
  int team_panels = 6;       // panels per team launch where teams work in groups (the first block rows of the hybrid schedule; team_fit = 1 without hybrid), each followed by ONE trailing update with K = 128 x that
  int team_hybrid = 2;       // more than team_whole_max panels: the first block rows by team launches of team_panels panels + trailing updates (1: by the launched schedule), ONE team launch (Cholesky + inverse) for the rest; 0: team_fit = 1 means panel groups throughout
  int team_tail_share = 5;   // hybrid schedule: eighths of the compute units the tail's teams take (the rest is for the early inverse underneath)
  int team_whole_max = 24;   // panels up to which ONE team launch factors and inverts everything (beyond: the hybrid schedule)
  int team_crit_load = 4;    // teams: the workgroups that stream the critical units carry nothing else while the others get by with <= this many units each
  int team_stream = 1;       // teams: U[p][p+1] and the last row of A[p+1][p+1] are formed 16 rows at a time underneath potrf(p) by a workgroup of their own
  int trsm_wave = 1;         // row solves of the factorization through the wave-level single-tile kernel (0: the 128 x 128 GEMM kernel)
  int merge_x3 = 1;          // the second product of an inverse merge in the three-buffer triangular kernel: 0 never, 1 from 4096 rows, 2 whenever possible
  int potrf_scalar = 0;      // probes build: 11..14 = timing-only variants of the diagonal-block kernel
  int force_cu_count = 0;    // test hook (probes build): pretend the device has this many compute units (selection and reserved mask only)
};

// what the decision reads from the context
struct CholPlanInput {
  int nb = 0, m = 0;         // panels, factorizations
  int sched_m = 0;           // > 0: choose as for this many outputs (the helper context of an output-sharded fit)
  int ncu = 0;               // compute units of the device
  bool inv_stream = false;   // the early inverse has its stream
  bool cu_masks_ok = false, gated_off = false, sched_retry = false;
  bool refit = false;        // not the first factorization of the context (fits_done > 0)
  bool want_kinv = false;    // an inference: a schedule that can leaves Ky^-1 behind
};

// (the numbering is bocf_get_stat "last_schedule")
enum CholSchedule { CHOL_LAUNCHED = 0, CHOL_RESERVED = 2, CHOL_TEAM_WHOLE = 3, CHOL_TEAM_GROUPS = 4, CHOL_HYBRID = 5 };

struct CholPlan {
  CholSchedule schedule = CHOL_LAUNCHED;
  int ncu = 0;               // compute units the plan was made for (force_cu_count applied)
  int G = 1;                 // launched schedule: panels per trailing update (hybrid: of its launched first part)
  int h = 1;                 // split of the inverse (largest power of two below nb); hybrid: block rows of the first part
  int panels = 0;            // team launches of this many panels, each followed by a trailing update (schedule 4; hybrid: its first part, 0 = launched)
  int mb = 0, T = 0;         // outputs per team launch, workgroups per team (schedules 3, 4 and the hybrid's first part)
  int T_tail = 0;            // hybrid: workgroups per team of the launch for the last nb - h block rows
  bool kinv = false;         // schedule 3 also accumulates Ky^-1
  int reserved_cus = 0;      // schedule 2: compute units reserved for the chain
  int inv_after = -1;        // the early inverse starts behind the row solve of this panel (-1: none)
  int flag_ints = 0;         // device-side counters + time-out word (0: the schedule waits on none)
  int err_off = 0;           // index of the time-out word in that block
};

// split of the inverse: h = the largest power of two below nb; blocks [0, h) form complete pairs at every level below h
inline int trtri_split(int nb) {
  int h = 1;
  while (2 * h < nb) h *= 2;
  return h;
}

// counters of one output of a team launch (the layout is chol_team_kernel's)
inline int chol_team_flag_words(int nb) { return ((4 * nb + 4 * nb * nb + 3) / 4) * 4; }

// workgroups per team: every workgroup of a launch must be resident at once -- one 12-wave workgroup per compute unit at most -- of which
// `share` eighths (0: all), and no more than the diagonal workgroup, the streaming workgroup and one per unit
inline int chol_team_size(int ncu, int mb, int units, int share) {
  int T = ncu / mb;
  if (share > 0) T = T * share / 8;
  return T > 2 + units ? 2 + units : T;
}

inline CholPlan plan_cholesky(const CholPlanInput& in, const CholOptions& o) {
  const int nb = in.nb, m = in.m;
  const int m_sched = in.sched_m > 0 ? in.sched_m : m;     // (a shard helper chooses as the replicated fit of ALL outputs would)
  const int ncu = o.force_cu_count > 0 ? o.force_cu_count : in.ncu;
  CholPlan p;
  p.ncu = ncu;
  p.h = trtri_split(nb);
  p.mb = m < ncu / 2 ? m : ncu / 2;
  const int team_words = chol_team_flag_words(nb);
  auto team_flags = [&]() { p.flag_ints = m * team_words + 4; p.err_off = m * team_words; };
  // the early inverse behind the launched and team-group schedules: by size from 24 panels -- N = 3072: 3.64 -> 3.57 ms, N = 3584: 4.84 -> 4.52;
  // a tie below
  const bool inv24 = o.overlap_inverse > 0 || (o.overlap_inverse < 0 && nb >= 24 && m_sched >= 2);
  const int inv_after24 = inv24 && nb >= 8 && in.inv_stream ? p.h - 1 : -1;
  // schedule: option "lookahead" = 2 (default by size: nb >= 8, at most 64 factorizations) -> reserved-CU lookahead
  // reserved-CU schedule with device-side dependencies: where the CHAIN of diagonal blocks sets the pace (few panels, or few
  // outputs per panel) it wins -- N = 2048 m = 4: 2.83 -> 2.52 ms, N = 3072: 5.4 -> 4.6, N = 4096 m = 1: 5.83 -> 4.57 -- where the
  // trailing updates do (N >= 6144 with m = 4: 17.7 vs 18.9 ms) the aggregated single-stream schedule does.
  // "lookahead" = 2 forces it, -1 (default) chooses by size, 0 never uses it.  (Removed in round 3, all measured slower in plain runs and
  // kept until then for A/B: 1 = next panel's diagonal block + row solve on a second stream with stream events, 3 / 4 = panel pairs with
  // lookahead on two / three masked streams; their numbers are in DESIGN.md 10 and profiles/r02.)
  // re-measured at the end of round 3 (tools/fit_schedule_sweep.sh, profiles/r03/fit_schedule_sweep.txt; the diagonal-block kernel, the row
  // products and the inverse all got faster since the rule was set, the cross-stream hand-overs did not): with two or more outputs the
  // single-stream schedule now wins from N = 2048 up by 10-50 % (N = 3072, m = 4: 3.62 against 5.38 ms; N = 4096, m = 2: 4.26 against 6.27);
  // the reserved-CU chain keeps ONE output (7-9 % at every size) and two outputs up to 12 panels (4 %)
  const bool reserved_auto = o.lookahead < 0 && nb >= 8 && ((m_sched == 1 && nb <= 32) || (m_sched == 2 && nb <= 12));
  // The gated (multi-stream) schedules are not used: after dependency time-outs (gated_off), for the redo of an attempt that timed out
  // (sched_retry), and for the FIRST factorization of a context -- it pays the one-time costs (code-object loads, allocations, stream
  // creation) that would otherwise sit between the launch of a polling kernel and the launch of the kernel it waits for.
  const bool gated_ok = in.cu_masks_ok && !in.gated_off && !in.sched_retry && in.refit;
  // resident teams: few panels, not after dependency time-outs, not for the redo of an attempt that timed out
  const bool team_ok = !in.gated_off && !in.sched_retry && (o.team_fit > 0 || (o.lookahead < 0 && o.aggregate <= 0));
  // by size (m = 4, Cholesky + inverse in ms, launched / teams): 9 panels 1.05 / 0.56, 12: 1.34 / 0.75, 16: 1.76 / 1.10, 20: 2.56 / 1.8, 24: 3.32 / 2.51,
  // 32: 5.23 / 5.84 -- from there the K = 128 .. 512 unit products of the teams (~0.2 TFLOP/s per CU) lose to the launched GEMMs
  const bool team_auto = o.team_fit < 0 && nb >= 2 && nb <= 24;
  if ((o.team_fit > 0 || team_auto) && team_ok && (nb <= o.team_whole_max || !o.team_hybrid) && nb >= 2 && ncu >= 4) {
    const int G = nb <= 24 ? 0 : o.team_panels;
    const bool whole = G <= 0 || G >= nb;                 // ONE launch: factorization and inverse [and Ky^-1]; else groups of G panels
    const int units = whole ? 2 * (nb * (nb + 1) / 2 - 1) + nb * (nb - 1) + (in.want_kinv ? nb * (nb + 1) : 0) : 2 * (G * nb - 1);
    const int T = chol_team_size(ncu, p.mb, units, 0);
    if (T >= 2 && (!whole || nb <= TEAM_MAX_NB)) {
      p.schedule = whole ? CHOL_TEAM_WHOLE : CHOL_TEAM_GROUPS;
      p.T = T;
      p.kinv = whole && in.want_kinv;
      p.panels = whole ? 0 : G;
      p.inv_after = whole ? -1 : inv_after24;
      team_flags();
      return p;
    }
  }
  if ((o.lookahead == 2 || reserved_auto) && gated_ok && nb >= (o.lookahead == 2 ? 2 : o.lookahead_min_nb) && m <= 64 && o.aggregate <= 0) {
    const int want = ((m + 7) / 8) * 8;                    // 8 k reserved CUs: k from every XCD
    if (want < ncu / 2) {                                  // (else not applicable on this device / for this many outputs)
      p.schedule = CHOL_RESERVED;
      p.reserved_cus = want;
      // the early inverse from 16 panels; it starts behind the row work of panel h - 1, which the last panel pair has none of
      const bool inv16 = o.overlap_inverse > 0 || (o.overlap_inverse < 0 && nb >= 16 && m_sched >= 2);
      p.inv_after = inv16 && in.inv_stream && nb >= 8 && nb - p.h >= 2 ? p.h - 1 : -1;
      p.flag_ints = (5 * nb + 1 + 3) / 4 * 4;              // 5 counters per panel + the time-out word (a multiple of 16 bytes)
      p.err_off = 5 * nb;
      return p;
    }
  }
  // measured (m = 4): N=2048 4 % slower, N=4096 3 % faster, N=8192 5 % faster -- the diagonal-block workgroup runs 1.6-2x
  // slower when it shares its CU with trailing-update waves, which eats most of what the overlap hides
  // measured (m = 4, ms): N=2048 3.82 / 3.90 / 4.13 for G = 1 / 2 / 4; N=4096 11.45 / 11.17 / 11.45; N=8192 56.3 / 50.4 / 48.7
  // re-measured with the MFMA diagonal-block kernel and the row-staged epilogue (profiles/r02/fit_schedule_sweep.txt):
  // G = 1 is best up to N = 3072, 2 at 4096, 3 at 6144 and 8192
  // (G = 3 at N = 4096 is 0.15 ms faster than G = 2 with the factor-wave diagonal kernel, but at cond(Ky) ~ 4e9 the other summation order moves
  // two of config 3's small acquisition values by 2.5e-5 relative, past the 1e-5 gate of test_config3_full_size: not taken)
  // re-measured at the end of round 3 (m = 4, Cholesky ms for G = 1 / 2 / 3): N = 2048 1.27 / 1.19 / 1.20, 2560 1.77 / 1.69 / 1.65, 3072 3.05 / 2.92 / 3.06,
  // 3584 3.65 / 3.49 / 3.66, 4096 4.73 / 4.30 / 4.16, 5120 9.71 / 9.30 / 9.27, 6144 13.6 / 12.8 / 12.4: pairs from 16 panels, triples from 32 (with alpha
  // refined every G sits a decade inside the truth gate of tests/test_gpu_round3.py, so the choice is a matter of speed only)
  const int G_use = o.aggregate > 0 ? o.aggregate : (nb >= 32 ? 3 : (nb >= 16 ? 2 : 1));
  // more than team_whole_max panels: the launched schedule (or team groups) for the first h block rows, one team launch for the last nb - h
  // (the split one level lower -- 8 + 24 panels at N = 4096 -- was measured: 6.5 ms against 4.9).  Chosen only when both parts apply.
  if (team_ok && (o.team_fit > 0 || (o.team_fit < 0 && o.lookahead < 0 && o.aggregate <= 0)) && nb > o.team_whole_max && o.team_hybrid &&
      nb - p.h <= 24 && nb - p.h >= 2 && in.inv_stream && ncu >= 4) {
    const int nt = nb - p.h;
    const int T_tail = chol_team_size(ncu, p.mb, 2 * (nt * (nt + 1) / 2 - 1) + nt * (nt - 1), o.team_tail_share);   // (leave CUs to the inverse underneath)
    const int panels = o.team_hybrid == 2 ? (o.team_panels > 0 ? o.team_panels : 4) : 0;
    const int T = panels > 0 ? chol_team_size(ncu, p.mb, 2 * (panels * nb - 1), 0) : 0;
    if (T_tail >= 2 && (panels == 0 || T >= 2)) {
      p.schedule = CHOL_HYBRID;
      p.G = G_use;
      p.panels = panels;
      p.T = T;
      p.T_tail = T_tail;
      p.inv_after = p.h - 1;
      team_flags();
      return p;
    }
  }
  p.schedule = CHOL_LAUNCHED;
  p.G = G_use > 1 && nb >= 2 * G_use ? G_use : 1;
  p.inv_after = inv_after24;
  return p;
}
