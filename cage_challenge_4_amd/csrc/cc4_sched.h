// cc4_sched.h -- the index arithmetic of the persistent schedule (cc4_persist.h; RunArgs in cc4_args.h), stated once: which episodes a
// partition and a policy group hold, what a ticket names, how a call's K steps are cut into runs, the layout of a progress word, the exchange's groups of
// 32.  Pure integer functions and constants -- no HIP builtin, no atomic, no argument block: the kernels, the gate kernels, the host units and the CPU
// oracle (oracle/cc4_oracle.cpp, cc4o_sched_*) all compile this one text, and tests/test_sched_cpu.py checks it against brute force without a GPU.
// The integer types are those of the device code that calls them: partition sizes are signed, a ticket and its counter's size are unsigned (the divisions
// on the lane that holds the ticket stay unsigned).
#pragma once
#include "cc4_rng.h"      // CC4_HD

namespace cc4 {

// ---- partitions: the batch is cut into P of them, one per CU; partition p holds episodes p, p + P, ..
CC4_HD constexpr int part_of(int e, int P) { return e % P; }
CC4_HD constexpr int part_episodes(int n, int P, int p) { return (n - p + P - 1) / P; }                 // <= 0: none (n < P)
CC4_HD constexpr int part_episode(int p, int P, int i) { return p + i * P; }                            // its episode number i

// ---- policy groups of a rollout: episode number i of a partition is of group i % PG, so every CU holds episodes of every group
CC4_HD constexpr int pgroup_of(int e, int P, int PG) { return (e / P) % PG; }
CC4_HD constexpr int pgroup_episodes(int ne, int PG, int g) { return (ne - g + PG - 1) / PG; }          // of a partition's ne episodes; <= 0: none
CC4_HD constexpr int pgroup_slot(int e, int P, int PG) { return (e % P) * PG + (e / P) % PG; }          // the (partition, group) counter that counts e
// threads over ONE group's episodes, whole blocks of P: thread i < pgroup_threads is episode pgroup_episode(i, ..) if that is below n
CC4_HD constexpr int pgroup_threads(int n, int P, int PG) { return ((n + P - 1) / P + PG - 1) / PG * P; }
CC4_HD constexpr int pgroup_episode(int i, int P, int PG, int g) { return ((i / P) * PG + g) * P + i % P; }

// ---- tickets: counter idx of partition `line` hands out the nph runs of the partition's episodes number idx, idx + pg, .. (pg = 1, idx = 0: all of them; a
// rollout: policy group idx of pg) in run-major order -- tickets 0 .. cnt-1 are run 0 of its cnt episodes, the next cnt are run 1, ..
CC4_HD constexpr uint32_t ticket_count(int n, int P, int line, int idx, int pg) { return (uint32_t)pgroup_episodes(part_episodes(n, P, line), pg, idx); }
CC4_HD constexpr uint32_t ticket_total(uint32_t cnt, int nph) { return cnt * (uint32_t)nph; }
CC4_HD constexpr uint32_t ticket_run(uint32_t t, uint32_t cnt) { return t / cnt; }                       // (cnt > 0: a ticket below ticket_total)
// (the same from a signed count, as part_episodes and pgroup_episodes give it -- checked > 0 by the caller; the division stays unsigned)
CC4_HD constexpr uint32_t ticket_total(int cnt, int nph) { return ticket_total((uint32_t)cnt, nph); }
CC4_HD constexpr uint32_t ticket_run(uint32_t t, int cnt) { return ticket_run(t, (uint32_t)cnt); }
CC4_HD constexpr void ticket_item(uint32_t t, uint32_t cnt, int line, int idx, int pg, int P, int& j, int& ee) {
  j = (int)ticket_run(t, cnt);
  ee = part_episode(line, P, (int)(t % cnt) * pg + idx);
}

// ---- runs: a call's K steps as nA runs of SA steps, then nB of SB, then single steps -- nph runs in all
struct RunSplit { int SA, nA, SB, nB, nph; };
CC4_HD constexpr RunSplit run_split_steps(int k) { return RunSplit{1, k, 1, 0, k}; }                     // every step a run of its own (a rollout; SA = 1)
// cfg*: CC4_PERSIST_RUNS = "SA,SB,nB,single" (cc4_handle::run_SA ..).  nB runs of SB steps and `single` single steps close the call, runs of SA fill the
// rest, and what is left over goes to the single steps.  SA = 0, the default: 4 steps, 8 from K >= 64.
CC4_HD constexpr RunSplit run_split(int k, int cfgSA, int cfgSB, int cfgnB, int cfgsingle) {
  const int SA = cfgSA > 0 ? cfgSA : (k >= 64 ? 8 : 4);
  if (SA <= 1) return run_split_steps(k);
  int single = cfgsingle < k ? cfgsingle : k;
  int nB = cfgSB > 1 ? cfgnB : 0;
  while (nB > 0 && single + nB * cfgSB > k) --nB;
  const int nA = (k - single - nB * cfgSB) / SA;
  single = k - nA * SA - nB * cfgSB;
  return RunSplit{SA, nA, cfgSB > 1 ? cfgSB : 1, nB, nA + nB + single};
}
// The pattern of a call, chosen on the host (run_args): an explicit CC4_PERSIST_RUNS passes through; so does the unset one (0,1,0,0) for a call of fewer than
// RUN_LONG_K steps -- run_split's default above, which every call shape of the tests and the hand-over cells is described by.  A LONG call with no
// pattern given gets runs of run_long_sa(k) steps, and what they leave over becomes ONE closing run instead of single steps (100 = 12 x 8 + one run of
// 4: 13 items an episode, not 16; 500 = 20 x 24 + one run of 20: 21, not 66) -- every item pays the hand-over between two items of a wave (DESIGN 3.3:
// about 8 us of the wave's time), a single step as much as a run of 8.
// The thresholds and lengths are measured values, profiles/r23_runs_k500.txt: at K = 100 the closing run gains 3.3 % on the default (runs of 8); at
// K = 500 it gains 1.0 % with runs of 8 and 2.2 - 2.8 % with runs of 16 to 32, a plateau on which 24 measured best in both sweeps -- taken only from
// the length it was measured at (at 250 and 300 steps longer runs are ahead but inside the noise bound, at 100 and 200 no different).  Longer runs
// WITHOUT the closing run lose: 24 and 32 leave 20 single steps.
// For the headline kernel k_run_philox1 ONLY (run_args' `head`, decided in persist_launch).  With the exchange on (k_run_philox1x) a run is held against the
// ring of 32 step slabs: a wave counts its item's last packed row only with its next item's first step (persist_step_out's pend_e), and that item's
// claim waits for the slab of ITS first step (xchg_wait_slab).  With runs of 24 the wave that finishes run j of an episode and draws a ticket of run
// j + 2 -- the ordinary order of 24 waves over a partition's 32 episodes -- waits for the gather of the chunk that ends with step 24 j + 23, which waits
// for the very count the wave holds: the launch stands until the exchange's watchdog (2 s) gives the exchange up.  Runs of 8 would need a ticket four
// runs ahead.  The other builds (plan, rollout, numpy stream, caller's actions) are out of this pattern's measurements and keep run_split's default.
struct RunConfig { int SA, SB, nB, single; };
constexpr int RUN_LONG_K = 100, RUN_LONG_SA = 8;              // from this many steps: runs of 8 and a closing run
constexpr int RUN_LONGER_K = 500, RUN_LONGER_SA = 24;         // from this many: runs of 24 and a closing run
CC4_HD constexpr int run_long_sa(int k) { return k >= RUN_LONGER_K ? RUN_LONGER_SA : RUN_LONG_SA; }
CC4_HD constexpr RunConfig run_config_for_call(int k, int cfgSA, int cfgSB, int cfgnB, int cfgsingle) {
  if (cfgSA != 0 || cfgSB != 1 || cfgnB != 0 || cfgsingle != 0 || k < RUN_LONG_K) return RunConfig{cfgSA, cfgSB, cfgnB, cfgsingle};
  const int SA = run_long_sa(k), rest = k % SA;
  return rest > 1 ? RunConfig{SA, rest, 1, 0} : RunConfig{SA, 1, 0, 0};       // (rest == 1: the one step left over is a single step)
}
CC4_HD constexpr RunSplit run_split_for_call(int k, int cfgSA, int cfgSB, int cfgnB, int cfgsingle) {
  const RunConfig c = run_config_for_call(k, cfgSA, cfgSB, cfgnB, cfgsingle);
  return run_split(k, c.SA, c.SB, c.nB, c.single);
}
// run j of the call: its first step and its length
CC4_HD constexpr void run_span(const RunSplit& s, int j, int& k0, int& len) {
  if (j < s.nA) { k0 = j * s.SA; len = s.SA; }
  else if (j < s.nA + s.nB) { k0 = s.nA * s.SA + (j - s.nA) * s.SB; len = s.SB; }
  else { k0 = s.nA * s.SA + s.nB * s.SB + (j - s.nA - s.nB); len = 1; }
}

// ---- the progress word of an episode: the steps it has completed since the words were last cleared in the low PROGRESS_STEP_BITS bits, above them the
// runner of its last run: 1 + the partition of that CU, RUNNER_NONE before the first run, RUNNER_FOREIGN for a CU that owns no partition
constexpr int PROGRESS_STEP_BITS = 23;
constexpr uint32_t PG_STEPS = (1u << PROGRESS_STEP_BITS) - 1u;
constexpr uint32_t RUNNER_NONE = 0u, RUNNER_FOREIGN = 511u;
constexpr int MAX_PARTITIONS = 510;                    // persist_setup refuses a device with more CUs
constexpr uint32_t PROGRESS_CLEAR_AT = 0x700000u;      // persist_launch clears the words in front of a call that would take them past this many steps
constexpr int ROLLOUT_MAX_K = 0x100000;                // cc4_rollout_begin: the longest rollout
constexpr int MAX_XCD_PARTITIONS = 64;                 // one lane per partition of the wave's XCD (pick_balanced) ..
constexpr int MAX_XCD_FIRST = 255;                     // .. whose first partition travels as a byte (RunArgs.xcc_lo)
CC4_HD constexpr uint32_t progress_pack(uint32_t steps, uint32_t runner) { return steps | (runner << PROGRESS_STEP_BITS); }
CC4_HD constexpr uint32_t progress_steps(uint32_t w) { return w & PG_STEPS; }
CC4_HD constexpr uint32_t progress_runner(uint32_t w) { return w >> PROGRESS_STEP_BITS; }
CC4_HD constexpr uint32_t runner_of(int own) { return own >= 0 ? (uint32_t)own + 1u : RUNNER_FOREIGN; }   // own: the CU's partition, < 0: it has none
static_assert(PROGRESS_CLEAR_AT + (uint32_t)ROLLOUT_MAX_K - 1u <= PG_STEPS, "a largest rollout on top of the clear threshold still fits the steps field");
static_assert(PROGRESS_STEP_BITS + 9 == 32 && RUNNER_FOREIGN < (1u << 9) && runner_of(MAX_PARTITIONS - 1) < RUNNER_FOREIGN && runner_of(0) != RUNNER_NONE,
              "the runner ids -- none, 1 + partition, foreign -- are distinct and fit the nine bits above the steps");
static_assert(progress_steps(progress_pack(PG_STEPS, RUNNER_FOREIGN)) == PG_STEPS && progress_runner(progress_pack(PG_STEPS, RUNNER_FOREIGN)) == RUNNER_FOREIGN, "round trip");

// ---- the exchange's groups.  The persistent kernels count episode e in its partition, part_of(e, G); the plain multi-step kernels (k_run_philox,
// k_run_philox8, k_run_philox1m) in groups of 32 neighbouring episodes:
CC4_HD constexpr int xchg_group32(int e) { return e >> 5; }
CC4_HD constexpr int xchg_group32_size(int n, int g) { return n - (g << 5) < 32 ? n - (g << 5) : 32; }   // what the gate waits for; <= 0: none
CC4_HD constexpr int xchg_groups32(int n) { return (n + 31) / 32; }                                       // the groups that hold an episode
CC4_HD constexpr int xchg_groups32_alloc(int n) { return n / 32 + 1; }                                    // counter rows the handle allocates: never fewer, never none

// ---- known cases
constexpr bool same_split(const RunSplit& a, int SA, int nA, int SB, int nB, int nph) { return a.SA == SA && a.nA == nA && a.SB == SB && a.nB == nB && a.nph == nph; }
static_assert(same_split(run_split(20, 0, 1, 0, 0), 4, 5, 1, 0, 5), "the default split of 20 steps: five runs of 4");
static_assert(same_split(run_split(500, 0, 1, 0, 0), 8, 62, 1, 0, 66), "the default split of 500 steps: 62 runs of 8, then 4 single steps");
static_assert(same_split(run_split(7, 1, 1, 0, 0), 1, 7, 1, 0, 7) && same_split(run_split(30, 8, 2, 3, 1), 8, 2, 2, 3, 13), "SA = 1: every step a run; 8,2,3,1 on 30 steps: 16 + 6 + 8 single");
static_assert(same_split(run_split_for_call(99, 0, 1, 0, 0), 8, 12, 1, 0, 15) && same_split(run_split_for_call(100, 0, 1, 0, 0), 8, 12, 4, 1, 13) &&
              same_split(run_split_for_call(500, 0, 1, 0, 0), 24, 20, 20, 1, 21) && same_split(run_split_for_call(505, 0, 1, 0, 0), 24, 21, 1, 0, 22) &&
              same_split(run_split_for_call(500, 8, 1, 0, 0), 8, 62, 1, 0, 66), "a long call with no pattern given: what is left over is one closing run; an explicit pattern stays");
static_assert(part_episodes(5000, 256, 135) == 20 && part_episodes(5000, 256, 136) == 19 && part_episodes(3, 8, 5) == 0, "5000 episodes on 256 CUs: 136 partitions of 20, 120 of 19");
static_assert(ticket_count(5000, 256, 136, 3, 4) == 4u && ticket_count(3, 8, 1, 1, 2) == 0u, "19 episodes in 4 groups: 5 5 5 4; one episode: nothing in group 1");
static_assert(pgroup_slot(pgroup_episode(700, 256, 4, 3), 256, 4) == part_of(700, 256) * 4 + 3 && xchg_groups32(5000) == 157 && xchg_group32_size(5000, 156) == 8, "");

}  // namespace cc4
