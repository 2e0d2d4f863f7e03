// Stand-alone check of the run pattern the host chooses for a persistent call (csrc/cc4_sched.h: run_config_for_call, run_split, run_span), built with
// the host compiler and the address / undefined-behaviour sanitizers and run as a child process by tests/test_run_pattern_cpu.py.  For every call length
// k = 1 .. 2000: the runs of run_split(k, run_config_for_call(k, default)) tile the k steps exactly, every run is at least one step long and nph counts
// them; below RUN_LONG_K the split is run_split's own default field for field; at and above it there is no single-step item unless k % run_long_sa(k) == 1,
// and what the runs of SA leave over is ONE closing run; an explicit pattern passes through unchanged at every k.  Exit status 0: no failure.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../cage_challenge_4_amd/csrc/cc4_sched.h"
using namespace cc4;

static long fails = 0, checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { if (fails++ < 30) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// the runs of a split, walked as the kernel walks them: every step of the call is covered once, in order; returns the number of one-step runs
static int walk(const RunSplit& s, int k, const char* what) {
  std::vector<int> seen((size_t)k, 0);     // exactly k entries: a run past the call's end is the sanitizer's finding
  int next = 0, singles = 0;
  CHECK(s.nph >= 1 && s.nph <= k, "%s k=%d: nph %d", what, k, s.nph);
  CHECK(s.nA >= 0 && s.nB >= 0 && s.SA >= 1 && s.SB >= 1, "%s k=%d: SA %d nA %d SB %d nB %d", what, k, s.SA, s.nA, s.SB, s.nB);
  for (int j = 0; j < s.nph; ++j) {
    int k0 = -1, len = -1;
    run_span(s, j, k0, len);
    CHECK(len >= 1, "%s k=%d: run %d has %d steps", what, k, j, len);
    CHECK(k0 == next, "%s k=%d: run %d starts at step %d, the run before it ended at %d", what, k, j, k0, next);
    if (len < 1 || k0 != next || k0 + len > k) { CHECK(k0 + len <= k, "%s k=%d: run %d = [%d, %d) leaves the call", what, k, j, k0, k0 + len); return -1; }
    for (int q = 0; q < len; ++q) ++seen[(size_t)(k0 + q)];
    next = k0 + len;
    if (len == 1) ++singles;
  }
  CHECK(next == k, "%s k=%d: the runs cover %d steps", what, k, next);
  for (int q = 0; q < k; ++q) CHECK(seen[(size_t)q] == 1, "%s k=%d: step %d covered %d times", what, k, q, seen[(size_t)q]);
  return singles;
}
static bool same(const RunSplit& a, const RunSplit& b) { return a.SA == b.SA && a.nA == b.nA && a.SB == b.SB && a.nB == b.nB && a.nph == b.nph; }

int main() {
  static_assert(RUN_LONG_K > 70, "calls of up to 70 steps keep run_split's default: the hand-over tests describe them by it");
  static_assert(RUN_LONG_SA >= 2 && RUN_LONGER_SA >= RUN_LONG_SA && RUN_LONGER_K >= RUN_LONG_K, "a long call's runs are runs, a longer call's are no shorter");
  const int explicit_cfg[][4] = {{1, 1, 0, 0}, {4, 2, 2, 2}, {8, 2, 3, 1}, {16, 1, 0, 0}, {8, 4, 1, 0}, {0, 2, 3, 1}, {32, 20, 1, 0}, {3, 1, 0, 5}};
  for (int k = 1; k <= 2000; ++k) {
    const RunConfig c = run_config_for_call(k, 0, 1, 0, 0);
    const RunSplit s = run_split(k, c.SA, c.SB, c.nB, c.single);
    const int singles = walk(s, k, "default");
    if (k < RUN_LONG_K) {
      CHECK(c.SA == 0 && c.SB == 1 && c.nB == 0 && c.single == 0, "k=%d below the threshold: the configuration changed to %d,%d,%d,%d", k, c.SA, c.SB, c.nB, c.single);
      CHECK(same(s, run_split(k, 0, 1, 0, 0)), "k=%d below the threshold: not run_split's default", k);
    } else {
      const int SA = run_long_sa(k), rest = k % SA;
      CHECK(SA == (k >= RUN_LONGER_K ? RUN_LONGER_SA : RUN_LONG_SA), "k=%d: runs of %d", k, SA);
      CHECK(s.SA == SA && s.nA == k / SA, "k=%d: %d runs of %d", k, s.nA, s.SA);
      CHECK(singles == (rest == 1 ? 1 : 0), "k=%d: %d single-step items (k %% SA = %d)", k, singles, rest);
      CHECK(s.nph == k / SA + (rest ? 1 : 0), "k=%d: nph %d -- what is left over is one closing run", k, s.nph);
    }
    for (const auto& q : explicit_cfg) {
      const RunConfig e = run_config_for_call(k, q[0], q[1], q[2], q[3]);
      CHECK(e.SA == q[0] && e.SB == q[1] && e.nB == q[2] && e.single == q[3], "k=%d: the explicit pattern %d,%d,%d,%d came back as %d,%d,%d,%d", k, q[0], q[1], q[2], q[3], e.SA, e.SB, e.nB, e.single);
      (void)walk(run_split(k, e.SA, e.SB, e.nB, e.single), k, "explicit");
    }
  }
  printf("run_pattern_check: from %d steps runs of %d, from %d runs of %d, %ld checks, %ld failures\n", RUN_LONG_K, RUN_LONG_SA, RUN_LONGER_K, RUN_LONGER_SA, checks, fails);
  return fails ? 1 : 0;
}
