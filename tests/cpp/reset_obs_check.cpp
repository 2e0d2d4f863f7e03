// Stand-alone run of the scenario generation and the four observation enumerations of csrc/cc4_engine.h on the host build of the engine
// (tests/test_reset_obs_cpu.py builds this with the host compiler and the address / undefined-behaviour sanitizers and runs it as a child
// process).  64 seeds in each RNG mode: a fresh env_reset, 12 steps of random actions and messages, a continued reset, 12 more steps, a
// second continued reset.  The hot row, the cold row and the work areas are heap blocks of exactly their size, so that a store of the
// generation outside them is the sanitizer's finding.  On every state the 578 observation values are enumerated four ways -- part by part
// (env_flat_obs), by position (env_flat_obs_at), by kind (env_flat_obs_sorted), and the per-step values from the table form
// (obs_fast_entry / obs_fast_value) -- and must agree.  The four are not independent witnesses: they share the layout helpers (obs_block_pos,
// obs_block_value, obs_msg_*), and the by-kind enumeration reads its first 384 values through the table, so this finds a disagreement between
// the part-by-part loops and the helpers, a position named twice or never, and memory errors -- not a mistake inside a shared helper.  The
// layout itself is pinned by the reference's goldens (tests/test_oracle_golden.py).  Exit status 0: every value agreed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../cage_challenge_4_amd/csrc/cc4_engine.h"
using namespace cc4;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static long fails = 0, cases = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "MISMATCH %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static void check_obs(const EnvState* s, int mode, int seed, const char* stage) {
  int32_t by_part[OBS_TOTAL], by_kind[OBS_TOTAL], hits[OBS_TOTAL];
  env_flat_obs<int32_t>(s, by_part);
  for (int i = 0; i < OBS_TOTAL; ++i) { by_kind[i] = -1; hits[i] = 0; }
  for (int v = 0; v < OBS_TOTAL; ++v) {
    int idx = -1;
    const int val = env_flat_obs_sorted(s, v, &idx);
    CHECK(idx >= 0 && idx < OBS_TOTAL, "mode %d seed %d %s: value %d of the by-kind enumeration names position %d", mode, seed, stage, v, idx);
    if (idx < 0 || idx >= OBS_TOTAL) continue;
    by_kind[idx] = val; hits[idx]++;
    if (v < OBS_FAST) {
      const uint32_t e = obs_fast_entry(v);
      CHECK((int)(e & 0x3FFu) == idx && obs_fast_value(e, s) == val, "mode %d seed %d %s: table entry %d", mode, seed, stage, v);
    }
  }
  for (int i = 0; i < OBS_TOTAL; ++i) {
    const int at = env_flat_obs_at(s, i);
    CHECK(hits[i] == 1 && by_part[i] == at && by_part[i] == by_kind[i], "mode %d seed %d %s: position %d: by part %d, by position %d, by kind %d (named %d times)",
          mode, seed, stage, i, by_part[i], at, by_kind[i], hits[i]);
  }
}

int main() {
  const int steps = 500, seeds = 64, between = 12;
  long regenerated = 0, nonzero = 0;
  for (int mode = 0; mode < 2; ++mode)
    for (int seed = 0; seed < seeds; ++seed) {
      EnvState* s = (EnvState*)calloc(1, sizeof(EnvState));
      EnvCold* c = (EnvCold*)calloc(1, cold_row_bytes(steps));
      StepWork* w = (StepWork*)calloc(1, sizeof(StepWork));
      uint32_t* ws = (uint32_t*)calloc(RESET_WS_WORDS, sizeof(uint32_t));
      if (!s || !c || !w || !ws) { fprintf(stderr, "out of memory\n"); return 2; }
      Ctx x{s, c, &s->rng, s->hd, w};
      for (int round = 0; round < 3; ++round) {
        env_reset(x, 9000 + (uint64_t)seed, mode, steps, round > 0, 0, 0, mode == 1 ? ws : nullptr);
        ++regenerated;
        CHECK(s->err == 0 && s->step_count == 0 && s->rng_mode == mode && s->n_green >= 3 * (NSUB - 1), "mode %d seed %d round %d: err %u step %d greens %d",
              mode, seed, round, (unsigned)s->err, (int)s->step_count, (int)s->n_green);
        check_obs(s, mode, seed, round == 0 ? "fresh reset" : "continued reset");
        if (round == 2) break;
        for (int t = 0; t < between; ++t) {
          int32_t act[NBLUE]; uint8_t msg[NBLUE * MSG_LEN];
          for (int b = 0; b < NBLUE; ++b) act[b] = (int32_t)(rnd() % (uint64_t)(b == 4 ? ACT_LONG : ACT_SHORT));
          for (int i = 0; i < NBLUE * MSG_LEN; ++i) msg[i] = (uint8_t)(rnd() & 1u);
          memset(w, 0, sizeof(StepWork));
          env_step(x, act, msg);
          check_obs(s, mode, seed, "step");
          for (int h = 0; h < MAXH; ++h) nonzero += s->hev[h] != 0;
        }
      }
      free(ws); free(w); free(c); free(s);
    }
  CHECK(nonzero > 0, "no host event in any stepped state: the event values were never exercised");
  printf("reset_obs_check: %ld generations, %ld checks, %ld mismatches\n", regenerated, cases, fails);
  return fails ? 1 : 0;
}
