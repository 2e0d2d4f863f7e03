// Stand-alone check of the host side of the reward terms (csrc/cc4_reward_terms.h): reward_terms_from_row -- the serial statement of what
// k_reward_terms computes, built from the same per-item functions -- on rows and records filled by hand, against a restatement that shares nothing
// with it: the BlueRewardMachine table written out as in Shared/BlueRewardMachine.py, host / 17, the zone list (tests/test_reward_terms_cpu.py builds
// this with the host compiler and the address / undefined-behaviour sanitizers and runs it as a child process).  The hot row and the record are heap
// blocks of exactly their size, so a read past either is the sanitizer's finding.  Covered: a stamp stale by one, equal, and 0 on a row that has
// taken no step; n_green 0, 80 and past 80; all bits of the six bitmap words set; bits above n_green; green hosts and an Impact host at 136, 137 and
// 255; an Impact without a session; a failure whose weight is 0; every pattern of the five Restore stamps; a phase outside the table; no cold row.
// Exit status 0: every case agreed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include "../../cage_challenge_4_amd/csrc/cc4_reward_terms.h"
using namespace cc4;

static long fails = 0, cases = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "MISMATCH %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// BlueRewardMachine.get_phase_rewards: [phase][subnet][LWF, ASF, RIA]
static const int TAB[3][9][3] = {
  {{-1, -3, -1}, {-1, -1, -1}, {-1, -3, -1}, {-1, -1, -1}, {0, -5, -5}, {-1, -1, -3}, {-1, -1, -3}, {-1, -1, -3}, {0, 0, -1}},
  {{-2, -1, -3}, {-10, 0, -10}, {-1, -1, -1}, {-1, -1, -1}, {0, 0, 0}, {-1, -1, -3}, {-1, -1, -3}, {-1, -1, -3}, {0, 0, 0}},
  {{-1, -3, -3}, {-1, -1, -1}, {-2, -1, -3}, {-10, 0, -10}, {0, 0, 0}, {-1, -1, -3}, {-1, -1, -3}, {-1, -1, -3}, {0, 0, 0}}};
static const int ZONE[9] = {0, 1, 2, 3, -1, 4, 4, 4, -1};

static int32_t terms[RT_CELLS], words[RT_WORDS];

// the restatement: nothing of cc4_reward_terms.h
static void expect(const EnvState* s, const RewardRec* r, int32_t* T, int32_t* W) {
  memset(T, 0, sizeof(int32_t) * 36); memset(W, 0, sizeof(int32_t) * 16);
  W[1] = s->step_count; W[2] = s->phase;
  if (!r || s->step_count < 1 || r->stamp != (uint32_t)s->step_count) return;
  W[0] = 1;
  const bool phase_ok = s->phase >= 0 && s->phase <= 2;
  const int ng = s->n_green > 80 ? 80 : s->n_green;
  for (int g = 0; g < ng && phase_ok; ++g) {
    const int h = s->green_host[g];
    if (h >= 137) continue;
    if ((r->lwf[g / 32] >> (g % 32)) & 1u) { T[(h / 17) * 4 + 0] += TAB[s->phase][h / 17][0]; T[(h / 17) * 4 + 3] += 1; }
    if ((r->asf[g / 32] >> (g % 32)) & 1u) { T[(h / 17) * 4 + 1] += TAB[s->phase][h / 17][1]; T[(h / 17) * 4 + 3] += 1; }
  }
  for (int a = 0; a < 6 && phase_ok; ++a) {
    const RedHdr& hd = s->red[a].h;
    if (hd.exec_type != RA_IMPACT || hd.nsess == 0 || hd.exec_host >= 137) continue;
    T[(hd.exec_host / 17) * 4 + 2] += TAB[s->phase][hd.exec_host / 17][2]; T[(hd.exec_host / 17) * 4 + 3] += 1;
  }
  for (int sn = 0; sn < 9; ++sn) {
    const int v = T[sn * 4] + T[sn * 4 + 1] + T[sn * 4 + 2];
    W[3] += v;
    W[ZONE[sn] < 0 ? 10 : 5 + ZONE[sn]] += v;
  }
  for (int b = 0; b < 5; ++b) if (r->restore_at[b] == r->stamp) { W[4] -= 1; W[5 + b] -= 1; W[11 + b] = -1; }
}
static void compare(const EnvState* s, const RewardRec* r, const char* what) {
  int32_t T[36], W[16];
  expect(s, r, T, W);
  memset(terms, 0x5A, sizeof terms); memset(words, 0x5A, sizeof words);
  reward_terms_from_row(s, r, terms, words);
  for (int k = 0; k < 36; ++k) CHECK(terms[k] == T[k], "%s: terms[%d][%d] = %d, expected %d", what, k / 4, k % 4, terms[k], T[k]);
  for (int k = 0; k < 16; ++k) CHECK(words[k] == W[k], "%s: words[%d] = %d, expected %d", what, k, words[k], W[k]);
  if (words[0]) {
    int sh = words[10];
    for (int b = 0; b < 5; ++b) sh += words[5 + b];
    CHECK(sh == words[3] + words[4], "%s: the shares add up to %d, brm + cost = %d", what, sh, words[3] + words[4]);
    for (int k = 0; k < 36; ++k) if (k % 4 != 3) CHECK(terms[k] <= 0, "%s: terms[%d][%d] = %d > 0", what, k / 4, k % 4, terms[k]);
  } else {
    for (int k = 0; k < 36; ++k) CHECK(terms[k] == 0, "%s: terms[%d] = %d with valid 0", what, k, terms[k]);
    for (int k = 0; k < 16; ++k) if (k != 1 && k != 2) CHECK(words[k] == 0, "%s: words[%d] = %d with valid 0", what, k, words[k]);
  }
}
static void set_impact(EnvState* s, int a, int type, int host, int nsess) {
  s->red[a].h.exec_type = (uint8_t)type; s->red[a].h.exec_host = (uint8_t)host; s->red[a].h.nsess = (uint8_t)nsess;
}

int main() {
  EnvState* s = static_cast<EnvState*>(aligned_alloc(alignof(EnvState), sizeof(EnvState)));
  RewardRec* r = static_cast<RewardRec*>(aligned_alloc(alignof(RewardRec), sizeof(RewardRec)));      // exactly the record
  if (!s || !r) return 2;
  memset(s, 0, sizeof(EnvState));
  memset(r, 0, sizeof(RewardRec));
  CHECK(sizeof(RewardRec) == 64 && offsetof(EnvCold, rwd) % 16 == 0 && sizeof(EnvCold) % 16 == 0, "record %zu bytes at %zu, fixed part %zu", sizeof(RewardRec),
        offsetof(EnvCold, rwd), sizeof(EnvCold));
  CHECK(offsetof(EnvCold, rwd) >= offsetof(EnvCold, xrate) && offsetof(EnvCold, rwd) + sizeof(RewardRec) <= sizeof(EnvCold), "the record lies in the tail span");
  for (int p = 0; p < 3; ++p) for (int sn = 0; sn < 9; ++sn) for (int w = 0; w < 3; ++w)
    CHECK(reward_table_fn(p, sn, w) == TAB[p][sn][w], "the engine's table at (%d, %d, %d)", p, sn, w);

  // the green agents: subnet by subnet as reset fills them, ten per subnet on the user slots 1..10 of the eight subnets with hosts
  for (int g = 0; g < MAXG; ++g) s->green_host[g] = (uint8_t)((g / 10) * 17 + 1 + g % 10);
  s->steps = 500; s->step_count = 7; s->phase = 1; s->n_green = 80;
  for (int a = 0; a < NRED; ++a) set_impact(s, a, RA_SLEEP, 0, 1);

  // ---- a full record whose stamp is stale by one, and one from the future: nothing but step_count and phase
  memset(r, 0xFF, sizeof(RewardRec));
  r->stamp = 6; for (int b = 0; b < NBLUE; ++b) r->restore_at[b] = 6;
  set_impact(s, 2, RA_IMPACT, 20, 3);
  compare(s, r, "stamp stale by one");
  CHECK(words[0] == 0 && words[1] == 7 && words[2] == 1, "stale: %d %d %d", words[0], words[1], words[2]);
  r->stamp = 8;
  compare(s, r, "stamp ahead by one");
  CHECK(words[0] == 0, "ahead: valid %d", words[0]);
  // ---- no cold row
  compare(s, nullptr, "no cold row");
  CHECK(words[0] == 0 && words[1] == 7, "null: %d %d", words[0], words[1]);
  // ---- a row that has taken no step, with a zeroed record (a regenerated episode): stamp == step_count == 0 is not valid
  s->step_count = 0; memset(r, 0, sizeof(RewardRec));
  compare(s, r, "no step taken");
  CHECK(words[0] == 0, "no step: valid %d", words[0]);
  s->step_count = 7;

  // ---- stamp equal, all bits of the six bitmap words set (80 agents charged both kinds, 16 bits above MAXG), the Impact of above, in every phase
  for (int p = 0; p < 3; ++p) {
    s->phase = p;
    memset(r, 0, sizeof(RewardRec));
    r->stamp = 7;
    for (int w = 0; w < 3; ++w) { r->lwf[w] = 0xFFFFFFFFu; r->asf[w] = 0xFFFFFFFFu; }
    compare(s, r, "all bits");
    CHECK(words[0] == 1 && words[4] == 0, "all bits: valid %d cost %d", words[0], words[4]);
    int ev = 0;
    for (int sn = 0; sn < 9; ++sn) ev += terms[sn * 4 + 3];
    CHECK(ev == 161, "all bits, phase %d: %d events", p, ev);
    CHECK(terms[1 * 4 + 3] == 21 && terms[8 * 4 + 3] == 0, "events of subnet 1: %d, of the internet: %d", terms[1 * 4 + 3], terms[8 * 4 + 3]);
  }
  // phase 1, subnet 1: ten LocalWork failures at -10, ten AccessService failures at 0, the Impact on host 20 at -10
  s->phase = 1;
  compare(s, r, "phase 1");
  CHECK(terms[4] == -100 && terms[5] == 0 && terms[6] == -10 && terms[7] == 21 && words[6] == -110, "subnet 1: %d %d %d %d, agent 1: %d", terms[4], terms[5], terms[6], terms[7], words[6]);
  // the contractor network in phase 1 costs nothing: 20 events, no penalty, nothing unowned
  CHECK(terms[16] == 0 && terms[17] == 0 && terms[19] == 20 && words[10] == 0, "subnet 4: %d %d %d, unowned %d", terms[16], terms[17], terms[19], words[10]);

  // ---- n_green: 0, 10 (bits above it set), past MAXG (clamped)
  for (int ng : {0, 1, 10, 64, 65, 79, 80, 81, 200, 255}) {
    s->n_green = (uint8_t)ng;
    compare(s, r, "n_green");
    int ev = 0;
    for (int sn = 0; sn < 9; ++sn) ev += terms[sn * 4 + 3];
    CHECK(ev == 2 * (ng > 80 ? 80 : ng) + 1, "n_green %d: %d events", ng, ev);
  }
  s->n_green = 80;

  // ---- green hosts past the table: 137 and 255 contribute nothing, 136 (the internet root) is subnet 8
  s->phase = 0;
  s->green_host[3] = 137; s->green_host[4] = 255; s->green_host[79] = 136; s->green_host[64] = 137;
  compare(s, r, "green hosts past the table");
  CHECK(terms[0 * 4 + 3] == 16 && terms[8 * 4 + 3] == 2 && terms[7 * 4 + 3] == 18, "events %d %d %d", terms[3], terms[8 * 4 + 3], terms[7 * 4 + 3]);
  for (int g = 0; g < MAXG; ++g) s->green_host[g] = (uint8_t)((g / 10) * 17 + 1 + g % 10);

  // ---- Impacts: host 136 (-1 in phase 0, unowned), 137 and 255 (nothing), no session (nothing), another action type (nothing), all six at once
  memset(r, 0, sizeof(RewardRec)); r->stamp = 7;
  set_impact(s, 2, RA_SLEEP, 0, 1);
  for (int host : {0, 16, 17, 68, 84, 85, 135, 136, 137, 200, 255}) {
    set_impact(s, 5, RA_IMPACT, host, 1);
    compare(s, r, "impact host");
    CHECK(words[3] == (host < 137 ? TAB[0][host / 17][2] : 0), "impact on %d: brm %d", host, words[3]);
  }
  set_impact(s, 5, RA_IMPACT, 136, 1);
  compare(s, r, "impact on the internet root");
  CHECK(terms[8 * 4 + 2] == -1 && terms[8 * 4 + 3] == 1 && words[10] == -1 && words[3] == -1, "internet: %d %d unowned %d", terms[34], terms[35], words[10]);
  set_impact(s, 5, RA_IMPACT, 20, 0);
  compare(s, r, "impact without a session");
  CHECK(words[3] == 0, "no session: brm %d", words[3]);
  for (int a = 0; a < NRED; ++a) set_impact(s, a, RA_IMPACT, 70 + a * 10, 255);
  compare(s, r, "six impacts");
  int ev6 = 0;
  for (int sn = 0; sn < 9; ++sn) ev6 += terms[sn * 4 + 3];
  CHECK(ev6 == 6, "six impacts: %d events", ev6);
  for (int a = 0; a < NRED; ++a) set_impact(s, a, RA_SLEEP, 0, 1);

  // ---- every pattern of the five Restore stamps: equal to the stamp, stale by one, zero
  r->lwf[0] = 1u;                                                   // agent 0 of subnet 0 failed LocalWork: -1 in phase 0
  for (int m = 0; m < 32; ++m)
    for (uint32_t other : {0u, 6u, 8u}) {
      for (int b = 0; b < NBLUE; ++b) r->restore_at[b] = ((m >> b) & 1) ? 7u : other;
      compare(s, r, "restore pattern");
      CHECK(words[4] == -__builtin_popcount((unsigned)m) && words[3] == -1, "pattern %d: cost %d brm %d", m, words[4], words[3]);
      for (int b = 0; b < NBLUE; ++b) CHECK(words[11 + b] == -((m >> b) & 1) && words[5 + b] == -((m >> b) & 1) - (b == 0), "pattern %d agent %d", m, b);
    }

  // ---- a phase outside the table charges nothing (and indexes nothing)
  memset(r, 0xFF, sizeof(RewardRec)); r->stamp = 7;
  set_impact(s, 1, RA_IMPACT, 20, 1);
  for (int p : {3, 255, -1}) {
    s->phase = p;
    compare(s, r, "phase outside the table");
    CHECK(words[0] == 1 && words[3] == 0, "phase %d: valid %d brm %d", p, words[0], words[3]);
  }

  printf("reward_terms_check: %ld checks, %ld mismatches\n", cases, fails);
  free(s); free(r);
  return fails ? 1 : 0;
}
