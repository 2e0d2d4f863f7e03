// Stand-alone check of the table form of the red FSM's option switch and of the per-lane forms of the step's single-lane sections in
// csrc/cc4_engine.h against the serial forms the header keeps (tests/test_fsm_tail_forms_cpu.py builds this with the host compiler and the
// address / undefined-behaviour sanitizers and runs it as a child process).  Exit status 0: every case agreed.
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

static EnvState* s;
static StepWork work;

// the serial reservation and every agent's lane form on the same pool and actions
static void check_reserve(const uint32_t used[RS_POOL / 32], uint32_t exploit, const char* what) {
  for (int w = 0; w < RS_POOL / 32; ++w) s->spool_used[w] = used[w];
  for (int r = 0; r < NRED; ++r) {
    Act a{};
    // the agents without an Exploit hold any other type, RA_NONE among them
    int ty = (int)(rnd() % 11);
    if (ty >= RA_EXPLOIT) ++ty;
    a.type = (uint8_t)(((exploit >> r) & 1u) ? (int)RA_EXPLOIT : ty);
    s->rexec[r] = a;
  }
  memset(work.rs_slot, 0xAA, sizeof(work.rs_slot));
  Ctx x{s, nullptr, &s->rng, nullptr, &work};
  rs_reserve(x);
  for (int w = 0; w < RS_POOL / 32; ++w) CHECK(s->spool_used[w] == used[w], "%s: rs_reserve changed spool_used", what);   // it only plans
  int want_free = 0;
  for (int w = 0; w < RS_POOL / 32; ++w) want_free += 32 - __builtin_popcount(used[w]);
  int asked = 0;
  for (int r = 0; r < NRED; ++r) {
    const int lane = rs_reserve_lane(s, exploit, r);
    CHECK(lane == (int)work.rs_slot[r], "%s: exploit %02x agent %d: lane form %d, serial %d (used %08x %08x %08x %08x %08x %08x)", what, exploit, r, lane,
          (int)work.rs_slot[r], used[0], used[1], used[2], used[3], used[4], used[5]);
    if ((exploit >> r) & 1u) { CHECK((lane == 0xFF) == (asked >= want_free), "%s: agent %d is asker %d of a pool with %d free, slot %d", what, r, asked, want_free, lane); ++asked; }
    else CHECK(lane == 0xFF, "%s: agent %d has no Exploit, slot %d", what, r, lane);
  }
}

int main() {
  // ---- the option table of fsm_get_action against its switch: both policies, every state value 0..255
  for (int d = 0; d < 2; ++d)
    for (int st = 0; st <= 0xFF; ++st)
      CHECK(fsm_pk(d != 0, st) == fsm_pk_switch(d != 0, st), "fsm_pk discovery %d state %d: %08x vs %08x", d, st, fsm_pk(d != 0, st), fsm_pk_switch(d != 0, st));

  s = (EnvState*)calloc(1, sizeof(EnvState));
  if (!s) return 2;
  // ---- item 4: the lane form of the slot reservation against rs_reserve
  const int NW = RS_POOL / 32;
  for (uint32_t exploit = 0; exploit < (1u << NRED); ++exploit) {
    uint32_t used[NW];
    // empty and full pool
    for (int w = 0; w < NW; ++w) used[w] = 0; check_reserve(used, exploit, "empty pool");
    for (int w = 0; w < NW; ++w) used[w] = 0xFFFFFFFFu; check_reserve(used, exploit, "full pool");
    // the next free records straddle every word boundary: everything used below boundary b except the last j records of word b - 1, for
    // every j 0..6 (six askers at most), the words above either free, or used but for a few records
    for (int b = 1; b <= NW; ++b)
      for (int j = 0; j <= NRED; ++j)
        for (int above = 0; above < 4; ++above) {
          for (int w = 0; w < NW; ++w) used[w] = w < b ? 0xFFFFFFFFu : (above == 0 ? 0u : (above == 1 ? 0xFFFFFFFEu : (above == 2 ? 0x7FFFFFFFu : 0xFFFFFFFFu)));
          if (j) used[b - 1] &= ~(((1u << j) - 1u) << (32 - j));
          check_reserve(used, exploit, "word boundary");
          // ... and with holes spread over several words below it (one free record per word)
          for (int w = 0; w + 1 < b; ++w) used[w] &= ~(1u << ((7 * w + j) & 31));
          check_reserve(used, exploit, "one hole per word");
        }
    // exactly n free records, n 0..7, placed at random: fewer free records than askers gives 0xFF to the rest
    for (int n = 0; n <= NRED + 1; ++n)
      for (int rep = 0; rep < 40; ++rep) {
        for (int w = 0; w < NW; ++w) used[w] = 0xFFFFFFFFu;
        for (int k = 0; k < n;) { const int bit = (int)(rnd() % RS_POOL); if ((used[bit >> 5] >> (bit & 31)) & 1u) { used[bit >> 5] &= ~(1u << (bit & 31)); ++k; } }
        check_reserve(used, exploit, "n free records");
      }
    // random fills of every density
    for (int rep = 0; rep < 400; ++rep) {
      for (int w = 0; w < NW; ++w) { uint32_t v = (uint32_t)rnd(); for (int k = 0; k < rep % 6; ++k) v |= (uint32_t)rnd(); if (rep % 7 == 0) v &= (uint32_t)rnd(); used[w] = v; }
      check_reserve(used, exploit, "random fill");
    }
  }
  // ---- item 5: the ballot of the agents' own pend_r slots is non-zero exactly when step_red_merge appends something, and a step without one leaves
  // everything as the merge would
  for (uint32_t mask = 0; mask < (1u << NRED); ++mask)
    for (int full = 0; full < 2; ++full) {
      for (int r = 0; r < NRED; ++r) work.pend_r[r] = ((mask >> r) & 1u) ? ((uint32_t)(r + 1) << 16) | (uint32_t)(100 + r) : 0u;
      s->npend = (uint8_t)(full ? MAX_PEND : 2); s->pend[0] = 0x10001u; s->pend[1] = 0x20002u; s->err = 0;
      bool any = false;
      for (int r = 0; r < NRED; ++r) any = any || work.pend_r[r] != 0;
      const int before = s->npend;
      Ctx x{s, nullptr, &s->rng, nullptr, &work};
      step_red_merge(x);
      const bool changed = s->npend != before || s->err != 0;
      CHECK(changed == any, "pend_r mask %02x (list %s): ballot %d, merge changed %d", mask, full ? "full" : "short", (int)any, (int)changed);
      for (int r = 0; r < NRED; ++r) CHECK(work.pend_r[r] == 0, "pend_r[%d] cleared", r);
      if (!full) { int k = 2; for (int r = 0; r < NRED; ++r) if ((mask >> r) & 1u) { CHECK(s->pend[k] == (((uint32_t)(r + 1) << 16) | (uint32_t)(100 + r)), "agent order, entry %d", k); ++k; } CHECK(k == s->npend, "count"); }
    }
  s->npend = 0; s->err = 0;
  // ---- item 6: the agents' own Impact terms added to brm, then step_end without its loop, against step_end: every phase x subnet x set of
  // Impact agents, with the other agents holding every other action type, agents without sessions, and other terms already in brm
  for (int phase = 0; phase < 3; ++phase)
    for (int sn = 0; sn < NSUB; ++sn)
      for (uint32_t mask = 0; mask < (1u << NRED); ++mask)
        for (int rep = 0; rep < 6; ++rep) {
          s->phase = phase; s->steps = 500; s->n_green = 0;
          for (int r = 0; r < NRED; ++r) {
            RedHdr& h = s->red[r].h;
            h.exec_type = (uint8_t)(((mask >> r) & 1u) ? (int)RA_IMPACT : (int)((rnd() % 11 + RA_IMPACT + 1) % 12));
            // rep 0: every agent names a host of subnet sn; later: the Impact agents spread over the subnets from sn on
            h.exec_host = (uint8_t)h_make(rep == 0 ? sn : (sn + r * rep) % NSUB, (int)(rnd() % SLOTS));
            h.nsess = (uint8_t)(rep == 1 ? 0 : (rep == 2 ? (r & 1) : 1 + rnd() % 5));
          }
          const int brm0 = rep < 3 ? 0 : -(int)(rnd() % 40), n_restore = rep < 4 ? 0 : (int)(rnd() % 4), step0 = (int)(rnd() % 497);
          float want_reward, want_cost; int want_done, want_step;
          {
            s->brm = brm0; s->n_restore = n_restore; s->step_count = step0; s->rng.mode = 1;
            Ctx x{s, nullptr, &s->rng, nullptr, &work};
            step_end(x, nullptr, false);
            want_reward = s->reward; want_cost = s->action_cost; want_done = s->done; want_step = s->step_count;
            CHECK(s->brm == 0 && s->n_restore == 0 && s->n_actions == NBLUE + NRED, "step_end leaves the next step's accumulators");
          }
          {
            s->brm = brm0; s->n_restore = n_restore; s->step_count = step0; s->reward = -12345.0f;
            int sum = 0;
            for (int r = 0; r < NRED; ++r) sum += step_impact_term(s, r);     // (the kernel: an LDS atomic per non-zero term)
            s->brm += sum;
            Ctx x{s, nullptr, &s->rng, nullptr, &work};
            step_end(x, nullptr, false, false);
            CHECK(s->reward == want_reward && s->action_cost == want_cost && s->done == want_done && s->step_count == want_step && s->brm == 0,
                  "phase %d subnet %d mask %02x rep %d: reward %g vs %g", phase, sn, mask, rep, (double)s->reward, (double)want_reward);
          }
        }
  free(s);
  printf("fsm_tail_forms_check: %ld cases, %ld mismatches\n", cases, fails);
  return fails ? 1 : 0;
}
