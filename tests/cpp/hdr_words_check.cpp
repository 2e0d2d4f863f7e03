// Stand-alone check of the word view of RedHdr and Act in csrc/cc4_state.h (hget / hset / hinc, aget / aset, act_word / act_pack / act_unpack /
// act_tick, hdr_tick_reset, hdr_obs_word, hdr_load / hdr_store, act_load / act_store) against plain member loads and stores of the structs
// (tests/test_hdr_words_cpu.py builds this with the host compiler and the address / undefined-behaviour sanitizers and runs it as a child
// process).  Exit status 0: every case agreed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../cage_challenge_4_amd/csrc/cc4_state.h"
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

static RedHdr random_hdr() {
  RedHdr h;
  uint64_t v[4] = {rnd(), rnd(), rnd(), rnd()};
  memcpy(&h, v, sizeof h);
  return h;
}
static bool same(const RedHdr& a, const RedHdr& b) { return memcmp(&a, &b, sizeof(RedHdr)) == 0; }
static bool same(const Act& a, const Act& b) { return memcmp(&a, &b, sizeof(Act)) == 0; }

// the values a field is set to: 0, 1, its maximum, both sides of every byte boundary inside it, and the same plus bits above the field (a set
// keeps the member's truncation)
static int values_for(int width, uint32_t* out) {
  int n = 0;
  out[n++] = 0; out[n++] = 1; out[n++] = (width >= 32 ? 0xFFFFFFFFu : (1u << width) - 1u);
  for (int b = 8; b < width; b += 8) { out[n++] = (1u << b) - 1u; out[n++] = 1u << b; }
  out[n++] = (1u << width) | 1u; out[n++] = 0xFFFFFF00u; out[n++] = (uint32_t)rnd();
  return n;
}

// one field of the header: get == member load; set / inc through the view == member store, every other byte untouched
#define HDR_FIELD(F, member, T)                                                                                             \
  do {                                                                                                                      \
    RedHdr m = h0;                                                                                                          \
    RedHdrW W = hdr_load(&h0);                                                                                              \
    CHECK(hget<F>(W) == (uint32_t)m.member, #member " get %u vs %u", hget<F>(W), (unsigned)m.member);                      \
    uint32_t vals[16];                                                                                                      \
    const int nv = values_for(8 * (int)sizeof(T), vals);                                                                    \
    for (int i = 0; i < nv; ++i) {                                                                                          \
      m = h0; W = hdr_load(&h0);                                                                                            \
      m.member = (T)vals[i]; hset<F>(W, vals[i]);                                                                           \
      RedHdr back = random_hdr(); hdr_store(&back, W);                                                                      \
      CHECK(same(back, m), #member " set %08x", vals[i]);                                                                   \
      CHECK(hget<F>(W) == (uint32_t)m.member, #member " get after set %08x", vals[i]);                                      \
      m.member++; hinc<F>(W);                                                                                               \
      hdr_store(&back, W);                                                                                                  \
      CHECK(same(back, m), #member " inc from %08x", vals[i]);                                                              \
    }                                                                                                                       \
  } while (0)

#define ACT_FIELD(F, member, T)                                                                                             \
  do {                                                                                                                      \
    const ActW w0 = act_load(&a0);                                                                                          \
    CHECK(aget<F>(w0) == (uint32_t)a0.member, #member " get %u vs %u", aget<F>(w0), (unsigned)a0.member);                  \
    uint32_t vals[16];                                                                                                      \
    const int nv = values_for(8 * (int)sizeof(T), vals);                                                                    \
    for (int i = 0; i < nv; ++i) {                                                                                          \
      Act m = a0; m.member = (T)vals[i];                                                                                    \
      const ActW w = aset<F>(w0, vals[i]);                                                                                  \
      Act back; memset(&back, 0xA5, sizeof back); act_store(&back, w);                                                      \
      CHECK(same(back, m), "Act." #member " set %08x", vals[i]);                                                            \
      CHECK(aget<F>(w) == (uint32_t)m.member, "Act." #member " get after set %08x", vals[i]);                               \
    }                                                                                                                       \
  } while (0)

int main() {
  for (int rep = 0; rep < 20000; ++rep) {
    const RedHdr h0 = random_hdr();
    // load / store round trip, whole and by halves
    {
      const RedHdrW W = hdr_load(&h0);
      RedHdr back = random_hdr(); const RedHdr other = back;
      hdr_store(&back, W);
      CHECK(same(back, h0), "round trip rep %d", rep);
      back = other; hdr_store(&back, W, HDR_LO);
      CHECK(memcmp(&back, &h0, 16) == 0 && memcmp((char*)&back + 16, (const char*)&other + 16, 16) == 0, "low half rep %d", rep);
      back = other; hdr_store(&back, W, HDR_HI);
      CHECK(memcmp(&back, &other, 16) == 0 && memcmp((char*)&back + 16, (const char*)&h0 + 16, 16) == 0, "high half rep %d", rep);
    }
    HDR_FIELD(RH_Q_TYPE, queue.type, uint8_t);     HDR_FIELD(RH_Q_HOST, queue.host, uint8_t);       HDR_FIELD(RH_Q_ARG, queue.arg, uint8_t);
    HDR_FIELD(RH_Q_TICKS, queue.ticks, uint8_t);   HDR_FIELD(RH_Q_SID, queue.sid, uint16_t);        HDR_FIELD(RH_Q_BUSY, queue.busy, uint16_t);
    HDR_FIELD(RH_AS_SUBNET, as_subnet, uint16_t);  HDR_FIELD(RH_FSM_STEP, fsm_step, uint16_t);      HDR_FIELD(RH_NEW_SESS_ID, new_sess_id, uint16_t);
    HDR_FIELD(RH_NSESS, nsess, uint8_t);           HDR_FIELD(RH_NKNOWN, nknown, uint8_t);           HDR_FIELD(RH_FSM_N, fsm_n, uint8_t);
    HDR_FIELD(RH_NOBS, nobs, uint8_t);             HDR_FIELD(RH_NLIVE, nlive, uint8_t);             HDR_FIELD(RH_ACTIVE, active, uint8_t);
    HDR_FIELD(RH_OBS_SUCCESS, obs_success, uint8_t);     HDR_FIELD(RH_OBS_ACT_TYPE, obs_act_type, uint8_t);
    HDR_FIELD(RH_OBS_ACT_HOST, obs_act_host, uint8_t);   HDR_FIELD(RH_OBS_ACT_ARG, obs_act_arg, uint8_t);
    HDR_FIELD(RH_EXEC_TYPE, exec_type, uint8_t);   HDR_FIELD(RH_EXEC_HOST, exec_host, uint8_t);     HDR_FIELD(RH_NEW_SESS_HOST, new_sess_host, uint8_t);
    HDR_FIELD(RH_START_HOST, start_host, uint8_t); HDR_FIELD(RH_RSC_DIRTY, rsc_dirty, uint8_t);     HDR_FIELD(RH_RSC_LISTED, rsc_listed, uint8_t);
    HDR_FIELD(RH_FSM_DIRTY, fsm_dirty, uint8_t);

    Act a0; { const uint64_t v = rnd(); memcpy(&a0, &v, 8); }
    ACT_FIELD(AW_TYPE, type, uint8_t);  ACT_FIELD(AW_HOST, host, uint8_t);  ACT_FIELD(AW_ARG, arg, uint8_t);
    ACT_FIELD(AW_TICKS, ticks, uint8_t); ACT_FIELD(AW_SID, sid, uint16_t);  ACT_FIELD(AW_BUSY, busy, uint16_t);
    // pack / unpack / the word from its fields
    {
      const ActW w = act_load(&a0);
      CHECK(act_pack(a0) == w, "act_pack rep %d", rep);
      CHECK(same(act_unpack(w), a0), "act_unpack rep %d", rep);
      CHECK(act_word(a0.type, a0.host, a0.arg, a0.ticks, a0.sid, a0.busy) == w, "act_word rep %d", rep);
      CHECK(act_word(a0.type | 0x100u, a0.host | 0xF00u, a0.arg | 0x100u, a0.ticks | 0x100u, a0.sid | 0x10000u, a0.busy | 0x10000u) == w, "act_word truncates rep %d", rep);
    }
    // the header's queue as an action word
    {
      RedHdrW W = hdr_load(&h0);
      CHECK(hdr_queue(W) == act_load(&h0.queue), "hdr_queue rep %d", rep);
      RedHdr m = h0; m.queue = a0;
      hdr_set_queue(W, act_load(&a0));
      RedHdr back; hdr_store(&back, W);
      CHECK(same(back, m), "hdr_set_queue rep %d", rep);
    }
    // ticks-- on the word: ticks 1 and 2 (what a queue holds), 0 and 255 (the member wraps inside its byte), and random
    for (int k = 0; k < 5; ++k) {
      Act m = a0;
      if (k < 4) m.ticks = (uint8_t)(k == 0 ? 1 : (k == 1 ? 2 : (k == 2 ? 0 : 255)));
      const ActW w = act_tick(act_load(&m));
      m.ticks--;
      Act back; act_store(&back, w);
      CHECK(same(back, m), "act_tick k %d rep %d", k, rep);
      CHECK((aget<AW_TICKS>(w) < 1) == (m.ticks < 1), "act_tick's expiry k %d rep %d", k, rep);
    }
    // the tick's masks against the field-by-field resets
    {
      RedHdr m = h0;
      m.nobs = 0; m.obs_success = 0; m.obs_act_type = RA_NONE; m.new_sess_host = 0xFF; m.rsc_listed = 0;
      RedHdrW W = hdr_load(&h0);
      hdr_tick_reset(W);
      RedHdr back; hdr_store(&back, W);
      CHECK(same(back, m), "tick reset rep %d", rep);
      // ... and the in-progress case on top: obs_first(IN_PROGRESS) as constants
      m.obs_success = T_IN_PROGRESS; m.obs_act_type = RA_NONE; m.obs_act_host = 0; m.obs_act_arg = 0;
      W.w[hdr_field(RH_OBS_SUCCESS).word] = hdr_obs_word(T_IN_PROGRESS, RA_NONE, 0, 0);
      hdr_store(&back, W);
      CHECK(same(back, m), "tick in progress rep %d", rep);
    }
    // obs_first as a word: one test, one word store -- with obs_success already set and not set
    for (int set = 0; set < 2; ++set) {
      RedHdr m = h0;
      m.obs_success = (uint8_t)(set ? 1 + rnd() % 4 : 0);
      const RedHdr start = m;
      const uint8_t succ = (uint8_t)(1 + rnd() % 4), ty = (uint8_t)(rnd() % 12), host = (uint8_t)rnd(), arg = (uint8_t)rnd();
      if (m.obs_success == 0) { m.obs_success = succ; m.obs_act_type = ty; m.obs_act_host = host; m.obs_act_arg = arg; }
      RedHdrW W = hdr_load(&start);
      if (hget<RH_OBS_SUCCESS>(W) == 0) W.w[hdr_field(RH_OBS_SUCCESS).word] = hdr_obs_word(succ, ty, host, arg);
      RedHdr back; hdr_store(&back, W);
      CHECK(same(back, m), "obs_first set %d rep %d", set, rep);
    }
  }
  printf("hdr_words_check: %ld cases, %ld mismatches\n", cases, fails);
  return fails ? 1 : 0;
}
