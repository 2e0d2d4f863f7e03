// Stand-alone check of the host side of the masked action sampling (csrc/cc4_sample.h): sample_from_row -- the serial statement of what
// k_sample_actions computes, float32, built from the header's per-item functions -- against a deliberately different formulation here: the valid
// slots from a slot layout written out by hand, a Philox4x32-10 of its own, and every number in double (tests/test_sample_cpu.py builds this with the
// host compiler and the address / undefined-behaviour sanitizers and runs it as a child process).  The hot row, the logits and the outputs are heap
// blocks of exactly their size, so a read or write past any of them is the sanitizer's finding.  Covered: exists bitmaps that are full, empty, one
// server and one user per subnet, and full but for the first and the last host of each agent's zone; random logits at T 1, 0.5 and 0.25, sampled and
// greedy, with and without the busy rule and busy agents, without logits, without stats; -inf on valid slots, all but one -inf, all -inf, NaN and
// +inf on a valid slot, NaN and 3e38 on invalid slots.
// The tolerance (float32 against double): an action must be the double formulation's where its winning margin is at least
// tau = 2^-12 max(1, max |z|), else one of its top two; logp and entropy within 2^-12 max(1, |value|).
// Exit status 0: every case agreed.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../cage_challenge_4_amd/csrc/cc4_sample.h"
using namespace cc4;

static long fails = 0, cases = 0, close_calls = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "MISMATCH %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static const int SEG[6] = {0, 82, 164, 246, 328, 570};
static const int ZONE_SUBNETS[5][3] = {{0, -1, -1}, {1, -1, -1}, {2, -1, -1}, {3, -1, -1}, {6, 7, 5}};      // in the wrapper's (alphabetical) order
static EnvState* s;
static uint32_t rnd_state = 2024;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static float rnd_logit(float scale) { return ((float)(rnd() & 0xFFFF) / 32768.0f - 1.0f) * scale; }

// position j (0..15) of a subnet in the wrapper's host order: the six server positions, then the ten user positions
static int zone_host(int subnet, int j) { return subnet * 17 + (j < 6 ? 11 + j : 1 + (j - 6)); }
static bool host_exists(int h) { return (s->exists[h >> 5] >> (h & 31)) & 1u; }
static void set_host(int h, bool on) { if (on) s->exists[h >> 5] |= 1u << (h & 31); else s->exists[h >> 5] &= ~(1u << (h & 31)); }
// the mask, from the layout of the action list: Analyse x hosts, Monitor, Remove x hosts, Restore x hosts, Sleep, Allow x 8 per subnet, Block x same,
// DeployDecoy x hosts -- a host slot is valid iff its host exists, the others always
static bool slot_valid(int b, int i) {
  const int nsub = b == 4 ? 3 : 1, nh = 16 * nsub, nc = 8 * nsub;
  int j;
  if (i < nh) j = i;
  else if (i == nh) return true;
  else if (i < 3 * nh + 1) j = (i - nh - 1) % nh;
  else if (i < 3 * nh + 2 + 2 * nc) return true;
  else j = i - (3 * nh + 2 + 2 * nc);
  return host_exists(zone_host(ZONE_SUBNETS[b][j / 16], j % 16));
}
static void philox(uint32_t c[4], uint64_t key) {
  uint64_t k0 = key & 0xFFFFFFFFull, k1 = key >> 32;
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ (uint32_t)k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ (uint32_t)k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 = (k0 + 0x9E3779B9ull) & 0xFFFFFFFFull; k1 = (k1 + 0xBB67AE85ull) & 0xFFFFFFFFull;
  }
}
struct Want { int a, second; double logp, ent, margin, zmax; bool refused; };
static Want in_double(int b, const float* logits, uint64_t seed0, uint32_t t, int e, float T, int flags) {
  Want w = {-1, -1, 0.0, 0.0, INFINITY, 1.0, false};
  if ((flags & 2) && s->blue[b].queue.busy) return w;
  const double r = (double)(1.0f / T);
  const int n = SEG[b + 1] - SEG[b];
  std::vector<int> idx;
  std::vector<double> x;
  for (int i = 0; i < n; ++i) if (slot_valid(b, i)) {
    double v = logits ? (double)logits[SEG[b] + i] * r : 0.0;
    if (fabs(v) > 3.4028234663852886e38) v = v > 0 ? INFINITY : -INFINITY;      // x is a float32 product: it overflows where float32 does
    idx.push_back(i); x.push_back(v);
  }
  double m = -INFINITY;
  for (double v : x) { if (v != v || v == INFINITY) w.refused = true; if (v > m) m = v; }
  if (m == -INFINITY) w.refused = true;
  if (w.refused) return w;
  double S = 0.0, best = -INFINITY, next = -INFINITY;
  for (double v : x) S += exp(v - m);
  for (size_t k = 0; k < x.size(); ++k) {
    const double p = exp(x[k] - m) / S;
    if (p > 0.0) w.ent -= p * log(p);
    if (x[k] == -INFINITY) continue;
    double g = 0.0;
    if (!(flags & 1)) {
      uint32_t c[4] = {t, (uint32_t)b, 0x5A3Bu, (uint32_t)idx[k] / 4u};
      philox(c, seed0 + (uint64_t)e);
      const double u = (2.0 * (double)(c[idx[k] % 4] >> 9) + 1.0) / 16777216.0;
      g = -log(-log(u));
    }
    const double z = x[k] + g;
    if (fabs(z) > w.zmax) w.zmax = fabs(z);
    if (z > best) { next = best; w.second = w.a; best = z; w.a = idx[k]; w.logp = x[k] - m - log(S); }
    else if (z > next) { next = z; w.second = idx[k]; }
  }
  w.margin = best - next;
  return w;
}
// the statement under test into heap blocks of exactly five actions and ten stats, on a heap copy of exactly 570 logits
static void run(const char* what, const float* logits, uint64_t seed0, uint32_t t, int e, float T, int flags, bool with_stats = true, int expect_refused = -1) {
  float* lg = nullptr;
  if (logits) { lg = static_cast<float*>(malloc(sizeof(float) * 570)); if (!lg) exit(2); memcpy(lg, logits, sizeof(float) * 570); }
  int32_t* act = static_cast<int32_t*>(malloc(sizeof(int32_t) * 5));
  float* st = with_stats ? static_cast<float*>(malloc(sizeof(float) * 10)) : nullptr;
  if (!act || (with_stats && !st)) exit(2);
  memset(act, 0x5A, sizeof(int32_t) * 5);
  if (st) memset(st, 0x5A, sizeof(float) * 10);
  const int refused = sample_from_row(s, lg, seed0, t, e, 1.0f / T, flags, act, st);
  int want_refused = 0;
  for (int b = 0; b < 5; ++b) {
    const Want w = in_double(b, logits, seed0, t, e, T, flags);
    want_refused += w.refused ? 1 : 0;
    const double tau = ldexp(w.zmax, -12);
    if (w.margin >= tau) CHECK(act[b] == w.a, "%s agent %d: action %d, want %d (margin %g)", what, b, act[b], w.a, w.margin);
    else { ++close_calls; CHECK(act[b] == w.a || act[b] == w.second, "%s agent %d: action %d, want %d or %d", what, b, act[b], w.a, w.second); }
    if (act[b] >= 0) CHECK(slot_valid(b, act[b]), "%s agent %d: action %d is masked", what, b, act[b]);
    if (st) {
      double lp = w.logp;
      if (act[b] != w.a && act[b] >= 0 && logits) lp += ((double)logits[SEG[b] + act[b]] - (double)logits[SEG[b] + w.a]) * (double)(1.0f / T);
      CHECK(fabs(st[2 * b] - lp) <= ldexp(fmax(1.0, fabs(lp)), -12), "%s agent %d: logp %.9g, want %.9g", what, b, st[2 * b], lp);
      CHECK(fabs(st[2 * b + 1] - w.ent) <= ldexp(fmax(1.0, fabs(w.ent)), -12), "%s agent %d: entropy %.9g, want %.9g", what, b, st[2 * b + 1], w.ent);
    }
  }
  CHECK(refused == want_refused, "%s: %d agents refused, want %d", what, refused, want_refused);
  if (expect_refused >= 0) CHECK(refused == expect_refused, "%s: %d agents refused, the case is built for %d", what, refused, expect_refused);
  free(lg); free(act); free(st);
}

static void topology(int kind) {
  memset(s->exists, 0, sizeof s->exists);
  for (int b = 0; b < 5; ++b)
    for (int k = 0; k < (b == 4 ? 3 : 1); ++k)
      for (int j = 0; j < 16; ++j) set_host(zone_host(ZONE_SUBNETS[b][k], j), kind == 0 || kind == 3 || (kind == 2 && (j == 0 || j == 6)));
  if (kind == 3)
    for (int b = 0; b < 5; ++b) { set_host(zone_host(ZONE_SUBNETS[b][0], 0), false); set_host(zone_host(ZONE_SUBNETS[b][b == 4 ? 2 : 0], 15), false); }
}

int main() {
  s = static_cast<EnvState*>(aligned_alloc(alignof(EnvState), sizeof(EnvState)));
  if (!s) return 2;
  memset(s, 0, sizeof(EnvState));
  static const char* const names[4] = {"full", "empty", "one server and one user", "first and last host missing"};
  std::vector<float> lg(570);
  for (int kind = 0; kind < 4; ++kind) {
    topology(kind);
    for (int b = 0; b < 5; ++b) {                  // the layout written out here is the header's mask
      const int n = SEG[b + 1] - SEG[b];
      int valid = 0;
      for (int i = 0; i < n; ++i) { CHECK(slot_valid(b, i) == (blue_mask_slot(s, b, i) != 0), "%s: mask of agent %d slot %d", names[kind], b, i); valid += slot_valid(b, i); }
      CHECK(valid >= 2 + 16 * (b == 4 ? 3 : 1), "%s: agent %d keeps Monitor, Sleep, Allow and Block", names[kind], b);
    }
    for (int rep = 0; rep < 24; ++rep) {
      const float T = rep % 3 == 0 ? 1.0f : (rep % 3 == 1 ? 0.5f : 0.25f);
      for (int b = 0; b < 5; ++b) s->blue[b].queue.busy = (uint8_t)((rnd() & 3) == 0);
      for (float& v : lg) v = rnd_logit(rep & 1 ? 20.0f : 3.0f);
      const int flags = rep & 3;
      run(names[kind], lg.data(), 1000 + rep, (uint32_t)rep, rep * 7, T, flags);
      run(names[kind], lg.data(), 1000 + rep, 0xFFFFFFFFu, 0x7FFFFFFF, T, flags, false);
      run(names[kind], nullptr, 0xFFFFFFFFFFFFFFFFull, (uint32_t)rep, rep, T, flags);
    }
    for (int b = 0; b < 5; ++b) s->blue[b].queue.busy = 0;
    // crafted: the first valid slot of each agent
    int first[5], last[5];
    for (int b = 0; b < 5; ++b) { first[b] = last[b] = -1; for (int i = 0; i < SEG[b + 1] - SEG[b]; ++i) if (slot_valid(b, i)) { if (first[b] < 0) first[b] = i; last[b] = i; } }
    for (int greedy = 0; greedy < 2; ++greedy) {
      for (float& v : lg) v = rnd_logit(5.0f);
      for (int b = 0; b < 5; ++b) for (int i = 0; i < SEG[b + 1] - SEG[b]; ++i) if (!slot_valid(b, i)) lg[SEG[b] + i] = (i & 1) ? NAN : 3e38f;
      run("NaN and 3e38 on invalid slots", lg.data(), 5, 6, 7, 1.0f, greedy, true, 0);
      std::vector<float> v = lg;
      for (int b = 0; b < 5; ++b) for (int i = 0; i < SEG[b + 1] - SEG[b]; ++i) if (slot_valid(b, i) && i != last[b]) v[SEG[b] + i] = -INFINITY;
      run("all but the last valid slot -inf", v.data(), 5, 6, 7, 0.5f, greedy, true, 0);
      v = lg;
      for (int i = 0; i < 82; ++i) v[SEG[1] + i] = -INFINITY;
      v[SEG[3] + first[3]] = -INFINITY;
      run("agent 1 all -inf, one -inf for agent 3", v.data(), 5, 6, 7, 1.0f, greedy, true, 1);
      v = lg;
      v[SEG[0] + first[0]] = NAN; v[SEG[4] + last[4]] = INFINITY;
      run("NaN for agent 0, +inf for agent 4", v.data(), 5, 6, 7, 1.0f, greedy, true, 2);
      v = lg;
      v[SEG[2] + first[2]] = 3e38f;
      run("a product that overflows for agent 2", v.data(), 5, 6, 7, 0.25f, greedy, true, 1);
    }
  }
  free(s);
  printf("sample_check: %ld checks, %ld close calls, %ld mismatches\n", cases, close_calls, fails);
  return fails ? 1 : 0;
}
