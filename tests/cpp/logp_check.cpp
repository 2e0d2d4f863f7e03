// Stand-alone check of the host side of "log-probabilities of stored blue actions" (csrc/cc4_logp.h): logp_from_row and logp_grad_from_row -- the
// serial statements of what k_logp_fwd and k_logp_bwd compute, float32, built from the header's per-item functions -- against a deliberately
// different formulation here: segment bounds written out by hand, every number in double, probabilities formed as exp(x - m) / S and the gradient
// from them, none of the header's helpers (tests/test_logp_cpu.py builds this with the host compiler and the address / undefined-behaviour
// sanitizers and runs it as a child process).  The logits, the mask, the actions, aux, g and the gradient are heap blocks of exactly their size,
// so a read or write past any of them is the sanitizer's finding.  Covered: masks that are full, random, only one slot per agent, and empty for one
// agent; random logits at T 1, 0.5 and 0.25; stored actions that are valid, -1, on an invalid slot, -2, L_b and far outside; -inf on valid slots
// (as the action too), all but one -inf, all -inf, NaN and +inf on a valid slot, a product that overflows, NaN and 3e38 on invalid slots.
// The tolerances (float32 against double): logp, entropy, m, logS within 2^-12 max(1, |value|); a gradient value within
// 2^-12 max(1, 1 / T) max(1, |value|).
// Exit status 0: every case agreed.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../cage_challenge_4_amd/csrc/cc4_logp.h"

static long fails = 0, cases = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "MISMATCH %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static const int SEG[6] = {0, 82, 164, 246, 328, 570};
static uint32_t rnd_state = 2025;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static float rnd_unit() { return (float)(rnd() & 0xFFFF) / 32768.0f - 1.0f; }

struct Want { bool skipped, refused; double logp, ent, m, logS; std::vector<double> grad; };
static Want in_double(int b, const float* logits, const uint8_t* mask, int a, float T, const float* g) {
  const int n = SEG[b + 1] - SEG[b];
  Want w = {a == -1, false, 0.0, 0.0, 0.0, 0.0, std::vector<double>(n, 0.0)};
  if (w.skipped) return w;
  const double r = (double)(1.0f / T);
  std::vector<double> x(n, 0.0);
  int nvalid = 0;
  bool finite_one = false;
  for (int i = 0; i < n; ++i) {
    if (!mask[SEG[b] + i]) continue;
    ++nvalid;
    double v = (double)logits[SEG[b] + i] * r;
    if (fabs(v) > 3.4028234663852886e38) v = v > 0 ? INFINITY : -INFINITY;      // x is a float32 product: it overflows where float32 does
    x[i] = v;
    if (v != v || v == INFINITY) w.refused = true;
    if (v != -INFINITY) finite_one = true;
  }
  if (!nvalid || !finite_one || a < -1 || a >= n || !mask[SEG[b] + (a < 0 || a >= n ? 0 : a)]) w.refused = true;
  if (w.refused) { w.m = NAN; return w; }
  w.m = -INFINITY;
  for (int i = 0; i < n; ++i) if (mask[SEG[b] + i] && x[i] > w.m) w.m = x[i];
  double S = 0.0;
  for (int i = 0; i < n; ++i) if (mask[SEG[b] + i]) S += exp(x[i] - w.m);
  w.logS = log(S);
  w.logp = x[a] - w.m - w.logS;
  for (int i = 0; i < n; ++i) {
    if (!mask[SEG[b] + i]) continue;
    const double p = exp(x[i] - w.m) / S;
    if (p > 0.0) w.ent -= p * log(p);
  }
  for (int i = 0; i < n; ++i) {
    if (!mask[SEG[b] + i]) continue;
    const double p = exp(x[i] - w.m) / S;
    double d = (double)g[2 * b] * ((i == a ? 1.0 : 0.0) - p);
    if (p > 0.0) d -= (double)g[2 * b + 1] * p * (log(p) + w.ent);
    w.grad[i] = r * d;
  }
  return w;
}
static bool near(double v, double ref, double scale = 1.0) {
  if (ref != ref) return v != v;
  if (isinf(ref)) return v == ref;
  return fabs(v - ref) <= ldexp(scale * fmax(1.0, fabs(ref)), -12);
}
// the statements under test on heap blocks of exactly their size
static void run(const char* what, const float* logits, const uint8_t* mask, const int* actions, float T, int expect_refused = -1) {
  float* lg = static_cast<float*>(malloc(sizeof(float) * 570));
  uint8_t* mk = static_cast<uint8_t*>(malloc(570));
  int32_t* ac = static_cast<int32_t*>(malloc(sizeof(int32_t) * 5));
  float* aux = static_cast<float*>(malloc(sizeof(float) * 20));
  float* g = static_cast<float*>(malloc(sizeof(float) * 10));
  float* grad = static_cast<float*>(malloc(sizeof(float) * 570));
  if (!lg || !mk || !ac || !aux || !g || !grad) exit(2);
  memcpy(lg, logits, sizeof(float) * 570);
  memcpy(mk, mask, 570);
  for (int b = 0; b < 5; ++b) ac[b] = actions[b];
  for (int k = 0; k < 10; ++k) g[k] = rnd_unit();
  memset(aux, 0x5A, sizeof(float) * 20);
  memset(grad, 0x5A, sizeof(float) * 570);
  const int refused = cc4::logp_from_row(lg, mk, ac, 1.0f / T, aux);
  cc4::logp_grad_from_row(lg, mk, ac, 1.0f / T, aux, g, grad);
  int want_refused = 0;
  const double gs = fmax(1.0, (double)(1.0f / T));
  for (int b = 0; b < 5; ++b) {
    const Want w = in_double(b, logits, mask, actions[b], T, g);
    want_refused += w.refused ? 1 : 0;
    const float* o = aux + 4 * b;
    CHECK(near(o[0], w.logp), "%s agent %d: logp %.9g, want %.9g", what, b, o[0], w.logp);
    CHECK(near(o[1], w.ent), "%s agent %d: entropy %.9g, want %.9g", what, b, o[1], w.ent);
    CHECK(near(o[2], w.m), "%s agent %d: m %.9g, want %.9g", what, b, o[2], w.m);
    CHECK(near(o[3], w.logS), "%s agent %d: logS %.9g, want %.9g", what, b, o[3], w.logS);
    if (w.skipped || w.refused) CHECK(o[0] == 0.0f && o[1] == 0.0f && o[3] == 0.0f, "%s agent %d: the empty aux", what, b);
    for (int i = 0; i < SEG[b + 1] - SEG[b]; ++i) {
      const float v = grad[SEG[b] + i];
      CHECK(near(v, w.grad[i], gs), "%s agent %d slot %d: gradient %.9g, want %.9g", what, b, i, v, w.grad[i]);
      if (w.skipped || w.refused || !mask[SEG[b] + i]) CHECK(v == 0.0f, "%s agent %d slot %d: gradient %.9g, want exactly 0", what, b, i, v);
    }
  }
  CHECK(refused == want_refused, "%s: %d agents refused, want %d", what, refused, want_refused);
  if (expect_refused >= 0) CHECK(refused == expect_refused, "%s: %d agents refused, the case is built for %d", what, refused, expect_refused);
  free(lg); free(mk); free(ac); free(aux); free(g); free(grad);
}

int main() {
  std::vector<float> lg(570);
  std::vector<uint8_t> mask(570);
  static const char* const names[4] = {"full", "random", "one slot per agent", "agent 2 empty"};
  for (int kind = 0; kind < 4; ++kind) {
    int first[5], last[5], off[5];       // off: an invalid slot, or -1
    for (int rep = 0; rep < 24; ++rep) {
      for (int f = 0; f < 570; ++f) mask[f] = kind == 0 ? 1 : (kind == 2 ? 0 : (uint8_t)((rnd() & 3) != 0) * (uint8_t)(1 + (rnd() & 1) * 254));
      if (kind == 2) for (int b = 0; b < 5; ++b) mask[SEG[b] + (int)(rnd() % (uint32_t)(SEG[b + 1] - SEG[b]))] = 1;
      if (kind == 3) for (int i = 0; i < 82; ++i) mask[SEG[2] + i] = 0;
      for (int b = 0; b < 5; ++b) {
        first[b] = last[b] = off[b] = -1;
        for (int i = 0; i < SEG[b + 1] - SEG[b]; ++i) {
          if (mask[SEG[b] + i]) { if (first[b] < 0) first[b] = i; last[b] = i; } else off[b] = i;
        }
      }
      const float T = rep % 3 == 0 ? 1.0f : (rep % 3 == 1 ? 0.5f : 0.25f);
      for (float& v : lg) v = rnd_unit() * (rep & 1 ? 20.0f : 3.0f);
      int act[5];
      for (int b = 0; b < 5; ++b) {                       // a valid slot, chosen at random
        const int n = SEG[b + 1] - SEG[b];
        int a = (int)(rnd() % (uint32_t)n);
        while (first[b] >= 0 && !mask[SEG[b] + a]) a = (a + 1) % n;
        act[b] = first[b] >= 0 ? a : 0;
      }
      const int empty = kind == 3 ? 1 : 0;
      run(names[kind], lg.data(), mask.data(), act, T, empty);
      int edge[5];
      for (int b = 0; b < 5; ++b) edge[b] = rep & 1 ? first[b] : last[b];
      if (kind == 3) edge[2] = 0;
      run(names[kind], lg.data(), mask.data(), edge, T, empty);
      if (rep >= 6) continue;
      // the stored actions that are not slots: -1 skips, the others refuse
      int v[5];
      for (int b = 0; b < 5; ++b) v[b] = b == rep % 5 ? -1 : act[b];
      run("an agent skipped", lg.data(), mask.data(), v, T, rep % 5 == 2 ? 0 : empty);
      for (int b = 0; b < 5; ++b) v[b] = -1;
      run("all skipped", lg.data(), mask.data(), v, T, 0);
      const int outside[4] = {-2, SEG[rep % 5 + 1] - SEG[rep % 5], 0x7FFFFFFF, (int)0x80000000};
      for (int k = 0; k < 4; ++k) {
        for (int b = 0; b < 5; ++b) v[b] = b == rep % 5 ? outside[k] : act[b];
        run("an action outside the segment", lg.data(), mask.data(), v, T, kind == 3 && rep % 5 == 2 ? 1 : empty + 1);
      }
      if (off[rep % 5] >= 0 && !(kind == 3 && rep % 5 == 2)) {
        for (int b = 0; b < 5; ++b) v[b] = b == rep % 5 ? off[b] : act[b];
        run("an action on an invalid slot", lg.data(), mask.data(), v, T, empty + 1);
      }
      // crafted logits
      std::vector<float> c = lg;
      for (int f = 0; f < 570; ++f) if (!mask[f]) c[f] = (f & 1) ? NAN : 3e38f;
      run("NaN and 3e38 on invalid slots", c.data(), mask.data(), act, T == 0.25f ? 0.5f : T, empty);
      c = lg;
      for (int b = 0; b < 5; ++b) for (int i = 0; i < SEG[b + 1] - SEG[b]; ++i) if (mask[SEG[b] + i] && i != act[b]) c[SEG[b] + i] = -INFINITY;
      run("all but the action's slot -inf", c.data(), mask.data(), act, T, empty);
      if (kind != 2) {
        c = lg;
        for (int b = 0; b < 5; ++b) if (first[b] >= 0 && first[b] != last[b]) c[SEG[b] + first[b]] = -INFINITY;
        run("one valid slot -inf", c.data(), mask.data(), edge[0] == first[0] ? act : edge, T, empty);
        for (int b = 0; b < 5; ++b) v[b] = first[b] >= 0 ? first[b] : 0;
        run("the action on a valid -inf slot", c.data(), mask.data(), v, T, empty);
      }
      c = lg;
      for (int i = 0; i < 82; ++i) c[SEG[1] + i] = -INFINITY;
      run("agent 1 all -inf", c.data(), mask.data(), act, T, empty + 1);
      c = lg;
      c[SEG[0] + last[0]] = NAN; c[SEG[4] + first[4]] = INFINITY;
      run("NaN for agent 0, +inf for agent 4", c.data(), mask.data(), act, T, empty + 2);
      c = lg;
      c[SEG[3] + first[3]] = 3e38f;
      run("a product that overflows for agent 3", c.data(), mask.data(), act, 0.25f, empty + 1);
    }
  }
  printf("logp_check: %ld checks, %ld mismatches\n", cases, fails);
  return fails ? 1 : 0;
}
