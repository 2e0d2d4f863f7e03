// cc4_sample.h -- masked sampling of the blue actions from policy logits (include/cc4.h "Masked sampling of blue actions"): one statement, for the
// device kernel (cc4_k_sample.hip: k_sample_actions, one wavefront per entry) and the host function (cc4_sample_actions_from_row:
// sample_from_row, serial), of the step from a policy's [570] logits to the [5] action indices step() takes, with the log-probability and the
// entropy of what was drawn.
//   actions [5] int32 per entry, stats [5][2] float (logp, entropy).
// Source: of the hot row the exists bits (through blue_mask_slot, cc4_engine.h: the rule of the action mask) and blue[b].queue.busy (bv_busy).
//
// For agent b (slots i = 0 .. L_b - 1 of its segment of the logits row, L_b = 82 or 242, segment offsets 0, 82, 164, 246, 328):
//   valid_i = blue_mask_slot(s, b, i); the agent's Sleep slot is always valid, so the valid set is never empty
//   x_i     = l_i * r in float32, r = 1.0f / T rounded once (no logits: x_i = 0)
//   noise   Philox4x32-10, key seed0 + e (e: the entry's id -- the episode or bank slot, never its position in ids), counter
//           (t, b, SA_TAG, i >> 2); slot i takes word w = block[i & 3]
//           u = (2 (w >> 9) + 1) 2^-24: an odd multiple of 2^-24 below 1, exact in float32 and strictly inside (0, 1)
//           g = -logf(-logf(u)) with the accurate logf; CC4_SAMPLE_GREEDY: g = 0
//   z_i     = x_i + g_i; the action is the valid slot with the largest z_i, the lowest index among equals (Gumbel-max: a draw from softmax(x over
//           the valid slots)); a valid slot with x_i = -inf has z_i = -inf and is never chosen
//   m       = max of the valid x_i;  S = sum over valid i of expf(x_i - m)
//   logp    = x_a - m - logf(S);  entropy = logf(S) - (sum over valid i with expf(x_i - m) > 0 of expf(x_i - m) (x_i - m)) / S
//   refused a valid x_i that is NaN or +inf, or every valid x_i = -inf: action -1, logp = entropy = 0, and the caller is told (the kernel raises
//           CF_RANGE, the host function returns 1); the other agents of the entry are unaffected
//   busy    with CC4_SAMPLE_BUSY an agent whose queue is busy gets action -1 ("submits nothing": blue_decode resolves it like Sleep) and zero stats
// Logits of invalid slots are never interpreted.  The per-item functions:
//   sa_agent / sa_off / sa_len   the segment of a slot of the row
//   sa_x, sa_refuses             the scaled logit, and whether it refuses its agent
//   sa_block, sa_gumbel, sa_noise  a block of four slots' noise words, g of a word, and g of (seed0, t, e, b, i)
//   sa_better                    the order of the arg-max: larger score, then lower index
//   sa_stats                     logp and entropy from (x_a, m, S, sum e (x - m))
#pragma once
#include <math.h>
#include "cc4_blue_view.h"

namespace cc4 {

enum : int { SA_SLOTS = MASK_TOTAL, SA_STATS = 2, SA_NONE = -1 };
enum : int { SA_GREEDY = 1, SA_BUSY = 2, SA_FLAGS = SA_GREEDY | SA_BUSY };
constexpr uint32_t SA_TAG = 0x5A3Bu;       // third counter word of the noise blocks (random_blue_action: 0xB10E)
static_assert(SA_SLOTS == 4 * ACT_SHORT + ACT_LONG && NBLUE == 5 && SA_TAG != 0xB10Eu, "four short segments and a long one; a counter tag of its own");

CC4_HD constexpr int sa_off(int b) { return b * ACT_SHORT; }
CC4_HD constexpr int sa_len(int b) { return b == NBLUE - 1 ? ACT_LONG : ACT_SHORT; }
CC4_HD int sa_agent(int f) { const int b = f / ACT_SHORT; return b < NBLUE - 1 ? b : NBLUE - 1; }      // 0 <= f < SA_SLOTS

CC4_HD float sa_inf() { return __builtin_inff(); }
CC4_HD float sa_x(float l, float inv_t) { return l * inv_t; }
CC4_HD bool sa_refuses(float x) { return x != x || x == sa_inf(); }
CC4_HD float sa_uniform(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * (1.0f / 16777216.0f); }      // (the integer is below 2^24: the conversion is exact)
// block G of agent b's noise: the words of slots 4 G .. 4 G + 3 (vec: philox4x32_10's form for a lane-private block on the device)
CC4_HD void sa_block(uint64_t seed0, uint32_t t, int e, int b, int G, uint32_t c[4], bool vec = false) {
  c[0] = t; c[1] = (uint32_t)b; c[2] = SA_TAG; c[3] = (uint32_t)G;
  const uint64_t key = seed0 + (uint64_t)e;
  philox4x32_10(c, (uint32_t)key, (uint32_t)(key >> 32), vec);
}
CC4_HD float sa_gumbel(uint32_t w) { return -logf(-logf(sa_uniform(w))); }
CC4_HD float sa_noise(uint64_t seed0, uint32_t t, int e, int b, int i) {
  uint32_t c[4];
  sa_block(seed0, t, e, b, i >> 2, c);
  const int k = i & 3;
  return sa_gumbel(k == 0 ? c[0] : (k == 1 ? c[1] : (k == 2 ? c[2] : c[3])));
}
// (z, i) beats (zb, ib); an agent's search starts from (-inf, INT_MAX), which no finite score loses to
CC4_HD bool sa_better(float z, int i, float zb, int ib) { return z > zb || (z == zb && i < ib); }
CC4_HD void sa_stats(float xa, float m, float S, float sx, float* logp, float* ent) {
  const float ls = logf(S);
  *logp = xa - m - ls;
  *ent = ls - sx / S;
}

// The serial statement: actions [5], stats [5][2] (or null) from one hot row and its 570 logits (null: all zero).  Returns the number of agents
// the logits refused.  inv_t: 1.0f / T for a finite T > 0, flags within SA_FLAGS (the caller checks both).
inline int sample_from_row(const EnvState* s, const float* logits, uint64_t seed0, uint32_t t, int e, float inv_t, int flags, int32_t* actions, float* stats) {
  int refused = 0;
  for (int b = 0; b < NBLUE; ++b) {
    actions[b] = SA_NONE;
    if (stats) stats[b * SA_STATS] = stats[b * SA_STATS + 1] = 0.0f;
    if ((flags & SA_BUSY) && bv_busy(s, b)) continue;
    const float* const l = logits ? logits + sa_off(b) : nullptr;
    const int n = sa_len(b);
    bool bad = false;
    float m = -sa_inf();
    for (int i = 0; i < n; ++i) {
      if (!blue_mask_slot(s, b, i)) continue;
      const float x = l ? sa_x(l[i], inv_t) : 0.0f;
      bad = bad || sa_refuses(x);
      m = x > m ? x : m;
    }
    if (bad || m == -sa_inf()) { ++refused; continue; }
    float S = 0.0f, sx = 0.0f, zb = -sa_inf(), xa = 0.0f;
    int ib = 0x7FFFFFFF;
    for (int i = 0; i < n; ++i) {
      if (!blue_mask_slot(s, b, i)) continue;
      const float x = l ? sa_x(l[i], inv_t) : 0.0f;
      const float d = x - m, ex = expf(d);
      S += ex;
      sx += ex > 0.0f ? ex * d : 0.0f;
      if (x == -sa_inf()) continue;
      const float z = (flags & SA_GREEDY) ? x : x + sa_noise(seed0, t, e, b, i);
      if (sa_better(z, i, zb, ib)) { zb = z; ib = i; xa = x; }
    }
    actions[b] = ib;
    if (stats) sa_stats(xa, m, S, sx, &stats[b * SA_STATS], &stats[b * SA_STATS + 1]);
  }
  return refused;
}

}  // namespace cc4
