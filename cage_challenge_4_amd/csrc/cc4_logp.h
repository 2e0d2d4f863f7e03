// cc4_logp.h -- log-probability and entropy of STORED blue actions under new logits, and their derivative (include/cc4.h "Log-probabilities of
// stored blue actions"): the definition of cc4_sample.h with the draw left out, one statement for the device kernels (cc4_k_logp.hip: k_logp_fwd,
// k_logp_bwd, one wavefront per row) and the host functions (cc4_logp_actions_host, cc4_logp_actions_grad_host: logp_from_row, logp_grad_from_row,
// serial).  A pure function of tensors: the mask is the stored action-mask row, -1 among the stored actions is the busy rule; no env, no hot row.
//   aux [5][4] float per row: (logp, entropy, m, logS) -- the last two are what the derivative needs, so that it is elementwise
//   g   [5][2] float per row: (d loss / d logp, d loss / d entropy);  grad [570]: d loss / d logits
//
// For agent b (slots i = 0 .. L_b - 1 of its segment: sa_off, sa_len) with the stored action a:
//   valid_i = mask[off_b + i] != 0;  x_i = l_i * r in float32 (sa_x);  m = max of the valid x_i;  S = sum over valid i of expf(x_i - m)
//   logS = logf(S);  logp = x_a - m - logS;  H = logS - (sum over valid i with expf(x_i - m) > 0 of expf(x_i - m) (x_i - m)) / S      (sa_stats)
//   skipped  a == -1: aux (0, 0, 0, 0), gradient 0 on the whole segment
//   refused  a valid x_i that is NaN or +inf (sa_refuses), every valid x_i = -inf, no valid slot, a < -1 or a >= L_b, or slot a invalid:
//            aux (0, 0, NaN, 0), gradient 0 on the whole segment; the caller is told (the kernel ORs LP_REFUSED into its fault word, the host
//            function counts the agent).  The other agents of the row are unaffected
//   grad     lp_i = x_i - m - logS, p_i = expf(lp_i):  grad_i = r (g0 ([i == a] - p_i) - g1 p_i (lp_i + H)) for valid i, the g1 term 0 where
//            p_i == 0 (a valid -inf slot: 0 log 0 = 0);  0 for invalid slots
// Logits of invalid slots are never interpreted.  The per-item functions:
//   lp_aux                 the four words from (x_a, m, S, sum e (x - m))
//   lp_skipped, lp_refused what the derivative reads off (a, aux): the whole segment is zero
//   lp_grad                one slot of the gradient
#pragma once
#include "cc4_sample.h"

namespace cc4 {

enum : int { LP_AUX = 4, LP_G = 2, LP_REFUSED = 1 };
enum : int { LP_LOGP = 0, LP_ENT = 1, LP_M = 2, LP_LOGS = 3 };

CC4_HD float lp_nan() { return __builtin_nanf(""); }
CC4_HD void lp_aux(float xa, float m, float S, float sx, float* aux) {
  sa_stats(xa, m, S, sx, &aux[LP_LOGP], &aux[LP_ENT]);
  aux[LP_M] = m;
  aux[LP_LOGS] = logf(S);
}
CC4_HD void lp_aux_empty(bool refused, float* aux) {
  aux[LP_LOGP] = aux[LP_ENT] = aux[LP_LOGS] = 0.0f;
  aux[LP_M] = refused ? lp_nan() : 0.0f;
}
CC4_HD bool lp_skipped(int a) { return a == SA_NONE; }
CC4_HD bool lp_refused(float m) { return m != m; }      // (the m of an agent that was evaluated is a valid x that does not refuse: never NaN)
// slot i of an evaluated agent (neither skipped nor refused), valid, with scaled logit x; is_a: i == a
CC4_HD float lp_grad(float x, bool is_a, float m, float logS, float H, float g0, float g1, float inv_t) {
  const float lp = x - m - logS, p = expf(lp);
  const float t0 = g0 * ((is_a ? 1.0f : 0.0f) - p);
  const float t1 = p > 0.0f ? g1 * p * (lp + H) : 0.0f;
  return inv_t * (t0 - t1);
}

// The serial statements.  aux [5][4] from one mask row, its 570 logits and the 5 stored actions; returns the number of refused agents.
// inv_t: 1.0f / T for a finite T > 0 (the caller checks it).
inline int logp_from_row(const float* logits, const uint8_t* mask, const int32_t* actions, float inv_t, float* aux) {
  int refused = 0;
  for (int b = 0; b < NBLUE; ++b) {
    float* const o = aux + b * LP_AUX;
    const int a = actions[b], n = sa_len(b);
    const float* const l = logits + sa_off(b);
    const uint8_t* const v = mask + sa_off(b);
    if (lp_skipped(a)) { lp_aux_empty(false, o); continue; }
    bool bad = a < 0 || a >= n || !v[a];
    float m = -sa_inf();
    for (int i = 0; i < n; ++i) {
      if (!v[i]) continue;
      const float x = sa_x(l[i], inv_t);
      bad = bad || sa_refuses(x);
      m = x > m ? x : m;
    }
    if (bad || m == -sa_inf()) { ++refused; lp_aux_empty(true, o); continue; }
    float S = 0.0f, sx = 0.0f;
    for (int i = 0; i < n; ++i) {
      if (!v[i]) continue;
      const float d = sa_x(l[i], inv_t) - m, ex = expf(d);
      S += ex;
      sx += ex > 0.0f ? ex * d : 0.0f;
    }
    lp_aux(sa_x(l[a], inv_t), m, S, sx, o);
  }
  return refused;
}
// grad [570] from the same inputs, the aux the forward left and g [5][2]
inline void logp_grad_from_row(const float* logits, const uint8_t* mask, const int32_t* actions, float inv_t, const float* aux, const float* g, float* grad) {
  for (int b = 0; b < NBLUE; ++b) {
    const float* const w = aux + b * LP_AUX;
    const int a = actions[b];
    const bool zero = lp_skipped(a) || lp_refused(w[LP_M]);
    for (int i = 0; i < sa_len(b); ++i) {
      const int f = sa_off(b) + i;
      grad[f] = zero || !mask[f] ? 0.0f : lp_grad(sa_x(logits[f], inv_t), i == a, w[LP_M], w[LP_LOGS], w[LP_ENT], g[b * LP_G], g[b * LP_G + 1], inv_t);
    }
  }
}

}  // namespace cc4
