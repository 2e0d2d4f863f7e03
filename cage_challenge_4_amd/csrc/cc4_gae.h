// cc4_gae.h -- advantages, returns and loss weights of a STORED rollout (generalised advantage estimation; include/cc4.h "Advantages and returns
// of a stored rollout"): one statement for the device kernel (cc4_k_gae.hip: k_gae, one lane per column) and the host function (cc4_gae_host:
// gae_columns, serial).  A pure function of the caller's tensors: no env, no hot row, no handle.
//   T rows, N episodes, A value heads per episode (1 <= A <= 8); column c = n * A + a
//   rewards [T][N] (reward_heads 1: shared by the heads) or [T][N][A] (reward_heads A) float32;  values [T][N][A], last [N][A] (the value of the
//   observation after row T-1);  dones [T][N] bytes;  done0 [N] bytes or NULL (the env's done before the first call; NULL: all zero);  actions
//   [T][N][A] int32 or NULL;  adv, ret [T][N][A] float32;  weight [T][N][A] bytes (0 / 1) or NULL
//
// The layouts.  GAE_SKIP_AFTER_DONE is this env's autoreset layout: the call that follows a `done` takes no step -- it regenerates the episode and
// returns reward 0 and the new scenario's first observation -- so the row it stored is no transition: it gets adv 0, ret = its own value and
// weight 0, and the trace is cut at it.  `done` here is always truncation (episodes end at the horizon only), and the observation returned with it
// is the old episode's last one, which the row that follows (the skip row) stores: with GAE_BOOTSTRAP_DONE (needs GAE_SKIP_AFTER_DONE) the done
// row bootstraps from that row's value instead of from 0.  Without GAE_SKIP_AFTER_DONE the layout is the plain one: a done cuts the trace, every
// row is a transition, done0 is ignored.
//
// Per column, for t = T-1 .. 0, with A_next = 0 and v_next = last before the first iteration (gae_row):
//   prev   = t == 0 ? done0[n] : dones[t-1][n]            (the stored bytes, != 0)
//   skip   = SKIP_AFTER_DONE && prev
//   d      = dones[t][n] != 0
//   vb     = d ? (BOOTSTRAP_DONE ? v_next : 0) : v_next
//   An     = d ? 0 : A_next
//   delta  = (r + gamma * vb) - v                         three rounded float32 operations in this order
//   adv    = skip ? 0 : delta + (gamma * lambda) * An     gamma * lambda rounded once, outside the loop
//   ret    = skip ? v : adv + v
//   weight = !skip && (actions == NULL || actions[t][n][a] != -1)
//   A_next = adv;  v_next = v
// skip reads only the previous row's stored byte (the engine writes 0 into a skip row's own done; a stored 1 there is taken as stored and makes
// the next row a skip row too), so the backward scan needs no forward state.  Non-finite inputs propagate; nothing is refused on the device.
// Plain *, +, - and no fmaf: the library is built with -ffp-contract=off, so the host and the device round alike, bit for bit.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "cc4_rng.h"      // CC4_HD

namespace cc4 {

enum : int { GAE_SKIP_AFTER_DONE = 1, GAE_BOOTSTRAP_DONE = 2, GAE_FLAGS = 3, GAE_MAX_HEADS = 8, GAE_NO_ACTION = -1 };

// the arguments of k_gae: cc4_gae_device's, the dtype code of values and last included
struct GaeArgs {
  const float* rewards; const void* values; const void* last; const uint8_t* dones; const uint8_t* done0; const int32_t* actions;
  float* adv; float* ret; uint8_t* weight;
  int32_t reward_heads, dtype, T, N, A, flags;
  float gamma, lambda;
};
struct GaeCarry { float adv, v; };                 // A_next, v_next
struct GaeOut { float adv, ret; bool weight; };

// one row of one column.  prev, d: the stored done bytes of the row before and of this row; acted: no actions given, or this one is not -1;
// gl = gamma * lambda, rounded once by the caller
CC4_HD GaeOut gae_row(float r, float v, bool prev, bool d, bool acted, float gamma, float gl, int flags, GaeCarry& c) {
  const bool skip = (flags & GAE_SKIP_AFTER_DONE) && prev;
  const float vb = d ? ((flags & GAE_BOOTSTRAP_DONE) ? c.v : 0.0f) : c.v;
  const float an = d ? 0.0f : c.adv;
  const float gv = gamma * vb;
  const float rg = r + gv;
  const float delta = rg - v;
  const float ga = gl * an;
  const float adv = skip ? 0.0f : delta + ga;
  const float ret = skip ? v : adv + v;
  c.adv = adv;
  c.v = v;
  return GaeOut{adv, ret, !skip && acted};
}

// what both entry points refuse (-2), the pointers aside
inline bool gae_bad(int32_t reward_heads, int32_t T, int32_t N, int32_t A, float gamma, float lambda, int32_t flags) {
  if (T < 0 || N < 0 || A < 1 || A > GAE_MAX_HEADS || (reward_heads != 1 && reward_heads != A)) return true;
  if (!(gamma >= 0.0f && gamma <= 1.0f) || !(lambda >= 0.0f && lambda <= 1.0f)) return true;      // (a NaN fails both compares)
  if ((flags & ~(int32_t)GAE_FLAGS) || ((flags & GAE_BOOTSTRAP_DONE) && !(flags & GAE_SKIP_AFTER_DONE))) return true;
  return (int64_t)N * A > INT32_MAX;
}

// The serial statement over every column: float32 values.
inline void gae_columns(const float* rewards, int reward_heads, const float* values, const float* last, const uint8_t* dones, const uint8_t* done0,
                        const int32_t* actions, int T, int N, int A, float gamma, float lambda, int flags, float* adv, float* ret, uint8_t* weight) {
  const size_t NA = (size_t)N * (size_t)A;
  const float gl = gamma * lambda;
  for (size_t col = 0; col < NA; ++col) {
    const size_t n = col / (size_t)A;
    GaeCarry c{0.0f, last[col]};
    for (int t = T - 1; t >= 0; --t) {
      const size_t i = (size_t)t * NA + col, in = (size_t)t * (size_t)N + n;
      const bool prev = t == 0 ? (done0 && done0[n] != 0) : dones[in - (size_t)N] != 0;
      const GaeOut o = gae_row(rewards[reward_heads == 1 ? in : i], values[i], prev, dones[in] != 0, !actions || actions[i] != GAE_NO_ACTION, gamma, gl,
                               flags, c);
      adv[i] = o.adv;
      ret[i] = o.ret;
      if (weight) weight[i] = o.weight ? 1 : 0;
    }
  }
}

}  // namespace cc4
