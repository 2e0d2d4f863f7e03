// cc4_row_wave.h -- one wavefront over one 570-slot row of logits: what k_sample_actions (cc4_k_sample.hip) and k_logp_fwd / k_logp_bwd
// (cc4_k_logp.hip) share, stated once so that the two softmax kernels round alike by construction.  Device code only, everything forced inline
// (no device function is called across units); the definitions of the numbers are cc4_sample.h's.  Lane l owns slots l + 64 j (j < ROW_ROUNDS):
// every load instruction reads 64 consecutive values, so nothing beyond the element's alignment is assumed of a row.  The per-agent functions
// take hooks that ride in their loops (the sampler's arg-max, logp's look for the stored action's slot) and touch neither m nor S nor sx.
// Not here: the sampler's noise passes, and anything of the serial host statements (cc4_sample.h, cc4_logp.h).
#pragma once
#include <hip/hip_runtime.h>
#include "cc4_args.h"
#include "cc4_sample.h"

constexpr int ROW_ROUNDS = (SA_SLOTS + WAVE - 1) / WAVE;      // slots per lane
static_assert(ROW_ROUNDS == 9, "the lanes of a row");
// no slot of agent b among the 64 of round j: a constant where j and b count unrolled loops, so the code of the other rounds does not exist
__host__ __device__ constexpr bool round_misses(int j, int b) { return WAVE * j + WAVE - 1 < sa_off(b) || WAVE * j >= sa_off(b) + sa_len(b); }

// this lane's slots; bit j of vmask: slot j is valid (x[j] of any other slot is 0)
struct RowSlots {
  float x[ROW_ROUNDS];
  int ag[ROW_ROUNDS];
  uint32_t vmask;
  __device__ __forceinline__ bool has(int j, int b) const { return ag[j] == b && ((vmask >> j) & 1u); }      // a valid slot of agent b
};
struct RowNoHook { template <class... A> __device__ __forceinline__ void operator()(A...) const {} };

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) { const float o = __shfl_xor(v, d); v = o > v ? o : v; }
  return v;
}

// slot(b, f, &x): whether slot f of the row (of agent b) is valid, and if so its scaled logit
template <class Slot> __device__ __forceinline__ void row_load(RowSlots& r, int lane, Slot&& slot) {
  r.vmask = 0;
#pragma unroll
  for (int j = 0; j < ROW_ROUNDS; ++j) {
    const int f = lane + WAVE * j;
    r.x[j] = 0.0f; r.ag[j] = 0;
    if (f < SA_SLOTS) {
      r.ag[j] = sa_agent(f);
      if (slot(r.ag[j], f, &r.x[j])) r.vmask |= 1u << j;
    }
  }
}

// the maximum of agent b's valid x over the wave; false: refused (a valid x refuses, or none is above -inf).  each(j): once per valid slot of the agent in this lane
template <class Each> __device__ __forceinline__ bool row_agent_max(const RowSlots& r, const int b, float* m_out, Each&& each) {
  bool bad = false;
  float m = -sa_inf();
#pragma unroll
  for (int j = 0; j < ROW_ROUNDS; ++j) {
    if (round_misses(j, b)) continue;
    if (r.has(j, b)) { bad = bad || sa_refuses(r.x[j]); m = r.x[j] > m ? r.x[j] : m; each(j); }
  }
  *m_out = m = wave_max(m);
  return !(__ballot(bad) != 0ull || m == -sa_inf());
}

// S = sum of expf(x - m) and sx = sum of e (x - m): over j ascending in the lane, then the butterfly d = 1, 2 .. 32.  each(j): once per valid slot
// of the agent in this lane, behind its terms; merge(d): once per butterfly step, behind the sums'
template <class Each, class Merge>
__device__ __forceinline__ void row_agent_sums(const RowSlots& r, const int b, const float m, float* S_out, float* sx_out, Each&& each, Merge&& merge) {
  float S = 0.0f, sx = 0.0f;
#pragma unroll
  for (int j = 0; j < ROW_ROUNDS; ++j) {
    if (round_misses(j, b)) continue;
    if (!r.has(j, b)) continue;
    const float d = r.x[j] - m, ex = expf(d);
    S += ex;
    sx += ex > 0.0f ? ex * d : 0.0f;
    each(j);
  }
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    S += __shfl_xor(S, d);
    sx += __shfl_xor(sx, d);
    merge(d);
  }
  *S_out = S; *sx_out = sx;
}
