// cc4_k_logp.hip -- log-probability and entropy of stored blue actions under new logits, and their derivative: the learner's half of the masked
// sampling (the definition: cc4_logp.h, shared with the host functions).  Pure functions of the caller's tensors on the caller's stream: no handle,
// no hot row, no LDS.  One wavefront per row, LP_WAVES rows per workgroup (cc4_kernel_decls.h); a wave never meets another, so there is no barrier
// and a workgroup's last waves may leave at once.
//   k_logp_fwd  cc4_logp_actions_device.
//                 1. lane l owns slots l + 64 j (j < 9) of the 570-slot row (the layout, the load and the reductions of step 2: cc4_row_wave.h,
//                    shared with k_sample_actions); validity is the mask byte; the scaled logits stay in registers;
//                 2. the five stored actions are wave-uniform (scalar loads); per agent that is not skipped: the maximum of the valid x by a
//                    butterfly of shuffles, "some valid x refuses" and "the action's slot is a valid slot of this segment" as ballots, x_a read
//                    from the lane that owns it, then in one more butterfly the sum of exponentials and the sum of e (x - m) -- the one
//                    row_agent_sums k_sample_actions runs, so the two kernels round alike;
//                 3. lanes 0..19 store one of the row's twenty aux words each; a refused agent ORs LP_REFUSED into the fault word.
//   k_logp_bwd  cc4_logp_actions_grad_device: the same lane layout, elementwise.  The row's 5 actions, 20 aux words and 10 g words are wave-uniform
//               (scalar loads, no reduction anywhere); a lane picks its agent's by compares against the segment offsets -- which of the five a
//               round of 64 slots can hold at all is known to the compiler -- and stores the whole row in the logits' dtype, zeros on invalid
//               slots and on skipped or refused agents included, so the caller's buffer needs no initialisation.
#include <hip/hip_runtime.h>
#include "cc4_logp.h"
#include "cc4_elem.h"
#include "cc4_row_wave.h"
#include "cc4_kernel_decls.h"

static_assert(LP_REFUSED == CC4_LOGP_REFUSED && SA_SLOTS == CC4_MASK_PER_ENV && NBLUE == CC4_NUM_BLUE, "include/cc4.h states the bit and the shapes");
static_assert(NBLUE * LP_AUX <= WAVE, "the lanes of step 3");

// the row of this wavefront, wave-uniform to the compiler too; -1: none
__device__ __forceinline__ int lp_row(int n) {
  const int r = (int)blockIdx.x * LP_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);
  return r < n ? r : -1;
}

template <int DT>
__device__ __forceinline__ void logp_fwd_row(const void* __restrict__ logits, const uint8_t* __restrict__ mask, const int32_t* __restrict__ actions, int row,
                                             int lane, float inv_t, float* __restrict__ aux, int32_t* __restrict__ fault) {
  using E = typename Elem<DT>::type;
  const E* const lrow = static_cast<const E*>(logits) + (size_t)row * SA_SLOTS;
  const uint8_t* const mrow = mask + (size_t)row * SA_SLOTS;
  const int32_t* const arow = actions + (size_t)row * NBLUE;

  // 1. this lane's slots: agent, validity, scaled logit (the logit is loaded beside the mask byte, not behind it)
  RowSlots r;
  row_load(r, lane, [&](int, int f, float* x) {
    const E raw = lrow[f];
    if (mrow[f] == 0) return false;
    *x = sa_x(elem_to_float<DT>(raw), inv_t);
    return true;
  });

  // 2. per agent
  float st = 0.0f;             // lanes 0 .. 19: aux word `lane`
  bool refused = false;
#pragma unroll
  for (int b = 0; b < NBLUE; ++b) {
    const int a = arow[b];                                         // (wave-uniform)
    float w[LP_AUX];
    lp_aux_empty(false, w);
    if (!lp_skipped(a)) {
      const int fa = sa_off(b) + a;                                // the action's slot of the row, if it is one of the segment's
      const bool in_seg = a >= 0 && a < sa_len(b);
      bool hit = false;
      float m, S, sx, xa = 0.0f;
      const bool ok = row_agent_max(r, b, &m, [&](int j) {
        if (in_seg && lane + WAVE * j == fa) { hit = true; xa = r.x[j]; }
      });
      if (!ok || __ballot(hit) == 0ull) {
        refused = true;
        lp_aux_empty(true, w);
      } else {
        xa = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xa), fa & (WAVE - 1)));
        row_agent_sums(r, b, m, &S, &sx, RowNoHook{}, RowNoHook{});
        lp_aux(xa, m, S, sx, w);
      }
    }
#pragma unroll
    for (int k = 0; k < LP_AUX; ++k)
      if (lane == b * LP_AUX + k) st = w[k];
  }
  if (refused && lane == 0) atomicOr(fault, (int32_t)LP_REFUSED);

  // 3. the outputs
  if (lane < NBLUE * LP_AUX) aux[(size_t)row * (NBLUE * LP_AUX) + lane] = st;
}

__global__ __launch_bounds__(LP_WAVES * WAVE) void k_logp_fwd(const void* __restrict__ logits, int dtype, const uint8_t* __restrict__ mask,
                                                             const int32_t* __restrict__ actions, int n, float inv_t, float* __restrict__ aux,
                                                             int32_t* __restrict__ fault) {
  const int row = lp_row(n), lane = (int)threadIdx.x % WAVE;
  if (row < 0) return;
  if (dtype == 3) logp_fwd_row<3>(logits, mask, actions, row, lane, inv_t, aux, fault);
  else if (dtype == 2) logp_fwd_row<2>(logits, mask, actions, row, lane, inv_t, aux, fault);
  else logp_fwd_row<1>(logits, mask, actions, row, lane, inv_t, aux, fault);
}

template <int DT>
__device__ __forceinline__ void logp_bwd_row(const void* __restrict__ logits, const uint8_t* __restrict__ mask, const int32_t* __restrict__ actions, int row,
                                             int lane, float inv_t, const float* __restrict__ aux, const float* __restrict__ g, void* __restrict__ grad) {
  using E = typename Elem<DT>::type;
  const E* const lrow = static_cast<const E*>(logits) + (size_t)row * SA_SLOTS;
  E* const grow = static_cast<E*>(grad) + (size_t)row * SA_SLOTS;
  const uint8_t* const mrow = mask + (size_t)row * SA_SLOTS;
  // the row's words, wave-uniform
  int a[NBLUE];
  bool zero[NBLUE];
  float m[NBLUE], ls[NBLUE], H[NBLUE], g0[NBLUE], g1[NBLUE];
#pragma unroll
  for (int b = 0; b < NBLUE; ++b) {
    const float* const w = aux + (size_t)row * (NBLUE * LP_AUX) + b * LP_AUX;
    a[b] = actions[(size_t)row * NBLUE + b];
    m[b] = w[LP_M]; ls[b] = w[LP_LOGS]; H[b] = w[LP_ENT];
    g0[b] = g[(size_t)row * (NBLUE * LP_G) + b * LP_G];
    g1[b] = g[(size_t)row * (NBLUE * LP_G) + b * LP_G + 1];
    zero[b] = lp_skipped(a[b]) || lp_refused(m[b]);
  }
#pragma unroll
  for (int j = 0; j < ROW_ROUNDS; ++j) {
    const int f = lane + WAVE * j;
    if (f >= SA_SLOTS) continue;
    const int ab = sa_agent(f);
    int fa = 0;
    bool z = true;
    float pm = 0.0f, pls = 0.0f, pH = 0.0f, p0 = 0.0f, p1 = 0.0f;
#pragma unroll
    for (int b = 0; b < NBLUE; ++b) {
      if (round_misses(j, b)) continue;
      if (ab == b) { fa = sa_off(b) + a[b]; z = zero[b]; pm = m[b]; pls = ls[b]; pH = H[b]; p0 = g0[b]; p1 = g1[b]; }
    }
    const E raw = lrow[f];
    float gr = 0.0f;
    if (!z && mrow[f] != 0) gr = lp_grad(sa_x(elem_to_float<DT>(raw), inv_t), f == fa, pm, pls, pH, p0, p1, inv_t);
    grow[f] = elem_from_float<DT>(gr);
  }
}

__global__ __launch_bounds__(LP_WAVES * WAVE) void k_logp_bwd(const void* __restrict__ logits, int dtype, const uint8_t* __restrict__ mask,
                                                             const int32_t* __restrict__ actions, int n, float inv_t, const float* __restrict__ aux,
                                                             const float* __restrict__ g, void* __restrict__ grad) {
  const int row = lp_row(n), lane = (int)threadIdx.x % WAVE;
  if (row < 0) return;
  if (dtype == 3) logp_bwd_row<3>(logits, mask, actions, row, lane, inv_t, aux, g, grad);
  else if (dtype == 2) logp_bwd_row<2>(logits, mask, actions, row, lane, inv_t, aux, g, grad);
  else logp_bwd_row<1>(logits, mask, actions, row, lane, inv_t, aux, g, grad);
}
