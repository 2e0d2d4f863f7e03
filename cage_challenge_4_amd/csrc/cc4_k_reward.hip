// cc4_k_reward.hip -- the pieces of the step reward as device tensors: the kernel beside the step (the definition: cc4_reward_terms.h, shared with the
// host function).
//   k_reward_terms   cc4_reward_terms_device: one wavefront per requested episode or bank slot, the rows read where view_rows (cc4_view_src.h)
//                    finds them -- a snapshot slot carries the record in the tail of the fixed part of the cold row.
//                      1. the 36 cells are zeroed in LDS (144 bytes: one of the 1280-byte granules LDS is handed out in);
//                      2. when the record describes the row's last step: one green agent per lane (agents 64.. in a second pass of 16 lanes) tests its
//                         bit in the two bitmaps and adds its subnet's table value and an event to its cells with LDS atomics; lanes 0..5 add the six red
//                         agents' Impact terms.  No assumption on how the agents are laid out over the subnets;
//                      3. lanes 0..8 store one subnet's four cells each, lanes 16..19 four of the 16 words each: 16-byte stores from consecutive lanes
//                         to consecutive addresses, 144 + 64 bytes.
//                    Read per episode: phase, step_count, n_green, green_host, the red headers' exec / nsess words, and the 64-byte record.
//                    The empty output of a refused entry: all zero.
#include "cc4_view_src.h"
#include "cc4_reward_terms.h"
#include "cc4_kernel_decls.h"

static_assert(RT_SUBNETS == CC4_REWARD_SUBNETS && RT_COLS == CC4_REWARD_COLS && RT_WORDS == CC4_REWARD_WORDS && NBLUE == CC4_NUM_BLUE, "include/cc4.h states the shapes");
static_assert(RT_SUBNETS <= 16 && RT_WORDS / 4 <= WAVE - 16 && MAXG <= 2 * WAVE && NRED <= WAVE, "the lanes of step 2 and 3");

__global__ __launch_bounds__(WAVE) void k_reward_terms(RewardArgs a) {
  __shared__ int32_t cells[RT_CELLS];
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (i >= a.src.count) return;
  uint4* const ot = reinterpret_cast<uint4*>(a.terms + (size_t)i * RT_CELLS);
  uint4* const ow = a.words ? reinterpret_cast<uint4*>(a.words + (size_t)i * RT_WORDS) : nullptr;
  const ViewRows vr = view_rows(a.src, i, lane);        // (wave-uniform: cc4_view_src.h)
  if (vr.fault) {
    if (lane < RT_SUBNETS) ot[lane] = make_uint4(0u, 0u, 0u, 0u);
    else if (ow && lane >= 16 && lane < 16 + RT_WORDS / 4) ow[lane - 16] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const EnvState* const s = vr.s;
  const EnvCold* const c = vr.c;
  const RewardRec* const r = &c->rwd;

  if (lane < RT_CELLS) cells[lane] = 0;
  __syncthreads();
  const bool valid = rt_valid(s, r);
  if (valid) {
    RtHit h;
    for (int g = lane; g < MAXG; g += WAVE) {
      if (rt_green(s, r, g, RTC_LWF, &h)) rt_fold(cells, h);
      if (rt_green(s, r, g, RTC_ASF, &h)) rt_fold(cells, h);
    }
    if (lane < NRED && rt_impact(s, lane, &h)) rt_fold(cells, h);
  }
  __syncthreads();
  if (lane < RT_SUBNETS) {
    const int32_t* const p = cells + lane * RT_COLS;
    ot[lane] = make_uint4((uint32_t)p[0], (uint32_t)p[1], (uint32_t)p[2], (uint32_t)p[3]);
  } else if (ow && lane >= 16 && lane < 16 + RT_WORDS / 4) {
    const int k = 4 * (lane - 16);
    ow[lane - 16] = make_uint4((uint32_t)rt_word(s, r, valid, cells, k), (uint32_t)rt_word(s, r, valid, cells, k + 1),
                               (uint32_t)rt_word(s, r, valid, cells, k + 2), (uint32_t)rt_word(s, r, valid, cells, k + 3));
  }
}
