// cc4_k_sample.hip -- masked sampling of the blue actions from policy logits: the kernel beside the step (the definition: cc4_sample.h, shared with
// the host function).
//   k_sample_actions  cc4_sample_actions_device: one wavefront per requested episode or bank slot, the hot row read where view_rows (cc4_view_src.h)
//                     finds it; row i of the logits belongs to entry i.
//                       1. lane l owns slots l + 64 j (j < 9) of the 570-slot row and keeps their scaled logits in registers (the layout, the
//                          load and the reductions of step 3: cc4_row_wave.h, shared with k_logp_fwd); validity is blue_mask_slot of the hot row;
//                       2. the noise, in three passes through 1024 bytes of LDS (one 1280-byte granule): agents 0..2, agent 3, agent 4.  In a pass
//                          every lane computes ONE Philox block -- a block is four slots' words -- and stores its words where the owners of those
//                          slots read them, one conflict-free word per lane and round: 3 block computations per lane instead of the 9 of "every
//                          slot computes its own block and keeps a word", which was half of the kernel's vector work.  A pass whose
//                          agents are all busy is skipped, greedy calls skip all three;
//                       3. per agent: the maximum of the valid x by a butterfly of shuffles, then in one more butterfly the sum of exponentials and
//                          the sum of e (x - m), with the (score, index) arg-max riding in the same two loops; "some valid x refuses" is a ballot;
//                       4. lanes 0..4 store one agent's action each, lanes 0..9 one of the ten stat words.
//                     The empty output of a refused entry: actions -1, zero stats.
#include "cc4_view_src.h"
#include "cc4_sample.h"
#include "cc4_elem.h"
#include "cc4_row_wave.h"
#include "cc4_kernel_decls.h"

static_assert(SA_GREEDY == CC4_SAMPLE_GREEDY && SA_BUSY == CC4_SAMPLE_BUSY && SA_TAG == CC4_SAMPLE_TAG && SA_SLOTS == CC4_MASK_PER_ENV && NBLUE == CC4_NUM_BLUE, "include/cc4.h states the flags and the shapes");
static_assert(NBLUE * SA_STATS <= WAVE, "the lanes of step 4");
// the passes of step 2: first agent, agents, and the slots they cover
constexpr int SA_PASSES = 3, SA_PASS_WORDS = 256;
constexpr int SA_SHORT_BLOCKS = (ACT_SHORT + 3) / 4, SA_LONG_BLOCKS = (ACT_LONG + 3) / 4;
__host__ __device__ constexpr int sa_pass_first(int p) { return p == 0 ? 0 : p + 2; }
__host__ __device__ constexpr int sa_pass_agents(int p) { return p == 0 ? 3 : 1; }
__host__ __device__ constexpr int sa_pass_base(int p) { return sa_off(sa_pass_first(p)); }
__host__ __device__ constexpr int sa_pass_end(int p) { return p == SA_PASSES - 1 ? (int)SA_SLOTS : sa_off(sa_pass_first(p) + sa_pass_agents(p)); }
static_assert(sa_pass_end(0) == sa_pass_base(1) && sa_pass_end(1) == sa_pass_base(2) && sa_pass_end(2) == SA_SLOTS && sa_pass_first(2) == NBLUE - 1, "the passes cover the row");
static_assert(3 * SA_SHORT_BLOCKS <= WAVE && SA_LONG_BLOCKS <= WAVE && 3 * ACT_SHORT <= SA_PASS_WORDS && ACT_LONG <= SA_PASS_WORDS, "a block per lane, a word per slot of the pass");

__global__ __launch_bounds__(WAVE) void k_sample_actions(SampleArgs a) {
  __shared__ uint32_t nz[SA_PASS_WORDS];                 // the noise words of the current pass's slots
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (i >= a.src.count) return;
  int32_t* const oa = a.actions + (size_t)i * NBLUE;
  float* const os = a.stats ? a.stats + (size_t)i * (NBLUE * SA_STATS) : nullptr;
  const ViewRows vr = view_rows(a.src, i, lane);        // (wave-uniform: cc4_view_src.h)
  if (vr.fault) {
    if (lane < NBLUE) oa[lane] = SA_NONE;
    if (os && lane < NBLUE * SA_STATS) os[lane] = 0.0f;
    return;
  }
  const EnvState* const s = vr.s;
  const int e = a.src.ids ? a.src.ids[i] : i;           // the entry's id: what view_rows resolved
  const bool greedy = (a.flags & SA_GREEDY) != 0;
  const void* const row = a.logits ? static_cast<const char*>(a.logits) + (size_t)i * SA_SLOTS * (a.dtype == 3 ? 4u : 2u) : nullptr;

  // 1. this lane's slots: agent, validity, scaled logit
  RowSlots r;
  row_load(r, lane, [&](int b, int f, float* x) {
    if (!blue_mask_slot(s, b, f - sa_off(b))) return false;
    if (row) *x = sa_x(elem_load(row, a.dtype, f), a.inv_t);
    return true;
  });

  // 2. the noise of this lane's valid slots
  float g[ROW_ROUNDS];
#pragma unroll
  for (int j = 0; j < ROW_ROUNDS; ++j) g[j] = 0.0f;
  if (!greedy) {
#pragma unroll
    for (int p = 0; p < SA_PASSES; ++p) {
      bool wanted = false;                                           // (wave-uniform)
#pragma unroll
      for (int b = sa_pass_first(p); b < sa_pass_first(p) + sa_pass_agents(p); ++b) wanted = wanted || !((a.flags & SA_BUSY) && bv_busy(s, b));
      if (!wanted) continue;
      const int b = sa_pass_agents(p) == 1 ? sa_pass_first(p) : lane / SA_SHORT_BLOCKS;
      const int G = sa_pass_agents(p) == 1 ? lane : lane % SA_SHORT_BLOCKS;
      if (p > 0) __syncthreads();                                    // the last pass's words have been read
      if (b < sa_pass_first(p) + sa_pass_agents(p) && G < (sa_len(sa_pass_first(p)) + 3) / 4) {
        uint32_t c[4];
        sa_block(a.seed0, a.t, e, b, G, c, true);
        const int at = sa_off(b) - sa_pass_base(p) + 4 * G, n = sa_len(sa_pass_first(p)) - 4 * G;      // n: slots of the block inside the segment
        nz[at] = c[0];
        if (n > 1) nz[at + 1] = c[1];
        if (n > 2) nz[at + 2] = c[2];
        if (n > 3) nz[at + 3] = c[3];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < ROW_ROUNDS; ++j) {
        if (WAVE * j + WAVE - 1 < sa_pass_base(p) || WAVE * j >= sa_pass_end(p)) continue;      // no slot of the pass in this round
        const int f = lane + WAVE * j;
        if (f >= sa_pass_base(p) && f < sa_pass_end(p) && ((r.vmask >> j) & 1u)) g[j] = sa_gumbel(nz[f - sa_pass_base(p)]);
      }
    }
  }

  // 3. per agent
  int act = SA_NONE;           // lanes 0 .. 4: the action of agent `lane`
  float st = 0.0f;             // lanes 0 .. 9: stat word `lane`
  bool refused = false;
#pragma unroll
  for (int b = 0; b < NBLUE; ++b) {
    if ((a.flags & SA_BUSY) && bv_busy(s, b)) continue;            // (wave-uniform)
    float m, S, sx, zb = -sa_inf(), xa = 0.0f;
    int ib = 0x7FFFFFFF;
    if (!row_agent_max(r, b, &m, RowNoHook{})) { refused = true; continue; }
    row_agent_sums(r, b, m, &S, &sx,
      [&](int j) {                                                   // the lane's arg-max of the scores
        if (r.x[j] == -sa_inf()) return;
        const float z = r.x[j] + g[j];
        if (sa_better(z, lane + WAVE * j - sa_off(b), zb, ib)) { zb = z; ib = lane + WAVE * j - sa_off(b); xa = r.x[j]; }
      },
      [&](int d) {                                                   // ... and the wave's
        const float zo = __shfl_xor(zb, d), xo = __shfl_xor(xa, d);
        const int io = __shfl_xor(ib, d);
        if (sa_better(zo, io, zb, ib)) { zb = zo; ib = io; xa = xo; }
      });
    float logp, ent;
    sa_stats(xa, m, S, sx, &logp, &ent);
    if (lane == b) act = ib;
    if (lane == b * SA_STATS) st = logp;
    if (lane == b * SA_STATS + 1) st = ent;
  }
  if (refused && lane == 0) atomicOr(a.src.fault, CF_RANGE);

  // 4. the outputs
  if (lane < NBLUE) oa[lane] = act;
  if (os && lane < NBLUE * SA_STATS) os[lane] = st;
}
