// cc4_k_sample.hip -- masked sampling of the blue actions from policy logits: the kernel beside the step (the definition: cc4_sample.h, shared with
// the host function).
//   k_sample_actions  cc4_sample_actions_device: one wavefront per requested episode or bank slot, the hot row read where view_rows (cc4_view_src.h)
//                     finds it; row i of the logits belongs to entry i.
//                       1. lane l owns slots l + 64 j (j < 9) of the 570-slot row -- every load instruction reads 64 consecutive values, 4 or 2 bytes
//                          each, so no row alignment beyond the element's is assumed -- and keeps their scaled logits in registers; which agent a slot
//                          belongs to is a compare against the four segment offsets, and which of the nine j can hold a slot of agent b at all is
//                          known to the compiler;
//                       2. the noise, in three passes through 1024 bytes of LDS (one 1280-byte granule): agents 0..2, agent 3, agent 4.  In a pass
//                          every lane computes ONE Philox block -- a block is four slots' words -- and stores its words where the owners of those
//                          slots read them, one conflict-free word per lane and round: 3 block computations per lane instead of the 9 of "every
//                          slot computes its own block and keeps a word", which was half of the kernel's vector work.  A pass whose
//                          agents are all busy is skipped, greedy calls skip all three;
//                       3. per agent: the maximum of the valid x by a butterfly of shuffles, then in one more butterfly the sum of exponentials, the
//                          sum of e (x - m) and the (score, index) arg-max; "some valid x refuses" is a ballot;
//                       4. lanes 0..4 store one agent's action each, lanes 0..9 one of the ten stat words.
//                     The empty output of a refused entry: actions -1, zero stats.
#include "cc4_view_src.h"
#include "cc4_sample.h"
#include "cc4_kernel_decls.h"

static_assert(SA_GREEDY == CC4_SAMPLE_GREEDY && SA_BUSY == CC4_SAMPLE_BUSY && SA_TAG == CC4_SAMPLE_TAG && SA_SLOTS == CC4_MASK_PER_ENV && NBLUE == CC4_NUM_BLUE, "include/cc4.h states the flags and the shapes");
constexpr int SA_ROUNDS = (SA_SLOTS + WAVE - 1) / WAVE;      // slots per lane
static_assert(SA_ROUNDS == 9 && NBLUE * SA_STATS <= WAVE, "the lanes of step 1 and 4");
// the passes of step 2: first agent, agents, and the slots they cover
constexpr int SA_PASSES = 3, SA_PASS_WORDS = 256;
constexpr int SA_SHORT_BLOCKS = (ACT_SHORT + 3) / 4, SA_LONG_BLOCKS = (ACT_LONG + 3) / 4;
__host__ __device__ constexpr int sa_pass_first(int p) { return p == 0 ? 0 : p + 2; }
__host__ __device__ constexpr int sa_pass_agents(int p) { return p == 0 ? 3 : 1; }
__host__ __device__ constexpr int sa_pass_base(int p) { return sa_off(sa_pass_first(p)); }
__host__ __device__ constexpr int sa_pass_end(int p) { return p == SA_PASSES - 1 ? (int)SA_SLOTS : sa_off(sa_pass_first(p) + sa_pass_agents(p)); }
static_assert(sa_pass_end(0) == sa_pass_base(1) && sa_pass_end(1) == sa_pass_base(2) && sa_pass_end(2) == SA_SLOTS && sa_pass_first(2) == NBLUE - 1, "the passes cover the row");
static_assert(3 * SA_SHORT_BLOCKS <= WAVE && SA_LONG_BLOCKS <= WAVE && 3 * ACT_SHORT <= SA_PASS_WORDS && ACT_LONG <= SA_PASS_WORDS, "a block per lane, a word per slot of the pass");

// logits value f of a row in the dtype codes of cc4_policy_outputs (1 float16, 2 bfloat16, 3 float32)
__device__ __forceinline__ float sa_load(const void* row, int dtype, int f) {
  if (dtype == 3) return static_cast<const float*>(row)[f];
  const uint16_t h = static_cast<const uint16_t*>(row)[f];
  if (dtype == 2) return __uint_as_float((uint32_t)h << 16);
  _Float16 v;
  __builtin_memcpy(&v, &h, 2);
  return (float)v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) { const float o = __shfl_xor(v, d); v = o > v ? o : v; }
  return v;
}

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
  float x[SA_ROUNDS];
  int ag[SA_ROUNDS];
  uint32_t vmask = 0;
#pragma unroll
  for (int j = 0; j < SA_ROUNDS; ++j) {
    const int f = lane + WAVE * j;
    x[j] = 0.0f; ag[j] = 0;
    if (f < SA_SLOTS) {
      const int b = sa_agent(f);
      ag[j] = b;
      if (blue_mask_slot(s, b, f - sa_off(b))) {
        vmask |= 1u << j;
        if (row) x[j] = sa_x(sa_load(row, a.dtype, f), a.inv_t);
      }
    }
  }

  // 2. the noise of this lane's valid slots
  float g[SA_ROUNDS];
#pragma unroll
  for (int j = 0; j < SA_ROUNDS; ++j) g[j] = 0.0f;
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
      for (int j = 0; j < SA_ROUNDS; ++j) {
        if (WAVE * j + WAVE - 1 < sa_pass_base(p) || WAVE * j >= sa_pass_end(p)) continue;      // no slot of the pass in this round
        const int f = lane + WAVE * j;
        if (f >= sa_pass_base(p) && f < sa_pass_end(p) && ((vmask >> j) & 1u)) g[j] = sa_gumbel(nz[f - sa_pass_base(p)]);
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
    bool bad = false;
    float m = -sa_inf();
#pragma unroll
    for (int j = 0; j < SA_ROUNDS; ++j) {
      if (WAVE * j + WAVE - 1 < sa_off(b) || WAVE * j >= sa_off(b) + sa_len(b)) continue;      // no slot of agent b in this round
      if (ag[j] == b && ((vmask >> j) & 1u)) { bad = bad || sa_refuses(x[j]); m = x[j] > m ? x[j] : m; }
    }
    m = wave_max(m);
    if (__ballot(bad) != 0ull || m == -sa_inf()) { refused = true; continue; }
    float S = 0.0f, sx = 0.0f, zb = -sa_inf(), xa = 0.0f;
    int ib = 0x7FFFFFFF;
#pragma unroll
    for (int j = 0; j < SA_ROUNDS; ++j) {
      if (WAVE * j + WAVE - 1 < sa_off(b) || WAVE * j >= sa_off(b) + sa_len(b)) continue;
      if (ag[j] != b || !((vmask >> j) & 1u)) continue;
      const int k = lane + WAVE * j - sa_off(b);
      const float d = x[j] - m, ex = expf(d);
      S += ex;
      sx += ex > 0.0f ? ex * d : 0.0f;
      if (x[j] == -sa_inf()) continue;
      const float z = x[j] + g[j];
      if (sa_better(z, k, zb, ib)) { zb = z; ib = k; xa = x[j]; }
    }
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      S += __shfl_xor(S, d);
      sx += __shfl_xor(sx, d);
      const float zo = __shfl_xor(zb, d), xo = __shfl_xor(xa, d);
      const int io = __shfl_xor(ib, d);
      if (sa_better(zo, io, zb, ib)) { zb = zo; ib = io; xa = xo; }
    }
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
