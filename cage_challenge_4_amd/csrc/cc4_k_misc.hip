// cc4_k_misc.hip -- k_reset and the small kernels of libcc4.so (exchange gate, CU discovery, stand-in policies, seeds, digest, event-log helpers).
#include "cc4_persist.h"      // (cu_slot: k_discover)
#include "cc4_kernel_decls.h"
#include "cc4_digest.h"       // (k_digest)

// The gate of a chunk of steps [k_lo, k_hi] on the communication stream: returns when every group has counted all its episodes in every
// step of the chunk (counts of one episode's consecutive steps may arrive out of order: each wave counts where ITS stores have drained),
// and hands the counters back (zero) for steps k + ring.  P > 0: the groups are the P partitions of the persistent kernel (episodes
// g, g + P, ..: part_episodes), else groups of 32 neighbouring episodes (xchg_group32_size).  Gives up after `ticks` and says so in *fail (the host reports it).
// ONE wave, polling at a growing interval (4 us .. 31 us; the gate of a call's LAST step, behind which the host waits, stays at 4 us): the gate shares a CU with blocks of the step kernel, and in the multi-step kernels
// a block is an episode -- whatever slows one CU's blocks sets the pace of the launch (four busily polling waves cost 1024 episodes 1.2 us per step).
__global__ __launch_bounds__(WAVE) void k_xchg_gate(uint32_t* gcnt, int ring, int groups, int n, int P, int k_lo, int k_hi, long long ticks, uint32_t* fail, int max_naps) {
  const int t = (int)threadIdx.x, steps = k_hi - k_lo + 1;
  const long long t0 = wall_clock64();
  for (int i = t; i < groups * steps; i += (int)blockDim.x) {
    const int g = i / steps, k = k_lo + i % steps;
    const int size = P > 0 ? part_episodes(n, P, g) : xchg_group32_size(n, g);
    if (size <= 0) continue;
    uint32_t* c = gcnt + (size_t)g * (size_t)ring + (k % ring);
    int naps = 1;
    while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (uint32_t)size) {
      for (int q = 0; q < naps; ++q) __builtin_amdgcn_s_sleep(127);
      if (naps < max_naps) naps <<= 1;
      if (wall_clock64() - t0 > ticks) { __hip_atomic_store(fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
    }
    __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
// which compute units does this device have?  Many small waves without LDS, each reporting the CU it landed on and idling long enough for
// the grid to spread over the whole chip.  (Not a census of how many waves of the REAL kernel a CU takes: LDS is allocated in 1280-byte
// granules, a proxy with another footprint lands differently -- r05 -- and the schedule does not need to know.)
__global__ __launch_bounds__(WAVE) void k_discover(int32_t* count, long long ticks) {
  if (threadIdx.x == 0) {
    atomicAdd(&count[cu_slot()], 1);
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
  }
}
__global__ __launch_bounds__(WAVE) void k_reset(ResetArgs a) {
  __shared__ uint8_t obs_lds[OBS_TOTAL + 2];
  __shared__ uint8_t mask_lds[MASK_TOTAL + 2];
  __shared__ StepWork work;
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= a.n) return;
  if (a.env_mask && !a.env_mask[e]) return;
  EnvCold* const cold_e = cold_at(a.cold, (size_t)e, cold_row_bytes(a.steps));
  EnvState* s = a.st + e;
  HostDyn* const hd = s->hd;
  for (int i = lane; i < (int)(sizeof(StepWork) / 4); i += WAVE) reinterpret_cast<uint32_t*>(&work)[i] = 0;
  __syncthreads();
  if (a.rng_mode == 1) {   // counter-based mode: hosts on lanes, the main stream walked in place (the row stays in HBM here)
    __shared__ uint32_t ws[RESET_WS_WORDS];
    reset_counter_mode_block<WAVE, false>(s, hd, cold_e, &work, lane, ws, a.seeds ? a.seeds[e] : 0, a.seeds == nullptr, a.steps, a.policy, a.topo);
    __syncthreads();
  } else if (lane == 0) {
    Ctx x{s, cold_e, &s->rng, hd, &work};
    env_reset(x, a.seeds ? a.seeds[e] : 0, 0, a.steps, a.seeds == nullptr, a.policy, a.topo);
  }
  if (lane == 0) {
    env_flat_obs<uint8_t>(s, obs_lds);
    blue_action_mask(s, mask_lds);
    a.reward[e] = 0.f; a.done[e] = s->done; a.err[e] = s->err;
  }
  __syncthreads();
  int32_t* o = a.obs + (size_t)e * OBS_TOTAL;
  for (int i = lane; i < OBS_TOTAL; i += WAVE) o[i] = obs_lds[i];
  uint8_t* m = a.mask + (size_t)e * MASK_TOTAL;
  for (int i = lane; i < MASK_TOTAL; i += WAVE) m[i] = mask_lds[i];
  if (a.obs8) store_packed_row(a.obs8 + (size_t)e * OBS_PACKED, obs_lds, lane, WAVE);
}

// uniform blue action indices over each agent's full range: Philox key (seed0, env),
// counter (t, agent, 0xB10E, 0)
__global__ void k_random_actions(int32_t* actions, int n, uint64_t seed0, uint32_t t, int e0) {      // episodes e0 .. n - 1
  int i = e0 * NBLUE + blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * NBLUE) return;
  int e = i / NBLUE, b = i % NBLUE;
  actions[i] = random_blue_action(seed0, t, e, b);
}

// debug: keeps a stream busy for about `cycles` clock ticks (cc4_debug_comm_delay_us: a slow exchange on demand)
__global__ void k_spin(long long cycles) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < cycles) __builtin_amdgcn_s_sleep(32);
}

// one block per gathered row: 148 packed bytes -> 578 byte values (thread j unpacks byte j into values 4j .. 4j+3)
__global__ void k_unpack_obs(const uint8_t* __restrict__ packed, uint8_t* __restrict__ out, int rows) {
  const int r = blockIdx.x, j = threadIdx.x;
  if (r >= rows || j >= OBS_PACKED) return;
  const uint32_t b = packed[(size_t)r * OBS_PACKED + j];
  uint8_t* o = out + (size_t)r * OBS_TOTAL + 4 * j;
#pragma unroll
  for (int k = 0; k < 4; ++k) if (4 * j + k < OBS_TOTAL) o[k] = (uint8_t)((b >> (2 * k)) & 3u);
}

// cc4_policy_outputs: the handle's outputs as a policy consumes them, in caller-owned buffers.  ONE launch, two kinds of blocks:
//   blocks [0, ep_blocks): one lane per episode -- reward, done, error word, and the action-mask row of every episode whose row was
//     (re)generated since its last step (step_count 0: cc4_reset, or the in-kernel autoreset of the step just taken); the wave ballots
//     those and rebuilds each one's 570 entries with all 64 lanes (blue_mask_slot, the rule of blue_action_mask).  Mask rows of the other
//     episodes are left as they are: a mask is a function of the scenario alone, so the caller's buffer is persistent.  Rows of episodes
//     that a copy overwrote (cc4_copy_episodes_device: the handle's per-episode "mask stale" mark) are rebuilt as well, and their marks cleared.
//   blocks [ep_blocks, grid): the observations as ONE flat array of n * 578 int32 values (a 2312-byte row is not 16-byte aligned, the
//     flat array is), grid-stride, one int4 load and one store of the four converted values per lane (4 / 8 / 8 / 16 bytes).  Every value is
//     0, 1 or 2 (CC4_OBS_PACKED_BYTES), so every dtype is exact; half and bfloat16 bit patterns come from a 4-entry table in one constant.
// Reads the handle's buffers; of its own it writes only the mask-stale marks.
// float16 (0, 1, 2, 3 -> 0x0000 0x3C00 0x4000 0x4200) / bfloat16 (-> 0x0000 0x3F80 0x4000 0x4040): the bit pattern of a value out of one constant
template <int DT> __device__ __forceinline__ uint32_t policy_half_bits(int x) {
  constexpr uint64_t tab = DT == 1 ? 0x420040003C000000ull : 0x404040003F800000ull;
  return (uint32_t)(tab >> (16 * (x & 3))) & 0xFFFFu;
}
template <int DT> __device__ __forceinline__ void policy_obs_put(void* out, size_t i, int4 v) {
  if constexpr (DT == 0) {          // uint8
    reinterpret_cast<uint32_t*>(out)[i] = (uint32_t)(v.x & 0xFF) | (uint32_t)(v.y & 0xFF) << 8 | (uint32_t)(v.z & 0xFF) << 16 | (uint32_t)(v.w & 0xFF) << 24;
  } else if constexpr (DT == 3) {   // float32
    reinterpret_cast<float4*>(out)[i] = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
  } else {                          // float16 / bfloat16
    reinterpret_cast<uint2*>(out)[i] = make_uint2(policy_half_bits<DT>(v.x) | policy_half_bits<DT>(v.y) << 16, policy_half_bits<DT>(v.z) | policy_half_bits<DT>(v.w) << 16);
  }
}
template <int DT> __device__ __forceinline__ void policy_obs_part(const int32_t* __restrict__ obs, void* __restrict__ out, size_t total, size_t i0, size_t stride) {
  const size_t nv = total / 4;
  const int4* __restrict__ src = reinterpret_cast<const int4*>(obs);
  for (size_t i = i0; i < nv; i += stride) policy_obs_put<DT>(out, i, src[i]);
  if (i0 == 0) {                    // an odd batch: the last two values one at a time (578 * n is even)
    for (size_t j = 4 * nv; j < total; ++j) {
      const int x = obs[j];
      if constexpr (DT == 0) reinterpret_cast<uint8_t*>(out)[j] = (uint8_t)x;
      else if constexpr (DT == 3) reinterpret_cast<float*>(out)[j] = (float)x;
      else reinterpret_cast<uint16_t*>(out)[j] = (uint16_t)policy_half_bits<DT>(x);
    }
  }
}
__global__ __launch_bounds__(256) void k_policy_outputs(const EnvState* __restrict__ st, const int32_t* __restrict__ obs, const float* __restrict__ reward,
                                                        const uint8_t* __restrict__ done, const uint32_t* __restrict__ err, int n, int ep_blocks, int dtype,
                                                        void* __restrict__ out_obs, uint8_t* __restrict__ out_mask, float* __restrict__ out_reward,
                                                        uint8_t* __restrict__ out_done, int32_t* __restrict__ out_err, uint8_t* __restrict__ mask_stale) {
  if ((int)blockIdx.x < ep_blocks) {
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x), lane = (int)threadIdx.x & (WAVE - 1);
    bool regen = false;
    if (e < n) {
      out_reward[e] = reward[e]; out_done[e] = done[e]; out_err[e] = (int32_t)err[e];
      regen = st[e].step_count == 0;
      if (mask_stale[e]) { regen = true; mask_stale[e] = 0; }     // a copy of another episode landed here (k_copy_episodes)
    }
    unsigned long long todo = __ballot(regen);
    while (todo) {
      const int k = __ffsll(todo) - 1;
      todo &= todo - 1;
      const int er = e - lane + k;
      const EnvState* s = st + er;
      uint8_t* m = out_mask + (size_t)er * MASK_TOTAL;
      for (int o = lane; o < MASK_TOTAL; o += WAVE) {
        const int b = o < 4 * ACT_SHORT ? o / ACT_SHORT : 4;
        m[o] = blue_mask_slot(s, b, o - b * ACT_SHORT);
      }
    }
    return;
  }
  const size_t total = (size_t)n * OBS_TOTAL;
  const size_t i0 = (size_t)(blockIdx.x - ep_blocks) * blockDim.x + threadIdx.x, stride = (size_t)(gridDim.x - ep_blocks) * blockDim.x;
  switch (dtype) {
    case 0: policy_obs_part<0>(obs, out_obs, total, i0, stride); break;
    case 1: policy_obs_part<1>(obs, out_obs, total, i0, stride); break;
    case 2: policy_obs_part<2>(obs, out_obs, total, i0, stride); break;
    default: policy_obs_part<3>(obs, out_obs, total, i0, stride); break;
  }
}

// cc4_set_policies_device: one lane per episode, the rule of row_assign (cc4_state.h).  A refused value leaves the episode as it is and raises CF_RANGE.
__global__ __launch_bounds__(256) void k_set_policies(EnvState* st, const int8_t* __restrict__ red, const int8_t* __restrict__ green, const int8_t* __restrict__ blue,
                                                      int n, uint32_t* fault) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= n) return;
  if (!row_assign(st + e, red ? red[e] : PA_KEEP, green ? green[e] : PA_KEEP, blue ? blue[e] : PA_KEEP)) atomicOr(fault, (uint32_t)CF_RANGE);
}
// cc4_policies_device: live classes and assignment of every episode as [n][3] (row_policies); either output may be null
__global__ __launch_bounds__(256) void k_get_policies(const EnvState* __restrict__ st, int8_t* __restrict__ live, int8_t* __restrict__ assigned, int n) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= n) return;
  row_policies(st + e, live ? live + 3 * (size_t)e : nullptr, assigned ? assigned + 3 * (size_t)e : nullptr);
}

// CybORG.set_seed (env.py:316-325) on every episode (episode_set_seed)
__global__ void k_set_seed(EnvState* st, EnvCold* cold, size_t cold_row, const uint64_t* seeds, int n, int rng_mode) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  episode_set_seed(st + e, cold_at(cold, (size_t)e, cold_row), seeds[e], rng_mode);
}

// an externally built numpy Generator(PCG64) handed over as CybORG(seed=generator) (env.py:73-76): its bit-generator state
// becomes the episode's stream (words per episode: state high, state low, increment high, increment low, has_uint32, uinteger)
__global__ void k_set_rng_state(EnvState* st, const uint64_t* w, int n) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  Rng r;
  rng_seed(&r, 0, 0);
  r.s_hi = w[6 * e]; r.s_lo = w[6 * e + 1]; r.inc_hi = w[6 * e + 2]; r.inc_lo = w[6 * e + 3];
  r.has32 = (uint32_t)w[6 * e + 4]; r.u32 = (uint32_t)w[6 * e + 5];
  st[e].rng = r;
  st[e].rng_split = 0;
}

__global__ void k_rng_state(const EnvState* st, uint64_t* out, int n) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const Rng& r = st[e].rng;
  uint64_t* o = out + 7 * (size_t)e;
  o[0] = r.s_hi; o[1] = r.s_lo; o[2] = r.inc_hi; o[3] = r.inc_lo; o[4] = r.has32; o[5] = r.u32; o[6] = r.ndraw;
}

// ---------------------------------------------------------------- rollouts: the caller-side kernels (cc4_rollout_*)
// gate of a policy pass: returns when every episode of policy group g has its packed row of the step in slot `slot` in memory (the step kernel
// counts them per partition, RunArgs.act_ready), and hands the counters back zeroed.  One wave, partitions on lanes; gives up after `ticks`.
__device__ __forceinline__ void rollout_gate_wait(uint32_t* cnt, int P, int PG, int ring, int g, int slot, int n, long long ticks, uint32_t* fail) {
  const long long t0 = wall_clock64();
  for (int p = (int)threadIdx.x; p < P; p += (int)blockDim.x) {
    const int want = pgroup_episodes(part_episodes(n, P, p), PG, g);      // of episodes p, p + P, ..: number i is of group i % PG
    if (want <= 0) continue;
    uint32_t* c = cnt + ((size_t)p * PG + (size_t)g) * (size_t)ring + slot;
    int naps = 1;
    while (__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (uint32_t)want) {
      for (int q = 0; q < naps; ++q) __builtin_amdgcn_s_sleep(8);
      if (naps < 8) naps <<= 1;
      if (wall_clock64() - t0 > ticks) { __hip_atomic_store(fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
    }
    __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
__global__ __launch_bounds__(WAVE) void k_rollout_gate(uint32_t* cnt, int P, int PG, int ring, int g, int slot, int n, long long ticks, uint32_t* fail) {
  __builtin_amdgcn_s_setprio(3);      // these waves run in what the persistent kernel leaves of a CU, beside 23 of its waves per CU: ahead of them in the SIMDs' issue arbitration
  rollout_gate_wait(cnt, P, PG, ring, g, slot, n, ticks, fail);
}
// publish and gate in one launch (cc4_rollout_sync): first the publish of a pass whose policy kernels precede this kernel on the stream (their stores
// are in memory: a kernel boundary lies between), then the gate of the next pass.  Half the stream operations of the separate calls.
__global__ __launch_bounds__(WAVE) void k_rollout_sync(uint32_t* ready, int pub_g, uint32_t pub_val, uint32_t* cnt, int P, int PG, int ring, int g, int slot, int n, long long ticks, uint32_t* fail) {
  __builtin_amdgcn_s_setprio(3);      // these waves run in what the persistent kernel leaves of a CU, beside 23 of its waves per CU: ahead of them in the SIMDs' issue arbitration
  // the publish: every CU partition's copy of the group's word (RunArgs.act_ready)
  if (pub_g >= 0) for (int p = (int)threadIdx.x; p < P; p += (int)blockDim.x) __hip_atomic_store(ready + (size_t)p * 32 + pub_g, pub_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (g >= 0) rollout_gate_wait(cnt, P, PG, ring, g, slot, n, ticks, fail);
}
// stand-in policies for one policy group (bench.py, tests): uniform random indices (the draws of k_random_actions), or indices computed FROM the
// packed observations of the step before (a policy that ignores its input proves nothing about the hand-over)
// (threads over the GROUP's episodes only -- thread i < pgroup_threads is episode pgroup_episode(i, ..) of group g, cc4_sched.h --: a launch is a quarter of the
// batch's waves, one dispatch round into the slots the persistent kernel leaves free)
__global__ __launch_bounds__(WAVE) void k_rollout_random_policy(int32_t* act, int n, int P, int PG, int g, uint64_t seed0, uint32_t t) {
  __builtin_amdgcn_s_setprio(3);      // these waves run in what the persistent kernel leaves of a CU, beside 23 of its waves per CU: ahead of them in the SIMDs' issue arbitration
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = pgroup_episode(i / NBLUE, P, PG, g), b = i % NBLUE;
  if (e >= n) return;
  act[e * NBLUE + b] = random_blue_action(seed0, t, e, b);
}
__device__ __host__ inline uint32_t rollout_obs_hash(const uint32_t* row) {      // 37 words of a packed observation row
  uint32_t hsh = 2166136261u;
  for (int w = 0; w < OBS_PACKED / 4; ++w) { hsh ^= row[w]; hsh *= 16777619u; }
  return hsh;
}
__global__ __launch_bounds__(WAVE) void k_rollout_hash_policy(int32_t* act, const uint8_t* packed, int n, int P, int PG, int g, uint32_t j) {
  __builtin_amdgcn_s_setprio(3);
  const int e = pgroup_episode(blockIdx.x * blockDim.x + threadIdx.x, P, PG, g);
  if (e >= n) return;
  const uint32_t hsh = rollout_obs_hash(reinterpret_cast<const uint32_t*>(packed + (size_t)e * OBS_PACKED));
  for (int b = 0; b < NBLUE; ++b) act[e * NBLUE + b] = (int32_t)((hsh + 2654435761u * (uint32_t)(b + 1) + 40503u * j) % (uint32_t)(b == 4 ? ACT_LONG : ACT_SHORT));
}
// the packed rows of the observations as they stand in the int32 buffer (what a rollout's first policy pass reads)
__global__ __launch_bounds__(WAVE) void k_pack_obs_rows(uint8_t* packed, const int32_t* obs, int n) {
  const int e = blockIdx.x;
  if (e < n) pack_row_from_obs(packed + (size_t)e * OBS_PACKED, obs + (size_t)e * OBS_TOTAL, (int)threadIdx.x);
}

// CC4_PERSIST_VERIFY: a digest per episode of everything a call of cc4_run_random_steps leaves behind -- hot row, cold row, observations,
// reward / done / error word, the drawn actions -- in three words (hot, cold, outputs), so that a mismatch says where
__global__ __launch_bounds__(WAVE) void k_digest(const EnvState* st, const EnvCold* cold, size_t cold_row, const int32_t* obs, const float* reward,
                                                 const uint8_t* done, const uint32_t* err, const int32_t* actions, uint64_t* out, int n) {
  static_assert(DIGEST_LANES == WAVE && DIGEST_OBS == OBS_TOTAL && DIGEST_ACTIONS == NBLUE && sizeof(EnvState) % 16 == 0, "cc4_digest.h states the digest for these shapes");
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= n) return;
  // the definition: cc4_digest.h (a lane's chains there, the cross-lane sums here)
  const uint64_t h_hot = digest_wave_sum(digest_row_lane(st + e, sizeof(EnvState) / 16, lane));
  const uint64_t h_cold = digest_wave_sum(digest_row_lane(cold_at(cold, (size_t)e, cold_row), cold_row / 16, lane));
  const uint64_t h = digest_wave_sum(digest_out_lane(obs + (size_t)e * OBS_TOTAL, actions + (size_t)e * NBLUE, __float_as_uint(reward[e]), done[e], err[e], lane));
  if (lane == 0) { out[3 * (size_t)e] = h_hot; out[3 * (size_t)e + 1] = h_cold; out[3 * (size_t)e + 2] = h; }
}


// event-log helpers (cc4_enable_event_log, cc4_replay_logged)
extern "C" {
__global__ void k_set_evlog(EnvCold* cold, size_t row_bytes, int n, uint32_t on) {
  int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) { EnvCold* c = cold_at(cold, (size_t)e, row_bytes); c->evlog.enabled = on; c->evlog.n = 0; }
}
__global__ void k_copy_evlog(EnvCold* dst, const EnvCold* src, size_t row_bytes, int n) {
  const int e = blockIdx.x;
  if (e >= n) return;
  const uint32_t* s = reinterpret_cast<const uint32_t*>(&cold_at(const_cast<EnvCold*>(src), (size_t)e, row_bytes)->evlog);
  uint32_t* d = reinterpret_cast<uint32_t*>(&cold_at(dst, (size_t)e, row_bytes)->evlog);
  for (int i = threadIdx.x; i < (int)(sizeof(EvLog) / 4); i += blockDim.x) d[i] = s[i];
}
}
