// cc4_kernels.h -- the device helpers the kernels of libcc4.so share: row staging, the observation encode and the packed observation rows, the
// exchange's slab protocol, episode_set_seed, and the counter-mode scenario generation on the threads of a block.  The argument blocks and constants
// that the host side shares with the kernels are in cc4_args.h; nothing here needs the C++ host library (cc4_host.h).  The kernels themselves:
//   cc4_k_pcg.hip      numpy-stream mode: k_step<LOG>, k_run_pcg
//   cc4_k_philox4.hip  counter mode, four wavefronts per episode: k_step_philox<LOG, MINW>, k_run_philox, k_run_philox8
//   cc4_k_philox1.hip  counter mode, one wavefront per episode: k_step_philox1<LOG>, k_run_philox1m (cc4_philox1_body.h: the step's body)
//   cc4_k_run1.hip     the persistent kernel of large batches: k_run_philox1 (cc4_persist.h: its schedule, shared with k_run_pcg; cc4_sched.h: the index
//                      arithmetic of that schedule, of the gates and of the host side -- partitions, tickets, runs, the progress word, the groups of 32)
//                      -- the headline build: compiled for calls that draw their actions in the kernel and carry no actions or messages
//   cc4_k_run1g.hip    the same schedule with every run-time flag, k_run_philox1g: what persist_launch sends a call of any other shape
//   cc4_k_run1x.hip    its other builds: k_run_philox1x (beside RCCL), k_run_philox1r (rollouts with the policy in the loop)
//   cc4_k_plan.hip     the plan build of the persistent kernel, k_run_philox1p (cc4_run_plan_device), and the plan call's helpers; the numpy-stream
//                      plan build k_run_pcgp sits beside k_run_pcg (the numpy-stream step body and its jump table are private to cc4_k_pcg.hip)
//   cc4_k_misc.hip     k_reset and the small helpers (exchange gate, CU discovery, stand-in policies, digest, ...)
//   cc4_k_copy.hip     episode copies: k_copy_claim, k_copy_episodes (cc4_copy_episodes_device)
//   cc4_k_feat.hip     the true state as tensors: k_state_features (cc4_state_features_device; needs none of the helpers here, only cc4_features.h)
//   cc4_k_red.hip      the red agents as learners: k_red_submit (cc4_step_red_device), k_red_view (cc4_red_view_device); only cc4_red_view.h
//   cc4_k_blue.hip     blue's own knowledge as tensors: k_blue_view (cc4_blue_view_device); only cc4_blue_view.h
//   cc4_k_edges.hip    the Monitor's connections as edge lists: k_blue_edges (cc4_blue_edges_device); only cc4_blue_edges.h
//   cc4_k_reward.hip   the pieces of the step reward as tensors: k_reward_terms (cc4_reward_terms_device); only cc4_reward_terms.h
//   cc4_k_sample.hip   policy logits to valid blue actions: k_sample_actions (cc4_sample_actions_device); only cc4_sample.h
//   cc4_k_logp.hip     stored blue actions under new logits, with gradients: k_logp_fwd, k_logp_bwd (cc4_logp_actions_device, cc4_logp_actions_grad_device);
//                      only cc4_logp.h, no rows and no handle
//   cc4_k_gae.hip      advantages and returns of a stored rollout: k_gae (cc4_gae_device); only cc4_gae.h, no rows and no handle
// cc4_kernel_decls.h declares them for the host side.  No MFMA anywhere: the path is integer / indexing.
#pragma once
#include "cc4_args.h"

// CC4_BOUNDARY_PROF (a measurement build, make EXTRA=-DCC4_BOUNDARY_PROF; tools/persist_boundary.py): the headline kernel splits what a wave pays between
// the last step of one item and the first step_phase of its next into four sums of wall-clock ticks, kept in lane 0's registers and written once per wave
// at exit into the CC4_PERSIST_TIMELINE words (timeline_report prints them).  The shipped build compiles none of it.
#ifdef CC4_BOUNDARY_PROF
#define CC4_BP(...) do { if constexpr (HEAD) { __VA_ARGS__; } } while (0)
__shared__ unsigned long long cc4_bp_staged;      // lane 0, philox1_body: the item's rows are in LDS, step_phase is next
#else
#define CC4_BP(...) do {} while (0)
#endif

// uniform blue action index of (episode e, agent b) at step t: Philox key (seed0 + e), counter (t, b, 0xB10E, 0)
__device__ __forceinline__ int32_t random_blue_action(uint64_t seed0, uint32_t t, int e, int b) {
  uint32_t c[4] = {t, (uint32_t)b, 0xB10Eu, 0u};
  uint64_t key = seed0 + (uint64_t)e;
  philox4x32_10(c, (uint32_t)key, (uint32_t)(key >> 32));
  uint32_t range = b == 4 ? ACT_LONG : ACT_SHORT;
  return (int32_t)(((uint64_t)c[0] * range) >> 32);
}

// ---------------------------------------------------------------- kernels
// HBM -> LDS row staging with 8 independent 16-byte loads in flight per lane (a plain copy loop serialises on vmcnt)
template <int NVEC>
__device__ __forceinline__ void stage_in(uint4* __restrict__ lds, const uint4* __restrict__ src, int lane) {
  constexpr int U = NVEC / WAVE < 8 ? (NVEC / WAVE > 0 ? NVEC / WAVE : 1) : 8;
  int i = lane;
  for (; i + (U - 1) * WAVE < NVEC; i += U * WAVE) {
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = src[i + u * WAVE];
#pragma unroll
    for (int u = 0; u < U; ++u) lds[i + u * WAVE] = v[u];
  }
  for (; i < NVEC; i += WAVE) lds[i] = src[i];
}
template <int NVEC>
__device__ __forceinline__ void stage_out(uint4* __restrict__ dst, const uint4* __restrict__ lds, int lane) {
  constexpr int U = NVEC / WAVE < 8 ? (NVEC / WAVE > 0 ? NVEC / WAVE : 1) : 8;
  int i = lane;
  for (; i + (U - 1) * WAVE < NVEC; i += U * WAVE) {
    uint4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = lds[i + u * WAVE];
#pragma unroll
    for (int u = 0; u < U; ++u) dst[i + u * WAVE] = v[u];
  }
  for (; i < NVEC; i += WAVE) dst[i] = lds[i];
}

// byte j of an episode's packed observation row: values 4j .. 4j+3 (from a byte-per-value row in LDS), 2 bits each, low bits first
__device__ __forceinline__ uint8_t pack_obs_byte(const uint8_t* vals, int j) {
  uint32_t b = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { const int i = 4 * j + k; if (i < OBS_TOTAL) b |= (uint32_t)(vals[i] & 3u) << (2 * k); }
  return (uint8_t)b;
}

// An episode's packed observation row (OBS_PACKED bytes = 37 words) to memory, one word per thread, as SYSTEM-scope (write-through) stores:
// the reader is the exchange -- a copy engine, an RCCL kernel on any XCD, a peer GPU -- and, when the writer is a one-launch kernel, there is
// no kernel boundary that would write the XCD's L2 back first (tools/micro/ring_protocol.hip: plain stores arrive stale, these do not).
__device__ __forceinline__ void store_packed_row(uint8_t* o8, const uint8_t* vals, int t, int nt) {
  uint32_t* o32 = reinterpret_cast<uint32_t*>(o8);
  for (int w = t; w < OBS_PACKED / 4; w += nt) {
    const uint32_t v = (uint32_t)pack_obs_byte(vals, 4 * w) | ((uint32_t)pack_obs_byte(vals, 4 * w + 1) << 8) |
                       ((uint32_t)pack_obs_byte(vals, 4 * w + 2) << 16) | ((uint32_t)pack_obs_byte(vals, 4 * w + 3) << 24);
    __hip_atomic_store(o32 + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// The same row packed from the int32 observation row the wave has just (re)written in global memory -- the output buffer persists between
// steps, so it holds every current value although a step only rewrites the ones that changed.  For the one-wave kernels: a byte copy of the
// 578 values in LDS would cost them a seventh 1280-byte LDS granule and with it two of their twenty resident waves per CU
// (profiles/r05_lds_residency.txt).  The wave's own stores are drained first (the vector L1 is write-through: they are in the XCD's L2),
// the loads are agent-scope (served by that L2, never by a stale L1 line).
__device__ __forceinline__ void pack_row_from_obs(uint8_t* o8, const int32_t* o, int lane) {
  // call with the wave's stores drained (s_waitcnt vmcnt(0)): then plain loads see them -- the row was written by this wave, by earlier
  // waves of this CU (same L1; a stolen partition's item starts with an L1 invalidate), or before the launch
  static_assert((OBS_TOTAL * 4) % 8 == 0, "rows of the int32 observation buffer are 8-byte aligned: two values per load");
  if (lane < OBS_PACKED / 4) {
    const uint2* o2 = reinterpret_cast<const uint2*>(o + 16 * lane);
    uint2 w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = (16 * lane + 2 * k < OBS_TOTAL) ? o2[k] : make_uint2(0u, 0u);     // (578 is even: a pair is inside the row or outside)
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v |= ((w[k].x & 3u) << (4 * k)) | ((w[k].y & 3u) << (4 * k + 2));
    __hip_atomic_store(reinterpret_cast<uint32_t*>(o8) + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
// ---- the exchange's slab protocol (XchgArgs)
// lane 0: a wait gave up -- both timeout flags raised, every later wait of the launch returns at once
__device__ __forceinline__ void raise_timeout(const XchgArgs& x) {
  __hip_atomic_store(x.timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(x.timeout_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// lane / thread 0 only.  `seen` = the highest value of *gathered this wave has read so far (it only grows): the word is read again --
// an uncached round trip to memory, ~2 us in the middle of the item hand-over -- only when the value at hand does not cover step k.
__device__ __forceinline__ void xchg_wait_slab(const XchgArgs& x, uint32_t k, uint32_t& seen) {
  if (k < (uint32_t)x.ring || !x.gathered) return;      // (no `gathered` word: a rollout -- slab k % ring was consumed by the policy pass of step k - ring + 1, which every episode is long past)
  const uint32_t need = k - (uint32_t)x.ring + 1u;
  if (seen >= need) return;
  seen = __hip_atomic_load(x.gathered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (seen >= need) return;
  if (__hip_atomic_load(x.timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) return;
  // Thousands of waves polling one uncached word starve the very write they wait for (tools/micro/ring_protocol.hip: a saturated chip
  // of spinning pollers took 57 us per exchange step instead of < 16): the interval between two polls of a wave doubles from ~3 us to ~50 us.
  const long long w0 = wall_clock64();
  int naps = 1;
  while ((seen = __hip_atomic_load(x.gathered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) < need) {
    for (int i = 0; i < naps; ++i) __builtin_amdgcn_s_sleep(127);
    if (naps < 16) naps <<= 1;
    if (wall_clock64() - w0 > x.wait_ticks || __hip_atomic_load(x.timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) { raise_timeout(x); return; }
  }
}
// One episode's packed row of step k is in memory (the stores that wrote it have drained): counted in the episode's group (a partition of
// the persistent kernel: part_of(e, RunArgs.G); 32 neighbouring episodes of the multi-step kernels: xchg_group32(e) -- cc4_sched.h), slot k % ring.  A no-return agent-scope atomic: the wave
// does not wait for it.  (r05 on the way here: one system-scope counter per step -- 8192 atomics on one word serialise at ~12 ns each,
// twice the step --, then two levels with the group's last episode adding the group to it -- two dependent atomics, ~2 us per item.)
__device__ __forceinline__ void xchg_count(const XchgArgs& x, uint32_t k, int group) {
  (void)__hip_atomic_fetch_add(x.gcnt + (size_t)group * (size_t)x.ring + (k % (uint32_t)x.ring), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The hand-off of the plain multi-step loops, every block looping over the K steps of ITS episode e.  xchg_step_out: by the block's first wave, behind the
// drain of step k (s_waitcnt vmcnt(0), barrier) -- the row of step k - 1 is in memory by now (this step's drain covered its store) and is counted; this
// step's row goes out through store_row(its place in slab k % ring): from a byte row in LDS (store_packed_row) or read back from the int32 row
// (pack_row_from_obs), nothing waited for.  WAIT: the slab must be free -- its previous occupant, step k - ring, gathered -- and is checked here, by the
// one wave that writes it (a loop that does not ask for it has checked at the top of the step).  xchg_last_out: on leaving, the last row drained and counted.
template <bool WAIT, class StoreRow>
__device__ __forceinline__ void xchg_step_out(const XchgArgs& x, int n, int e, int k, uint32_t& seen, StoreRow store_row) {
  if (threadIdx.x == 0) { if (k > 0) xchg_count(x, (uint32_t)(k - 1), xchg_group32(e)); if (WAIT) xchg_wait_slab(x, (uint32_t)k, seen); }
  store_row(x.slab + ((size_t)(k % x.ring) * (size_t)n + (size_t)e) * OBS_PACKED);
}
__device__ __forceinline__ void xchg_last_out(const XchgArgs& x, int e, int K) {
  if (x.slab && K > 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0) xchg_count(x, (uint32_t)(K - 1), xchg_group32(e));
  }
}
// Monitor's end-turn roll-over of the hosts' event bytes, four hosts per lane (monitor_roll4): the watched-hosts byte masks of the 35 words
struct MonitorWatchTab { uint32_t v[(MAXH + 3) / 4]; };
constexpr MonitorWatchTab make_monitor_watch_tab() { MonitorWatchTab t{}; for (int w = 0; w < (MAXH + 3) / 4; ++w) t.v[w] = monitor_watch_mask(w); return t; }
static __device__ const MonitorWatchTab monitor_watch_tab = make_monitor_watch_tab();
__device__ __forceinline__ void monitor_roll_all(EnvState* s, int lane) {
  static_assert((MAXH + 3) / 4 <= WAVE && offsetof(EnvState, hev) % 4 == 0, "one pass of the wave over aligned words");
  if (lane < (MAXH + 3) / 4) {
    uint32_t* const w = reinterpret_cast<uint32_t*>(s->hev) + lane;
    *w = monitor_roll4(*w, monitor_watch_tab.v[lane]);
  }
}
// The observation values that can change with every step: position, source byte and mask of value v = obs_fast_entry(v) (cc4_engine.h), as a table the
// compiler fills (one copy per translation unit, 1.5 KB of constant memory that the vector L1 keeps).  Until r06 the entries were computed per value and
// step (r03 A/B: a dozen shifts and multiplies beat one load while the kernels waited on memory, not on the vector unit); at 24 waves per CU the step is
// bound by vector issue slots and those instructions were a sixth of it (profiles/r06_valu_phases.txt: 453 of 2 689 per episode-step).
// Device entry: byte position in the vector (4 x index, 12 bits) | byte offset of the source byte in the staged row << 12 (hev[] and msg[][] both live in
// the agent part, below 8 KB) | bit mask << 25 (the event masks are nibbles), so that a value is one LDS byte read, an and, a compare and a store.
struct ObsFastTab { uint32_t v[OBS_FAST]; };
constexpr ObsFastTab make_obs_fast_tab() {
  ObsFastTab t{};
  for (int v = 0; v < OBS_FAST; ++v) {
    const uint32_t e = obs_fast_entry(v), src = (e >> 10) & 0xFFu;
    const uint32_t off = src < (uint32_t)MAXH ? (uint32_t)offsetof(EnvState, hev) + src : (uint32_t)offsetof(EnvState, msg) + (src - (uint32_t)MAXH);
    t.v[v] = ((e & 0x3FFu) << 2) | (off << 12) | ((e >> 18) << 25);
  }
  return t;
}
static_assert(offsetof(EnvState, hev) + MAXH <= 8192 && offsetof(EnvState, msg) + NBLUE * MSG_LEN <= 8192, "source offsets fit 13 bits");
static_assert((EV_CUR_PROC | EV_OLD_PROC | EV_CUR_CONN | EV_OLD_CONN) < 128 && OBS_TOTAL * 4 <= 4096, "mask and byte position fit their fields");
static __device__ const ObsFastTab obs_fast_tab = make_obs_fast_tab();
// msgs_clean: the message values ([224, 384) of the enumeration) need no rewrite -- no agent sent a message with this step nor with the step before, whose
// encode wrote their zeros (the persistent kernels know that of every step of a launch but the first: cc4_run_random_steps carries no messages)
template <int nt>
__device__ __forceinline__ void encode_obs_fast(const EnvState* s, int32_t* o, uint8_t* obs_bytes, bool pack, int t, bool msgs_clean = false) {
  constexpr int NV = (OBS_FAST + nt - 1) / nt;
  constexpr int K_MSG = (224 + nt - 1) / nt;             // rounds from this one on hold message values only
  constexpr bool EXACT = OBS_FAST % nt == 0;             // one wave: 6 x 64 values, no lane is ever out of range
  const uint32_t tt = (uint32_t)t;
  __builtin_assume(tt < (uint32_t)nt);
  uint32_t ent[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) { const uint32_t v = tt + (uint32_t)(k * nt); ent[k] = (EXACT || v < (uint32_t)OBS_FAST) ? obs_fast_tab.v[v] : 0u; }   // NV independent loads, one wait
  const uint8_t* const row = reinterpret_cast<const uint8_t*>(s);
  char* const ob = reinterpret_cast<char*>(o);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const uint32_t v = tt + (uint32_t)(k * nt);
    if (!EXACT && v >= (uint32_t)OBS_FAST) continue;
    if (k >= K_MSG && msgs_clean) continue;              // (wave-uniform)
    const uint32_t byte = row[(ent[k] >> 12) & 0x1FFFu];
    const int val = (byte & (ent[k] >> 25)) != 0 ? 1 : 0;
    const uint32_t pos = ent[k] & 0xFFFu;
    *reinterpret_cast<int32_t*>(ob + pos) = val;
    if (pack) obs_bytes[pos >> 2] = (uint8_t)val;
  }
}
// The slowly varying observation values by kind, one wave (env_flat_obs_sorted's enumeration: 63 blocked bits, 63 comms-policy bits, 63 subnet one-hots,
// 5 phase words -- one pass of the wave each): `dirty` = what the step changed (EnvState.obs_dirty: OD_BLOCKS, OD_PHASE), OD_ALL after a reset or when the
// caller's buffer is new (the one-hots never change otherwise)
__device__ __forceinline__ void encode_obs_slow(const EnvState* s, int32_t* o, uint32_t dirty, int lane) {
  if (!dirty) return;
  auto put = [&](int v) { int i; const int val = env_flat_obs_sorted(s, v, &i); o[i] = val; };
  if ((dirty & OD_BLOCKS) && lane < 63) put(OBS_FAST + lane);
  if (dirty & OD_PHASE) { if (lane < 63) put(OBS_FAST + 63 + lane); if (lane < 5) put(OBS_FAST + 189 + lane); }
  if ((dirty & ~(uint32_t)(OD_BLOCKS | OD_PHASE)) && lane < 63) put(OBS_FAST + 126 + lane);
}
// CybORG.set_seed (env.py:316-325) applied to one episode: a fresh generator for the controller, the state and the hosts; the agents'
// policies keep the old one until the next reset (EnvCold.rng2); the episode itself stays as it is.  k_set_seed and the reseed of
// k_copy_episodes.
__device__ __forceinline__ void episode_set_seed(EnvState* s, EnvCold* c, uint64_t seed, int rng_mode) {
  if (rng_mode == 0) {        // numpy stream: the agents' policies stay on the stream they were created with (see EnvCold.rng2)
    if (!s->rng_split) c->rng2 = s->rng;
    s->rng_split = 1;
  }
  rng_seed(&s->rng, seed, (uint32_t)rng_mode);
  if (rng_mode == 1) { rng_begin_episode(&s->rng); rng_park(&s->rng); }   // counter mode: the words a reset leaves behind
}
// ---- the counter-mode scenario generation on the NT threads of a block (thread t): the phases of env_reset_counter_mode (cc4_engine.h, which walks them
// serially for the oracle) with a barrier behind each but the last, which is the caller's: thread 0 first stores what the call site publishes of the new
// episode (reward, done), then the block meets -- the row cleared by all threads, the topology on thread 0, the hosts on threads, pid
// uniqueness in the reference's order and the agents on thread 0 (once per episode), the pid bitmaps cleared, the hosts' sessions on threads, the
// rest on thread 0.  ws = the pid work area, [RESET_WS_WORDS] in LDS or memory; continue_stream: a new episode on the same key (CybORG.reset(seed=None)),
// `seed` unused.  RNG_COPY: thread 0 walks the main reset stream on a copy in registers across the phases (the in-kernel regenerations; k_reset
// walks it in place).
template <int NT, bool RNG_COPY>
__device__ __forceinline__ void reset_counter_mode_block(EnvState* s, HostDyn* const hd, EnvCold* const cold_e, StepWork* const work, const int t, uint32_t* const ws,
                                                         const uint64_t seed, const bool continue_stream, const int steps, const int policy, const uint32_t topo) {
  reset_zero(s, hd, cold_e, t, NT);
  __syncthreads();
  Rng rr; ResetCarry carry; carry.env_key = 0;
  Ctx xm{s, cold_e, RNG_COPY ? &rr : &s->rng, hd, work};
  if (t == 0) {
    if (RNG_COPY) { rr = s->rng; rr.mode = 1; }
    carry = reset_topology<1>(xm, seed, steps, continue_stream, policy, topo, ws, RNG_COPY, ResetHostLater{});
  }
  __syncthreads();
  Rng rh; rng_fork(&rh, &s->rng, ST_GEN_HOST); rh.mode = 1;
  Ctx xh{s, cold_e, &rh, hd, work};
  if constexpr (NT >= MAXH) { if (t < MAXH) reset_gen_host<1>(xh, t); } else { for (int h = t; h < MAXH; h += NT) reset_gen_host<1>(xh, h); }
  __syncthreads();
  if (t == 0) { reset_pid_serial(xm, reset_used_set(s)); reset_agents(xm); }
  __syncthreads();
  reset_used_clear(s, t, NT);
  __syncthreads();
  if constexpr (NT >= MAXH) { if (t < MAXH) reset_host_sessions(xh, t); } else { for (int h = t; h < MAXH; h += NT) reset_host_sessions(xh, h); }
  __syncthreads();
  if (t == 0) reset_finish(xm, carry, steps, topo, RNG_COPY);
}
