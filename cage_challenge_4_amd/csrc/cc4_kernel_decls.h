// cc4_kernel_decls.h -- the kernels of libcc4.so as the host side (cc4_api*.hip) sees them: declarations only; each is defined -- and, where it is a
// template, explicitly instantiated -- in the translation unit cc4_kernels.h names.
#pragma once
#include "cc4_args.h"
#include "cc4_gae.h"

constexpr int PT = 4 * WAVE;       // threads per episode block of the four-wave kernels (cc4_k_philox4.hip: PW = 4)
// per-step kernels
template <bool LOG> __global__ void k_step(StepArgs a);
template <bool LOG, int MINW> __global__ void k_step_philox(StepArgs a);
template <bool LOG> __global__ void k_step_philox1(StepArgs a);
extern template __global__ void k_step<false>(StepArgs);
extern template __global__ void k_step<true>(StepArgs);
extern template __global__ void k_step_philox<false, 1>(StepArgs);
extern template __global__ void k_step_philox<false, 7>(StepArgs);
extern template __global__ void k_step_philox<false, 8>(StepArgs);
extern template __global__ void k_step_philox<true, 1>(StepArgs);
extern template __global__ void k_step_philox1<false>(StepArgs);
extern template __global__ void k_step_philox1<true>(StepArgs);
// one-launch kernels
__global__ void k_run_philox(StepArgs a, int K, uint32_t t0, XchgArgs x);
__global__ void k_run_philox8(StepArgs a, int K, uint32_t t0, XchgArgs x);
__global__ void k_run_philox1m(StepArgs a, int K, uint32_t t0, XchgArgs x);
__global__ void k_run_philox1(StepArgs a, RunArgs ra);      // the headline build: in-kernel action draw only (persist_launch)
__global__ void k_run_philox1g(StepArgs a, RunArgs ra, XchgArgs x);      // the same schedule with every run-time flag (cc4_k_run1g.hip)
__global__ void k_run_philox1x(StepArgs a, RunArgs ra, XchgArgs x);
__global__ void k_run_philox1r(StepArgs a, RunArgs ra, XchgArgs x);
__global__ void k_run_pcg(StepArgs a, RunArgs ra, XchgArgs x);
// cc4_run_plan_device (cc4_k_plan.hip; k_run_pcgp: cc4_k_pcg.hip)
__global__ void k_run_philox1p(StepArgs a, RunArgs ra, PlanArgs pl);
__global__ void k_run_pcgp(StepArgs a, RunArgs ra, PlanArgs pl);
__global__ void k_plan_collect(int n, const EnvState* st, const int32_t* obs, const float* reward, const uint8_t* done, const uint32_t* err,
                               float* row_reward, uint8_t* row_done, uint8_t* row_packed, uint32_t* err_or);
__global__ void k_plan_finish(int n, uint32_t* err, uint32_t* err_or, uint8_t* mask_stale, float* reward, const float* last_reward, uint8_t* done, const uint8_t* last_done);
template <int DT> __global__ void k_unpack_rows(const uint8_t* __restrict__ packed, void* __restrict__ out, long long rows);
extern template __global__ void k_unpack_rows<0>(const uint8_t*, void*, long long);
extern template __global__ void k_unpack_rows<1>(const uint8_t*, void*, long long);
extern template __global__ void k_unpack_rows<2>(const uint8_t*, void*, long long);
extern template __global__ void k_unpack_rows<3>(const uint8_t*, void*, long long);
// reset and helpers (cc4_k_misc.hip)
__global__ void k_reset(ResetArgs a);
__global__ void k_xchg_gate(uint32_t* gcnt, int ring, int groups, int n, int P, int k_lo, int k_hi, long long ticks, uint32_t* fail, int max_naps);
__global__ void k_discover(int32_t* count, long long ticks);
__global__ void k_random_actions(int32_t* actions, int n, uint64_t seed0, uint32_t t, int e0 = 0);
__global__ void k_spin(long long cycles);
__global__ void k_unpack_obs(const uint8_t* __restrict__ packed, uint8_t* __restrict__ out, int rows);
__global__ void k_policy_outputs(const EnvState* __restrict__ st, const int32_t* __restrict__ obs, const float* __restrict__ reward,
                                 const uint8_t* __restrict__ done, const uint32_t* __restrict__ err, int n, int ep_blocks, int dtype,
                                 void* __restrict__ out_obs, uint8_t* __restrict__ out_mask, float* __restrict__ out_reward,
                                 uint8_t* __restrict__ out_done, int32_t* __restrict__ out_err, uint8_t* __restrict__ mask_stale);
// episode copies (cc4_k_copy.hip): phase 1 claims the destinations, phase 2 copies the live extents
__global__ void k_copy_claim(CopyArgs a);
__global__ void k_copy_episodes(CopyArgs a);
// state features (cc4_k_feat.hip): one wavefront per requested episode or bank slot
__global__ void k_state_features(FeatArgs a);
// the red agents as learners (cc4_k_red.hip): submitted red actions into the handle's records, one lane per (episode, agent); the agents' view, one
// wavefront per requested episode or bank slot
__global__ void k_red_submit(RedSubmitArgs a);
__global__ void k_red_view(RedViewArgs a);
// blue's own knowledge (cc4_k_blue.hip): one wavefront per requested episode or bank slot
__global__ void k_blue_view(BlueViewArgs a);
// the Monitor's connections as edge lists (cc4_k_edges.hip): one wavefront per requested episode or bank slot
__global__ void k_blue_edges(BlueEdgesArgs a);
// reward terms (cc4_k_reward.hip): one wavefront per requested episode or bank slot
__global__ void k_reward_terms(RewardArgs a);
// masked sampling of the blue actions from policy logits (cc4_k_sample.hip): one wavefront per requested episode or bank slot
__global__ void k_sample_actions(SampleArgs a);
// log-probability and entropy of stored blue actions, and their derivative (cc4_k_logp.hip): one wavefront per row of the caller's tensors,
// LP_WAVES rows per workgroup (measured: profiles/r29_logp.txt; make EXTRA=-DCC4_LOGP_WAVES=k builds another)
#ifndef CC4_LOGP_WAVES
#define CC4_LOGP_WAVES 4
#endif
constexpr int LP_WAVES = CC4_LOGP_WAVES;
__global__ void k_logp_fwd(const void* __restrict__ logits, int dtype, const uint8_t* __restrict__ mask, const int32_t* __restrict__ actions, int n,
                           float inv_t, float* __restrict__ aux, int32_t* __restrict__ fault);
__global__ void k_logp_bwd(const void* __restrict__ logits, int dtype, const uint8_t* __restrict__ mask, const int32_t* __restrict__ actions, int n,
                           float inv_t, const float* __restrict__ aux, const float* __restrict__ g, void* __restrict__ grad);
// advantages and returns of a stored rollout (cc4_k_gae.hip): one lane per column of the caller's tensors, GAE_WAVES wavefronts per workgroup,
// the rows in blocks of GAE_ROWS.  Measured (profiles/r31_gae.txt): 16 rows ahead beat 8 and 4 at T >= 128 (the kernel waits on memory, one wave
// per SIMD), 24 and 32 spill scalar registers and lose at T = 20; 1, 2 and 4 waves per workgroup are within 2 % of each other at 8192 episodes,
// one is the fastest at 1024; make EXTRA="-DCC4_GAE_WAVES=k -DCC4_GAE_ROWS=r" builds another
#ifndef CC4_GAE_WAVES
#define CC4_GAE_WAVES 1
#endif
#ifndef CC4_GAE_ROWS
#define CC4_GAE_ROWS 16
#endif
constexpr int GAE_WAVES = CC4_GAE_WAVES, GAE_ROWS = CC4_GAE_ROWS;
__global__ void k_gae(GaeArgs a);
// per-episode opponent classes (cc4_k_misc.hip): one lane per episode
__global__ void k_set_policies(EnvState* st, const int8_t* __restrict__ red, const int8_t* __restrict__ green, const int8_t* __restrict__ blue, int n, uint32_t* fault);
__global__ void k_get_policies(const EnvState* __restrict__ st, int8_t* __restrict__ live, int8_t* __restrict__ assigned, int n);
__global__ void k_set_seed(EnvState* st, EnvCold* cold, size_t cold_row, const uint64_t* seeds, int n, int rng_mode);
__global__ void k_set_rng_state(EnvState* st, const uint64_t* w, int n);
__global__ void k_rng_state(const EnvState* st, uint64_t* out, int n);
__global__ void k_rollout_gate(uint32_t* cnt, int P, int PG, int ring, int g, int slot, int n, long long ticks, uint32_t* fail);
__global__ void k_rollout_sync(uint32_t* ready, int pub_g, uint32_t pub_val, uint32_t* cnt, int P, int PG, int ring, int g, int slot, int n, long long ticks, uint32_t* fail);
__global__ void k_rollout_random_policy(int32_t* act, int n, int P, int PG, int g, uint64_t seed0, uint32_t t);
__global__ void k_rollout_hash_policy(int32_t* act, const uint8_t* packed, int n, int P, int PG, int g, uint32_t j);
__global__ void k_pack_obs_rows(uint8_t* packed, const int32_t* obs, int n);
__global__ void k_digest(const EnvState* st, const EnvCold* cold, size_t cold_row, const int32_t* obs, const float* reward,
                         const uint8_t* done, const uint32_t* err, const int32_t* actions, uint64_t* out, int n);
extern "C" __global__ void k_set_evlog(EnvCold* cold, size_t row_bytes, int n, uint32_t on);
extern "C" __global__ void k_copy_evlog(EnvCold* dst, const EnvCold* src, size_t row_bytes, int n);
// the numpy-stream kernels' jump table (cc4_k_pcg.hip)
hipError_t cc4_upload_pcg_tables();
