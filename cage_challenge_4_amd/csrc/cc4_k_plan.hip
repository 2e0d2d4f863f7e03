// cc4_k_plan.hip -- cc4_run_plan_device: the plan build of the persistent counter-mode kernel, k_run_philox1p, and the small kernels around a plan call
// (k_plan_collect: the per-step form's trajectory row; k_plan_finish: the call's error words; k_unpack_rows: cc4_unpack_rows_device).  Same schedule
// (cc4_persist.h) and step body (cc4_philox1_body.h) as k_run_philox1, which is not touched: the PLAN flag exists in this entry and in k_run_pcgp only.
#include "cc4_philox1_body.h"
#include "cc4_persist.h"

// k steps of the batch in one launch with the blue actions of step j from row j of a plan the caller wrote before the launch (PlanArgs): no exchange,
// no rollout protocol -- nothing outside the kernel is waited for.  Register budget as k_run_philox1 (six waves per SIMD).
__global__ __launch_bounds__(WAVE, CC4_PERSIST_MINW) void k_run_philox1p(StepArgs a, RunArgs ra, PlanArgs pl) { persist_loop<false, false, false, true>(a, ra, XchgArgs{}, pl); }

// The per-step form of a plan call, behind every step's launch (one block per episode): the step's reward / done into the trajectory's row, its packed
// observation row from the int32 row (a kernel boundary lies between the step and this read), its error word OR-ed into the call's.
__global__ __launch_bounds__(WAVE) void k_plan_collect(int n, const EnvState* st, const int32_t* obs, const float* reward, const uint8_t* done, const uint32_t* err,
                                                       float* row_reward, uint8_t* row_done, uint8_t* row_packed, uint32_t* err_or) {
  const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (e >= n) return;
  if (row_packed) pack_row_from_obs(row_packed + (size_t)e * OBS_PACKED, obs + (size_t)e * OBS_TOTAL, lane);
  if (lane == 0) {
    if (row_reward) row_reward[e] = reward[e];
    if (row_done) row_done[e] = done[e];
    const uint32_t f = err[e] | (st[e].step_count == 0 ? PLAN_REGEN : 0u);
    if (f) err_or[e] |= f;
  }
}
// Behind a plan call's last step: the flags any step raised into the handle's error words (a regeneration inside the plan clears the row's word; the
// caller must still see what the single steps would have shown), the call's word zeroed for the next call; the one-launch form wrote reward / done of
// the last step into the trajectory only -- copied into the handle's buffers here.
// An episode some step regenerated (autoreset) has a new scenario: its mask-stale mark makes the next cc4_policy_outputs rebuild its action-mask row.
__global__ void k_plan_finish(int n, uint32_t* err, uint32_t* err_or, uint8_t* mask_stale, float* reward, const float* last_reward, uint8_t* done, const uint8_t* last_done) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= n) return;
  const uint32_t f = err_or[e];
  if (f) { err[e] |= f & ~PLAN_REGEN; err_or[e] = 0u; if (f & PLAN_REGEN) mask_stale[e] = 1; }
  if (last_reward) reward[e] = last_reward[e];
  if (last_done) done[e] = last_done[e];
}

// cc4_unpack_rows_device: packed observation rows -> [rows][578] values in the caller's dtype (0 uint8, 1 float16, 2 bfloat16, 3 float32).  One lane
// per packed byte (four values), grid-stride over rows * OBS_PACKED bytes; every value is 0, 1 or 2, so every dtype is exact.
template <int DT> __device__ __forceinline__ void unpack_put(void* out, size_t i, uint32_t v) {
  if constexpr (DT == 0) reinterpret_cast<uint8_t*>(out)[i] = (uint8_t)v;
  else if constexpr (DT == 3) reinterpret_cast<float*>(out)[i] = (float)v;
  else {      // float16 (0, 1, 2, 3 -> 0x0000 0x3C00 0x4000 0x4200) / bfloat16 (-> 0x0000 0x3F80 0x4000 0x4040)
    constexpr uint64_t tab = DT == 1 ? 0x420040003C000000ull : 0x404040003F800000ull;
    reinterpret_cast<uint16_t*>(out)[i] = (uint16_t)(tab >> (16 * v));
  }
}
template <int DT> __global__ __launch_bounds__(256) void k_unpack_rows(const uint8_t* __restrict__ packed, void* __restrict__ out, long long rows) {
  const size_t total = (size_t)rows * OBS_PACKED, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const size_t r = i / OBS_PACKED; const int j = (int)(i - r * OBS_PACKED);
    const uint32_t b = packed[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) if (4 * j + k < OBS_TOTAL) unpack_put<DT>(out, r * OBS_TOTAL + (size_t)(4 * j + k), (b >> (2 * k)) & 3u);
  }
}
template __global__ void k_unpack_rows<0>(const uint8_t*, void*, long long);
template __global__ void k_unpack_rows<1>(const uint8_t*, void*, long long);
template __global__ void k_unpack_rows<2>(const uint8_t*, void*, long long);
template __global__ void k_unpack_rows<3>(const uint8_t*, void*, long long);
