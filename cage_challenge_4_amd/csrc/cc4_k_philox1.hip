// cc4_k_philox1.hip -- counter mode, one wavefront per episode: k_step_philox1<LOG> and the multi-step k_run_philox1m.  See cc4_kernels.h.
#include "cc4_philox1_body.h"

template <bool LOG>
__global__ __launch_bounds__(WAVE, CC4_LEAN_MINW) void k_step_philox1(StepArgs a) {
  const int e = a.e0 + (int)blockIdx.x;
  if (e >= a.n) return;
  philox1_body<LOG, false>(a, e, a.rand_t, 0u, (int)threadIdx.x);
}
// The plain multi-step form of the one-wave kernel: one wave per episode, every wave loops over the K steps of ITS episode -- no
// tickets, no affinity: a wave only reads what it wrote itself.  For batches one launch holds at once (cc4_create; CC4_RUN1=0/1
// overrides): more waves than residency slots would simply start as slots free up (8192 episodes: 5120 at once, the other 3072
// behind them on a chip that is no longer full).
__global__ __launch_bounds__(WAVE, 5) void k_run_philox1m(StepArgs a, int K, uint32_t t0, XchgArgs x) {
  a.prof = nullptr; a.obs8 = nullptr; a.ext = nullptr;
  const int e = (int)blockIdx.x;
  uint32_t seen = 0;
  for (int k = 0; k < K; ++k) {
    if (x.slab) {
      if (threadIdx.x == 0) xchg_wait_slab(x, (uint32_t)k, seen);
      __syncthreads();
    }
    int lane_i = (int)threadIdx.x;
    asm volatile("" : "+v"(lane_i));
    philox1_body<false, true>(a, e, t0 + (uint32_t)k, (uint32_t)k, lane_i, k == 0, k == K - 1);      // the agent part stays in LDS from the first step to the last
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // this step's row is read back from the int32 row (the slab was waited for at the top of the step)
    if (x.slab) xchg_step_out<false>(x, a.n, e, k, seen, [&](uint8_t* row) { pack_row_from_obs(row, a.obs + (size_t)e * OBS_TOTAL, (int)threadIdx.x); });
  }
  xchg_last_out(x, e, K);
}

// the kernels the host side launches (cc4_kernel_decls.h)
template __global__ void k_step_philox1<false>(StepArgs);
template __global__ void k_step_philox1<true>(StepArgs);
