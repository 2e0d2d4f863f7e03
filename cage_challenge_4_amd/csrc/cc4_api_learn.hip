// cc4_api_learn.hip -- the host side of libcc4.so: the learner's pure functions, which read no row of the batch at all -- log-probabilities of stored
// actions with gradients (include/cc4.h; the kernels: cc4_k_logp.hip; the definition: cc4_logp.h), and the advantages and returns of a stored rollout
// (cc4_k_gae.hip; cc4_gae.h).  Pure functions of the caller's tensors: no handle and so no entry prologue, no stream of the library's -- one launch
// on the caller's stream on the device current to the calling thread (autograd's backward thread is as good as any).  Every one has the same
// definition on the host.  (The sampling itself reads the hot rows: a view, cc4_api_views.hip.)
#include "cc4_host.h"
#include "cc4_logp.h"
#include "cc4_gae.h"

// one launch on the caller's stream: 0, or -1 if it failed
template <class... Params, class... Args> static int launch_on(void* stream, void (*kernel)(Params...), int64_t blocks, int threads, Args... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), 0, static_cast<hipStream_t>(stream), args...);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// ---- the learner's half of the sampling: log-probability and entropy of stored actions under new logits, and their derivative.  -2 with nothing
// enqueued: a null pointer, n < 0, a dtype outside 1..3, a temperature that is not finite and positive; n == 0 a no-op; -1: the launch failed.
static bool logp_bad(int32_t dtype, int32_t n, float temperature) { return !dtype_ok(dtype) || n < 0 || !temperature_ok(temperature); }
static int64_t logp_blocks(int32_t n) { return ((int64_t)n + LP_WAVES - 1) / LP_WAVES; }
int cc4_logp_actions_device(void* stream, const void* d_logits, int32_t dtype, const uint8_t* d_mask, const int32_t* d_actions, int32_t n, float temperature,
                            float* d_aux, int32_t* d_fault) {
  if (!d_logits || !d_mask || !d_actions || !d_aux || !d_fault || logp_bad(dtype, n, temperature)) return -2;
  if (n == 0) return 0;
  return launch_on(stream, k_logp_fwd, logp_blocks(n), LP_WAVES * WAVE, d_logits, (int)dtype, d_mask, d_actions, (int)n, 1.0f / temperature, d_aux, d_fault);
}
int cc4_logp_actions_grad_device(void* stream, const void* d_logits, int32_t dtype, const uint8_t* d_mask, const int32_t* d_actions, int32_t n,
                                 float temperature, const float* d_aux, const float* d_g, void* d_grad) {
  if (!d_logits || !d_mask || !d_actions || !d_aux || !d_g || !d_grad || logp_bad(dtype, n, temperature)) return -2;
  if (n == 0) return 0;
  return launch_on(stream, k_logp_bwd, logp_blocks(n), LP_WAVES * WAVE, d_logits, (int)dtype, d_mask, d_actions, (int)n, 1.0f / temperature, d_aux, d_g,
                   d_grad);
}
// ... and on the host, one row of float32 logits: the number of refused agents (0 .. 5), or -2; the derivative 0 or -2.  No device.
int cc4_logp_actions_host(const float* logits, const uint8_t* mask, const int32_t* actions, float temperature, float* aux) {
  if (!logits || !mask || !actions || !aux || logp_bad(3, 0, temperature)) return -2;
  return logp_from_row(logits, mask, actions, 1.0f / temperature, aux);
}
int cc4_logp_actions_grad_host(const float* logits, const uint8_t* mask, const int32_t* actions, float temperature, const float* aux, const float* g,
                               float* grad) {
  if (!logits || !mask || !actions || !aux || !g || !grad || logp_bad(3, 0, temperature)) return -2;
  logp_grad_from_row(logits, mask, actions, 1.0f / temperature, aux, g, grad);
  return 0;
}

// ---- advantages, returns and loss weights of a stored rollout (cc4_gae.h; cc4_k_gae.hip).  As the log-probabilities: a pure function of the
// caller's tensors, no handle, no prologue, one launch on the caller's stream.  -2 with nothing enqueued: a null required pointer or gae_bad;
// T == 0 or N == 0 a no-op; -1: the launch failed.
int cc4_gae_device(void* stream, const float* d_rewards, int32_t reward_heads, const void* d_values, int32_t dtype, const void* d_last, const uint8_t* d_dones,
                   const uint8_t* d_done0, const int32_t* d_actions, int32_t T, int32_t N, int32_t A, float gamma, float lambda, int32_t flags, float* d_adv,
                   float* d_ret, uint8_t* d_weight) {
  if (!d_rewards || !d_values || !d_last || !d_dones || !d_adv || !d_ret || !dtype_ok(dtype) || gae_bad(reward_heads, T, N, A, gamma, lambda, flags))
    return -2;
  if (T == 0 || N == 0) return 0;
  const int64_t cols = (int64_t)N * A, per_block = (int64_t)GAE_WAVES * WAVE;
  const GaeArgs a{d_rewards, d_values, d_last, d_dones, d_done0, d_actions, d_adv, d_ret, d_weight, reward_heads, dtype, T, N, A, flags, gamma, lambda};
  return launch_on(stream, k_gae, (cols + per_block - 1) / per_block, GAE_WAVES * WAVE, a);
}
// ... and on the host, float32 values; no device
int cc4_gae_host(const float* rewards, int32_t reward_heads, const float* values, const float* last, const uint8_t* dones, const uint8_t* done0,
                 const int32_t* actions, int32_t T, int32_t N, int32_t A, float gamma, float lambda, int32_t flags, float* adv, float* ret, uint8_t* weight) {
  if (!rewards || !values || !last || !dones || !adv || !ret || gae_bad(reward_heads, T, N, A, gamma, lambda, flags)) return -2;
  gae_columns(rewards, reward_heads, values, last, dones, done0, actions, T, N, A, gamma, lambda, flags, adv, ret, weight);
  return 0;
}
int32_t cc4_gae_rows(void) { return GAE_ROWS; }
