// cc4_api_rollout.hip -- the host side of libcc4.so: rollouts with the policy in the loop (cc4_rollout_begin .. cc4_rollout_end).
// (The functions of the C ABI take their linkage from their declarations in include/cc4.h and include/cc4_debug.h.)
#include "cc4_host.h"

// ---- rollouts with the policy in the loop (include/cc4.h).  ONE launch of the persistent kernel per k-step rollout; the caller's policy
// runs between the steps on the caller's stream, one policy group of episodes at a time, ordered against the stepping through device words only.
static int rollout_ready(cc4_handle* h, const char* who) {
  if (h->rollout_k <= 0) { h->err = std::string(who) + ": no rollout is in flight (cc4_rollout_begin)"; return -2; }
  return 0;
}
int cc4_rollout_begin(cc4_handle* h, int32_t k) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (h->rollout_k > 0) { h->err = "cc4_rollout_begin: a rollout is in flight (cc4_rollout_end)"; return -2; }
  if (k <= 0 || k > ROLLOUT_MAX_K) { h->err = "cc4_rollout_begin: 1 .. 2^20 steps"; return -2; }
  if (h->cfg.rng_mode != 1 || h->comm || h->evlog_on || h->ext_seen || h->d_prof) { h->err = "cc4_rollout_begin: for counter-mode handles without a communicator, event log, submitted red / green actions or recorded reward terms (cc4_enable_reward_terms)"; return -2; }
  if (h->persist_state == 0) { if (persist_setup(h)) return -1; }
  if (h->persist_state != 1) { h->err = "cc4_rollout_begin: this handle has no persistent kernel (a batch the chip holds at once, or a device picture the schedule refuses): step it with cc4_step_device"; return -2; }
  if (join_groups(h)) return -1;
  h->prev_valid = false;
  const size_t n = (size_t)h->cfg.num_envs, row = n * OBS_PACKED;
  if (!h->d_ract) {
    if (dev_alloc(h, &h->d_ract, 2 * n * NBLUE * sizeof(int32_t)) || dev_alloc(h, &h->d_rready, (size_t)CC4_SLOTS * 32 * sizeof(uint32_t)) ||
        dev_alloc(h, &h->d_rcnt, (size_t)h->run_P * RPG_MAX * cc4_handle::XRING * sizeof(uint32_t)) || dev_alloc(h, &h->d_rfail, sizeof(uint32_t))) return -1;
    for (int g = 0; g < RPG_MAX; ++g) if (new_stream(h, &h->gpolicy[g])) return -1;
    h->policy_stream = h->gpolicy[0];
    if (new_event(h, &h->rev, hipEventDisableTiming)) return -1;
    if (const char* v = getenv("CC4_ROLLOUT_WATCHDOG_MS")) h->rollout_watchdog_ms = atoi(v) > 0 ? atoi(v) : 2000;
    if (const char* v = getenv("CC4_ROLLOUT_MARGIN")) h->rollout_margin = atoi(v) >= 0 ? atoi(v) : 1;
    if (const char* v = getenv("CC4_ROLLOUT_GROUPS")) { h->rpg = atoi(v); if (h->rpg < 1) h->rpg = 1; if (h->rpg > RPG_MAX) h->rpg = RPG_MAX; }
  }
  if (!h->d_xslab && dev_alloc(h, &h->d_xslab, row * cc4_handle::XRING)) return -1;
  if (!h->d_xflags && dev_alloc(h, &h->d_xflags, 2 * sizeof(uint32_t))) return -1;
  if (ensure_watchdog_word(h)) return -1;
  *h->h_xtimeout = 0;
  HIPCHK(h, hipMemsetAsync(h->d_xflags, 0, 2 * sizeof(uint32_t), h->stream));
  // (debug, CC4_ROLLOUT_PREPUBLISH=1: every pass counts as published from the start -- what the stepping itself costs in a rollout, without the waits)
  HIPCHK(h, hipMemsetAsync(h->d_rready, getenv("CC4_ROLLOUT_PREPUBLISH") ? 0x7F : 0, (size_t)h->run_P * 32 * sizeof(uint32_t), h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_rcnt, 0, (size_t)h->run_P * RPG_MAX * cc4_handle::XRING * sizeof(uint32_t), h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_rfail, 0, sizeof(uint32_t), h->stream));
  // what the first policy pass reads: the observations as they stand, packed into the slab in front of step 0's
  hipLaunchKernelGGL(k_pack_obs_rows, dim3((unsigned)n), dim3(WAVE), 0, h->stream, h->d_xslab + (size_t)(cc4_handle::XRING - 1) * row, h->d_obs, (int)n);
  HIPCHK(h, hipEventRecord(h->rev, h->stream));
  StepArgs a = step_args(h);
  a.full_obs = h->full_obs_next ? 1 : 0;
  XchgArgs x{h->d_xslab, nullptr, h->d_xflags + 1, cc4_handle::XRING, 0, h->d_rcnt, h->d_xtimeout};
  // this parity's ticket lines start from zero.  A rollout counts in words 0 .. PG-1 of its lines and its last tickets clear the same words of the
  // other parity; a one-launch call counts in word 0 and clears only word 0.  So behind a rollout and an odd number of one-launch calls, words
  // 1 .. PG-1 of this parity still hold the earlier rollout's final counts: its groups would look handed out (a smaller k) or name steps the
  // progress words never reach (a larger k).  (The one-launch calls keep their memset-free hand-over: a rollout is the rare call.)
  HIPCHK(h, hipMemsetAsync(h->d_pool + (size_t)h->pool_parity * CC4_SLOTS * TK_STRIDE, 0, (size_t)h->run_P * TK_STRIDE * sizeof(uint32_t), h->stream));
  if (persist_launch(h, a, k, 0u, x, nullptr, nullptr, true)) return -1;
  HIPCHK(h, hipGetLastError());
  h->stat_steps += k;
  h->full_obs_next = false;
  h->main_ahead = h->ngroups > 1;
  h->rollout_k = k;
  return 0;
}
int cc4_rollout_groups(cc4_handle* h, int32_t* groups, int32_t* block) {
  if (h->persist_state == 0) { HIPCHK(h, hipSetDevice(h->cfg.device_id)); if (persist_setup(h)) return -1; }
  *groups = h->rpg; *block = h->run_P > 0 ? h->run_P : h->cus;
  return 0;
}
int cc4_rollout_obs_packed(cc4_handle* h, int32_t j, const uint8_t** d_rows) {
  if (!h->d_xslab || !h->d_ract) { h->err = "cc4_rollout_obs_packed: no rollout was begun on this handle"; return -2; }      // (also behind cc4_rollout_end: the ring keeps the last 32 steps)
  if (j < 0) { h->err = "cc4_rollout_obs_packed: step out of range"; return -2; }
  *d_rows = h->d_xslab + (size_t)((j + cc4_handle::XRING - 1) % cc4_handle::XRING) * (size_t)h->cfg.num_envs * OBS_PACKED;
  return 0;
}
int cc4_rollout_actions(cc4_handle* h, int32_t j, int32_t** d_actions) {
  if (!h->d_ract) { h->err = "cc4_rollout_actions: no rollout was begun on this handle"; return -2; }
  *d_actions = h->d_ract + (size_t)(j & 1) * (size_t)h->cfg.num_envs * NBLUE;
  return 0;
}
int cc4_rollout_policy_stream(cc4_handle* h, void** hip_stream) {
  if (!h->policy_stream) { h->err = "cc4_rollout_policy_stream: no rollout was begun on this handle"; return -2; }
  *hip_stream = h->policy_stream;
  return 0;
}
int cc4_rollout_wait_obs(cc4_handle* h, int32_t g, int32_t j, void* hip_stream) {
  if (rollout_ready(h, "cc4_rollout_wait_obs")) return -2;
  if (g < 0 || g >= h->rpg || j < 0 || j >= h->rollout_k) { h->err = "cc4_rollout_wait_obs: group or step out of range"; return -2; }
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->gpolicy[g];
  if (j == 0) { HIPCHK(h, hipStreamWaitEvent(st, h->rev, 0)); return 0; }
  hipLaunchKernelGGL(k_rollout_gate, dim3(1), dim3(WAVE), 0, st, h->d_rcnt, h->run_P, h->rpg, (int)cc4_handle::XRING, (int)g, (int)((j - 1) % cc4_handle::XRING), h->cfg.num_envs,
                     (long long)h->rollout_watchdog_ms * wall_khz(h), h->d_rfail);
  HIPCHK(h, hipGetLastError());
  return 0;
}
int cc4_rollout_sync(cc4_handle* h, int32_t pub_g, int32_t pub_j, int32_t gate_g, int32_t gate_j, void* hip_stream);
int cc4_rollout_publish(cc4_handle* h, int32_t g, int32_t j, void* hip_stream) {
  if (rollout_ready(h, "cc4_rollout_publish")) return -2;
  if (g < 0 || g >= h->rpg || j < 0 || j >= h->rollout_k) { h->err = "cc4_rollout_publish: group or step out of range"; return -2; }
  return cc4_rollout_sync(h, g, j, -1, 0, hip_stream);       // (a one-wave kernel: the word is published once per CU partition)
}
int cc4_rollout_sync(cc4_handle* h, int32_t pub_g, int32_t pub_j, int32_t gate_g, int32_t gate_j, void* hip_stream) {
  if (rollout_ready(h, "cc4_rollout_sync")) return -2;
  if (pub_g >= h->rpg || gate_g >= h->rpg || (pub_g >= 0 && (pub_j < 0 || pub_j >= h->rollout_k)) || (gate_g >= 0 && (gate_j < 0 || gate_j >= h->rollout_k))) { h->err = "cc4_rollout_sync: group or step out of range"; return -2; }
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->gpolicy[gate_g >= 0 ? gate_g : (pub_g >= 0 ? pub_g : 0)];
  if (gate_g >= 0 && gate_j == 0) { HIPCHK(h, hipStreamWaitEvent(st, h->rev, 0)); gate_g = -1; }      // (the observations as they stood: behind the event)
  if (pub_g < 0 && gate_g < 0) return 0;
  hipLaunchKernelGGL(k_rollout_sync, dim3(1), dim3(WAVE), 0, st, h->d_rready, (int)pub_g, (uint32_t)(pub_j + 1), h->d_rcnt, h->run_P, h->rpg, (int)cc4_handle::XRING, (int)gate_g,
                     (int)(gate_g >= 0 ? (gate_j - 1) % cc4_handle::XRING : 0), h->cfg.num_envs, (long long)h->rollout_watchdog_ms * wall_khz(h), h->d_rfail);
  HIPCHK(h, hipGetLastError());
  return 0;
}
int cc4_rollout_random_policy(cc4_handle* h, int32_t g, int32_t j, uint64_t seed0, uint32_t t, void* hip_stream) {
  if (rollout_ready(h, "cc4_rollout_random_policy")) return -2;
  if (g < 0 || g >= h->rpg || j < 0 || j >= h->rollout_k) { h->err = "cc4_rollout_random_policy: group or step out of range"; return -2; }
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->gpolicy[g];
  const int tot = h->cfg.num_envs * NBLUE;
  const int grp = pgroup_threads(h->cfg.num_envs, h->run_P, h->rpg) * NBLUE;      // threads over the group's episodes (whole blocks of P), one per agent
  hipLaunchKernelGGL(k_rollout_random_policy, dim3((grp + WAVE - 1) / WAVE), dim3(WAVE), 0, st, h->d_ract + (size_t)(j & 1) * (size_t)tot, h->cfg.num_envs, h->run_P, h->rpg, (int)g, seed0, t);
  HIPCHK(h, hipGetLastError());
  return 0;
}
int cc4_rollout_hash_policy(cc4_handle* h, int32_t g, int32_t j, void* hip_stream) {
  if (rollout_ready(h, "cc4_rollout_hash_policy")) return -2;
  if (g < 0 || g >= h->rpg || j < 0 || j >= h->rollout_k) { h->err = "cc4_rollout_hash_policy: group or step out of range"; return -2; }
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : h->gpolicy[g];
  const int n = h->cfg.num_envs;
  const uint8_t* rows = h->d_xslab + (size_t)((j + cc4_handle::XRING - 1) % cc4_handle::XRING) * (size_t)n * OBS_PACKED;
  const int grp = pgroup_threads(n, h->run_P, h->rpg);
  hipLaunchKernelGGL(k_rollout_hash_policy, dim3((grp + WAVE - 1) / WAVE), dim3(WAVE), 0, st, h->d_ract + (size_t)(j & 1) * (size_t)n * NBLUE, rows, n, h->run_P, h->rpg, (int)g, (uint32_t)j);
  HIPCHK(h, hipGetLastError());
  return 0;
}
int cc4_rollout_end(cc4_handle* h) {
  if (rollout_ready(h, "cc4_rollout_end")) return -2;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  h->rollout_entering = true;
  const hipError_t e1 = hipStreamSynchronize(h->stream);
  hipError_t e2 = hipSuccess;
  for (int g = 0; g < RPG_MAX; ++g) { const hipError_t e = hipStreamSynchronize(h->gpolicy[g]); if (e != hipSuccess) e2 = e; }
  h->rollout_entering = false;
  const int k = h->rollout_k;
  h->rollout_k = 0;
  HIPCHK(h, e1); HIPCHK(h, e2);
  uint32_t gate_failed = 0;
  HIPCHK(h, hipMemcpy(&gate_failed, h->d_rfail, sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (*reinterpret_cast<volatile uint32_t*>(h->h_xtimeout) || gate_failed) {
    // a wave whose progress wait ran into the watchdog left its item unrun (persist_loop): progress words short of the call's end, tickets never
    // drawn and so the other parity's lines never cleared.  The schedule's counters start over, as at its setup.
    HIPCHK(h, hipMemsetAsync(h->d_pool, 0, 2 * (size_t)CC4_SLOTS * TK_STRIDE * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_run, 0, h->run_words * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pool_base = 0; h->pool_parity = 0;
    h->err = "cc4_rollout_end: a step of the " + std::to_string(k) + "-step rollout waited longer than " + std::to_string(h->rollout_watchdog_ms) +
             " ms for its actions (or a policy gate for its observations): not every group's policy pass of every step was published -- the episodes were "
             "stepped with whatever the action slots held (CC4_ROLLOUT_WATCHDOG_MS)";
    return -6;
  }
  return 0;
}
// A whole rollout with a stand-in policy (0: random indices, 1: hash of the observations), driven from here: begin, the passes of all steps -- two
// stream operations each (cc4_rollout_sync, the policy kernel) --, end.  What bench.py times as `policy_in_loop`, and what a trainer written against the C ABI would do.
int cc4_rollout_standin(cc4_handle* h, int32_t k, int32_t policy, uint64_t seed0, uint32_t t0) {
  int rc = cc4_rollout_begin(h, k);
  if (rc) return rc;
  // every policy group has a stream and a chain of its own: [publish of its pass of step j - 1 + gate of step j] -> policy of step j -> ...
  for (int j = 0; j < k && !rc; ++j)
    for (int g = 0; g < h->rpg && !rc; ++g) {
      rc = cc4_rollout_sync(h, j > 0 ? g : -1, j - 1, g, j, nullptr);
      if (!rc) rc = policy == 0 ? cc4_rollout_random_policy(h, g, j, seed0, t0 + (uint32_t)j, nullptr) : cc4_rollout_hash_policy(h, g, j, nullptr);
    }
  for (int g = 0; g < h->rpg && !rc; ++g) rc = cc4_rollout_sync(h, g, k - 1, -1, 0, nullptr);
  const int end = cc4_rollout_end(h);
  return rc ? rc : end;
}
