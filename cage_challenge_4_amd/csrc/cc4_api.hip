// cc4_api.hip -- the host side of libcc4.so, its core: create / destroy (what a handle allocates, here or in any other unit, is registered with its
// owner -- cc4_host.h dev_alloc .. release -- and cc4_destroy releases the list), the prologue of every entry point (enter), the episode groups and
// their streams (join_groups, fork_groups), the launches of one step (launch_step), reset, the step entry points and the getters (copy_to_host),
// episode copies, state get / set, the event log and the replay.  The handle itself: cc4_host.h; k steps
// per call: cc4_api_run.hip; rollouts: cc4_api_rollout.hip; the communicator and the exchange: cc4_api_comm.hip; the derived views: cc4_api_views.hip;
// debug hooks: cc4_api_debug.hip.
#include "cc4_host.h"
#include "cc4_export.h"

static thread_local std::string g_create_err;
// the handles that exist (shadow handles among them) and the call-local device blocks (DevTemp): what cc4_debug_live_resources counts
static std::mutex g_handles_mu;
static std::vector<cc4_handle*> g_handles;
std::atomic<int64_t> g_scoped_blocks{0};

// The ROCm runtime multiplexes HIP streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and two streams that share a
// queue run their kernels one after the other.  Three launches per step fit the default; a fourth stream needs more queues
// (measured, r03 profiles/r03_hwq_sweep.txt: 8192 episodes, 3 / 4 launches per step: 715 / 445 M with 4 queues, 717 / 742 M with
// 8).  The variable is read when the runtime initialises, so it is set when this library is loaded (never overriding the
// user's choice) -- and whether the four streams of a handle really run side by side is measured on those very streams when the
// handle is created, not assumed (streams_run_concurrently): a process that initialised HIP earlier, or one whose other streams
// already occupy the queues (a second handle next to a busy first one), keeps three launches per step.
__attribute__((constructor)) static void cc4_runtime_env() { setenv("GPU_MAX_HW_QUEUES", "16", 0); }

// 1 if kernels launched on the n given streams at the same time run side by side, 0 if some of them share a hardware queue and
// run one after the other (or the probe failed).  ~1 ms.
static int streams_run_concurrently(hipStream_t* st, int n) {
  if (n < 2) return 1;
  int khz = 100000, dev = 0;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev);
  if (khz <= 0) khz = 100000;
  const long long ticks = 300LL * khz / 1000;            // 300 us per kernel
  bool ok = true;
  double one = 0, all = 0;
  for (int pass = 0; pass < 2 && ok; ++pass) {             // pass 0: one stream (also warms the kernel up), pass 1: all of them
    const int m = pass ? n : 1;
    auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < m; ++i) hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, st[i], ticks);
    for (int i = 0; i < m && ok; ++i) ok = hipStreamSynchronize(st[i]) == hipSuccess;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    (pass ? all : one) = us;
  }
  return ok && all < 1.5 * (one > 300.0 ? one : 300.0);
}

// The red / green / blue policy choice of a configuration as the kernels read it (StepArgs.policy, ResetArgs.policy).
static int policy_bits(const cc4_config& c) {
  return (c.red_policy & 3) | (c.green_policy ? GP_SLEEP_BIT : 0) | (c.green_policy == 2 ? GP_OPEN_BIT : 0) | (c.blue_policy ? BP_RANDOM_BIT : 0);
}
// The part of a step launch's arguments that every launch of a handle shares: its rows and outputs, its configuration.  Everything else is zero /
// null, and a call site sets what is particular to it by field name (inputs, the fused action draw, full_obs, obs8, prof, ext).
StepArgs step_args(const cc4_handle* h) {
  StepArgs a{};
  a.st = h->d_state; a.cold = h->d_cold;
  a.obs = h->d_obs; a.reward = h->d_reward; a.done = h->d_done; a.err = h->d_err;
  a.n = h->cfg.num_envs; a.autoreset = h->cfg.autoreset; a.steps = h->cfg.steps; a.rng_mode = h->cfg.rng_mode;
  a.policy = policy_bits(h->cfg);
  a.topo = (uint32_t)h->cfg.topology_seed;
  a.reset_ws = h->d_reset_ws;
  return a;
}
// The same for the persistent kernels' RunArgs of a k-step call: the schedule's tables and the runs its k steps are cut into (run_split, cc4_sched.h).
// persist_launch sets by name what is per call: the ticket counters' parity, base, the rollout's fields, the timeline.
// head: the call launches the headline kernel k_run_philox1 (persist_launch decides) -- only that one takes the long-call pattern of run_config_for_call:
// the builds with the exchange hold a run against the ring of step slabs (run_config_for_call's comment), and the others keep the split they were measured with.
RunArgs run_args(const cc4_handle* h, int k, uint32_t t0, bool head) {
  RunArgs ra{};
  ra.progress = h->d_run; ra.slot_part = h->d_slot_part;
  ra.P = h->run_P; ra.K = k; ra.G = h->run_G; ra.t0 = t0;
  memcpy(ra.xcc_lo, h->xcc_lo, 8); memcpy(ra.xcc_n, h->xcc_n, 8);
  ra.thr = h->run_thr;
  ra.runs = head ? run_split_for_call(k, h->run_SA, h->run_SB, h->run_nB, h->run_single)      // (a long call with no CC4_PERSIST_RUNS given: run_config_for_call's pattern)
                 : run_split(k, h->run_SA, h->run_SB, h->run_nB, h->run_single);
  return ra;
}

// How a step of this handle is cut into launches, and which build of the counter-mode kernel they run (the kernels are
// chosen from what one LAUNCH puts on a CU and from what the whole batch does).
void configure_groups(cc4_handle* h, int ng) {
  const int n = h->cfg.num_envs, cus = h->cus;
  if (ng < 1) ng = 1;
  if (ng > cc4_handle::MAX_GROUPS) ng = cc4_handle::MAX_GROUPS;
  if (ng > n) ng = n;
  h->ngroups = ng;
  for (int g = 0; g <= ng; ++g) h->glo[g] = (int)(((long long)n * g) / ng);
  const int gsize = (n + ng - 1) / ng;                                 // episodes per launch
  const int bpc = (gsize + cus - 1) / cus;                             // episode blocks of one launch per CU
  const int bpc_all = (n + cus - 1) / cus;                             // ... of all launches of a step
  // four-wave kernel: one round of <= 5 blocks per CU runs the unconstrained build; else the build whose residency fills whole
  // rounds best (exactly 8 per CU -- 2048 episodes on 256 CUs -- is one round of the 8-block build)
  h->philox_minw = bpc <= 5 ? 1 : (bpc == 8 ? 8 : 7);
  // ... and with several launches per step what counts is what they put on a CU together (r03 profiles: three launches, register
  // budget 1 / 7 / 8: 1024 episodes 176 / 174 / 164 M, 2048: 295 / 302 / 278, 4096: 355 / 442 / 417)
  // (r04 flags, four launches: 1536 episodes 269 / 266 / 257, 2048: 329 / 333 / 323, 3072: 364 / 433 / 423, 4096: 369 / 471 / 490 -- one wave: 507)
  if (ng > 1) h->philox_minw = bpc_all <= 6 ? 1 : 7;
  if (const char* v = getenv("CC4_PHILOX_MINW")) h->philox_minw = atoi(v);   // tuning override: 1, 7 or 8
  // The one-wave-per-episode build when a single launch puts more than eight episodes on a CU, or the launches of a step
  // together more than thirteen.  Measured on MI355X (M agent-env steps/s, four waves / one wave per episode; r02, one launch per
  // step): 1024 episodes 168 / 131, 2048: 262 / 238, 2304: 249 / 260, 3072: 294 / 322, 4096: 319 / 395, 8192: 391 / 510;
  // (r03, three launches per step): 1024: 175 / 137, 2048: 295 / 249, 3072: 347 / 345, 4096: 442 / 422, 6144: 455 / 556,
  // 8192: 466 / 659.  (The same kernel with the host table in LDS as well is no faster anywhere.)
  // (after the r03 changes to the one-wave kernel -- event bytes staged, rows on cache-line boundaries -- with four launches per
  // step: 2048 episodes 312 / 276, 3072: 401 / 388, 4096: 442 / 487, 5120: 453 / 560, 6144: 458 / 627)
  h->philox_lean = bpc > 8 || bpc_all > 13;
  if (const char* v = getenv("CC4_PHILOX_LEAN")) h->philox_lean = atoi(v) != 0;   // tuning / test override
}

// Every API call other than the step launches works on the main stream: order it behind whatever the group streams still
// hold (device-side waits, no host synchronisation), and remember that the next step launches must be ordered behind it.
int join_groups(cc4_handle* h) {
  // (nearly every entry point comes through here: while a rollout's kernel is running the handle's rows and streams are its alone)
  if (h->rollout_k > 0 && !h->rollout_entering) { h->err = "a rollout is in flight on this handle: cc4_rollout_end first"; return -1; }
  if (h->ngroups > 1) {
    if (h->groups_busy) {
      for (int g = 1; g < h->ngroups; ++g) {
        HIPCHK(h, hipEventRecord(h->gev[g], h->gstream[g]));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->gev[g], 0));
      }
      h->groups_busy = false;
    }
    h->main_ahead = true;
    h->joined_between = true;
  }
  return 0;
}
// ... and the other direction, in front of launches on the group streams: they start behind what the main stream holds (an upload, a reset, a launch
// of the whole batch).  The one place that records mev.
int fork_groups(cc4_handle* h) {
  if (h->ngroups > 1 && h->main_ahead) {
    HIPCHK(h, hipEventRecord(h->mev, h->stream));
    for (int g = 1; g < h->ngroups; ++g) HIPCHK(h, hipStreamWaitEvent(h->gstream[g], h->mev, 0));
    h->main_ahead = false;
  }
  return 0;
}
// (a handle with a communicator never has a rollout in flight -- cc4_rollout_begin refuses it -- so the order of the two refusals cannot be observed)
int enter_refused(cc4_handle* h, const char* who, unsigned refuse) {
  if ((refuse & EN_NO_ROLLOUT) && h->rollout_k > 0) { h->err = std::string(who) + ": a rollout is in flight on this handle: cc4_rollout_end first"; return -2; }
  if ((refuse & EN_NO_COMM) && h->comm) { h->err = std::string(who) + ": not on a handle with a communicator"; return -2; }
  return 0;
}
int enter(cc4_handle* h, const char* who, unsigned refuse) {
  if (int rc = enter_refused(h, who, refuse)) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return join_groups(h) ? -1 : 0;
}
// `bytes` from the device to the caller's memory behind everything the handle holds, and the wait for it (0 bytes: the wait alone)
int copy_to_host(cc4_handle* h, const char* who, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (int rc = enter(h, who)) return rc;
  if (bytes) HIPCHK(h, hipMemcpyAsync(dst, src, bytes, kind, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
int sync_all(cc4_handle* h) {
  // (!groups_busy: whatever the group streams were given, the main stream already waits for -- join_groups, or the joined end of
  // cc4_run_random_steps -- and a host wait on an idle stream is not free: ~8 us each inside a short timed region)
  for (int g = h->ngroups - 1; g >= 1; --g) if (h->groups_busy) HIPCHK(h, hipStreamSynchronize(h->gstream[g]));
  // (a query first: behind a call that ended with a synchronisation of its own -- cc4_run_random_steps -- the stream is idle, and asking is cheaper than waiting)
  if (hipStreamQuery(h->stream) != hipSuccess) { (void)hipGetLastError(); HIPCHK(h, hipStreamSynchronize(h->stream)); }
  h->groups_busy = false;
  h->joined_between = true;
  return 0;
}

// wall_clock64 ticks per millisecond (the constant 100 MHz reference clock): asked once per handle
int wall_khz(cc4_handle* h) {
  if (h->khz <= 0) { int khz = 100000; (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->cfg.device_id); h->khz = khz > 0 ? khz : 100000; }
  return h->khz;
}
// the pinned host word a kernel raises when one of its waits gives up (XchgArgs.timeout_host), and its device address
int ensure_watchdog_word(cc4_handle* h) {
  if (!h->h_xtimeout) {
    if (pin_alloc(h, &h->h_xtimeout, sizeof(uint32_t))) return -1;
    HIPCHK(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_xtimeout), h->h_xtimeout, 0));
  }
  return 0;
}

// rand: draw the blue actions inside the step kernel from (seed0, t) and record them in the handle's action buffer
// one group's launch of a step: the kernel cc4_create picked for this handle, on the group's stream, carrying `start` / `stop` as the
// launch's own timing events (or null)
void launch_group(cc4_handle* h, StepArgs a, int g, bool full, hipEvent_t start, hipEvent_t stop) {
  launch_range(h, a, h->glo[g], h->glo[g + 1], h->gstream[g], full, start, stop);
}
void launch_range(cc4_handle* h, StepArgs a, int e0, int e1, hipStream_t st, bool full, hipEvent_t start, hipEvent_t stop) {
  a.e0 = e0; a.n = e1; a.dbg_stop = h->dbg_stop;
  if (h->dbg_stop) a.full_obs = 0;     // (a restored batch would get every observation value rewritten: the measurement wants the steady-state encode)
  const size_t lds1 = offsetof(EnvState, hd);     // one-wave kernels: the agent part
  const dim3 grid(a.n - a.e0);
  if (h->cfg.rng_mode == 1) {
    if (h->philox_lean) {
      if (full || h->d_prof || (h->dbg_stop && !getenv("CC4_DEBUG_STOP_FAST"))) hipExtLaunchKernelGGL(k_step_philox1<true>, grid, dim3(WAVE), lds1, st, start, stop, 0, a);
      else hipExtLaunchKernelGGL(k_step_philox1<false>, grid, dim3(WAVE), lds1, st, start, stop, 0, a);
    }
    else if (full) hipExtLaunchKernelGGL((k_step_philox<true, 1>), grid, dim3(PT), sizeof(EnvState), st, start, stop, 0, a);
    else if (h->philox_minw == 8) hipExtLaunchKernelGGL((k_step_philox<false, 8>), grid, dim3(PT), sizeof(EnvState), st, start, stop, 0, a);
    else if (h->philox_minw == 7) hipExtLaunchKernelGGL((k_step_philox<false, 7>), grid, dim3(PT), sizeof(EnvState), st, start, stop, 0, a);
    else hipExtLaunchKernelGGL((k_step_philox<false, CC4_SMALL_MINW>), grid, dim3(PT), sizeof(EnvState), st, start, stop, 0, a);
  } else {
    if (full || h->d_prof) hipExtLaunchKernelGGL(k_step<true>, grid, dim3(WAVE), lds1, st, start, stop, 0, a);
    else hipExtLaunchKernelGGL(k_step<false>, grid, dim3(WAVE), lds1, st, start, stop, 0, a);
  }
}

// api_step: one of the step entry points (cc4_step / _ex / _fetch / _device), as opposed to the loop of cc4_run_random_steps.  When the caller did
// something with the WHOLE batch since the last step (an upload, a fetch, a policy kernel over all observations: anything that went through
// join_groups or waited for the streams), the groups cannot run ahead of each other anyway -- a launch per group then pays a fork and a join
// across streams per step for nothing: ONE launch on the main stream (8192 episodes, k_random_actions + cc4_step_device per step: 334 -> 583 M;
// a loop of cc4_step_device with nothing in between keeps the groups and their overlap across steps).
int launch_step(cc4_handle* h, const int32_t* d_actions, const uint8_t* d_msgs, bool rand, uint64_t seed0,
                       uint32_t t, bool ext_uploaded, bool api_step) {
  if (h->ext_seen && h->ext_dirty && !ext_uploaded) {     // this step submits no red / green action: every record says so
    if (join_groups(h)) return -1;
    HIPCHK(h, hipMemsetAsync(h->d_ext, 0xFF, (size_t)h->cfg.num_envs * EXT_PER_ENV * sizeof(ExtAct), h->stream));
    h->ext_dirty = false; h->ext_green_dirty = false;
  }
  const bool full = h->evlog_on || h->ext_seen;
  // the byte-observation buffer about to be overwritten may still be read by an overlapped all-gather
  int buf = h->comm ? (h->obs_buf + 1) % cc4_handle::OBS_RING : 0;
  if (h->comm && h->gather_seq[buf] > h->gathers_waited) {
    // the last all-gather that read this buffer must be complete; wait for a slightly newer one (the communication stream is
    // in order), so the next OBS_WAIT_EVERY-1 launches need no wait of their own -- but never for the newest one, which is
    // the one meant to overlap this step
    long long q = h->gather_seq[buf] + cc4_handle::OBS_WAIT_EVERY - 1;
    if (q > h->gathers_issued - 1) q = h->gathers_issued - 1;
    if (q < h->gather_seq[buf]) q = h->gather_seq[buf];
    // waited for by the host, not by the stream: the all-gather in question is several steps old and normally complete, and
    // a wait packet in the compute queue costs stream time whether or not it has to wait
    hipError_t qs = hipEventQuery(h->ev_comm[q % cc4_handle::OBS_RING]);
    if (qs == hipErrorNotReady) { h->gather_stalls++; HIPCHK(h, hipEventSynchronize(h->ev_comm[q % cc4_handle::OBS_RING])); }
    else HIPCHK(h, qs);
    h->gathers_waited = q;
  }
  const bool whole = api_step && h->whole_batch_steps && h->ngroups > 1 && h->joined_between && !h->groups_busy && !h->comm;
  h->joined_between = false;
  if (!whole && fork_groups(h)) return -1;   // e.g. an action upload or a reset on the main stream: the group streams start behind it
  if (h->keep_prev) {      // the rows as they stand before this step (cc4_replay_logged); a small handle: one launch per step, main stream
    const size_t n = (size_t)h->cfg.num_envs;
    HIPCHK(h, hipMemcpyAsync(h->d_prev_state, h->d_state, n * sizeof(EnvState), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_prev_cold, h->d_cold, n * h->cold_row, hipMemcpyDeviceToDevice, h->stream));
    h->prev_actions = d_actions; h->prev_msgs = d_msgs; h->prev_full_obs = h->full_obs_next; h->prev_ext = h->ext_seen;
    h->prev_valid = !rand;
  }
  StepArgs a = step_args(h);
  a.actions = d_actions; a.msgs = d_msgs;
  a.obs8 = h->comm ? h->d_obs8[buf] : nullptr;
  a.rand_out = rand ? h->d_actions : nullptr; a.rand_seed0 = seed0; a.rand_t = t;
  a.full_obs = h->full_obs_next ? 1 : 0;
  a.prof = h->d_prof;
  a.ext = h->ext_seen ? h->d_ext : nullptr;
  h->full_obs_next = false;
  if (whole) {
    hipEvent_t stop = h->tev_stop[0], start = h->tev_start[0];
    for (int g = 0; g < h->ngroups; ++g) h->tev_start[g] = h->tev_stop[g] = nullptr;
    // (fewer waves per CU so that the batch runs in whole rounds -- 8192 episodes: 16 per CU, two even rounds instead of 1.6 at 20 -- is slower at every
    // residency tried: 578 M at 20, 567 at 18, 538 at 16, 503 at 14; tools/ab/ab_whole_residency.sh)
    launch_range(h, a, 0, h->cfg.num_envs, h->stream, full, start, stop);
    HIPCHK(h, hipGetLastError());
    h->step_event_attached = false;
    h->main_ahead = true;            // (the group streams have not been ordered behind this launch)
    h->obs_buf = buf;
    return 0;
  }
  for (int g = 0; g < h->ngroups; ++g) {
    // with a communicator, the launch carries ev_step[buf][g] as its stop event: the event rides on the kernel's own completion
    // signal, where a separate hipEventRecord would put a marker packet between two step kernels (~5 us of idle stream time)
    hipEvent_t stop = h->comm ? h->ev_step[buf][g] : h->tev_stop[g];
    hipEvent_t start = h->comm ? nullptr : h->tev_start[g];        // timing rides on the kernels' own signals too: no marker packets
    h->tev_start[g] = h->tev_stop[g] = nullptr;
    launch_group(h, a, g, full, start, stop);
    HIPCHK(h, hipGetLastError());
  }
  h->step_event_attached = h->comm != nullptr;
  if (h->ngroups > 1) h->groups_busy = true;
  h->obs_buf = buf;
  h->obs8_from_slab = -1;           // (this step's packed rows are in the ring buffer it wrote)
  return 0;
}

extern "C" {

const char* cc4_last_error(cc4_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }
size_t cc4_state_bytes(void) { return sizeof(EnvState); }
int cc4_device_count(void) { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }
size_t cc4_algorithmic_bytes_per_env_step(void) {
  // state row in + out, flat obs out (int32), actions in, reward + done + err out (DESIGN.md "algorithmic bytes")
  return 2 * sizeof(EnvState) + 4 * OBS_TOTAL + 4 * NBLUE + 4 + 1 + 4;
}
size_t cc4_hot_bytes(void) { return offsetof(EnvState, hd); }
const char* cc4_step_kernel(cc4_handle* h) {
  if (!h) return "";
  if (h->cfg.rng_mode != 1) return "k_step";
  return h->philox_lean ? "k_step_philox1" : "k_step_philox";
}

// the kernel cc4_run_random_steps launches on this handle as it stands (no communicator, no event log): the step kernel, once per
// step and group -- or one of the one-launch forms
const char* cc4_run_kernel(cc4_handle* h) {
  if (!h) return "";
  const bool plain = (!h->comm || h->xchg_on) && !h->evlog_on && !h->ext_seen && !h->d_prof && !h->dbg_stop;
  if (plain && h->multistep) return h->multistep_minb == 8 ? "k_run_philox8" : "k_run_philox";
  if (plain && h->run1m) return "k_run_philox1m";
  if (plain && h->persist_state >= 0) return h->cfg.rng_mode == 0 ? "k_run_pcg" : (h->comm ? "k_run_philox1x" : "k_run_philox1");      // (calls of fewer than persist_min_k steps: the per-step launches)
  return cc4_step_kernel(h);
}
const char* cc4_run_kernel_for(cc4_handle* h, int32_t k) {
  if (!h) return "";
  // (the persistent kernel's discovery pass runs on first use: asking which kernel a call of k steps will launch is such a use -- the answer depends on it,
  // and a caller that asks before its timed region keeps it out of that region)
  if (h->persist_state == 0 && !h->run1m && !h->multistep && (!h->comm || h->xchg_on) && !h->evlog_on && !h->ext_seen && !h->d_prof && k >= h->persist_min_k && hipSetDevice(h->cfg.device_id) == hipSuccess) (void)persist_setup(h);
  const char* r = cc4_run_kernel(h);
  if (k < 2) return cc4_step_kernel(h);
  if (!h->multistep && !h->run1m && h->persist_state >= 0 && k < h->persist_min_k) return cc4_step_kernel(h);
  return r;
}

int cc4_create(const cc4_config* cfg, cc4_handle** out) {
  if (!cfg || !out || cfg->num_envs <= 0 || cfg->steps <= 0 || cfg->red_policy < 0 || cfg->red_policy > 3 ||
      cfg->green_policy < 0 || cfg->green_policy > 2 || cfg->blue_policy < 0 || cfg->blue_policy > 1 || cfg->rng_mode < 0 || cfg->rng_mode > 1) { g_create_err = "cc4_create: bad config"; return -2; }
  if (cfg->topology_seed != 0 && cfg->rng_mode != 1) { g_create_err = "cc4_create: topology_seed needs rng_mode 1 (the numpy stream draws scenario and dynamics from one generator)"; return -2; }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_err = "cc4_create: no HIP device available (libcc4 has no CPU fallback)";
    return -3;
  }
  if (cfg->device_id < 0 || cfg->device_id >= ndev) { g_create_err = "cc4_create: device_id out of range"; return -2; }
  cc4_handle* h = new cc4_handle();
  h->cfg = *cfg;
  *out = h;
  { std::lock_guard<std::mutex> lk(g_handles_mu); g_handles.push_back(h); }
  // how a host thread waits for the device is the runtime's default unless CC4_HOST_WAIT=spin|yield|block says otherwise (spinning by default was
  // tried in r06: no measurable gain on a 20-step call, and the exchange's soak test failed once under it); ignored (hipErrorSetOnActiveProcess) when
  // the process has initialised the device some other way already
  if (const char* v = getenv("CC4_HOST_WAIT")) {
    static std::once_flag once;
    std::call_once(once, [v] {
      unsigned flags = hipDeviceScheduleAuto;
      if (!strcmp(v, "spin")) flags = hipDeviceScheduleSpin; else if (!strcmp(v, "yield")) flags = hipDeviceScheduleYield; else if (!strcmp(v, "block")) flags = hipDeviceScheduleBlockingSync;
      (void)hipSetDeviceFlags(flags);
      (void)hipGetLastError();
    });
  }
  HIPCHK(h, hipSetDevice(cfg->device_id));
  if (cc4_upload_pcg_tables() != hipSuccess) { h->err = "cc4_create: the numpy-stream kernel's jump table could not be uploaded"; return -1; }
  {
    hipDeviceProp_t prop;
    HIPCHK(h, hipGetDeviceProperties(&prop, cfg->device_id));
    h->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  }
  {
    // Episode groups (see cc4_handle::ngroups).  Measured on MI355X (r03, profiles/r03_groups_sweep_philox.txt; M agent-env steps/s,
    // counter mode, 1 / 2 / 3 launches per step): 1024 episodes 165 / 173 / 175, 2048: 257 / 289 / 295, 4096: 392 / 413 / 442,
    // 8192: 503 / 629 / 659, 16384: 570 / 710 / 701; numpy stream, 8192 episodes: 272 / 352 / 363.  A fourth stream halves the
    // rate (the runtime's hardware queues), so three it is.  CC4_GROUPS overrides (1 .. 4).
    int ng = cfg->num_envs >= 1024 ? 3 : (cfg->num_envs >= 512 ? 2 : 1);
    // (a fourth launch where four streams really overlap: decided below, once the streams exist)
    h->auto_groups = getenv("CC4_GROUPS") == nullptr;
    if (const char* v = getenv("CC4_GROUPS")) ng = atoi(v);
    configure_groups(h, ng);
  }
  if (new_stream(h, &h->stream)) return -1;
  h->gstream[0] = h->stream;
  for (int g = 1; g < h->ngroups; ++g) {   // only the streams that are used: the runtime spreads streams over few hardware queues
    if (new_stream(h, &h->gstream[g]) || new_event(h, &h->gev[g], hipEventDisableTiming)) return -1;
  }
  if (new_event(h, &h->mev, hipEventDisableTiming) || new_event(h, &h->ev_wait, hipEventDisableTiming) || new_event(h, &h->ev_signal, hipEventDisableTiming)) return -1;
  if (h->auto_groups && h->ngroups == 3) {
    // a fourth launch per step where this handle's four streams really run side by side (8192 episodes 717 -> 742 M, 2048: 310 ->
    // 314 M, 1024: 179 -> 183 M; with two of them on one hardware queue: 445 M)
    if (new_stream(h, &h->gstream[3])) return -1;
    if (streams_run_concurrently(h->gstream, 4)) {
      if (new_event(h, &h->gev[3], hipEventDisableTiming)) return -1;
      configure_groups(h, 4);
    } else release(h, &h->gstream[3]);
  }
  size_t n = (size_t)cfg->num_envs;
  h->cold_row = cold_row_bytes(cfg->steps);
  if (dev_alloc(h, &h->d_state, n * sizeof(EnvState)) || dev_alloc(h, &h->d_cold, n * h->cold_row)) return -1;
  // counter mode: the one-wave kernel's generation work area; numpy stream: the LCG window of the green actions (wave_green_exec), 1 KB per episode
  if (dev_alloc(h, &h->d_reset_ws, cfg->rng_mode == 1 ? n * RESET_WS_WORDS * sizeof(uint32_t) : n * 128 * sizeof(uint64_t))) return -1;
  h->in_bytes = n * NBLUE * sizeof(int32_t) + n * NBLUE * MSG_LEN;
  h->small_io = cfg->num_envs <= cc4_handle::SMALL_IO_ENVS;
  if (const char* v = getenv("CC4_SMALL_IO")) h->small_io = h->small_io && atoi(v) != 0;
  if (h->small_io) {      // (d_actions: the device's name for pin_in -- the owner knows pin_in only; d_obs / pin_out below alike)
    if (pin_alloc(h, &h->pin_in, h->in_bytes)) return -1;
    HIPCHK(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_actions), h->pin_in, 0));
    memset(h->pin_in, 0, h->in_bytes);
  } else if (dev_alloc(h, &h->d_actions, h->in_bytes)) return -1;
  h->d_msgs = reinterpret_cast<uint8_t*>(h->d_actions) + n * NBLUE * sizeof(int32_t);
  if (dev_alloc(h, &h->d_seeds, n * sizeof(uint64_t)) || dev_alloc(h, &h->d_envmask, n)) return -1;
  h->out_bytes = n * OBS_TOTAL * sizeof(int32_t) + n * sizeof(float) + n * sizeof(uint32_t) + n;
  if (h->small_io) {
    if (pin_alloc(h, &h->pin_out, h->out_bytes)) return -1;
    HIPCHK(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->d_obs), h->pin_out, 0));
  } else if (dev_alloc(h, &h->d_obs, h->out_bytes)) return -1;
  h->d_reward = reinterpret_cast<float*>(h->d_obs + n * OBS_TOTAL);
  h->d_err = reinterpret_cast<uint32_t*>(h->d_reward + n);
  h->d_done = reinterpret_cast<uint8_t*>(h->d_err + n);
  if (dev_alloc(h, &h->d_mask, n * MASK_TOTAL) || dev_alloc(h, &h->d_rng, n * 7 * sizeof(uint64_t))) return -1;
  if (dev_alloc(h, &h->d_claim, n * sizeof(uint32_t) + sizeof(uint32_t)) || dev_alloc(h, &h->d_mask_stale, n)) return -1;     // [n] claim words + the fault word
  h->d_copy_fault = h->d_claim + n;
  HIPCHK(h, hipMemsetAsync(h->d_claim, 0, n * sizeof(uint32_t) + sizeof(uint32_t), h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_mask_stale, 0, n, h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_state, 0, n * sizeof(EnvState), h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_cold, 0, n * h->cold_row, h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_obs, 0, n * OBS_TOTAL * sizeof(int32_t), h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_done, 0, n, h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_err, 0, n * sizeof(uint32_t), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (choose_run_form(h, 0)) return -1;
  if (const char* v = getenv("CC4_PERSIST_MIN_K")) h->persist_min_k = atoi(v);
  if (const char* v = getenv("CC4_WHOLE_BATCH_STEPS")) h->whole_batch_steps = atoi(v) != 0;
  if (const char* v = getenv("CC4_PERSIST_VERIFY")) h->verify = atoi(v) != 0;
  if (const char* v = getenv("CC4_PERSIST_VERIFY_EVERY")) h->verify_every = atoi(v) > 0 ? atoi(v) : 0;
  return 0;
}

void cc4_destroy(cc4_handle* h) {
  if (!h) return;
  enq_pool_stop(h);
  (void)hipSetDevice(h->cfg.device_id);
  for (const OwnedList::Entry& e : h->own.entries) if (e.kind == OWN_STREAM && *e.field) (void)hipStreamSynchronize(static_cast<hipStream_t>(*e.field));
  if (h->comm) ncclCommDestroy(h->comm);
  if (h->shadow) { cc4_destroy(h->shadow); h->shadow = nullptr; (void)hipSetDevice(h->cfg.device_id); }
  h->own.release_all();
  { std::lock_guard<std::mutex> lk(g_handles_mu); g_handles.erase(std::remove(g_handles.begin(), g_handles.end(), h), g_handles.end()); }
  delete h;
}
// debug: what the handles of this process (and the call-local blocks of calls in flight) hold -- out[0] device blocks, [1] pinned blocks, [2] events, [3] streams
int cc4_debug_live_resources(int64_t out[4]) {
  if (!out) return -2;
  out[OWN_DEVICE] = g_scoped_blocks.load(); out[OWN_PINNED] = out[OWN_EVENT] = out[OWN_STREAM] = 0;
  std::lock_guard<std::mutex> lk(g_handles_mu);
  for (const cc4_handle* h : g_handles) h->own.count_live(out);
  return 0;
}

// the launch of a reset on the main stream (joined by the caller), from seeds and a mask on the device (either may be null), and its bookkeeping: what
// cc4_reset does behind its uploads and cc4_reset_device on the caller's own pointers
static int reset_launch(cc4_handle* h, const uint64_t* d_seeds, const uint8_t* d_env_mask) {
  ResetArgs a{h->d_state, h->d_cold, d_seeds, d_env_mask, h->d_obs, h->d_reward,
              h->d_done, h->d_err, h->d_mask, h->cfg.num_envs, h->cfg.steps, h->cfg.rng_mode,
              policy_bits(h->cfg), (uint32_t)h->cfg.topology_seed,
              h->comm ? h->d_obs8[h->obs_buf] : nullptr};
  // with a communicator the reset also writes the packed exchange row of its observations into the current ring buffer; an
  // overlapped all-gather may still be reading that buffer
  if (h->comm && h->gathers_issued > h->gathers_waited) { HIPCHK(h, hipStreamSynchronize(h->comm_stream)); h->gathers_waited = h->gathers_issued; }
  if (h->comm && h->obs8_from_slab >= 0) {      // the reset writes the current ring buffer's packed rows itself -- all of them, unless it is masked
    const size_t row = (size_t)h->cfg.num_envs * OBS_PACKED;
    if (d_env_mask) HIPCHK(h, hipMemcpyAsync(h->d_obs8[h->obs_buf], h->d_xslab + (size_t)h->obs8_from_slab * row, row, hipMemcpyDeviceToDevice, h->stream));
    h->obs8_from_slab = -1;
  }
  hipLaunchKernelGGL(k_reset, dim3(h->cfg.num_envs), dim3(WAVE), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  h->prev_valid = false;            // (cc4_replay_logged: no step to repeat)
  h->step_event_attached = false;   // the buffer's event must be recorded again before the next all-gather
  return 0;
}
int cc4_reset(cc4_handle* h, const uint64_t* seeds, const uint8_t* env_mask) {
  if (int rc = enter(h, "cc4_reset")) return rc;
  size_t n = (size_t)h->cfg.num_envs;
  if (seeds) HIPCHK(h, hipMemcpyAsync(h->d_seeds, seeds, n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  if (env_mask) HIPCHK(h, hipMemcpyAsync(h->d_envmask, env_mask, n, hipMemcpyHostToDevice, h->stream));
  if (int rc = reset_launch(h, seeds ? h->d_seeds : nullptr, env_mask ? h->d_envmask : nullptr)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
// cc4_reset on seeds and a mask that are on the device already (a criterion a kernel of the caller's evaluated: env_mask = done): no upload, no host wait
int cc4_reset_device(cc4_handle* h, const uint64_t* d_seeds, const uint8_t* d_env_mask) {
  if (int rc = enter_refused(h, "cc4_reset_device", EN_NO_ROLLOUT)) return rc;
  if (h->comm) { h->err = "cc4_reset_device: not on a handle with a communicator (cc4_reset orders the exchange's buffers through the host)"; return -2; }
  if (reinterpret_cast<uintptr_t>(d_seeds) % 8) { h->err = "cc4_reset_device: the seeds must be 8-byte aligned"; return -2; }
  if (int rc = enter(h, "cc4_reset_device")) return rc;
  return reset_launch(h, d_seeds, d_env_mask);
}

// ---- per-episode opponent classes (include/cc4.h "Mixed opponents in one batch"; the rule: row_assign / row_policies, cc4_state.h).  An assignment
// is a byte of the hot row that only the regenerations read: no step launch needs ordering behind these beyond the main stream's own.
int cc4_set_policies_device(cc4_handle* h, const int8_t* d_red, const int8_t* d_green, const int8_t* d_blue) {
  if (int rc = enter_refused(h, "cc4_set_policies_device", EN_NO_ROLLOUT)) return rc;
  if (!d_red && !d_green && !d_blue) return 0;
  if (int rc = enter(h, "cc4_set_policies_device")) return rc;
  const int n = h->cfg.num_envs;
  hipLaunchKernelGGL(k_set_policies, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_state, d_red, d_green, d_blue, n, h->d_copy_fault);
  HIPCHK(h, hipGetLastError());
  h->prev_valid = false;        // (cc4_replay_logged would repeat a step from rows that have moved on)
  return 0;
}
int cc4_set_policies(cc4_handle* h, const int8_t* red, const int8_t* green, const int8_t* blue) {
  if (int rc = enter_refused(h, "cc4_set_policies", EN_NO_ROLLOUT)) return rc;
  if (!red && !green && !blue) return 0;
  if (int rc = enter(h, "cc4_set_policies")) return rc;
  const size_t n = (size_t)h->cfg.num_envs;
  if (!h->d_pol && dev_alloc(h, &h->d_pol, 6 * n)) return -1;
  const int8_t* src[3] = {red, green, blue};
  const int8_t* dev[3] = {nullptr, nullptr, nullptr};
  for (int c = 0; c < 3; ++c) if (src[c]) { HIPCHK(h, hipMemcpyAsync(h->d_pol + c * n, src[c], n, hipMemcpyHostToDevice, h->stream)); dev[c] = h->d_pol + c * n; }
  if (int rc = cc4_set_policies_device(h, dev[0], dev[1], dev[2])) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));     // (the host arrays may go away once the call returns)
  return 0;
}
int cc4_policies_device(cc4_handle* h, int8_t* d_live, int8_t* d_assigned) {
  if (int rc = enter_refused(h, "cc4_policies_device", EN_NO_ROLLOUT)) return rc;
  if (!d_live && !d_assigned) return 0;
  if (int rc = enter(h, "cc4_policies_device")) return rc;
  const int n = h->cfg.num_envs;
  hipLaunchKernelGGL(k_get_policies, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_state, d_live, d_assigned, n);
  HIPCHK(h, hipGetLastError());
  return 0;
}
int cc4_get_policies(cc4_handle* h, int8_t* live, int8_t* assigned) {
  if (int rc = enter_refused(h, "cc4_get_policies", EN_NO_ROLLOUT)) return rc;
  if (!live && !assigned) return 0;
  if (int rc = enter(h, "cc4_get_policies")) return rc;
  const size_t n = (size_t)h->cfg.num_envs;
  if (!h->d_pol && dev_alloc(h, &h->d_pol, 6 * n)) return -1;
  if (int rc = cc4_policies_device(h, live ? h->d_pol : nullptr, assigned ? h->d_pol + 3 * n : nullptr)) return rc;
  if (live) HIPCHK(h, hipMemcpyAsync(live, h->d_pol, 3 * n, hipMemcpyDeviceToHost, h->stream));
  if (assigned) HIPCHK(h, hipMemcpyAsync(assigned, h->d_pol + 3 * n, 3 * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
// The same definition on one hot row (cc4_get_state, a checkpoint): no device, no handle.
int cc4_row_set_policies(void* hot_row, int red, int green, int blue) {
  if (!hot_row) return -2;
  RowCopy r;      // (the agent part of the row is all the rule reads: no more of the caller's bytes is touched)
  if (!(r.s = static_cast<EnvState*>(row_copy(hot_row, offsetof(EnvState, hd), alignof(EnvState), sizeof(EnvState))))) return -1;
  const bool ok = row_assign(r.s, red, green, blue);
  if (ok) static_cast<uint8_t*>(hot_row)[offsetof(EnvState, assign)] = r.s->assign;
  return ok ? 0 : -2;
}
int cc4_row_get_policies(const void* hot_row, int8_t live[3], int8_t assigned[3]) {
  if (!hot_row) return -2;
  RowCopy r;
  if (!(r.s = static_cast<EnvState*>(row_copy(hot_row, offsetof(EnvState, hd), alignof(EnvState), sizeof(EnvState))))) return -1;
  row_policies(r.s, live, assigned);
  return 0;
}

// the blue actions and messages of a step from the caller's memory into the handle's buffers, on the main stream (either may be null: none given)
static int upload_inputs(cc4_handle* h, const int32_t* actions, const uint8_t* messages) {
  const size_t n = (size_t)h->cfg.num_envs;
  if (actions) HIPCHK(h, hipMemcpyAsync(h->d_actions, actions, n * NBLUE * sizeof(int32_t), hipMemcpyDefault, h->stream));
  if (messages) HIPCHK(h, hipMemcpyAsync(h->d_msgs, messages, n * NBLUE * MSG_LEN, hipMemcpyDefault, h->stream));
  return 0;
}
int cc4_step(cc4_handle* h, const int32_t* actions, const uint8_t* messages) {
  if (int rc = enter(h, "cc4_step")) return rc;
  if (upload_inputs(h, actions, messages)) return -1;
  if (launch_step(h, actions ? h->d_actions : nullptr, messages ? h->d_msgs : nullptr, false, 0, 0, false, true)) return -1;
  return sync_all(h);
}

// the four outputs out of the pinned block (laid out as the device allocation: obs | reward | err | done)
static void unstage_outputs(const cc4_handle* h, int32_t* obs, float* reward, uint8_t* done, uint32_t* err) {
  const size_t n = (size_t)h->cfg.num_envs;
  const size_t b_obs = n * OBS_TOTAL * sizeof(int32_t), b_rew = n * sizeof(float), b_err = n * sizeof(uint32_t);
  if (obs) memcpy(obs, h->pin_out, b_obs);
  if (reward) memcpy(reward, h->pin_out + b_obs, b_rew);
  if (err) memcpy(err, h->pin_out + b_obs + b_rew, b_err);
  if (done) memcpy(done, h->pin_out + b_obs + b_rew + b_err, n);
}
// The outputs of the last step (or reset) in one copy and one host synchronisation: observations, reward, done and error flags live in
// one device allocation.  Batches of up to PIN_MAX_ENVS episodes come through a pinned staging buffer (the copy is a real asynchronous
// DMA; a copy into pageable memory is staged by the runtime, call by call).  Any of the four pointers may be null.
static int fetch_outputs(cc4_handle* h, int32_t* obs, float* reward, uint8_t* done, uint32_t* err) {
  if (join_groups(h)) return -1;
  const size_t n = (size_t)h->cfg.num_envs;
  const size_t b_obs = n * OBS_TOTAL * sizeof(int32_t), b_rew = n * sizeof(float), b_err = n * sizeof(uint32_t);
  if (h->small_io) {                                          // the kernels wrote into pinned host memory: wait, then read it
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unstage_outputs(h, obs, reward, done, err);
    return 0;
  }
  if (h->cfg.num_envs <= PIN_MAX_ENVS) {
    if (!h->pin_out && pin_alloc(h, &h->pin_out, h->out_bytes)) return -1;
    const size_t lo = obs ? 0 : b_obs;                         // (a caller that wants no observations does not pay for them)
    HIPCHK(h, hipMemcpyAsync(h->pin_out + lo, reinterpret_cast<const uint8_t*>(h->d_obs) + lo, h->out_bytes - lo, hipMemcpyDefault, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    unstage_outputs(h, obs, reward, done, err);
    return 0;
  }
  if (obs) HIPCHK(h, hipMemcpyAsync(obs, h->d_obs, b_obs, hipMemcpyDefault, h->stream));
  if (reward) HIPCHK(h, hipMemcpyAsync(reward, h->d_reward, b_rew, hipMemcpyDefault, h->stream));
  if (err) HIPCHK(h, hipMemcpyAsync(err, h->d_err, b_err, hipMemcpyDefault, h->stream));
  if (done) HIPCHK(h, hipMemcpyAsync(done, h->d_done, n, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
int cc4_fetch(cc4_handle* h, int32_t* obs, float* reward, uint8_t* done, uint32_t* err) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return fetch_outputs(h, obs, reward, done, err);
}
// cc4_step + cc4_fetch with one host synchronisation in all: inputs up in one copy, the step's launches, outputs down in one copy
int cc4_step_fetch(cc4_handle* h, const int32_t* actions, const uint8_t* messages, int32_t* obs, float* reward, uint8_t* done, uint32_t* err) {
  if (int rc = enter(h, "cc4_step_fetch")) return rc;
  const size_t n = (size_t)h->cfg.num_envs;
  const size_t b_act = n * NBLUE * sizeof(int32_t), b_msg = n * NBLUE * MSG_LEN;
  if (h->small_io) {                                          // (every earlier launch has completed: each call of this surface ends with a host wait)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (actions) memcpy(h->pin_in, actions, b_act);
    if (messages) memcpy(h->pin_in + b_act, messages, b_msg);
  } else if (h->cfg.num_envs <= PIN_MAX_ENVS && (actions || messages)) {
    if (!h->pin_in && pin_alloc(h, &h->pin_in, h->in_bytes)) return -1;
    if (actions) memcpy(h->pin_in, actions, b_act);
    if (messages) memcpy(h->pin_in + b_act, messages, b_msg);
    const size_t lo = actions ? 0 : b_act, hi = messages ? b_act + b_msg : b_act;
    HIPCHK(h, hipMemcpyAsync(reinterpret_cast<uint8_t*>(h->d_actions) + lo, h->pin_in + lo, hi - lo, hipMemcpyDefault, h->stream));
  } else if (upload_inputs(h, actions, messages)) return -1;
  if (launch_step(h, actions ? h->d_actions : nullptr, messages ? h->d_msgs : nullptr, false, 0, 0, false, true)) return -1;
  return fetch_outputs(h, obs, reward, done, err);
}

// cc4_step plus the red / green entries of the step's `actions` dict (SimulationController.py:236-240)
int cc4_step_ex(cc4_handle* h, const int32_t* actions, const uint8_t* messages, const cc4_agent_action* red, const cc4_agent_action* green) {
  static_assert(sizeof(cc4_agent_action) == sizeof(ExtAct) && offsetof(cc4_agent_action, session) == offsetof(ExtAct, sid) &&
                offsetof(cc4_agent_action, rate0) == offsetof(ExtAct, rate0) && offsetof(cc4_agent_action, flags) == offsetof(ExtAct, flags),
                "cc4_agent_action (include/cc4.h) is ExtAct (csrc/cc4_state.h)");
  if (!red && !green) return cc4_step(h, actions, messages);
  if (int rc = enter(h, "cc4_step_ex")) return rc;
  const size_t n = (size_t)h->cfg.num_envs;
  if (!h->d_ext && dev_alloc(h, &h->d_ext, n * EXT_PER_ENV * sizeof(ExtAct))) return -1;
  h->h_ext.resize(n * EXT_PER_ENV);
  memset(h->h_ext.data(), 0xFF, h->h_ext.size() * sizeof(ExtAct));      // type -1 everywhere: nothing submitted
  for (size_t e = 0; e < n; ++e) {
    if (red) memcpy(&h->h_ext[e * EXT_PER_ENV], red + e * NRED, NRED * sizeof(ExtAct));
    if (green) memcpy(&h->h_ext[e * EXT_PER_ENV + NRED], green + e * MAXG, MAXG * sizeof(ExtAct));
  }
  for (size_t i = 0; i < h->h_ext.size(); ++i) {     // what the kernels index with must be in range; everything else is the engine's validity check
    ExtAct& a = h->h_ext[i];
    const bool is_red = (i % EXT_PER_ENV) < (size_t)NRED;
    if (a.type == XA_NONE) continue;
    if (a.type < 0 || (is_red ? a.type > RA_INVALID : a.type > XG_INVALID) || a.host >= MAXH || (is_red && a.type == RA_DRS && a.arg >= NSUB) ||
        (is_red && a.type == RA_WITHDRAW && a.arg >= MAXH) || (!is_red && a.ticks > 1)) {
      h->err = "cc4_step_ex: action record " + std::to_string(i % EXT_PER_ENV) + " of episode " + std::to_string(i / EXT_PER_ENV) + " is out of range (type / host / subnet; a green action takes one tick)";
      return -2;
    }
  }
  HIPCHK(h, hipMemcpyAsync(h->d_ext, h->h_ext.data(), h->h_ext.size() * sizeof(ExtAct), hipMemcpyHostToDevice, h->stream));
  h->ext_seen = true; h->ext_submitted = true; h->ext_dirty = true; h->ext_green_dirty = green != nullptr;
  if (upload_inputs(h, actions, messages)) return -1;
  if (launch_step(h, actions ? h->d_actions : nullptr, messages ? h->d_msgs : nullptr, false, 0, 0, true, true)) return -1;
  return sync_all(h);
}

// direct edits of one episode between steps (state_edit, csrc/cc4_engine.h): the row and its cold part come to the host, the
// engine's own host build edits them, they go back
int cc4_edit_state(cc4_handle* h, int32_t env, int32_t op, int32_t a0, int32_t a1, int32_t a2) {
  if (env < 0 || env >= h->cfg.num_envs) { h->err = "cc4_edit_state: env out of range"; return -2; }
  FetchedRow r;
  int rc = r.fetch(h, env);
  if (rc == 0) {
    EnvState* const st = r.st; EnvCold* const cold = r.cold;
    StepWork w; memset(&w, 0, sizeof(w));
    Ctx x{st, cold, &st->rng, st->hd, &w};
    rc = state_edit(x, op, a0, a1, a2);
    // -1: an unknown op or a bad argument (the row is as it was), or an op a full container refused -- that one has raised its flag in
    // EnvState.err and may have left a process and a pid draw behind, so the row goes back in either case
    if (rc < 0) h->err = "cc4_edit_state: unknown op, bad argument, or refused by a full container (see the episode's error flags)";
    int r2 = cc4_set_state(h, env, st); if (r2 == 0) r2 = cc4_set_cold(h, env, cold); if (r2) rc = r2;
  }
  return rc;
}

int cc4_step_device(cc4_handle* h, const int32_t* d_actions, const uint8_t* d_messages) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return launch_step(h, d_actions, d_messages, false, 0, 0, false, true);
}

// ---- the red agents as learners (include/cc4.h; cc4_k_red.hip; the definition: cc4_red_view.h).
// cc4_step_device with the red agents' actions from a device tensor: k_red_submit on the main stream, behind whatever the group streams still hold (it
// reads the rows as they stand before the step and writes records the last step's kernels may still read), fills d_ext; the step's launches follow with
// the records marked as uploaded.  No upload, no host copy, no host wait.
int cc4_step_red_device(cc4_handle* h, const int32_t* d_actions, const uint8_t* d_messages, const int32_t* d_red) {
  const char* who = "cc4_step_red_device";
  if (!d_red) { h->err = std::string(who) + ": no red actions (cc4_step_device steps without them)"; return -2; }
  if (int rc = enter_refused(h, who, EN_NO_ROLLOUT | EN_NO_COMM)) return rc;
  if (reinterpret_cast<uintptr_t>(d_red) % 16) { h->err = std::string(who) + ": the red actions must be 16-byte aligned"; return -2; }
  if (int rc = enter(h, who)) return rc;
  const int n = h->cfg.num_envs;
  if (!h->d_ext && dev_alloc(h, &h->d_ext, (size_t)n * EXT_PER_ENV * sizeof(ExtAct))) return -1;     // (ext_green_dirty is still true: the kernel writes every record)
  RedSubmitArgs a{h->d_state, d_red, h->d_ext, n, h->ext_green_dirty ? 1 : 0, h->d_copy_fault};
  hipLaunchKernelGGL(k_red_submit, dim3((n * NRED + 255) / 256), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  h->ext_seen = true; h->ext_submitted = true; h->ext_dirty = true; h->ext_green_dirty = false;
  return launch_step(h, d_actions, d_messages, false, 0, 0, true, true);
}

// ---- group-wise stepping for a policy that lives on the GPU.  A step of a large batch is one launch per episode group, each group on its
// own stream, and the groups never wait for each other -- unless the caller's policy makes them: a policy kernel over the WHOLE batch
// between two steps is a barrier across the groups (cc4_step_device behind it: bench.py `policy_in_loop`).  A policy is batch-independent,
// though: applied per group, on the group's own stream, it keeps the groups' pipelines apart.  cc4_group_info says which episodes a group
// holds and which stream its launches run on (the caller enqueues its policy kernel for those episodes there); cc4_step_group_device
// launches that group's step behind it.  Without a communicator, event log or submitted red / green actions.
int cc4_group_info(cc4_handle* h, int32_t g, int32_t* lo, int32_t* hi, void** hip_stream) {
  if (g < 0 || g >= h->ngroups) { h->err = "cc4_group_info: no such group"; return -2; }
  if (lo) *lo = h->glo[g];
  if (hi) *hi = h->glo[g + 1];
  if (hip_stream) *hip_stream = reinterpret_cast<void*>(h->gstream[g]);
  return 0;
}
static int group_prologue(cc4_handle* h, int32_t g, const char* who) {
  if (g < 0 || g >= h->ngroups) { h->err = std::string(who) + ": no such group"; return -2; }
  if (h->comm || h->evlog_on || h->ext_seen) { h->err = std::string(who) + ": group-wise stepping serves handles without a communicator, event log, submitted red / green actions or recorded reward terms (cc4_enable_reward_terms)"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return fork_groups(h) ? -1 : 0;     // e.g. a reset or an upload on the main stream: the group streams start behind it (no join: the groups stay apart)
}
int cc4_step_group_device(cc4_handle* h, int32_t g, const int32_t* d_actions, const uint8_t* d_messages) {
  if (int rc = group_prologue(h, g, "cc4_step_group_device")) return rc;
  if (h->full_obs_next) { h->full_obs_gmask = (1u << h->ngroups) - 1u; h->full_obs_next = false; }
  const bool full_obs = (h->full_obs_gmask >> g) & 1u;
  h->full_obs_gmask &= ~(1u << g);
  StepArgs a = step_args(h);
  a.actions = d_actions; a.msgs = d_messages;
  a.full_obs = full_obs ? 1 : 0;
  a.prof = h->d_prof;
  launch_group(h, a, g, false, nullptr, nullptr);
  HIPCHK(h, hipGetLastError());
  if (h->ngroups > 1) h->groups_busy = true;
  return 0;
}
// the stand-in policy of bench.py for one group: uniform random action indices for the group's episodes into the handle's device action
// buffer, on the group's stream (what a policy network's kernel would do there)
int cc4_random_actions_group_device(cc4_handle* h, int32_t g, uint64_t seed0, uint32_t t) {
  if (int rc = group_prologue(h, g, "cc4_random_actions_group_device")) return rc;
  const int tot = (h->glo[g + 1] - h->glo[g]) * NBLUE;
  hipLaunchKernelGGL(k_random_actions, dim3((tot + 255) / 256), dim3(256), 0, h->gstream[g], h->d_actions, h->glo[g + 1], seed0, t, h->glo[g]);
  HIPCHK(h, hipGetLastError());
  if (h->ngroups > 1) h->groups_busy = true;
  return 0;
}

int cc4_get_obs(cc4_handle* h, int32_t* obs) {
  return copy_to_host(h, "cc4_get_obs", obs, h->d_obs, (size_t)h->cfg.num_envs * OBS_TOTAL * sizeof(int32_t), hipMemcpyDefault);
}
int cc4_get_reward_done(cc4_handle* h, float* reward, uint8_t* done) {
  if (int rc = enter(h, "cc4_get_reward_done")) return rc;      // (two pieces behind one prologue and in front of one wait: not two copy_to_host)
  const size_t n = (size_t)h->cfg.num_envs;
  if (reward) HIPCHK(h, hipMemcpyAsync(reward, h->d_reward, n * sizeof(float), hipMemcpyDefault, h->stream));
  if (done) HIPCHK(h, hipMemcpyAsync(done, h->d_done, n, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
int cc4_get_action_mask(cc4_handle* h, uint8_t* mask) {
  return copy_to_host(h, "cc4_get_action_mask", mask, h->d_mask, (size_t)h->cfg.num_envs * MASK_TOTAL, hipMemcpyDeviceToHost);
}
int cc4_get_err(cc4_handle* h, uint32_t* err) {
  return copy_to_host(h, "cc4_get_err", err, h->d_err, (size_t)h->cfg.num_envs * sizeof(uint32_t), hipMemcpyDefault);
}
int cc4_get_rng_state(cc4_handle* h, uint64_t* out) {
  if (int rc = enter(h, "cc4_get_rng_state")) return rc;
  int n = h->cfg.num_envs;
  hipLaunchKernelGGL(k_rng_state, dim3((n + 127) / 128), dim3(128), 0, h->stream, h->d_state, h->d_rng, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out, h->d_rng, (size_t)n * 7 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
int cc4_set_seed(cc4_handle* h, const uint64_t* seeds) {
  h->prev_valid = false;        // (cc4_replay_logged would repeat a step from rows that have moved on)
  if (int rc = enter(h, "cc4_set_seed")) return rc;
  int n = h->cfg.num_envs;
  HIPCHK(h, hipMemcpyAsync(h->d_seeds, seeds, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_set_seed, dim3((n + 127) / 128), dim3(128), 0, h->stream, h->d_state, h->d_cold, h->cold_row, h->d_seeds, n, h->cfg.rng_mode);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
int cc4_set_rng_state(cc4_handle* h, const uint64_t* words) {
  h->prev_valid = false;
  if (h->cfg.rng_mode != 0) { h->err = "cc4_set_rng_state: a numpy PCG64 state needs rng_mode 0"; return -2; }
  if (int rc = enter(h, "cc4_set_rng_state")) return rc;
  int n = h->cfg.num_envs;
  HIPCHK(h, hipMemcpyAsync(h->d_rng, words, (size_t)n * 6 * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));   // d_rng holds 7 words per episode
  hipLaunchKernelGGL(k_set_rng_state, dim3((n + 127) / 128), dim3(128), 0, h->stream, h->d_state, h->d_rng, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
int cc4_obs_device(cc4_handle* h, int32_t** p) { *p = h->d_obs; return 0; }
int cc4_reward_device(cc4_handle* h, float** p) { *p = h->d_reward; return 0; }
int cc4_done_device(cc4_handle* h, uint8_t** p) { *p = h->d_done; return 0; }
int cc4_actions_device(cc4_handle* h, int32_t** p) { *p = h->d_actions; return 0; }
// host copy of the handle's device action buffer: the indices cc4_step uploaded, or the ones the last step of
// cc4_run_random_steps / cc4_random_actions_device drew on the device
int cc4_get_actions(cc4_handle* h, int32_t* out) {
  return copy_to_host(h, "cc4_get_actions", out, h->d_actions, (size_t)h->cfg.num_envs * NBLUE * sizeof(int32_t), hipMemcpyDefault);
}

int cc4_random_actions_device(cc4_handle* h, uint64_t seed0, uint32_t t) {
  if (int rc = enter(h, "cc4_random_actions_device")) return rc;
  int tot = h->cfg.num_envs * NBLUE;
  hipLaunchKernelGGL(k_random_actions, dim3((tot + 255) / 256), dim3(256), 0, h->stream, h->d_actions, h->cfg.num_envs, seed0, t, 0);
  HIPCHK(h, hipGetLastError());
  return 0;
}
// ---- a policy on a stream of the caller's (a PyTorch learner on the same GPU): ordering in both directions without a host wait, and the
// outputs written into the caller's own tensors by one kernel (k_policy_outputs)
int cc4_stream_wait(cc4_handle* h, void* hip_stream) {
  if (h->rollout_k > 0 && !h->rollout_entering) { h->err = "cc4_stream_wait: a rollout is in flight on this handle: cc4_rollout_end first"; return -1; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipEventRecord(h->ev_wait, reinterpret_cast<hipStream_t>(hip_stream)));
  HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_wait, 0));
  if (h->ngroups > 1) h->main_ahead = true;      // the group streams follow at their next launch (launch_step / group_prologue)
  return 0;
}
int cc4_stream_signal(cc4_handle* h, void* hip_stream) {
  if (int rc = enter(h, "cc4_stream_signal")) return rc;
  HIPCHK(h, hipEventRecord(h->ev_signal, h->stream));
  HIPCHK(h, hipStreamWaitEvent(reinterpret_cast<hipStream_t>(hip_stream), h->ev_signal, 0));
  return 0;
}
int cc4_policy_outputs(cc4_handle* h, int32_t obs_dtype, void* d_obs, uint8_t* d_mask, float* d_reward, uint8_t* d_done, int32_t* d_err) {
  if (obs_dtype < 0 || obs_dtype > 3) { h->err = "cc4_policy_outputs: obs_dtype must be 0 (uint8), 1 (float16), 2 (bfloat16) or 3 (float32)"; return -2; }
  if (!d_obs || !d_mask || !d_reward || !d_done || !d_err) { h->err = "cc4_policy_outputs: every output buffer is required"; return -2; }
  static const uintptr_t align[4] = {4, 8, 8, 16};          // one store of four values per lane
  if (reinterpret_cast<uintptr_t>(d_obs) % align[obs_dtype] || reinterpret_cast<uintptr_t>(d_reward) % 4 || reinterpret_cast<uintptr_t>(d_err) % 4) {
    h->err = "cc4_policy_outputs: the observation buffer must be aligned to four values, reward and error buffers to 4 bytes"; return -2;
  }
  if (int rc = enter(h, "cc4_policy_outputs")) return rc;
  const int n = h->cfg.num_envs, tpb = 256;
  const int ep_blocks = (n + tpb - 1) / tpb;
  const long long vecs = (long long)n * OBS_TOTAL / 4;
  // the observations are a streaming copy: enough blocks to fill the chip (8 per CU), each lane looping over what is left
  const int obs_blocks = (int)std::max(1LL, std::min((vecs + tpb - 1) / tpb, 8LL * h->cus));
  hipLaunchKernelGGL(k_policy_outputs, dim3(ep_blocks + obs_blocks), dim3(tpb), 0, h->stream, h->d_state, h->d_obs, h->d_reward, h->d_done, h->d_err,
                     n, ep_blocks, (int)obs_dtype, d_obs, d_mask, d_reward, d_done, d_err, h->d_mask_stale);
  HIPCHK(h, hipGetLastError());
  return 0;
}
// ---- episode copies (cc4_k_copy.hip).  Two launches on the main stream, no host synchronisation: k_copy_claim (one lane per entry) claims the
// destinations with a stamp no other call of the process uses, k_copy_episodes (one workgroup per entry) checks the claims and copies.
static std::atomic<uint32_t> g_copy_stamp{0};
size_t cc4_snapshot_bytes(cc4_handle* h) { return h ? slot_bytes(h->cold_row) : 0; }
int cc4_copy_episodes_device(cc4_handle* h, int32_t n, const void* d_src_bank, int32_t src_capacity, const int32_t* d_src,
                             void* d_dst_bank, int32_t dst_capacity, const int32_t* d_dst, const uint64_t* d_seeds) {
  const char* who = "cc4_copy_episodes_device";
  if (n < 0 || (n > 0 && (!d_src || !d_dst))) { h->err = std::string(who) + ": n < 0, or no index arrays"; return -2; }
  if (int rc = enter_refused(h, who, EN_NO_ROLLOUT | EN_NO_COMM)) return rc;
  if (d_src_bank && d_dst_bank) { h->err = std::string(who) + ": bank -> bank copies are not supported (one side must be the handle's episodes)"; return -2; }
  if (d_seeds && d_dst_bank) { h->err = std::string(who) + ": seeds apply to copies into the handle's episodes only"; return -2; }
  if ((d_src_bank && src_capacity < 0) || (d_dst_bank && dst_capacity < 0)) { h->err = std::string(who) + ": negative bank capacity"; return -2; }
  if (reinterpret_cast<uintptr_t>(d_src_bank) % 64 || reinterpret_cast<uintptr_t>(d_dst_bank) % 64) { h->err = std::string(who) + ": a bank must be 64-byte aligned"; return -2; }
  if (n == 0) return 0;
  if (int rc = enter(h, "cc4_copy_episodes_device")) return rc;
  h->prev_valid = false;        // (cc4_replay_logged would repeat a step from rows that have moved on)
  uint32_t stamp = g_copy_stamp.fetch_add(1) % 0x7FFFFFFFu + 1u;     // 1 .. 2^31 - 1: claim words 2 * stamp and 2 * stamp + 1, never 0
  CopyArgs a{h->d_state, h->d_cold, h->cold_row, h->d_obs, h->d_reward, h->d_done, h->d_err, h->d_mask, h->d_mask_stale, h->d_claim,
             static_cast<const uint8_t*>(d_src_bank), static_cast<uint8_t*>(d_dst_bank), slot_bytes(h->cold_row), d_src, d_dst, d_seeds,
             n, h->cfg.num_envs, d_src_bank ? src_capacity : h->cfg.num_envs, d_dst_bank ? dst_capacity : h->cfg.num_envs,
             h->cfg.steps, h->cfg.rng_mode, h->evlog_on, stamp, h->d_copy_fault};
  hipLaunchKernelGGL(k_copy_claim, dim3((n + 255) / 256), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  hipLaunchKernelGGL(k_copy_episodes, dim3(n), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  if (h->ngroups > 1) h->main_ahead = true;      // the group streams follow at their next launch
  return 0;
}
int cc4_copy_faults(cc4_handle* h, uint32_t* out) {
  if (int rc = enter(h, "cc4_copy_faults")) return rc;
  HIPCHK(h, hipMemcpyAsync(out, h->d_copy_fault, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemsetAsync(h->d_copy_fault, 0, sizeof(uint32_t), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
int cc4_clone_episodes(cc4_handle* h, int32_t n, const int32_t* src, const int32_t* dst, const uint64_t* seeds) {
  if (n < 0 || n > h->cfg.num_envs) { h->err = "cc4_clone_episodes: n must be 0 .. num_envs"; return -2; }
  if (n == 0) return 0;
  if (int rc = enter(h, "cc4_clone_episodes", EN_NO_ROLLOUT)) return rc;
  const size_t N = (size_t)h->cfg.num_envs;
  if (!h->d_copy_idx && dev_alloc(h, &h->d_copy_idx, 2 * N * sizeof(int32_t))) return -1;
  if (seeds && !h->d_copy_seeds && dev_alloc(h, &h->d_copy_seeds, N * sizeof(uint64_t))) return -1;
  HIPCHK(h, hipMemcpyAsync(h->d_copy_idx, src, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d_copy_idx + N, dst, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  if (seeds) HIPCHK(h, hipMemcpyAsync(h->d_copy_seeds, seeds, (size_t)n * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
  if (int rc = cc4_copy_episodes_device(h, n, nullptr, 0, h->d_copy_idx, nullptr, 0, h->d_copy_idx + N, seeds ? h->d_copy_seeds : nullptr)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));     // (the host arrays may go away once the call returns)
  return 0;
}
int cc4_synchronize(cc4_handle* h) {
  if (h->rollout_k > 0) { h->err = "cc4_synchronize: a rollout is in flight on this handle (its kernel ends when every pass is published): cc4_rollout_end"; return -1; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return sync_all(h);
}
int cc4_launches_per_step(cc4_handle* h) { return h ? h->ngroups : 0; }
// host-side counters since cc4_create: steps issued by cc4_run_random_steps, microseconds the host spent enqueueing their step
// launches and their all-gathers, all-gathers issued, and how many times a step had to WAIT for an old all-gather before it
// could reuse that observation buffer (0 = the exchange never held the compute stream up)
int cc4_host_stats(cc4_handle* h, double* out /* [5] */) {
  out[0] = (double)h->stat_steps; out[1] = h->stat_launch_us; out[2] = h->stat_gather_us; out[3] = (double)h->gathers_issued; out[4] = (double)h->gather_stalls;
  return 0;
}

int cc4_get_state(cc4_handle* h, int32_t env, void* buf) {
  if (env < 0 || env >= h->cfg.num_envs) { h->err = "cc4_get_state: env out of range"; return -2; }
  return copy_to_host(h, "cc4_get_state", buf, h->d_state + env, sizeof(EnvState), hipMemcpyDeviceToHost);
}
int cc4_get_states(cc4_handle* h, int32_t first, int32_t count, void* buf) {
  if (first < 0 || count < 0 || first + count > h->cfg.num_envs) { h->err = "cc4_get_states: range out of the batch"; return -2; }
  return copy_to_host(h, "cc4_get_states", buf, h->d_state + first, (size_t)count * sizeof(EnvState), hipMemcpyDeviceToHost);
}
int cc4_set_state(cc4_handle* h, int32_t env, const void* buf) {
  h->prev_valid = false;        // (also every cc4_edit_state, which writes the rows back through here)
  if (env < 0 || env >= h->cfg.num_envs) { h->err = "cc4_set_state: env out of range"; return -2; }
  {   // the cold containers of this handle were sized from cfg.steps; the row says how long ITS episode is (EnvState.steps)
    const int st_steps = static_cast<const EnvState*>(buf)->steps;
    // (0 = a never-reset, all-zero row; a negative length would turn into negative container capacities on the device)
    if (st_steps < 0 || (st_steps > 0 && cold_row_bytes(st_steps) != h->cold_row)) {
      h->err = "cc4_set_state: the row belongs to an episode of " + std::to_string(st_steps) + " steps, whose cold containers differ from this handle's (steps=" + std::to_string(h->cfg.steps) + ")";
      return -2;
    }
  }
  if (int rc = enter(h, "cc4_set_state")) return rc;
  HIPCHK(h, hipMemcpyAsync(h->d_state + env, buf, sizeof(EnvState), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->full_obs_next = true;      // the observation buffer still holds the previous occupant's slowly varying values
  return 0;
}

size_t cc4_cold_bytes(cc4_handle* h) { return h ? h->cold_row : 0; }
int FetchedRow::fetch(cc4_handle* h, int32_t env) {
  st = static_cast<EnvState*>(malloc(sizeof(EnvState)));
  cold = static_cast<EnvCold*>(malloc(h->cold_row));
  if (!st || !cold) { h->err = "no host memory for an episode's rows"; return -1; }
  if (int rc = cc4_get_state(h, env, st)) return rc;
  return cc4_get_cold(h, env, cold);
}
int cc4_get_cold(cc4_handle* h, int32_t env, void* buf) {
  if (env < 0 || env >= h->cfg.num_envs) { h->err = "cc4_get_cold: env out of range"; return -2; }
  return copy_to_host(h, "cc4_get_cold", buf, cold_at(h->d_cold, (size_t)env, h->cold_row), h->cold_row, hipMemcpyDeviceToHost);
}
int cc4_set_cold(cc4_handle* h, int32_t env, const void* buf) {
  h->prev_valid = false;
  if (env < 0 || env >= h->cfg.num_envs) { h->err = "cc4_set_cold: env out of range"; return -2; }
  if (int rc = enter(h, "cc4_set_cold")) return rc;
  HIPCHK(h, hipMemcpyAsync(cold_at(h->d_cold, (size_t)env, h->cold_row), buf, h->cold_row, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}

int cc4_get_topology(cc4_handle* h, int32_t env, uint8_t* out) {
  if (env < 0 || env >= h->cfg.num_envs) { h->err = "cc4_get_topology: env out of range"; return -2; }
  FetchedRow r;
  if (int rc = r.fetch(h, env)) return rc;
  for (int i = 0; i < NSUB; ++i) { out[i] = r.st->cidr_octet[i]; out[9 + i] = r.st->n_users[i]; out[18 + i] = r.st->n_servers[i]; }
  for (int i = 0; i < MAXH; ++i) { out[27 + 2 * i] = bit_get(r.st->exists, i) ? 1 : 0; out[28 + 2 * i] = r.cold->hs[i].ip_octet; }
  return 0;
}

int cc4_enable_event_log(cc4_handle* h, int32_t enable) {
  if (int rc = enter(h, "cc4_enable_event_log")) return rc;
  hipLaunchKernelGGL(k_set_evlog, dim3((h->cfg.num_envs + 255) / 256), dim3(256), 0, h->stream, h->d_cold, h->cold_row, h->cfg.num_envs, enable ? 1u : 0u);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->evlog_on = enable ? 1 : 0;
  return 0;
}
// The event log on demand (handles of up to 16 episodes without a communicator).  cc4_keep_previous(1): every step launch is preceded by a
// device-side copy of the episodes' rows.  cc4_replay_logged: the LAST step again, on that copy, with the logging build of the step kernel
// and the same inputs (the action / message / submitted-action buffers still hold them) -- the copy ends where the live rows are, and its
// event log is copied into the live cold rows: cc4_get_true_state then reports the HostEvents entries of the last step although the step
// itself ran the fast build.  With no step since the reset the log is simply empty.  Same generator positions: logging draws nothing in
// the numpy-stream mode and only side streams in the counter mode.
int cc4_keep_previous(cc4_handle* h, int32_t on) {
  if (on && (h->comm || h->cfg.num_envs > 16 || h->cfg.autoreset)) { h->err = "cc4_keep_previous: for handles of up to 16 episodes without a communicator or autoreset"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t n = (size_t)h->cfg.num_envs;
  if (on && !h->d_prev_state) {
    if (dev_alloc(h, &h->d_prev_state, n * sizeof(EnvState)) || dev_alloc(h, &h->d_prev_cold, n * h->cold_row) || dev_alloc(h, &h->d_prev_out, h->out_bytes)) return -1;
  }
  h->keep_prev = on != 0;
  h->prev_valid = false;
  return 0;
}
int cc4_replay_logged(cc4_handle* h) {
  if (!h->keep_prev) { h->err = "cc4_replay_logged: cc4_keep_previous is off"; return -2; }
  if (int rc = enter(h, "cc4_replay_logged")) return rc;
  const int n = h->cfg.num_envs;
  if (!h->prev_valid) {      // no step since the reset (or steps whose inputs are gone): an enabled, empty log
    hipLaunchKernelGGL(k_set_evlog, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_cold, h->cold_row, n, 1u);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
  }
  hipLaunchKernelGGL(k_set_evlog, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_prev_cold, h->cold_row, n, 1u);
  HIPCHK(h, hipGetLastError());
  int32_t* o = reinterpret_cast<int32_t*>(h->d_prev_out);
  float* rw = reinterpret_cast<float*>(o + (size_t)n * OBS_TOTAL);
  uint32_t* er = reinterpret_cast<uint32_t*>(rw + n);
  uint8_t* dn = reinterpret_cast<uint8_t*>(er + n);
  StepArgs a = step_args(h);
  a.st = h->d_prev_state; a.cold = h->d_prev_cold;
  a.actions = h->prev_actions; a.msgs = h->prev_msgs;
  a.obs = o; a.reward = rw; a.done = dn; a.err = er;
  a.autoreset = 0;
  a.full_obs = 1;
  a.ext = h->prev_ext ? h->d_ext : nullptr;
  for (int g = 0; g < h->ngroups; ++g) launch_group(h, a, g, true, nullptr, nullptr);
  HIPCHK(h, hipGetLastError());
  if (h->ngroups > 1) { h->groups_busy = true; if (join_groups(h)) return -1; }
  hipLaunchKernelGGL(k_copy_evlog, dim3(n), dim3(64), 0, h->stream, h->d_cold, h->d_prev_cold, h->cold_row, n);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->prev_valid = false;          // (the copy has moved on: a second replay would repeat the step from the wrong rows)
  return 0;
}
int64_t cc4_get_true_state(cc4_handle* h, int32_t env, char* json, size_t cap) {
  if (env < 0 || env >= h->cfg.num_envs) { h->err = "cc4_get_true_state: env out of range"; return -2; }
  FetchedRow r;
  if (int rc = r.fetch(h, env)) return rc;
  const std::string doc = export_true_state(*r.st, *r.cold);
  if (json && cap >= doc.size() + 1) memcpy(json, doc.c_str(), doc.size() + 1);
  return (int64_t)doc.size() + 1;
}

}  // extern "C"
