// cc4_host.h -- what the host-side translation units of libcc4.so share (cc4_api*.hip; no kernel unit includes it): the handle, who owns what it
// allocates (dev_alloc .. release over cc4_owned.h: the only place that allocates or frees device memory, pinned memory, events and streams), the
// enqueue threads' block, and the helpers that are called across units.  Those are part of no ABI: hidden, so that libcc4.so exports the C ABI only.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <cmath>
#include <string>
#include <chrono>
#include <vector>
#include <deque>
#include <map>
#include <algorithm>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <atomic>

#include "../../include/cc4_debug.h"
#include "cc4_args.h"
#include "cc4_kernel_decls.h"
#include "cc4_export.h"
#include "cc4_digest.h"
#include "cc4_owned.h"
#define CC4_HOST __attribute__((visibility("hidden")))

// the runtime's releasers for the owner of a handle's resources (cc4_handle::own), in the order of OwnedKind
inline void free_device(void* p) { (void)hipFree(p); }
inline void free_pinned(void* p) { (void)hipHostFree(p); }
inline void free_event(void* p) { (void)hipEventDestroy(static_cast<hipEvent_t>(p)); }
inline void free_stream(void* p) { (void)hipStreamDestroy(static_cast<hipStream_t>(p)); }

struct cc4_handle {
  cc4_config cfg;
  // every device block, pinned block, event and stream below is registered here by the call that creates it (dev_alloc, pin_alloc, new_event,
  // new_stream), wherever and whenever that is; cc4_destroy releases the list.  Not registered, because nothing frees them: pointers INTO a block (d_msgs,
  // d_reward, d_err, d_done, d_copy_fault), device addresses of pinned memory (d_xtimeout; d_actions and d_obs of a small handle), second names (gstream[0], tev_*).
  OwnedList own{{free_device, free_pinned, free_event, free_stream}, {}};
  hipStream_t stream = nullptr;
  EnvState* d_state = nullptr; EnvCold* d_cold = nullptr;
  size_t cold_row = 0;             // bytes per cold row: fixed part + the containers sized from cfg.steps (cold_row_bytes)
  int32_t* d_actions = nullptr; uint8_t* d_msgs = nullptr; uint64_t* d_seeds = nullptr; uint8_t* d_envmask = nullptr;
  int32_t* d_obs = nullptr; float* d_reward = nullptr; uint8_t* d_done = nullptr; uint32_t* d_err = nullptr;
  uint8_t* d_mask = nullptr; uint64_t* d_rng = nullptr;
  // d_obs | d_reward | d_err | d_done are ONE allocation (base d_obs), d_actions | d_msgs another (base d_actions): cc4_step_fetch moves
  // a step's inputs and outputs with one copy each; small batches go through pinned staging buffers (a copy to or from pageable
  // memory is staged by the runtime anyway, synchronously and per call)
  size_t out_bytes = 0, in_bytes = 0;
  uint8_t* pin_out = nullptr; uint8_t* pin_in = nullptr;
  // Handles of up to SMALL_IO_ENVS episodes (the single-episode wrapper surface) keep both blocks in pinned HOST memory the device reads
  // and writes directly: the step kernel fetches its five action indices over PCIe and posts its results there, so a step is a launch and
  // one host wait -- no copy engine in either direction (each DMA costs ~10 us of latency for a few hundred bytes).  CC4_SMALL_IO=0: off.
  static constexpr int SMALL_IO_ENVS = 16;
  bool small_io = false;
  // cc4_keep_previous / cc4_replay_logged (small handles): the rows as they stood before the last step, so that the step can be repeated
  // with the event log on when -- and only when -- somebody asks what happened in it (the single-episode wrapper surface: flat
  // observations need no log, and the logging build of the numpy-stream kernel walks its green actions serially: +30 us per step)
  bool keep_prev = false, prev_valid = false;
  EnvState* d_prev_state = nullptr; EnvCold* d_prev_cold = nullptr; uint8_t* d_prev_out = nullptr;
  const int32_t* prev_actions = nullptr; const uint8_t* prev_msgs = nullptr; bool prev_full_obs = false, prev_ext = false;
  // byte observations and gathered observations ([world*N][578]) in a ring of OBS_RING buffers: the all-gather of step t
  // overlaps later steps, and the compute stream waits for the communication stream only once per OBS_WAIT_EVERY steps
  // (a cross-stream wait in front of every launch costs the stream ~10 us)
  static constexpr int OBS_RING = 8, OBS_WAIT_EVERY = 4;
  static constexpr int MAX_GROUPS = cc4_handle_max_groups;          // launches per step (episode groups, below); CC4_GROUPS may ask for up to this many
  uint8_t* d_obs8[OBS_RING] = {};
  uint8_t* d_all_obs8[OBS_RING] = {};
  long long gather_seq[OBS_RING] = {};           // sequence number of the last all-gather that read buffer b (0 = none)
  long long gathers_issued = 0, gathers_waited = 0;
  hipEvent_t tev_start[cc4_handle_max_groups] = {}, tev_stop[cc4_handle_max_groups] = {};   // timing events the NEXT launch of a group carries (cc4_run_random_steps)
  long long comm_delay_ticks = 0;                // debug: spin this long on the communication stream ahead of every all-gather
  long long gather_stalls = 0;                   // a step launch found the all-gather it had to wait for still running
  long long stat_steps = 0; double stat_launch_us = 0, stat_gather_us = 0;   // cc4_host_stats
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_step[OBS_RING][MAX_GROUPS] = {}, ev_comm[OBS_RING] = {};   // ev_step[b][g]: group g's launch that wrote buffer b; ev_comm[q % OBS_RING]: all-gather number q has completed
  int obs_buf = 0;                               // buffer written by the most recent step
  int gather_buf = -1;                           // buffer of the most recent all-gather (-1: none issued)
  bool step_event_attached = false;              // ev_step[obs_buf] was recorded by the launch of that step itself
  // A step of a large batch is issued as `ngroups` launches, one per contiguous group of episodes, each group on its own HIP
  // stream (group 0 on `stream`): episodes are independent, a group's next step depends only on its own previous one, so while
  // one group's launch drains -- its last blocks running on a half-empty chip -- the other group's launch fills the free
  // slots, and the chip stays full across step boundaries.  Measured on MI355X (r03, 8192 episodes, counter mode): one launch
  // per step 507 M agent-env steps/s, two groups of 4096 on two streams 639 M (a single 32768-episode launch per step: 605 M).
  int ngroups = 1;
  int cus = 256;                                 // compute units of the device
  int glo[MAX_GROUPS + 1] = {};                  // group g = episodes [glo[g], glo[g + 1])
  hipStream_t gstream[MAX_GROUPS] = {};          // gstream[0] == stream
  hipEvent_t gev[MAX_GROUPS] = {};               // group stream -> main stream ordering (join_groups)
  hipEvent_t mev = nullptr;                      // main stream -> group streams ordering: recorded and waited for in fork_groups (cc4_api.hip), nowhere else
  hipEvent_t ev_wait = nullptr, ev_signal = nullptr;   // a caller's stream -> main stream (cc4_stream_wait), main stream -> a caller's stream (cc4_stream_signal)
  bool auto_groups = true;                       // the number of groups is the library's choice (no CC4_GROUPS)
  bool groups_busy = false;                      // a group stream other than the main one may hold unfinished step launches
  bool joined_between = false;                   // something ordered the main stream behind all groups (or waited for them) since the last step launches:
                                                 // the caller works on the WHOLE batch between steps (launch_step: one launch then, not one per group)
  bool main_ahead = false;                       // the main stream holds work the group streams have not been ordered behind
  unsigned long long* d_prof = nullptr;
  int dbg_stop = 0;                  // cc4_debug_stop_phase
  uint32_t* d_reset_ws = nullptr;    // k_step_philox1's generation work area, [num_envs][RESET_WS_WORDS]
  uint8_t* d_unpacked = nullptr;                 // [world*N][578] bytes: cc4_unpack_obs_device
  int evlog_on = 0;               // cc4_enable_event_log
  // externally submitted red / green actions (cc4_step_ex).  Once a handle has taken any, its steps run the full builds of the
  // kernels (an action queued for several ticks carries its own rates into later steps), with d_ext all XA_NONE for the steps
  // that submit nothing
  // the persistent run kernel (k_run_philox1: K steps of the batch in one launch; RunArgs): per-episode progress, the CU table, the ticket counters
  uint32_t* d_run = nullptr;      // [n] progress words
  int32_t* d_slot_part = nullptr; // [CC4_SLOTS] CU slot id -> 1 + partition (persist_setup)
  unsigned long long* d_timeline = nullptr;   // CC4_PERSIST_TIMELINE: per-wave time stamps of the current persistent launch
  size_t run_words = 0;           // words of d_run
  int run_P = 0, run_grid = 0;    // partitions (= CUs that take waves), waves per launch; 0: the persistent path is off
  int run_G = 0;                  // exchange groups of the persistent kernel (episode e counts in group e % run_G): the device's CUs
  uint8_t xcc_lo[8] = {0}, xcc_n[8] = {0};
  int run_thr = 16;               // a wave helps the partition that lags most once its own is more than this many tickets ahead (CC4_PERSIST_THR)
  uint32_t* d_pool = nullptr;     // [2][CC4_SLOTS][TK_STRIDE] the partitions' ticket counters, one set per call parity
  int run_SA = 0, run_SB = 1, run_nB = 0, run_single = 0;   // runs of steps (run_args -> RunArgs.runs; CC4_PERSIST_RUNS="SA,SB,nB,single"; SA = 1: every step an item, as in r05;
                                                            // SA = 0: chosen per call -- 4 steps, 8 in calls of 64 steps and more: profiles/r06_runs_ab.txt, r06_sched_ab2.txt)
  RunSplit last_runs{};           // the runs of the most recent persistent launch (cc4_debug_last_run_split)
  uint32_t pool_base = 0;         // steps every episode's progress word stands at (the words are not cleared between calls)
  int pool_parity = 0;
  int persist_state = -1;         // -1 off / unavailable, 0 not set up yet (persist_setup on first use), 1 on
  bool whole_batch_steps = true;  // CC4_WHOLE_BATCH_STEPS=0: the step entry points always launch per group (A/B)
  int run_margin = 0;             // episode blocks per CU the one-launch forms leave free (choose_run_form)
  // the per-step hand-off out of the one-launch kernels (XchgArgs): with a communicator, cc4_run_random_steps stays ONE launch and the
  // communication stream follows the kernel's per-step counters (xchg_*)
  static constexpr int XRING = 32;
  bool xchg_on = false;           // cc4_comm_init; CC4_EXCHANGE_INKERNEL=0 keeps the per-step launches
  int xchg_chunk = 8;             // steps per gate / publish on the communication stream (CC4_EXCHANGE_CHUNK; their slabs go out in ONE all-gather: the host
                                  // pays ~25 us to enqueue a wait, an all-gather and a publish -- more than a step of a small batch lasts)
  uint8_t* d_xslab = nullptr;     // [XRING][n][OBS_PACKED]
  uint8_t* d_xall = nullptr;      // [XRING][world * n][OBS_PACKED]
  int khz = 0;                    // wall-clock rate (hipDeviceAttributeWallClockRate), asked once
  // ---- rollouts with the policy in the loop (cc4_rollout_begin .. cc4_rollout_end)
  int32_t* d_ract = nullptr;      // [2][n][5] action slots (step j reads slot j % 2)
  uint32_t* d_rready = nullptr;   // [P][32] words: word g of partition p's line = actions of steps < value are published for policy group g (every line holds the same)
  uint32_t* d_rcnt = nullptr;     // [P][RPG][XRING] episodes of (partition, policy group) whose packed row of step j is in memory (slot j % XRING)
  uint32_t* d_rfail = nullptr;    // [1] a gate gave up
  hipStream_t policy_stream = nullptr;   // = gpolicy[0]
  hipStream_t gpolicy[4] = {nullptr, nullptr, nullptr, nullptr};   // one policy stream per policy group: the groups' gate -> policy -> publish chains run side by side
  hipEvent_t rev = nullptr;       // the rollout's starting observations are packed (slab XRING - 1)
  int rollout_k = 0;              // > 0: a rollout of that many steps is in flight
  bool rollout_entering = false;  // cc4_rollout_end is draining it (its own calls may pass join_groups)
  int rollout_watchdog_ms = 2000;
  int rollout_margin = 1;
  int rpg = 4;                    // policy groups (CC4_ROLLOUT_GROUPS, 1 .. RPG_MAX)
  int obs8_from_slab = -1;        // >= 0: the per-step ring's current buffer is to be filled from this slab of the exchange ring (xchg_end), when somebody reads it
  uint32_t* d_xflags = nullptr;   // [0] gathered, [1] timeout (what the waits poll)
  uint32_t* d_xgcnt = nullptr;    // [groups][XRING] group counters (xchg_count)
  uint32_t* h_xtimeout = nullptr; // pinned host word the kernel raises when a wait gives up (read without a copy)
  uint32_t* d_xtimeout = nullptr; // its device address
  int xflags_clean = 0;           // the flags are cleared already (behind the previous call) and xev says when
  hipEvent_t xev = nullptr;
  long long xchg_calls = 0, xchg_timeouts = 0;
  int xchg_watchdog_ms = 2000;
  uint8_t* last_gathered = nullptr;   // gathered rows of the most recent all-gather, whichever path issued it
  uint8_t* d_xlog = nullptr;      // debug (cc4_debug_gather_log): every gathered slab in issue order, [xlog_cap][world * n][OBS_PACKED]
  int xlog_cap = 0, xlog_n = 0;
  bool persist_refused = false;   // persist_setup found an unexpected picture (said so on stderr; cc4_run_kernel reports the per-step kernel)
  // CC4_PERSIST_VERIFY=1: every one-launch call of cc4_run_random_steps is repeated with per-step launches on a shadow handle that starts
  // from a copy of this handle's rows, and the two results are compared episode by episode (verify_*)
  bool verify = false, is_shadow = false;
  int verify_every = 1024;        // without CC4_PERSIST_VERIFY: every verify_every-th persistent call is checked all the same (CC4_PERSIST_VERIFY_EVERY; 0: never)
  uint64_t persist_calls = 0;
  cc4_handle* shadow = nullptr;
  uint64_t* d_digest = nullptr;   // [num_envs] per-episode digest
  uint32_t* d_plan_err = nullptr; // [num_envs] cc4_run_plan_device: the error flags the steps of the call in flight raised (zero between calls)
  long long verify_calls = 0, verify_mismatches = 0;
  // test hook (cc4_debug_verify_plant): ONE difference planted in the shadow's side of the next checked call, between its runs and its compare (part -1: none armed)
  struct VerifyPlant { int32_t part = -1, env = 0, step = 0; int64_t offset = 0; } plant;
  int persist_min_k = 10;         // shorter calls keep the per-step launches: a launch's ramp and tail cost a few steps' worth (with the tail's items shared
                                  // among the CUs of an XCD: K = 10: 733 vs 685 M, K = 20: 813 vs 742 M, K = 32: 857 vs 756 M; CC4_PERSIST_MIN_K)
  struct EnqPool* pool = nullptr; // one enqueue thread per group stream beyond the first (cc4_run_random_steps; enq_*)
  bool enq_threads = false;
  bool run1m = false;             // cc4_run_random_steps as ONE launch of k_run_philox1m (batches of the one-wave kernel that one launch holds)
  int multistep_minb = 5;         // which build of it: 5 (k_run_philox) or 8 blocks per CU (k_run_philox8)
  bool multistep = false;         // k_run_philox: cc4_run_random_steps as ONE launch, every block looping over the steps of its episode
  ExtAct* d_ext = nullptr;        // [num_envs][EXT_PER_ENV]
  bool ext_seen = false, ext_dirty = false;   // dirty: d_ext holds the records of an earlier step
  // ext_seen = ext_submitted || terms_on.  ext_submitted: a red or green action was submitted on this handle (cc4_step_ex, cc4_step_red_device): it never
  // leaves the full builds.  terms_on: cc4_enable_reward_terms -- the same machinery with all-none records, which the switch may take back
  bool ext_submitted = false, terms_on = false;
  // ext_green_dirty: false only while the GREEN records of d_ext are known to be all XA_NONE; cc4_step_red_device then writes its six red records per episode
  // and nothing else, otherwise it sets the green records to none as well.  True from the start (d_ext not allocated, or allocated and never written: a
  // cc4_step_ex that refused its records has allocated it already).  Cleared by: k_red_submit with clear_green (cc4_step_red_device), the upload of a
  // cc4_step_ex without green actions, the memset of launch_step.  Set by: the upload of a cc4_step_ex with green actions.
  bool ext_green_dirty = true;
  std::vector<ExtAct> h_ext;
  bool full_obs_next = true;      // the next step launch rewrites every observation value (fresh handle, restored state)
  uint32_t full_obs_gmask = 0;    // ... per group, for the group-wise launches of cc4_step_group_device
  bool philox_lean = false;       // k_step_philox1 (one wave per episode) instead of k_step_philox (cc4_create)
  int philox_minw = 1;            // which register budget of k_step_philox this batch size runs (1, 7 or 8 blocks per CU; cc4_create)
  ncclComm_t comm = nullptr; int rank = 0, world = 1;
  // episode copies (cc4_copy_episodes_device): claim words of the episodes, the OR of the copies' fault bits, the per-episode "mask stale" marks
  // k_policy_outputs honours; the host-array surface (cc4_clone_episodes) stages its indices and seeds in d_copy_idx
  uint32_t* d_claim = nullptr; uint32_t* d_copy_fault = nullptr; uint8_t* d_mask_stale = nullptr;
  int32_t* d_copy_idx = nullptr; uint64_t* d_copy_seeds = nullptr;
  int8_t* d_pol = nullptr;       // [6 n] staging of the host-array surface of the per-episode classes (cc4_set_policies: three [n] inputs; cc4_get_policies: two [n][3] outputs)
  std::deque<hipEvent_t> evs;                    // timing events of cc4_run_random_steps: [group][2 * timed group of launches + {start, stop}] (a deque: its elements are
                                                 // owned fields, and they stay where they are when it grows)
  std::string err;
};

#define HIPCHK(h, call)                                                                        \
  do {                                                                                         \
    hipError_t _e = (call);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(_e);                            \
      return -1;                                                                               \
    }                                                                                          \
  } while (0)

// ---- what the entry points that take a tensor's dtype code or a sampling temperature accept (the views' sample_bad, cc4_api_learn.hip)
inline bool dtype_ok(int32_t dtype) { return dtype >= 1 && dtype <= 3; }      // 1 float16, 2 bfloat16, 3 float32
inline bool temperature_ok(float t) { return t > 0.0f && std::isfinite(t); }      // finite and positive (a NaN fails the compare)

// ---- what a handle allocates (cc4_handle::own).  The field is registered before it is filled, so a failure anywhere later still finds it; a field
// that holds something already gives that back first (the free-and-reallocate sites: d_run, d_xlog, d_timeline).  0 or -1 with h->err set.
template <class T> void** own_field(cc4_handle* h, T** field, OwnedKind kind) {
  void** const f = reinterpret_cast<void**>(field);
  h->own.add(f, kind); h->own.release(f);
  return f;
}
template <class T> int dev_alloc(cc4_handle* h, T** field, size_t bytes) { HIPCHK(h, hipMalloc(own_field(h, field, OWN_DEVICE), bytes)); return 0; }
template <class T> int pin_alloc(cc4_handle* h, T** field, size_t bytes) { HIPCHK(h, hipHostMalloc(own_field(h, field, OWN_PINNED), bytes, hipHostMallocDefault)); return 0; }
inline int new_event(cc4_handle* h, hipEvent_t* ev, unsigned flags) { own_field(h, ev, OWN_EVENT); HIPCHK(h, hipEventCreateWithFlags(ev, flags)); return 0; }
inline int new_stream(cc4_handle* h, hipStream_t* st) { own_field(h, st, OWN_STREAM); HIPCHK(h, hipStreamCreateWithFlags(st, hipStreamNonBlocking)); return 0; }
template <class T> void release(cc4_handle* h, T** field) { h->own.release(reinterpret_cast<void**>(field)); }
// a device block that lives as long as one call: freed on every path out of it
CC4_HOST extern std::atomic<int64_t> g_scoped_blocks;      // how many of them exist (cc4_debug_live_resources)
template <class T> struct DevTemp {
  T* p = nullptr;
  DevTemp() = default;
  DevTemp(const DevTemp&) = delete;
  ~DevTemp() { if (p) { (void)hipFree(p); g_scoped_blocks.fetch_sub(1); } }
  int alloc(cc4_handle* h, size_t bytes) { HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&p), bytes)); g_scoped_blocks.fetch_add(1); return 0; }
};
// ---- host copies of rows, freed on every path.  RowCopy: a caller's bytes (cc4_get_state, a checkpoint) may sit at any address, so what a host-side definition
// reads is copied into aligned memory (cc4_api_views.hip row_copies; the cold parts are null without a cold row).  FetchedRow: one episode's rows out of a handle.
struct RowCopy {
  EnvState* s = nullptr;
  EvLog* lg = nullptr; uint32_t* sus = nullptr; RewardRec* rwd = nullptr;
  ~RowCopy() { free(s); free(lg); free(sus); free(rwd); }
};
inline void* row_copy(const void* src, size_t bytes, size_t align, size_t room = 0) {      // room: the block's size where it is more than the bytes copied
  void* p = aligned_alloc(align, (std::max(bytes, room) + align - 1) / align * align);
  if (p) memcpy(p, src, bytes);
  return p;
}
struct FetchedRow {
  EnvState* st = nullptr; EnvCold* cold = nullptr;
  ~FetchedRow() { free(st); free(cold); }
  CC4_HOST int fetch(cc4_handle* h, int32_t env);      // 0, or what cc4_get_state / cc4_get_cold returned (-1 as well without memory)
};

// ---- one enqueue thread per group stream (cc4_run_random_steps without a communicator).  The groups of a batch never wait for each
// other, so their launches need not come from one thread: the first launch on a stream that has been synchronised costs the calling
// thread ~10 us (3.5 us in the steady state), four in a row delay the last group's first kernel by 30-45 us in every timed region;
// issued side by side they cost one.  A worker spins for 200 us after a call (CC4_ENQ_SPIN_US; a loop of calls keeps it hot), then sleeps.
struct EnqPool {
  std::vector<std::thread> th;
  std::mutex mu; std::condition_variable cv;
  std::atomic<uint64_t> gen{0};
  std::atomic<int> pending{0}, failed{0};
  std::atomic<bool> quit{false};
  int spin_us = 200;            // how long a worker spins for the next call before it parks on the condition variable (CC4_ENQ_SPIN_US): a loop of
                                // calls with nothing in between keeps it hot, a caller that does host work between bursts gets its cores back
  StepArgs a{}; int k = 0; uint32_t t0 = 0; bool full = false, first_full_obs = false;
  hipEvent_t start[cc4_handle_max_groups] = {}, stop[cc4_handle_max_groups] = {};
};
// batches of up to this many episodes move their step inputs and outputs through pinned staging buffers (fetch_outputs, cc4_step_fetch)
constexpr int PIN_MAX_ENVS = 4096;

// cc4_api.hip: stream ordering, the launches of one step, what a handle asks the device once
CC4_HOST void configure_groups(cc4_handle* h, int ng);
// The prologue of an entry point.  enter_refused: the refusals the entry point asks for, -2 with `who` in front of the reason, or 0.  enter: those, then
// the handle's device and join_groups (-1).  An entry point whose own argument checks stand between its refusals and the join calls the two parts itself.
enum : unsigned { EN_NO_ROLLOUT = 1, EN_NO_COMM = 2 };
CC4_HOST int enter_refused(cc4_handle* h, const char* who, unsigned refuse);
CC4_HOST int enter(cc4_handle* h, const char* who, unsigned refuse = 0);
CC4_HOST int join_groups(cc4_handle* h);
CC4_HOST int fork_groups(cc4_handle* h);
CC4_HOST int copy_to_host(cc4_handle* h, const char* who, void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
CC4_HOST int sync_all(cc4_handle* h);
CC4_HOST int wall_khz(cc4_handle* h);
CC4_HOST int ensure_watchdog_word(cc4_handle* h);
CC4_HOST StepArgs step_args(const cc4_handle* h);
CC4_HOST RunArgs run_args(const cc4_handle* h, int k, uint32_t t0, bool head);
CC4_HOST void launch_group(cc4_handle* h, StepArgs a, int g, bool full, hipEvent_t start, hipEvent_t stop);
CC4_HOST void launch_range(cc4_handle* h, StepArgs a, int e0, int e1, hipStream_t st, bool full, hipEvent_t start, hipEvent_t stop);
CC4_HOST int launch_step(cc4_handle* h, const int32_t* d_actions, const uint8_t* d_msgs, bool rand = false, uint64_t seed0 = 0, uint32_t t = 0, bool ext_uploaded = false, bool api_step = false);
// cc4_api_run.hip: the one-launch forms, the persistent kernel, the self-check's shadow handle
CC4_HOST int choose_run_form(cc4_handle* h, int margin, int persist_margin = -1);
CC4_HOST void enq_pool_stop(cc4_handle* h);
CC4_HOST int persist_setup(cc4_handle* h);
CC4_HOST int persist_launch(cc4_handle* h, StepArgs a, int k, uint32_t t0, const XchgArgs& x, hipEvent_t e0, hipEvent_t e1, bool rollout, const PlanArgs* pl = nullptr);
CC4_HOST int ensure_shadow(cc4_handle* h);
CC4_HOST int verify_digest(cc4_handle* h, std::vector<uint64_t>& out);
// cc4_api_comm.hip: the exchange around a one-launch kernel
CC4_HOST int xchg_begin(cc4_handle* h, int k, XchgArgs* x);
CC4_HOST int xchg_enqueue(cc4_handle* h, int k, const XchgArgs& x, int form);
CC4_HOST int xchg_end(cc4_handle* h, int k);
// cc4_api_debug.hip: the debug reports of cc4_run_random_steps (CC4_PERSIST_TIMELINE, CC4_EXCHANGE_PROF)
CC4_HOST int timeline_report(cc4_handle* h, int k, bool timed);
CC4_HOST void exchange_prof_report(int k, const std::chrono::steady_clock::time_point (&t)[6]);
