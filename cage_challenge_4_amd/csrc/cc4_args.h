// cc4_args.h -- what the host side and the kernels of libcc4.so share: the constants, the argument blocks of the kernels (StepArgs, XchgArgs, RunArgs,
// PlanArgs, ResetArgs, CopyArgs, RedSubmitArgs, and ViewSrc with the six view blocks FeatArgs, RedViewArgs, BlueViewArgs, BlueEdgesArgs, RewardArgs, SampleArgs), the snapshot-slot layout, and the register budgets of the kernels.  No device helper (cc4_kernels.h) and nothing of
// the C++ host library (cc4_host.h).  The index arithmetic of the persistent schedule -- partitions, tickets, runs, the progress word -- is in cc4_sched.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/cc4.h"
#include "cc4_engine.h"
#include "cc4_sched.h"

using namespace cc4;

static_assert(sizeof(EnvState) % 16 == 0 && offsetof(EnvState, hd) % 16 == 0, "EnvState rows are staged with 16-byte accesses");
constexpr int ROW_VEC = (int)(sizeof(EnvState) / 16);
constexpr int HOT_VEC = (int)(offsetof(EnvState, hd) / 16);   // the part in front of the host table
constexpr int WAVE = 64;
constexpr int OBS_PACKED = CC4_OBS_PACKED_BYTES;   // every flat-observation value is 0, 1 or 2: the exchange moves 2 bits per value
static_assert(OBS_PACKED % 4 == 0 && OBS_PACKED * 4 >= OBS_TOTAL, "packed observation row: whole words, four values per byte");
constexpr int PROF_SLOTS = 128;   // 16 phase slots, 8 per red agent (16..63), then (cycles, count) per red action type (64..)

constexpr int cc4_handle_max_groups = 8;   // cc4_handle::MAX_GROUPS

// Register budgets: the minimum waves per SIMD (= resident blocks per CU) the allocation of a kernel must allow -- __launch_bounds__' second argument
#ifndef CC4_PERSIST_MINW
#define CC4_PERSIST_MINW 6        // k_run_philox1, k_run_philox1p: 24 waves per CU
#endif
#ifndef CC4_LEAN_MINW
#define CC4_LEAN_MINW 1           // k_step_philox1
#endif
#ifndef CC4_SMALL_MINW
#define CC4_SMALL_MINW 1          // k_step_philox of small batches (cc4_k_philox4.hip: MINW)
#endif
#ifndef CC4_PHILOX_BIG_MINW
#define CC4_PHILOX_BIG_MINW 7     // k_step_philox of large ones
#endif

struct StepArgs {
  EnvState* st; EnvCold* cold;
  const int32_t* actions; const uint8_t* msgs;
  int32_t* obs; float* reward; uint8_t* done; uint32_t* err;
  uint8_t* obs8;               // the same observations packed 2 bits per value, OBS_PACKED bytes per episode (what the multi-GPU
                               // all-gather moves), or null
  int32_t* rand_out;           // when non-null: draw the blue actions in-kernel (k_random_actions fused) and record them here
  uint64_t rand_seed0; uint32_t rand_t;
  int n, autoreset, steps, rng_mode, policy;
  int full_obs;               // rewrite every observation value (the output buffer may hold another episode's slowly varying part)
  uint32_t topo;              // cc4_config.topology_seed
  unsigned long long* prof;   // optional [n][PROF_SLOTS] cycle counters (cc4_debug_profile): 16 phase slots + 8 per red agent
  uint32_t* reset_ws;         // k_step_philox1: [n][RESET_WS_WORDS] work area of the in-kernel scenario generation (the other
                              // kernels keep it in LDS; an episode regenerates once in steps-per-episode launches)
  const ExtAct* ext;          // [n][EXT_PER_ENV] externally submitted red / green actions of this step (cc4_step_ex), or null; read by the
                              // full builds of the step kernels only (template parameter LOG)
  int e0;                     // first episode of this launch: block b steps episode e0 + b (a step of a large batch is issued as
                              // several launches on separate streams: see cc4_handle::ngroups); n = one past its last episode
  int act_sys;                // the actions were written by ANOTHER kernel while this one runs (a rollout, RunArgs.act_ready): system-scope loads,
                              // past this XCD's L2, which may still hold the line from two steps ago
  int dbg_stop;               // measurement (cc4_debug_stop_phase, full build of k_step_philox1 only): the step ends after its phase number dbg_stop and
                              // writes no row back -- the instruction counters of such launches, differenced, are the instructions of each phase
};

// The per-step hand-off out of the one-launch kernels (cc4_run_random_steps with a communicator).  Step k of the launch writes
// its packed rows into slab k % ring and, once an episode's row is in memory, counts it in its group's counter of that step (a no-return
// atomic: nothing waits for it); on the communication stream a one-block gate kernel (k_xchg_gate) waits until every group has counted
// every step of a chunk, the chunk's slabs are gathered, and gathered = last + 1 is published (hipStreamWriteValue32); step k + ring of any
// episode waits for gathered > k before it overwrites the slab.  The exchange lags the stepping by up to `ring` steps, with no launch
// boundary in the compute queue.  A wait that lasts longer than wait_ticks gives up, raises *timeout (the host falls back to per-step
// launches and says so) and every later wait of the launch returns at once: a stuck exchange never hangs the kernel.
struct XchgArgs {
  uint8_t* slab;                 // [ring][n][OBS_PACKED], or null: no exchange
  uint32_t* gathered;            // [1]
  uint32_t* timeout;             // [1]
  int ring;
  long long wait_ticks;          // wall_clock64 ticks (100 MHz)
  uint32_t* gcnt;                // [groups][ring]: episodes of a group that finished step k (slot k % ring), see xchg_count
  uint32_t* timeout_host;        // the same flag in pinned host memory, WRITTEN only (the host reads it without a copy; the waits poll the
                                 // device word: a thousand blocks polling a word across PCIe cost a 1024-episode batch 12 us per step)
};

// ---- the persistent kernels (cc4_persist.h: persist_loop): K steps of the whole batch in ONE launch.
// A step-per-launch schedule ends every launch with a tail (its last blocks run on a half-empty chip) and starts the next with a
// ramp; cutting the batch into four groups on four streams hides most of that, not all: 8192 episodes x 29.6 us of
// dependent work per episode-step over 5120 resident waves would take 47.4 us per step, four launches take 53.4.  Here the grid is
// one wave per residency slot, and every wave pulls items until the K steps of all episodes are done -- no launch boundary inside,
// no tail but the last one.
//  * Partitions.  The batch is cut into one partition per CU (episode e -> partition e % P, P = the CUs the device showed at first use,
//    numbered in slot order); a wave reads its CU's identity from the hardware (cu_slot) and finds the CU's partition in slot_part.
//    A CU's vector L1 is never refreshed by another CU's stores, and the XCDs' L2s are not coherent with each other
//    (MI355X_MICROARCH.md, "inter-workgroup visibility"): an episode normally stays on ONE CU, whose waves share its write-through L1,
//    so the hand-over between two of them needs ordering only -- the writer drains its stores (s_waitcnt vmcnt(0)) before it publishes.
//  * Items.  An item is a RUN of consecutive steps of one episode: nA runs of SA steps, then nB of SB, then single steps (nph runs in
//    all, K steps).  Inside a run the agent part stays in LDS -- no write-back and re-stage between the steps, one ticket, one progress
//    wait and one store drain per run instead of per step; the short runs at the end keep the launch's tail one step long.
//  * Order per episode.  A partition's ticket counter hands its runs out in the order (run 0 of its episodes, run 1, ..): a run may
//    start once progress[e] says the steps before it are done, which the wave that ran them stores when their rows are back in memory.
//    With 32 episodes and 20 waves per CU the predecessor finished a dozen tickets ago; the wait is a single load, normally.
//  * Balance inside the XCD.  A wave looks at the ticket counters of its XCD's partitions before every run and, when its own partition
//    is more than `thr` tickets AHEAD of the one that lags most -- or handed out --, takes its run from that one.  The partitions of an
//    XCD so finish within a run of each other.  An episode's progress word carries, beside the steps done, the id of the CU that ran
//    its last run: a run on ANOTHER CU than that one starts with an agent-scope acquire (buffer_inv sc1: tools/micro/l1_inv_scope.hip --
//    nothing less drops a CU's stale L1 lines; profiles/r06_l1_inv_scope.txt), a run on the same CU with none.  Never across XCDs.
//  * No memset between calls.  The ticket counters exist twice, one set per call parity: the wave that draws a partition's last ticket
//    clears its counter of the other parity; progress[] counts steps since the handle last cleared it (`base` = where every episode
//    stands when the call starts).
// The mappings themselves -- episode <-> partition and policy group, ticket -> (run, episode), the runs of K steps, the fields of a progress word and their
// limits -- are defined ONCE, in cc4_sched.h: kernels, gates, host and the CPU oracle compile the same functions (tests/test_sched_cpu.py).
// (The schedules before this one -- owned partitions with stealing, per-XCD pools -- are in docs/HISTORY.md.)
struct RunArgs {
  // ---- constant for a handle (run_args)
  uint32_t* progress;          // [n] progress_pack (cc4_sched.h): the steps episode e has completed since the words were cleared | the runner of its last
                               // run (1 + the partition of that CU; RUNNER_NONE: none yet)
  const int32_t* slot_part;    // [CC4_SLOTS] CU slot id -> 1 + its partition, 0 = no such CU on this device (k_discover at first use: partitions in
                               // slot order, so the CUs of an XCD own neighbouring partitions and their ticket / progress words share cache lines
                               // only with each other -- handed out in arrival order they interleave the XCDs, and a 20-step call was 6 % slower)
  int P, K;
  int G;                       // the exchange counts episode e in group e % G (the gate kernel's groups: G = the CUs of the device)
  uint32_t t0;                 // action time of step 0 (random_blue_action)
  RunSplit runs;               // the runs of this call's K steps: SA, nA, SB, nB, nph (run_split)
  uint8_t xcc_lo[8], xcc_n[8]; // XCC id -> first partition / number of partitions of that XCD
  int thr;
  // ---- per call (persist_launch)
  uint32_t* ticket;            // this call's ticket counters: partition p's line at word p * TK_STRIDE
  uint32_t* ticket_next;       // the other parity's
  uint32_t base;
  unsigned long long* timeline; // debug (CC4_PERSIST_TIMELINE=1): per wave [entry, first item start, last item end, items] in wall_clock64 ticks, or null
  // ---- rollouts with the policy in the loop (cc4_rollout_begin): the blue actions of step j are written, while this launch runs, by kernels of
  // the caller's on the caller's stream -- one policy group of episodes at a time: group of e = (e / P) % PG, so every CU holds episodes of every
  // group and works on one group while another waits for its policy.  Step j of an episode of group g starts once act_ready[g] > j (published by
  // the caller behind its policy kernels, cc4_rollout_publish); it reads slot j % 2 of `act` with system-scope loads, writes its packed
  // observation row into slab j % ring with system-scope stores (XchgArgs.slab) and counts itself in cnt[(e % P) * PG + g][j % ring] once that
  // row is in memory -- what the gate of the caller's next policy pass waits for (cc4_rollout_wait_obs).  Every step is an item of its own, and
  // every (partition, policy group) has a ticket counter of its own (words 0 .. PG-1 of the partition's ticket line).
  const uint32_t* act_ready;   // [P][32 words]: one cache line per CU partition, word g = the steps of policy group g whose actions are published -- the
                               // publisher writes all P copies, a wave polls its own CU's (thousands of waves polling ONE uncached line starve the very
                               // store they wait for: ~50 us per pass, profiles/r06_rollout.txt); null: no rollout
  const int32_t* act;          // [2][n][5]
  int PG;
  long long act_wait_ticks;    // watchdog: a step that waits longer for its actions gives up, raises XchgArgs.timeout, and every later wait returns at once
};
constexpr int TK_STRIDE = 32;      // words between two partitions' ticket counters (a cache line of their own each)
constexpr int CC4_SLOTS = 2048;    // CU slot ids (cu_slot): (XCC id << 8) | HW_ID[15:8]
constexpr int RPG_MAX = 4;         // policy groups of a rollout (cc4_handle::rpg of them, CC4_ROLLOUT_GROUPS): group of episode e = (e / P) % groups -- the others step while one group's policy pass is under way

// cc4_run_plan_device in one launch (persist_loop<.., PLAN>): the caller's plan and trajectory, all on the device, one row of the whole batch per step
struct PlanArgs {
  const int32_t* actions;      // [K][n][5] wrapper indices: step j reads row j
  const uint8_t* msgs;         // [K][n][5][8], or null
  float* rewards;              // [K][n], or null: every step writes the handle's reward buffer as always
  uint8_t* dones;              // [K][n], or null
  uint8_t* obs_packed;         // [K][n][OBS_PACKED], or null: the packed observation row after every step
  uint32_t* err_or;            // [n] the error flags any step of the call raised (zero between calls: k_plan_finish moves them into the handle's error words)
};
constexpr uint32_t PLAN_REGEN = 0x80000000u;   // ... and, beside the E_* flags, "a step of the call regenerated the episode" (autoreset): k_plan_finish marks its mask row stale

struct ResetArgs {
  EnvState* st; EnvCold* cold; const uint64_t* seeds; const uint8_t* env_mask;
  int32_t* obs; float* reward; uint8_t* done; uint32_t* err; uint8_t* mask;
  int n, steps, rng_mode, policy;
  uint32_t topo;
  uint8_t* obs8;               // packed exchange row of the reset observations (multi-GPU), or null
};

// ---- episode copies (cc4_copy_episodes_device, cc4_k_copy.hip).  A snapshot slot of a bank: [SlotHdr | hot row | cold row (padded to 64 bytes) |
// outputs: packed observation row, reward, error word, done (padded to 64 bytes)]; offsets only, no pointers: a bank may travel through host memory.
struct alignas(16) SlotHdr {
  uint32_t magic, version;     // SLOT_MAGIC / SLOT_VERSION: a slot that was never written has neither
  int32_t steps, rng_mode;     // of the handle that wrote it: a load into a handle of another configuration is refused
  uint32_t claim;              // phase 1 of a save claims its destination slots here (0 once written)
  uint32_t pad[11];
};
static_assert(sizeof(SlotHdr) == 64, "64-byte slot header");
constexpr uint32_t SLOT_MAGIC = 0x45344343u;   // "CC4E"
constexpr uint32_t SLOT_VERSION = (1u << 24) | (uint32_t)((sizeof(EnvState) + sizeof(EnvCold)) & 0xFFFFFFu);   // a layout change changes it
constexpr size_t SLOT_OUT_BYTES = 192;         // OBS_PACKED + reward + err + done, rounded up to 64
CC4_HD size_t slot_cold_off() { return sizeof(SlotHdr) + sizeof(EnvState); }
CC4_HD size_t slot_out_off(size_t cold_row) { return slot_cold_off() + ((cold_row + 63) & ~(size_t)63); }
CC4_HD size_t slot_bytes(size_t cold_row) { return slot_out_off(cold_row) + SLOT_OUT_BYTES; }
static_assert(OBS_PACKED + 12 <= (int)SLOT_OUT_BYTES && sizeof(SlotHdr) % 64 == 0 && sizeof(EnvState) % 64 == 0, "slot layout");
enum : uint32_t { CF_RANGE = CC4_COPY_RANGE, CF_DUP_DST = CC4_COPY_DUP_DST, CF_SRC_IS_DST = CC4_COPY_SRC_IS_DST, CF_SLOT_EMPTY = CC4_COPY_SLOT_EMPTY,
                  CF_SLOT_CONFIG = CC4_COPY_SLOT_CONFIG };   // cc4_copy_faults bits
// The test of a slot's header before anything reads the slot: 0, or the fault bit of a slot that was never written / that a handle of another
// configuration wrote (the derived views' view_rows and k_copy_episodes)
CC4_HD uint32_t slot_hdr_fault(const SlotHdr* hdr, int steps, int rng_mode) {
  if (hdr->magic != SLOT_MAGIC || hdr->version != SLOT_VERSION) return CF_SLOT_EMPTY;
  return hdr->steps != steps || hdr->rng_mode != rng_mode ? CF_SLOT_CONFIG : 0u;
}
struct CopyArgs {
  EnvState* st; EnvCold* cold; size_t cold_row;          // the handle's episodes
  int32_t* obs; float* reward; uint8_t* done; uint32_t* err; uint8_t* mask; uint8_t* mask_stale;
  uint32_t* claim;                                       // [n] claim words of the handle's episodes
  const uint8_t* src_bank; uint8_t* dst_bank; size_t slot;   // banks (null: the handle's episodes), bytes per slot
  const int32_t* src; const int32_t* dst; const uint64_t* seeds;
  int count, n, src_cap, dst_cap, steps, rng_mode, evlog_on;
  uint32_t stamp;                                        // this call's claims: 2 * stamp (one entry names it), 2 * stamp + 1 (several)
  uint32_t* fault;
};

// ---- the derived views (cc4_state_features_device, cc4_red_view_device, cc4_blue_view_device, cc4_blue_edges_device, cc4_reward_terms_device,
// cc4_sample_actions_device): kernels
// that read tensors out of the batch without stepping it, one wavefront per entry.  Their common call shape, stated once: entry i reads episode
// ids[i] (null: i) of the handle -- its hot row and, at cold_at(cold, e, cold_row), its cold row -- or the two rows inside slot ids[i] of a snapshot
// bank; an index out of range, a slot that was never written or one of another configuration gives the view's empty output and raises its CF_* bit in
// the handle's fault word.  ViewSrc is that source, the first member of every view's argument block; view_rows (cc4_kernels.h) resolves an entry.
struct ViewSrc {
  const EnvState* st; const EnvCold* cold; size_t cold_row;   // the handle's rows (bank == null)
  const uint8_t* bank; size_t slot;                      // or a snapshot bank and the bytes per slot
  const int32_t* ids;                                    // [count] or null
  int count, cap, steps, rng_mode;                       // cap: episodes of the handle / slots of the bank
  uint32_t* fault;
};
// state features (cc4_k_feat.hip; the definition: cc4_features.h): the hot row only
struct FeatArgs {
  ViewSrc src;
  uint8_t* hosts;                                        // [count][137][16], 16-byte aligned
  int32_t* glob;                                         // [count][32] or null
};

// ---- the red agents as learners (cc4_k_red.hip; the definition: cc4_red_view.h).  cc4_step_red_device: red[e][r] = (type, host, arg, session) becomes
// record r of ext[e]; clear_green: the green records of every episode are set to none as well.
struct RedSubmitArgs {
  const EnvState* st;                                    // the handle's hot rows as they stand before the step (CC4_RED_SID_AUTO)
  const int32_t* red;                                    // [n][NRED][4], 16-byte aligned
  ExtAct* ext;                                           // [n][EXT_PER_ENV]
  int n, clear_green;
  uint32_t* fault;
};
// what each red agent knows (the same file and definition): the hot row only
struct RedViewArgs {
  ViewSrc src;
  uint8_t* hosts;                                        // [count][NRED][137][8], 16-byte aligned
  int32_t* scal;                                         // [count][NRED][16] or null
};
// blue's own knowledge (cc4_k_blue.hip; the definition: cc4_blue_view.h): of the cold row the event log and the sus lists
struct BlueViewArgs {
  ViewSrc src;
  uint8_t* hosts;                                        // [count][NBLUE][137][8], 8-byte aligned
  int32_t* scal;                                         // [count][NBLUE][16] or null
};
// the Monitor's connections as edge lists (cc4_k_edges.hip; the definition: cc4_blue_edges.h): of the cold row the event log
struct BlueEdgesArgs {
  ViewSrc src;
  int max_edges;
  int32_t* edges;                                        // [count][max_edges][8], 16-byte aligned
  int32_t* counts;                                       // [count][8] or null
};
// reward terms (cc4_k_reward.hip; the definition: cc4_reward_terms.h): of the hot row about 150 bytes, of the cold row the 64-byte record EnvCold.rwd
struct RewardArgs {
  ViewSrc src;
  int32_t* terms;                                        // [count][9][4], 16-byte aligned
  int32_t* words;                                        // [count][16], 16-byte aligned, or null
};
// masked sampling of the blue actions from policy logits (cc4_k_sample.hip; the definition: cc4_sample.h): of the hot row the exists bits and the agents'
// busy bytes; beside the rows one input, the logits
struct SampleArgs {
  ViewSrc src;
  const void* logits;                                    // [count][570] in dtype, row i belongs to entry i, 4-byte aligned; or null: all zero
  int dtype;                                             // 1 float16, 2 bfloat16, 3 float32 (the codes of cc4_policy_outputs)
  uint64_t seed0; uint32_t t;                            // the noise: Philox key seed0 + the entry's id, counter word t
  float inv_t;                                           // 1 / temperature
  int flags;                                             // CC4_SAMPLE_*
  int32_t* actions;                                      // [count][5], 4-byte aligned
  float* stats;                                          // [count][5][2] (logp, entropy) or null
};
