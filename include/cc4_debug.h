/* cc4_debug.h -- debug, experiment and test hooks of libcc4.so.  Not part of the drop-in boundary (include/cc4.h): nothing a user of the reference's
 * API needs; tools/ and tests/ call them. */
#ifndef CC4_DEBUG_H
#define CC4_DEBUG_H
#include "cc4.h"
#ifdef __cplusplus
extern "C" {
#endif

/* debug: per-episode cycle counters of the step kernels ([N][128] u64: 16 phase slots, 8 per red agent, then (cycles, count) per red action type; see
 * tools/phase_profile.py, tools/tail_profile.py) */
int cc4_debug_profile(cc4_handle* h, int enable, unsigned long long* out);

/* test hooks: keep the gathered rows of the next `steps` steps exchanged from inside a one-launch kernel (0 frees the log); read `count`
 * of them from step `first` as [count][world*N][CC4_OBS_PACKED_BYTES]; returns the number of steps logged so far. */
int cc4_debug_gather_log(cc4_handle* h, int32_t steps);
int cc4_get_gather_log(cc4_handle* h, uint8_t* out, int32_t first, int32_t count);

/* test hook: from now on every all-gather is preceded, on the communication stream, by a kernel that idles for about `us`
 * microseconds (0: off) -- an exchange slower than the steps, which makes the guard of the observation ring actually wait */
int cc4_debug_comm_delay_us(cc4_handle* h, int us);

/* measurement (tools/valu_phases.py): the per-step launches of k_step_philox1 end behind phase `phase` (1..13: csrc/cc4_philox1_body.h CC4_STOP) and write no
 * row back; 14 = whole steps, still of the full build; 0 = off.  Restore the batch (cc4_set_state / cc4_set_cold) after such a step. */
int cc4_debug_stop_phase(cc4_handle* h, int phase);

/* debug: where a rollout stands (see csrc/cc4_api_debug.hip) */
int cc4_debug_rollout_state(cc4_handle* h, int64_t* out /* [22] */);
/* test hook: the persistent schedule's progress words as if `base` steps had run since they were last cleared (they are cleared when a call would take
 * them past 0x700000): every episode's word = base, no last runner.  Sets up the persistent path if that was not done yet.  -2: no persistent
 * kernel on this handle, a rollout in flight, or base > 0x700000. */
int cc4_debug_persist_base(cc4_handle* h, uint32_t base);
/* test hook: `bytes` bytes of device memory of this handle's device -- e.g. an action slot of a rollout (cc4_rollout_actions), packed observation rows
 * (cc4_rollout_obs_packed) -- copied to the host, behind everything enqueued on the handle's streams. */
int cc4_debug_copy_from_device(cc4_handle* h, void* host_dst, const void* device_src, size_t bytes);
/* test hook: the self-check's shadow handle (CC4_PERSIST_VERIFY / CC4_PERSIST_VERIFY_EVERY: created with the handle's first persistent call), NULL where
 * there is none.  It stays the handle's own: the read-only getters (cc4_get_states, cc4_get_rng_state, cc4_get_err, cc4_fetch, cc4_get_cold) give the
 * shadow's side of the last checked call; it is never stepped, reset or destroyed through this pointer. */
int cc4_debug_shadow_handle(cc4_handle* h, cc4_handle** out);
/* test hook, read-only: which builds this handle's counter-mode launches take -- out[0] 1 = the one-wave step kernel (k_step_philox1), 0 = the four-wave
 * one; out[1] the four-wave step kernel's register budget (k_step_philox<., 1 / 7 / 8>: cc4_step_kernel names all three alike); out[2] the multi-step
 * build (5: k_run_philox, 8: k_run_philox8; meaningful where cc4_run_kernel names one of them). */
int cc4_debug_step_build(cc4_handle* h, int32_t out[3]);
/* test hook, read-only: the runs of steps the most recent launch of a persistent kernel (k_run_philox1 and its kin, k_run_pcg) was cut into -- out[0] steps
 * of a run, out[1] how many of them, out[2] / out[3] the same of the closing runs, out[4] the items of an episode (all zero: no such launch yet).  Only the
 * headline kernel k_run_philox1 takes the long-call pattern (csrc/cc4_sched.h run_config_for_call). */
int cc4_debug_last_run_split(cc4_handle* h, int32_t out[5]);

#ifdef __cplusplus
}
#endif
#endif
