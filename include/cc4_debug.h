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

/* ---- The self-check's digest (CC4_PERSIST_VERIFY / CC4_PERSIST_VERIFY_EVERY, include/cc4.h cc4_verify_stats): what a checked call compares.
 *
 * Both sides of a checked call -- the handle after its one-launch kernel, the shadow handle after its per-step launches -- are reduced to THREE
 * unsigned 64-bit words per episode: word 0 of the hot row, word 1 of the cold row, word 2 of the outputs.  A side's words are [N][3].  Episode e
 * disagrees where word i of the one side differs from word i of the other: i = 0 is reported as "hot row", 1 as "cold row", 2 as "outputs".
 * All arithmetic is modulo 2^64.
 *
 *   mix(h, v) = (h XOR (v + 0x9E3779B97F4A7C15 + (h << 6) + (h >> 2))) * 0xD6E8FEB86659FD93      (the shifts of h as it came in, logical)
 *
 *   A ROW WORD.  The row is nv = bytes / 16 vectors of 16 bytes (hot row: cc4_state_bytes(); cold row: cc4_cold_bytes(h); both multiples of 16).
 *   Vector i is four little-endian 32-bit words x, y, z, w at its bytes 0, 4, 8, 12.  There are 64 lanes.  Lane L starts from
 *   h = 0x1234567 + L and takes the vectors i = L, L + 64, L + 128, ... < nv in ascending order; for each, h = mix(h, x * 2^32 + y) and then
 *   h = mix(h, z * 2^32 + w).  Behind its last vector every lane -- one that had no vector too -- closes with h = mix(h, L).  The row word is the sum of
 *   the 64 lanes' h.
 *
 *   THE OUTPUTS WORD.  Lane L starts from h = 0x89ABCDEF + L and takes the episode's 578 observation values (int32, as cc4_get_obs gives them) of
 *   index i = L, L + 64, ... < 578 in ascending order: h = mix(h, value as an unsigned 32-bit number).  Then lanes 0..4 take one more value each:
 *   lane b the action index of blue agent b in the handle's action buffer (cc4_get_actions, int32 as unsigned 32 bits).  Then lane 8 takes two more:
 *   the reward's float32 bit pattern as an unsigned 32-bit number, then done * 2^32 + err (done: the byte of cc4_fetch, err: the episode's error
 *   word).  Then every lane closes with h = mix(h, L).  The outputs word is the sum of the 64 lanes' h.
 *   (The closing round: without it the last value of a lane moved the sum by an amount that did not depend on the lane, and equal changes in two lanes'
 *   last values gave equal words, opposite ones cancelled.)
 *
 * cc4_debug_digest_rows: the three words on the host from one episode's rows and outputs (csrc/cc4_digest.h, the code k_digest runs, lanes in a
 *   loop); needs no device and no handle.  -2: a NULL argument, cold_bytes no multiple of 16.
 * cc4_debug_digest: the kernel over this handle's episodes as they stand ([N][3]); changes nothing a step reads. */
int cc4_debug_digest_rows(const void* hot_row, const void* cold_row, size_t cold_bytes, const int32_t* obs /* [578] */,
                          float reward, uint8_t done, uint32_t err, const int32_t* actions /* [5] */, uint64_t out[3]);
int cc4_debug_digest(cc4_handle* h, uint64_t* out /* [N][3] */);
/* test hook: arms ONE planted difference for the next CHECKED call of this handle (unchecked calls leave it armed; part -1 disarms; arming replaces
 * what was armed, a refused call of this hook leaves nothing armed).  After both sides have run and before they are digested / their trajectory rows
 * compared, one byte of the SHADOW's side is XORed with 1:
 * part 0 hot row byte `offset` of episode `env`; 1 cold row byte `offset`; 2 the low byte of observation value `offset` (0..577); 3 the reward's low
 * byte; 4 done; 5 the error word's low byte; 6 the low byte of drawn action `offset` (0..4); 7 / 8 / 9 (plan calls only) the shadow's recorded reward
 * (low byte) / done / packed-row byte `offset` (0..147) of plan step `step`.  offset is 0 for parts 3, 4, 5, 7, 8, step is 0 for parts 0..6.
 * The byte lies in memory that only the digest and the host's compare read before the next checked call re-seeds the shadow from this handle: it is
 * never stepped, never written to this handle, and no kernel takes another path for it.  The checked call then returns -5 as for any disagreement.
 * -2 from this hook: out of range, a shadow handle, a handle with a communicator, a handle none of whose calls is ever checked (CC4_PERSIST_VERIFY
 * unset and CC4_PERSIST_VERIFY_EVERY=0).  A checked call that meets an armed part 7 / 8 / 9 it cannot apply -- cc4_run_random_steps, a plan call of
 * `step` steps or fewer, a plan call that does not record that row -- steps nothing, disarms it and returns -2. */
int cc4_debug_verify_plant(cc4_handle* h, int32_t part, int32_t env, int64_t offset, int32_t step);

/* What the handles of this process hold: out[0] device blocks, out[1] pinned host blocks, out[2] events, out[3] streams -- every live handle's (shadow
 * handles of the self-check among them) and the call-local device blocks of calls in flight.  A handle registers what it allocates, whichever call
 * does so and however late, and cc4_destroy releases all of it: the counts are back where they stood once the handles made since are destroyed. */
int cc4_debug_live_resources(int64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
