// cc4_k_blue.hip -- blue's own knowledge as device tensors: the kernel beside the step (the definition: cc4_blue_view.h, shared with the host function).
//   k_blue_view   cc4_blue_view_device: one wavefront per requested episode or bank slot, a streaming kernel like k_red_view (the rows are read where
//                 view_rows, cc4_view_src.h, finds them -- a snapshot slot carries the log header, the live log entries and the live sus spans at the
//                 same offsets).
//                   1. the summary is zeroed in LDS: two words per host, a half word per (agent, host), two words per agent -- 2508 bytes, two of the
//                      1280-byte granules LDS is handed out in (cc4_blue_view.h: why not two words per pair);
//                   2. the lanes stride over the entries of the step's event log (when it is valid: at most MAX_EV, 12 bytes each) and over the five sus
//                      lists (at most cold_sus_cap(steps) entries each, 4 bytes each, consecutive lanes consecutive entries): counts and bits go into
//                      the LDS words with LDS atomics;
//                   3. the lanes stride over the 685 (agent, host) rows: one 8-byte store per lane, consecutive lanes, consecutive addresses (5 x 137 is
//                      odd: the block of an odd output index is 8- but not 16-byte aligned, so there is no two-rows-per-store form as in k_red_view);
//                   4. the lanes write the 80 agent words.
//                 The empty output of a refused entry: all-zero rows.
#include "cc4_view_src.h"
#include "cc4_blue_view.h"
#include "cc4_kernel_decls.h"

static_assert(BV_HOSTS == CC4_BLUE_VIEW_HOSTS && BV_PER_HOST == CC4_BLUE_VIEW_PER_HOST && BV_SCALARS == CC4_BLUE_VIEW_SCALARS && NBLUE == CC4_NUM_BLUE &&
              BV_PORT_PID == CC4_BLUE_VIEW_PORT_PID && BV_OWN_DECOY == CC4_BLUE_VIEW_OWN_DECOY, "include/cc4.h states the shapes");

__global__ __launch_bounds__(WAVE) void k_blue_view(BlueViewArgs a) {
  __shared__ uint32_t hw[BV_HW_WORDS];                  // the two summary words of every host
  __shared__ uint32_t rem[BV_REM_WORDS];                // the remote count of every (agent, host), two to a word
  __shared__ uint32_t agt[2 * NBLUE];                   // dec[b], tot[b]
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (i >= a.src.count) return;
  uint2* const out = reinterpret_cast<uint2*>(a.hosts + (size_t)i * BV_HOST_BYTES);
  int32_t* const os = a.scal ? a.scal + (size_t)i * (NBLUE * BV_SCALARS) : nullptr;
  const ViewRows vr = view_rows(a.src, i, lane);        // (wave-uniform: cc4_view_src.h)
  if (vr.fault) {
    for (int k = lane; k < BV_ROWS; k += WAVE) out[k] = make_uint2(0u, 0u);
    if (os) for (int k = lane; k < NBLUE * BV_SCALARS; k += WAVE) os[k] = 0;
    return;
  }
  const EnvState* const s = vr.s;
  const EnvCold* const c = vr.c;
  uint32_t* const dec = agt, * const tot = agt + NBLUE;

  for (int k = lane; k < BV_HW_WORDS; k += WAVE) hw[k] = 0u;
  for (int k = lane; k < BV_REM_WORDS; k += WAVE) rem[k] = 0u;
  if (lane < 2 * NBLUE) agt[lane] = 0u;
  __syncthreads();
  const EvLog* const lg = &c->evlog;
  const bool valid = bv_events_valid(s, lg);
  if (valid) {
    const int n = (int)lg->n;                           // (<= MAX_EV: bv_events_valid)
    for (int k = lane; k < n; k += WAVE) bv_fold_event(s, lg->rec[k], (uint32_t)k, hw, rem, dec, tot);
  }
  for (int b = 0; b < NBLUE; ++b) {
    const uint32_t* const p = cold_sus(c, a.src.steps, b);
    const int n = bv_nsus(s, b, a.src.steps);
    for (int k = lane; k < n; k += WAVE) bv_fold_sus(s, b, p[k], hw);
  }
  __syncthreads();
  for (int k = lane; k < BV_ROWS; k += WAVE) {
    const int b = k / MAXH, h = k - b * MAXH;
    const BvRow row = bv_host_row(s, b, h, hw[2 * h], hw[2 * h + 1], bv_rem_get(rem, k), dec[b]);
    out[k] = make_uint2(row.w[0], row.w[1]);
  }
  if (os) for (int k = lane; k < NBLUE * BV_SCALARS; k += WAVE) os[k] = bv_scalar(s, valid, tot[k / BV_SCALARS], k / BV_SCALARS, k % BV_SCALARS);
}
