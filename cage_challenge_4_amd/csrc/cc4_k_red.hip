// cc4_k_red.hip -- the red agents as learners: the two kernels beside the step (the definition of both: cc4_red_view.h, shared with the host functions).
//   k_red_submit  cc4_step_red_device: one lane per (episode, red agent) turns the caller's four words into the agent's ExtAct record of the handle's
//                 d_ext -- validated (a refused record becomes XA_NONE and raises CF_RANGE), CC4_RED_SID_AUTO resolved from the episode's row as it stands
//                 before the step -- and, when the buffer may hold green records of an earlier cc4_step_ex, sets the episode's green records to none
//                 (lane r those of green agents r, r + 6, ..).  The step kernels then read the records as they read uploaded ones.
//   k_red_view    cc4_red_view_device: one wavefront per requested episode, a streaming kernel like k_state_features (the row is read where
//                 view_rows, cc4_view_src.h, finds it).
//                   1. the lanes stride over the six agents' session lists (6 x 64 entries) and observation entries (6 x 32): sessions per (agent, host),
//                      "a root session", "an abstract session" and the observation byte go into one LDS word per pair with LDS atomics;
//                   2. the lanes stride over the 822 (agent, host) rows two at a time: one 16-byte store per lane, consecutive lanes, consecutive addresses;
//                   3. lanes 0..63 and 0..31 write the 96 agent words.
//                 The empty output of a refused entry: all-zero rows.
#include "cc4_view_src.h"
#include "cc4_red_view.h"
#include "cc4_kernel_decls.h"

static_assert(RV_HOSTS == CC4_RED_VIEW_HOSTS && RV_PER_HOST == CC4_RED_VIEW_PER_HOST && RV_SCALARS == CC4_RED_VIEW_SCALARS && RED_ACT_WORDS == CC4_RED_ACT_WORDS &&
              RED_SID_AUTO == CC4_RED_SID_AUTO && NRED == CC4_NUM_RED, "include/cc4.h states the shapes");

__global__ __launch_bounds__(256) void k_red_submit(RedSubmitArgs a) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= a.n * NRED) return;
  const int e = i / NRED, r = i - e * NRED;
  const int4 v = reinterpret_cast<const int4*>(a.red)[i];             // type, host, arg, session
  ExtActW rec;
  if (!red_record(a.st + e, r, v.x, v.y, v.z, v.w, &rec)) atomicOr(a.fault, CF_RANGE);
  uint64_t* const row = reinterpret_cast<uint64_t*>(a.ext + (size_t)e * EXT_PER_ENV);
  uint64_t* o = row + 3 * r;
  o[0] = rec.w[0]; o[1] = rec.w[1]; o[2] = rec.w[2];
  if (a.clear_green)
    for (int g = r; g < MAXG; g += NRED) { o = row + 3 * (NRED + g); o[0] = ~0ull; o[1] = ~0ull; o[2] = ~0ull; }
}

__global__ __launch_bounds__(WAVE) void k_red_view(RedViewArgs a) {
  __shared__ uint32_t sum[NRED * MAXH];                 // the summary word of every (agent, host)
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (i >= a.src.count) return;
  uint4* const out = reinterpret_cast<uint4*>(a.hosts + (size_t)i * RV_HOST_BYTES);
  int32_t* const os = a.scal ? a.scal + (size_t)i * (NRED * RV_SCALARS) : nullptr;
  const ViewRows vr = view_rows(a.src, i, lane);        // (wave-uniform: cc4_view_src.h)
  if (vr.fault) {
    for (int k = lane; k < RV_HOST_VECS; k += WAVE) out[k] = make_uint4(0u, 0u, 0u, 0u);
    if (os) for (int k = lane; k < NRED * RV_SCALARS; k += WAVE) os[k] = 0;
    return;
  }
  const EnvState* const s = vr.s;

  for (int k = lane; k < NRED * MAXH; k += WAVE) sum[k] = 0u;
  __syncthreads();
  for (int k = lane; k < NRED * MAX_RS; k += WAVE) {
    const int r = k / MAX_RS;
    int h; uint32_t fl;
    if (!rv_sess_item(s, r, k - r * MAX_RS, &h, &fl)) continue;
    atomicAdd(&sum[r * MAXH + h], (uint32_t)RVS_ONE);
    if (rv_sess_bits(fl)) atomicOr(&sum[r * MAXH + h], rv_sess_bits(fl));
  }
  for (int k = lane; k < NRED * MAX_OBS; k += WAVE) {
    const int r = k / MAX_OBS;
    int h; uint32_t fl;
    if (rv_obs_item(s, r, k - r * MAX_OBS, &h, &fl)) atomicOr(&sum[r * MAXH + h], rv_obs_bits(fl));
  }
  __syncthreads();
  static_assert((NRED * MAXH) % 2 == 0 && RV_HOST_VECS * 2 == NRED * MAXH, "two (agent, host) rows per 16-byte store");
  for (int k = lane; k < RV_HOST_VECS; k += WAVE) {
    const int p = 2 * k, q = p + 1;
    const RvRow lo = rv_host_row(s, p / MAXH, p % MAXH, sum[p]), hi = rv_host_row(s, q / MAXH, q % MAXH, sum[q]);
    out[k] = make_uint4(lo.w[0], lo.w[1], hi.w[0], hi.w[1]);
  }
  if (os) for (int k = lane; k < NRED * RV_SCALARS; k += WAVE) os[k] = rv_scalar(s, k / RV_SCALARS, k % RV_SCALARS);
}
