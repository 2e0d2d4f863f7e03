// cc4_k_feat.hip -- the privileged global state of the batch as tensors (cc4_state_features_device): k_state_features, one wavefront per requested
// episode.  The definition is cc4_features.h, shared with the host function; this file only walks it with 64 lanes.
//   1. the lanes stride over the 192 records of the session pool (spool_used says which are live) and over the green agents: sessions per host,
//      "a root session is here" and "a green agent lives here" go into 147 words of LDS with LDS atomics;
//   2. the lanes stride over the hosts: the second 32 bytes of the HostDyn row (svcs, nproc, nsf) as two 16-byte loads, the host's 16 bytes as
//      one 16-byte store -- consecutive lanes, consecutive hosts;
//   3. lanes 0..31 write the episode words.
// A streaming kernel: the hot row is read where view_rows (cc4_view_src.h) finds it, nothing is staged.  The empty output of a refused entry: an
// all-zero row.
#include "cc4_view_src.h"
#include "cc4_features.h"
#include "cc4_kernel_decls.h"

static_assert(FEAT_HOSTS == CC4_FEAT_HOSTS && FEAT_PER_HOST == CC4_FEAT_PER_HOST && FEAT_GLOBAL == CC4_FEAT_GLOBAL, "include/cc4.h states the shapes");

__global__ __launch_bounds__(WAVE) void k_state_features(FeatArgs a) {
  __shared__ uint32_t sum[MAXH + 10];                   // sessions per host, then the two host bitmaps
  uint32_t* const cnt = sum; uint32_t* const rootm = sum + MAXH; uint32_t* const greenm = sum + MAXH + 5;
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (i >= a.src.count) return;
  uint4* const out = reinterpret_cast<uint4*>(a.hosts + (size_t)i * (FEAT_HOSTS * FEAT_PER_HOST));
  int32_t* const og = a.glob ? a.glob + (size_t)i * FEAT_GLOBAL : nullptr;
  const ViewRows vr = view_rows(a.src, i, lane);        // (wave-uniform: cc4_view_src.h)
  if (vr.fault) {
    for (int h = lane; h < FEAT_HOSTS; h += WAVE) out[h] = make_uint4(0u, 0u, 0u, 0u);
    if (og && lane < FEAT_GLOBAL) og[lane] = 0;
    return;
  }
  const EnvState* const s = vr.s;

  for (int k = lane; k < MAXH + 10; k += WAVE) sum[k] = 0u;
  __syncthreads();
  for (int k = lane; k < RS_POOL; k += WAVE) {
    int h; bool root;
    if (!feat_sess_item(s, k, &h, &root)) continue;
    atomicAdd(&cnt[h], 1u);
    if (root) atomicOr(&rootm[h >> 5], 1u << (h & 31));
  }
  for (int g = lane; g < MAXG; g += WAVE) {
    const int h = feat_green_item(s, g);
    if (h >= 0) atomicOr(&greenm[h >> 5], 1u << (h & 31));
  }
  __syncthreads();
  for (int h = lane; h < FEAT_HOSTS; h += WAVE) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (bit_get(s->exists, h)) {
      const uint4* row = reinterpret_cast<const uint4*>(&s->hd[h]) + 2;
      const uint4 lo = row[0], hi = row[1];
      const uint32_t hd[FEAT_HD_WORDS] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
      const FeatRow r = feat_host_row(s, h, hd, cnt[h], bit_get(rootm, h), bit_get(greenm, h));
      v = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    }
    out[h] = v;
  }
  if (og && lane < FEAT_GLOBAL) og[lane] = feat_global_word(s, lane);
}
