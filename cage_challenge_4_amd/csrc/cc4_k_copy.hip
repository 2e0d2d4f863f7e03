// cc4_k_copy.hip -- episode copies (cc4_copy_episodes_device): clone, save into a bank, load from a bank.
//
// A copy makes the destination behave as the source: the hot row whole, the cold row on its live extents (cold_live_span, cc4_state.h),
// and the outputs of the last step (observation row, reward, done, error word).  Two launches on the handle's main stream:
//   k_copy_claim     one lane per entry: the entry's destination is claimed with this call's stamp (2 * stamp: one entry names it,
//                    2 * stamp + 1: several do).  Claim words: the handle's [n] array for its own episodes, SlotHdr.claim for a bank slot.
//   k_copy_episodes  one workgroup per entry.  Entries with an index out of range, a duplicated destination, a source that is also a
//                    destination of the call, or a bank slot that was never written / comes from another configuration are skipped and
//                    say so in the fault word (CF_*).  The others copy; no two of them write the same row, and none reads a row another writes.
#include "cc4_kernels.h"
#include "cc4_kernel_decls.h"

constexpr int CT = 256;                          // threads per entry (four waves)
constexpr int SPAN_PER_LANE = (COLD_SPANS + WAVE - 1) / WAVE;   // spans one lane of wave 0 computes (contiguous), 6

__global__ __launch_bounds__(256) void k_copy_claim(CopyArgs a) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= a.count) return;
  const int s = a.src[i], d = a.dst[i];
  if (s < 0 || s >= a.src_cap || d < 0 || d >= a.dst_cap) return;          // (reported by phase 2)
  uint32_t* w = a.dst_bank ? &reinterpret_cast<SlotHdr*>(a.dst_bank + (size_t)d * a.slot)->claim : a.claim + d;
  const uint32_t once = 2u * a.stamp, many = once + 1u;
  uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const uint32_t want = (old == once || old == many) ? many : once;    // (any other value is a claim of an earlier call)
    if (old == want) break;
    const uint32_t prev = atomicCAS(w, old, want);
    if (prev == old) break;
    old = prev;
  }
}

__device__ __forceinline__ void copy_words(uint32_t* d, const uint32_t* s, int nw, int t, int nt) {
  for (int k = t; k < nw; k += nt) d[k] = s[k];
}

__global__ __launch_bounds__(CT) void k_copy_episodes(CopyArgs a) {
  __shared__ uint32_t sp_off[COLD_SPANS], sp_len[COLD_SPANS], sp_cum[COLD_SPANS + 1];   // byte offset, bytes, first 16-byte vector of each span
  __shared__ int ok;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & (WAVE - 1);
  if (i >= a.count) return;
  const int s = a.src[i], d = a.dst[i];
  const uint32_t once = 2u * a.stamp, many = once + 1u;
  if (t == 0) {
    uint32_t f = 0;
    if (s < 0 || s >= a.src_cap || d < 0 || d >= a.dst_cap) f = CF_RANGE;
    else {
      const uint32_t dc = a.dst_bank ? __hip_atomic_load(&reinterpret_cast<const SlotHdr*>(a.dst_bank + (size_t)d * a.slot)->claim, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                     : __hip_atomic_load(a.claim + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (dc == many) f |= CF_DUP_DST;
      if (!a.src_bank && !a.dst_bank) {           // a clone: the source must not be overwritten by another entry of the call
        const uint32_t sc = __hip_atomic_load(a.claim + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (sc == once || sc == many) f |= CF_SRC_IS_DST;
      }
      if (a.src_bank) f |= slot_hdr_fault(reinterpret_cast<const SlotHdr*>(a.src_bank + (size_t)s * a.slot), a.steps, a.rng_mode);
    }
    if (f) atomicOr(a.fault, f);
    ok = f == 0;
  }
  __syncthreads();
  if (!ok) return;
  const EnvState* hs = a.src_bank ? reinterpret_cast<const EnvState*>(a.src_bank + (size_t)s * a.slot + sizeof(SlotHdr)) : a.st + s;
  const uint8_t* cs = a.src_bank ? a.src_bank + (size_t)s * a.slot + slot_cold_off() : reinterpret_cast<const uint8_t*>(cold_at(a.cold, (size_t)s, a.cold_row));
  EnvState* hd = a.dst_bank ? reinterpret_cast<EnvState*>(a.dst_bank + (size_t)d * a.slot + sizeof(SlotHdr)) : a.st + d;
  uint8_t* cd = a.dst_bank ? a.dst_bank + (size_t)d * a.slot + slot_cold_off() : reinterpret_cast<uint8_t*>(cold_at(a.cold, (size_t)d, a.cold_row));

  // wave 0: the live spans of the source's cold row (from its hot row's counts) and their prefix sum in 16-byte vectors
  if (t < WAVE) {
    const uint32_t ev_n = reinterpret_cast<const EnvCold*>(cs)->evlog.n;
    uint32_t len[SPAN_PER_LANE], sum = 0;
#pragma unroll
    for (int j = 0; j < SPAN_PER_LANE; ++j) {
      const int k = lane * SPAN_PER_LANE + j;
      len[j] = 0;
      if (k < COLD_SPANS) {
        const ColdSpan c = cold_live_span(hs, a.steps, a.rng_mode, a.evlog_on, ev_n, k);
        sp_off[k] = c.off; sp_len[k] = c.bytes;
        len[j] = c.bytes >> 4;
        sum += len[j];
      }
    }
    uint32_t inc = sum;                            // inclusive scan of the lanes' sums
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      const uint32_t v = __shfl_up(inc, (unsigned)o, WAVE);
      if (lane >= o) inc += v;
    }
    uint32_t run = inc - sum;
#pragma unroll
    for (int j = 0; j < SPAN_PER_LANE; ++j) {
      const int k = lane * SPAN_PER_LANE + j;
      if (k < COLD_SPANS) { sp_cum[k] = run; run += len[j]; }
    }
    if (lane == WAVE - 1) sp_cum[COLD_SPANS] = inc;
  }
  // meanwhile the hot row: one long span of 16-byte vectors
  {
    const uint4* src = reinterpret_cast<const uint4*>(hs);
    uint4* dst = reinterpret_cast<uint4*>(hd);
    for (int v = t; v < ROW_VEC; v += CT) dst[v] = src[v];
  }
  __syncthreads();
  // the cold spans: vector v of the call's list lies in span k with sp_cum[k] <= v < sp_cum[k + 1] (empty spans share their cum with the next)
  const uint32_t total = sp_cum[COLD_SPANS];
  for (uint32_t v = (uint32_t)t; v < total; v += CT) {
    int lo = 0, hi = COLD_SPANS - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sp_cum[mid] <= v) lo = mid; else hi = mid - 1;
    }
    const uint32_t off = sp_off[lo] + 16u * (v - sp_cum[lo]);
    *reinterpret_cast<uint4*>(cd + off) = *reinterpret_cast<const uint4*>(cs + off);
  }
  for (int k = t; k < COLD_SPANS; k += CT) {        // the spans' last 0..3 words
    const uint32_t b = sp_len[k], tail = (b & 15u) >> 2, off = sp_off[k] + (b & ~15u);
    for (uint32_t w = 0; w < tail; ++w) reinterpret_cast<uint32_t*>(cd + off)[w] = reinterpret_cast<const uint32_t*>(cs + off)[w];
  }

  // the outputs of the last step
  if (a.dst_bank) {
    uint8_t* out = a.dst_bank + (size_t)d * a.slot + slot_out_off(a.cold_row);
    if (t < WAVE) pack_row_from_obs(out, a.obs + (size_t)s * OBS_TOTAL, lane);
    if (t == WAVE) {
      *reinterpret_cast<float*>(out + OBS_PACKED) = a.reward[s];
      *reinterpret_cast<uint32_t*>(out + OBS_PACKED + 4) = a.err[s];
      out[OBS_PACKED + 8] = a.done[s];
    }
  } else {
    int32_t* o = a.obs + (size_t)d * OBS_TOTAL;
    if (a.src_bank) {
      const uint32_t* pk = reinterpret_cast<const uint32_t*>(a.src_bank + (size_t)s * a.slot + slot_out_off(a.cold_row));
      for (int k = t; k < OBS_TOTAL; k += CT) o[k] = (int32_t)((pk[k >> 4] >> (2 * (k & 15))) & 3u);
      if (t == WAVE) {
        const uint8_t* b = reinterpret_cast<const uint8_t*>(pk);
        a.reward[d] = *reinterpret_cast<const float*>(b + OBS_PACKED);
        a.err[d] = *reinterpret_cast<const uint32_t*>(b + OBS_PACKED + 4);
        a.done[d] = b[OBS_PACKED + 8];
      }
    } else {
      copy_words(reinterpret_cast<uint32_t*>(o), reinterpret_cast<const uint32_t*>(a.obs + (size_t)s * OBS_TOTAL), OBS_TOTAL, t, CT);
      if (t == WAVE) { a.reward[d] = a.reward[s]; a.err[d] = a.err[s]; a.done[d] = a.done[s]; }
    }
    // the handle's mask row, from the copied row (blue_mask_slot: the rule of blue_action_mask); the caller's persistent buffer follows
    // at the next cc4_policy_outputs
    uint8_t* m = a.mask + (size_t)d * MASK_TOTAL;
    for (int k = t; k < MASK_TOTAL; k += CT) {
      const int b = k < 4 * ACT_SHORT ? k / ACT_SHORT : 4;
      m[k] = blue_mask_slot(hs, b, k - b * ACT_SHORT);
    }
    if (t == 0) a.mask_stale[d] = 1;
  }
  __syncthreads();                                  // (the copied rows are in place: the epilogue edits them)
  if (t == 0) {
    EvLog* lg = &reinterpret_cast<EnvCold*>(cd)->evlog;    // the log switch is the destination handle's; entries travel only when it is on
    lg->enabled = a.evlog_on ? 1u : 0u;
    if (!a.evlog_on) lg->n = 0;
    if (a.dst_bank) {
      SlotHdr* hdr = reinterpret_cast<SlotHdr*>(a.dst_bank + (size_t)d * a.slot);
      hdr->magic = SLOT_MAGIC; hdr->version = SLOT_VERSION; hdr->steps = a.steps; hdr->rng_mode = a.rng_mode;
      hdr->claim = 0u;                              // (no other entry of the call names this slot: a duplicate would have been skipped)
    } else if (a.seeds) {
      episode_set_seed(hd, reinterpret_cast<EnvCold*>(cd), a.seeds[i], a.rng_mode);   // deepcopy(env); env.set_seed(seed)
    }
  }
}
