// cc4_view_src.h -- the one resolver of the derived-view kernels (k_state_features, k_red_view, k_blue_view, k_blue_edges, k_reward_terms, k_sample_actions): which rows
// entry i of a call reads, or why it reads none.  The contract is stated at ViewSrc (cc4_args.h); this is its only implementation on the device.
#pragma once
#include "cc4_args.h"

struct ViewRows {
  uint32_t fault;              // 0, or the CF_* bit of a refused entry (then s and c are null and the kernel writes the view's empty output)
  const EnvState* s;           // the entry's hot row where it lies: the handle's, or the one inside the bank slot ([SlotHdr | hot row | cold row | ..])
  const EnvCold* c;            // its cold row likewise (a copy carries the live parts at the same offsets)
};

// Everything here is computed from blockIdx and from loads every lane makes at the same address: it stays in scalar registers, and the callers branch
// on it uniformly.  A refused entry raises its bit in the handle's fault word from lane 0.
__device__ __forceinline__ ViewRows view_rows(const ViewSrc& a, int i, int lane) {
  const int e = a.ids ? a.ids[i] : i;
  const uint8_t* slot = nullptr;
  uint32_t f = 0;
  if (e < 0 || e >= a.cap) f = CF_RANGE;
  else if (a.bank) {
    slot = a.bank + (size_t)e * a.slot;
    f = slot_hdr_fault(reinterpret_cast<const SlotHdr*>(slot), a.steps, a.rng_mode);
  }
  if (f) {
    if (lane == 0) atomicOr(a.fault, f);
    return ViewRows{f, nullptr, nullptr};
  }
  if (slot) return ViewRows{0u, reinterpret_cast<const EnvState*>(slot + sizeof(SlotHdr)), reinterpret_cast<const EnvCold*>(slot + slot_cold_off())};
  return ViewRows{0u, a.st + e, cold_at(a.cold, (size_t)e, a.cold_row)};
}
