// cc4_k_gae.hip -- advantages, returns and loss weights of a stored rollout (the definition: cc4_gae.h, shared with the host function).  A pure
// function of the caller's tensors on the caller's stream: no handle, no hot row, no LDS, no barrier.
//   k_gae  cc4_gae_device.  One lane per column c = n * A + a, GAE_WAVES wavefronts per workgroup (cc4_kernel_decls.h); the lanes of a wave hold
//          consecutive columns, so a row of values, actions, adv, ret and weight is read or written as 64 consecutive elements per instruction;
//          n = c / A once per lane: the rewards (shared by the heads) and the done bytes are read at n, neighbouring lanes share the addresses.
//          The recurrence is a dependent chain of two float operations per row, and no load depends on it.  So the rows go in blocks of GAE_ROWS
//          from the last row down: every load of a block is issued first, the chain of the block runs from registers, then the stores.  The short
//          block (T % GAE_ROWS rows, or all of T < GAE_ROWS) holds the LAST rows and is the same code with a shorter count: it loads GAE_ROWS
//          rows all the same (row 0 again past its count), runs and stores only its own.  The block of the last rows is the one that reads `last`.  A block of rows
//          [lo, hi) reads the done bytes of rows lo-1 .. hi-1: a row's `prev` is the byte of the row before it (done0 in front of row 0).
#include <hip/hip_runtime.h>
#include "cc4_gae.h"
#include "cc4_elem.h"
#include "cc4_kernel_decls.h"

static_assert(GAE_SKIP_AFTER_DONE == CC4_GAE_SKIP_AFTER_DONE && GAE_BOOTSTRAP_DONE == CC4_GAE_BOOTSTRAP_DONE, "include/cc4.h states the flags");
static_assert(GAE_ROWS >= 1 && GAE_ROWS <= 32 && GAE_WAVES >= 1 && GAE_WAVES <= 16, "a block of rows lives in registers; a workgroup is at most 1024 threads");

// A lane's place in the tensors: its pointers at the row the next block starts with (the last row first), stepped down by one row's elements per
// row -- one 64-bit add of a uniform stride per array and row.  (One wave per SIMD issues an instruction every few cycles at best, so t * N * A + c
// formed per lane, row and array would be most of what the vector unit does; and with every row's base kept on the scalar unit the bases spill
// into lanes and come back through readlanes.  Both forms were compiled and read in the ISA; this one has no spills: DESIGN 3.16.)
template <class E> struct GaeLane {
  const E* v; const float* r; const uint8_t* d; const int32_t* act;
  float* adv; float* ret; uint8_t* w;
  size_t row, rrow, drow;        // one row's elements: N * A; of the rewards; N
  uint32_t dn;                   // the lane's episode
};

// rows [hi - cnt, hi) of the lane's column, cnt <= GAE_ROWS (every index below is a constant after unrolling: the arrays are registers).  FIRST:
// the block of the last rows, which reads `last` among its loads -- v_next of row T-1 -- instead of a load and a wait of its own in front of the loop
template <int DT, bool ACT, bool FIRST>
__device__ __forceinline__ void gae_block(const GaeArgs& a, GaeLane<typename Elem<DT>::type>& l, const float last, const int hi, const int cnt,
                                          const float gl, GaeCarry& carry) {
  float r[GAE_ROWS], v[GAE_ROWS];
  uint8_t d[GAE_ROWS + 1];         // d[k]: row hi-1-k; d[cnt]: the row in front of the block
  int32_t act[GAE_ROWS];
  // 1. the loads, with no branch on cnt among them: a row past the count reads the block's lowest row again and is neither used nor stored
#pragma unroll
  for (int k = 0; k < GAE_ROWS; ++k) {
    v[k] = elem_to_float<DT>(*l.v);
    r[k] = *l.r;
    d[k] = *l.d;
    act[k] = 0;
    if constexpr (ACT) act[k] = *l.act;
    if (k + 1 < cnt) {
      l.v -= l.row; l.r -= l.rrow; l.d -= l.drow;
      if constexpr (ACT) l.act -= l.row;
    }
  }
  if constexpr (FIRST) carry.v = last;
  // the byte in front of the block: of the row below, or of done0 in front of row 0 (the one block that takes the branch)
  const int lo = hi - cnt;
  uint8_t front = *(lo > 0 ? l.d - l.drow : l.d);
  if (lo == 0) front = a.done0 ? a.done0[l.dn] : (uint8_t)0;
  d[GAE_ROWS] = 0;
#pragma unroll
  for (int k = 1; k <= GAE_ROWS; ++k)
    if (k == cnt) d[k] = front;
  // 2. the chain, 3. the stores
  GaeOut o[GAE_ROWS];
#pragma unroll
  for (int k = 0; k < GAE_ROWS; ++k)
    if (k < cnt) o[k] = gae_row(r[k], v[k], d[k + 1] != 0, d[k] != 0, act[k] != GAE_NO_ACTION, a.gamma, gl, a.flags, carry);
#pragma unroll
  for (int k = 0; k < GAE_ROWS; ++k) {
    if (k < cnt) {
      *l.adv = o[k].adv;
      *l.ret = o[k].ret;
      if (a.weight) *l.w = o[k].weight ? 1 : 0;
      if (k + 1 < cnt) {
        l.adv -= l.row; l.ret -= l.row;
        if (a.weight) l.w -= l.row;
      }
    }
  }
  // on to the next block's first row (not below row 0: the pointers of the last block stay where they are)
  if (lo > 0) {
    l.v -= l.row; l.r -= l.rrow; l.d -= l.drow; l.adv -= l.row; l.ret -= l.row;
    if (a.weight) l.w -= l.row;
    if constexpr (ACT) l.act -= l.row;
  }
}

// ACT: actions are given (a build of its own: a branch among the loads would put a wait behind each)
template <int DT, bool ACT>
__device__ __forceinline__ void gae_column(const GaeArgs& a, const size_t c, const size_t NA) {
  using E = typename Elem<DT>::type;
  const uint32_t n = (uint32_t)c / (uint32_t)a.A;      // (N * A <= INT32_MAX: a 32-bit division)
  const bool per_head = a.reward_heads != 1;
  const size_t top = (size_t)(a.T - 1), rrow = per_head ? NA : (size_t)a.N;
  GaeLane<E> l{static_cast<const E*>(a.values) + top * NA + c, a.rewards + top * rrow + (per_head ? c : (size_t)n), a.dones + top * (size_t)a.N + n,
               ACT ? a.actions + top * NA + c : nullptr, a.adv + top * NA + c, a.ret + top * NA + c, a.weight ? a.weight + top * NA + c : nullptr,
               NA, rrow, (size_t)a.N, n};
  const float gl = a.gamma * a.lambda;
  const float last = elem_to_float<DT>(static_cast<const E*>(a.last)[c]);
  GaeCarry carry{0.0f, 0.0f};
  const int tail = a.T % GAE_ROWS, first = tail ? tail : GAE_ROWS;      // (T >= 1)
  gae_block<DT, ACT, true>(a, l, last, a.T, first, gl, carry);
  for (int hi = a.T - first; hi > 0; hi -= GAE_ROWS) gae_block<DT, ACT, false>(a, l, 0.0f, hi, GAE_ROWS, gl, carry);
}

__global__ __launch_bounds__(GAE_WAVES * WAVE) void k_gae(GaeArgs a) {
  const size_t NA = (size_t)a.N * (size_t)a.A;
  const size_t c = (size_t)blockIdx.x * (size_t)(GAE_WAVES * WAVE) + threadIdx.x;
  if (c >= NA) return;
  if (a.actions) {
    if (a.dtype == 3) gae_column<3, true>(a, c, NA);
    else if (a.dtype == 2) gae_column<2, true>(a, c, NA);
    else gae_column<1, true>(a, c, NA);
  } else {
    if (a.dtype == 3) gae_column<3, false>(a, c, NA);
    else if (a.dtype == 2) gae_column<2, false>(a, c, NA);
    else gae_column<1, false>(a, c, NA);
  }
}
