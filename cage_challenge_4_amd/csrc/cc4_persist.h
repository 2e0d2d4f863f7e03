// cc4_persist.h -- the schedule of the persistent kernels (k_run_philox1 / k_run_philox1x / k_run_philox1r / k_run_pcg and the plan builds k_run_philox1p / k_run_pcgp): one wave per residency slot pulling runs of
// steps of episodes from its CU's partition.  See cc4_args.h (RunArgs) and DESIGN 3.3; the index arithmetic it rests on -- partitions, tickets, runs, the
// progress word -- is cc4_sched.h's.
#pragma once
#include "cc4_kernels.h"

// the step bodies (defined in cc4_k_pcg.hip / cc4_philox1_body.h)
template <bool LOG> __device__ __forceinline__ void pcg_body(StepArgs a, const int e, const int lane, const bool first = true, const bool last = true);
template <bool LOG, bool PERSIST, bool HEAD> __device__ __forceinline__ void philox1_body(StepArgs a, const int e, const uint32_t rand_t, const uint32_t item_k, const int lane,
                                                                const bool first, const bool last);

// the CU this wave runs on, as a slot id below CC4_SLOTS: (XCC id << 8) | HW_ID[15:8]
__device__ __forceinline__ int cu_slot() {
  const uint32_t hw = __builtin_amdgcn_s_getreg(((16 - 1) << 11) | (0 << 6) | 4);     // HW_REG_HW_ID bits 15:0: wave, simd, pipe | cu, sh, se
  const uint32_t xcc = __builtin_amdgcn_s_getreg(((4 - 1) << 11) | (0 << 6) | 20);    // HW_REG_XCC_ID bits 3:0
  return (int)(((xcc & 7u) << 8) | ((hw >> 8) & 0xFFu));
}
static_assert(MAX_XCD_PARTITIONS == WAVE, "pick_balanced: one lane per partition of the wave's XCD");
// lane 0: the actions of step j for policy group g are published.  Polls a device word at a growing interval (see xchg_wait_slab).
__device__ __forceinline__ void rollout_wait_actions(const RunArgs& ra, const XchgArgs& x, int line, int g, uint32_t j) {
  const uint32_t* w = ra.act_ready + (size_t)line * 32 + g;
  if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) > j) return;
  if (__hip_atomic_load(x.timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) return;
  const long long w0 = wall_clock64();
  int naps = 1;
  while (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) <= j) {
    for (int i = 0; i < naps; ++i) __builtin_amdgcn_s_sleep(32);
    if (naps < 4) naps <<= 1;
    if (wall_clock64() - w0 > ra.act_wait_ticks || __hip_atomic_load(x.timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) { raise_timeout(x); return; }
  }
}
// lane 0, the progress wait: until episode ee has finished the steps before step k; returns its progress word.  watchdog (a rollout; every other
// wait is unbounded): under the bound of the action waits, act_wait_ticks from the wait's start.  A ticket of this call names a step
// whose predecessor some wave holds or will draw, so the wait normally ends; a ticket line that does not belong to this call, or a predecessor a wave
// gave up, would leave it spinning for good.  On expiry both timeout flags are raised and ok = false: the caller leaves without running the item,
// and cc4_rollout_end reports -6 instead of hanging.
__device__ __forceinline__ uint32_t wait_progress(const RunArgs& ra, const XchgArgs& x, int ee, uint32_t k, const bool watchdog, bool& ok) {
  const long long w0 = watchdog ? wall_clock64() : 0;
  uint32_t w;
  ok = true;
  while ((progress_steps(w = __hip_atomic_load(&ra.progress[ee], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) - ra.base) < k) {
    if (watchdog && wall_clock64() - w0 > ra.act_wait_ticks) { raise_timeout(x); ok = false; break; }
    __builtin_amdgcn_s_sleep(8);
  }
  return w;
}
// lane 0, the ticket draw: one ticket of counter idx of partition `line`'s ticket line.  The counter hands out the nph runs of the partition's episodes
// number idx, idx + pg, .. (pg = 1, idx = 0: all of them; a rollout: policy group idx of pg) in run-major order; whoever draws its last ticket clears the
// counter of the OTHER parity for the next call (exactly one wave per counter and call draws it, whoever runs the partition -- no memset between calls).
// false: handed out meanwhile; else run j of episode ee (ticket_item, cc4_sched.h).
__device__ __forceinline__ bool draw_ticket(const RunArgs& ra, int n, int line, int idx, int pg, int& j, int& ee) {
  const uint32_t cnt = ticket_count(n, ra.P, line, idx, pg), total = ticket_total(cnt, ra.runs.nph);
  const uint32_t t = __hip_atomic_fetch_add(ra.ticket + line * TK_STRIDE + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t + 1u == total) __hip_atomic_store(ra.ticket_next + line * TK_STRIDE + idx, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t >= total) return false;
  ticket_item(t, cnt, line, idx, pg, ra.P, j, ee);
  return true;
}

// The exchange: step k of episode e is out -- called behind a drain of the wave's stores and a barrier, between the steps of a run and at its end.
// pend_e / pend_k: the row this wave stored last and has not counted yet.
template <bool PCG>
__device__ __forceinline__ void persist_step_out(const StepArgs& a, const RunArgs& ra, const XchgArgs& x, const bool rollout, const int lane, const int e, const uint32_t k,
                                                 int& pend_e, uint32_t& pend_k) {
  if constexpr (PCG) {     // (the numpy-stream body stored the row itself, from its LDS byte row: drained by now)
    if (lane == 0) xchg_count(x, k, part_of(e, ra.G));
  } else {
    // the row this wave stored LAST (a step ago, or with its previous item) is in memory -- the drain covered it: counted.  Then this episode's row of
    // step k, read back from the int32 row before the episode's next step may touch it (the loads feed the store, the store is issued ahead of
    // the progress word) -- not waited for: it drains with the wave's next step or item, or when the wave leaves.
    if (lane == 0 && pend_e >= 0) xchg_count(x, pend_k, part_of(pend_e, ra.G));
    pack_row_from_obs(x.slab + ((size_t)(k % (uint32_t)x.ring) * (size_t)a.n + (size_t)e) * OBS_PACKED, a.obs + (size_t)e * OBS_TOTAL, lane);
    pend_e = e; pend_k = k;
    if (rollout) {
      // a rollout: the caller's next policy pass waits for this count -- not deferred to the wave's next item
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) xchg_count(x, k, pgroup_slot(e, ra.P, ra.PG));
      pend_e = -1;
    }
  }
}

// The schedule (RunArgs).  The batch is cut into one partition per CU (episode e -> partition e % P); a partition's tickets hand out RUNS of
// consecutive steps of its episodes in step-major order; a run of episode e may start once progress[e] says the steps before it are done.  A wave
// normally serves its own CU's partition -- an episode then stays on one CU, whose waves share a write-through L1: no cache maintenance -- but it
// looks at the ticket counters of its XCD's partitions before every run and takes the run from the partition that lags most when its own is more
// than `thr` tickets ahead of it, or handed out.  The progress word carries the CU that ran the episode's last run: a run on ANOTHER CU starts with
// an agent-scope acquire (buffer_inv sc1; nothing less drops stale L1 lines: tools/micro/l1_inv_scope.hip).  Never across XCDs: their L2s do not
// agree without a write-back.  The hand-over between two waves: the writer drains its stores (s_waitcnt vmcnt(0): the L1 is write-through, a drained
// store is in the XCD's L2), then publishes the progress word; the reader reads the word, then the rows.
// ROLLOUT: the build that serves cc4_rollout_begin (k_run_philox1r) -- the actions-in protocol is compiled into that kernel only (in the others its code
// cost the headline kernel 30 more spilled registers)
// XCHG: the build serves the exchange (the packed rows of every step into the slab ring, counted for the communication stream's gates).  The
// headline kernel k_run_philox1 is built without it: handles with a communicator launch k_run_philox1x.
// PLAN: the build serves cc4_run_plan_device (k_run_philox1p / k_run_pcgp; PlanArgs) -- step j of the call reads its blue actions and messages from row j
// of the caller's plan and writes reward / done / packed observation row into row j of the caller's trajectory.  The plan was complete before the launch
// and the trajectory is read behind its end: plain loads, no gate, no counter, no watchdog.  In every other build `pl` is dead and folds away.
// HEAD: the build of the headline kernel k_run_philox1 (counter mode, no exchange, no rollout, no plan), launched only for calls whose blue actions are
// drawn in the kernel and that carry no actions and no messages (persist_launch decides): the step body is compiled knowing that (philox1_body).
template <bool PCG, bool ROLLOUT = false, bool XCHG = true, bool PLAN = false, bool HEAD = false>
__device__ __forceinline__ void persist_loop(StepArgs a, RunArgs ra, const XchgArgs x, const PlanArgs pl = PlanArgs{}) {
  static_assert(!HEAD || (!PCG && !ROLLOUT && !XCHG && !PLAN), "the headline build: counter mode, nothing but the steps");
  // (the item travels from lane 0 to the wave through v_readfirstlane, not through LDS)
  const int lane = threadIdx.x;
  const int my_slot = cu_slot();
  a.prof = nullptr; a.obs8 = nullptr; a.ext = nullptr;
  uint32_t seen_gathered = 0;
  unsigned long long tl_first = 0, tl_last = 0, tl_items = 0;
  const unsigned long long tl_entry = ra.timeline ? wall_clock64() : 0;
#ifdef CC4_BOUNDARY_PROF
  // the measurement build (cc4_kernels.h, CC4_BP): the last stamp, the sums of the four parts (A: the stage-out's drain + publish, B: pick up to the drawn
  // ticket, C: progress wait + acquire, D: stage-in up to step_phase) and the boundaries counted (an item that follows an item on this wave)
  unsigned long long bp_t = 0, bp_A = 0, bp_B = 0, bp_C = 0, bp_D = 0, bp_n = 0;
#endif
  auto tl_flush = [&]() {
#ifdef CC4_BOUNDARY_PROF
    if (HEAD && ra.timeline && lane == 0) { unsigned long long* t = ra.timeline + 4 * (size_t)blockIdx.x; t[0] = ((tl_last - tl_first) & 0xFFFFFFFFull) | (bp_n << 32) | (1ull << 63); t[1] = (bp_A & 0xFFFFFFFFull) | (bp_B << 32); t[2] = (bp_C & 0xFFFFFFFFull) | (bp_D << 32); t[3] = tl_items | ((unsigned long long)(my_slot + 1) << 32); return; }
#endif
    if (ra.timeline && lane == 0) { unsigned long long* t = ra.timeline + 4 * (size_t)blockIdx.x; t[0] = tl_entry; t[1] = tl_first; t[2] = tl_last; t[3] = tl_items | ((unsigned long long)(my_slot + 1) << 32); } };
  int pend_e = -1; uint32_t pend_k = 0;  // the exchange: the item whose packed row this wave stored last and has not counted yet (its store drains with the next item)
  auto flush_pending = [&]() {
    if (XCHG && x.slab && pend_e >= 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); if (lane == 0) xchg_count(x, pend_k, part_of(pend_e, ra.G)); pend_e = -1; }
  };
  const int my_xcc = my_slot >> 8;
  const int xlo = ra.xcc_lo[my_xcc], xn = ra.xcc_n[my_xcc];     // this XCD's partitions
  // the CU's own partition, from the table of the compute units this device showed at first use (-1: a CU that is not in it only helps out), and
  // its id in the progress words
  const int own = ra.slot_part[my_slot] - 1;
  const uint32_t my_id = runner_of(own);
  const bool rollout = ROLLOUT && ra.act_ready;
  if (xn <= 0) { tl_flush(); return; }

  // ---- the item a wave picks (lane 0's counts): e = its episode (-5: look again, -4: leave), k = its run, sh = the episode's last run was on another CU
  struct Item { int e, k, sh; };
  // lane 0: a ticket of (line, idx, pg) as draw_ticket, then the waits for the run's predecessor and, with the exchange on, for the slab of its first step.  1: the item is in `it`, 0: handed out, -1: the wait gave up
  auto claim = [&](int line, int idx, int pg, Item& it) -> int {
    int j, ee;
    if (!draw_ticket(ra, a.n, line, idx, pg, j, ee)) return 0;
    CC4_BP(const unsigned long long now = wall_clock64(); if (tl_items) bp_B += now - bp_t; bp_t = now);
    int k, len; run_span(ra.runs, j, k, len);
    bool ok;
    const uint32_t w = wait_progress(ra, x, ee, (uint32_t)k, rollout, ok);
    if (!ok) return -1;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    CC4_BP(const unsigned long long now = wall_clock64(); if (tl_items) bp_C += now - bp_t; bp_t = now);
    if (XCHG && !rollout && x.slab) xchg_wait_slab(x, (uint32_t)k, seen_gathered);      // (a rollout has no `gathered` word: see xchg_wait_slab)
    const uint32_t last = progress_runner(w);
    it.e = ee; it.k = j; it.sh = (last != RUNNER_NONE && last != my_id) ? 1 : 0;     // the episode's last run was on another CU: its lines in this CU's L1 may be stale
    return 1;
  };
  // A rollout (every step a run of its own: nph = K): every (partition, policy group) has a ticket counter of its own (words 0 .. PG-1 of the partition's
  // ticket line), and a wave only ever draws a ticket of a group whose NEXT step is published -- it never holds a ticket it cannot run.  (With ONE
  // step-major sequence over all groups the waves piled up on tickets of unpublished passes while the published group's next tickets lay further down
  // the sequence: the groups advanced in lock step, 114 us per step whatever their number -- profiles/r06_rollout.txt.)  A CU serves its own partition only.
  auto pick_rollout = [&]() -> Item {
    Item it{-4, 0, 0};
    if (own < 0 || lane != 0) return it;
    const int ne = part_episodes(a.n, ra.P, own);
    const uint32_t* rdy = ra.act_ready + (size_t)own * 32;
    const uint32_t* tkl = ra.ticket + (size_t)own * TK_STRIDE;
    int naps = 1;
    const long long w0 = wall_clock64();
    for (;;) {
      int best_g = -1; uint32_t best_j = 0xFFFFFFFFu; bool left = false;
      for (int g = 0; g < ra.PG; ++g) {
        const int ng = pgroup_episodes(ne, ra.PG, g);
        if (ng <= 0) continue;
        const uint32_t t = __hip_atomic_load(tkl + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t >= ticket_total(ng, ra.runs.nph)) continue;
        left = true;
        const uint32_t j = ticket_run(t, ng);
        if (j < best_j && __hip_atomic_load(rdy + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) > j) { best_j = j; best_g = g; }
      }
      if (!left) return it;                                         // every group of this partition is handed out: leave
      if (best_g >= 0) {
        const int got = claim(own, best_g, ra.PG, it);
        if (got == 0) continue;
        if (got > 0) rollout_wait_actions(ra, x, own, best_g, (uint32_t)it.k);   // (another wave may have drawn the last published ticket in between: then this one is of the next step)
        return it;                                                  // (the wait gave up: it.e is -4, this wave leaves)
      }
      // nothing is published that this partition has not handed out: wait (a growing nap, the watchdog of the action waits)
      for (int q = 0; q < naps; ++q) __builtin_amdgcn_s_sleep(32);
      if (naps < 4) naps <<= 1;
      if (__hip_atomic_load(x.timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) || wall_clock64() - w0 > ra.act_wait_ticks) {
        raise_timeout(x);
        // give up on the policy: run what is left with whatever the slots hold (cc4_rollout_end reports it), behind an agent-scope acquire
        for (int g = 0; g < ra.PG; ++g) {
          if (pgroup_episodes(ne, ra.PG, g) <= 0) continue;
          const int got = claim(own, g, ra.PG, it);
          if (got > 0) it.sh = 1;
          if (got != 0) return it;
        }
      }
    }
  };
  // The balanced schedule, all lanes: where the XCD's partitions stand; the run comes from the wave's own partition unless that one is more than `thr`
  // tickets ahead of the one that lags most, or handed out
  auto pick_balanced = [&]() -> Item {
    Item it{-5, 0, 0};
    const int q = xlo + lane;
    uint32_t tk = 0xFFFFFFFFu, tot_q = 0;
    // (every partition's counter on a cache line of its own, TK_STRIDE words apart: 24 waves of one CU on a line, not the 768 of an XCD -- with the
    // XCD's 32 counters on ONE line, its atomics and these loads took the L2 ~50 ns each and the schedule ran at 556 M instead of 884 M)
    if (lane < xn) { tk = __hip_atomic_load(&ra.ticket[q * TK_STRIDE], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); tot_q = ticket_total(part_episodes(a.n, ra.P, q), ra.runs.nph); }
    const bool has = lane < xn && tk < tot_q;
    uint32_t key = has ? ((tk << 6) | (uint32_t)lane) : 0xFFFFFFFFu;          // least tickets handed out = lags most (the partitions' sizes differ by one episode at most)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { const uint32_t k2 = (uint32_t)__shfl_xor((int)key, off); key = k2 < key ? k2 : key; }
    const uint32_t kmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
    if (kmin == 0xFFFFFFFFu) { it.e = -4; return it; }                        // every partition of this XCD is handed out: leave
    int target = (int)(kmin & 63u);
    if (own >= 0) {
      const int ol = own - xlo;
      const uint32_t tk_own = (uint32_t)__builtin_amdgcn_readlane((int)tk, ol);
      const uint32_t tot_own = (uint32_t)__builtin_amdgcn_readlane((int)tot_q, ol);
      if (tk_own < tot_own && tk_own <= (kmin >> 6) + (uint32_t)ra.thr) target = ol;
    }
    if (lane == 0) (void)claim(xlo + target, 0, 1, it);                        // (0: handed out meanwhile -- look again)
    return it;
  };
  for (;;) {
    // ---- pick an item
    const Item it = rollout ? pick_rollout() : pick_balanced();
    const int e = __builtin_amdgcn_readfirstlane(it.e);               // (all lanes are active here: the first active lane is lane 0)
    if (e == -4) { flush_pending(); tl_flush(); return; }
    if (e == -5) continue;
    int run_k0, run_len;
    run_span(ra.runs, __builtin_amdgcn_readfirstlane(it.k), run_k0, run_len);
    if (ra.timeline && !tl_items) tl_first = wall_clock64();
    // ---- acquire, if the episode's last run was on another CU
    if (__builtin_amdgcn_readfirstlane(it.sh)) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");      // (buffer_inv sc1: the CU's L1 dropped.  buffer_inv sc0 does NOT drop it: profiles/r06_l1_inv_scope.txt)
    // ---- the steps of the run
    uint32_t item_k = (uint32_t)run_k0;
    uint32_t err_acc = 0;          // PLAN, lane 0: the error flags of the run's steps (a regeneration inside the run clears the row's word)
    for (int q = 0; q < run_len; ++q, ++item_k) {
      if (q > 0) {
        if (XCHG && x.slab) {
          // a further step of the run with the exchange on: what the last step stored is drained and handed off as at a run's end, and the slab of
          // this step must have been gathered
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          persist_step_out<PCG>(a, ra, x, rollout, lane, e, item_k - 1u, pend_e, pend_k);
          if (lane == 0) xchg_wait_slab(x, item_k, seen_gathered);
        }
        __syncthreads();
      }
      int lane_i = (int)threadIdx.x;
      asm volatile("" : "+v"(lane_i));
      if (rollout) { a.actions = ra.act + (size_t)(item_k & 1u) * (size_t)a.n * NBLUE; a.rand_out = nullptr; a.act_sys = 1; }
      if constexpr (PLAN) {
        // row item_k of the plan in, row item_k of the trajectory out (the handle's own reward / done buffers where the caller gave none).  The packed
        // row is written by the step body itself behind a drain of its own (StepArgs.obs8, as in the per-step launches): every step of a run gets one
        const size_t row = (size_t)item_k * (size_t)a.n;
        a.actions = pl.actions + row * NBLUE; a.msgs = pl.msgs ? pl.msgs + row * (NBLUE * MSG_LEN) : nullptr; a.rand_out = nullptr;
        if (pl.rewards) a.reward = pl.rewards + row;
        if (pl.dones) a.done = pl.dones + row;
        a.obs8 = pl.obs_packed ? pl.obs_packed + row * OBS_PACKED : nullptr;
      }
      if constexpr (PCG) {
        StepArgs b = a;
        b.rand_t = ra.t0 + item_k; b.full_obs = (a.full_obs && item_k == 0) ? 1 : 0;
        if (XCHG && x.slab) b.obs8 = x.slab + (size_t)(item_k % (uint32_t)x.ring) * (size_t)a.n * OBS_PACKED;
        pcg_body<false>(b, e, lane_i, q == 0, q == run_len - 1);
      } else {
        philox1_body<false, true, HEAD>(a, e, ra.t0 + item_k, item_k, lane_i, q == 0, q == run_len - 1);    // (a.obs8 is null: the packed row is written by persist_step_out, behind the drain)
      }
      if constexpr (PLAN) {          // (the agent part is still in LDS; the body's last barrier is behind the step's last set_err)
        extern __shared__ uint4 plan_lds[];
        const EnvState* const sp = reinterpret_cast<const EnvState*>(plan_lds);
        if (lane == 0) err_acc |= sp->err | (sp->step_count == 0 ? PLAN_REGEN : 0u);     // (regenerated by this step: the caller's action-mask row is stale)
      }
    }
    --item_k;        // the run's last step
    CC4_BP(if (tl_items) { bp_D += cc4_bp_staged - bp_t; ++bp_n; } bp_t = wall_clock64());
    // ---- release: the item is done when everything it wrote has left this wave: then the next step of the episode may start (on this XCD)
    // Every lane DRAINS its own stores -- an explicit s_waitcnt vmcnt(0): the vector L1 is write-through, so a drained store is in
    // the XCD's L2 --, the barrier collects the lanes, lane 0 publishes.  The consumer is a wave of the same CU unless the partition is
    // shared, in which case it drops its L1 first (agent-scope acquire above).  The workgroup-scope fence beside it only pins the compiler:
    // without tgsplit the backend emits NO vmcnt wait for it (waves of a work-group share a CU), and the episode's rows and its progress
    // word sit in different L2 channels -- with the fence alone the word can land first.  (r05 ran that way for a day: one disagreement in
    // ~60 self-checked calls, CC4_PERSIST_VERIFY, 5632 episodes, hot row of one episode after a 10-step call.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (XCHG && x.slab) persist_step_out<PCG>(a, ra, x, rollout, lane, e, item_k, pend_e, pend_k);
    if constexpr (PLAN) {          // what some step of the run flagged, for the call's error word (k_plan_finish ORs it into the handle's): rare, nothing waits for it
      if (lane == 0 && err_acc) (void)__hip_atomic_fetch_or(pl.err_or + e, err_acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // ---- publish progress
    if (lane == 0) __hip_atomic_store(&ra.progress[e], progress_pack(ra.base + item_k + 1u, my_id), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ra.timeline) { tl_last = wall_clock64(); ++tl_items; }
    CC4_BP(bp_A += tl_last - bp_t; bp_t = tl_last);
  }
}
