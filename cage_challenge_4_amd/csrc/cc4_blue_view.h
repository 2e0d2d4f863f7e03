// cc4_blue_view.h -- blue's own knowledge as fixed-shape tensors (include/cc4.h "Blue's own knowledge"): one statement, for the device kernel
// (cc4_k_blue.hip: k_blue_view, one wavefront per episode) and the host function (cc4_blue_view_from_row: blue_view_from_row, serial), of what the
// reference hands a blue agent in its dict observation and BlueFlatWrapper's 578 values drop: whether the agent is busy, the outcome of its own
// action, what Analyse found, what a deployed decoy is, the suspicious pids Remove would act on, and per host the entries of the end-turn Monitor --
// how many connection and process entries, on which service ports, and from which remote hosts.
//   [5][137][8] uint8 per (agent, host), [5][16] int32 per agent.
// Sources: the hot row (blue[b].queue / nsus / parent_host / last_ok, bexec[b], hev, exists, phase, step_count, and hd_files of the ONE host the
// agent's own Analyse named) and two parts of the cold row: the per-step event log (EvLog) and the agents' sus lists.  Nothing of red's tables, of
// the session pool, of another agent's sus list or of the rest of the host table enters.
//
// The event log and the step it belongs to.  step_phase (cc4_engine.h) opens a step with evlog.n = 0 and evlog.step = step_count, the count BEFORE
// the step; step_end then increments step_count.  Between steps the log therefore describes the step just taken exactly when
//   evlog.step + 1 == step_count            (and step_count >= 1: a regenerated episode has taken no step)
// The log is usable -- events_valid, word 10 -- iff evlog.enabled is set, that relation holds and evlog.n <= MAX_EV (a larger count means entries
// were dropped: a truncated log is not reported as a complete one).  Otherwise columns 3..6, the decoy part of column 7 and word 11 are zero;
// everything else is still filled.
//
// Leak rule.  Row (b, h) is all zero unless h exists in b's zone, or h was the remote address of an entry on a host of b's zone this step -- and then
// only column 5 is set.  Entries of the log on hosts outside every blue zone (contractor network, internet) reach no row.
// Malformed entries (a row from elsewhere): an entry whose host is >= 137 is dropped, a remote address >= 137 (0xFF is "none") counts nowhere, the
// local address is never used as an index, counts are clamped to the containers' capacities.
//
// The per-item functions:
//   bv_events_valid  the relation above
//   bv_fold_event    entry i of the log into the summary words of its host, the remote count of (agent, remote host), and the agent's words
//   bv_fold_sus      one entry of sus[b] into its host's saturating count
//   bv_host_row      one (agent, host) row of 8 bytes from the summary and the hot row
//   bv_scalar        one of the 16 words of an agent
#pragma once
#include "cc4_engine.h"

namespace cc4 {

enum : int { BV_HOSTS = MAXH, BV_PER_HOST = 8, BV_SCALARS = 16, BV_ROWS = NBLUE * MAXH, BV_HOST_BYTES = BV_ROWS * BV_PER_HOST };
enum : int { BVC_IN_ZONE = 0, BVC_EVENTS, BVC_SUS_PIDS, BVC_CONN_ENTRIES, BVC_PROC_ENTRIES, BVC_REMOTE_SEEN, BVC_PORTS, BVC_OWN };
enum : int { BVW_BUSY = 0, BVW_Q_TYPE, BVW_Q_HOST, BVW_Q_TICKS, BVW_EXEC_TYPE, BVW_EXEC_HOST, BVW_EXEC_ARG, BVW_SUCCESS, BVW_NSUS, BVW_PARENT_HOST,
             BVW_EVENTS_VALID, BVW_ZONE_ENTRIES, BVW_PHASE, BVW_STEP_COUNT, BVW_RESERVED0, BVW_RESERVED1 };
enum : int { BV_PORT_PID = 0x40, BV_OWN_DECOY = 0x80 };      // column 6 bit 6: an entry on the host carried a pid; column 7: 0x80 | K_* kind of the deployed decoy
static_assert((int)BVC_OWN == (int)BV_PER_HOST - 1 && (int)BVW_RESERVED1 == (int)BV_SCALARS - 1 && BV_HOST_BYTES % 8 == 0 && BV_ROWS % 2 == 1,
              "the columns and words of include/cc4.h; an episode's block is whole 8-byte rows, an odd number of them");
static_assert((PB_22 | PB_80 | PB_3390 | PB_25 | PB_1 | PB_443) == 0x3F && (HF_CMD | HF_ESC | HF_ESC_LAST) == 7, "six port bits below BV_PORT_PID; three file bits");

// ---- the summary -- LDS on the device (atomics), local arrays on the host.  A host lies in at most one agent's zone, so what is counted ON a host
// needs one place per host, not per (agent, host); only "was the remote address of an entry in b's zone" is per pair:
//   hw[2 h]      bits 0..15 connection entries (kind 0) on host h, with rep     16..31 process entries (kind 1), with rep
//   hw[2 h + 1]  bits 0..6 the ports byte     24..31 sus pids of the zone's agent on h, saturating
//   rem[k >> 1]  for pair k = b * 137 + h, the half word k & 1: times h was the remote address of an entry in b's zone, with rep
// (627 words in all with the agents' ten below: two of the 1280-byte granules LDS is handed out in.  Two words per pair would be 5480 bytes, five
// granules, 25 workgroups per CU where a batch of 8192 on 256 CUs needs 32: a second round of workgroups, measured in profiles/r22_blue_view.txt.)
// The 16-bit counts cannot carry into their neighbours: a log holds at most MAX_EV entries of rep <= 255 each.
static_assert(MAX_EV * 255 < 65536, "the 16-bit counts of a summary word never wrap before the clamp");
// ... and per agent: dec[b] = ((i + 1) << 8) | kind of the LAST kind-2 entry i that names the host of the agent's own resolved DeployDecoy (0: none),
// tot[b] = entries of the step on the zone's hosts, with rep.
enum : int { BVS_PROC_SHIFT = 16, BVS_SUS_SHIFT = 24, BV_HW_WORDS = 2 * MAXH, BV_REM_WORDS = (BV_ROWS + 1) / 2 };

CC4_HD void bv_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicAdd(p, v);
#else
  *p += v;
#endif
}
CC4_HD void bv_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}
CC4_HD void bv_max(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMax(p, v);
#else
  if (v > *p) *p = v;
#endif
}
// the top byte of *p counts up to 255 and stays there
CC4_HD void bv_sat_inc_top(uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t old = *p;
  while ((old >> BVS_SUS_SHIFT) != 255u) {
    const uint32_t seen = atomicCAS(p, old, old + (1u << BVS_SUS_SHIFT));
    if (seen == old) break;
    old = seen;
  }
#else
  if ((*p >> BVS_SUS_SHIFT) != 255u) *p += 1u << BVS_SUS_SHIFT;
#endif
}

CC4_HD bool bv_busy(const EnvState* s, int b) { return s->blue[b].queue.busy != 0; }
// host h is a host of agent b's zone in this episode
CC4_HD bool bv_in_zone(const EnvState* s, int b, int h) { return h >= 0 && h < MAXH && blue_of_subnet(h_subnet(h)) == b && bit_get(s->exists, h); }
CC4_HD bool bv_events_valid(const EnvState* s, const EvLog* lg) {
  return lg && lg->enabled != 0 && s->step_count >= 1 && lg->step == (uint32_t)(s->step_count - 1) && lg->n <= (uint32_t)MAX_EV;
}
CC4_HD uint32_t bv_port_bit(uint32_t port) {
  return port == 22 ? PB_22 : (port == 80 ? PB_80 : (port == 3390 ? PB_3390 : (port == 25 ? PB_25 : (port == 1 ? PB_1 : (port == 443 ? PB_443 : 0)))));
}
CC4_HD void bv_rem_add(uint32_t* rem, int k, uint32_t v) { bv_add(&rem[k >> 1], v << (16 * (k & 1))); }
CC4_HD uint32_t bv_rem_get(const uint32_t* rem, int k) { return (rem[k >> 1] >> (16 * (k & 1))) & 0xFFFFu; }
// Entry i of a valid log.  hw: [BV_HW_WORDS], rem: [BV_REM_WORDS], dec / tot: [NBLUE].
CC4_HD void bv_fold_event(const EnvState* s, const EvRec& e, uint32_t i, uint32_t* hw, uint32_t* rem, uint32_t* dec, uint32_t* tot) {
  const int h = e.host;
  if (h >= MAXH) return;
  const int b = blue_of_subnet(h_subnet(h));
  if (b < 0 || !bit_get(s->exists, h)) return;
  if (e.kind == 2) {        // blue_decoy's own observation: laddr is the K_* kind of the decoy
    const Act& x = s->bexec[b];
    if (!bv_busy(s, b) && x.type == BA_DECOY && x.host == h) bv_max(&dec[b], ((i + 1u) << 8) | (uint32_t)(e.laddr & 0x7F));
    return;
  }
  const uint32_t rep = e.rep;
  if (e.kind > 2 || rep == 0) return;
  uint32_t* const w = hw + 2 * h;
  bv_add(&w[0], e.kind == 0 ? rep : rep << BVS_PROC_SHIFT);
  const uint32_t bits = (e.kind == 0 ? bv_port_bit(e.lport) : 0u) | (e.pid ? (uint32_t)BV_PORT_PID : 0u);
  if (bits) bv_or(&w[1], bits);
  if (e.raddr < MAXH) bv_rem_add(rem, b * MAXH + (int)e.raddr, rep);
  bv_add(&tot[b], rep);
}
// One entry of sus[b]: (host << 16) | pid.
CC4_HD void bv_fold_sus(const EnvState* s, int b, uint32_t entry, uint32_t* hw) {
  const int h = (int)(entry >> 16);
  if (bv_in_zone(s, b, h)) bv_sat_inc_top(&hw[2 * h + 1]);
}
CC4_HD int bv_nsus(const EnvState* s, int b, int steps) { const int n = s->blue[b].nsus, cap = cold_sus_cap(steps); return n < cap ? n : cap; }

struct BvRow { uint32_t w[2]; };        // one (agent, host) row, little-endian: byte c = column c
// w0, w1: the host's two summary words; rem16: the pair's remote count
CC4_HD BvRow bv_host_row(const EnvState* s, int b, int h, uint32_t w0, uint32_t w1, uint32_t rem16, uint32_t dec_b) {
  const uint32_t remote = rem16 > 255u ? 255u : rem16;
  BvRow o;
  o.w[0] = 0; o.w[1] = remote << 8;                       // the one column that may be set outside the zone
  if (!bv_in_zone(s, b, h)) return o;
  const uint32_t conn16 = w0 & 0xFFFFu, proc16 = w0 >> BVS_PROC_SHIFT;
  const uint32_t conn = conn16 > 255u ? 255u : conn16, proc = proc16 > 255u ? 255u : proc16;
  uint32_t own = 0;
  const Act& x = s->bexec[b];
  if (!bv_busy(s, b) && x.host == h) {
    if (x.type == BA_ANALYSE) own = (uint32_t)hd_files(s->hd[h]) & 7u;
    else if (x.type == BA_DECOY && dec_b) own = (uint32_t)BV_OWN_DECOY | (dec_b & 0x7Fu);
  }
  o.w[0] = 1u | ((uint32_t)s->hev[h] & 0xFu) << 8 | (w1 >> BVS_SUS_SHIFT) << 16 | conn << 24;
  o.w[1] |= proc | (w1 & 0x7Fu) << 16 | own << 24;
  return o;
}
// 'success' of the agent's own action as the reference's dict observation reports it: IN_PROGRESS while a multi-tick action runs; Sleep UNKNOWN;
// Monitor, Analyse, Remove, Restore and DeployDecoy TRUE once they resolve (their parameters are validated on submission); Block/AllowTrafficZone
// whether the pair's state changed (BlueAgent.last_ok)
CC4_HD int32_t bv_success(const EnvState* s, int b) {
  if (bv_busy(s, b)) return T_IN_PROGRESS;
  const int t = s->bexec[b].type;
  if (t == BA_SLEEP) return T_UNKNOWN;
  if (t >= BA_MONITOR && t <= BA_DECOY) return T_TRUE;
  if (t == BA_BLOCK || t == BA_ALLOW) return s->blue[b].last_ok;
  return 0;
}
CC4_HD int32_t bv_scalar(const EnvState* s, bool ev_valid, uint32_t tot_b, int b, int k) {
  const BlueAgent& A = s->blue[b];
  const bool busy = bv_busy(s, b);
  switch (k) {
    case BVW_BUSY: return busy ? 1 : 0;
    case BVW_Q_TYPE: return busy ? (int32_t)A.queue.type : (int32_t)BA_SLEEP;
    case BVW_Q_HOST: return busy ? (int32_t)A.queue.host : 255;
    case BVW_Q_TICKS: return busy ? (int32_t)A.queue.ticks : 0;
    case BVW_EXEC_TYPE: return s->bexec[b].type;
    case BVW_EXEC_HOST: return s->bexec[b].host;
    case BVW_EXEC_ARG: return s->bexec[b].arg;
    case BVW_SUCCESS: return bv_success(s, b);
    case BVW_NSUS: return A.nsus;
    case BVW_PARENT_HOST: return A.parent_host;
    case BVW_EVENTS_VALID: return ev_valid ? 1 : 0;
    case BVW_ZONE_ENTRIES: return (int32_t)tot_b;
    case BVW_PHASE: return s->phase;
    case BVW_STEP_COUNT: return s->step_count;
    default: return 0;
  }
}

// The serial statement: hosts [5][137][8], scal [5][16] (or null) from one hot row, the episode's event log and its sus lists
// (sus: [NBLUE][cold_sus_cap(steps)] as in the cold row; lg and sus null together: no cold row -- columns 2..6 and the decoy bits 0, events_valid 0).
inline void blue_view_from_row(const EnvState* s, const EvLog* lg, const uint32_t* sus, int steps, uint8_t* hosts, int32_t* scal) {
  uint32_t hw[BV_HW_WORDS] = {}, rem[BV_REM_WORDS] = {}, dec[NBLUE] = {}, tot[NBLUE] = {};
  const bool valid = bv_events_valid(s, lg);
  if (valid) for (uint32_t i = 0; i < lg->n; ++i) bv_fold_event(s, lg->rec[i], i, hw, rem, dec, tot);
  if (sus)
    for (int b = 0; b < NBLUE; ++b) {
      const uint32_t* const p = sus + (size_t)b * (size_t)cold_sus_cap(steps);
      for (int i = 0, n = bv_nsus(s, b, steps); i < n; ++i) bv_fold_sus(s, b, p[i], hw);
    }
  for (int k = 0; k < BV_ROWS; ++k) {
    const int b = k / MAXH, h = k - b * MAXH;
    const BvRow row = bv_host_row(s, b, h, hw[2 * h], hw[2 * h + 1], bv_rem_get(rem, k), dec[b]);
    __builtin_memcpy(hosts + (size_t)k * BV_PER_HOST, row.w, BV_PER_HOST);
  }
  if (scal) for (int k = 0; k < NBLUE * BV_SCALARS; ++k) scal[k] = bv_scalar(s, valid, tot[k / BV_SCALARS], k / BV_SCALARS, k % BV_SCALARS);
}

}  // namespace cc4
