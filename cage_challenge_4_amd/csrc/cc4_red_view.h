// cc4_red_view.h -- the red agents as learners (include/cc4.h "Red agents as learners"): one statement, for the device kernels (cc4_k_red.hip) and the
// host functions, of
//   * the conversion and validation of a submitted red action, four int32 words -> one ExtAct record (cc4_step_red_device: k_red_submit, one lane per
//     episode and agent; cc4_red_record_from_row on the host);
//   * what each red agent knows as fixed-shape tensors (cc4_red_view_device: k_red_view, one wavefront per episode; cc4_red_view_from_row, serial):
//     [6][137][8] uint8 per host, [6][16] int32 per agent.
// Everything is computed from the part of the hot row in front of the host table, and for agent r from red[r] and the records of the session pool its own
// list names: nothing of another agent's sessions, of blue's state or of the host table enters, and the FSM classes' per-host states (a scripted policy's
// memory, not an observation) are left out.  The per-item functions:
//   red_auto_sid     the id CC4_RED_SID_AUTO stands for: the agent's first listed session
//   red_record       (type, host, arg, session) -> the record's three 64-bit words, or "refused"
//   rv_sess_item     entry i of agent r's session list: its host and RS_* flags
//   rv_obs_item      entry i of agent r's last observation: its host and OE_* flags
//   rv_host_row      one (agent, host) row of 8 bytes from the agent's bitmaps and the host's summary word
//   rv_scalar        one of the 16 words of an agent
#pragma once
#include "cc4_engine.h"

namespace cc4 {

enum : int { RED_ACT_WORDS = 4, RED_SID_AUTO = -1, RED_SID_NONE = 0xFFFF };
enum : int { RV_HOSTS = MAXH, RV_PER_HOST = 8, RV_SCALARS = 16, RV_HOST_BYTES = NRED * MAXH * RV_PER_HOST, RV_HOST_VECS = RV_HOST_BYTES / 16 };
enum : int { RVC_KNOWN_IP = 0, RVC_KNOWN_HOSTNAME, RVC_SESSION_LEVEL, RVC_SESSIONS, RVC_OBS, RVC_ABSTRACT, RVC_START, RVC_RESERVED };
enum : int { RVW_ACTIVE = 0, RVW_BUSY, RVW_Q_TYPE, RVW_Q_HOST, RVW_Q_TICKS, RVW_OBS_SUCCESS, RVW_OBS_ACT_TYPE, RVW_OBS_ACT_HOST, RVW_OBS_ACT_ARG, RVW_NSESS, RVW_AS_SUBNET,
             RVW_NEW_SESS_HOST, RVW_AUTO_SID, RVW_EXEC_TYPE, RVW_EXEC_HOST, RVW_STEP_COUNT };
static_assert((int)RVC_RESERVED == (int)RV_PER_HOST - 1 && (int)RVW_STEP_COUNT == (int)RV_SCALARS - 1 && RV_HOST_BYTES % 16 == 0, "the columns and words of include/cc4.h");

// ---- submitted actions.  A record as the step kernels read it (ExtAct, 24 bytes) is three 64-bit words: the eight small fields, rate0, rate1.
struct ExtActW { uint64_t w[3]; };
static_assert(sizeof(ExtAct) == sizeof(ExtActW) && offsetof(ExtAct, type) == 0 && offsetof(ExtAct, host) == 1 && offsetof(ExtAct, arg) == 2 && offsetof(ExtAct, ticks) == 3 &&
              offsetof(ExtAct, sid) == 4 && offsetof(ExtAct, flags) == 6 && offsetof(ExtAct, rate0) == 8 && offsetof(ExtAct, rate1) == 16, "ExtAct as three words");
CC4_HD ExtActW ext_none() { return ExtActW{{~0ull, ~0ull, ~0ull}}; }      // XA_NONE as cc4_step_ex and launch_step leave it: every byte 0xFF

// the id of the agent's first listed session (state.sessions[red_agent_r], dict order), or RED_SID_NONE
CC4_HD uint32_t red_auto_sid(const EnvState* s, int r) {
  const RedAgent& A = s->red[r];
  if (A.h.nsess == 0 || A.sord[0] >= RS_POOL) return (uint32_t)RED_SID_NONE;
  return s->spool[A.sord[0]].id;
}
// One submitted action of red_agent_r: type as cc4_agent_action (XA_NONE: the agent's own policy acts), host, arg, session (an id, or RED_SID_AUTO --
// resolved from the row as it stands; an agent without a session gets id 0 and the engine's validity check decides).  ticks 0, no flags, no rates: the
// class's own.  False and *out = none: a refused record -- what the kernels index with must be in range (the rules of cc4_step_ex: the type, host < MAXH,
// a DiscoverRemoteSystems subnet < NSUB, a Withdraw hostname < MAXH), and what the record's fields cannot hold is refused too (arg beyond a byte, a
// session that is neither an id 0..65535 nor RED_SID_AUTO).
CC4_HD bool red_record(const EnvState* s, int r, int32_t type, int32_t host, int32_t arg, int32_t session, ExtActW* out) {
  *out = ext_none();
  if (type == XA_NONE) return true;
  if (type < 0 || type > RA_INVALID || host < 0 || host >= MAXH || arg < 0 || arg > 255 || session < RED_SID_AUTO || session > 0xFFFF) return false;
  if ((type == RA_DRS && arg >= NSUB) || (type == RA_WITHDRAW && arg >= MAXH)) return false;
  uint32_t sid = (uint32_t)session;
  if (session == RED_SID_AUTO) { sid = red_auto_sid(s, r); if (sid == (uint32_t)RED_SID_NONE) sid = 0; }
  out->w[0] = (uint64_t)(uint32_t)type | (uint64_t)(uint32_t)host << 8 | (uint64_t)(uint32_t)arg << 16 | (uint64_t)(sid & 0xFFFFu) << 32;
  out->w[1] = 0; out->w[2] = 0;
  return true;
}

// ---- the view.  The summary of one (agent, host): bits 0..7 the agent's sessions on the host, 8..15 the observation byte, 16 "one of them is a root
// session", 17 "one of them is abstract" -- one LDS word per pair on the device (atomics), a local array on the host.
enum : uint32_t { RVS_ONE = 1u, RVS_OBS_SHIFT = 8, RVS_ROOT = 1u << 16, RVS_ABSTRACT = 1u << 17 };
CC4_HD bool rv_sess_item(const EnvState* s, int r, int i, int* host, uint32_t* flags) {
  const RedAgent& A = s->red[r];
  if (i >= (int)A.h.nsess || i >= MAX_RS) return false;
  const int slot = A.sord[i];
  if (slot >= RS_POOL) return false;           // (a row from elsewhere must not index past the pool or the summary)
  const RSess& q = s->spool[slot];
  *host = q.host; *flags = q.flags;
  return q.host < MAXH;
}
CC4_HD uint32_t rv_sess_bits(uint32_t flags) { return ((flags & RS_ROOT) ? RVS_ROOT : 0u) | ((flags & RS_ABSTRACT) ? RVS_ABSTRACT : 0u); }
CC4_HD bool rv_obs_item(const EnvState* s, int r, int i, int* host, uint32_t* flags) {
  const RedAgent& A = s->red[r];
  if (i >= (int)A.h.nobs || i >= MAX_OBS) return false;
  *host = A.obs[i].host; *flags = A.obs[i].flags;
  return A.obs[i].host < MAXH;
}
CC4_HD uint32_t rv_obs_bits(uint32_t flags) { return (0x80u | (flags & (uint32_t)(OE_KEY_IP | OE_SESS | OE_IFACE | OE_SYSHN))) << RVS_OBS_SHIFT; }
struct RvRow { uint32_t w[2]; };        // one (agent, host) row, little-endian: byte c = column c
CC4_HD RvRow rv_host_row(const EnvState* s, int r, int h, uint32_t sum) {
  const RedAgent& A = s->red[r];
  const uint32_t cnt = sum & 0xFFu, level = cnt == 0 ? 0u : ((sum & RVS_ROOT) ? 2u : 1u);
  RvRow o;
  o.w[0] = (uint32_t)bit_get(A.as_ip, h) | (uint32_t)bit_get(A.as_hn, h) << 8 | level << 16 | cnt << 24;
  o.w[1] = ((sum >> RVS_OBS_SHIFT) & 0xFFu) | ((sum & RVS_ABSTRACT) ? 1u : 0u) << 8 | ((int)A.h.start_host == h ? 1u : 0u) << 16;
  return o;
}
static_assert(MAX_RS <= 255, "a host's session count of one agent fits the summary's low byte");
CC4_HD int32_t rv_scalar(const EnvState* s, int r, int k) {
  const RedHdr& H = s->red[r].h;
  const bool busy = H.queue.busy != 0;
  switch (k) {
    case RVW_ACTIVE: return H.active ? 1 : 0;
    case RVW_BUSY: return busy ? 1 : 0;
    case RVW_Q_TYPE: return busy ? (int32_t)H.queue.type : (int32_t)RA_NONE;
    case RVW_Q_HOST: return busy ? (int32_t)H.queue.host : 255;
    case RVW_Q_TICKS: return busy ? (int32_t)H.queue.ticks : 0;
    case RVW_OBS_SUCCESS: return H.obs_success;
    case RVW_OBS_ACT_TYPE: return H.obs_act_type;
    case RVW_OBS_ACT_HOST: return H.obs_act_host;
    case RVW_OBS_ACT_ARG: return H.obs_act_arg;
    case RVW_NSESS: return H.nsess;
    case RVW_AS_SUBNET: return H.as_subnet;
    case RVW_NEW_SESS_HOST: return H.new_sess_host;
    case RVW_AUTO_SID: return (int32_t)red_auto_sid(s, r);
    case RVW_EXEC_TYPE: return H.exec_type;
    case RVW_EXEC_HOST: return H.exec_host;
    default: return s->step_count;
  }
}

// The serial statement: hosts [6][137][8], scal [6][16] (or null) from one hot row.
inline void red_view_from_row(const EnvState* s, uint8_t* hosts, int32_t* scal) {
  for (int r = 0; r < NRED; ++r) {
    uint32_t sum[MAXH] = {};
    int h; uint32_t fl;
    for (int i = 0; i < MAX_RS; ++i) if (rv_sess_item(s, r, i, &h, &fl)) { sum[h] += RVS_ONE; sum[h] |= rv_sess_bits(fl); }
    for (int i = 0; i < MAX_OBS; ++i) if (rv_obs_item(s, r, i, &h, &fl)) sum[h] |= rv_obs_bits(fl);
    for (h = 0; h < MAXH; ++h) {
      const RvRow row = rv_host_row(s, r, h, sum[h]);
      __builtin_memcpy(hosts + ((size_t)r * MAXH + (size_t)h) * RV_PER_HOST, row.w, RV_PER_HOST);
    }
    if (scal) for (int k = 0; k < RV_SCALARS; ++k) scal[r * RV_SCALARS + k] = rv_scalar(s, r, k);
  }
}

}  // namespace cc4
