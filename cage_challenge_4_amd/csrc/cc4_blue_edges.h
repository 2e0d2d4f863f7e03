// cc4_blue_edges.h -- the Monitor's connection entries as an edge list (include/cc4.h "Monitor's connections as edge lists"): one statement, for the
// device kernel (cc4_k_edges.hip: k_blue_edges, one wavefront per episode) and the host function (cc4_blue_edges_from_row: blue_edges_from_row,
// serial), of WHO TALKED TO WHOM in the step just taken -- what the reference's dict observation hands a blue agent as
//   Processes[..].Connections[..] = {local_address, local_port, remote_address, remote_port}
// and cc4_blue_view.h only counts (conn_entries, remote_seen).
//   edges [E][8] int32 per episode (E = the caller's max_edges, 1 .. BE_MAX), counts [8] int32.
// Source: the per-step event log of the cold row (EvLog, cc4_state.h) and, of the hot row, exists and step_count.
//
// An entry e of the log QUALIFIES iff the log is valid (bv_events_valid, cc4_blue_view.h: enabled, describes the step just taken, not truncated),
//   e.kind == 0 (network_connections), e.rep > 0, e.host < 137 and exists, b = blue_of_subnet(h_subnet(e.host)) >= 0, and e.raddr < 137.
// Its KEY is (b, host, raddr, laddr, lport, rport): 3 + 8 + 8 + 8 + 16 + 16 = 59 bits, one 64-bit word, b in the top bits.  Entries with equal
// keys merge into one edge whose count is the sum of their rep (at most MAX_EV x 255: no clamp).  The edges are listed in ascending key order --
// the agents' segments are contiguous, agent 0 first -- so the output is a function of the MULTISET of entries and never of their physical order:
// on the device the log is appended by atomicAdd (ev_log, cc4_engine.h) and its order is not deterministic.
//
// Leak rule.  An edge exists only for an entry on an existing host of the agent's own zone.  e.order (whether a green or a red agent acted -- the
// reference never tells blue) and e.pid enter nowhere: not the key, not the count, not the order of the list.  Nothing of red's tables, of the
// session pool or of the host table enters; entries on hosts outside every blue zone (contractor network, internet) give no edge.
//
// The order is established by RANKING, not by sorting: the position of an edge is the number of distinct smaller keys.  With at most 160 entries
// a lane ranks its (at most three) entries by reading all keys once; every lane reads the same key in the same iteration, which LDS serves as a
// broadcast, and no entry ever moves, so there is no exchange network, no padding to a power of two and no barrier inside the pass.
// The per-item functions:
//   be_key       does entry e qualify, and its key
//   be_is_head   entry i (by compacted index) is the first of its key: the one that writes the edge.  Ties have identical keys, and count and
//                position are functions of the key alone, so which of them writes cannot show
//   be_rank      for a head: the merged count, its position in the list, and the start of its agent's segment
//   be_row       the eight words of an edge
#pragma once
#include "cc4_blue_view.h"

namespace cc4 {

enum : int { BE_MAX = MAX_EV, BE_COLS = 8, BE_WORDS = 8 };
enum : int { BEC_AGENT = 0, BEC_HOST, BEC_LOCAL, BEC_REMOTE, BEC_LOCAL_PORT, BEC_REMOTE_PORT, BEC_COUNT, BEC_SLOT };
enum : int { BEW_TOTAL = NBLUE, BEW_EVENTS_VALID, BEW_STEP_COUNT };
enum : int { BE_KEY_AGENT_SHIFT = 56 };
constexpr uint32_t BE_HEAD = 0x80000000u;      // in the rep word of a compacted entry: the entry is the head of its key
static_assert((int)BEC_SLOT == (int)BE_COLS - 1 && (int)BEW_STEP_COUNT == (int)BE_WORDS - 1 && NBLUE <= 8 && MAXH <= 256, "the columns and words of include/cc4.h; the key's fields");

CC4_HD bool be_key(const EnvState* s, const EvRec& e, uint64_t* key) {
  const int h = e.host;
  if (e.kind != 0 || e.rep == 0 || h >= MAXH || e.raddr >= MAXH) return false;
  const int b = blue_of_subnet(h_subnet(h));
  if (b < 0 || !bit_get(s->exists, h)) return false;
  *key = (uint64_t)b << BE_KEY_AGENT_SHIFT | (uint64_t)h << 48 | (uint64_t)e.raddr << 40 | (uint64_t)e.laddr << 32 | (uint64_t)e.lport << 16 | (uint64_t)e.rport;
  return true;
}
CC4_HD int be_agent(uint64_t key) { return (int)(key >> BE_KEY_AGENT_SHIFT); }
CC4_HD bool be_is_head(const uint64_t* keys, int i) {
  const uint64_t k = keys[i];
  bool head = true;
  for (int j = 0; j < i; ++j) head = head && keys[j] != k;
  return head;
}
// keys / reps: the m compacted entries; reps carry BE_HEAD where be_is_head holds.  For head i:
//   count  sum of rep over the entries of its key     pos  distinct keys below it     seg  distinct keys of the agents before its own
CC4_HD void be_rank(const uint64_t* keys, const uint32_t* reps, int m, int i, uint32_t* count, int* pos, int* seg) {
  const uint64_t k = keys[i], base = (uint64_t)be_agent(k) << BE_KEY_AGENT_SHIFT;
  uint32_t c = 0;
  int p = 0, g = 0;
  for (int j = 0; j < m; ++j) {
    const uint64_t kj = keys[j];
    const uint32_t rj = reps[j];
    c += kj == k ? (rj & ~BE_HEAD) : 0u;
    const int head = (int)(rj >> 31);
    p += kj < k ? head : 0;
    g += kj < base ? head : 0;
  }
  *count = c; *pos = p; *seg = g;
}
struct BeRow { int32_t w[BE_COLS]; };
CC4_HD BeRow be_row(uint64_t key, uint32_t count, int slot) {
  const int laddr = (int)(key >> 32) & 0xFF;
  BeRow o;
  o.w[BEC_AGENT] = be_agent(key); o.w[BEC_HOST] = (int)(key >> 48) & 0xFF; o.w[BEC_LOCAL] = laddr < MAXH ? laddr : -1; o.w[BEC_REMOTE] = (int)(key >> 40) & 0xFF;
  o.w[BEC_LOCAL_PORT] = (int)(key >> 16) & 0xFFFF; o.w[BEC_REMOTE_PORT] = (int)key & 0xFFFF; o.w[BEC_COUNT] = (int32_t)count; o.w[BEC_SLOT] = slot;
  return o;
}

// The serial statement: edges [max_edges][8], counts [8] (or null) from one hot row and the episode's event log (lg null: no cold row -- no edges).
// max_edges: 1 .. BE_MAX (the caller checks).
inline void blue_edges_from_row(const EnvState* s, const EvLog* lg, int max_edges, int32_t* edges, int32_t* counts) {
  uint64_t keys[BE_MAX];
  uint32_t reps[BE_MAX];
  int m = 0, seg[NBLUE] = {}, total = 0;
  const bool valid = bv_events_valid(s, lg);
  if (valid)
    for (uint32_t i = 0; i < lg->n; ++i) {
      uint64_t k;
      if (be_key(s, lg->rec[i], &k)) { keys[m] = k; reps[m] = lg->rec[i].rep; ++m; }
    }
  for (int i = 0; i < m; ++i) if (be_is_head(keys, i)) reps[i] |= BE_HEAD;
  for (int i = 0; i < m; ++i) {
    if (!(reps[i] & BE_HEAD)) continue;
    uint32_t c; int p, g;
    be_rank(keys, reps, m, i, &c, &p, &g);
    ++seg[be_agent(keys[i])]; ++total;
    if (p < max_edges) { const BeRow r = be_row(keys[i], c, p - g); __builtin_memcpy(edges + (size_t)p * BE_COLS, r.w, sizeof r.w); }
  }
  for (int k = (total < max_edges ? total : max_edges) * BE_COLS; k < max_edges * BE_COLS; ++k) edges[k] = -1;
  if (counts) {
    for (int b = 0; b < NBLUE; ++b) counts[b] = seg[b];
    counts[BEW_TOTAL] = total; counts[BEW_EVENTS_VALID] = valid ? 1 : 0; counts[BEW_STEP_COUNT] = s->step_count;
  }
}

}  // namespace cc4
