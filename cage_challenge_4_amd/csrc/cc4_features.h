// cc4_features.h -- the privileged global state of one episode as fixed-shape tensors (cc4_state_features_device / cc4_state_features_from_row,
// include/cc4.h: the two tables there are the definition).  Everything is computed from the HOT row alone: [137][16] uint8 per host,
// [32] int32 per episode.  One statement for both sides: the kernel (cc4_k_feat.hip: k_state_features, one wavefront per episode) and the host
// function (feat_from_row below, serial) call the same per-item functions; what differs is who walks the items and where the per-host session
// summary lives (LDS words filled with LDS atomics / a local array).
//   feat_sess_item    one record of the session pool: live?  its host, and whether it is a root session
//   feat_green_item   one green agent: its host
//   feat_host_row     one host's 16 bytes from the row, the second half of its HostDyn (svcs, nproc, nsf) and the host's session summary
//   feat_global_word  one of the 32 episode words
#pragma once
#include "cc4_engine.h"

namespace cc4 {

enum : int { FEAT_HOSTS = MAXH, FEAT_PER_HOST = 16, FEAT_GLOBAL = 32 };
enum : int { FC_EXISTS = 0, FC_KIND, FC_RED_LEVEL, FC_RED_AGENTS, FC_RED_SESSIONS, FC_RED_KNOWS, FC_SVC_ACTIVE, FC_SVC_PRESENT, FC_DECOYS, FC_REL_MIN,
             FC_EVENTS, FC_FILES, FC_NPROC, FC_GREEN, FC_BLUE_SUS, FC_BLUE_AGENT };
enum : int { FG_STEP = 0, FG_STEPS = 1, FG_PHASE = 2, FG_DONE = 3, FG_N_GREEN = 4, FG_BLOCKS = 5, FG_RED_ACTIVE = 14, FG_RED_BUSY = 15, FG_BLUE_BUSY = 16,
             FG_RED_NSESS = 17, FG_RED_EXEC = 23, FG_ERR = 29 };
static_assert((int)FC_BLUE_AGENT == (int)FEAT_PER_HOST - 1 && FG_BLOCKS + NSUB == FG_RED_ACTIVE && FG_RED_NSESS + NRED == FG_RED_EXEC && FG_RED_EXEC + NRED == FG_ERR &&
              (int)FG_ERR < (int)FEAT_GLOBAL, "the columns and words of include/cc4.h");

// The second 32 bytes of a HostDyn row as eight words: word i < MAXSV = svcs[i] (pid | kind << 16 | st << 24), word 7 = nproc | gtmp << 16 | nsf << 24.
// The process slots in front of them are not needed.
enum : int { FEAT_HD_WORDS = 8 };
static_assert(offsetof(HostDyn, svcs) == 32 && sizeof(Svc) == 4 && offsetof(HostDyn, nproc) == 32 + 4 * MAXSV && offsetof(HostDyn, nsf) == 63 && MAXSV == 7,
              "svcs, nproc and nsf are the second half of a HostDyn row");
struct FeatRow { uint32_t w[4]; };      // one host's 16 bytes, little-endian: byte c of the row = column c

// record i of the session pool: false if it is free; else its host and whether the session has RS_ROOT
CC4_HD bool feat_sess_item(const EnvState* s, int i, int* host, bool* root) {
  if (!bit_get(s->spool_used, i)) return false;
  const RSess& q = s->spool[i];
  *host = q.host;
  *root = (q.flags & RS_ROOT) != 0;
  return q.host < MAXH;                 // (a record never names another host; a row from elsewhere must not index past the summary)
}
// green agent g: its host, or -1
CC4_HD int feat_green_item(const EnvState* s, int g) {
  if (g >= (int)s->n_green || g >= MAXG) return -1;
  const int h = s->green_host[g];
  return h < MAXH ? h : -1;
}
CC4_HD int feat_host_kind(int h) {
  if (h == H_INTERNET) return 3;
  const int slot = h % SLOTS;
  return slot == 0 ? 0 : (slot <= MAX_USERS ? 1 : 2);
}
// hd: the eight words above of host h; nsess / root: the red sessions on h over all six agents and whether one of them is a root session;
// green: a green agent lives on h.  A host that is not in the topology is all zero.
CC4_HD FeatRow feat_host_row(const EnvState* s, int h, const uint32_t (&hd)[FEAT_HD_WORDS], uint32_t nsess, bool root, bool green) {
  FeatRow o{{0u, 0u, 0u, 0u}};
  if (!bit_get(s->exists, h)) return o;
  uint32_t agents = 0, knows = 0;
  CC4_UNROLL for (int r = 0; r < NRED; ++r) {
    agents |= (uint32_t)bit_get(s->red[r].live_hosts, h) << r;
    knows |= (uint32_t)bit_get(s->red[r].as_ip, h) << r;
  }
  const uint32_t nsf = hd[7] >> 24, nsvc = nsf & 0xFu, nproc = hd[7] & 0xFFFFu;
  uint32_t active = 0, present = 0, decoys = 0, rel = 0x7Fu;
  CC4_UNROLL for (int i = 0; i < MAXSV; ++i) {
    if ((uint32_t)i >= nsvc) continue;
    const uint32_t kind = (hd[i] >> 16) & 0xFFu, st = hd[i] >> 24;
    if (kind <= (uint32_t)K_SMTP) { present |= 1u << kind; if (st & SV_ACTIVE) active |= 1u << kind; }
    else if (kind <= (uint32_t)K_DEC_VSFTPD) decoys |= 1u << (kind - (uint32_t)K_DEC_APACHE);
    const uint32_t r20 = st & 0x7Fu;
    if (r20 < rel) rel = r20;
  }
  if (nsvc == 0) rel = 0;
  bool sus = false;
  CC4_UNROLL for (int b = 0; b < NBLUE; ++b) sus = sus || bit_get(s->blue[b].sus_hosts, h);
  const int zone = blue_of_subnet(h / SLOTS);
  const uint32_t level = nsess == 0 ? 0u : (root ? 2u : 1u);
  o.w[0] = 1u | ((uint32_t)feat_host_kind(h) << 8) | (level << 16) | (agents << 24);
  o.w[1] = (nsess < 255u ? nsess : 255u) | (knows << 8) | (active << 16) | (present << 24);
  o.w[2] = decoys | ((rel & 0xFFu) << 8) | ((uint32_t)(s->hev[h] & 15u) << 16) | ((nsf >> 4) & (uint32_t)(HF_CMD | HF_ESC)) << 24;
  o.w[3] = (nproc < 255u ? nproc : 255u) | ((green ? 1u : 0u) << 8) | ((sus ? 1u : 0u) << 16) | ((zone < 0 ? 255u : (uint32_t)zone) << 24);
  return o;
}
CC4_HD int32_t feat_global_word(const EnvState* s, int k) {
  if (k == FG_STEP) return s->step_count;
  if (k == FG_STEPS) return s->steps;
  if (k == FG_PHASE) return s->phase;
  if (k == FG_DONE) return (int32_t)s->done;
  if (k == FG_N_GREEN) return (int32_t)s->n_green;
  if (k < FG_RED_ACTIVE) return (int32_t)s->blocks[k - FG_BLOCKS];
  if (k <= FG_BLUE_BUSY) {
    uint32_t m = 0;
    if (k == FG_RED_ACTIVE) { CC4_UNROLL for (int r = 0; r < NRED; ++r) m |= (s->red[r].h.active ? 1u : 0u) << r; }
    else if (k == FG_RED_BUSY) { CC4_UNROLL for (int r = 0; r < NRED; ++r) m |= (s->red[r].h.queue.busy ? 1u : 0u) << r; }
    else { CC4_UNROLL for (int b = 0; b < NBLUE; ++b) m |= (s->blue[b].queue.busy ? 1u : 0u) << b; }
    return (int32_t)m;
  }
  if (k < FG_RED_EXEC) return (int32_t)s->red[k - FG_RED_NSESS].h.nsess;
  if (k < FG_ERR) return (int32_t)s->red[k - FG_RED_EXEC].h.exec_type;
  if (k == FG_ERR) return (int32_t)s->err;
  return 0;
}

// The serial statement: hosts [137][16], glob [32] (or null) from one hot row.
inline void feat_from_row(const EnvState* s, uint8_t* hosts, int32_t* glob) {
  uint32_t cnt[MAXH] = {}, rootm[5] = {}, greenm[5] = {};
  for (int i = 0; i < RS_POOL; ++i) {
    int h; bool root;
    if (!feat_sess_item(s, i, &h, &root)) continue;
    cnt[h]++;
    if (root) rootm[h >> 5] |= 1u << (h & 31);
  }
  for (int g = 0; g < MAXG; ++g) { const int h = feat_green_item(s, g); if (h >= 0) greenm[h >> 5] |= 1u << (h & 31); }
  for (int h = 0; h < MAXH; ++h) {
    uint32_t hd[FEAT_HD_WORDS];
    __builtin_memcpy(hd, reinterpret_cast<const uint8_t*>(&s->hd[h]) + 32, sizeof(hd));
    const FeatRow r = feat_host_row(s, h, hd, cnt[h], bit_get(rootm, h), bit_get(greenm, h));
    __builtin_memcpy(hosts + (size_t)h * FEAT_PER_HOST, r.w, FEAT_PER_HOST);
  }
  if (glob) for (int k = 0; k < FEAT_GLOBAL; ++k) glob[k] = feat_global_word(s, k);
}

}  // namespace cc4
