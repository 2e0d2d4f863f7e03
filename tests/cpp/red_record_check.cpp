// Stand-alone check of the host side of the red agents as learners (csrc/cc4_red_view.h): red_record -- the one conversion and validation of a
// submitted red action that k_red_submit and cc4_red_record_from_row share -- against the record cc4_step_ex would be handed, rule by rule, and
// red_view_from_row on rows filled by hand (tests/test_red_record_cpu.py builds this with the host compiler and the address / undefined-behaviour
// sanitizers and runs it as a child process).  Exit status 0: every case agreed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include "../../cage_challenge_4_amd/csrc/cc4_red_view.h"
using namespace cc4;

static long fails = 0, cases = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "MISMATCH %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// agent r gets `n` sessions with ids id0, id0 + 1, .. in pool slots slot0, slot0 + 1, .. on hosts host0, host0 + 1, ..
static void give_sessions(EnvState* s, int r, int n, int id0, int slot0, int host0, int flags) {
  RedAgent& A = s->red[r];
  A.h.nsess = (uint8_t)n;
  for (int i = 0; i < n; ++i) {
    A.sord[i] = (uint8_t)(slot0 + i);
    RSess& q = s->spool[slot0 + i];
    q.id = (uint16_t)(id0 + i); q.host = (uint8_t)(host0 + i); q.flags = (uint8_t)flags; q.pid = 1;
    s->spool_used[(slot0 + i) >> 5] |= 1u << ((slot0 + i) & 31);
  }
}
static bool is_none(const ExtActW& w) { return w.w[0] == ~0ull && w.w[1] == ~0ull && w.w[2] == ~0ull; }
// what the record must be, written member by member
static bool same_record(const ExtActW& w, int type, int host, int arg, int sid) {
  ExtAct a;
  memset(&a, 0, sizeof a);
  a.type = (int8_t)type; a.host = (uint8_t)host; a.arg = (uint8_t)arg; a.ticks = 0; a.sid = (uint16_t)sid; a.flags = 0; a.rate0 = 0.0; a.rate1 = 0.0;
  return memcmp(&a, w.w, sizeof a) == 0;
}
// the host loop of cc4_step_ex on a red record (csrc/cc4_api.hip): true = refused
static bool step_ex_refuses(int type, int host, int arg) {
  if (type == XA_NONE) return false;
  return type < 0 || type > RA_INVALID || host >= MAXH || (type == RA_DRS && arg >= NSUB) || (type == RA_WITHDRAW && arg >= MAXH);
}

int main() {
  EnvState* s = static_cast<EnvState*>(aligned_alloc(alignof(EnvState), sizeof(EnvState)));
  if (!s) return 2;
  memset(s, 0, sizeof(EnvState));
  give_sessions(s, 1, 1, 7, 10, 20, 0);                       // agent 0: none; agent 1: one session (id 7); agent 2: five (ids 300..304)
  give_sessions(s, 2, 5, 300, 40, 30, RS_ROOT);
  ExtActW w;

  // ---- every refusal rule, over the whole grid of types, hosts and args that a byte-sized field can hold, against cc4_step_ex's loop
  for (int type = -3; type <= 13; ++type)
    for (int host : {0, 1, 135, 136, 137, 200, 255})
      for (int arg : {0, 8, 9, 136, 137, 200, 255}) {
        const bool ok = red_record(s, 1, type, host, arg, 7, &w);
        CHECK(ok == !step_ex_refuses(type, host, arg), "type %d host %d arg %d: ok %d", type, host, arg, (int)ok);
        if (!ok || type == XA_NONE) CHECK(is_none(w), "type %d host %d arg %d: a refused / absent record is none", type, host, arg);
        else CHECK(same_record(w, type, host, arg, 7), "type %d host %d arg %d: the record's bytes", type, host, arg);
      }
  // the four cases by name: a type 11, a host 137, a DiscoverRemoteSystems subnet 9, a Withdraw hostname 200
  CHECK(!red_record(s, 1, 11, 3, 0, 7, &w) && is_none(w), "type 11");
  CHECK(!red_record(s, 1, RA_EXPLOIT, 137, 0, 7, &w) && is_none(w), "host 137");
  CHECK(!red_record(s, 1, RA_DRS, 3, 9, 7, &w) && is_none(w), "subnet 9");
  CHECK(!red_record(s, 1, RA_WITHDRAW, 3, 200, 7, &w) && is_none(w), "withdraw 200");
  CHECK(red_record(s, 1, RA_DRS, 3, 8, 7, &w) && red_record(s, 1, RA_WITHDRAW, 3, 136, 7, &w) && red_record(s, 1, RA_IMPACT, 136, 200, 7, &w), "the last values in range");
  // what the record's fields cannot hold
  CHECK(!red_record(s, 1, RA_EXPLOIT, -1, 0, 7, &w) && is_none(w), "host -1");
  CHECK(!red_record(s, 1, RA_EXPLOIT, 3, -1, 7, &w) && !red_record(s, 1, RA_EXPLOIT, 3, 256, 7, &w), "arg beyond a byte");
  CHECK(!red_record(s, 1, RA_EXPLOIT, 3, 0, -2, &w) && !red_record(s, 1, RA_EXPLOIT, 3, 0, 65536, &w) && is_none(w), "session beyond an id");
  CHECK(!red_record(s, 1, -128, 3, 0, 7, &w) && !red_record(s, 1, 255, 3, 0, 7, &w) && !red_record(s, 1, 0x7FFFFFFF, 3, 0, 7, &w) &&
        !red_record(s, 1, (int32_t)0x80000000u, 3, 0, 7, &w), "types far out of range");
  CHECK(red_record(s, 1, XA_NONE, 999, -999, 123456, &w) && is_none(w), "no action: the other words are not looked at");
  CHECK(red_record(s, 1, RA_SLEEP, 5, 6, 65535, &w) && same_record(w, RA_SLEEP, 5, 6, 65535), "the largest id");

  // ---- CC4_RED_SID_AUTO with no, one and several sessions
  CHECK(red_auto_sid(s, 0) == (uint32_t)RED_SID_NONE && red_auto_sid(s, 1) == 7 && red_auto_sid(s, 2) == 300, "auto ids %u %u %u", red_auto_sid(s, 0), red_auto_sid(s, 1), red_auto_sid(s, 2));
  CHECK(red_record(s, 0, RA_EXPLOIT, 20, 0, RED_SID_AUTO, &w) && same_record(w, RA_EXPLOIT, 20, 0, 0), "auto without a session: id 0");
  CHECK(red_record(s, 1, RA_EXPLOIT, 20, 0, RED_SID_AUTO, &w) && same_record(w, RA_EXPLOIT, 20, 0, 7), "auto with one session");
  CHECK(red_record(s, 2, RA_PRIVESC, 31, 0, RED_SID_AUTO, &w) && same_record(w, RA_PRIVESC, 31, 0, 300), "auto with five sessions: the first listed");
  s->red[2].sord[0] = 44; s->red[2].sord[4] = 40;             // the list's order decides, not the ids or the pool slots
  CHECK(red_record(s, 2, RA_PRIVESC, 31, 0, RED_SID_AUTO, &w) && same_record(w, RA_PRIVESC, 31, 0, 304), "auto follows the list's order");
  s->red[2].sord[0] = 250;                                    // a list entry past the pool (a row from elsewhere): no read past it
  CHECK(red_auto_sid(s, 2) == (uint32_t)RED_SID_NONE && red_record(s, 2, RA_PRIVESC, 31, 0, RED_SID_AUTO, &w) && same_record(w, RA_PRIVESC, 31, 0, 0), "a list entry past the pool");
  s->red[2].sord[0] = 44;

  // ---- the view of the same row: sessions of the agent only, the leak rule, a list of the full length, entries that point outside
  uint8_t* hosts = static_cast<uint8_t*>(malloc(RV_HOST_BYTES));
  int32_t* scal = static_cast<int32_t*>(malloc(sizeof(int32_t) * NRED * RV_SCALARS));
  if (!hosts || !scal) return 2;
  s->red[1].h.start_host = 20; s->red[1].h.active = 1; s->red[1].as_ip[0] = 1u << 5;
  s->red[1].h.nobs = 2; s->red[1].obs[0] = ObsEnt{9, OE_KEY_IP}; s->red[1].obs[1] = ObsEnt{9, OE_SESS};
  for (int r = 0; r < NRED; ++r) if (r != 1) s->red[r].h.start_host = 0xFF;
  s->step_count = 12;
  red_view_from_row(s, hosts, scal);
  auto col = [&](int r, int h, int c) { return (int)hosts[((size_t)r * MAXH + h) * RV_PER_HOST + c]; };
  CHECK(col(1, 20, RVC_SESSION_LEVEL) == 1 && col(1, 20, RVC_SESSIONS) == 1 && col(1, 20, RVC_START) == 1 && col(1, 20, RVC_ABSTRACT) == 0, "agent 1's session host");
  CHECK(col(1, 5, RVC_KNOWN_IP) == 1 && col(1, 5, RVC_KNOWN_HOSTNAME) == 0 && col(1, 9, RVC_OBS) == (0x80 | OE_KEY_IP | OE_SESS), "agent 1's knowledge and observation");
  CHECK(col(2, 30, RVC_SESSION_LEVEL) == 2 && col(2, 34, RVC_SESSIONS) == 1, "agent 2's root sessions");
  for (int h = 0; h < MAXH; ++h) {
    for (int c = 0; c < RV_PER_HOST; ++c) CHECK(col(0, h, c) == 0 && col(3, h, c) == 0, "agents without knowledge: host %d column %d", h, c);
    if (h >= 30 && h <= 34) for (int c = 0; c < RV_PER_HOST; ++c) CHECK(col(1, h, c) == 0, "agent 2's sessions do not show in agent 1's view: host %d column %d", h, c);
  }
  CHECK(scal[1 * RV_SCALARS + RVW_ACTIVE] == 1 && scal[1 * RV_SCALARS + RVW_BUSY] == 0 && scal[1 * RV_SCALARS + RVW_Q_TYPE] == RA_NONE && scal[1 * RV_SCALARS + RVW_Q_HOST] == 255 &&
        scal[1 * RV_SCALARS + RVW_NSESS] == 1 && scal[1 * RV_SCALARS + RVW_AUTO_SID] == 7 && scal[0 * RV_SCALARS + RVW_AUTO_SID] == RED_SID_NONE &&
        scal[2 * RV_SCALARS + RVW_AUTO_SID] == 304 && scal[5 * RV_SCALARS + RVW_STEP_COUNT] == 12, "the agent words");
  // a full list on one host saturates nowhere and counts 64; a claimed length past the list, entries past the pool and hosts past the table are not read past
  give_sessions(s, 4, MAX_RS, 1000, 100, 50, RS_ABSTRACT);
  for (int i = 0; i < MAX_RS; ++i) s->spool[100 + i].host = 50;
  s->red[4].h.nsess = 255;
  s->red[5].h.nsess = 3; s->red[5].sord[0] = 255; s->red[5].sord[1] = 191; s->spool[191].host = 200; s->red[5].sord[2] = 10;
  s->red[5].h.nobs = 255; for (int i = 0; i < MAX_OBS; ++i) s->red[5].obs[i] = ObsEnt{(uint8_t)(130 + i), OE_IFACE};
  red_view_from_row(s, hosts, nullptr);
  CHECK(col(4, 50, RVC_SESSIONS) == MAX_RS && col(4, 50, RVC_ABSTRACT) == 1 && col(4, 50, RVC_SESSION_LEVEL) == 1, "a full session list on one host: %d", col(4, 50, RVC_SESSIONS));
  CHECK(col(5, 20, RVC_SESSIONS) == 1 && col(5, 136, RVC_OBS) == (0x80 | OE_IFACE) && col(5, 130, RVC_OBS) == (0x80 | OE_IFACE), "entries that point outside are skipped");

  free(hosts); free(scal); free(s);
  printf("red_record_check: %ld cases, %ld mismatches\n", cases, fails);
  return fails ? 1 : 0;
}
