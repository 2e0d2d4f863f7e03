// Stand-alone check of the host side of blue's own knowledge (csrc/cc4_blue_view.h): blue_view_from_row -- the serial statement of what k_blue_view
// computes, built from the same per-item functions -- on rows, event logs and sus lists filled by hand, against values worked out by hand
// (tests/test_blue_view_cpu.py builds this with the host compiler and the address / undefined-behaviour sanitizers and runs it as a child
// process).  The log and the sus lists are heap blocks of exactly their size, so a read past either is the sanitizer's finding.  Covered: the
// log's count at 0, MAX_EV, MAX_EV + 1 and 0xFFFFFFFF; entries whose host / local address / remote address is 136, 137 or 255; rep 0, 10 and 255;
// 160 x 255 on one host (the clamp, and no carry into the neighbouring fields); nsus at and past the capacity; an executed action whose host is
// past the table; a stale and a disabled log; no cold row at all.  Exit status 0: every case agreed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <initializer_list>
#include "../../cage_challenge_4_amd/csrc/cc4_blue_view.h"
using namespace cc4;

static long fails = 0, cases = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "MISMATCH %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static uint8_t hosts[BV_HOST_BYTES];
static int32_t scal[NBLUE * BV_SCALARS];
static int col(int b, int h, int c) { return hosts[(b * MAXH + h) * BV_PER_HOST + c]; }
static int word(int b, int k) { return scal[b * BV_SCALARS + k]; }
static const int ZONE[9] = {0, 1, 2, 3, -1, 4, 4, 4, -1};

static EvRec ev(int host, int kind, int laddr, int lport, int raddr, int pid, int rep) {
  EvRec e;
  memset(&e, 0, sizeof e);
  e.host = (uint8_t)host; e.kind = (uint8_t)kind; e.laddr = (uint8_t)laddr; e.lport = (uint16_t)lport; e.raddr = (uint8_t)raddr;
  e.rport = 50000; e.pid = (uint16_t)pid; e.rep = (uint8_t)rep; e.order = 200;
  return e;
}
static void set_act(Act* a, int type, int host, int arg) { memset(a, 0, sizeof *a); a->type = (uint8_t)type; a->host = (uint8_t)host; a->arg = (uint8_t)arg; }
// the leak rule on the whole output: outside the existing hosts of the agent's zone only column 5; inside, column 0 is 1
static void leak_rule(const EnvState* s, const char* what) {
  for (int b = 0; b < NBLUE; ++b)
    for (int h = 0; h < MAXH; ++h) {
      const bool in = ZONE[h / 17] == b && bit_get(s->exists, h);
      if (in) CHECK(col(b, h, 0) == 1, "%s: in_zone of (%d, %d)", what, b, h);
      else for (int c = 0; c < 8; ++c) if (c != 5) CHECK(col(b, h, c) == 0, "%s: (%d, %d) column %d = %d outside the zone", what, b, h, c, col(b, h, c));
    }
  for (int b = 0; b < NBLUE; ++b) CHECK(word(b, 14) == 0 && word(b, 15) == 0, "%s: reserved words of %d", what, b);
}
static bool event_columns_zero() {
  for (int k = 0; k < BV_ROWS; ++k) for (int c = 3; c <= 6; ++c) if (hosts[k * BV_PER_HOST + c]) return false;
  for (int b = 0; b < NBLUE; ++b) if (word(b, 11)) return false;
  return true;
}

int main() {
  EnvState* s = static_cast<EnvState*>(aligned_alloc(alignof(EnvState), sizeof(EnvState)));
  EvLog* lg = static_cast<EvLog*>(aligned_alloc(alignof(EvLog), sizeof(EvLog)));        // exactly the log: a read past rec[MAX_EV - 1] is a finding
  const int steps = 500, cap = cold_sus_cap(steps);
  uint32_t* sus = static_cast<uint32_t*>(malloc(sizeof(uint32_t) * NBLUE * cap));       // exactly the five lists
  if (!s || !lg || !sus) return 2;
  CHECK(cap == 768 && cold_sus_cap(30) == 64, "capacities %d %d", cap, cold_sus_cap(30));
  memset(s, 0, sizeof(EnvState));
  memset(lg, 0, sizeof(EvLog));
  memset(sus, 0xFF, sizeof(uint32_t) * NBLUE * cap);
  for (int h = 0; h < MAXH; ++h) if (h != 5) bit_set(s->exists, h);                     // host 5 is not part of the topology
  s->steps = steps; s->step_count = 7; s->phase = 1;
  for (int b = 0; b < NBLUE; ++b) { set_act(&s->bexec[b], BA_SLEEP, 0, 0); s->blue[b].parent_host = (uint8_t)(b < 4 ? 17 * b + 11 : 5 * 17 + 11); }
  for (int h = 0; h < MAXH; ++h) s->hev[h] = 0xFC;                                      // only the low four bits are events
  lg->enabled = 1; lg->step = 6;

  // ---- an empty, valid log: nothing in the event columns, the rest filled
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  leak_rule(s, "empty log");
  CHECK(event_columns_zero(), "empty log: event columns");
  for (int b = 0; b < NBLUE; ++b) {
    CHECK(word(b, 0) == 0 && word(b, 1) == BA_SLEEP && word(b, 2) == 255 && word(b, 3) == 0, "idle agent %d: queue words", b);
    CHECK(word(b, 4) == BA_SLEEP && word(b, 7) == T_UNKNOWN && word(b, 8) == 0 && word(b, 10) == 1 && word(b, 12) == 1 && word(b, 13) == 7, "agent %d: words", b);
    CHECK(word(b, 9) == s->blue[b].parent_host, "agent %d: parent host", b);
  }
  CHECK(col(0, 1, 1) == 0xC && col(4, 86, 1) == 0xC && col(0, 5, 0) == 0 && col(0, 70, 0) == 0 && col(0, 136, 0) == 0, "events nibble / hosts outside");

  // ---- entries by hand
  int n = 0;
  lg->rec[n++] = ev(1, 0, 1, 22, 70, 0, 1);          // (0, 1): one connection on port 22 from host 70 (contractor network)
  lg->rec[n++] = ev(136, 0, 136, 22, 1, 0, 1);       // on the internet root: in no zone -- dropped whole, its remote address too
  lg->rec[n++] = ev(137, 0, 1, 22, 1, 0, 1);         // host past the table
  lg->rec[n++] = ev(255, 0, 1, 22, 1, 0, 1);
  lg->rec[n++] = ev(2, 0, 137, 80, 136, 0, 10);      // (0, 2): ten, port 80, from the internet root; a local address past the table is never an index
  lg->rec[n++] = ev(2, 0, 255, 7, 137, 0, 1);        // (0, 2): one more, no service port, a remote address past the table counts nowhere
  lg->rec[n++] = ev(2, 1, 255, 0, 255, 999, 1);      // (0, 2): a process entry with a pid
  lg->rec[n++] = ev(3, 0, 3, 25, 4, 0, 0);           // rep 0: appended zero times
  lg->rec[n++] = ev(3, 0, 3, 3390, 3, 0, 255);       // (0, 3): 255 from itself
  lg->rec[n++] = ev(18, 1, 18, 22, 255, 0, 1);       // (1, 18): a process entry; its local port is not a service-port bit
  lg->rec[n++] = ev(5, 0, 5, 22, 1, 0, 1);           // a host that does not exist
  lg->rec[n++] = ev(4, 3, 4, 22, 1, 0, 1);           // an unknown kind
  lg->rec[n++] = ev(86, 0, 86, 443, 1, 0, 1);        // (4, 86): from host 1, which lies in agent 0's zone
  lg->rec[n++] = ev(19, 2, 6, 0, 255, 4242, 1);      // a decoy entry nobody's executed action names
  lg->n = (uint32_t)n;
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  leak_rule(s, "entries");
  CHECK(col(0, 1, 3) == 1 && col(0, 1, 4) == 0 && col(0, 1, 6) == PB_22 && col(0, 1, 5) == 0, "(0, 1): %d %d %d %d", col(0, 1, 3), col(0, 1, 4), col(0, 1, 6), col(0, 1, 5));
  CHECK(col(0, 70, 5) == 1 && col(0, 136, 5) == 10 && col(4, 1, 5) == 1 && col(0, 3, 5) == 255, "remote_seen: %d %d %d %d", col(0, 70, 5), col(0, 136, 5), col(4, 1, 5), col(0, 3, 5));
  CHECK(col(0, 2, 3) == 11 && col(0, 2, 4) == 1 && col(0, 2, 6) == (PB_80 | BV_PORT_PID), "(0, 2): %d %d %d", col(0, 2, 3), col(0, 2, 4), col(0, 2, 6));
  CHECK(col(0, 3, 3) == 255 && col(0, 3, 4) == 0 && col(0, 3, 6) == PB_3390, "(0, 3): %d %d %d", col(0, 3, 3), col(0, 3, 4), col(0, 3, 6));
  CHECK(col(1, 18, 3) == 0 && col(1, 18, 4) == 1 && col(1, 18, 6) == 0, "(1, 18): %d %d %d", col(1, 18, 3), col(1, 18, 4), col(1, 18, 6));
  CHECK(col(4, 86, 3) == 1 && col(4, 86, 6) == PB_443 && col(0, 4, 3) == 0 && col(0, 5, 5) == 0 && col(1, 19, 7) == 0, "(4, 86), kind 3, host 5, decoy");
  CHECK(word(0, 11) == 1 + 10 + 1 + 1 + 255 && word(1, 11) == 1 && word(2, 11) == 0 && word(3, 11) == 0 && word(4, 11) == 1, "zone entries: %d %d %d", word(0, 11), word(1, 11), word(4, 11));
  int set5 = 0;
  for (int k = 0; k < BV_ROWS; ++k) set5 += hosts[k * BV_PER_HOST + 5] != 0;
  CHECK(set5 == 4, "rows with remote_seen: %d", set5);

  // ---- the agent's own action: Analyse (files of that one host), DeployDecoy (its log entry), busy, a host past the table
  s->hd[1].nsf = (uint8_t)((HF_CMD | HF_ESC | HF_ESC_LAST) << 4 | 3);
  s->hd[2].nsf = (uint8_t)(HF_CMD << 4);
  set_act(&s->bexec[0], BA_ANALYSE, 1, 0);
  set_act(&s->bexec[1], BA_DECOY, 19, 0);
  set_act(&s->bexec[2], BA_BLOCK, 2, 5); s->blue[2].last_ok = T_FALSE;
  set_act(&s->bexec[3], BA_ALLOW, 3, 4); s->blue[3].last_ok = T_TRUE;
  set_act(&s->bexec[4], BA_RESTORE, 86, 0);
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  leak_rule(s, "own actions");
  CHECK(col(0, 1, 7) == 7 && col(0, 2, 7) == 0 && col(1, 19, 7) == (BV_OWN_DECOY | 6) && col(4, 86, 7) == 0, "own: %d %d %d", col(0, 1, 7), col(0, 2, 7), col(1, 19, 7));
  CHECK(word(0, 7) == T_TRUE && word(1, 7) == T_TRUE && word(2, 7) == T_FALSE && word(3, 7) == T_TRUE && word(4, 7) == T_TRUE, "success words");
  CHECK(word(2, 4) == BA_BLOCK && word(2, 5) == 2 && word(2, 6) == 5 && word(1, 5) == 19, "executed action words");
  int own = 0;
  for (int k = 0; k < BV_ROWS; ++k) own += hosts[k * BV_PER_HOST + 7] != 0;
  CHECK(own == 2, "rows with an own result: %d", own);
  lg->rec[n] = ev(19, 2, 8, 0, 255, 4243, 1); lg->n = (uint32_t)n + 1;       // a later decoy entry for the same host wins
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  CHECK(col(1, 19, 7) == (BV_OWN_DECOY | 8), "the last decoy entry: %d", col(1, 19, 7));
  lg->n = (uint32_t)n;
  s->blue[0].queue.busy = 1; s->blue[0].queue.type = BA_RESTORE; s->blue[0].queue.host = 3; s->blue[0].queue.ticks = 4;
  s->blue[1].queue.busy = 1; s->blue[1].queue.type = BA_REMOVE; s->blue[1].queue.host = 20; s->blue[1].queue.ticks = 2;
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  CHECK(col(0, 1, 7) == 0 && col(1, 19, 7) == 0 && word(0, 0) == 1 && word(0, 1) == BA_RESTORE && word(0, 2) == 3 && word(0, 3) == 4 && word(0, 7) == T_IN_PROGRESS, "a busy agent");
  s->blue[0].queue.busy = 0; s->blue[1].queue.busy = 0;
  for (int host : {137, 200, 255}) {
    set_act(&s->bexec[0], BA_ANALYSE, host, 0);
    set_act(&s->bexec[1], BA_DECOY, host, 0);
    blue_view_from_row(s, lg, sus, steps, hosts, scal);
    leak_rule(s, "executed host past the table");
    own = 0;
    for (int k = 0; k < BV_ROWS; ++k) own += hosts[k * BV_PER_HOST + 7] != 0;
    CHECK(own == 0 && word(0, 5) == host && word(0, 7) == T_TRUE, "executed host %d: %d rows with an own result", host, own);
  }
  set_act(&s->bexec[0], BA_ANALYSE, 18, 0);         // a host of another agent's zone: nothing of its files
  s->hd[18].nsf = (uint8_t)(HF_CMD << 4);
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  leak_rule(s, "Analyse outside the zone");
  CHECK(col(0, 18, 7) == 0 && col(1, 18, 7) == 0, "Analyse outside the zone");
  set_act(&s->bexec[0], 9, 1, 0);                   // a type past the table
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  CHECK(word(0, 7) == 0 && col(0, 1, 7) == 0, "an unknown executed type");
  set_act(&s->bexec[0], BA_SLEEP, 0, 0); set_act(&s->bexec[1], BA_SLEEP, 0, 0);

  // ---- the count of the log: MAX_EV entries of rep 255 on one host (the clamp; no carry into the neighbouring fields), MAX_EV + 1, 0xFFFFFFFF
  for (int i = 0; i < MAX_EV; ++i) lg->rec[i] = ev(1, 0, 1, 9999, 2, 0, 255);
  lg->n = MAX_EV;
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  leak_rule(s, "160 x 255");
  CHECK(col(0, 1, 3) == 255 && col(0, 1, 4) == 0 && col(0, 1, 6) == 0 && col(0, 1, 2) == 0, "160 x 255 connections: %d %d %d %d", col(0, 1, 3), col(0, 1, 4), col(0, 1, 6), col(0, 1, 2));
  CHECK(col(0, 2, 5) == 255 && col(0, 2, 6) == 0 && col(0, 2, 2) == 0 && col(0, 2, 3) == 0, "160 x 255 remote: %d %d %d", col(0, 2, 5), col(0, 2, 6), col(0, 2, 2));
  CHECK(word(0, 11) == MAX_EV * 255 && word(0, 10) == 1, "160 x 255: zone entries %d", word(0, 11));
  for (int i = 0; i < MAX_EV; ++i) lg->rec[i] = ev(1, 1, 1, 22, 255, 1 + i, 255);
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  CHECK(col(0, 1, 3) == 0 && col(0, 1, 4) == 255 && col(0, 1, 6) == BV_PORT_PID && col(0, 1, 5) == 0, "160 x 255 process entries: %d %d %d", col(0, 1, 3), col(0, 1, 4), col(0, 1, 6));
  for (uint32_t cnt : {(uint32_t)MAX_EV + 1u, 0xFFFFFFFFu, 0x80000000u}) {
    lg->n = cnt;
    blue_view_from_row(s, lg, sus, steps, hosts, scal);
    leak_rule(s, "truncated log");
    CHECK(event_columns_zero() && word(0, 10) == 0 && word(4, 10) == 0, "a log of %u entries is not valid", cnt);
  }
  // ---- a stale, a future and a disabled log; a row that has taken no step
  lg->n = MAX_EV;
  for (uint32_t st : {5u, 7u, 0u, 0xFFFFFFFFu}) {
    lg->step = st;
    blue_view_from_row(s, lg, sus, steps, hosts, scal);
    CHECK(event_columns_zero() && word(0, 10) == 0, "a log of step %u for a row at step_count 7", st);
  }
  lg->step = 6; lg->enabled = 0;
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  CHECK(event_columns_zero() && word(0, 10) == 0, "a disabled log");
  lg->enabled = 1; s->step_count = 0; lg->step = 0xFFFFFFFFu;
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  CHECK(event_columns_zero() && word(0, 10) == 0 && word(0, 13) == 0, "a regenerated episode has no step behind it");
  s->step_count = 7; lg->step = 6; lg->n = 0;

  // ---- sus lists: counts per host, entries that name no host of the zone, saturation, nsus at and past the capacity
  for (int b = 0; b < NBLUE; ++b) for (int i = 0; i < cap; ++i) sus[b * cap + i] = (uint32_t)(b < 4 ? 17 * b + 1 : 86) << 16 | (uint32_t)(1000 + i);
  sus[0] = 18u << 16 | 5;          // agent 0's list names a host of agent 1's zone
  sus[1] = 137u << 16 | 5; sus[2] = 255u << 16 | 5; sus[3] = 0xFFFFu << 16 | 5; sus[4] = 5u << 16 | 5;      // past the table; not in the topology
  sus[5] = 2u << 16 | 5;
  s->blue[0].nsus = 6; s->blue[1].nsus = 254; s->blue[2].nsus = 255; s->blue[3].nsus = 256; s->blue[4].nsus = (uint16_t)cap;
  blue_view_from_row(s, lg, sus, steps, hosts, scal);
  leak_rule(s, "sus lists");
  CHECK(col(0, 2, 2) == 1 && col(0, 1, 2) == 0 && col(1, 18, 2) == 254 && col(2, 35, 2) == 255 && col(3, 52, 2) == 255 && col(4, 86, 2) == 255, "sus_pids: %d %d %d %d %d %d",
        col(0, 2, 2), col(0, 1, 2), col(1, 18, 2), col(2, 35, 2), col(3, 52, 2), col(4, 86, 2));
  CHECK(word(0, 8) == 6 && word(3, 8) == 256 && word(4, 8) == cap && event_columns_zero(), "nsus words");
  int withsus = 0;
  for (int k = 0; k < BV_ROWS; ++k) withsus += hosts[k * BV_PER_HOST + 2] != 0;
  CHECK(withsus == 5, "rows with sus pids: %d", withsus);
  for (int ns : {cap + 1, 65535}) {                 // past the capacity: the list is read to its capacity and no further
    s->blue[4].nsus = (uint16_t)ns; s->blue[0].nsus = (uint16_t)ns;
    blue_view_from_row(s, lg, sus, steps, hosts, scal);
    leak_rule(s, "nsus past the capacity");
    CHECK(col(4, 86, 2) == 255 && col(0, 1, 2) == 255 && col(0, 2, 2) == 1 && word(4, 8) == ns, "nsus %d: %d %d %d", ns, col(4, 86, 2), col(0, 1, 2), col(0, 2, 2));
  }
  {                                                   // a short episode: its capacity is 64, and so is the block
    const int cap30 = cold_sus_cap(30);
    uint32_t* small = static_cast<uint32_t*>(malloc(sizeof(uint32_t) * NBLUE * cap30));
    if (!small) return 2;
    for (int i = 0; i < NBLUE * cap30; ++i) small[i] = 86u << 16 | (uint32_t)i;
    s->blue[0].nsus = 0; s->blue[4].nsus = 65535;
    blue_view_from_row(s, lg, small, 30, hosts, scal);
    CHECK(col(4, 86, 2) == cap30 && col(3, 86, 2) == 0, "steps 30: %d", col(4, 86, 2));
    free(small);
  }

  // ---- no cold row: columns 2..6 and the decoy bits 0, events_valid 0, the hot row's part as before; no agent words wanted
  set_act(&s->bexec[0], BA_ANALYSE, 1, 0);
  set_act(&s->bexec[1], BA_DECOY, 19, 0);
  blue_view_from_row(s, nullptr, nullptr, steps, hosts, scal);
  leak_rule(s, "no cold row");
  bool cold_cols = false;
  for (int k = 0; k < BV_ROWS; ++k) for (int c = 2; c <= 6; ++c) cold_cols |= hosts[k * BV_PER_HOST + c] != 0;
  CHECK(!cold_cols && col(0, 1, 7) == 7 && col(1, 19, 7) == 0 && word(0, 10) == 0 && word(4, 8) == 65535 && word(0, 7) == T_TRUE, "no cold row");
  memset(hosts, 0xEE, sizeof hosts);
  blue_view_from_row(s, lg, sus, steps, hosts, nullptr);
  CHECK(col(0, 1, 0) == 1 && col(0, 70, 0) == 0, "no agent words wanted");

  printf("blue_view_check: %ld cases, %ld mismatches\n", cases, fails);
  free(s); free(lg); free(sus);
  return fails ? 1 : 0;
}
