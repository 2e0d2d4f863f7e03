// Stand-alone check of the host side of the Monitor's connection edges (csrc/cc4_blue_edges.h): blue_edges_from_row -- the serial statement of what
// k_blue_edges computes, built from the same per-item functions (ranking: position = distinct smaller keys) -- against a deliberately different
// formulation here: a std::map from the key tuple to the summed count, walked in order (tests/test_blue_edges_cpu.py builds this with the host
// compiler and the address / undefined-behaviour sanitizers and runs it as a child process).  The hot row, the log and the outputs are heap blocks
// of exactly their size, so a read or write past any of them is the sanitizer's finding.  Covered: logs of 0, 1, 64, 65, 160 and 161 entries; 160
// equal keys; keys that differ only in the remote port; one multiset in three physical orders; equal keys under different order bytes and pids;
// entries that do not qualify (kind 1 and 2, rep 0, a host past the table, a host that does not exist, hosts of subnets 4 and 8, no remote
// address) and a local address past the table; max_edges 1, total - 1, total and 160; a stale log, a disabled log, no cold row.
// Exit status 0: every case agreed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <array>
#include <initializer_list>
#include <map>
#include <vector>
#include "../../cage_challenge_4_amd/csrc/cc4_blue_edges.h"
using namespace cc4;

static long fails = 0, cases = 0;
#define CHECK(cond, ...) do { ++cases; if (!(cond)) { if (fails++ < 20) { fprintf(stderr, "MISMATCH %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

static const int ZONE[9] = {0, 1, 2, 3, -1, 4, 4, 4, -1};
static EnvState* s;
static EvLog* lg;

static EvRec ev(int host, int kind, int laddr, int lport, int raddr, int rport, int rep, int pid = 0, int order = 200) {
  EvRec e;
  memset(&e, 0, sizeof e);
  e.host = (uint8_t)host; e.kind = (uint8_t)kind; e.laddr = (uint8_t)laddr; e.lport = (uint16_t)lport; e.raddr = (uint8_t)raddr;
  e.rport = (uint16_t)rport; e.pid = (uint16_t)pid; e.rep = (uint8_t)rep; e.order = (uint8_t)order;
  return e;
}
static uint32_t rnd_state = 12345;
static uint32_t rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

typedef std::array<int, 6> Key;      // agent, host, remote, local byte, local port, remote port
// the other formulation: filter, std::map, in-order walk
static void by_map(const EvLog* log, bool usable, int E, std::vector<int32_t>* edges, int32_t* counts) {
  std::map<Key, long> ms;
  if (usable)
    for (uint32_t i = 0; i < log->n; ++i) {
      const EvRec& e = log->rec[i];
      if (e.kind != 0 || e.rep == 0 || e.host > 136 || e.raddr > 136) continue;
      if (!((s->exists[e.host >> 5] >> (e.host & 31)) & 1u)) continue;
      const int b = ZONE[e.host / 17];
      if (b < 0) continue;
      ms[Key{b, e.host, e.raddr, e.laddr, e.lport, e.rport}] += e.rep;
    }
  edges->assign((size_t)E * 8, -1);
  for (int k = 0; k < 8; ++k) counts[k] = 0;
  int at = 0;
  for (const auto& kv : ms) {
    const Key& k = kv.first;
    if (at < E) {
      int32_t* r = edges->data() + (size_t)at * 8;
      r[0] = k[0]; r[1] = k[1]; r[2] = k[3] <= 136 ? k[3] : -1; r[3] = k[2]; r[4] = k[4]; r[5] = k[5]; r[6] = (int32_t)kv.second; r[7] = counts[k[0]];
    }
    ++counts[k[0]]; ++counts[5]; ++at;
  }
  counts[6] = usable ? 1 : 0; counts[7] = s->step_count;
}
// the statement under test into heap blocks of exactly max_edges rows and 8 words; returns the total
static int run(const char* what, const EvLog* log, bool usable, int E, std::vector<int32_t>* keep = nullptr) {
  int32_t* edges = static_cast<int32_t*>(malloc(sizeof(int32_t) * 8 * (size_t)E));
  int32_t* counts = static_cast<int32_t*>(malloc(sizeof(int32_t) * 8));
  if (!edges || !counts) exit(2);
  memset(edges, 0x5A, sizeof(int32_t) * 8 * (size_t)E);
  memset(counts, 0x5A, sizeof(int32_t) * 8);
  blue_edges_from_row(s, log, E, edges, counts);
  std::vector<int32_t> want;
  int32_t wc[8];
  by_map(log, usable, E, &want, wc);
  CHECK(memcmp(edges, want.data(), sizeof(int32_t) * 8 * (size_t)E) == 0, "%s, max_edges %d: edges", what, E);
  CHECK(memcmp(counts, wc, sizeof wc) == 0, "%s, max_edges %d: counts %d %d %d %d %d %d %d %d", what, E, counts[0], counts[1], counts[2], counts[3], counts[4], counts[5], counts[6], counts[7]);
  int sum = 0;
  for (int b = 0; b < NBLUE; ++b) sum += counts[b];
  CHECK(sum == counts[5], "%s: the agents' counts sum to the total", what);
  for (int r = 0; r < E; ++r) {                       // structure: -1 rows exactly past the edges; slots restart per agent
    const bool live = r < counts[5];
    CHECK((edges[8 * r] >= 0) == live, "%s: row %d of %d", what, r, counts[5]);
    if (live) CHECK(edges[8 * r + 7] == (r == 0 || edges[8 * (r - 1)] != edges[8 * r] ? 0 : edges[8 * (r - 1) + 7] + 1), "%s: slot of row %d", what, r);
  }
  memset(edges, 0x5A, sizeof(int32_t) * 8 * (size_t)E);      // no counts wanted
  blue_edges_from_row(s, log, E, edges, nullptr);
  CHECK(memcmp(edges, want.data(), sizeof(int32_t) * 8 * (size_t)E) == 0, "%s, max_edges %d: edges without counts", what, E);
  if (keep) keep->assign(edges, edges + 8 * (size_t)E);
  const int total = counts[5];
  free(edges); free(counts);
  return total;
}
static void run_all(const char* what, const EvLog* log, bool usable) {
  const int total = run(what, log, usable, BE_MAX);
  for (int E : {1, total - 1, total, 7}) if (E >= 1 && E <= BE_MAX) run(what, log, usable, E);
}
// zone hosts that exist (host 5 does not), a few ports and remote hosts: duplicates are frequent
static EvRec random_entry() {
  static const int hosts[] = {1, 2, 3, 18, 19, 35, 52, 53, 86, 87, 103, 120};
  static const int ports[] = {22, 80, 443, 0};
  static const int remotes[] = {1, 18, 70, 71, 136, 86};
  const int h = hosts[rnd() % 12];
  return ev(h, 0, rnd() % 3 ? h : (int)(rnd() % 137), ports[rnd() % 4], remotes[rnd() % 6], 50000 + (int)(rnd() % 3), 1 + (int)(rnd() % 3 == 0) * 9, (int)(rnd() % 2000), (int)(rnd() % 206));
}

int main() {
  s = static_cast<EnvState*>(aligned_alloc(alignof(EnvState), sizeof(EnvState)));      // exactly the row, exactly the log
  lg = static_cast<EvLog*>(aligned_alloc(alignof(EvLog), sizeof(EvLog)));
  if (!s || !lg) return 2;
  memset(s, 0, sizeof(EnvState));
  memset(lg, 0, sizeof(EvLog));
  for (int h = 0; h < MAXH; ++h) if (h != 5) bit_set(s->exists, h);
  s->steps = 500; s->step_count = 7;
  lg->enabled = 1; lg->step = 6;

  // ---- random logs of every length the kernel treats differently (rounds of 64), and one entry past the log's capacity
  for (int n : {0, 1, 63, 64, 65, 128, 160}) {
    for (int i = 0; i < n; ++i) lg->rec[i] = random_entry();
    lg->n = (uint32_t)n;
    char what[64];
    snprintf(what, sizeof what, "%d random entries", n);
    run_all(what, lg, true);
  }
  for (uint32_t n : {161u, 0xFFFFFFFFu}) {
    lg->n = n;
    CHECK(run("a truncated log", lg, false, BE_MAX) == 0, "a log of %u entries gives no edges", n);
    run("a truncated log", lg, false, 1);
  }
  // ---- 160 equal keys: one edge whose count is the sum; with rep 255 the largest count there is
  for (int rep : {1, 255}) {
    for (int i = 0; i < MAX_EV; ++i) lg->rec[i] = ev(1, 0, 1, 22, 70, 50000, rep, i, i);
    lg->n = MAX_EV;
    std::vector<int32_t> got;
    CHECK(run("160 equal keys", lg, true, BE_MAX, &got) == 1 && got[6] == MAX_EV * rep && got[7] == 0 && got[8] == -1, "160 equal keys: count %d", got[6]);
    run("160 equal keys", lg, true, 1);
  }
  // ---- 160 distinct keys that differ only in the remote port, descending in the log
  for (int i = 0; i < MAX_EV; ++i) lg->rec[i] = ev(18, 0, 18, 22, 70, 60000 - i, 1);
  {
    std::vector<int32_t> got;
    CHECK(run("remote ports", lg, true, BE_MAX, &got) == MAX_EV && got[5] == 60000 - 159 && got[8 * 159 + 5] == 60000 && got[8 * 159 + 7] == 159 && got[0] == 1, "remote ports");
    run("remote ports", lg, true, 159); run("remote ports", lg, true, 1);
  }
  // ---- one multiset in three physical orders: identical bytes
  {
    EvRec base[100];
    for (int i = 0; i < 100; ++i) base[i] = random_entry();
    std::vector<int32_t> a, b, c;
    for (int i = 0; i < 100; ++i) lg->rec[i] = base[i];
    lg->n = 100;
    run_all("order 1", lg, true); run("order 1", lg, true, BE_MAX, &a);
    for (int i = 0; i < 100; ++i) lg->rec[i] = base[99 - i];
    run("order 2", lg, true, BE_MAX, &b);
    for (int i = 0; i < 100; ++i) lg->rec[i] = base[(i * 37 + 11) % 100];
    run("order 3", lg, true, BE_MAX, &c);
    CHECK(a == b && a == c, "the list is a function of the multiset");
    // ... and the order byte and the pid reach nothing
    for (int i = 0; i < 100; ++i) { lg->rec[i] = base[i]; lg->rec[i].order = (uint8_t)(i % 2 ? 200 + i % 6 : i); lg->rec[i].pid = (uint16_t)(7 * i); }
    run("order bytes and pids", lg, true, BE_MAX, &b);
    CHECK(a == b, "order bytes and pids reach nothing");
  }
  // ---- what does not qualify, one by one among entries that do
  {
    int n = 0;
    lg->rec[n++] = ev(1, 0, 1, 22, 70, 50000, 1);
    lg->rec[n++] = ev(1, 1, 1, 22, 70, 50000, 1);         // a process entry
    lg->rec[n++] = ev(1, 2, 6, 0, 70, 0, 1);              // a decoy entry
    lg->rec[n++] = ev(1, 3, 1, 22, 70, 50000, 1);         // an unknown kind
    lg->rec[n++] = ev(1, 0, 1, 22, 70, 50000, 0);         // appended zero times
    lg->rec[n++] = ev(137, 0, 1, 22, 70, 50000, 1);       // hosts past the table
    lg->rec[n++] = ev(255, 0, 1, 22, 70, 50000, 1);
    lg->rec[n++] = ev(5, 0, 5, 22, 70, 50000, 1);         // a host that does not exist
    lg->rec[n++] = ev(70, 0, 70, 22, 1, 50000, 1);        // the contractor network: no zone
    lg->rec[n++] = ev(136, 0, 136, 22, 1, 50000, 1);      // the internet root: no zone
    lg->rec[n++] = ev(2, 0, 2, 22, 0xFF, 0, 1);           // no remote address
    lg->rec[n++] = ev(2, 0, 2, 22, 137, 0, 1);
    lg->rec[n++] = ev(2, 0, 137, 22, 136, 1, 3);          // local addresses past the table: column 2 is -1, the byte still tells keys apart
    lg->rec[n++] = ev(2, 0, 255, 22, 136, 1, 4);
    lg->rec[n++] = ev(120, 0, 120, 0, 5, 0, 2);           // a remote host that does not exist is still a host id
    lg->n = (uint32_t)n;
    std::vector<int32_t> got;
    const int total = run("qualification", lg, true, BE_MAX, &got);
    static const int32_t want[4][8] = {{0, 1, 1, 70, 22, 50000, 1, 0}, {0, 2, -1, 136, 22, 1, 3, 1}, {0, 2, -1, 136, 22, 1, 4, 2}, {4, 120, 120, 5, 0, 0, 2, 0}};
    CHECK(total == 4 && memcmp(got.data(), want, sizeof want) == 0, "qualification: %d edges", total);
    run_all("qualification", lg, true);
  }
  // ---- a stale, a future and a disabled log; a row that has taken no step; no cold row
  for (int i = 0; i < 100; ++i) lg->rec[i] = random_entry();
  lg->n = 100;
  for (uint32_t st : {5u, 7u, 0u, 0xFFFFFFFFu}) { lg->step = st; CHECK(run("a stale log", lg, false, BE_MAX) == 0, "a log of step %u for a row at step_count 7", st); }
  lg->step = 6; lg->enabled = 0;
  CHECK(run("a disabled log", lg, false, BE_MAX) == 0, "a disabled log");
  lg->enabled = 1; s->step_count = 0; lg->step = 0xFFFFFFFFu;
  CHECK(run("no step taken", lg, false, 3) == 0, "a regenerated episode has no step behind it");
  s->step_count = 7; lg->step = 6;
  CHECK(run("no cold row", nullptr, false, BE_MAX) == 0 && run("no cold row", nullptr, false, 1) == 0, "no cold row");
  CHECK(run("valid again", lg, true, BE_MAX) > 20, "the same log, valid");

  printf("blue_edges_check: %ld cases, %ld mismatches\n", cases, fails);
  free(s); free(lg);
  return fails ? 1 : 0;
}
