// Stand-alone run of the engine (csrc/cc4_engine.h, host build) on episodes whose bounded containers are one below, at and past their capacity
// (tests/test_capacity_cpu.py builds this with the host compiler and the address / undefined-behaviour sanitizers and runs it as a child
// process).  The hot rows and the cold rows of all episodes are two heap blocks of exactly n rows, back to back as a handle holds them.  Crafted
// episodes sit on the even rows and on the last one; the odd rows in between are never generated and must still be all zero at the end -- a store
// past a container's capacity lands in the neighbouring field (sus[4] is followed by povf[0]), in the next episode's row (the last host's povf row
// ends the cold row) or behind the block, where it is the sanitizer's finding.  Every variant is filled through state_edit (and by stores into
// the row where no op exists), takes its overflowing operation -- an edit, a submitted exploit or phishing e-mail, a DeployDecoy / Monitor of a
// blue agent -- and then 2 x steps steps of seeded random blue actions with autoreset, in both RNG modes.  Exit status 0: no out-of-bounds access,
// every neighbour row untouched, every designed flag raised on the step of its operation.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../cage_challenge_4_amd/csrc/cc4_engine.h"
using namespace cc4;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static long fails = 0, checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { if (fails++ < 30) { fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

enum Container { RS_ADD, RS_EXPLOIT, RS_REASSIGN, POOL0, POOL1, POOL2, POOL3, POOL_PHISH, KNOWN, KNOWN256, PROC_PIN, PROC_EDIT, PROC_DECOY, PROC_EXPLOIT,
                 PROC_PHISH, SUS0_END, SUS4_END, SUS0_MON, SUS4_MON, PEND, N_CONTAINERS };
enum Variant { M1, CAP, OVER, N_VARIANTS };
static const int RED_SUB[NRED][3] = {{4, -1, -1}, {0, -1, -1}, {1, -1, -1}, {2, -1, -1}, {3, -1, -1}, {5, 6, 7}};
static const int BLUE_SUB[NBLUE][3] = {{0, -1, -1}, {1, -1, -1}, {2, -1, -1}, {3, -1, -1}, {5, 6, 7}};

struct Ep {
  Ctx x; StepWork w; int steps;
  ExtAct ext[EXT_PER_ENV]; bool has_ext = false;
  int32_t blue[NBLUE]; bool has_blue = false;
  struct Edit { int op, a0, a1, a2, want; }; std::vector<Edit> edits;
  uint32_t flag = 0; Variant v = CAP; int container = 0;
  EnvState* s() { return x.s; }
  int edit(int op, int a0, int a1, int a2) { memset(&w, 0, sizeof(w)); return state_edit(x, op, a0, a1, a2); }
  std::vector<int> zone(const int* subs) {
    std::vector<int> out;
    for (int h = 0; h < H_INTERNET; ++h) {
      if (!bit_get(s()->exists, h) || h % SLOTS == 0) continue;
      for (int i = 0; i < 3; ++i) if (subs[i] == h / SLOTS) out.push_back(h);
    }
    return out;
  }
  int nsess_all() { int n = 0; for (int r = 0; r < NRED; ++r) n += s()->red[r].h.nsess; return n; }
  void fill_agent(int r, int total, int avoid = -1, int salt = 0) {
    std::vector<int> z = zone(RED_SUB[r]);
    for (int j = salt; s()->red[r].h.nsess < total; ++j) {
      const int h = z[(size_t)j % z.size()];
      if (h == avoid) continue;
      const int before = s()->red[r].h.nsess;
      int mx = -1; for (int i = 0; i < before; ++i) mx = rsw_id(rs_at(s(), s()->red[r], i)) > mx ? rsw_id(rs_at(s(), s()->red[r], i)) : mx;
      const int rc = edit(SE_ADD_RED_SESSION, r, h, (j % 4 == 1 ? 1 : 0) | (j % 5 == 2 ? 2 : 0) | (j % 3 != 0 ? 4 : 0));
      CHECK(rc == mx + 1 && s()->red[r].h.nsess == before + 1, "agent %d: add %d gave ident %d after max %d", r, before, rc, mx);
      if (rc < 0) break;
    }
  }
  void fill_pool(int free_records, int avoid = -1) {
    int per[NRED]; for (int r = 0; r < NRED; ++r) per[r] = RS_POOL / NRED;
    for (int k = NRED - 1, sum = RS_POOL; sum > RS_POOL - free_records; k = (k + NRED - 1) % NRED) { per[k]--; sum--; }
    for (int r = 0; r < NRED; ++r) fill_agent(r, per[r], avoid, r);
    CHECK(nsess_all() == RS_POOL - free_records, "pool holds %d", nsess_all());
  }
  void fill_host(int h, int total) {
    while ((int)x.hd[h].nproc < total) {
      const int n = x.hd[h].nproc;
      const int rc = (n % 3 != 0) ? edit(SE_DEPLOY_DECOY, h, K_DEC_VSFTPD, 0) : edit(SE_ADD_SERVICE, h, K_OT, n % 2);
      CHECK(rc >= 1 && (int)x.hd[h].nproc == n + 1, "host %d: add at %d gave %d", h, n, rc);
      if (rc < 0) break;
    }
  }
  bool has_kind(int h, int kind) { for (int i = 0; i < (int)x.hd[h].nproc; ++i) if (pw_kind(proc_get(x, h, i)) == kind) return true; return false; }
  int sshd_host(const std::vector<int>& z) { for (size_t i = z.size(); i-- > 0;) if (has_kind(z[i], K_SSHD)) return z[i]; return -1; }
  void ext_clear() { if (!has_ext) { memset(ext, 0xFF, sizeof(ext)); has_ext = true; } }
  // a submitted exploit of agent r that succeeds whatever the draws: its last abstract session knows port 22 of a host that runs sshd, and nothing else
  int ssh_exploit(int r, int tgt = -1) {
    RedAgent& A = s()->red[r];
    int idx = -1;
    for (int i = 0; i < A.h.nsess; ++i) if (rsw_flags(rs_at(s(), A, i)) & RS_ABSTRACT) idx = i;
    if (tgt < 0) tgt = sshd_host(zone(RED_SUB[r]));
    CHECK(idx >= 0 && tgt >= 0, "agent %d has no abstract session or its zone no sshd", r);
    if (idx < 0 || tgt < 0) return -1;
    x.c->kports[A.sord[idx]][tgt] = (uint8_t)(PB_HAS | PB_22);
    ext_clear();
    ExtAct& a = ext[r];
    memset(&a, 0, sizeof(a));
    a.type = RA_EXPLOIT; a.host = (uint8_t)tgt; a.sid = (uint16_t)rsw_id(rs_at(s(), A, idx)); a.ticks = 1; a.flags = XF_SKIP_VALID;
    return tgt;
  }
  int phish(int only = -1) {   // GreenLocalWork with phishing_error_rate 1 of a green agent on a host without red sessions
    for (int g = 0; g < s()->n_green; ++g) {
      const int h = s()->green_host[g];
      if (bit_get(s()->red_hosts, h) || (only >= 0 && h != only)) continue;
      ext_clear();
      ExtAct& a = ext[NRED + g];
      memset(&a, 0, sizeof(a));
      a.type = XG_LOCAL; a.host = (uint8_t)h; a.flags = XF_RATE1 | XF_SKIP_VALID; a.rate1 = 1.0;
      return h;
    }
    CHECK(false, "no green host without red sessions");
    return -1;
  }
  void poke_sus(int b, int count) {
    std::vector<int> z = zone(BLUE_SUB[b]);
    for (int k = 0; k < count; ++k) {
      const int h = z[(size_t)k % z.size()];
      cold_sus(x.c, steps, b)[k] = ((uint32_t)h << 16) | (uint32_t)(60001 + k);
      bit_set(s()->blue[b].sus_hosts, h);
    }
    s()->blue[b].nsus = (uint16_t)count;
  }
  void poke_pend(int count, bool defended) {
    std::vector<int> z = zone(defended ? BLUE_SUB[0] : RED_SUB[0]);
    for (int k = 0; k < count; ++k) s()->pend[k] = ((uint32_t)z[(size_t)k % z.size()] << 16) | (uint32_t)(61000 + k);
    s()->npend = (uint8_t)count;
  }
};

static void craft(Ep& p, int c, Variant v) {
  const int level = v == M1 ? -1 : 0, full = PIN + cold_povf_cap(p.steps);
  const bool op = v != CAP;
  EnvState* s = p.s();
  p.container = c; p.v = v;
  if (c == RS_ADD || c == RS_EXPLOIT || c == RS_REASSIGN) {
    p.flag = E_RSESS_OVERFLOW;
    std::vector<int> z = p.zone(RED_SUB[1]);
    p.fill_agent(1, MAX_RS + level);
    if (op && c == RS_REASSIGN) p.edit(SE_ADD_RED_SESSION, 0, z[2], 1);
    else if (op && c == RS_ADD) p.edits.push_back({SE_ADD_RED_SESSION, 1, z[1], 1 | 4, v == M1 ? MAX_RS - 1 : -1});
    else if (op) p.ssh_exploit(1);
  } else if (c >= POOL0 && c <= POOL3) {
    p.flag = E_RSESS_OVERFLOW;
    const int k = c - POOL0;
    p.fill_pool(k + (v == M1 ? 1 : 0));
    for (int r = 0; r < k + (op ? 1 : 0); ++r) p.ssh_exploit(r + 1);
  } else if (c == POOL_PHISH) {
    p.flag = E_RSESS_OVERFLOW;
    const int gh = s->green_host[0];
    p.fill_pool(v == M1 ? 1 : 0, gh);
    if (op) p.phish(gh);
  } else if (c == KNOWN || c == KNOWN256) {
    p.flag = E_KS_OVERFLOW;
    const int r = 2;
    RedAgent& A = s->red[r];
    std::vector<int> z = p.zone(RED_SUB[r]);
    p.fill_agent(r, 5);
    if (c == KNOWN256) s->spool[A.sord[4]].id = 300;
    const int n = MAX_KS + level;
    for (int k = 0; k < n; ++k) {
      const int id = (c == KNOWN256 && k == n - 1) ? 300 : k;
      p.x.c->known_sid[r][k] = (uint16_t)id;
      if (id < 256) bit_set(A.known_bm, id);
    }
    A.h.nknown = (uint8_t)n;
    if (op) {
      if (c == KNOWN) { for (int i = 0; i < 3; ++i) p.edit(SE_ADD_RED_SESSION, r, z[0], 0); s->spool[A.sord[A.h.nsess - 1]].id = 200; }
      const int rc = p.edit(SE_ADD_RED_SESSION, r, z[1], 1 | 4);
      CHECK(rc == (c == KNOWN ? 201 : 301), "ident %d", rc);
    }
  } else if (c == PROC_PIN) {
    for (int sn = 0; sn < 4; ++sn) { const int subs[3] = {sn, -1, -1}; for (int h : p.zone(subs)) p.fill_host(h, PIN + (v == M1 ? -1 : (v == CAP ? 0 : 1))); }
  } else if (c == PROC_EDIT) {
    p.flag = E_PROC_OVERFLOW;
    int top = 0;
    for (int h = 0; h < H_INTERNET; ++h) if (bit_get(s->exists, h)) top = h;
    const int hs[2] = {top, H_INTERNET};
    for (int h : hs) { p.fill_host(h, full + level); if (op) p.edits.push_back({SE_DEPLOY_DECOY, h, K_DEC_VSFTPD, 0, v == M1 ? 1 : -1}); }
  } else if (c == PROC_DECOY) {
    p.flag = E_PROC_OVERFLOW;
    for (int b = 0; b < NBLUE; ++b) p.blue[b] = -1;
    p.has_blue = true;
    for (int b = 0; b < NBLUE; b += 4) {
      const int h = p.zone(BLUE_SUB[b]).back();
      p.fill_host(h, full + level);
      if (op) p.blue[b] = BLUE_RAW_ACTION | (BA_DECOY << 8) | h | (1 << BLUE_DUR_SHIFT);
    }
  } else if (c == PROC_EXPLOIT) {
    p.flag = E_PROC_OVERFLOW;
    p.fill_agent(3, 6);
    const int tgt = p.sshd_host(p.zone(RED_SUB[3]));
    p.fill_host(tgt, full + level);
    if (op) p.ssh_exploit(3, tgt);
  } else if (c == PROC_PHISH) {
    p.flag = E_PROC_OVERFLOW;
    p.fill_agent(0, 3);
    int h = -1;
    for (int g = 0; g < s->n_green; ++g) if (!bit_get(s->red_hosts, s->green_host[g]) && s->green_host[g] > h) h = s->green_host[g];
    p.fill_host(h, full + level);
    if (op) p.phish(h);
  } else if (c >= SUS0_END && c <= SUS4_MON) {
    p.flag = E_SUS_OVERFLOW;
    const int b = (c == SUS0_END || c == SUS0_MON) ? 0 : 4;
    p.poke_sus(b, cold_sus_cap(p.steps) + level);
    if (op) {
      s->pend[0] = ((uint32_t)p.zone(BLUE_SUB[b])[1] << 16) | 60000u; s->npend = 1;
      if (c == SUS0_MON || c == SUS4_MON) { for (int k = 0; k < NBLUE; ++k) p.blue[k] = -1; p.has_blue = true; p.blue[b] = BLUE_RAW_ACTION | (BA_MONITOR << 8); }
    }
  } else if (c == PEND) {
    p.flag = E_PEND_OVERFLOW;
    if (op) p.fill_agent(1, 4);
    p.poke_pend(MAX_PEND + level, false);
    if (op) p.ssh_exploit(1);
  }
}

int main() {
  const int steps = 60, per_mode = N_CONTAINERS * N_VARIANTS, n = 2 * per_mode;   // crafted on the even rows and the last one
  const size_t cold_row = cold_row_bytes(steps);
  long raised[7] = {0, 0, 0, 0, 0, 0, 0}, stepped = 0;
  for (int mode = 0; mode < 2; ++mode) {
    EnvState* hot = (EnvState*)aligned_alloc(64, sizeof(EnvState) * (size_t)n);
    unsigned char* cold = (unsigned char*)malloc(cold_row * (size_t)n);
    if (!hot || !cold) { fprintf(stderr, "out of memory\n"); return 2; }
    memset(hot, 0, sizeof(EnvState) * (size_t)n); memset(cold, 0, cold_row * (size_t)n);
    std::vector<Ep> eps((size_t)per_mode);
    auto row_of = [&](int i) { return i == per_mode - 1 ? n - 1 : 2 * i; };
    uint32_t ws[RESET_WS_WORDS];
    for (int i = 0; i < per_mode; ++i) {
      Ep& p = eps[(size_t)i];
      const int e = row_of(i);
      p.steps = steps;
      p.x = Ctx{&hot[e], cold_at(reinterpret_cast<EnvCold*>(cold), (size_t)e, cold_row), &hot[e].rng, hot[e].hd, &p.w};
      memset(&p.w, 0, sizeof(p.w));
      env_reset(p.x, 1030 + (uint64_t)i, mode, steps, false, 0, 0, mode == 1 ? ws : nullptr);
      craft(p, i / N_VARIANTS, (Variant)(i % N_VARIANTS));
      CHECK(hot[e].err == 0, "mode %d variant %d: err %u after the fill", mode, i, (unsigned)hot[e].err);
      for (const Ep::Edit& ed : p.edits) { const int rc = p.edit(ed.op, ed.a0, ed.a1, ed.a2); CHECK(rc == ed.want, "mode %d variant %d: edit gave %d, not %d", mode, i, rc, ed.want); }
    }
    for (int t = 0; t < 2 * steps; ++t)
      for (int i = 0; i < per_mode; ++i) {
        Ep& p = eps[(size_t)i];
        EnvState* s = p.s();
        memset(&p.w, 0, sizeof(p.w));
        if (s->done) { env_reset(p.x, 0, mode, steps, true, 0, 0, mode == 1 ? ws : nullptr); continue; }
        int32_t act[NBLUE];
        for (int b = 0; b < NBLUE; ++b) act[b] = t == 0 ? (p.has_blue ? p.blue[b] : -1) : (int32_t)(rnd() % (uint64_t)(b == 4 ? ACT_LONG : ACT_SHORT));
        static ExtAct none[EXT_PER_ENV]; static bool init = false;
        if (!init) { memset(none, 0xFF, sizeof(none)); init = true; }
        p.x.ext = (t == 0 && p.has_ext) ? p.ext : none;
        const uint32_t before = s->err;
        env_step(p.x, act, nullptr);
        ++stepped;
        for (int f = 0; f < 7; ++f) if ((s->err & ~before) >> f & 1u) raised[f]++;
        // (what else the first step raises is not asserted here: a phishing e-mail of the default green agents may land in a crafted container;
        // tests/test_capacity_cpu.py chooses its seed so that none does and asserts the whole word)
        if (t == 0 && p.v == OVER && p.flag) CHECK((s->err & p.flag) != 0, "mode %d container %d: flag %u not raised (err %u)", mode, p.container, (unsigned)p.flag, (unsigned)s->err);
      }
    for (int e = 1; e < n - 1; e += (e == n - 3 ? 1 : 2)) {
      bool clean = true;
      const unsigned char* a = reinterpret_cast<const unsigned char*>(&hot[e]);
      for (size_t k = 0; k < sizeof(EnvState) && clean; ++k) clean = a[k] == 0;
      const unsigned char* b = cold + cold_row * (size_t)e;
      for (size_t k = 0; k < cold_row && clean; ++k) clean = b[k] == 0;
      CHECK(clean, "mode %d: the rows of episode %d, never generated, were written", mode, e);
    }
    free(cold); free(hot);
  }
  CHECK(raised[0] && raised[1] && raised[2] && raised[4] && raised[6], "a flag was never raised: %ld %ld %ld %ld %ld", raised[0], raised[1], raised[2], raised[4], raised[6]);
  printf("capacity_check: %ld steps, E_PROC %ld E_RSESS %ld E_KS %ld E_SUS %ld E_OBS %ld E_PEND %ld raised, %ld checks, %ld failures\n", stepped, raised[0], raised[1],
         raised[2], raised[4], raised[5], raised[6], checks, fails);
  return fails ? 1 : 0;
}
