// cc4_api_debug.hip -- the host side of libcc4.so: the debug and measurement hooks (include/cc4_debug.h) and the two debug reports of cc4_run_random_steps.
// (The functions of the C ABI take their linkage from their declarations in include/cc4.h and include/cc4_debug.h.)
#include "cc4_host.h"

// debug (CC4_PERSIST_TIMELINE): where a persistent call's time goes between the kernel's entry and its last item (ticks of the 100 MHz wall clock); frees
// the call's time stamps.  timed: the call carried the timing events evs[0], evs[1].
int timeline_report(cc4_handle* h, int k, bool timed) {
  std::vector<unsigned long long> tl(4 * (size_t)h->run_grid);
  HIPCHK(h, hipMemcpy(tl.data(), h->d_timeline, tl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  release(h, &h->d_timeline);
#ifdef CC4_BOUNDARY_PROF
  // the measurement build's words of a k_run_philox1 launch (bit 63 of word 0; persist_loop's tl_flush): the hand-over between two items of a wave in four parts
  { double sA = 0, sB = 0, sC = 0, sD = 0, sn = 0, items = 0, busy_ticks = 0; int nw = 0; std::vector<double> per;
    bool head = false;
    for (int w = 0; w < h->run_grid; ++w) { const unsigned long long* t = &tl[4 * (size_t)w]; if (!(t[0] >> 63)) continue; head = true;
      const double n = (double)((t[0] >> 32) & 0x7FFFFFFFull); if (n <= 0) continue; ++nw;
      const double A = (double)(uint32_t)t[1], B = (double)(t[1] >> 32), C = (double)(uint32_t)t[2], D = (double)(t[2] >> 32);
      sA += A; sB += B; sC += C; sD += D; sn += n; items += (double)(uint32_t)t[3]; busy_ticks += (double)(uint32_t)t[0]; per.push_back((A + B + C + D) / n / 100.0); }
    if (head) {
      float ms = 0.f; if (timed) (void)hipEventElapsedTime(&ms, h->evs[0], h->evs[1]);
      std::sort(per.begin(), per.end());
      const size_t m = per.size();
      const RunSplit rs = h->last_runs;
      if (m) fprintf(stderr, "[cc4 boundary] k=%d runs SA=%d nA=%d SB=%d nB=%d nph=%d: %d waves with a boundary, %.0f boundaries (%.0f items); per boundary, mean us: stage-out drain + publish %.3f, pick %.3f, "
                      "progress wait + acquire %.3f, stage-in %.3f, all %.3f; per wave all: min %.3f / median %.3f / 90%% %.3f / max %.3f us; boundaries are %.2f %% of the waves' busy time "
                      "(first item's start to last item's end, mean %.1f us); kernel (events) %.1f us\n", k, rs.SA, rs.nA, rs.SB, rs.nB, rs.nph, nw, sn, items,
                      sA / sn / 100.0, sB / sn / 100.0, sC / sn / 100.0, sD / sn / 100.0, (sA + sB + sC + sD) / sn / 100.0, per[0], per[m / 2], per[m * 9 / 10], per[m - 1],
                      100.0 * (sA + sB + sC + sD) / busy_ticks, busy_ticks / nw / 100.0, ms * 1000.0);
      return 0;
    }
  }
#endif
  unsigned long long e0 = ~0ull, e1 = 0, f1 = 0, l0 = ~0ull, l1 = 0; double fs = 0, ls = 0, items = 0; int nw = 0, idle = 0;
  for (int w = 0; w < h->run_grid; ++w) { const unsigned long long* t = &tl[4 * (size_t)w]; if (!t[0]) continue; ++nw; e0 = t[0] < e0 ? t[0] : e0; e1 = t[0] > e1 ? t[0] : e1; if (!(uint32_t)t[3]) { ++idle; continue; } f1 = t[1] > f1 ? t[1] : f1; l0 = t[2] < l0 ? t[2] : l0; l1 = t[2] > l1 ? t[2] : l1; fs += (double)t[1]; ls += (double)t[2]; items += (double)(uint32_t)t[3]; }
  const int busy = nw - idle;
  float ms = 0.f; if (timed) (void)hipEventElapsedTime(&ms, h->evs[0], h->evs[1]);
  fprintf(stderr, "[cc4 timeline] k=%d: %d waves reported (%d without an item); entry spread %.1f us; first item starts: mean +%.1f us, last +%.1f us after the first entry; "
                  "last item ends: earliest +%.1f us, mean +%.1f us, latest +%.1f us; items per busy wave %.1f; kernel (events) %.1f us\n",
          k, nw, idle, (e1 - e0) / 100.0, busy ? (fs / busy - (double)e0) / 100.0 : 0.0, (f1 - e0) / 100.0, (l0 - e0) / 100.0, busy ? (ls / busy - (double)e0) / 100.0 : 0.0, (l1 - e0) / 100.0, busy ? items / busy : 0.0, ms * 1000.0);
  // per CU: when its LAST wave ran dry, and how many items its waves executed (more than its own partition's = it helped out)
  { std::map<int, std::pair<unsigned long long, double>> cu;
    for (int w = 0; w < h->run_grid; ++w) { const unsigned long long* t = &tl[4 * (size_t)w]; if (!t[0] || !(uint32_t)t[3]) continue; auto& c = cu[(int)((t[3] >> 32) - 1)]; if (t[2] > c.first) c.first = t[2]; c.second += (double)(uint32_t)t[3]; }
    std::vector<double> last, its; for (auto& kv : cu) { last.push_back((kv.second.first - e0) / 100.0); its.push_back(kv.second.second); }
    std::sort(last.begin(), last.end()); std::sort(its.begin(), its.end());
    if (!last.empty()) { const size_t m = last.size(); fprintf(stderr, "[cc4 timeline]   per CU (%zu): last wave dry at min %.1f / 10%% %.1f / median %.1f / 90%% %.1f / max %.1f us; items executed min %.0f / median %.0f / max %.0f\n", m,
                               last[0], last[m / 10], last[m / 2], last[m * 9 / 10], last[m - 1], its[0], its[m / 2], its[m - 1]); } }
  // per XCD: when its waves ran dry (intra-XCD sharing evens a tail out inside an XCD; what is left between XCDs is not shareable)
  { double xs[8] = {0}, xi[8] = {0}; unsigned long long xl[8] = {0}, xf[8]; int xn[8] = {0}; for (int i = 0; i < 8; ++i) xf[i] = ~0ull;
    for (int w = 0; w < h->run_grid; ++w) { const unsigned long long* t = &tl[4 * (size_t)w]; if (!t[0] || !(uint32_t)t[3]) continue; const int xc = (int)(((t[3] >> 32) - 1) >> 8) & 7;
      xs[xc] += (double)t[2]; xi[xc] += (double)(uint32_t)t[3]; ++xn[xc]; if (t[2] > xl[xc]) xl[xc] = t[2]; if (t[2] < xf[xc]) xf[xc] = t[2]; }
    for (int i = 0; i < 8; ++i) if (xn[i]) fprintf(stderr, "[cc4 timeline]   XCD %d: %d busy waves, %.0f items; waves ran dry: earliest +%.1f, mean +%.1f, latest +%.1f us\n", i, xn[i], xi[i],
                                                  (xf[i] - e0) / 100.0, (xs[i] / xn[i] - (double)e0) / 100.0, (xl[i] - e0) / 100.0); }
  return 0;
}
// debug (CC4_EXCHANGE_PROF): where the host's time goes around a one-launch call with the exchange; t = before xchg_begin, before the launch, before
// xchg_enqueue, before and after the wait for the kernel, after xchg_end
void exchange_prof_report(int k, const std::chrono::steady_clock::time_point (&t)[6]) {
  static double xp[6] = {0}; static long xpn = 0;
  auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
  xp[0] += us(t[0], t[1]); xp[1] += us(t[1], t[2]); xp[2] += us(t[2], t[3]); xp[3] += us(t[3], t[4]); xp[4] += us(t[4], t[5]); xp[5] += us(t[0], t[5]);
  if (++xpn % 200 == 0) {
    fprintf(stderr, "[cc4 exchange prof] k=%d, mean of 200 calls (us): begin %.1f, launch %.1f, enqueue of the chunks %.1f, wait for the kernel %.1f, then for the communication stream %.1f; call %.1f\n",
            k, xp[0] / 200, xp[1] / 200, xp[2] / 200, xp[3] / 200, xp[4] / 200, xp[5] / 200);
    for (double& v : xp) v = 0;
  }
}
// debug: where a rollout stands / stood -- out[0..1] gate-failed flag and the kernel's timeout flag, out[2 + g] the groups' published step counts,
// out[6 + 4 * slot + g] = sum over the partitions of the count of (policy group g, ring slot), slots 0..3
int cc4_debug_rollout_state(cc4_handle* h, int64_t* out /* [22] */) {
  if (!h->d_rcnt) { h->err = "cc4_debug_rollout_state: no rollout was begun on this handle"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  std::vector<uint32_t> rd(32), cnt((size_t)h->run_P * RPG_MAX * cc4_handle::XRING);
  uint32_t fail = 0;
  HIPCHK(h, hipMemcpy(rd.data(), h->d_rready, rd.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(cnt.data(), h->d_rcnt, cnt.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(h, hipMemcpy(&fail, h->d_rfail, 4, hipMemcpyDeviceToHost));
  out[0] = fail; out[1] = *reinterpret_cast<volatile uint32_t*>(h->h_xtimeout);
  for (int g = 0; g < h->rpg; ++g) out[2 + g] = rd[g];
  for (int slot = 0; slot < 4; ++slot) for (int g = 0; g < h->rpg; ++g) {
    int64_t sum = 0;
    for (int p = 0; p < h->run_P; ++p) sum += cnt[((size_t)p * h->rpg + g) * cc4_handle::XRING + slot];
    out[6 + 4 * slot + g] = sum;
  }
  return 0;
}

// debug: enable (buf != NULL first call allocates) / read per-episode cycle counters [N][64] (16 phase slots, then 8 per red agent)
int cc4_debug_profile(cc4_handle* h, int enable, unsigned long long* out) {
  if (int rc = enter(h, "cc4_debug_profile")) return rc;
  size_t bytes = (size_t)h->cfg.num_envs * PROF_SLOTS * sizeof(unsigned long long);
  if (enable && !h->d_prof) { if (dev_alloc(h, &h->d_prof, bytes)) return -1; HIPCHK(h, hipMemsetAsync(h->d_prof, 0, bytes, h->stream)); }
  if (out && h->d_prof) { HIPCHK(h, hipMemcpyAsync(out, h->d_prof, bytes, hipMemcpyDeviceToHost, h->stream)); HIPCHK(h, hipStreamSynchronize(h->stream)); }
  if (!enable) release(h, &h->d_prof);
  return 0;
}

// measurement (tools/valu_phases.py): from now on the per-step launches of k_step_philox1 (its full build) end behind phase `phase` of the step (1..13,
// csrc/cc4_philox1_body.h CC4_STOP) and write no row back; 14 = whole steps of the full build; 0 = whole steps of the usual build again.  The caller restores the batch (cc4_set_state / cc4_set_cold) after such a step.
int cc4_debug_stop_phase(cc4_handle* h, int phase) {
  if (join_groups(h)) return -1;
  if (phase < 0 || phase > 14 || !h->philox_lean) { h->err = "cc4_debug_stop_phase: phase 0..14, on a handle whose step kernel is k_step_philox1"; return -2; }
  h->dbg_stop = phase;
  return 0;
}

// test hook: the persistent schedule's progress words as if `base` steps had run since they were last cleared (every episode's word = base, no
// runner; pool_base = base) -- the wrap of persist_launch within a few steps' reach
int cc4_debug_persist_base(cc4_handle* h, uint32_t base) {
  if (h->rollout_k > 0) { h->err = "cc4_debug_persist_base: a rollout is in flight on this handle"; return -2; }      // (its own, shorter sentence)
  if (base > PROGRESS_CLEAR_AT) { char msg[64]; snprintf(msg, sizeof msg, "cc4_debug_persist_base: base 0 .. %#x", PROGRESS_CLEAR_AT); h->err = msg; return -2; }
  if (int rc = enter(h, "cc4_debug_persist_base")) return rc;
  if (h->persist_state == 0) { if (persist_setup(h)) return -1; }
  if (h->persist_state != 1) { h->err = "cc4_debug_persist_base: this handle has no persistent kernel"; return -2; }
  HIPCHK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(h->d_run), (int)base, (size_t)h->cfg.num_envs, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->pool_base = base;
  return 0;
}
int cc4_debug_copy_from_device(cc4_handle* h, void* host_dst, const void* device_src, size_t bytes) {
  if (int rc = enter(h, "cc4_debug_copy_from_device")) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int g = 0; g < 4; ++g) if (h->gpolicy[g]) HIPCHK(h, hipStreamSynchronize(h->gpolicy[g]));
  HIPCHK(h, hipMemcpy(host_dst, device_src, bytes, hipMemcpyDeviceToHost));
  return 0;
}
// test hook: the self-check's shadow handle, NULL where the handle has none (tests/handover_util.py reads the shadow's side of a checked call through it)
int cc4_debug_shadow_handle(cc4_handle* h, cc4_handle** out) {
  if (!h || !out) return -2;
  *out = h->shadow;
  return 0;
}
// the self-check's digest of one episode on the host (csrc/cc4_digest.h: the definition k_digest runs, its 64 lanes in a loop); needs no device and no handle
int cc4_debug_digest_rows(const void* hot_row, const void* cold_row, size_t cold_bytes, const int32_t* obs, float reward, uint8_t done, uint32_t err,
                          const int32_t* actions, uint64_t out[3]) {
  if (!hot_row || !cold_row || !obs || !actions || !out || cold_bytes % 16) return -2;
  uint32_t reward_bits;
  __builtin_memcpy(&reward_bits, &reward, 4);
  out[0] = digest_row_word(hot_row, sizeof(EnvState) / 16);
  out[1] = digest_row_word(cold_row, cold_bytes / 16);
  out[2] = digest_out_word(obs, actions, reward_bits, done, err);
  return 0;
}
// test hook, read-only: k_digest over this handle's episodes as they stand (what a checked call computes of either side)
int cc4_debug_digest(cc4_handle* h, uint64_t* out /* [N][3] */) {
  if (!h || !out) return -2;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  std::vector<uint64_t> d;
  if (verify_digest(h, d)) return -1;
  memcpy(out, d.data(), d.size() * sizeof(uint64_t));
  return 0;
}
// test hook: arm (part -1: disarm) the one planted difference of the next checked call (cc4_api_run.hip plant_apply: a byte of the shadow's side, data only)
int cc4_debug_verify_plant(cc4_handle* h, int32_t part, int32_t env, int64_t offset, int32_t step) {
  if (!h) return -2;
  h->plant.part = -1;
  if (part == -1) return 0;
  const char* who = "cc4_debug_verify_plant";
  if (h->is_shadow || h->comm) { h->err = std::string(who) + ": not on a shadow handle or a handle with a communicator (its calls are never checked)"; return -2; }
  if (!h->verify && h->verify_every <= 0) { h->err = std::string(who) + ": no call of this handle is ever checked (CC4_PERSIST_VERIFY unset, CC4_PERSIST_VERIFY_EVERY=0)"; return -2; }
  static const int64_t span[10] = {(int64_t)sizeof(EnvState), 0 /* the cold row */, OBS_TOTAL, 1, 1, 1, NBLUE, 1, 1, OBS_PACKED};
  const bool traj = part >= 7 && part <= 9;
  if (part < 0 || part > 9 || env < 0 || env >= h->cfg.num_envs || offset < 0 || offset >= (part == 1 ? (int64_t)h->cold_row : span[part]) || step < 0 || (!traj && step != 0)) {
    h->err = std::string(who) + ": part 0..9 (-1 disarms), env 0..N-1, offset inside the part (0 where it has none), step >= 0 (0 unless part 7..9)"; return -2;
  }
  h->plant.part = part; h->plant.env = env; h->plant.offset = offset; h->plant.step = step;
  return 0;
}
// test hook, read-only: the builds launch_range and run_one_launch pick on this handle (the one-wave step kernel or the four-wave one, the four-wave
// kernel's register budget, the multi-step build) -- cc4_step_kernel has one name for k_step_philox<., 1 / 7 / 8>
int cc4_debug_step_build(cc4_handle* h, int32_t out[3]) {
  if (!h || !out) return -2;
  out[0] = h->philox_lean ? 1 : 0; out[1] = h->philox_minw; out[2] = h->multistep_minb;
  return 0;
}
int cc4_debug_last_run_split(cc4_handle* h, int32_t out[5]) {
  if (!h || !out) return -2;
  const RunSplit& r = h->last_runs;
  out[0] = r.SA; out[1] = r.nA; out[2] = r.SB; out[3] = r.nB; out[4] = r.nph;
  return 0;
}
// debug / test hook: every all-gather is preceded by a kernel that keeps the communication stream busy for about `us`
// microseconds -- an exchange slower than the step, which is what makes the observation ring's reuse guard work for its living
int cc4_debug_comm_delay_us(cc4_handle* h, int us) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  h->comm_delay_ticks = (long long)us * wall_khz(h) / 1000;
  return 0;
}
