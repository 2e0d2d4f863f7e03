// cc4_api_run.hip -- the host side of libcc4.so, k steps per call: which one-launch form a handle takes (choose_run_form), the persistent kernel's
// set-up and launch, the enqueue threads, cc4_run_random_steps and its three schedules, the self-check of the one-launch forms, the plan calls.
// (The functions of the C ABI take their linkage from their declarations in include/cc4.h and include/cc4_debug.h.)
#include "cc4_host.h"

static void enq_run_group(cc4_handle* h, EnqPool* P, int g) {
  StepArgs a = P->a;
  for (int i = 0; i < P->k; ++i) {
    a.rand_t = P->t0 + (uint32_t)i;
    a.full_obs = (i == 0 && P->first_full_obs) ? 1 : 0;
    launch_group(h, a, g, P->full, i == 0 ? P->start[g] : nullptr, i == P->k - 1 ? P->stop[g] : nullptr);
  }
  if (g > 0 && hipEventRecord(h->gev[g], h->gstream[g]) != hipSuccess) P->failed.fetch_add(1);   // the main stream waits for it: one host wait per call
  if (hipGetLastError() != hipSuccess) P->failed.fetch_add(1);
}
static void enq_worker(cc4_handle* h, EnqPool* P, int g) {
  (void)hipSetDevice(h->cfg.device_id);
  uint64_t seen = 0;
  for (;;) {
    auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    while (P->gen.load(std::memory_order_acquire) == seen && !P->quit.load(std::memory_order_relaxed)) {
      __builtin_ia32_pause();
      if ((++spins & 255) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(P->spin_us)) {
        std::unique_lock<std::mutex> lk(P->mu);
        P->cv.wait(lk, [&] { return P->gen.load(std::memory_order_acquire) != seen || P->quit.load(); });
      }
    }
    if (P->quit.load()) return;
    seen = P->gen.load(std::memory_order_acquire);
    enq_run_group(h, P, g);
    P->pending.fetch_sub(1, std::memory_order_release);
  }
}
static void enq_pool_start(cc4_handle* h) {
  if (h->pool || h->ngroups < 2) return;
  h->pool = new EnqPool;
  if (const char* v = getenv("CC4_ENQ_SPIN_US")) h->pool->spin_us = atoi(v) > 0 ? atoi(v) : 0;
  for (int g = 1; g < h->ngroups; ++g) h->pool->th.emplace_back(enq_worker, h, h->pool, g);
}
void enq_pool_stop(cc4_handle* h) {
  if (!h->pool) return;
  { std::lock_guard<std::mutex> lk(h->pool->mu); h->pool->quit.store(true); }
  h->pool->cv.notify_all();
  for (auto& t : h->pool->th) t.join();
  delete h->pool; h->pool = nullptr;
}

// the persistent kernel of a handle's mode
static const void* persist_kernel(const cc4_handle* h) {
  if (h->cfg.rng_mode == 0) return reinterpret_cast<const void*>(k_run_pcg);
  return h->comm ? reinterpret_cast<const void*>(k_run_philox1x) : reinterpret_cast<const void*>(k_run_philox1);
}


// Which form cc4_run_random_steps takes on this handle (decided at cc4_create, again at cc4_comm_init): the multi-step form of the four-wave
// kernel (k_run_philox / k_run_philox8) for batches the chip holds at once, the plain multi-step form of the one-wave kernel (k_run_philox1m)
// up to 20 episodes per CU, the persistent kernel beyond.  `margin` = episode blocks per CU the multi-step kernels leave free,
// `persist_margin` = waves per CU the persistent kernel's grid leaves free (see cc4_comm_init).
int choose_run_form(cc4_handle* h, int margin, int persist_margin) {
  const cc4_config* cfg = &h->cfg;
  if (persist_margin < 0) persist_margin = margin;
  h->multistep = false; h->run1m = false;
  if (cfg->rng_mode == 1 && !h->philox_lean) {
    // the multi-step form of the four-wave kernel (k_run_philox): for batches the chip holds at once
    int per_cu = 0, per_cu8 = 0;
    HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_run_philox, PT, sizeof(EnvState)));
    HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu8, k_run_philox8, PT, sizeof(EnvState)));
    h->multistep = per_cu - margin > 0 && cfg->num_envs <= (per_cu - margin) * h->cus;
    h->multistep_minb = 5;
    if (!h->multistep && per_cu8 > per_cu && cfg->num_envs <= (per_cu8 - margin) * h->cus) { h->multistep = true; h->multistep_minb = 8; }
    if (const char* v = getenv("CC4_MULTISTEP")) {            // 0: off; 1: on (the build that holds the batch); 5 / 8: that build
      const int m = atoi(v);
      h->multistep = m != 0;
      if (m == 5 || m == 8) h->multistep_minb = m;
    }
    if (getenv("CC4_PERSIST_DEBUG")) fprintf(stderr, "[cc4] k_run_philox: %d / %d blocks per CU resident (margin %d), multistep %d (build %d)\n", per_cu, per_cu8, margin, (int)h->multistep, h->multistep_minb);
  }
  if (cfg->rng_mode == 1 && !h->multistep) {
    // (whichever per-step kernel the handle runs: a batch of 2049-5120 episodes that cc4_step serves with the four-wave kernel is served here by the one-wave loop)
    // the plain multi-step form of the one-wave kernel (k_run_philox1m) where one launch holds the whole batch: 20 waves per CU
    // (4096 episodes 507 -> 709 M, 5120: 586 -> 811 M; beyond the residency the second round runs on a half-empty chip and four
    // streams of per-step launches win: 8192: 740 vs 789 M, 16384: 812 vs 864 M -- profiles/r04_run1m_ab.txt)
    int per_cu = 0;
    HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_run_philox1m, WAVE, offsetof(EnvState, hd)));
    h->run1m = per_cu - margin > 0 && cfg->num_envs <= (per_cu - margin) * h->cus;
    if (const char* v = getenv("CC4_RUN1")) h->run1m = atoi(v) != 0;
  }
  // one enqueue thread per group stream in cc4_run_random_steps (EnqPool): on where the host has cores to spare; CC4_ENQ_THREADS=0/1 decides otherwise
  h->enq_threads = std::thread::hardware_concurrency() >= 8;
  if (const char* v = getenv("CC4_ENQ_THREADS")) h->enq_threads = atoi(v) != 0;
  // the persistent run kernel of large batches (k_run_philox1): set up on first use (persist_setup); CC4_PERSIST=0 keeps it off
  h->persist_state = -1;
  h->run_margin = persist_margin;
  bool persist_mode = cfg->rng_mode == 1 && !h->multistep && !h->run1m;
  persist_mode = persist_mode || cfg->rng_mode == 0;
  if (persist_mode) {
    int per_cu = 0;
    HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, persist_kernel(h), WAVE, offsetof(EnvState, hd)));
    const int grid = (per_cu - persist_margin) * h->cus;
    // batches of more than the chip holds at once (with the tail shared, also just more).  The numpy-stream mode has no other one-launch form: there
    // the persistent kernel also serves batches from half the residency up (a partition of fewer episodes than the CU has waves just leaves waves idle)
    // (counter mode: what neither multi-step kernel holds -- 5121 .. 6144 episodes at 20 / 24 waves per CU -- is the persistent kernel's as well)
    if (per_cu - persist_margin > 0 && (cfg->num_envs > grid || 2 * cfg->num_envs > grid)) h->persist_state = 0;
  }
  if (const char* v = getenv("CC4_PERSIST")) { if (atoi(v) == 0) h->persist_state = -1; }
  return 0;
}
// The persistent run kernel (cc4_run_random_steps without a communicator, batches beyond what one launch holds): one wave per
// residency slot, the batch cut into one partition per CU.  Which CUs the device has is found once per handle (k_discover: many small
// waves reporting HW_REG_XCC_ID / HW_REG_HW_ID; the path stays off unless exactly as many CUs show up as the device properties
// promise -- a mis-decoded id would merge CUs and show here); how many waves of the run kernel a CU takes is the dispatcher's business.
// History: r04 built it with the step body as a call and measured it 18-38 % slower than four streams of per-step launches; the call
// was the brake (a kernel that contains one loses a quarter of its rate).  Inlined (lane id opaque per item) and compiled without
// machine LICM (which hoisted ~200 registers' worth of loop-invariant values across the item loop and spilled them) it is the faster
// schedule from ~20 steps per call on: 8192 episodes 795 -> 917 M at K = 500 (profiles/r04_persistent_kernel_ab.txt).
int persist_setup(cc4_handle* h) {
  h->persist_state = -1;
  const size_t n = (size_t)h->cfg.num_envs;
  int per_cu = 0;
  HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, persist_kernel(h), WAVE, offsetof(EnvState, hd)));
  // (the occupancy query divides 160 KB by the kernel's LDS bytes; the hardware allocates 1280-byte granules -- profiles/r05_lds_residency.txt)
  hipFuncAttributes fa{};
  HIPCHK(h, hipFuncGetAttributes(&fa, persist_kernel(h)));
  const int granules = (int)((offsetof(EnvState, hd) + fa.sharedSizeBytes + 1279) / 1280);
  if (granules > 0 && 128 / granules < per_cu) per_cu = 128 / granules;
  per_cu -= h->run_margin;            // (with ranks to talk to: a slot per CU stays free for RCCL's kernels)
  if (per_cu <= 0) return 0;
  // The hand-over between two items of an episode relies on what gfx942 / gfx950 do in their default (non-tgsplit) mode: the waves of a
  // CU share one write-through vector L1 (validated on MI355X in SPX mode, the only partition mode of this pool).  Any other
  // architecture keeps the per-step launches -- and says so.
  hipDeviceProp_t prop;
  HIPCHK(h, hipGetDeviceProperties(&prop, h->cfg.device_id));
  if (!(strncmp(prop.gcnArchName, "gfx942", 6) == 0 || strncmp(prop.gcnArchName, "gfx950", 6) == 0)) {
    fprintf(stderr, "[cc4] the persistent run kernel stays OFF for this handle (per-step launches instead): architecture %s is neither gfx942 nor gfx950\n", prop.gcnArchName);
    h->persist_refused = true;
    return 0;
  }
  if (join_groups(h)) return -1;
  std::vector<int32_t> count(CC4_SLOTS);
  {
    DevTemp<int32_t> d_count;
    if (d_count.alloc(h, CC4_SLOTS * sizeof(int32_t))) return -1;
    HIPCHK(h, hipMemsetAsync(d_count.p, 0, CC4_SLOTS * sizeof(int32_t), h->stream));
    hipLaunchKernelGGL(k_discover, dim3(24 * h->cus), dim3(WAVE), 0, h->stream, d_count.p, 100LL * wall_khz(h) / 1000);   // ~100 us each
    HIPCHK(h, hipMemcpyAsync(count.data(), d_count.p, CC4_SLOTS * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  std::vector<int32_t> table(CC4_SLOTS, 0);
  int P = 0;
  for (int sl = 0; sl < CC4_SLOTS; ++sl) if (count[sl] > 0) table[sl] = ++P;        // 1 + partition, in slot order: an XCD's CUs own neighbouring partitions
  if (getenv("CC4_PERSIST_DEBUG")) fprintf(stderr, "[cc4] persistent kernel: %d compute units seen (device: %d), %d LDS granules per wave, %d waves per CU\n", P, h->cus, granules, per_cu);
  {
    // the partition mode the hand-over was validated in: SPX -- one device, all eight XCDs, every CU of each (MI355X: 8 x 32).  Another
    // picture (CPX / DPX / QPX partitions, a part with CUs fused off differently per XCD) may well work -- an XCD's L2 is still the
    // coherence point of its CUs -- but nobody has run the self-check there: CC4_PERSIST_ANY_PARTITION=1 takes the responsibility.
    int nx = 0, per_x[8] = {0};
    for (int sl = 0; sl < 8 << 8; ++sl) if (count[sl] > 0) ++per_x[sl >> 8];
    bool even = true;
    for (int xc = 0; xc < 8; ++xc) { if (per_x[xc]) ++nx; if (per_x[xc] && per_x[xc] != per_x[0]) even = false; }
    const bool spx = nx == 8 && even && per_x[0] > 0;
    if (!spx && !(getenv("CC4_PERSIST_ANY_PARTITION") && atoi(getenv("CC4_PERSIST_ANY_PARTITION")) != 0)) {
      fprintf(stderr, "[cc4] the persistent run kernel stays OFF for this handle (per-step launches instead): the device shows %d XCD(s) with %d..CUs each -- not the SPX "
                      "picture (8 XCDs, equal CU counts) the hand-over between waves was validated in; CC4_PERSIST_ANY_PARTITION=1 overrides\n", nx, per_x[0]);
      h->persist_refused = true;
      return 0;
    }
  }
  if (P != h->cus) {       // a CU id that does not tell CUs apart would put two CUs on one partition: never run on a guess
    fprintf(stderr, "[cc4] the persistent run kernel stays OFF for this handle (per-step launches instead): its discovery pass saw %d compute units, the device has %d\n", P, h->cus);
    h->persist_refused = true;
    return 0;
  }
  h->run_P = P; h->run_G = P; h->run_grid = per_cu * h->cus;
  if (const char* v = getenv("CC4_PERSIST_THR")) h->run_thr = atoi(v);
  if (const char* v = getenv("CC4_PERSIST_RUNS")) {
    int q[4] = {h->run_SA, h->run_SB, h->run_nB, h->run_single};
    (void)sscanf(v, "%d,%d,%d,%d", &q[0], &q[1], &q[2], &q[3]);
    h->run_SA = q[0] < 0 ? 0 : q[0]; h->run_SB = q[1] < 1 ? 1 : q[1]; h->run_nB = q[2] < 0 ? 0 : q[2]; h->run_single = q[3] < 0 ? 0 : q[3];
  }
  // the partitions of an XCD: a contiguous range (they are numbered in slot order, slot id = XCC id << 8 | CU)
  bool ok = true;
  for (int xc = 0; xc < 8; ++xc) {
    int lo = -1, cnt = 0;
    for (int sl = xc << 8; sl < (xc + 1) << 8; ++sl) if (table[sl] > 0) { if (lo < 0) lo = table[sl] - 1; ++cnt; }
    if (cnt > MAX_XCD_PARTITIONS || lo > MAX_XCD_FIRST) ok = false;          // (one lane per partition of the XCD; the range's start travels as a byte)
    h->xcc_lo[xc] = (uint8_t)(lo < 0 ? 0 : lo); h->xcc_n[xc] = (uint8_t)(cnt > MAX_XCD_PARTITIONS ? 0 : cnt);
  }
  for (int sl = 8 << 8; sl < CC4_SLOTS; ++sl) if (count[sl] > 0) ok = false;          // an XCC id beyond 7: not a device this schedule knows
  if (P > MAX_PARTITIONS) ok = false;                 // the runner's id in the progress words (runner_of, cc4_sched.h)
  if (!ok) {
    fprintf(stderr, "[cc4] the persistent run kernel stays OFF for this handle (per-step launches instead): more than %d CUs in an XCD, or more than %d CUs\n", MAX_XCD_PARTITIONS, MAX_PARTITIONS);
    h->persist_refused = true;
    return 0;
  }
  if (!h->d_pool && dev_alloc(h, &h->d_pool, 2 * (size_t)CC4_SLOTS * TK_STRIDE * sizeof(uint32_t))) return -1;
  HIPCHK(h, hipMemset(h->d_pool, 0, 2 * (size_t)CC4_SLOTS * TK_STRIDE * sizeof(uint32_t)));
  h->pool_base = 0; h->pool_parity = 0;
  if (!h->d_slot_part && dev_alloc(h, &h->d_slot_part, CC4_SLOTS * sizeof(int32_t))) return -1;
  HIPCHK(h, hipMemcpy(h->d_slot_part, table.data(), CC4_SLOTS * sizeof(int32_t), hipMemcpyHostToDevice));
  h->run_words = (size_t)n;                                                           // the progress words
  if (dev_alloc(h, &h->d_run, h->run_words * sizeof(uint32_t))) return -1;
  HIPCHK(h, hipMemset(h->d_run, 0, h->run_words * sizeof(uint32_t)));
  h->persist_state = 1;
  // the sampled self-check's shadow handle is created HERE, with the path itself (the first persistent call of a handle: normally a warm-up) -- a
  // cc4_create inside the 1024th call would cost that call ~45 ms; the checks themselves then cost ~6 calls' worth each (copies and digests of the
  // cold rows), i.e. ~0.6 % of a long run.  CC4_PERSIST_VERIFY_EVERY=0: no sampling, no second copy of the rows.
  if (!h->is_shadow && !h->comm && (h->verify || h->verify_every > 0)) { if (ensure_shadow(h)) return -1; }
  return 0;
}
static int run_random_steps_impl(cc4_handle* h, uint64_t seed0, uint32_t t0, int32_t k, float* ms_step_kernels);
// CC4_PERSIST_VERIFY=1 (a self-check mode, not a fast one): a call that takes a one-launch form -- the persistent kernels, whose hand-over
// between the steps of an episode leans on how a CU's L1 behaves, and the plain multi-step kernels -- is run a second time
// from the same starting rows with per-step launches on a shadow handle, and the two outcomes are compared episode by episode.
int verify_digest(cc4_handle* h, std::vector<uint64_t>& out) {
  const int n = h->cfg.num_envs;
  if (!h->d_digest && dev_alloc(h, &h->d_digest, 3 * (size_t)n * sizeof(uint64_t))) return -1;
  if (join_groups(h)) return -1;
  hipLaunchKernelGGL(k_digest, dim3(n), dim3(WAVE), 0, h->stream, h->d_state, h->d_cold, h->cold_row, h->d_obs, h->d_reward, h->d_done, h->d_err, h->d_actions, h->d_digest, n);
  HIPCHK(h, hipGetLastError());
  out.resize(3 * (size_t)n);
  HIPCHK(h, hipMemcpyAsync(out.data(), h->d_digest, out.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return 0;
}
// the shadow handle of the self-check: a second copy of the batch's rows, stepped with per-step launches only
int ensure_shadow(cc4_handle* h) {
  if (h->shadow) return 0;
  cc4_handle* sh = nullptr;
  if (cc4_create(&h->cfg, &sh) != 0) { h->err = std::string("CC4_PERSIST_VERIFY: the shadow handle could not be created: ") + cc4_last_error(sh); if (sh) cc4_destroy(sh); return -1; }
  sh->is_shadow = true; sh->verify = false; sh->verify_every = 0; sh->persist_state = -1; sh->multistep = false; sh->run1m = false;
  h->shadow = sh;
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  return 0;
}
// The mechanism of the self-check; WHEN a call is checked is its caller's business (cc4_run_random_steps, cc4_run_plan_device).
// shadow_seed: the shadow handle starts from a copy of this handle's rows and outputs, both handles' streams drained.
static int shadow_seed(cc4_handle* h) {
  if (ensure_shadow(h)) return -1;
  cc4_handle* sh = h->shadow;
  const size_t n = (size_t)h->cfg.num_envs;
  if (join_groups(h) || join_groups(sh)) return -1;
  HIPCHK(h, hipStreamSynchronize(sh->stream));
  HIPCHK(h, hipMemcpyAsync(sh->d_state, h->d_state, n * sizeof(EnvState), hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(sh->d_cold, h->d_cold, n * h->cold_row, hipMemcpyDeviceToDevice, h->stream));
  HIPCHK(h, hipMemcpyAsync(sh->d_obs, h->d_obs, h->out_bytes, hipMemcpyDefault, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));      // (behind whatever cc4_stream_wait ordered this handle after: a plan is complete for the shadow's stream too)
  sh->full_obs_next = h->full_obs_next; sh->main_ahead = sh->ngroups > 1;
  return 0;
}
// shadow_compare: both handles' episodes digested and compared; `what` = the first episode that differs, as text (empty: none does)
static int shadow_compare(cc4_handle* h, std::string& what) {
  std::vector<uint64_t> a, b;
  if (verify_digest(h, a)) return -1;
  if (verify_digest(h->shadow, b)) { h->err = "CC4_PERSIST_VERIFY: " + h->shadow->err; return -1; }
  h->verify_calls++;
  what.clear();
  for (size_t e = 0; e < (size_t)h->cfg.num_envs && what.empty(); ++e) {
    const int d = digest_differs(a.data(), b.data(), e);
    const bool hot = d & 1, cold = d & 2, outp = d & 4;
    if (d) what = "first episode " + std::to_string(e) + " (" + (hot ? "hot row " : "") + (cold ? "cold row " : "") + (outp ? "outputs" : "") + ")";
  }
  return 0;
}
// The planted difference of cc4_debug_verify_plant (include/cc4_debug.h), a test hook: data only -- one byte of the SHADOW's side XORed with 1 behind both
// sides' runs and in front of the digests and the trajectory compare, in memory that nothing steps before the next checked call re-seeds the shadow.
// plant_refuse: the armed plant does not fit the checked call it met (a trajectory part on a call that records no such row): nothing runs, nothing stays armed
static int plant_refuse(cc4_handle* h, const char* who) {
  h->plant.part = -1;
  h->err = std::string(who) + ": the difference armed with cc4_debug_verify_plant names a trajectory row this call does not record (disarmed; nothing was stepped)";
  return -2;
}
// s_rew / s_done / s_packed: the shadow's recorded trajectory of a plan call (NULL: not recorded, or no plan call)
static int plant_apply(cc4_handle* h, float* s_rew, uint8_t* s_done, uint8_t* s_packed) {
  const cc4_handle::VerifyPlant p = h->plant;
  if (p.part < 0) return 0;
  h->plant.part = -1;
  cc4_handle* sh = h->shadow;
  const size_t n = (size_t)h->cfg.num_envs, e = (size_t)p.env, off = (size_t)p.offset, row = (size_t)p.step * n + e;
  uint8_t* at = nullptr;
  switch (p.part) {
    case 0: at = reinterpret_cast<uint8_t*>(sh->d_state + e) + off; break;
    case 1: at = reinterpret_cast<uint8_t*>(cold_at(sh->d_cold, e, sh->cold_row)) + off; break;
    case 2: at = reinterpret_cast<uint8_t*>(sh->d_obs + e * OBS_TOTAL + off); break;
    case 3: at = reinterpret_cast<uint8_t*>(sh->d_reward + e); break;
    case 4: at = sh->d_done + e; break;
    case 5: at = reinterpret_cast<uint8_t*>(sh->d_err + e); break;
    case 6: at = reinterpret_cast<uint8_t*>(sh->d_actions + e * NBLUE + off); break;
    case 7: at = reinterpret_cast<uint8_t*>(s_rew + row); break;
    case 8: at = s_done + row; break;
    default: at = s_packed + row * OBS_PACKED + off; break;
  }
  if (join_groups(sh)) { h->err = "CC4_PERSIST_VERIFY: " + sh->err; return -1; }
  HIPCHK(h, hipStreamSynchronize(sh->stream));
  uint8_t byte = 0;
  HIPCHK(h, hipMemcpy(&byte, at, 1, hipMemcpyDefault));
  byte ^= 1;
  HIPCHK(h, hipMemcpy(at, &byte, 1, hipMemcpyDefault));
  return 0;
}
// a checked call disagreed with its shadow: counted, said on stderr, the call's return value
static int verify_mismatch(cc4_handle* h, const std::string& msg) {
  h->verify_mismatches++;
  h->err = "CC4_PERSIST_VERIFY: " + msg;
  fprintf(stderr, "[cc4] %s\n", h->err.c_str());
  return -5;
}
int cc4_run_random_steps(cc4_handle* h, uint64_t seed0, uint32_t t0, int32_t k, float* ms_step_kernels) {
  if (h->is_shadow || k < 2) return run_random_steps_impl(h, seed0, t0, k, ms_step_kernels);
  // The self-check: with CC4_PERSIST_VERIFY=1 every one-launch call is repeated on a shadow handle and compared; WITHOUT it every
  // verify_every-th call that takes the PERSISTENT form is (CC4_PERSIST_VERIFY_EVERY, default 1024, 0 = never; the communicator-less handles
  // only: a shadow handle cannot join the exchange) -- the hand-over between the waves of a CU rests on behaviour the memory model does not
  // promise, so the path keeps checking itself in production at < 1 % of its time (a checked call costs ~10 x a plain one; the shadow
  // handle -- a second copy of the batch's rows -- is allocated by the first checked call).
  bool check = h->verify;
  if (!check && h->verify_every > 0 && !h->comm && h->persist_state >= 0 && k >= h->persist_min_k && !h->run1m && !h->multistep) {
    if (++h->persist_calls % (uint64_t)h->verify_every == 0) check = true;
  }
  if (!check) return run_random_steps_impl(h, seed0, t0, k, ms_step_kernels);
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (strncmp(cc4_run_kernel_for(h, k), "k_run_", 6) != 0) return run_random_steps_impl(h, seed0, t0, k, ms_step_kernels);
  if (h->plant.part >= 7) return plant_refuse(h, "cc4_run_random_steps");
  if (shadow_seed(h)) return -1;
  cc4_handle* sh = h->shadow;
  int rc = run_random_steps_impl(h, seed0, t0, k, ms_step_kernels);
  if (rc) return rc;
  rc = run_random_steps_impl(sh, seed0, t0, k, nullptr);
  if (rc) { h->err = "CC4_PERSIST_VERIFY: the shadow run failed: " + sh->err; return rc; }
  if (plant_apply(h, nullptr, nullptr, nullptr)) return -1;
  std::string bad;
  if (shadow_compare(h, bad)) return -1;
  if (!bad.empty()) return verify_mismatch(h, std::string(cc4_run_kernel_for(h, k)) + " and the per-step launches disagree after " + std::to_string(k) + " steps: " + bad);
  return 0;
}
// out[0] calls checked, out[1] calls that disagreed (CC4_PERSIST_VERIFY)
int cc4_verify_stats(cc4_handle* h, int64_t* out /* [2] */) { out[0] = h->verify_calls; out[1] = h->verify_mismatches; return 0; }
// One launch of the persistent kernel for k steps of the whole batch (cc4_run_random_steps form 3; cc4_rollout_begin with rollout = true: every step
// an item of its own, the actions from the rollout's slots behind the caller's publishes).
// pl: a plan call (cc4_run_plan_device) -- the plan builds k_run_philox1p / k_run_pcgp on the same schedule, tickets and progress words.
// what k_run_philox1 is compiled for (philox1_body<.., HEAD>): a step that draws its blue actions itself and reads nothing else of a caller's
static bool head_shape(const StepArgs& a, const XchgArgs& x) {
  return a.rand_out && !a.actions && !a.msgs && !a.act_sys && !a.obs8 && !a.prof && !a.ext && !a.dbg_stop && !x.slab;
}
int persist_launch(cc4_handle* h, StepArgs a, int k, uint32_t t0, const XchgArgs& x, hipEvent_t e0, hipEvent_t e1, bool rollout, const PlanArgs* pl) {
  if (h->pool_base + (uint32_t)k > PROGRESS_CLEAR_AT) {      // (the progress words count steps since they were last cleared)
    HIPCHK(h, hipMemsetAsync(h->d_run, 0, h->run_words * sizeof(uint32_t), h->stream));
    h->pool_base = 0;
  }
  // (debug, CC4_PERSIST_TIMELINE: the handle's from the start, so that no path loses it; the stamps of a call nobody reported -- a rollout's -- go back here)
  if (h->d_timeline) release(h, &h->d_timeline);
  if (getenv("CC4_PERSIST_TIMELINE")) {
    const size_t tl_bytes = 4 * sizeof(unsigned long long) * (size_t)h->run_grid;
    if (dev_alloc(h, &h->d_timeline, tl_bytes)) return -1;
    HIPCHK(h, hipMemsetAsync(h->d_timeline, 0, tl_bytes, h->stream));
  }
  // the headline build knows its call's shape at compile time -- actions drawn in the kernel, none given, no messages, nothing of the debug or
  // exchange arguments: a call of any other shape takes the build that reads them at run time
  const bool head = !rollout && !pl && h->cfg.rng_mode != 0 && !h->comm && head_shape(a, x);
  RunArgs ra = run_args(h, k, t0, head);
  ra.ticket = h->d_pool + (size_t)h->pool_parity * CC4_SLOTS * TK_STRIDE;
  ra.ticket_next = h->d_pool + (size_t)(h->pool_parity ^ 1) * CC4_SLOTS * TK_STRIDE;
  ra.base = h->pool_base;
  ra.timeline = h->d_timeline;
  h->pool_parity ^= 1; h->pool_base += (uint32_t)k;
  if (rollout) {
    ra.runs = run_split_steps(k);
    ra.act_ready = h->d_rready; ra.act = h->d_ract; ra.PG = h->rpg;
    ra.act_wait_ticks = (long long)h->rollout_watchdog_ms * wall_khz(h);
  }
  h->last_runs = ra.runs;
  if (pl) {
    if (h->cfg.rng_mode == 0) hipExtLaunchKernelGGL(k_run_pcgp, dim3(h->run_grid), dim3(WAVE), offsetof(EnvState, hd), h->stream, e0, e1, 0, a, ra, *pl);
    else hipExtLaunchKernelGGL(k_run_philox1p, dim3(h->run_grid), dim3(WAVE), offsetof(EnvState, hd), h->stream, e0, e1, 0, a, ra, *pl);
  } else
  if (h->cfg.rng_mode == 0) hipExtLaunchKernelGGL(k_run_pcg, dim3(h->run_grid), dim3(WAVE), offsetof(EnvState, hd), h->stream, e0, e1, 0, a, ra, x);
  else
  if (h->comm) hipExtLaunchKernelGGL(k_run_philox1x, dim3(h->run_grid), dim3(WAVE), offsetof(EnvState, hd), h->stream, e0, e1, 0, a, ra, x);
  else {
    // a rollout leaves `rollout_margin` waves per CU to the caller's policy kernels and the gates (CC4_ROLLOUT_MARGIN)
    const int grid = rollout ? h->run_grid - h->rollout_margin * h->cus : h->run_grid;
    if (rollout) hipExtLaunchKernelGGL(k_run_philox1r, dim3(grid > h->cus ? grid : h->cus), dim3(WAVE), offsetof(EnvState, hd), h->stream, e0, e1, 0, a, ra, x);
    else if (head) hipExtLaunchKernelGGL(k_run_philox1, dim3(grid), dim3(WAVE), offsetof(EnvState, hd), h->stream, e0, e1, 0, a, ra);
    else hipExtLaunchKernelGGL(k_run_philox1g, dim3(grid), dim3(WAVE), offsetof(EnvState, hd), h->stream, e0, e1, 0, a, ra, x);
  }
  return 0;
}
// the timing events of cc4_run_random_steps (cc4_handle::evs): at least `count` of them
static int ensure_events(cc4_handle* h, size_t count) {
  while (h->evs.size() < count) {
    h->evs.push_back(nullptr);
    if (new_event(h, &h->evs.back(), hipEventDefault)) return -1;
  }
  return 0;
}
// ---- the three schedules of cc4_run_random_steps (run_random_steps_impl picks one)
// ONE launch for the k steps: form 1 = every block loops over the steps of its episode (k_run_philox / k_run_philox8), 2 = the same on one wave
// per episode (k_run_philox1m), 3 = the persistent form (k_run_philox1 / k_run_pcg: one wave per residency slot pulling (episode, step) items)
static int run_one_launch(cc4_handle* h, uint64_t seed0, uint32_t t0, int32_t k, float* ms_step_kernels, int form) {
  if (join_groups(h)) return -1;
  StepArgs a = step_args(h);
  a.rand_out = h->d_actions; a.rand_seed0 = seed0; a.rand_t = t0;
  a.full_obs = h->full_obs_next ? 1 : 0;
  XchgArgs x{};
  const bool exchange = h->comm != nullptr;
  static const bool xprof = getenv("CC4_EXCHANGE_PROF") != nullptr;      // debug: where the host's time goes around a one-launch call with the exchange
  const auto xp0 = std::chrono::steady_clock::now();
  if (exchange && xchg_begin(h, k, &x)) return -1;
  const auto xp1 = std::chrono::steady_clock::now();
  if (ms_step_kernels && ensure_events(h, 2)) return -1;
  hipEvent_t e0 = ms_step_kernels ? h->evs[0] : nullptr, e1 = ms_step_kernels ? h->evs[1] : nullptr;
  auto c0 = std::chrono::steady_clock::now();
  if (form == 1) {
    if (h->multistep_minb == 8) hipExtLaunchKernelGGL(k_run_philox8, dim3(h->cfg.num_envs), dim3(PT), sizeof(EnvState), h->stream, e0, e1, 0, a, (int)k, t0, x);
    else hipExtLaunchKernelGGL(k_run_philox, dim3(h->cfg.num_envs), dim3(PT), sizeof(EnvState), h->stream, e0, e1, 0, a, (int)k, t0, x);
  } else if (form == 2) {
    hipExtLaunchKernelGGL(k_run_philox1m, dim3(h->cfg.num_envs), dim3(WAVE), offsetof(EnvState, hd), h->stream, e0, e1, 0, a, (int)k, t0, x);
  } else {
    if (persist_launch(h, a, k, t0, x, e0, e1, false)) return -1;
  }
  HIPCHK(h, hipGetLastError());
  h->stat_launch_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c0).count();
  h->stat_steps += k;
  h->full_obs_next = false;     // (asked for, the first step of every episode rewrote all its observation values)
  h->main_ahead = h->ngroups > 1;
  const auto xp2 = std::chrono::steady_clock::now();
  if (exchange) {
    auto g0 = std::chrono::steady_clock::now();
    if (xchg_enqueue(h, k, x, form)) return -1;
    h->stat_gather_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - g0).count();
  }
  const auto xp3 = std::chrono::steady_clock::now();
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const auto xp4 = std::chrono::steady_clock::now();
  if (h->d_timeline && timeline_report(h, k, ms_step_kernels != nullptr)) return -1;
  if (exchange && xchg_end(h, k)) return -1;
  if (xprof && exchange) exchange_prof_report(k, {xp0, xp1, xp2, xp3, xp4, std::chrono::steady_clock::now()});
  if (ms_step_kernels) HIPCHK(h, hipEventElapsedTime(ms_step_kernels, h->evs[0], h->evs[1]));
  return 0;
}
// every group's k launches from its own thread (EnqPool); this thread takes group 0
static int run_threaded_groups(cc4_handle* h, uint64_t seed0, uint32_t t0, int32_t k, float* ms_step_kernels) {
  const int G = h->ngroups;
  EnqPool* P = h->pool;
  if (ms_step_kernels && ensure_events(h, 2 * (size_t)G)) return -1;
  // (this schedule runs with a pool of ngroups - 1 >= 1 threads only -- run_random_steps_impl -- so the test of ngroups > 1 in fork_groups, which the
  // copy that stood here did without, is always true here)
  if (fork_groups(h)) return -1;
  P->a = step_args(h);
  P->a.rand_out = h->d_actions; P->a.rand_seed0 = seed0; P->a.rand_t = t0;
  P->a.full_obs = 0;            // (enq_run_group sets it per launch: first_full_obs)
  P->k = k; P->t0 = t0; P->full = false; P->first_full_obs = h->full_obs_next;
  for (int g = 0; g < G; ++g) { P->start[g] = ms_step_kernels ? h->evs[2 * g] : nullptr; P->stop[g] = ms_step_kernels ? h->evs[2 * g + 1] : nullptr; }
  P->failed.store(0);
  P->pending.store(G - 1, std::memory_order_relaxed);
  auto c0 = std::chrono::steady_clock::now();
  { std::lock_guard<std::mutex> lk(P->mu); P->gen.fetch_add(1, std::memory_order_release); }
  P->cv.notify_all();
  enq_run_group(h, P, 0);
  while (P->pending.load(std::memory_order_acquire) != 0) __builtin_ia32_pause();
  h->stat_launch_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - c0).count();
  h->stat_steps += k;
  h->full_obs_next = false;
  h->groups_busy = true;
  if (P->failed.load()) { h->err = "cc4_run_random_steps: a step launch failed"; return -1; }
  for (int g = 1; g < G; ++g) HIPCHK(h, hipStreamWaitEvent(h->stream, h->gev[g], 0));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->groups_busy = false;
  if (ms_step_kernels) {
    float worst = 0.f;
    for (int g = 0; g < G; ++g) { float ms = 0.f; HIPCHK(h, hipEventElapsedTime(&ms, h->evs[2 * g], h->evs[2 * g + 1])); if (ms > worst) worst = ms; }
    *ms_step_kernels = worst;
  }
  return 0;
}
// one step after the other from this thread (launch_step: a launch per group), with an all-gather behind every step on a handle with a communicator
static int run_per_step(cc4_handle* h, uint64_t seed0, uint32_t t0, int32_t k, float* ms_step_kernels) {
  // Timing: HIP events on the launch streams around chunks of TIMED_CHUNK consecutive steps (an event pair around every single
  // launch costs the stream ~5 us of idle time per step); per stream, the sum over the chunks is the on-stream time of its k
  // launches, read back after the loop -- no host synchronisation inside the timed region.  With several episode groups
  // (cc4_handle::ngroups) every group's stream is timed; the slowest stream is reported: the on-stream time of the k STEPS.
  constexpr int TIMED_CHUNK = 25;
  const int G = h->ngroups;
  const int nchunks = ms_step_kernels ? (k + TIMED_CHUNK - 1) / TIMED_CHUNK : 0;
  if (ensure_events(h, 2 * (size_t)nchunks * G)) return -1;
  auto ev = [&](int chunk, int g, int which) { return h->evs[(size_t)(2 * (chunk * G + g) + which)]; };
  const bool hp = getenv("CC4_HOST_PROF") != nullptr;
  double t_launch = 0, t_ag = 0, t_first = 0;
  const long long stalls0 = h->gather_stalls;
  // Without a communicator the two timing events of a stream ride on its first and its last launch of the call (start / stop
  // event of hipExtLaunchKernelGGL: the kernels' own start and completion timestamps) -- marker packets from hipEventRecord cost
  // the streams 0.5 us per step at k = 500 and 1.2 us per step at k = 20 (tools/short_region_probe.py).  With a communicator the
  // launches' stop events belong to the exchange and the markers stay.
  const bool attach = ms_step_kernels && !h->comm;
  for (int i = 0; i < k; ++i) {
    if (attach) {
      if (i == 0) for (int g = 0; g < G; ++g) h->tev_start[g] = ev(0, g, 0);
      if (i == k - 1) for (int g = 0; g < G; ++g) h->tev_stop[g] = ev(0, g, 1);
    }
    if (ms_step_kernels && !attach && i % TIMED_CHUNK == 0) {
      if (fork_groups(h)) return -1;     // the group streams' first event must not be recorded ahead of what their first launch waits for
      for (int g = 0; g < G; ++g) HIPCHK(h, hipEventRecord(ev(i / TIMED_CHUNK, g, 0), h->gstream[g]));
    }
    auto c0 = std::chrono::steady_clock::now();
    if (launch_step(h, nullptr, nullptr, true, seed0, t0 + (uint32_t)i)) return -1;   // actions drawn in-kernel
    auto c1 = std::chrono::steady_clock::now();
    if (ms_step_kernels && !attach && (i % TIMED_CHUNK == TIMED_CHUNK - 1 || i == k - 1))
      for (int g = 0; g < G; ++g) HIPCHK(h, hipEventRecord(ev(i / TIMED_CHUNK, g, 1), h->gstream[g]));
    auto c2 = std::chrono::steady_clock::now();
    if (h->comm) { if (cc4_allgather_obs(h, nullptr)) return -1; }                       // overlaps the next step
    auto c3 = std::chrono::steady_clock::now();
    t_launch += std::chrono::duration<double, std::micro>(c1 - c0).count();
    if (i == 0) t_first = std::chrono::duration<double, std::micro>(c1 - c0).count();
    t_ag += std::chrono::duration<double, std::micro>(c3 - c2).count();
  }
  h->stat_steps += k; h->stat_launch_us += t_launch; h->stat_gather_us += t_ag;
  if (hp) fprintf(stderr, "[cc4 host prof] k=%d launch_step %.2f us/step (%d launches per step), allgather enqueue %.2f us/step, %lld buffer-reuse stalls; the call's first launch_step %.1f us\n", k, t_launch / k, G, t_ag / k, h->gather_stalls - stalls0, t_first);
  auto p0 = std::chrono::steady_clock::now();
  if (h->comm) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  if (sync_all(h)) return -1;
  auto p1 = std::chrono::steady_clock::now();
  if (hp) {
    auto q0 = std::chrono::steady_clock::now();
    if (sync_all(h)) return -1;
    auto q1 = std::chrono::steady_clock::now();
    fprintf(stderr, "[cc4 host prof] enqueue loop done -> all streams synchronised: %.1f us; a second sync_all on idle streams: %.1f us\n",
            std::chrono::duration<double, std::micro>(p1 - p0).count(), std::chrono::duration<double, std::micro>(q1 - q0).count());
  }
  if (ms_step_kernels) {
    float worst = 0.f;
    for (int g = 0; g < G; ++g) {
      float total = 0.f;
      for (int c = 0; c < (attach ? 1 : nchunks); ++c) {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, ev(c, g, 0), ev(c, g, 1)));
        total += ms;
      }
      if (total > worst) worst = total;
    }
    *ms_step_kernels = worst;
    if (hp) fprintf(stderr, "[cc4 host prof] reading the timing events: %.1f us\n", std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - p1).count());
  }
  return 0;
}
static int run_random_steps_impl(cc4_handle* h, uint64_t seed0, uint32_t t0, int32_t k, float* ms_step_kernels) {
  h->prev_valid = false;        // (every form of this call moves the rows without refreshing the kept copy of cc4_keep_previous)
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  if (k <= 0) { if (ms_step_kernels) *ms_step_kernels = 0.f; return 0; }   // nothing to launch, no timing event to read
  const bool plain = (!h->comm || h->xchg_on) && !h->evlog_on && !h->ext_seen && !h->d_prof && !h->dbg_stop;
  if (plain && h->persist_state == 0 && !h->run1m && !h->multistep && k >= h->persist_min_k) { if (persist_setup(h)) return -1; }
  const int form = !plain ? 0 : (h->multistep && k >= 2) ? 1 : (h->run1m && k >= 2) ? 2 : (h->persist_state == 1 && h->run_P > 0 && k >= h->persist_min_k) ? 3 : 0;
  if (form) return run_one_launch(h, seed0, t0, k, ms_step_kernels, form);
  if (h->enq_threads && !h->pool && h->ngroups > 1 && !h->comm) enq_pool_start(h);     // on first use: most handles never come here
  if (h->pool && (int)h->pool->th.size() == h->ngroups - 1 && !h->comm && !h->evlog_on && !h->ext_seen && !h->d_prof && k >= 1)
    return run_threaded_groups(h, seed0, t0, k, ms_step_kernels);
  return run_per_step(h, seed0, t0, k, ms_step_kernels);
}
// ---- cc4_run_plan_device (include/cc4.h): k steps with the blue actions of step j from row j of a plan on the device.  Two forms: ONE launch
// of the persistent kernel's plan build (k_run_philox1p / k_run_pcgp: PlanArgs) where cc4_run_random_steps would take the persistent form, else k
// launches of the step kernel, each followed by k_plan_collect (the step's trajectory row).  Neither waits on the host.
// 1: a plan call of k steps takes the one-launch form on this handle as it stands, 0: the per-step form, -1: the persistent kernel's set-up failed
static int plan_form(cc4_handle* h, int32_t k) {
  const bool plain = !h->comm && !h->evlog_on && !h->ext_seen && !h->d_prof && !h->dbg_stop;
  if (!plain || h->multistep || h->run1m || k < h->persist_min_k) return 0;
  if (h->persist_state == 0 && persist_setup(h)) return -1;      // (first use: the discovery pass, the only host wait a plan call can meet; cc4_plan_kernel_for ahead of time keeps it out of the caller's loop)
  return (h->persist_state == 1 && h->run_P > 0) ? 1 : 0;
}
static int run_plan_impl(cc4_handle* h, int32_t k, const int32_t* d_act, const uint8_t* d_msg, float* d_rew, uint8_t* d_done, uint8_t* d_packed, bool one_launch) {
  const size_t n = (size_t)h->cfg.num_envs;
  const int tpb = 256, nb = (int)((n + tpb - 1) / tpb);
  if (join_groups(h)) return -1;
  if (!h->d_plan_err) {
    if (dev_alloc(h, &h->d_plan_err, n * sizeof(uint32_t))) return -1;
    HIPCHK(h, hipMemsetAsync(h->d_plan_err, 0, n * sizeof(uint32_t), h->stream));
  }
  if (one_launch) {
    h->prev_valid = false;        // (as cc4_run_random_steps: the rows move without refreshing the kept copy of cc4_keep_previous)
    StepArgs a = step_args(h);
    a.actions = d_act; a.msgs = d_msg;
    a.full_obs = h->full_obs_next ? 1 : 0;
    const PlanArgs pl{d_act, d_msg, d_rew, d_done, d_packed, h->d_plan_err};
    if (persist_launch(h, a, k, 0u, XchgArgs{}, nullptr, nullptr, false, &pl)) return -1;
    HIPCHK(h, hipGetLastError());
    release(h, &h->d_timeline);      // (debug, CC4_PERSIST_TIMELINE: only cc4_run_random_steps reports it)
    h->stat_steps += k;
    h->full_obs_next = false;
    // the call's flags into the handle's error words; reward / done of the last step went into the trajectory's last row only
    hipLaunchKernelGGL(k_plan_finish, dim3(nb), dim3(tpb), 0, h->stream, (int)n, h->d_err, h->d_plan_err, h->d_mask_stale, h->d_reward,
                       d_rew ? d_rew + (size_t)(k - 1) * n : nullptr, h->d_done, d_done ? d_done + (size_t)(k - 1) * n : nullptr);
    HIPCHK(h, hipGetLastError());
  } else {
    for (int32_t j = 0; j < k; ++j) {
      // a step of the whole batch (one launch on the main stream when the handle steps in groups: launch_step's api_step form), then its row
      if (j > 0 && join_groups(h)) return -1;
      if (launch_step(h, d_act + (size_t)j * n * NBLUE, d_msg ? d_msg + (size_t)j * n * NBLUE * MSG_LEN : nullptr, false, 0, 0, false, true)) return -1;
      if (join_groups(h)) return -1;
      hipLaunchKernelGGL(k_plan_collect, dim3((unsigned)n), dim3(WAVE), 0, h->stream, (int)n, h->d_state, h->d_obs, h->d_reward, h->d_done, h->d_err,
                         d_rew ? d_rew + (size_t)j * n : nullptr, d_done ? d_done + (size_t)j * n : nullptr,
                         d_packed ? d_packed + (size_t)j * n * OBS_PACKED : nullptr, h->d_plan_err);
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_plan_finish, dim3(nb), dim3(tpb), 0, h->stream, (int)n, h->d_err, h->d_plan_err, h->d_mask_stale, h->d_reward, nullptr, h->d_done, nullptr);
    HIPCHK(h, hipGetLastError());
  }
  // the handle's own action buffer holds the call's last row (cc4_get_actions; cc4_replay_logged reads its step's inputs from there)
  const int32_t* last_act = d_act + (size_t)(k - 1) * n * NBLUE;
  if (last_act != h->d_actions) HIPCHK(h, hipMemcpyAsync(h->d_actions, last_act, n * NBLUE * sizeof(int32_t), hipMemcpyDefault, h->stream));
  if (d_msg && d_msg + (size_t)(k - 1) * n * NBLUE * MSG_LEN != h->d_msgs)
    HIPCHK(h, hipMemcpyAsync(h->d_msgs, d_msg + (size_t)(k - 1) * n * NBLUE * MSG_LEN, n * NBLUE * MSG_LEN, hipMemcpyDefault, h->stream));
  if (h->keep_prev && h->prev_valid) { h->prev_actions = h->d_actions; h->prev_msgs = d_msg ? h->d_msgs : nullptr; }
  if (h->ngroups > 1) h->main_ahead = true;      // the group streams follow at their next launch
  return 0;
}
const char* cc4_plan_kernel_for(cc4_handle* h, int32_t k) {
  if (!h) return "";
  if (k >= 1 && !h->comm && h->rollout_k <= 0 && hipSetDevice(h->cfg.device_id) == hipSuccess && plan_form(h, k) == 1)
    return h->cfg.rng_mode == 0 ? "k_run_pcgp" : "k_run_philox1p";
  return cc4_step_kernel(h);
}
int cc4_run_plan_device(cc4_handle* h, int32_t k, const int32_t* d_actions, const uint8_t* d_messages, float* d_rewards, uint8_t* d_dones, uint8_t* d_obs_packed) {
  const char* who = "cc4_run_plan_device";
  if (int rc = enter_refused(h, who, EN_NO_COMM | EN_NO_ROLLOUT)) return rc;
  if (k < 1 || !d_actions) { h->err = std::string(who) + ": k < 1, or no plan"; return -2; }
  if (reinterpret_cast<uintptr_t>(d_obs_packed) % 4 || reinterpret_cast<uintptr_t>(d_rewards) % 4 || reinterpret_cast<uintptr_t>(d_actions) % 4) {
    h->err = std::string(who) + ": plan, rewards and packed observation rows must be 4-byte aligned"; return -2;
  }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int form = plan_form(h, k);
  if (form < 0) return -1;
  if (h->is_shadow || form == 0) return run_plan_impl(h, k, d_actions, d_messages, d_rewards, d_dones, d_obs_packed, form == 1);
  // the self-check of the one-launch forms (cc4_run_random_steps): every call with CC4_PERSIST_VERIFY=1, else every verify_every-th persistent call
  bool check = h->verify;
  if (!check && h->verify_every > 0 && ++h->persist_calls % (uint64_t)h->verify_every == 0) check = true;
  if (!check) return run_plan_impl(h, k, d_actions, d_messages, d_rewards, d_dones, d_obs_packed, true);
  if (h->plant.part >= 7 && (h->plant.step >= k || !(h->plant.part == 7 ? (const void*)d_rewards : h->plant.part == 8 ? (const void*)d_dones : (const void*)d_obs_packed)))
    return plant_refuse(h, who);
  if (shadow_seed(h)) return -1;
  cc4_handle* sh = h->shadow;
  const size_t n = (size_t)h->cfg.num_envs;
  DevTemp<float> t_rew; DevTemp<uint8_t> t_done, t_packed;      // the shadow's trajectory: this call's alone
  if ((d_rewards && t_rew.alloc(h, (size_t)k * n * sizeof(float))) || (d_dones && t_done.alloc(h, (size_t)k * n)) || (d_obs_packed && t_packed.alloc(h, (size_t)k * n * OBS_PACKED))) {
    h->err = "CC4_PERSIST_VERIFY: no memory for the shadow's trajectory"; return -1;
  }
  float* const s_rew = t_rew.p; uint8_t* const s_done = t_done.p; uint8_t* const s_packed = t_packed.p;
  int rc = run_plan_impl(h, k, d_actions, d_messages, d_rewards, d_dones, d_obs_packed, true);
  if (rc) return rc;
  rc = run_plan_impl(sh, k, d_actions, d_messages, s_rew, s_done, s_packed, false);
  if (rc) { h->err = "CC4_PERSIST_VERIFY: the shadow run failed: " + sh->err; return rc; }
  if (plant_apply(h, s_rew, s_done, s_packed)) return -1;
  std::string bad;
  if (shadow_compare(h, bad)) return -1;
  // the trajectory, a step's row at a time (both streams are drained: shadow_compare waited for them) -- whether or not the final digests differ: the
  // first step at which the recorded rows part is what places a disagreement in the call's runs, the digest's episode alone does not
  std::vector<uint8_t> ra, rb;
  size_t differing = 0, first_e = 0;       // of the row that differs: how many episodes, and the first of them (0 episodes: the row could not be fetched)
  auto rows_differ = [&](const void* p, const void* q, size_t per_episode, int32_t j) {
    const size_t row_bytes = n * per_episode;
    ra.resize(row_bytes); rb.resize(row_bytes);
    differing = 0; first_e = 0;
    if (hipMemcpy(ra.data(), static_cast<const uint8_t*>(p) + (size_t)j * row_bytes, row_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(rb.data(), static_cast<const uint8_t*>(q) + (size_t)j * row_bytes, row_bytes, hipMemcpyDeviceToHost) != hipSuccess) return true;
    if (memcmp(ra.data(), rb.data(), row_bytes) == 0) return false;
    for (size_t e = 0; e < n; ++e)
      if (memcmp(ra.data() + e * per_episode, rb.data() + e * per_episode, per_episode) != 0) { if (!differing) first_e = e; ++differing; }
    return true;
  };
  std::string traj;
  for (int32_t j = 0; j < k && traj.empty(); ++j) {
    if (d_rewards && rows_differ(d_rewards, s_rew, sizeof(float), j)) traj = "rewards of step " + std::to_string(j);
    else if (d_dones && rows_differ(d_dones, s_done, 1, j)) traj = "dones of step " + std::to_string(j);
    else if (d_obs_packed && rows_differ(d_obs_packed, s_packed, OBS_PACKED, j)) traj = "packed observations of step " + std::to_string(j);
  }
  if (!traj.empty()) {
    traj = "first differing trajectory row: " + traj + (differing ? ", " + std::to_string(differing) + " episode(s) differ in it, first episode " + std::to_string(first_e)
                                                                    : std::string(" (the row could not be fetched)"));
    bad = bad.empty() ? traj : bad + "; " + traj;
  } else if (!bad.empty()) bad += "; no recorded trajectory row differs";
  if (!bad.empty()) return verify_mismatch(h, std::string(cc4_plan_kernel_for(h, k)) + " and the per-step launches disagree after a plan of " + std::to_string(k) + " steps: " + bad);
  return 0;
}
int cc4_unpack_rows_device(cc4_handle* h, int64_t rows, const uint8_t* d_packed, int32_t obs_dtype, void* d_out) {
  if (obs_dtype < 0 || obs_dtype > 3) { h->err = "cc4_unpack_rows_device: obs_dtype must be 0 (uint8), 1 (float16), 2 (bfloat16) or 3 (float32)"; return -2; }
  if (rows < 0 || (rows > 0 && (!d_packed || !d_out))) { h->err = "cc4_unpack_rows_device: rows < 0, or no buffers"; return -2; }
  static const uintptr_t align[4] = {1, 2, 2, 4};
  if (reinterpret_cast<uintptr_t>(d_out) % align[obs_dtype]) { h->err = "cc4_unpack_rows_device: the output buffer is not aligned to its element size"; return -2; }
  if (rows == 0) return 0;
  if (int rc = enter(h, "cc4_unpack_rows_device")) return rc;
  const long long bytes = (long long)rows * OBS_PACKED;
  const dim3 grid((unsigned)std::max(1LL, std::min((bytes + 255) / 256, 32LL * h->cus))), block(256);
  switch (obs_dtype) {
    case 0: hipLaunchKernelGGL(k_unpack_rows<0>, grid, block, 0, h->stream, d_packed, d_out, (long long)rows); break;
    case 1: hipLaunchKernelGGL(k_unpack_rows<1>, grid, block, 0, h->stream, d_packed, d_out, (long long)rows); break;
    case 2: hipLaunchKernelGGL(k_unpack_rows<2>, grid, block, 0, h->stream, d_packed, d_out, (long long)rows); break;
    default: hipLaunchKernelGGL(k_unpack_rows<3>, grid, block, 0, h->stream, d_packed, d_out, (long long)rows); break;
  }
  HIPCHK(h, hipGetLastError());
  return 0;
}
