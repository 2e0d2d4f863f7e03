// cc4_api_comm.hip -- the host side of libcc4.so with a communicator: the exchange around a one-launch kernel (xchg_*), cc4_comm_*, the per-step
// all-gathers, the gather log, the device-side unpacking of gathered rows.
// (The functions of the C ABI take their linkage from their declarations in include/cc4.h and include/cc4_debug.h.)
#include "cc4_host.h"

// ---- the exchange around a one-launch kernel (XchgArgs).  Before the launch: the call's flags cleared on the main stream, the
// communication stream ordered behind that.  After the launch: per chunk of steps, on the communication stream, wait for the chunk's last
// step to be complete (done[k] == episodes: the kernel counts an episode once its packed row is in memory), all-gather the chunk's
// slabs, publish gathered = k + 1.  After the main stream's synchronisation: the communication stream drained, the watchdog flag read.
int xchg_begin(cc4_handle* h, int k, XchgArgs* x) {
  (void)k;
  // counter rows for either kind of group: the partitions of the persistent kernel (one per CU) or groups of 32 neighbouring episodes
  const size_t groups = (size_t)(xchg_groups32_alloc(h->cfg.num_envs) > h->cus ? xchg_groups32_alloc(h->cfg.num_envs) : h->cus);
  {
    const size_t nb = (size_t)h->cfg.num_envs * OBS_PACKED;
    if (!h->d_xslab && dev_alloc(h, &h->d_xslab, nb * cc4_handle::XRING)) return -1;
    if (!h->d_xall && dev_alloc(h, &h->d_xall, nb * (size_t)h->world * cc4_handle::XRING)) return -1;
  }
  if (!h->d_xflags) { if (dev_alloc(h, &h->d_xflags, 2 * sizeof(uint32_t))) return -1; h->xflags_clean = 0; }
  if (!h->d_xgcnt) { if (dev_alloc(h, &h->d_xgcnt, groups * cc4_handle::XRING * sizeof(uint32_t))) return -1; h->xflags_clean = 0; }
  if (ensure_watchdog_word(h)) return -1;
  *h->h_xtimeout = 0;
  if (!h->xflags_clean) {       // normally cleared behind the previous call already (xchg_end): nothing of it in front of this call's launch
    HIPCHK(h, hipMemsetAsync(h->d_xflags, 0, 2 * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_xgcnt, 0, groups * cc4_handle::XRING * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipEventRecord(h->xev, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->xev, 0));
  }
  // (clean -- the usual case: the previous call's communication stream zeroed both words behind its last publish, xchg_enqueue, and the host
  // has waited for that stream since -- nothing of this call's is ordered behind anything: no memset, no event, no cross-stream wait)
  h->xflags_clean = 0;
  *x = XchgArgs{h->d_xslab, h->d_xflags, h->d_xflags + 1, cc4_handle::XRING, (long long)h->xchg_watchdog_ms * wall_khz(h), h->d_xgcnt, h->d_xtimeout};
  return 0;
}
// form: 3 = the persistent kernel (groups = its partitions), else groups of 32 neighbouring episodes
int xchg_enqueue(cc4_handle* h, int k, const XchgArgs& x, int form) {
  const size_t row = (size_t)h->cfg.num_envs * OBS_PACKED;
  const int C = h->xchg_chunk, n = h->cfg.num_envs;
  const int P = form == 3 ? h->run_G : 0, groups = form == 3 ? h->run_G : xchg_groups32(n);
  const long long gate_ticks = 30000LL * wall_khz(h);         // 30 s: a step kernel that never gets there (the host would wait for it forever anyway)
  for (int c0 = 0, hi = 0; c0 < k; c0 = hi + 1) {
    hi = (c0 + C < k ? c0 + C : k) - 1;
    if (hi == k - 1 && hi > c0) --hi;       // the call's last step is a chunk of its own: behind the kernel's end only ONE all-gather is left
    if (c0 % cc4_handle::XRING + (hi - c0) >= cc4_handle::XRING) hi = c0 + cc4_handle::XRING - 1 - c0 % cc4_handle::XRING;     // a chunk's slabs are neighbours in the ring
    hipLaunchKernelGGL(k_xchg_gate, dim3(1), dim3(WAVE), 0, h->comm_stream, x.gcnt, x.ring, groups, n, P, c0, hi, gate_ticks, x.timeout_host, hi == k - 1 ? 1 : 8);
    HIPCHK(h, hipGetLastError());
    if (h->comm_delay_ticks > 0) { hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, h->comm_stream, h->comm_delay_ticks); HIPCHK(h, hipGetLastError()); }
    // ONE all-gather for the chunk's m neighbouring slabs (an ncclAllGather costs the host ~10 us to enqueue, grouped or not: eight of them
    // per chunk were as much as the eight steps of a 1024-episode batch last).  The gathered block of a chunk is rank-major: rank r's rows of
    // the chunk's step j at ((r * m + j - c0) * N) -- for a chunk of one step, the call's last among them, plain [world * N] rows.
    const int s0 = c0 % cc4_handle::XRING, m = hi - c0 + 1;
    uint8_t* const block = h->d_xall + (size_t)s0 * row * (size_t)h->world;
    ncclResult_t r = ncclAllGather(h->d_xslab + (size_t)s0 * row, block, (size_t)m * row, ncclUint8, h->comm, h->comm_stream);
    if (r != ncclSuccess) { h->err = std::string("ncclAllGather: ") + ncclGetErrorString(r); return -1; }
    if (h->d_xlog) for (int j = c0; j <= hi && h->xlog_n < h->xlog_cap; ++j, ++h->xlog_n)     // debug: keep every step's gathered rows as [world * N] (cc4_debug_gather_log)
      for (int rk = 0; rk < h->world; ++rk)
        HIPCHK(h, hipMemcpyAsync(h->d_xlog + ((size_t)h->xlog_n * h->world + rk) * row, block + ((size_t)rk * m + (size_t)(j - c0)) * row, row, hipMemcpyDeviceToDevice, h->comm_stream));
    HIPCHK(h, hipStreamWriteValue32(h->comm_stream, x.gathered, (uint32_t)(hi + 1), 0));
  }
  // behind the call's last publish (every episode has counted its last step: nobody reads the two words any more) the communication stream
  // itself hands them back zeroed for the next call -- the host waits for this stream in xchg_end, so the next launch finds them clean
  HIPCHK(h, hipStreamWriteValue32(h->comm_stream, x.gathered, 0u, 0));
  HIPCHK(h, hipStreamWriteValue32(h->comm_stream, x.timeout, 0u, 0));
  h->gathers_issued += k;
  return 0;
}
int xchg_end(cc4_handle* h, int k) {
  const size_t row = (size_t)h->cfg.num_envs * OBS_PACKED;
  HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  h->gathers_waited = h->gathers_issued;
  const uint32_t flag = *reinterpret_cast<volatile uint32_t*>(h->h_xtimeout);      // (both streams are drained: the kernel's system-scope store has landed)
  h->xchg_calls++;
  const int last = (k - 1) % cc4_handle::XRING;
  h->last_gathered = h->d_xall + last * row * (size_t)h->world;      // (the call's last step is a chunk of its own: plain [world * N] rows)
  h->gather_buf = -2;                               // (not one of the per-step ring's buffers: last_gathered says where)
  // the per-step path's current buffer is to hold the observations of the last step as well -- filled when an explicit cc4_allgather_obs asks
  // for it (a per-step launch or a reset that follows writes a buffer of its own)
  h->obs8_from_slab = last;
  h->step_event_attached = false;
  if (flag) {   // a watchdog fired: some counts may never have been collected -- everything cleared the long way before the next call
    h->xflags_clean = 0;
  } else h->xflags_clean = 1;   // (both words zeroed by the communication stream behind its last publish, the group counters by the gates)
  if (flag) {
    // an item waited longer than the watchdog for its slab: the exchange did not keep up at all (e.g. its kernels found no room beside the
    // one-launch kernel).  The episodes are intact -- a wait that gives up only stops protecting slabs, so gathers of this call may have
    // carried a later step's rows -- and the handle goes back to per-step launches, loudly.
    h->xchg_timeouts++;
    h->xchg_on = false;
    // what this call gathered is not published as valid: the gather log forgets the call's steps, and the observations of the call's last
    // step -- whose slab nothing overwrote -- are gathered again through the per-step path when somebody asks (obs8_from_slab stays)
    h->last_gathered = nullptr; h->gather_buf = -1;
    if (h->d_xlog) h->xlog_n = h->xlog_n >= k ? h->xlog_n - k : 0;
    h->err = "the in-kernel exchange timed out in the last cc4_run_random_steps call (episodes intact; its all-gathers are void; per-step launches from now on)";
    release(h, &h->d_xall);      // (the gathered twin of the ring: world times the ring; the ring itself still holds the last step's rows)
    fprintf(stderr, "[cc4] the in-kernel exchange timed out (a step waited > %d ms for the all-gather of %d steps earlier): this handle returns to per-step launches with the exchange\n",
            h->xchg_watchdog_ms, cc4_handle::XRING);
  }
  return 0;
}

int cc4_comm_unique_id(void* id128) {
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return -1;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  memcpy(id128, &id, 128);
  return 0;
}
int cc4_comm_init(cc4_handle* h, int32_t rank, int32_t world, const void* id128) {
  if (int rc = enter(h, "cc4_comm_init")) return rc;
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  ncclResult_t r = ncclCommInitRank(&h->comm, world, id, rank);
  if (r != ncclSuccess) { h->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r); return -1; }
  h->rank = rank; h->world = world;
  if (!getenv("CC4_GROUPS")) {
    // With the exchange every launch carries a completion event and the host guards the observation ring, so a launch costs the
    // host several times what it costs without; small shards then run into the host.  Measured on MI355X with the exchange on a
    // one-rank communicator (r03, profiles/r03_exchange_groups_world1.txt; M agent-env steps/s, 1 / 2 / 3 launches per step):
    // 1024 episodes 159 / 104 / 111, 2048: 242 / 179 / 220, 4096: 380 / 282 / 420, 8192: 478 / 498 / 607.
    int ng = h->cfg.num_envs >= 4096 ? 3 : 1;      // (8192 episodes with the exchange, 3 / 4 launches per step: 563 / 509 M)
    if (const char* v = getenv("CC4_EXCHANGE_GROUPS")) { ng = atoi(v); if (ng <= 0 || ng > h->ngroups) ng = h->ngroups; }   // tuning override: 0 = keep the handle's groups
    if (ng != h->ngroups) {
      if (sync_all(h)) return -1;
      const int old = h->ngroups;
      configure_groups(h, ng);
      for (int g = old; g < h->ngroups; ++g) {
        if (!h->gstream[g] && new_stream(h, &h->gstream[g])) return -1;
        if (!h->gev[g] && new_event(h, &h->gev[g], hipEventDisableTiming)) return -1;
      }
      h->main_ahead = true;
    }
  }
  size_t nb = (size_t)h->cfg.num_envs * OBS_PACKED;
  if (new_stream(h, &h->comm_stream)) return -1;
  for (int b = 0; b < cc4_handle::OBS_RING; ++b) {
    if (dev_alloc(h, &h->d_obs8[b], nb) || dev_alloc(h, &h->d_all_obs8[b], nb * (size_t)world)) return -1;
    HIPCHK(h, hipMemsetAsync(h->d_obs8[b], 0, nb, h->stream));
    for (int g = 0; g < h->ngroups; ++g) if (new_event(h, &h->ev_step[b][g], hipEventDisableTiming)) return -1;
    if (new_event(h, &h->ev_comm[b], hipEventDisableTiming)) return -1;
  }
  // (the ring of step slabs the one-launch kernels write, XchgArgs, and its gathered twin -- 32 x (1 + world) x N x 148 B -- are allocated by
  // the first call that takes a one-launch form: xchg_begin)
  if (new_event(h, &h->xev, hipEventDisableTiming)) return -1;
  int can_wait = 0;
  (void)hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, h->cfg.device_id);
  h->xchg_on = can_wait != 0;
  if (const char* v = getenv("CC4_EXCHANGE_INKERNEL")) h->xchg_on = h->xchg_on && atoi(v) != 0;
  if (const char* v = getenv("CC4_EXCHANGE_CHUNK")) { h->xchg_chunk = atoi(v); if (h->xchg_chunk < 1) h->xchg_chunk = 1; if (h->xchg_chunk > cc4_handle::XRING / 2) h->xchg_chunk = cc4_handle::XRING / 2; }
  if (const char* v = getenv("CC4_EXCHANGE_WATCHDOG_MS")) { h->xchg_watchdog_ms = atoi(v) > 0 ? atoi(v) : 2000; }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  // the one-launch forms again, now that a step of one episode waits for the slowest episode of sixteen steps earlier: the multi-step kernels
  // must hold the whole batch with a block per CU to spare (at exactly full residency one block that is placed late stalls everybody until
  // the watchdog: tools/micro/ring_protocol.hip), and with peers RCCL's kernels need that room on every form (the persistent kernel's waves
  // pull items, so on one rank it keeps every slot)
  // (the numpy-stream persistent kernel has ONE build, six waves of 80 registers per SIMD: with a communicator its grid leaves eight waves per CU free, so
  // that every SIMD keeps room for the all-gather's kernels -- the counter mode runs its five-waves-per-SIMD build, k_run_philox1x, instead)
  // (counter mode: one wave per CU less also on a one-rank communicator -- r05 ran that case on a full grid, and r06 saw the soak test time out once)
  if (h->xchg_on) { if (choose_run_form(h, 1, h->cfg.rng_mode == 0 ? 8 : 1)) return -1; }
  return 0;
}
// the in-kernel exchange of this handle: out[0] on (1) / off (0), out[1] ring depth in steps, out[2] steps per publish (CC4_EXCHANGE_CHUNK),
// out[3] calls of cc4_run_random_steps it served, out[4] calls whose watchdog fired (the handle then returns to per-step launches)
int cc4_exchange_info(cc4_handle* h, int32_t* out /* [5] */) {
  out[0] = h->xchg_on ? 1 : 0; out[1] = cc4_handle::XRING; out[2] = h->xchg_chunk; out[3] = (int32_t)h->xchg_calls; out[4] = (int32_t)h->xchg_timeouts;
  return 0;
}
// debug / test hook: keep the gathered rows of the next `steps` steps cc4_run_random_steps exchanges from inside a one-launch kernel
// ([steps][world * N] packed rows, in step order), so that a test can check EVERY step's all-gather, not only the last of a burst.
// steps = 0 frees the log.
int cc4_debug_gather_log(cc4_handle* h, int32_t steps) {
  if (!h->comm) { h->err = "cc4_debug_gather_log: cc4_comm_init was not called"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  release(h, &h->d_xlog);
  h->xlog_cap = 0; h->xlog_n = 0;
  if (steps > 0) {
    if (dev_alloc(h, &h->d_xlog, (size_t)steps * h->world * h->cfg.num_envs * OBS_PACKED)) return -1;
    h->xlog_cap = steps;
  }
  return 0;
}
// host copy of the log: out [count][world * N][CC4_OBS_PACKED_BYTES]; returns the number of steps logged so far (< 0: error)
int cc4_get_gather_log(cc4_handle* h, uint8_t* out, int32_t first, int32_t count) {
  if (!h->d_xlog || first < 0 || count < 0 || first + count > h->xlog_n) { h->err = "cc4_get_gather_log: no log, or the range was not logged"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  const size_t row = (size_t)h->world * h->cfg.num_envs * OBS_PACKED;
  if (count) HIPCHK(h, hipMemcpy(out, h->d_xlog + (size_t)first * row, (size_t)count * row, hipMemcpyDeviceToHost));
  return h->xlog_n;
}
// What a multi-GPU run needs to PROVE its scaling line: RCCL's own view of the communicator (how many ranks it spans, which one this
// is, which device it is bound to) and the identity of the device this handle runs on.  out[0] ncclCommCount (1 without a
// communicator), out[1] ncclCommUserRank (0), out[2] ncclCommCuDevice (-1), out[3] the handle's HIP device ordinal, out[4] PCI
// domain, out[5] PCI bus, out[6] PCI device, out[7] compute units; uuid_hex: 32 hex digits + NUL of hipDeviceProp_t::uuid.
int cc4_comm_info(cc4_handle* h, int32_t* out, char* uuid_hex) {
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  int count = 1, urank = 0, cudev = -1;
  if (h->comm) {
    if (ncclCommCount(h->comm, &count) != ncclSuccess || ncclCommUserRank(h->comm, &urank) != ncclSuccess || ncclCommCuDevice(h->comm, &cudev) != ncclSuccess) {
      h->err = "cc4_comm_info: RCCL did not answer"; return -1;
    }
  }
  hipDeviceProp_t prop;
  HIPCHK(h, hipGetDeviceProperties(&prop, h->cfg.device_id));
  out[0] = count; out[1] = urank; out[2] = cudev; out[3] = h->cfg.device_id;
  out[4] = prop.pciDomainID; out[5] = prop.pciBusID; out[6] = prop.pciDeviceID; out[7] = prop.multiProcessorCount;
  if (uuid_hex) { for (int i = 0; i < 16; ++i) snprintf(uuid_hex + 2 * i, 3, "%02x", (unsigned)(unsigned char)prop.uuid.bytes[i]); }
  return 0;
}
// All-gather of the observations written by the most recent step (as bytes, [world*N][578]) over RCCL/xGMI on the
// handle's communication stream: it waits for that step's kernel, runs concurrently with whatever is enqueued next on
// the compute stream (later steps write other buffers of the ring), and is awaited by cc4_allgather_wait / the step that
// reuses its buffer.  *d_all_obs8 is valid after cc4_allgather_wait().
int cc4_allgather_obs(cc4_handle* h, uint8_t** d_all_obs8) {
  if (!h->comm) { h->err = "cc4_allgather_obs: cc4_comm_init was not called"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const int buf = h->obs_buf;
  if (h->obs8_from_slab >= 0) {    // the last step ran inside a one-launch kernel with the exchange: its packed rows are in the exchange ring
    const size_t row = (size_t)h->cfg.num_envs * OBS_PACKED;
    HIPCHK(h, hipMemcpyAsync(h->d_obs8[buf], h->d_xslab + (size_t)h->obs8_from_slab * row, row, hipMemcpyDeviceToDevice, h->stream));
    h->obs8_from_slab = -1;
  }
  if (!h->step_event_attached) {   // e.g. the observations of a reset: main-stream work, behind which the group streams' work was joined
    if (join_groups(h)) return -1;
    HIPCHK(h, hipEventRecord(h->ev_step[buf][0], h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_step[buf][0], 0));
  } else {
    for (int g = 0; g < h->ngroups; ++g) HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_step[buf][g], 0));
  }
  if (h->comm_delay_ticks > 0) { hipLaunchKernelGGL(k_spin, dim3(1), dim3(1), 0, h->comm_stream, h->comm_delay_ticks); HIPCHK(h, hipGetLastError()); }
  size_t cnt = (size_t)h->cfg.num_envs * OBS_PACKED;
  ncclResult_t r = ncclAllGather(h->d_obs8[buf], h->d_all_obs8[buf], cnt, ncclUint8, h->comm, h->comm_stream);
  if (r != ncclSuccess) { h->err = std::string("ncclAllGather: ") + ncclGetErrorString(r); return -1; }
  const long long q = ++h->gathers_issued;
  h->gather_seq[buf] = q;
  h->gather_buf = buf;
  h->last_gathered = h->d_all_obs8[buf];
  HIPCHK(h, hipEventRecord(h->ev_comm[q % cc4_handle::OBS_RING], h->comm_stream));
  if (d_all_obs8) *d_all_obs8 = h->d_all_obs8[buf];
  return 0;
}
int cc4_allgather_wait(cc4_handle* h) {
  if (!h->comm) { h->err = "cc4_allgather_wait: cc4_comm_init was not called"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  return 0;
}
// host copy of the gathered observations of the most recent cc4_allgather_obs (tests / debugging)
int cc4_get_allgathered_obs(cc4_handle* h, uint8_t* out /* [world*N][578] */) {
  if (!h->comm) { h->err = "cc4_get_allgathered_obs: cc4_comm_init was not called"; return -2; }
  if (!h->last_gathered) { h->err = "cc4_get_allgathered_obs: no all-gather has been issued"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  const size_t rows = (size_t)h->world * h->cfg.num_envs;
  std::vector<uint8_t> packed(rows * OBS_PACKED);
  HIPCHK(h, hipMemcpy(packed.data(), h->last_gathered, packed.size(), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < rows; ++r)      // unpack to one byte per value for the host caller
    for (int i = 0; i < OBS_TOTAL; ++i) out[r * OBS_TOTAL + i] = (uint8_t)((packed[r * OBS_PACKED + (i >> 2)] >> (2 * (i & 3))) & 3u);
  return 0;
}
// Device-side consumer of the exchange format: the gathered rows of the most recent cc4_allgather_obs ([world*N] rows of
// CC4_OBS_PACKED_BYTES, 2 bits per value) unpacked to [world*N][578] bytes in a buffer owned by the handle -- what a shared
// on-GPU policy reads.  Enqueued on the communication stream behind the all-gather; *d_obs_u8 is valid after
// cc4_allgather_wait() (or after any later operation ordered behind ev_comm of that gather).
int cc4_unpack_obs_device(cc4_handle* h, uint8_t** d_obs_u8) {
  if (!h->comm) { h->err = "cc4_unpack_obs_device: cc4_comm_init was not called"; return -2; }
  if (!h->last_gathered) { h->err = "cc4_unpack_obs_device: no all-gather has been issued"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  const size_t rows = (size_t)h->world * h->cfg.num_envs;
  if (!h->d_unpacked && dev_alloc(h, &h->d_unpacked, rows * OBS_TOTAL)) return -1;
  hipLaunchKernelGGL(k_unpack_obs, dim3((unsigned)rows), dim3(192), 0, h->comm_stream, h->last_gathered, h->d_unpacked, (int)rows);
  HIPCHK(h, hipGetLastError());
  if (d_obs_u8) *d_obs_u8 = h->d_unpacked;
  return 0;
}
// host copy of that buffer (tests)
int cc4_get_unpacked_obs(cc4_handle* h, uint8_t* out /* [world*N][578] */) {
  if (!h->d_unpacked) { h->err = "cc4_get_unpacked_obs: cc4_unpack_obs_device was not called"; return -2; }
  HIPCHK(h, hipSetDevice(h->cfg.device_id));
  HIPCHK(h, hipStreamSynchronize(h->comm_stream));
  HIPCHK(h, hipMemcpy(out, h->d_unpacked, (size_t)h->world * h->cfg.num_envs * OBS_TOTAL, hipMemcpyDeviceToHost));
  return 0;
}
