// cc4_api_views.hip -- the host side of libcc4.so: the derived views, which read tensors out of the batch without stepping it -- state features, the
// red agents' view, blue's own knowledge, the Monitor's connections as edge lists, reward terms, blue actions sampled from policy logits (include/cc4.h;
// the kernels: cc4_k_feat.hip, cc4_k_red.hip, cc4_k_blue.hip, cc4_k_edges.hip, cc4_k_reward.hip, cc4_k_sample.hip; the definitions: cc4_features.h,
// cc4_red_view.h, cc4_blue_view.h, cc4_blue_edges.h, cc4_reward_terms.h, cc4_sample.h).  Every view has a device entry point and the same definition on the host from one row; the call shape of the device entry
// points is stated at ViewSrc (cc4_args.h) and implemented once here: view_check, view_launch.
// (The learner's pure functions, which read no row at all and take no handle: cc4_api_learn.hip.)
#include "cc4_host.h"
#include "cc4_features.h"
#include "cc4_red_view.h"
#include "cc4_blue_view.h"
#include "cc4_blue_edges.h"
#include "cc4_reward_terms.h"
#include "cc4_sample.h"

// ---- the device entry points.  One launch on the main stream behind the group streams, no host synchronisation; a view only reads rows -- as the
// last step left them -- so the next step launches need no ordering behind it beyond the main stream's own.
// The refusals every view shares, in their order: VIEW_GO, 0 (n == 0: nothing to do), or -2 with the reason in h->err and nothing enqueued.  bad: a
// refusal of the view's own (null: none), tested between n < 0 and n == 0; out0 is required and align0-byte aligned, out1 optional and align1-byte
// aligned; outs: the view's sentence about the two.
constexpr int VIEW_GO = 1;
static int view_check(cc4_handle* h, const char* who, const char* bad, int32_t n, const void* out0, size_t align0, const void* out1, size_t align1,
                      const char* outs, const void* d_bank, int32_t capacity) {
  if (int rc = enter_refused(h, who, EN_NO_ROLLOUT)) return rc;
  if (n < 0) { h->err = std::string(who) + ": n < 0"; return -2; }
  if (bad) { h->err = std::string(who) + ": " + bad; return -2; }
  if (n == 0) return 0;
  if (!out0 || reinterpret_cast<uintptr_t>(out0) % align0 || reinterpret_cast<uintptr_t>(out1) % align1) { h->err = std::string(who) + ": " + outs; return -2; }
  if (d_bank && capacity < 1) { h->err = std::string(who) + ": a bank needs a capacity of at least one slot"; return -2; }
  if (reinterpret_cast<uintptr_t>(d_bank) % 64) { h->err = std::string(who) + ": a bank must be 64-byte aligned"; return -2; }
  return VIEW_GO;
}
// ... and the launch: the source every view reads from, then what is particular to the view (its outputs; max_edges), one wavefront per entry.
template <class Args, class... Rest> static int view_launch(cc4_handle* h, const char* who, void (*k_view)(Args), const void* d_bank, int32_t capacity, const int32_t* d_ids, int32_t n, Rest... rest) {
  if (int rc = enter(h, who)) return rc;
  const Args a{ViewSrc{h->d_state, h->d_cold, h->cold_row, static_cast<const uint8_t*>(d_bank), slot_bytes(h->cold_row), d_ids, n,
                       d_bank ? capacity : h->cfg.num_envs, h->cfg.steps, h->cfg.rng_mode, h->d_copy_fault}, rest...};
  hipLaunchKernelGGL(k_view, dim3(n), dim3(WAVE), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return 0;
}

int cc4_state_features_device(cc4_handle* h, const void* d_bank, int32_t capacity, const int32_t* d_ids, int32_t n, uint8_t* d_hosts, int32_t* d_global) {
  const int rc = view_check(h, "cc4_state_features_device", nullptr, n, d_hosts, 16, d_global, 4,
                            "the host-feature buffer is required and must be 16-byte aligned (the episode words: 4-byte aligned or NULL)", d_bank, capacity);
  return rc == VIEW_GO ? view_launch(h, "cc4_state_features_device", k_state_features, d_bank, capacity, d_ids, n, d_hosts, d_global) : rc;
}
int cc4_red_view_device(cc4_handle* h, const void* d_bank, int32_t capacity, const int32_t* d_ids, int32_t n, uint8_t* d_hosts, int32_t* d_scalars) {
  const int rc = view_check(h, "cc4_red_view_device", nullptr, n, d_hosts, 16, d_scalars, 4,
                            "the host-view buffer is required and must be 16-byte aligned (the agent words: 4-byte aligned or NULL)", d_bank, capacity);
  return rc == VIEW_GO ? view_launch(h, "cc4_red_view_device", k_red_view, d_bank, capacity, d_ids, n, d_hosts, d_scalars) : rc;
}
// of the cold rows: the event log and the sus lists
int cc4_blue_view_device(cc4_handle* h, const void* d_bank, int32_t capacity, const int32_t* d_ids, int32_t n, uint8_t* d_hosts, int32_t* d_scalars) {
  const int rc = view_check(h, "cc4_blue_view_device", nullptr, n, d_hosts, 8, d_scalars, 4,
                            "the host-view buffer is required and must be 8-byte aligned (the agent words: 4-byte aligned or NULL)", d_bank, capacity);
  return rc == VIEW_GO ? view_launch(h, "cc4_blue_view_device", k_blue_view, d_bank, capacity, d_ids, n, d_hosts, d_scalars) : rc;
}
// of the hot rows exists and step_count, of the cold rows the event log
int cc4_blue_edges_device(cc4_handle* h, const void* d_bank, int32_t capacity, const int32_t* d_ids, int32_t n, int32_t max_edges, int32_t* d_edges,
                          int32_t* d_counts) {
  const std::string range = "max_edges must be 1 .. " + std::to_string((int)BE_MAX);
  const int rc = view_check(h, "cc4_blue_edges_device", max_edges < 1 || max_edges > BE_MAX ? range.c_str() : nullptr, n, d_edges, 16, d_counts, 4,
                            "the edge buffer is required and must be 16-byte aligned (the counts: 4-byte aligned or NULL)", d_bank, capacity);
  return rc == VIEW_GO ? view_launch(h, "cc4_blue_edges_device", k_blue_edges, d_bank, capacity, d_ids, n, (int)max_edges, d_edges, d_counts) : rc;
}
// of the cold rows: the record
int cc4_reward_terms_device(cc4_handle* h, const void* d_bank, int32_t capacity, const int32_t* d_ids, int32_t n, int32_t* d_terms, int32_t* d_words) {
  const int rc = view_check(h, "cc4_reward_terms_device", nullptr, n, d_terms, 16, d_words, 16,
                            "the terms buffer is required and must be 16-byte aligned (the words: 16-byte aligned or NULL)", d_bank, capacity);
  return rc == VIEW_GO ? view_launch(h, "cc4_reward_terms_device", k_reward_terms, d_bank, capacity, d_ids, n, d_terms, d_words) : rc;
}
// of the hot rows exists and the agents' busy bytes; beside the rows one input, the logits.  The refusals of its own, in their order:
static const char* sample_bad(int32_t dtype, const void* logits, float temperature, int32_t flags) {
  if (!dtype_ok(dtype)) return "logits_dtype must be 1 (float16), 2 (bfloat16) or 3 (float32)";
  if (!temperature_ok(temperature)) return "the temperature must be finite and positive";
  if (flags & ~(int32_t)SA_FLAGS) return "unknown flag bits (CC4_SAMPLE_GREEDY | CC4_SAMPLE_BUSY)";
  if (reinterpret_cast<uintptr_t>(logits) % 4) return "the logits must be 4-byte aligned";
  return nullptr;
}
int cc4_sample_actions_device(cc4_handle* h, const void* d_bank, int32_t capacity, const int32_t* d_ids, int32_t n, int32_t logits_dtype, const void* d_logits,
                              uint64_t seed0, uint32_t t, float temperature, int32_t flags, int32_t* d_actions, float* d_stats) {
  const int rc = view_check(h, "cc4_sample_actions_device", sample_bad(logits_dtype, d_logits, temperature, flags), n, d_actions, 4, d_stats, 4,
                            "the action buffer is required and must be 4-byte aligned (the stats: 4-byte aligned or NULL)", d_bank, capacity);
  return rc == VIEW_GO ? view_launch(h, "cc4_sample_actions_device", k_sample_actions, d_bank, capacity, d_ids, n, d_logits, (int)logits_dtype, seed0, t, 1.0f / temperature, (int)flags,
                                     d_actions, d_stats) : rc;
}

// The switch of the reward record: the handle behaves as after a cc4_step_red_device whose records were all "the scripted class acts" -- d_ext filled with
// none-records, ext_seen set -- so launch_step and the `plain` tests of cc4_api_run.hip select the full builds and pass a.ext with no condition of their own.
int cc4_enable_reward_terms(cc4_handle* h, int32_t enable) {
  const char* who = "cc4_enable_reward_terms";
  if (int rc = enter(h, who, EN_NO_ROLLOUT)) return rc;
  if (enable) {
    if (!h->d_ext && dev_alloc(h, &h->d_ext, (size_t)h->cfg.num_envs * EXT_PER_ENV * sizeof(ExtAct))) return -1;
    if (!h->ext_seen || h->ext_dirty || h->ext_green_dirty) {
      HIPCHK(h, hipMemsetAsync(h->d_ext, 0xFF, (size_t)h->cfg.num_envs * EXT_PER_ENV * sizeof(ExtAct), h->stream));     // type -1 everywhere: nothing submitted
      h->ext_dirty = false; h->ext_green_dirty = false;
    }
    h->terms_on = true; h->ext_seen = true;
  } else {
    h->terms_on = false;
    h->ext_seen = h->ext_submitted;      // (a handle that has taken red / green actions keeps serving the rates a queued action came with)
  }
  return 0;
}
int cc4_reward_terms_enabled(cc4_handle* h) { return h && h->terms_on ? 1 : 0; }

// ---- the same definitions on the host, from one hot row and (for the views that read it, optionally) its cold row -- cc4_get_state / cc4_get_cold, a
// checkpoint: no device, no handle, through aligned copies of what a view reads (RowCopy, row_copy: cc4_host.h).
enum : unsigned { RC_EVLOG = 1, RC_SUS = 2, RC_RWD = 4 };
// 0, -1 (no memory) or -2 (no such episode length).  steps: null for a view that takes none; else <= 0 becomes the length the row itself was generated
// for, and it sizes the sus lists.  parts: what of the cold row the view reads.
static int row_copies(RowCopy& r, const void* hot_row, const void* cold_row, int32_t* steps, unsigned parts) {
  if (!(r.s = static_cast<EnvState*>(row_copy(hot_row, sizeof(EnvState), alignof(EnvState))))) return -1;
  if (steps) {
    if (*steps <= 0) *steps = r.s->steps;
    if (*steps <= 0 || *steps > (1 << 20)) return -2;
  }
  if (!cold_row) return 0;
  const char* const c = static_cast<const char*>(cold_row);
  if ((parts & RC_EVLOG) && !(r.lg = static_cast<EvLog*>(row_copy(c + offsetof(EnvCold, evlog), sizeof(EvLog), alignof(EvLog))))) return -1;
  if ((parts & RC_SUS) && !(r.sus = static_cast<uint32_t*>(row_copy(c + sizeof(EnvCold), sizeof(uint32_t) * (size_t)NBLUE * (size_t)cold_sus_cap(*steps), 16)))) return -1;
  if ((parts & RC_RWD) && !(r.rwd = static_cast<RewardRec*>(row_copy(c + offsetof(EnvCold, rwd), sizeof(RewardRec), alignof(RewardRec))))) return -1;
  return 0;
}

int cc4_state_features_from_row(const void* hot_row, uint8_t* hosts, int32_t* global) {
  if (!hot_row || !hosts) return -2;
  RowCopy r;
  if (int rc = row_copies(r, hot_row, nullptr, nullptr, 0)) return rc;
  feat_from_row(r.s, hosts, global);
  return 0;
}
int cc4_red_view_from_row(const void* hot_row, uint8_t* hosts, int32_t* scalars) {
  if (!hot_row || !hosts) return -2;
  RowCopy r;
  if (int rc = row_copies(r, hot_row, nullptr, nullptr, 0)) return rc;
  red_view_from_row(r.s, hosts, scalars);
  return 0;
}
int cc4_red_record_from_row(const void* hot_row, int32_t agent, const int32_t* words, cc4_agent_action* out) {
  if (!hot_row || !words || !out || agent < 0 || agent >= NRED) return -2;
  RowCopy r;
  if (int rc = row_copies(r, hot_row, nullptr, nullptr, 0)) return rc;
  ExtActW rec;
  const bool ok = red_record(r.s, agent, words[0], words[1], words[2], words[3], &rec);
  memcpy(out, rec.w, sizeof(*out));
  return ok ? 0 : 1;
}
int cc4_blue_view_from_row(const void* hot_row, const void* cold_row, int32_t steps, uint8_t* hosts, int32_t* scalars) {
  if (!hot_row || !hosts) return -2;
  RowCopy r;
  if (int rc = row_copies(r, hot_row, cold_row, &steps, RC_EVLOG | RC_SUS)) return rc;
  blue_view_from_row(r.s, r.lg, r.sus, steps, hosts, scalars);
  return 0;
}
int cc4_blue_edges_from_row(const void* hot_row, const void* cold_row, int32_t steps, int32_t max_edges, int32_t* edges, int32_t* counts) {
  if (!hot_row || !edges || max_edges < 1 || max_edges > BE_MAX) return -2;
  RowCopy r;
  if (int rc = row_copies(r, hot_row, cold_row, &steps, RC_EVLOG)) return rc;
  blue_edges_from_row(r.s, r.lg, max_edges, edges, counts);
  return 0;
}
int cc4_reward_terms_from_row(const void* hot_row, const void* cold_row, int32_t steps, int32_t* terms, int32_t* words) {
  if (!hot_row || !terms || !words) return -2;
  RowCopy r;
  if (int rc = row_copies(r, hot_row, cold_row, &steps, RC_RWD)) return rc;
  reward_terms_from_row(r.s, r.rwd, terms, words);
  return 0;
}
// 0, 1 (the logits refused some agent: cc4_sample.h), -2
int cc4_sample_actions_from_row(const void* hot_row, const float* logits, uint64_t seed0, uint32_t t, int32_t e, float temperature, int32_t flags,
                                int32_t* actions, float* stats) {
  if (!hot_row || !actions || sample_bad(3, nullptr, temperature, flags)) return -2;
  RowCopy r;
  if (int rc = row_copies(r, hot_row, nullptr, nullptr, 0)) return rc;
  float* l = nullptr;                                                      // (the caller's logits may sit at any address)
  if (logits && !(l = static_cast<float*>(row_copy(logits, sizeof(float) * SA_SLOTS, 16)))) return -1;
  const int refused = sample_from_row(r.s, l, seed0, t, e, 1.0f / temperature, flags, actions, stats);
  free(l);
  return refused ? 1 : 0;
}
