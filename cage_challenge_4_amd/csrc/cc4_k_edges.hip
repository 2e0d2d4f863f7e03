// cc4_k_edges.hip -- the Monitor's connection entries as device edge lists: the kernel beside the step (the definition: cc4_blue_edges.h, shared with
// the host function).
//   k_blue_edges  cc4_blue_edges_device: one wavefront per requested episode or bank slot, the rows read where view_rows (cc4_view_src.h) finds
//                 them -- a snapshot slot carries the log header and the live log entries at the same offsets.  A keyed merge of at most MAX_EV = 160 entries, by ranking in LDS:
//                   1. the lanes stride over the entries of the step's event log (when it is valid: at most MAX_EV, 12 bytes each); the qualifying ones
//                      are compacted into LDS -- 64-bit key, rep -- by ballot and prefix popcount, in three rounds of 64;
//                   2. each lane marks which of its (at most three) entries is the first of its key (the head);
//                   3. each head reads all keys once -- every lane the same key in the same iteration: an LDS broadcast -- for its merged count, its
//                      position (distinct smaller keys) and the start of its agent's segment; a head whose position is below max_edges stores its
//                      32-byte row as two 16-byte stores; the heads count themselves per agent with LDS atomics;
//                   4. the lanes write -1 into rows [min(total, max_edges), max_edges), 16 bytes a store, and the eight count words.
//                 LDS: 160 keys, 160 rep words, 8 counters = 1952 bytes, two of the 1280-byte granules.
//                 The empty output of a refused entry: all -1 rows and zero counts.
#include "cc4_view_src.h"
#include "cc4_blue_edges.h"
#include "cc4_kernel_decls.h"

static_assert(BE_MAX == CC4_BLUE_EDGES_MAX && BE_MAX == MAX_EV && BE_COLS == CC4_BLUE_EDGES_COLUMNS && BE_WORDS == CC4_BLUE_EDGES_WORDS,
              "include/cc4.h states the shapes; a list holds at most one edge per entry of the log");
constexpr int BE_ROUNDS = (BE_MAX + WAVE - 1) / WAVE;      // entries per lane

__global__ __launch_bounds__(WAVE) void k_blue_edges(BlueEdgesArgs a) {
  __shared__ uint64_t keys[BE_MAX];
  __shared__ uint32_t reps[BE_MAX];
  __shared__ uint32_t seg[BE_WORDS];                       // heads per agent (words 0 .. NBLUE - 1)
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (i >= a.src.count) return;
  const int E = a.max_edges;
  int4* const out = reinterpret_cast<int4*>(a.edges + (size_t)i * (size_t)E * BE_COLS);      // two int4 per row
  int32_t* const oc = a.counts ? a.counts + (size_t)i * BE_WORDS : nullptr;
  const ViewRows vr = view_rows(a.src, i, lane);        // (wave-uniform: cc4_view_src.h)
  const int4 none = make_int4(-1, -1, -1, -1);
  if (vr.fault) {
    for (int k = lane; k < 2 * E; k += WAVE) out[k] = none;
    if (oc && lane < BE_WORDS) oc[lane] = 0;
    return;
  }
  const EnvState* const s = vr.s;
  const EnvCold* const c = vr.c;
  const EvLog* const lg = &c->evlog;
  const bool valid = bv_events_valid(s, lg);
  const int n = valid ? (int)lg->n : 0;                    // (<= MAX_EV: bv_events_valid)

  // 1. compaction
  if (lane < BE_WORDS) seg[lane] = 0u;
  int m = 0;
  for (int r = 0; r < BE_ROUNDS; ++r) {
    const int k = r * WAVE + lane;
    uint64_t key = 0;
    uint32_t rep = 0;
    bool q = false;
    if (k < n) { const EvRec rec = lg->rec[k]; q = be_key(s, rec, &key); rep = rec.rep; }
    const unsigned long long bal = __ballot(q);
    if (q) { const int at = m + __popcll(bal & ((1ull << lane) - 1ull)); keys[at] = key; reps[at] = rep; }
    m += __popcll(bal);
  }
  __syncthreads();
  // 2. heads (a lane writes only the rep words of its own entries)
  for (int r = 0; r < BE_ROUNDS; ++r) {
    const int k = r * WAVE + lane;
    if (k < m && be_is_head(keys, k)) reps[k] |= BE_HEAD;
  }
  __syncthreads();
  // 3. rank and store
  for (int r = 0; r < BE_ROUNDS; ++r) {
    const int k = r * WAVE + lane;
    if (k >= m || !(reps[k] & BE_HEAD)) continue;
    uint32_t cnt; int pos, g;
    be_rank(keys, reps, m, k, &cnt, &pos, &g);
    const uint64_t key = keys[k];
    atomicAdd(&seg[be_agent(key)], 1u);
    if (pos < E) {
      const BeRow row = be_row(key, cnt, pos - g);
      out[2 * pos] = make_int4(row.w[0], row.w[1], row.w[2], row.w[3]);
      out[2 * pos + 1] = make_int4(row.w[4], row.w[5], row.w[6], row.w[7]);
    }
  }
  __syncthreads();
  // 4. the rest of the list, the counts
  int total = 0;
  for (int b = 0; b < NBLUE; ++b) total += (int)seg[b];
  for (int k = 2 * (total < E ? total : E) + lane; k < 2 * E; k += WAVE) out[k] = none;
  if (oc && lane < BE_WORDS)
    oc[lane] = lane < NBLUE ? (int32_t)seg[lane] : (lane == BEW_TOTAL ? total : (lane == BEW_EVENTS_VALID ? (valid ? 1 : 0) : (int32_t)s->step_count));
}
