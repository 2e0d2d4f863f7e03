// cc4_reward_terms.h -- why the last step's reward was what it was (include/cc4.h "Reward terms"): one statement, for the device kernel
// (cc4_k_reward.hip: k_reward_terms, one wavefront per episode) and the host function (cc4_reward_terms_from_row: reward_terms_from_row, serial), of
// the pieces the step adds up into EnvState.reward and then throws away:
//   terms [9][4] int32 per subnet (the engine's subnet ids)   0 LocalWork-failed penalties, 1 AccessService-failed penalties, 2 Impact penalties
//                                                             (all <= 0), 3 charged events, counted whatever their weight in this phase
//   words [16] int32                                          valid, step_count, phase, brm, action cost, the five blue agents' shares, the unowned
//                                                             rest, the five agents' own Restore costs
// Sources: of the hot row phase, step_count, n_green, green_host and the red agents' headers (exec_type, exec_host, nsess); of the cold row the
// 64-byte record EnvCold.rwd (cc4_state.h: RewardRec), which only a step that carries submitted-action records writes.
//
// The record and the step it belongs to.  step_phase writes rwd.stamp = step_count + 1, step_end increments step_count, every regeneration zeroes
// the record.  The record describes the step that produced the row exactly when
//   rwd.stamp == step_count            (and step_count >= 1: a regenerated episode has taken no step)
// Otherwise -- a regenerated episode, a step of a fast build or with the event log alone, cc4_edit_state(SE_SET_STEP), no cold row -- word 0 is 0 and
// everything but words 1 and 2 is zero.
// The green terms come from the two bitmaps of the record and the table: bit g charges reward_table(phase, h_subnet(green_host[g]), kind), as
// step_green_exec did (the phase of a row does not change behind step_phase; green_host never does).  The Impact terms need no record:
// step_impact_term reads exec_type, exec_host, nsess and phase, none of which changes behind it in the step (cc4_philox1_body.h, at its call).
// Agent b was charged a Restore in this step iff rwd.restore_at[b] == rwd.stamp.
// With valid set:   words[3] + words[4] == reward (exactly: both are small integers)      sum(words[5..9]) + words[10] == words[3] + words[4]
// Malformed rows (bytes from elsewhere): bits at g >= n_green (n_green clamped to MAXG), a green_host >= 137, an exec_host >= 137 and a phase
// outside 0..2 contribute nothing; nothing is ever used as an index before it is checked.
//
// The per-item functions:
//   rt_valid    the relation above
//   rt_green    green agent g's charge of one kind as a hit (subnet, column, value), if its bit is set
//   rt_impact   red agent r's executed Impact as a hit
//   rt_fold     a hit into the 36 cells (LDS atomics on the device)
//   rt_word     one of the 16 words from the cells
#pragma once
#include "cc4_engine.h"

namespace cc4 {

enum : int { RT_SUBNETS = NSUB, RT_COLS = 4, RT_CELLS = RT_SUBNETS * RT_COLS, RT_WORDS = 16 };
enum : int { RTC_LWF = 0, RTC_ASF, RTC_RIA, RTC_EVENTS };
enum : int { RTW_VALID = 0, RTW_STEP_COUNT, RTW_PHASE, RTW_BRM, RTW_ACTION_COST, RTW_SHARE0, RTW_UNOWNED = RTW_SHARE0 + NBLUE, RTW_RESTORE0 };
static_assert(RT_SUBNETS == 9 && (int)RTC_LWF == (int)RW_LWF && (int)RTC_ASF == (int)RW_ASF && (int)RTC_RIA == (int)RW_RIA && RTC_EVENTS == RT_COLS - 1 &&
              RTW_UNOWNED == 10 && RTW_RESTORE0 + NBLUE == RT_WORDS && RT_CELLS % 4 == 0, "the columns and words of include/cc4.h; the kinds are the table's");

CC4_HD bool rt_valid(const EnvState* s, const RewardRec* r) { return r && s->step_count >= 1 && r->stamp == (uint32_t)s->step_count; }

struct RtHit { int subnet, col, value; };
// kind: RTC_LWF or RTC_ASF
CC4_HD bool rt_green(const EnvState* s, const RewardRec* r, int g, int kind, RtHit* o) {
  const int ng = s->n_green < MAXG ? s->n_green : MAXG;
  if (g < 0 || g >= ng || (unsigned)s->phase > 2u || !bit_get(kind == RTC_LWF ? r->lwf : r->asf, g)) return false;
  const int gh = s->green_host[g];
  if (gh >= MAXH) return false;
  o->subnet = h_subnet(gh); o->col = kind; o->value = reward_table(s->phase, o->subnet, kind);
  return true;
}
CC4_HD bool rt_impact(const EnvState* s, int r, RtHit* o) {
  const RedHdr& h = s->red[r].h;
  const uint32_t w = hdr_word(&h, hdr_field(RH_EXEC_TYPE).word);
  const int eh = (int)wget<RH_EXEC_HOST>(w);
  if (wget<RH_EXEC_TYPE>(w) != RA_IMPACT || h.nsess == 0 || eh >= MAXH || (unsigned)s->phase > 2u) return false;
  o->subnet = h_subnet(eh); o->col = RTC_RIA; o->value = step_impact_term(s, r);       // (the step's own function, on the row as the step left it)
  return true;
}
CC4_HD void rt_fold(int32_t* cells, const RtHit& h) {
  int32_t* const c = cells + h.subnet * RT_COLS;
#if defined(__HIP_DEVICE_COMPILE__)
  if (h.value) atomicAdd(&c[h.col], h.value);
  atomicAdd(&c[RTC_EVENTS], 1);
#else
  c[h.col] += h.value; c[RTC_EVENTS] += 1;
#endif
}
// agent b's own Restore cost: -1 iff it submitted one in the step the record describes
CC4_HD int32_t rt_restore(const RewardRec* r, int b) { return r->restore_at[b] == r->stamp ? -1 : 0; }
// the penalties of the subnets agent b defends (b == -1: of those nobody defends)
CC4_HD int32_t rt_zone_sum(const int32_t* cells, int b) {
  int32_t v = 0;
  for (int sn = 0; sn < RT_SUBNETS; ++sn)
    if (blue_of_subnet(sn) == b) v += cells[sn * RT_COLS + RTC_LWF] + cells[sn * RT_COLS + RTC_ASF] + cells[sn * RT_COLS + RTC_RIA];
  return v;
}
// r may be null when valid is false; cells: the folded hits (all zero when valid is false)
CC4_HD int32_t rt_word(const EnvState* s, const RewardRec* r, bool valid, const int32_t* cells, int k) {
  if (k == RTW_STEP_COUNT) return s->step_count;
  if (k == RTW_PHASE) return s->phase;
  if (!valid || k < 0 || k >= RT_WORDS) return 0;
  if (k == RTW_VALID) return 1;
  if (k == RTW_BRM) { int32_t v = 0; for (int b = -1; b < NBLUE; ++b) v += rt_zone_sum(cells, b); return v; }
  if (k == RTW_ACTION_COST) { int32_t v = 0; for (int b = 0; b < NBLUE; ++b) v += rt_restore(r, b); return v; }
  if (k < RTW_UNOWNED) return rt_zone_sum(cells, k - RTW_SHARE0) + rt_restore(r, k - RTW_SHARE0);
  if (k == RTW_UNOWNED) return rt_zone_sum(cells, -1);
  return rt_restore(r, k - RTW_RESTORE0);
}

// The serial statement: terms [9][4], words [16] from one hot row and the record of its cold row (null: no cold row)
inline void reward_terms_from_row(const EnvState* s, const RewardRec* r, int32_t* terms, int32_t* words) {
  int32_t cells[RT_CELLS] = {};
  const bool valid = rt_valid(s, r);
  if (valid) {
    RtHit h;
    for (int g = 0; g < MAXG; ++g) {
      if (rt_green(s, r, g, RTC_LWF, &h)) rt_fold(cells, h);
      if (rt_green(s, r, g, RTC_ASF, &h)) rt_fold(cells, h);
    }
    for (int a = 0; a < NRED; ++a) if (rt_impact(s, a, &h)) rt_fold(cells, h);
  }
  for (int k = 0; k < RT_CELLS; ++k) terms[k] = cells[k];
  for (int k = 0; k < RT_WORDS; ++k) words[k] = rt_word(s, r, valid, cells, k);
}

}  // namespace cc4
