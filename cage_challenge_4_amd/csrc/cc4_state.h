// cc4_state.h -- packed per-episode state of the CC4 (CybORG v4) step engine.
//
// One episode ("env") = one EnvState (hot, < 16 KB, staged in LDS) + one EnvCold (host backup images, process-list overflow,
// ephemeral-port bitmaps and per-red-session port knowledge; stays in HBM, touched a handful of times per step).  Everything
// is fixed-size POD so that a whole episode can be staged with coalesced loads and snapshot with memcpy.
//
// Process lists (Host.processes) are unbounded in the reference (a blue agent may stack decoys on one host without limit,
// DecoyAction.py:47-114 / DecoyVsftpd.py:10-20): the first PIN entries of a host's list live in the hot row, the rest in the
// cold row (cold_povf).  What bounds a list is the episode length -- DeployDecoy takes two ticks, so an episode of `steps`
// steps stacks at most steps/2 decoys on one host -- so the cold containers are sized from EnterpriseScenarioGenerator(steps=...)
// when the handle is created (cold_povf_cap / cold_sus_cap below): 500 steps -> 376 + 8 = 384 process slots per host (250 decoys,
// 7 generated processes, 127 red shells; the differential fuzz reached 257 with a decoy-only blue policy), 1000 steps -> 632 + 8.
// E_PROC_OVERFLOW beyond.
//
// Host id layout: h = subnet*17 + slot; slot 0 router, 1..10 user_host_0..9, 11..16 server_host_0..5;
// internet root host = 136.  Subnet index = SUBNET enum order of
// CybORG/Simulator/Scenarios/EnterpriseScenarioGenerator.py:40-51.  Iterating existing hosts by
// increasing id == the reference's dict iteration order over state.hosts / state.ip_addresses.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "cc4_rng.h"

namespace cc4 {

enum : int {
  NSUB = 9, SLOTS = 17, MAXH = 137, H_INTERNET = 136,
  MAX_USERS = 10, MAX_SERVERS = 6, ZONE_HOSTS = 16,
  MAXG = 80,            // green agents (one per user host)
  NBLUE = 5, NRED = 6,
  PIN = 8,              // process slots per host in the hot row (every freshly generated host fits: <= 7 processes)
  MAXSV = 7,            // services per host: sshd, OT, {apache | decoy apache} + decoy vsftpd (both port 80), mysql,
                        // decoy tomcat, {smtp | decoy haraka} -- the port checks of DecoyAction exclude any eighth
  MAX_RS = 64,          // sessions per red agent (its ordered list of pool slots)
  RS_POOL = 192,        // red session records per episode, shared by the six agents (r03's occupancy experiment with 96 / MAX_KS 32:
                        // profiles/r03_occupancy_experiment.txt; both generation bitmaps are lent from this pool and need >= 152 records)
  MAX_KS = 96,          // known server-session ids per red agent (ActionSpace.server_session)
  MAX_OBS = 32,         // red observation entries per agent per step (a subnet sweep adds 16, every other source <= 4)
  MAX_PEND = 8,         // process_creation events carrying a pid, per step (one per red agent)
  EPH_WORDS = 340,      // 10880-bit bitmap >= 60000-49152 ephemeral ports (Host.py:183); 1360 B = 85 x 16 B
  OBS_SHORT = 92, OBS_LONG = 210, OBS_TOTAL = 4 * 92 + 210,   // 578
  ACT_SHORT = 82, ACT_LONG = 242, MASK_TOTAL = 4 * 82 + 242,  // 570
  MSG_LEN = 8,
};

// subnet indices (SUBNET enum order)
enum : int { S_RZA = 0, S_OZA = 1, S_RZB = 2, S_OZB = 3, S_CON = 4, S_PUB = 5, S_ADM = 6, S_OFF = 7, S_INT = 8 };

// process / service kinds. Kinds 0..8 double as service-table keys (host.services dict keys).
enum : int {
  K_SSHD = 0, K_OT = 1, K_APACHE = 2, K_MYSQL = 3, K_SMTP = 4,
  K_DEC_APACHE = 5, K_DEC_TOMCAT = 6, K_DEC_HARAKA = 7, K_DEC_VSFTPD = 8,
  K_SESS_BLUE = 9, K_SESS_GREEN = 10, K_SESS_RED = 11,  // Process(name=session_type) of Host.add_session
  K_SHELL = 12,                                          // cmd.sh of ExploitAction._create_new_session
  K_PLAIN = 13,                                          // a process without listening ports (state_edit SE_ADD_SERVICE: the hand-made
                                                         // Process(pid, name) of the reference's tests has no open_ports, so no scan sees it)
};
// listening-port bit codes
enum : int { PB_22 = 1, PB_80 = 2, PB_3390 = 4, PB_25 = 8, PB_1 = 16, PB_443 = 32, PB_HAS = 128 };

// error / bound-overflow flags (cc4 never silently truncates: any bit set => results for that env are flagged)
enum : uint32_t {
  E_PROC_OVERFLOW = 1u << 0, E_RSESS_OVERFLOW = 1u << 1, E_KS_OVERFLOW = 1u << 2, E_KB_OVERFLOW = 1u << 3 /* unused since r02 */,
  E_SUS_OVERFLOW = 1u << 4, E_OBS_OVERFLOW = 1u << 5, E_PEND_OVERFLOW = 1u << 6,
  E_STEP_PAST_END = 1u << 7,      // reference raises ValueError (State.py:539-540)
  E_UNREACHABLE = 1u << 8,        // a path the reference would crash on (documented in DESIGN.md)
  E_BLUE_GREEN_SESSION_KILLED = 1u << 10,   // a stale sus pid / Withdraw hit a blue or green session process (not modelled)
  E_FSM_NO_HOST = 1u << 11,                 // FSM agent with no selectable host (reference: choice([]) raises)
};

struct alignas(4) Proc { uint16_t pid; uint8_t kind; uint8_t flags; };       // flags bit0: user == root
struct alignas(4) Svc  { uint16_t pid; uint8_t kind; uint8_t st; };          // st bit7 active, low bits reliability/20
enum : int { PF_ROOT = 1, SV_ACTIVE = 0x80 };

enum : int { EV_CUR_CONN = 1, EV_CUR_PROC = 2, EV_OLD_CONN = 4, EV_OLD_PROC = 8 };
enum : int { OD_BLOCKS = 1, OD_PHASE = 2, OD_ALL = 7 };   // EnvState.obs_dirty (OD_ALL: what a full rewrite covers on top: the subnet one-hots)

// HostDyn.nsf high nibble: the malware files Analyse reports (Host.files; cleared by Restore): cmd.sh present, escalate.sh present, and
// which of the two was appended last (Observation.add_file_info re-appends a repeated name, so only that order survives)
enum : int { HF_CMD = 1, HF_ESC = 2, HF_ESC_LAST = 4 };
struct alignas(16) HostDyn {        // 64 bytes = four 16-byte vectors
  Proc procs[PIN];                  // entries 0 .. PIN-1 of Host.processes; the rest in the cold row (cold_povf)
  Svc svcs[MAXSV];
  uint16_t nproc;                   // length of the whole list (hot + cold part)
  uint8_t gtmp;                     // scratch of the scenario generation (OS distribution, contested-pid marks); 0 outside a reset.
                                    // (The host's event bits live in EnvState.hev: they change every step, this row does not.)
  uint8_t nsf;                      // low nibble: number of services; high nibble: HF_* bits
};
static_assert(sizeof(HostDyn) == 64, "HostDyn is four 16-byte vectors");
struct alignas(8) HostStatic {                 // Host.create_backup (Host.py:316-371)
  Proc procs[8];
  Svc svcs[5];
  uint8_t nproc, nsvc, exists, ip_octet;   // exists: bit 0 host exists, bit 1 OSDistribution (0 UBUNTU, 1 KALI: ESG.py:488-494)
};

// red sessions (state.sessions[red_agent_k], dict order == array order)
enum : int { RS_ABSTRACT = 1, RS_ROOT = 2, RS_ORIG = 4, RS_CHILD = 8 };   // RS_CHILD: session.parent is not None
// One record of the episode's session pool (EnvState.spool).  An agent's sessions are the pool slots listed in
// RedAgent.sord, in dict order; moving a session between agents (different_subnet_agent_reassignment) moves a list entry,
// not the record.  The port knowledge of an abstract session (RedAbstractSession.ports) is the cold row EnvCold.kports[slot].
struct alignas(8) RSess { uint16_t id; uint16_t pid; uint8_t host; uint8_t flags; uint8_t pad[2]; };

// FSM host states (FiniteStateRedAgent.py:441-452)
enum : int { FS_K = 0, FS_KD = 1, FS_S = 2, FS_SD = 3, FS_U = 4, FS_UD = 5, FS_R = 6, FS_RD = 7, FS_F = 8, FS_NONE = 0xFF };
// red action types in FSM action_list column order (FiniteStateRedAgent.py:393-411) + non-FSM
enum : int { RA_DRS = 0, RA_AGGR = 1, RA_STEALTH = 2, RA_DECEPTION = 3, RA_EXPLOIT = 4, RA_PRIVESC = 5, RA_IMPACT = 6,
             RA_DEGRADE = 7, RA_WITHDRAW = 8, RA_SLEEP = 9, RA_INVALID = 10, RA_NONE = 11 };
// blue action types
enum : int { BA_SLEEP = 0, BA_MONITOR = 1, BA_ANALYSE = 2, BA_REMOVE = 3, BA_RESTORE = 4, BA_DECOY = 5, BA_BLOCK = 6, BA_ALLOW = 7 };
// built-in policies selectable through EnterpriseScenarioGenerator(red_agent_class=, green_agent_class=)
enum : int { RP_FSM = 0, RP_SLEEP = 1, RP_DISCOVERY = 2, RP_RANDOM = 3, GP_SLEEP_BIT = 0x10,
             GP_OPEN_BIT = 0x40 /* with GP_SLEEP_BIT: the green agents have no policy of their own here (a host-side agent class submits
                                   their actions) but, unlike SleepAgent's, their action space holds the green actions (ESG.py:714,742-746) */,
             BP_RANDOM_BIT = 0x20 /* blue_agent_class=cc4BlueRandomAgent: acts for every blue agent no action is submitted for */ };
// TernaryEnum (Shared/Enums.py:5-25)
enum : int { T_TRUE = 1, T_UNKNOWN = 2, T_FALSE = 3, T_IN_PROGRESS = 4 };

struct alignas(8) Act { uint8_t type; uint8_t host; uint8_t arg; uint8_t ticks; uint16_t sid; uint16_t busy; };
// Act.host: target host (blue/red) ; Act.arg: subnet (DRS) or from-subnet (Block/Allow) ; Act.busy: bit 0 queued, bits 1-2: the
// action came with its own rates (AQ_RATE0 / AQ_RATE1: EnvCold.xrate[agent], see ExtAct)
enum : int { AQ_BUSY = 1, AQ_RATE0 = 2, AQ_RATE1 = 4 };

// One externally submitted red or green action of a step: SimulationController.step takes `actions[agent_name]` for ANY agent
// and asks the scenario's agent object only for the agents the dict has no entry for (SimulationController.py:236-240;
// CybORG.step(agent, action), env.py:125-161).  The blue agents' actions arrive as wrapper indices (cc4_step); these records are
// the red and green entries of the dict: [0, NRED) red_agent_r, [NRED, NRED + MAXG) green_agent_g.
//   type   XA_NONE: no entry -- the agent's own policy acts (and draws).  Red: RA_* (RA_INVALID = an action the agent's action
//          space does not hold: InvalidAction, SimulationController.py:1085-1091).  Green: XG_*.
//   host   ip_address / hostname parameter as a host id; arg: DiscoverRemoteSystems subnet index, Withdraw hostname host id
//   sid    session parameter;  ticks: `action.duration` when the caller set one (the reference's tests do), 0 = the class's own
//   flags  XF_RATE0 / XF_RATE1: rate0 / rate1 replace the action's probability attributes -- Aggressive / StealthServiceDiscovery
//          detection_rate (rate0); DiscoverDeception detection_rate (rate0), fp_rate (rate1); GreenLocalWork fp_detection_rate
//          (rate0), phishing_error_rate (rate1); GreenAccessService fp_detection_rate (rate0).
//          XF_SKIP_VALID: skip_valid_action_check=True (SimulationController.py:241)
enum : int { XA_NONE = -1, XG_ACCESS = 0, XG_LOCAL = 1, XG_SLEEP = 2, XG_INVALID = 3 };
enum : int { XF_RATE0 = 1, XF_RATE1 = 2, XF_SKIP_VALID = 4 };
struct alignas(8) ExtAct { int8_t type; uint8_t host; uint8_t arg; uint8_t ticks; uint16_t sid; uint8_t flags; uint8_t pad; double rate0, rate1; };
static_assert(sizeof(ExtAct) == 24, "ExtAct mirrors cc4_agent_action (include/cc4.h)");
enum : int { EXT_PER_ENV = NRED + MAXG };
// a blue wrapper index may carry `action.duration` as well: bits 20..27 (0 = the class's own duration)
enum : int { BLUE_DUR_SHIFT = 20, BLUE_IDX_MASK = (1 << BLUE_DUR_SHIFT) - 1 };

// red observation entry (one dict key of the agent's combined Observation)
enum : int { OE_KEY_IP = 1, OE_SESS = 2, OE_IFACE = 4, OE_SYSHN = 8 };
struct alignas(2) ObsEnt { uint8_t host; uint8_t flags; };

// A red agent's scalar fields, 32 bytes = two 16-byte vectors: the policy / tick path of a step reads them as one batch into
// registers, works there, and writes them back once (every field read separately is an LDS round trip on the agent's
// dependency chain) -- through the word view below (RedHdrW), not a copy of the struct.
struct alignas(16) RedHdr {
  Act queue;                         // actions_in_progress[agent]
  uint16_t as_subnet;                // ActionSpace.subnet known bits
  uint16_t fsm_step;
  uint16_t new_sess_id;
  uint8_t nsess, nknown, fsm_n, nobs;
  uint8_t nlive;                     // popcount(live_hosts)
  uint8_t active;                    // AgentInterface.active
  uint8_t obs_success;               // success of observations[0]
  uint8_t obs_act_type, obs_act_host, obs_act_arg;   // 'action' of observations[0] (RA_NONE if absent / not FSM-relevant)
  uint8_t exec_type, exec_host;      // self.action[agent][0] of this step (for reward)
  uint8_t new_sess_host;             // host of a session created by this agent's exploit this step (0xFF none)
  uint8_t start_host;                // static per episode
  uint8_t rsc_dirty;                 // session table changed since the last full RedSessionCheck observation
  uint8_t rsc_listed;                // this step's observation includes the RedSessionCheck listing of every session
  uint8_t fsm_dirty;                 // the set of session hosts may have changed since fsm_observe last merged a listing
  uint8_t pad[1];
};
static_assert(sizeof(RedHdr) == 32, "RedHdr is two 16-byte vectors");

// ---- The header and the action records as words. The layout in memory is RedHdr / Act, bit for bit; this is how the policy / tick
// path holds them: the header as eight 32-bit words, an Act as one 64-bit word, every field a (word, shift, width) taken from offsetof / sizeof of
// the structs, so a get is one bit-field extract and a set one insert.  Left as a struct copy, the compiler gives every byte field a register of
// its own, reads the 32 bytes with eight narrow LDS instructions and puts them together again in front of eight narrow writes.
struct WField { int word, shift, width; };
constexpr WField wfield_at(size_t off, size_t size) { return WField{(int)(off / 4), (int)(off % 4) * 8, (int)size * 8}; }
constexpr uint32_t wfield_max(WField f) { return f.width >= 32 ? 0xFFFFFFFFu : ((1u << f.width) - 1u); }
constexpr uint32_t wfield_mask(WField f) { return wfield_max(f) << f.shift; }
enum : int {
  RH_Q_TYPE, RH_Q_HOST, RH_Q_ARG, RH_Q_TICKS, RH_Q_SID, RH_Q_BUSY, RH_AS_SUBNET, RH_FSM_STEP, RH_NEW_SESS_ID, RH_NSESS, RH_NKNOWN, RH_FSM_N,
  RH_NOBS, RH_NLIVE, RH_ACTIVE, RH_OBS_SUCCESS, RH_OBS_ACT_TYPE, RH_OBS_ACT_HOST, RH_OBS_ACT_ARG, RH_EXEC_TYPE, RH_EXEC_HOST, RH_NEW_SESS_HOST,
  RH_START_HOST, RH_RSC_DIRTY, RH_RSC_LISTED, RH_FSM_DIRTY, RH_NFIELDS
};
enum : int { AW_TYPE, AW_HOST, AW_ARG, AW_TICKS, AW_SID, AW_BUSY, AW_NFIELDS };
#define CC4_WF(T, m) wfield_at(offsetof(T, m), sizeof(T::m))
#define CC4_WFQ(m) wfield_at(offsetof(RedHdr, queue) + offsetof(Act, m), sizeof(Act::m))
constexpr WField act_field(int f) {    // in the record's two words
  switch (f) {
    case AW_TYPE: return CC4_WF(Act, type);   case AW_HOST: return CC4_WF(Act, host);   case AW_ARG: return CC4_WF(Act, arg);
    case AW_TICKS: return CC4_WF(Act, ticks); case AW_SID: return CC4_WF(Act, sid);     default: return CC4_WF(Act, busy);
  }
}
constexpr WField hdr_field(int f) {
  switch (f) {
    case RH_Q_TYPE: return CC4_WFQ(type);   case RH_Q_HOST: return CC4_WFQ(host);   case RH_Q_ARG: return CC4_WFQ(arg);
    case RH_Q_TICKS: return CC4_WFQ(ticks); case RH_Q_SID: return CC4_WFQ(sid);     case RH_Q_BUSY: return CC4_WFQ(busy);
    case RH_AS_SUBNET: return CC4_WF(RedHdr, as_subnet);         case RH_FSM_STEP: return CC4_WF(RedHdr, fsm_step);
    case RH_NEW_SESS_ID: return CC4_WF(RedHdr, new_sess_id);     case RH_NSESS: return CC4_WF(RedHdr, nsess);
    case RH_NKNOWN: return CC4_WF(RedHdr, nknown);               case RH_FSM_N: return CC4_WF(RedHdr, fsm_n);
    case RH_NOBS: return CC4_WF(RedHdr, nobs);                   case RH_NLIVE: return CC4_WF(RedHdr, nlive);
    case RH_ACTIVE: return CC4_WF(RedHdr, active);               case RH_OBS_SUCCESS: return CC4_WF(RedHdr, obs_success);
    case RH_OBS_ACT_TYPE: return CC4_WF(RedHdr, obs_act_type);   case RH_OBS_ACT_HOST: return CC4_WF(RedHdr, obs_act_host);
    case RH_OBS_ACT_ARG: return CC4_WF(RedHdr, obs_act_arg);     case RH_EXEC_TYPE: return CC4_WF(RedHdr, exec_type);
    case RH_EXEC_HOST: return CC4_WF(RedHdr, exec_host);         case RH_NEW_SESS_HOST: return CC4_WF(RedHdr, new_sess_host);
    case RH_START_HOST: return CC4_WF(RedHdr, start_host);       case RH_RSC_DIRTY: return CC4_WF(RedHdr, rsc_dirty);
    case RH_RSC_LISTED: return CC4_WF(RedHdr, rsc_listed);       default: return CC4_WF(RedHdr, fsm_dirty);
  }
}
#undef CC4_WF
#undef CC4_WFQ
// every field lies inside one word, no two share a bit, and together they are the struct less its padding
constexpr bool wfields_tile(WField (*field)(int), int nfields, int nwords, int pad_bits) {
  uint32_t used[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int bits = 0;
  for (int f = 0; f < nfields; ++f) {
    const WField d = field(f);
    if (d.word < 0 || d.word >= nwords || d.width < 8 || d.shift + d.width > 32 || (used[d.word] & wfield_mask(d))) return false;
    used[d.word] |= wfield_mask(d); bits += d.width;
  }
  return bits + pad_bits == 32 * nwords;
}
static_assert(wfields_tile(hdr_field, RH_NFIELDS, 8, 8 * (int)sizeof(RedHdr::pad)), "the header's word fields are RedHdr's members");
static_assert(wfields_tile(act_field, AW_NFIELDS, 2, 0) && sizeof(Act) == 8, "the action word's fields are Act's members");
static_assert(hdr_field(RH_Q_TYPE).word == act_field(AW_TYPE).word && hdr_field(RH_Q_BUSY).word == act_field(AW_BUSY).word && offsetof(RedHdr, queue) == 0,
              "RedHdr.queue is words 0 and 1 of the header: the header's queue as an action word is w[0] | w[1] << 32");
static_assert(hdr_field(RH_OBS_SUCCESS).word == 5 && hdr_field(RH_OBS_SUCCESS).shift == 0 && hdr_field(RH_OBS_ACT_TYPE).word == 5 &&
              hdr_field(RH_OBS_ACT_HOST).word == 5 && hdr_field(RH_OBS_ACT_ARG).word == 5, "obs_first's four bytes are word 5, obs_success lowest");
static_assert(act_field(AW_TICKS).word == 0 && act_field(AW_TICKS).shift == 24 && hdr_field(RH_FSM_STEP).shift == 16 && hdr_field(RH_FSM_STEP).width == 16,
              "ticks and fsm_step are the top fields of their words: a count on the word wraps as the member does");

struct RedHdrW { uint32_t w[8]; };
typedef uint64_t ActW;
template <int F> CC4_HD uint32_t hget(const RedHdrW& H) { constexpr WField d = hdr_field(F); return (H.w[d.word] >> d.shift) & wfield_max(d); }
template <int F> CC4_HD void hset(RedHdrW& H, uint32_t v) {
  constexpr WField d = hdr_field(F);
  H.w[d.word] = (H.w[d.word] & ~wfield_mask(d)) | ((v & wfield_max(d)) << d.shift);
}
// field += 1, wrapping at the member's width
template <int F> CC4_HD void hinc(RedHdrW& H) {
  constexpr WField d = hdr_field(F);
  if (d.shift + d.width == 32) H.w[d.word] += 1u << d.shift; else hset<F>(H, hget<F>(H) + 1u);
}
template <int F> CC4_HD uint32_t aget(ActW a) { constexpr WField d = act_field(F); return ((uint32_t)(a >> (32 * d.word)) >> d.shift) & wfield_max(d); }
template <int F> CC4_HD ActW aset(ActW a, uint32_t v) {
  constexpr WField d = act_field(F);
  return (a & ~((uint64_t)wfield_mask(d) << (32 * d.word))) | ((uint64_t)(v & wfield_max(d)) << (32 * d.word + d.shift));
}
CC4_HD constexpr ActW act_word(uint32_t type, uint32_t host, uint32_t arg, uint32_t ticks, uint32_t sid, uint32_t busy) {
  return (uint64_t)((type & 0xFFu) << act_field(AW_TYPE).shift | (host & 0xFFu) << act_field(AW_HOST).shift | (arg & 0xFFu) << act_field(AW_ARG).shift |
                    (ticks & 0xFFu) << act_field(AW_TICKS).shift) |
         (uint64_t)((sid & 0xFFFFu) << act_field(AW_SID).shift | (busy & 0xFFFFu) << act_field(AW_BUSY).shift) << 32;
}
CC4_HD ActW act_tick(ActW a) { return (a & 0xFFFFFFFF00000000ull) | (uint32_t)((uint32_t)a - (1u << 24)); }   // ticks-- as the uint8_t member wraps
CC4_HD ActW act_pack(const Act& a) { return act_word(a.type, a.host, a.arg, a.ticks, a.sid, a.busy); }
CC4_HD Act act_unpack(ActW w) {
  Act a; a.type = (uint8_t)aget<AW_TYPE>(w); a.host = (uint8_t)aget<AW_HOST>(w); a.arg = (uint8_t)aget<AW_ARG>(w); a.ticks = (uint8_t)aget<AW_TICKS>(w);
  a.sid = (uint16_t)aget<AW_SID>(w); a.busy = (uint16_t)aget<AW_BUSY>(w);
  return a;
}
CC4_HD ActW hdr_queue(const RedHdrW& H) { return (uint64_t)H.w[0] | (uint64_t)H.w[1] << 32; }
CC4_HD void hdr_set_queue(RedHdrW& H, ActW q) { H.w[0] = (uint32_t)q; H.w[1] = (uint32_t)(q >> 32); }
// The tick's resets as masks (a new step's observation starts empty): nobs = 0, obs_success = 0, obs_act_type = RA_NONE, new_sess_host = 0xFF, rsc_listed = 0
CC4_HD void hdr_tick_reset(RedHdrW& H) {
  H.w[hdr_field(RH_NOBS).word] &= ~wfield_mask(hdr_field(RH_NOBS));
  uint32_t& ow = H.w[hdr_field(RH_OBS_SUCCESS).word];   // (obs_act_type shares it: static_assert above)
  ow = (ow & ~(wfield_mask(hdr_field(RH_OBS_SUCCESS)) | wfield_mask(hdr_field(RH_OBS_ACT_TYPE)))) | (uint32_t)RA_NONE << hdr_field(RH_OBS_ACT_TYPE).shift;
  H.w[hdr_field(RH_NEW_SESS_HOST).word] |= wfield_mask(hdr_field(RH_NEW_SESS_HOST));
  H.w[hdr_field(RH_RSC_LISTED).word] &= ~wfield_mask(hdr_field(RH_RSC_LISTED));
}
// obs_first(success, type, host, arg) as one word: the first observation of a step sets all four, a later one nothing
CC4_HD constexpr uint32_t hdr_obs_word(uint32_t success, uint32_t type, uint32_t host, uint32_t arg) {
  return (success & 0xFFu) | (type & 0xFFu) << hdr_field(RH_OBS_ACT_TYPE).shift | (host & 0xFFu) << hdr_field(RH_OBS_ACT_HOST).shift | (arg & 0xFFu) << hdr_field(RH_OBS_ACT_ARG).shift;
}
// Load and store.  On the device two 16-byte reads and two 16-byte writes (of LDS, where the row is staged); the loaded words are pinned in vector
// registers, or the optimiser narrows the reads back to the bytes each use wants.  On the host the same bytes through memcpy.
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t cc4_u32x4 __attribute__((ext_vector_type(4)));
#endif
enum : int { HDR_LO = 1, HDR_HI = 2, HDR_BOTH = 3 };   // which 16-byte vector(s) a load reads (the other's words are 0) or a store writes: a vector no path wrote may be skipped
CC4_HD RedHdrW hdr_load(const RedHdr* h, int which = HDR_BOTH) {
  RedHdrW H;
#if defined(__HIP_DEVICE_COMPILE__)
  cc4_u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
  if (which & HDR_LO) { __builtin_memcpy(&a, h, 16); asm volatile("" : "+v"(a)); }
  if (which & HDR_HI) { __builtin_memcpy(&b, reinterpret_cast<const char*>(h) + 16, 16); asm volatile("" : "+v"(b)); }
  H.w[0] = a.x; H.w[1] = a.y; H.w[2] = a.z; H.w[3] = a.w; H.w[4] = b.x; H.w[5] = b.y; H.w[6] = b.z; H.w[7] = b.w;
#else
  for (int i = 0; i < 8; ++i) H.w[i] = 0;
  if (which & HDR_LO) __builtin_memcpy(H.w, h, 16);
  if (which & HDR_HI) __builtin_memcpy(H.w + 4, reinterpret_cast<const char*>(h) + 16, 16);
#endif
  return H;
}
// one word of the header, for a phase that reads two fields of it and owns nothing (a read needs no owner)
CC4_HD uint32_t hdr_word(const RedHdr* h, int word) {
  uint32_t w; __builtin_memcpy(&w, reinterpret_cast<const char*>(__builtin_assume_aligned(h, 16)) + 4 * word, 4);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(w));
#endif
  return w;
}
template <int F> CC4_HD uint32_t wget(uint32_t w) { constexpr WField d = hdr_field(F); return (w >> d.shift) & wfield_max(d); }   // field F of its own word
CC4_HD void hdr_store(RedHdr* h, const RedHdrW& H, int which = HDR_BOTH) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (which & HDR_LO) { cc4_u32x4 a = {H.w[0], H.w[1], H.w[2], H.w[3]}; asm volatile("" : "+v"(a)); __builtin_memcpy(h, &a, 16); }
  if (which & HDR_HI) { cc4_u32x4 b = {H.w[4], H.w[5], H.w[6], H.w[7]}; asm volatile("" : "+v"(b)); __builtin_memcpy(reinterpret_cast<char*>(h) + 16, &b, 16); }
#else
  if (which & HDR_LO) __builtin_memcpy(h, H.w, 16);
  if (which & HDR_HI) __builtin_memcpy(reinterpret_cast<char*>(h) + 16, H.w + 4, 16);
#endif
}
// one 8-byte read / write per record (the word pinned like the header's: a load that two extracts share is otherwise split into their bytes)
CC4_HD ActW act_load(const Act* a) {
  ActW w; __builtin_memcpy(&w, a, 8);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(w));
#endif
  return w;
}
CC4_HD void act_store(Act* a, ActW w) { __builtin_memcpy(a, &w, 8); }

struct alignas(16) RedAgent {
  alignas(8) uint8_t sord[MAX_RS];   // state.sessions[agent] in dict order: pool slots (read eight at a time)
  uint32_t known_bm[8];              // ActionSpace.server_session keys with value True as a bitmap over ids 0..255.  The same set in
                                     // insertion order -- read once when a policy draws a session, scanned only for ids >= 256 -- is
                                     // EnvCold.known_sid[agent] (r06: 1152 bytes of the staged part moved behind the row; with rng2 gone
                                     // too the agent part is 5952 B, which with the kernels' statics is FIVE 1280-byte LDS granules)
  uint8_t fsm_order[MAXH];           // host_states dict insertion order, restricted to hosts whose state is not 'F'
                                     // ('F' is absorbing and excluded from known_hosts, FiniteStateRedAgent.py:114)
  uint8_t fsm_st4[(MAXH + 1) / 2];   // host_states[h]: one nibble per host, FS_* + 1 (0 = not in host_states): fsm_get / fsm_put
  uint32_t fsm_hn[5];                // host_states[ip]['hostname'] is not None
  uint32_t as_ip[5];                 // ActionSpace.ip_address[ip] == True
  uint32_t as_hn[5];                 // ActionSpace.hostname[name] == True
  ObsEnt obs[MAX_OBS];
  uint32_t obs_has[2][5];            // which (key type, host) pairs are already in obs[] this step
  uint32_t fsm_known[5];             // hosts present in host_states (fsm_state != FS_NONE)
  uint32_t fsm_ur[5];                // hosts whose state is U, UD, R or RD (the ones _session_removal_state_change looks at)
  uint32_t fsm_nodrs[5];             // hosts whose state a successful DiscoverRemoteSystems leaves alone (KD, SD, UD, RD, F)
  uint32_t live_hosts[5];            // hosts currently holding >= 1 session of this agent (kept exact by rs_add / rs_remove_at)
  RedHdr h;                          // the agent's scalars (32 bytes)
};

struct alignas(8) BlueAgent {
  uint32_t sus_hosts[5];             // hosts that have at least one entry in sus[] (entries are never removed)
  uint32_t pad2;
  Act queue;
  uint16_t nsus;
  uint8_t parent_host;
  uint8_t last_ok;                   // outcome of the last Block/AllowTrafficZone this agent resolved: 1 TRUE, 3 FALSE (T_*), 0 none
};

struct alignas(64) EnvState {
  Rng rng;
  int32_t step_count, steps, phase;
  int32_t phase_len[3];
  uint32_t err;
  float reward;                      // team reward of the last step (BlueRewardMachine + action_cost)
  uint8_t done, rng_mode, n_green;
  uint8_t policy;                    // bits 0-1 red policy (RP_*), bit 4 green policy (1 = SleepAgent)
  uint8_t rng_split;                 // 1 after CybORG.set_seed: the agents' policies keep drawing from rng2 (see there)
  uint8_t obs_dirty;                 // this step changed a slowly varying part of the flat observation (OD_BLOCKS: a pair of the block matrix, OD_PHASE:
                                     // the mission phase): the lane-parallel kernels rewrite those values only then (the output buffer persists)
  uint8_t assign;                    // the classes this episode regenerates into: 0 = the handle's configuration, else PA_SET | policy bits (below).  Read by
                                     // reset_topology, kept by reset_zero, written only by row_assign: it takes effect at the next regeneration, never mid-episode
  uint8_t pad0;
  uint16_t blocks[NSUB];             // blocks[to] bit from
  uint8_t cidr_octet[NSUB];
  uint8_t n_users[NSUB];
  alignas(8) uint8_t n_servers[NSUB];   // read as one 8-byte word by GreenAccessService
  uint8_t green_host[MAXG];
  uint32_t pend[MAX_PEND];           // (host<<16)|pid process_creation events not yet seen by Monitor
  uint8_t npend, pad1[3];
  uint32_t exists[5];                // host h is part of this episode's topology
  uint32_t red_hosts[5];             // hosts holding a session of ANY red agent (OR of RedAgent.live_hosts, kept incrementally)
  uint32_t spool_used[RS_POOL / 32]; // which records of spool[] are live
  uint8_t msg[NBLUE][MSG_LEN];       // messages submitted with the last step
  Act bexec[NBLUE];                  // self.action[blue_b][0] of the last step (also CybORG.get_last_action)
  Act rexec[NRED];
  int32_t brm;                       // BlueRewardMachine accumulator
  float action_cost;
  int32_t n_actions;                 // actions surviving filter_actions (length of the shuffled index list)
  int32_t n_restore;                 // Restore actions submitted this step (each costs -1)
  // (CybORG.set_seed's second generator -- the stream the policies keep drawing from until the next reset while rng_split is set --
  // is EnvCold.rng2: read by the numpy-stream kernel only, and only after a set_seed.)
  BlueAgent blue[NBLUE];
  RSess spool[RS_POOL];              // red session records of all six agents
  RedAgent red[NRED];
  // HostEvents of every host as EV_* bits (network_connections / process_creation of this step, and of the last one after the
  // end-turn Monitor rolled them over).  Every step raises a few dozen of them (ev_or), the Monitor rolls all 137 and the
  // observation encode reads all 137 -- in the part of the row that is staged in LDS, these are LDS operations; while they were a
  // byte of each HostDyn row, the kernels that leave the host table in HBM touched all 137 rows every step for them.
  alignas(4) uint8_t hev[MAXH + 39];  // (137 bytes + padding that puts the host table on a 64-byte boundary)
  // 64-byte alignment of the table and of the row (rows are allocated back to back from a 256-byte aligned base): every HostDyn is
  // exactly one cache line of HBM / L2 -- the kernels that leave the table there read and write single rows -- and the staged part
  // in front of it is whole lines, so stage-in and stage-out never share a line with a neighbour
  alignas(64) HostDyn hd[MAXH];      // last member: the numpy-stream kernel stages only the part in front of it
};
static_assert(offsetof(EnvState, hd) % 64 == 0 && sizeof(EnvState) % 64 == 0 && sizeof(EnvState) == offsetof(EnvState, hd) + sizeof(HostDyn) * MAXH, "the host table closes the row; row and table are whole cache lines");

// ---- the per-episode assignment of opponent classes (EnvState.assign; cc4_set_policies, cc4_row_set_policies).  An assignment is all three
// classes or none: PA_SET | red class | GP_SLEEP_BIT | BP_RANDOM_BIT, the encoding of EnvState.policy (GP_OPEN_BIT belongs with cc4_step_ex and is
// not assignable).  One definition for the device kernels, the host calls on a single row and the oracle.
enum : int { PA_SET = 0x80, PA_BITS = 3 | GP_SLEEP_BIT | BP_RANDOM_BIT, PA_KEEP = -1 /* CC4_POLICY_KEEP */, PA_DEFAULT = -2 /* CC4_POLICY_DEFAULT */ };
// the word of the row that holds `assign` and the byte's place in it: what reset_zero leaves standing
static_assert(offsetof(EnvState, assign) % 4 == 2, "EnvState.assign is byte 2 of its word");
enum : uint32_t { PA_WORD = (uint32_t)(offsetof(EnvState, assign) / 4), PA_WORD_MASK = 0x00FF0000u };
// the classes a regeneration gives the episode: its assignment, else the caller's (the handle's configuration)
CC4_HD int policy_at_reset(const EnvState* s, int handle_policy) { return (s->assign & PA_SET) ? (s->assign & PA_BITS) : handle_policy; }
// One episode's assignment from (red, green, blue): a class, PA_KEEP or PA_DEFAULT each.  All PA_KEEP: nothing.  PA_DEFAULT (the others PA_DEFAULT or
// PA_KEEP): no assignment.  Otherwise the classes given replace those of the assignment the episode has -- of its live classes if it has none.  False
// and the row untouched: a value out of range (red 0..3, green and blue 0..1), or PA_DEFAULT beside a class.
CC4_HD bool row_assign(EnvState* s, int red, int green, int blue) {
  if (red < PA_DEFAULT || red > 3 || green < PA_DEFAULT || green > 1 || blue < PA_DEFAULT || blue > 1) return false;
  const bool any_default = red == PA_DEFAULT || green == PA_DEFAULT || blue == PA_DEFAULT, any_class = red >= 0 || green >= 0 || blue >= 0;
  if (any_default && any_class) return false;
  if (any_default) { s->assign = 0; return true; }
  if (!any_class) return true;
  int b = ((s->assign & PA_SET) ? s->assign : s->policy) & PA_BITS;
  if (red >= 0) b = (b & ~3) | red;
  if (green >= 0) b = (b & ~GP_SLEEP_BIT) | (green ? GP_SLEEP_BIT : 0);
  if (blue >= 0) b = (b & ~BP_RANDOM_BIT) | (blue ? BP_RANDOM_BIT : 0);
  s->assign = (uint8_t)(PA_SET | b);
  return true;
}
// the live classes and the assignment (PA_DEFAULT where none) of one episode as (red, green, blue); either pointer may be null
CC4_HD void row_policies(const EnvState* s, int8_t* live, int8_t* assigned) {
  if (live) { live[0] = (int8_t)(s->policy & 3); live[1] = (int8_t)((s->policy & GP_SLEEP_BIT) ? ((s->policy & GP_OPEN_BIT) ? 2 : 1) : 0); live[2] = (int8_t)((s->policy & BP_RANDOM_BIT) ? 1 : 0); }
  if (assigned) {
    const int a = s->assign;
    const bool set = (a & PA_SET) != 0;
    assigned[0] = (int8_t)(set ? (a & 3) : PA_DEFAULT); assigned[1] = (int8_t)(set ? ((a & GP_SLEEP_BIT) ? 1 : 0) : PA_DEFAULT); assigned[2] = (int8_t)(set ? ((a & BP_RANDOM_BIT) ? 1 : 0) : PA_DEFAULT);
  }
}

// Work area of one step / one reset: temporaries the phases hand to each other.  Not part of the episode's state (LDS on the
// device, the caller's stack on the host); everything in it is dead between steps.
struct alignas(4) StepWork {        // (word accesses only; 404 bytes, not padded to 416: LDS is allocated in 1280-byte granules and the kernels sit at the edges)
  uint32_t scratch[64];              // ordered (lane 0) sections: small temporaries that would otherwise be dynamically
                                     // indexed private arrays (= scratch memory on the device)
  uint32_t phish_mask[4];            // bit g: green g's LocalWork asked for a PhishingEmail this step (word 3 unused)
  uint32_t pend_r[NRED];             // this step's pid-carrying event of red agent r (0 = none); merged into pend[] in agent order
  uint8_t rs_slot[NRED + 2];         // pool slot reserved for the session red agent r's exploit may create this step (rs_reserve)
  uint8_t green_act[MAXG];           // this step's green choice
  uint32_t hdirty[5];                // bit h: the HostDyn row of host h was written this step (hd_touch): the kernel that stages the host
                                     // table writes back only these rows -- one cache line each -- and a step touches a handful of the 137
};

// optional per-step event log (decoded Monitor observations with ports / peers / pids).  One record per
// HostEvents entry the step produced; the engine itself only needs the flags in HostDyn.ev.
enum : int { MAX_EV = 160 };
struct alignas(4) EvRec {
  uint8_t host;        // host whose events list receives the entry
  uint8_t kind;        // 0 network_connections, 1 process_creation
  uint8_t laddr;       // host whose address is the event's local_address
  uint8_t raddr;       // host whose address is the remote_address (0xFF: none)
  uint16_t lport;      // local_port (0: none)
  uint16_t rport;      // remote_port (0: none)
  uint16_t pid;        // pid (0: none)
  uint8_t rep;         // the entry is appended this many times (SSHBruteForce: 10)
  uint8_t order;       // acting agent in execution order: green host id (0..136), red 200 + r
};
struct alignas(16) EvLog { uint32_t n, step, enabled, pad; EvRec rec[MAX_EV]; };

// The pieces of a step's reward that the step itself throws away (the definition of what is made of them: cc4_reward_terms.h).  Written only by a
// step that carries submitted-action records (Ctx.ext: the full builds of the step kernels, cc4_step_ex, cc4_enable_reward_terms), zeroed by every
// regeneration (reset_finish).
//   lwf / asf     bit g: green_agent_g's action of the step charged the LocalWork-failed / AccessService-failed term of its subnet -- whatever the
//                 table's value in this phase.  Cleared by step_phase, set by step_green_exec: the green actions run behind barriers in every kernel
//   stamp         step_count + 1 as step_phase saw it = step_count as step_end leaves it: the record describes the row's last step iff they are equal
//   restore_at[b] step_count + 1 of the last step in which blue agent b SUBMITTED a Restore (what step_end charges -1 for).  A stamp, not a bit: in
//                 the lane-parallel kernels a submission may run before lane 0 has finished step_phase (see there), so nothing here is cleared by
//                 step_phase and set by a submission.  step_end zeroes the entries of earlier steps, so that after a recording step the record is a
//                 function of that step alone
struct alignas(16) RewardRec { uint32_t lwf[3], asf[3], stamp, pad0, restore_at[NBLUE], pad1[3]; };
static_assert(sizeof(RewardRec) == 64 && NBLUE == 5 && MAXG <= 96, "four 16-byte words; three bitmap words cover the green agents");

// The cold row of an episode: a fixed part (this struct) followed by two containers whose capacity depends on the episode length
// the handle was created for (EnterpriseScenarioGenerator(steps=...)):
//   uint32_t sus[NBLUE][cold_sus_cap(steps)]    VelociraptorServer.sus_pids of blue agent b: (host << 16) | pid, chronological
//                                               (appended by Monitor, read by Remove; counts and per-host presence stay hot)
//   Proc     povf[MAXH][cold_povf_cap(steps)]   entries PIN.. of each host's process list (HostDyn.nproc > PIN)
// Rows are cold_row_bytes(steps) apart (cold_at).  The capacities are pure functions of `steps`, and every use reads `steps`
// from the episode's own row (EnvState.steps: LDS on the device), so no kernel carries them in registers; cc4_set_state refuses
// a row whose `steps` would give other capacities than the handle's.
struct alignas(16) EnvCold {
  HostStatic hs[MAXH];               // backup images (Host.create_backup): read by Restore and reset only
  uint8_t hs_pad[8];                 // keeps what follows 16-byte aligned (137 * 56 + 8 = 7680)
  uint32_t eph[MAXH][EPH_WORDS];     // Host.ephemeral_ports as a bitmap (port-49152)
  EvLog evlog;                       // events of the last step when EvLog.enabled (cc4_enable_event_log)
  uint8_t kports[RS_POOL][MAXH + 7]; // RedAbstractSession.ports[ip]: PB_* bits | PB_HAS; row = pool slot of the session
  double xrate[NRED][2];             // the probability attributes an externally submitted red action was queued with (ExtAct.rate0 / rate1:
                                     // valid while the agent's queued / executing Act carries AQ_RATE0 / AQ_RATE1)
  uint32_t gfail[4];                 // bit g: green_agent_g's action of the last step returned Observation(False) (what CybORG.step /
                                     // parallel_step report as its 'success'; written by the full builds of the step only; word 3 unused)
  RewardRec rwd;                     // why the last step's reward was what it was (cc4_reward_terms.h); written by the full builds of the step only
  uint16_t known_sid[NRED][MAX_KS];  // ActionSpace.server_session keys with value True of red agent r, insertion order; entries
                                     // [0, RedHdr.nknown) are valid (RedAgent.known_bm holds the ids < 256 as a bitmap)
  // CybORG.set_seed (env.py:316-325) hands the new Generator to the controller, the state and the hosts
  // (SimulationController.set_np_random, SC:317-320; State.set_np_random, State.py:241-251) but not to the agent objects,
  // whose np_random was bound when they were created (SC:1041): until the next reset the green / red POLICIES keep drawing
  // from the old stream while everything else draws from the new one.  rng2 is that old stream while EnvState.rng_split is set
  // (numpy-stream mode; the counter mode, which is not bit-comparable with the reference anyway, re-keys all streams).
  Rng rng2;
};
static_assert(sizeof(EnvCold) % 16 == 0, "the containers behind the fixed part start 16-byte aligned");
// Suspicious pids per blue agent: one per pid-carrying process_creation event in its zone, i.e. per successful red exploit
// (ExploitAction.py:264-275); an exploit takes four ticks, so six red agents produce at most 1.5 * steps (500 steps -> 768).
CC4_HD int cold_sus_cap(int steps) { const int c = (3 * steps) / 2 + 18; return (c + 15) & ~15; }
// Process slots per host behind the PIN inline ones: steps / 2 decoys + 7 generated + 127 red shells (500 steps -> 376).
CC4_HD int cold_povf_cap(int steps) { const int c = steps / 2 + 126; return (c + 7) & ~7; }
CC4_HD size_t cold_row_bytes(int steps) {
  return sizeof(EnvCold) + 4u * ((size_t)NBLUE * (size_t)cold_sus_cap(steps) + (size_t)MAXH * (size_t)cold_povf_cap(steps));
}
CC4_HD EnvCold* cold_at(EnvCold* base, size_t e, size_t row_bytes) { return reinterpret_cast<EnvCold*>(reinterpret_cast<char*>(base) + e * row_bytes); }
CC4_HD const EnvCold* cold_at(const EnvCold* base, size_t e, size_t row_bytes) { return reinterpret_cast<const EnvCold*>(reinterpret_cast<const char*>(base) + e * row_bytes); }
CC4_HD uint32_t* cold_sus(EnvCold* c, int steps, int b) { return reinterpret_cast<uint32_t*>(c + 1) + (size_t)b * (size_t)cold_sus_cap(steps); }
CC4_HD const uint32_t* cold_sus(const EnvCold* c, int steps, int b) { return reinterpret_cast<const uint32_t*>(c + 1) + (size_t)b * (size_t)cold_sus_cap(steps); }
CC4_HD uint32_t* cold_povf(EnvCold* c, int steps, int h) {   // one Proc = one word: pid | kind << 16 | flags << 24
  return reinterpret_cast<uint32_t*>(c + 1) + (size_t)NBLUE * (size_t)cold_sus_cap(steps) + (size_t)h * (size_t)cold_povf_cap(steps);
}
CC4_HD const uint32_t* cold_povf(const EnvCold* c, int steps, int h) {
  return reinterpret_cast<const uint32_t*>(c + 1) + (size_t)NBLUE * (size_t)cold_sus_cap(steps) + (size_t)h * (size_t)cold_povf_cap(steps);
}

// The LIVE extents of a cold row: what a copy of the episode (cc4_copy_episodes_device) moves.  Everything else in the row is dead --
// written before it is read again by every path that uses it -- and keeps whatever the destination held:
//   CS_HS      hs (+ hs_pad)                              CS_EVHDR  the evlog header
//   CS_EVREC   evlog.rec[0, n) when the log is on         CS_TAIL   xrate, gfail, rwd, known_sid, rng2 (contiguous: the end of the fixed part)
//   CS_EPH     eph whole, numpy-stream mode only (eph_port / eph_clear return at once in the counter mode)
//   CS_FIXED + i                  kports[i] for the pool slots i set in spool_used (rs_add clears the row of a new abstract session)
//   CS_FIXED + RS_POOL + b        sus[b][0, blue[b].nsus)
//   CS_FIXED + RS_POOL + NBLUE + h  povf[h][0, nproc(h) - PIN) for hosts with nproc > PIN
// Counts are clamped to the containers' capacities (a copy never leaves the row whatever the hot row says).  Every span starts 16-byte
// aligned; its length is a multiple of 4 bytes.
enum : int { CS_HS = 0, CS_EVHDR = 1, CS_EVREC = 2, CS_TAIL = 3, CS_EPH = 4, CS_FIXED = 5, COLD_SPANS = CS_FIXED + RS_POOL + NBLUE + MAXH };
struct ColdSpan { uint32_t off, bytes; };
CC4_HD ColdSpan cold_live_span(const EnvState* s, int steps, int rng_mode, int evlog_on, uint32_t ev_n, int k) {
  constexpr uint32_t o_ev = (uint32_t)offsetof(EnvCold, evlog), o_tail = (uint32_t)offsetof(EnvCold, xrate);
  static_assert(offsetof(EnvCold, eph) % 16 == 0 && offsetof(EnvCold, evlog) % 16 == 0 && offsetof(EnvCold, kports) % 16 == 0 &&
                offsetof(EnvCold, xrate) % 16 == 0 && (MAXH + 7) % 16 == 0 && offsetof(EvLog, rec) == 16, "live spans start 16-byte aligned");
  static_assert(offsetof(EnvCold, gfail) > offsetof(EnvCold, xrate) && offsetof(EnvCold, rwd) > offsetof(EnvCold, gfail) && offsetof(EnvCold, rwd) % 16 == 0 &&
                offsetof(EnvCold, known_sid) > offsetof(EnvCold, rwd) &&
                offsetof(EnvCold, rng2) > offsetof(EnvCold, known_sid), "xrate .. rng2 close the fixed part");
  if (k == CS_HS) return {0u, (uint32_t)offsetof(EnvCold, eph)};
  if (k == CS_EVHDR) return {o_ev, 16u};
  if (k == CS_EVREC) return {o_ev + 16u, evlog_on ? (uint32_t)sizeof(EvRec) * (ev_n < (uint32_t)MAX_EV ? ev_n : (uint32_t)MAX_EV) : 0u};
  if (k == CS_TAIL) return {o_tail, (uint32_t)sizeof(EnvCold) - o_tail};
  if (k == CS_EPH) return {(uint32_t)offsetof(EnvCold, eph), rng_mode == 0 ? (uint32_t)sizeof(EnvCold::eph) : 0u};
  k -= CS_FIXED;
  if (k < RS_POOL) {
    const bool used = (s->spool_used[k >> 5] >> (k & 31)) & 1u;
    return {(uint32_t)offsetof(EnvCold, kports) + (uint32_t)k * (uint32_t)(MAXH + 7), used ? (uint32_t)(MAXH + 7) : 0u};
  }
  k -= RS_POOL;
  const uint32_t scap = (uint32_t)cold_sus_cap(steps), pcap = (uint32_t)cold_povf_cap(steps);
  if (k < NBLUE) {
    const uint32_t ns = s->blue[k].nsus;
    return {(uint32_t)sizeof(EnvCold) + 4u * scap * (uint32_t)k, 4u * (ns < scap ? ns : scap)};
  }
  k -= NBLUE;
  const uint32_t np = s->hd[k].nproc, nx = np > (uint32_t)PIN ? np - (uint32_t)PIN : 0u;
  return {(uint32_t)sizeof(EnvCold) + 4u * (scap * (uint32_t)NBLUE + pcap * (uint32_t)k), 4u * (nx < pcap ? nx : pcap)};
}

}  // namespace cc4
