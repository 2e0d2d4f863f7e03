"""Blue's own knowledge as fixed-shape arrays: what the reference hands a blue agent in its dict observation and the flat 578-value vector drops
(include/cc4.h, cc4_blue_view_device) -- whether the agent is busy, the outcome of its own action, what Analyse found, which decoy it deployed, the
suspicious pids Remove would act on, and per host the entries of the end-turn Monitor: how many, on which ports, from which remote hosts.

Per agent and host  [5, 137, 8] uint8   row h = host id (subnet * 17 + slot; 136 = the internet root), columns HOST_COLUMNS.
Per agent           [5, 16] int32       SCALAR_WORDS.
A row (b, h) is all zero unless h exists in b's zone, or h was the remote address of an entry in b's zone this step (then only 'remote_seen' is
set): nothing of red's tables, of the session pool, of another agent's suspicious pids or of the host table beyond the analysed host's files enters.
Columns 3..6, the decoy part of 'own' and word 11 need the per-step event log (enable_event_log()); word 10, 'events_valid', says whether they are
filled.  Without the log the view still carries busy / success / Analyse / sus_pids.

Three ways to the same numbers:
  CC4VecEnv.blue_view() / CC4TorchVecEnv.blue_view()   the HIP kernel over the batch (k_blue_view)
  from_row(hot, cold=None, steps=0)   the same definition compiled for the host (cc4_blue_view_from_row): from cc4_get_state / cc4_get_cold rows or
                                      a checkpoint, in a process without a GPU
  from_true_state(doc)                a NumPy restatement from the true-state document only: independent of the packed rows.  The document does not
                                      carry the queued action, so words 1..3 of the scalars (DOC_UNDEFINED_WORDS) stay zero."""
import numpy as np
from . import _lib as L
from . import _views as V
from ._view_util import MAX_EVENTS, ZONE_OF_SUBNET, _doc, _rows, call_from_row, events_valid  # noqa: F401  (MAX_EVENTS, events_valid: part of this module's surface)

NUM_BLUE, VIEW_HOSTS, VIEW_PER_HOST, VIEW_SCALARS = L.NUM_BLUE, L.BLUE_VIEW_HOSTS, L.BLUE_VIEW_PER_HOST, L.BLUE_VIEW_SCALARS

HOST_COLUMNS = {'in_zone': 0, 'events': 1, 'sus_pids': 2, 'conn_entries': 3, 'proc_entries': 4, 'remote_seen': 5, 'ports': 6, 'own': 7}
SCALAR_WORDS = {'busy': 0, 'queued_type': 1, 'queued_host': 2, 'queued_ticks': 3, 'exec_type': 4, 'exec_host': 5, 'exec_arg': 6, 'success': 7,
                'nsus': 8, 'parent_host': 9, 'events_valid': 10, 'zone_entries': 11, 'phase': 12, 'step_count': 13, 'reserved0': 14, 'reserved1': 15}
EVENT_COLUMNS = (3, 4, 5, 6)             # filled from the event log only
DOC_UNDEFINED_WORDS = (1, 2, 3)          # the queued action: not in the true-state document
DOC_WORDS = tuple(k for k in range(VIEW_SCALARS) if k not in DOC_UNDEFINED_WORDS)
PORT_BITS = {22: 1, 80: 2, 3390: 4, 25: 8, 1: 16, 443: 32}
PORT_PID, OWN_DECOY = 0x40, 0x80         # CC4_BLUE_VIEW_PORT_PID, CC4_BLUE_VIEW_OWN_DECOY
T_TRUE, T_UNKNOWN, T_FALSE, T_IN_PROGRESS = 1, 2, 3, 4
SLEEP, MONITOR, ANALYSE, REMOVE, RESTORE, DECOY, BLOCK, ALLOW = range(8)


def from_row(hot, cold=None, steps=0):
    """(hosts [5, 137, 8] uint8, scalars [5, 16] int32) of one packed hot row (CC4VecEnv.get_state(e)) and its cold row (the second part of
    CC4VecEnv.snapshot(e)).  cold=None: the event columns, 'sus_pids' and the decoy bits are zero and events_valid is 0.  steps: the episode
    length of the env the rows come from (it sizes the cold row, which must be the whole cc4_cold_bytes() of that env); 0: the length the hot
    row itself records."""
    return call_from_row('blue_view', *_rows(hot, cold), int(steps))[:2]


def from_true_state(doc):
    """The same arrays from a true-state document (the JSON text of cc4_get_true_state, its parsed form, or true_state.TrueState): from the
    "blue" entries (busy / traffic_ok / sus / parent), "last_blue", the hosts' "ev" / "files", "events" / "events_step" / "events_total", "phase"
    and "step" only.  Words DOC_UNDEFINED_WORDS of the scalars are left zero."""
    d = _doc(doc)
    hosts, scal = V.empty('blue_view')
    info = {hd['h']: hd for hd in d['hosts']}
    zone = {h: ZONE_OF_SUBNET[h // 17] for h in info}
    count = np.zeros((NUM_BLUE, VIEW_HOSTS, 4), np.int64)            # sus, conn, proc, remote
    for h, hd in info.items():
        if zone[h] >= 0:
            hosts[zone[h], h, 0] = 1
            hosts[zone[h], h, 1] = hd['ev'] & 15
    for b, ag in enumerate(d['blue']):
        for h, _pid in ag['sus']:
            if zone.get(h, -1) == b:
                count[b, h, 0] += 1
    valid = events_valid(d)
    decoy = {}
    total = [0] * NUM_BLUE
    if valid:
        for _order, seq, host, kind, laddr, lport, raddr, _rport, pid, rep in d['events']:
            b = zone.get(host, -1)
            if b < 0:
                continue
            if kind == 2:
                decoy[host] = max(decoy.get(host, (-1, 0)), (seq, laddr))
                continue
            if kind > 2 or rep == 0:
                continue
            count[b, host, 1 + kind] += rep
            total[b] += rep
            if kind == 0:
                hosts[b, host, 6] |= PORT_BITS.get(lport, 0)
            if pid:
                hosts[b, host, 6] |= PORT_PID
            if raddr < VIEW_HOSTS:
                count[b, raddr, 3] += rep
    count = np.minimum(count, 255)
    hosts[..., 2], hosts[..., 3], hosts[..., 4], hosts[..., 5] = count[..., 0], count[..., 1], count[..., 2], count[..., 3]
    for b, ag in enumerate(d['blue']):
        ty, host, arg = d['last_blue'][b]
        busy = bool(ag['busy'])
        if not busy and zone.get(host, -1) == b:
            if ty == ANALYSE:
                hosts[b, host, 7] = info[host].get('files', 0) & 7
            elif ty == DECOY and host in decoy:
                hosts[b, host, 7] = OWN_DECOY | (decoy[host][1] & 0x7F)
        if busy:
            ok = T_IN_PROGRESS
        elif ty == SLEEP:
            ok = T_UNKNOWN
        elif ty in (BLOCK, ALLOW):
            ok = ag['traffic_ok']
        else:
            ok = T_TRUE if ty <= DECOY else 0
        scal[b, 0] = int(busy)
        scal[b, 4:7] = (ty, host, arg)
        scal[b, 7], scal[b, 8], scal[b, 9] = ok, len(ag['sus']), ag['parent']
        scal[b, 10], scal[b, 11], scal[b, 12], scal[b, 13] = int(valid), total[b], d['phase'], d['step']
    return hosts, scal
