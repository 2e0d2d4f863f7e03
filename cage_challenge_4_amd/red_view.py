"""What each red agent knows, as fixed-shape arrays: what a learned attacker reads (include/cc4.h, cc4_red_view_device), and the red actions it
submits (cc4_step_red_device).

Per agent and host  [6, 137, 8] uint8   row h = host id (subnet * 17 + slot; 136 = the internet root), columns HOST_COLUMNS.
Per agent           [6, 16] int32       SCALAR_WORDS.
A host the agent does not know by ip or hostname, holds no session on, did not observe in the last step and did not start on is all zero:
nothing of another agent's sessions, of blue's state or of the host table enters the view.

Three ways to the same numbers:
  CC4VecEnv.red_view() / CC4TorchVecEnv.red_view()   the HIP kernel over the batch (k_red_view)
  from_row(row_bytes)          the same definition compiled for the host (cc4_red_view_from_row): from a cc4_get_state row or a checkpoint, in a
                               process without a GPU
  from_true_state(doc)         a NumPy restatement from the true-state document's "red" entries and "last_red": independent of the packed row.  The
                               document does not carry the queued action, so words 2..4 of the scalars (DOC_UNDEFINED_WORDS) stay zero.

A red action is four int32 words (type, host, arg, session), ACTION_WORDS; type ACT_NONE lets the agent's scripted policy act, session SID_AUTO
stands for the agent's first listed session (auto_sid)."""
import ctypes
import numpy as np
from . import _lib as L
from . import _views as V
from ._view_util import _bytes, _doc, call_from_row

NUM_RED, VIEW_HOSTS, VIEW_PER_HOST, VIEW_SCALARS = L.NUM_RED, L.RED_VIEW_HOSTS, L.RED_VIEW_PER_HOST, L.RED_VIEW_SCALARS
ACT_WORDS, SID_AUTO, ACT_NONE = L.RED_ACT_WORDS, L.RED_SID_AUTO, -1
SID_NONE = 65535

HOST_COLUMNS = {'known_ip': 0, 'known_hostname': 1, 'session_level': 2, 'sessions': 3, 'obs': 4, 'abstract': 5, 'start': 6, 'reserved': 7}
SCALAR_WORDS = {'active': 0, 'busy': 1, 'queued_type': 2, 'queued_host': 3, 'queued_ticks': 4, 'obs_success': 5, 'obs_act_type': 6, 'obs_act_host': 7,
                'obs_act_arg': 8, 'nsess': 9, 'as_subnet': 10, 'new_sess_host': 11, 'auto_sid': 12, 'exec_type': 13, 'exec_host': 14, 'step_count': 15}
ACTION_WORDS = {'type': 0, 'host': 1, 'arg': 2, 'session': 3}
DOC_UNDEFINED_WORDS = (2, 3, 4)          # the queued action: not in the true-state document
DOC_WORDS = tuple(k for k in range(VIEW_SCALARS) if k not in DOC_UNDEFINED_WORDS)
OBS_PRESENT = 0x80
_RS_ABSTRACT, _RS_ROOT = 1, 2


def _row(row_bytes):
    lib = L.load()
    return lib, _bytes(row_bytes, lib.cc4_state_bytes(), 'a hot row')


def from_row(row_bytes):
    """(hosts [6, 137, 8] uint8, scalars [6, 16] int32) of one packed hot row (CC4VecEnv.get_state(e), a row of get_states())."""
    return call_from_row('red_view', _row(row_bytes)[1])[:2]


def record_from_row(row_bytes, agent, words):
    """The record cc4_step_red_device makes of words = (type, host, arg, session) for red_agent_<agent> on this row: (record, refused) -- a
    one-element array of the cc4_agent_action dtype (type -1 when refused) and whether the words were refused."""
    lib, row = _row(row_bytes)
    w = np.ascontiguousarray(words, dtype=np.int32).ravel()
    if w.size != ACT_WORDS:
        raise ValueError(f'a red action has {ACT_WORDS} words (type, host, arg, session)')
    rec = np.zeros(1, dtype=L.AGENT_ACTION_DTYPE)
    vp = ctypes.c_void_p
    rc = lib.cc4_red_record_from_row(row.ctypes.data_as(vp), int(agent), w.ctypes.data_as(vp), rec.ctypes.data_as(vp))
    if rc not in (0, 1):
        raise L.CC4Error(f'cc4_red_record_from_row failed (rc={rc})')
    return rec, bool(rc)


def auto_sid(doc, r, none=0):
    """The session id SID_AUTO stands for in a record submitted for red_agent_r: the id of its first listed session -- `none` if it has no
    session (cc4_step_red_device submits id 0 then and the engine's validity check decides; the view's word 12 reports SID_NONE)."""
    sess = _doc(doc)['red'][r]['sessions']
    return int(sess[0][0]) if sess else none


def from_true_state(doc):
    """The same arrays from a true-state document (the JSON text of cc4_get_true_state, its parsed form, or true_state.TrueState): from the
    "red" entries, "last_red" and "step" only.  Words DOC_UNDEFINED_WORDS of the scalars are left zero."""
    d = _doc(doc)
    hosts, scal = V.empty('red_view')
    for r, ag in enumerate(d['red']):
        v = hosts[r]
        for h in range(VIEW_HOSTS):
            v[h, 0] = (ag['as_ip'][h >> 5] >> (h & 31)) & 1
            v[h, 1] = (ag['as_hostname'][h >> 5] >> (h & 31)) & 1
        count = np.zeros(VIEW_HOSTS, np.int64)
        for _sid, h, _pid, fl in ag['sessions']:
            count[h] += 1
            v[h, 2] = max(int(v[h, 2]), 2 if fl & _RS_ROOT else 1)
            if fl & _RS_ABSTRACT:
                v[h, 5] = 1
        v[:, 3] = np.minimum(count, 255)
        for h, fl in ag['obs']:
            v[h, 4] |= OBS_PRESENT | (fl & 15)
        if ag['start'] < VIEW_HOSTS:
            v[ag['start'], 6] = 1
        last = d['last_red'][r]
        scal[r, [0, 1]] = int(bool(ag['active'])), int(bool(ag['busy']))
        scal[r, 5] = ag['obs_success']
        scal[r, 6:9] = ag['obs_action']
        scal[r, 9], scal[r, 10], scal[r, 11] = len(ag['sessions']), ag['as_subnet'], ag['new_session'][0]
        scal[r, 12] = auto_sid(d, r, none=SID_NONE)
        scal[r, 13], scal[r, 14], scal[r, 15] = last[0], last[1], d['step']
    return hosts, scal

