"""The privileged global state of an episode as fixed-shape arrays: what a centralised critic reads (include/cc4.h, cc4_state_features_device).

Per host  [137, 16] uint8   row h = host id (subnet * 17 + slot; 136 = the internet root), columns HOST_COLUMNS; absent hosts are all zero.
Per episode   [32] int32    GLOBAL_WORDS.

Three ways to the same numbers:
  CC4VecEnv.state_features() / CC4TorchVecEnv.state_features()   the HIP kernel over the batch (k_state_features)
  from_row(row_bytes)          the same definition compiled for the host (cc4_state_features_from_row): from a cc4_get_state row or a checkpoint,
                               in a process without a GPU
  from_true_state(ts)          a NumPy restatement from a decoded true-state document (true_state.decode): independent of the packed row, and
                               what a user of the single-episode facade gets
"""
import numpy as np
from . import _lib as L
from . import _views as V
from ._view_util import _bytes, call_from_row

FEAT_HOSTS, FEAT_PER_HOST, FEAT_GLOBAL = L.FEAT_HOSTS, L.FEAT_PER_HOST, L.FEAT_GLOBAL

HOST_COLUMNS = {'exists': 0, 'kind': 1, 'red_level': 2, 'red_agents': 3, 'red_sessions': 4, 'red_knows': 5, 'svc_active': 6, 'svc_present': 7,
                'decoys': 8, 'rel_min': 9, 'events': 10, 'files': 11, 'nproc': 12, 'green': 13, 'blue_sus': 14, 'blue_agent': 15}
GLOBAL_WORDS = {'step_count': 0, 'steps': 1, 'phase': 2, 'done': 3, 'n_green': 4, 'blocks': slice(5, 14), 'red_active': 14, 'red_busy': 15,
                'blue_busy': 16, 'red_nsess': slice(17, 23), 'red_exec_type': slice(23, 29), 'err': 29}
KIND_ROUTER, KIND_USER, KIND_SERVER, KIND_INTERNET = 0, 1, 2, 3
NO_BLUE_AGENT = 255
_BLUE_OF_SUBNET = (0, 1, 2, 3, NO_BLUE_AGENT, 4, 4, 4, NO_BLUE_AGENT)     # ESG.py:643-649
_RS_ROOT = 2


def from_row(row_bytes):
    """(hosts [137, 16] uint8, glob [32] int32) of one packed hot row (CC4VecEnv.get_state(e), a row of get_states())."""
    return call_from_row('state_features', _bytes(row_bytes, L.load().cc4_state_bytes(), 'a hot row'))[:2]


def host_kind(h):
    if h == 136:
        return KIND_INTERNET
    slot = h % 17
    return KIND_ROUTER if slot == 0 else (KIND_USER if slot <= 10 else KIND_SERVER)


def from_true_state(ts, steps=0, err=0):
    """The same arrays from a decoded true-state document (true_state.TrueState, or the parsed JSON of cc4_get_true_state).  The document
    does not carry the episode length nor the error flags (CC4VecEnv.err): words 1 and 29 are `steps` and `err` as given."""
    d = ts if isinstance(ts, dict) else ts.raw
    hosts, glob = V.empty('state_features')
    nsess, root, agents = np.zeros(FEAT_HOSTS, np.int64), np.zeros(FEAT_HOSTS, bool), np.zeros(FEAT_HOSTS, np.int64)
    for r, ag in enumerate(d['red']):
        for _sid, h, _pid, fl in ag['sessions']:
            nsess[h] += 1
            root[h] |= bool(fl & _RS_ROOT)
            agents[h] |= 1 << r
    green = set(d['green_hosts'])
    sus = {h for ag in d['blue'] for h, _pid in ag['sus']}
    for hd in d['hosts']:
        h = hd['h']
        row = hosts[h]
        row[0] = 1
        row[1] = host_kind(h)
        row[2] = 0 if nsess[h] == 0 else (2 if root[h] else 1)
        row[3] = agents[h]
        row[4] = min(int(nsess[h]), 255)
        row[5] = sum(((ag['as_ip'][h >> 5] >> (h & 31)) & 1) << r for r, ag in enumerate(d['red']))
        rel = []
        for kind, active, percent, _pid in hd['svcs']:
            if kind <= 4:
                row[7] |= 1 << kind
                if active:
                    row[6] |= 1 << kind
            elif kind <= 8:
                row[8] |= 1 << (kind - 5)
            rel.append(percent // 20)
        row[9] = min(rel) if rel else 0
        row[10] = hd['ev'] & 15
        row[11] = hd.get('files', 0) & 3
        row[12] = min(len(hd['procs']), 255)
        row[13] = int(h in green)
        row[14] = int(h in sus)
        row[15] = _BLUE_OF_SUBNET[h // 17]
    glob[0], glob[1], glob[2], glob[3], glob[4] = d['step'], int(steps), d['phase'], d['done'], d['n_green']
    glob[5:14] = d['blocks']
    glob[14] = sum(int(bool(ag['active'])) << r for r, ag in enumerate(d['red']))
    glob[15] = sum(int(bool(ag['busy'])) << r for r, ag in enumerate(d['red']))
    glob[16] = sum(int(bool(ag['busy'])) << b for b, ag in enumerate(d['blue']))
    glob[17:23] = [len(ag['sessions']) for ag in d['red']]
    glob[23:29] = [la[0] for la in d['last_red']]
    glob[29] = np.array(int(err) & 0xFFFFFFFF, np.uint32).astype(np.int32)
    return hosts, glob
