"""Seeded random red actions for the tests of cc4_step_red_device (TEST INFRASTRUCTURE), and the views' properties stated from the true-state
document.

red_words draws, per (episode, agent), the four words (type, host, arg, session) the device path takes: every type -1..10, hosts over the whole id
range 0..136 (hosts that are not in the topology included), sessions split between ids the agent really holds (from the document) and
SID_AUTO.  Most records aim at what the agent knows -- an action has to pass the engine's validity check to resolve as itself -- the rest at
anything.  host_records turns the same words into the cc4_agent_action records the host path (cc4_step_ex) takes: ticks 0, no flags, SID_AUTO
resolved with red_view.auto_sid."""
import json

import numpy as np

from cage_challenge_4_amd import red_view as RV

NRED = 6
AGENT_ACTION_DTYPE = [('type', 'i1'), ('host', 'u1'), ('arg', 'u1'), ('ticks', 'u1'), ('session', 'u2'), ('flags', 'u1'), ('pad', 'u1'),
                      ('rate0', 'f8'), ('rate1', 'f8')]


def _bits(words):
    return [32 * w + b for w, v in enumerate(words) for b in range(32) if (v >> b) & 1]


def parse(docs):
    return [json.loads(d) if isinstance(d, (str, bytes)) else d for d in docs]


def red_words(docs, rng, p_none=0.15):
    """docs: one parsed true-state document per episode.  Returns int32 [N, 6, 4]."""
    out = np.zeros((len(docs), NRED, 4), np.int32)
    for e, d in enumerate(docs):
        for r in range(NRED):
            ag = d['red'][r]
            sess = [s[0] for s in ag['sessions']]
            sess_hosts = [s[1] for s in ag['sessions']]
            root_hosts = [s[1] for s in ag['sessions'] if s[3] & 2]
            ips, hns = _bits(ag['as_ip']), _bits(ag['as_hostname'])
            subs = [b for b in range(9) if (ag['as_subnet'] >> b) & 1]

            def pick(known, limit):
                if known and rng.random() < 0.8:
                    return int(known[rng.integers(len(known))])
                return int(rng.integers(limit))
            t = -1 if rng.random() < p_none else int(rng.integers(11))
            host, arg = int(rng.integers(137)), 0
            if t == 0:
                arg = pick(subs, 9)
            elif t in (1, 2, 3, 4):
                host = pick(ips, 137)
            elif t == 5:
                host = pick(sess_hosts or hns, 137)
            elif t in (6, 7):
                host = pick(root_hosts or sess_hosts or hns, 137)
            elif t == 8:
                arg = pick(sess_hosts or hns, 137)
                host = arg if rng.random() < 0.8 else int(rng.integers(137))
            u = rng.random()
            sid = RV.SID_AUTO if u < 0.5 else (int(sess[rng.integers(len(sess))]) if sess and u < 0.95 else int(rng.integers(0, 6)))
            out[e, r] = (t, host, arg, sid)
    return out


def host_records(words, docs):
    """The same actions as cc4_agent_action records for cc4_step_ex: [N, 6]."""
    rec = np.zeros(words.shape[:2], dtype=AGENT_ACTION_DTYPE)
    rec['type'] = words[..., 0]
    live = words[..., 0] != -1
    rec['host'][live] = words[..., 1][live]
    rec['arg'][live] = words[..., 2][live]
    for e, r in np.argwhere(live):
        sid = int(words[e, r, 3])
        rec['session'][e, r] = RV.auto_sid(docs[e], int(r)) if sid == RV.SID_AUTO else sid
    return rec


def resolved_types(docs):
    """The red action types that resolved in the last step somewhere in these episodes (last_red: executed = 1)."""
    return {la[0] for d in docs for la in d['last_red'] if la[3]}


def allowed_rows(doc):
    """[6, 137] bool: the (agent, host) pairs whose row may be non-zero -- the agent knows the host by ip or hostname, holds a session on it, has
    it in its last observation, or started on it."""
    ok = np.zeros((NRED, 137), bool)
    for r, ag in enumerate(doc['red']):
        for h in _bits(ag['as_ip']) + _bits(ag['as_hostname']) + [s[1] for s in ag['sessions']] + [o[0] for o in ag['obs']] + [ag['start']]:
            if h < 137:
                ok[r, h] = True
    return ok
