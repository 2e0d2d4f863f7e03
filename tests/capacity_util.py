"""Crafted episodes at the capacities of the engine's bounded containers (TEST INFRASTRUCTURE; DESIGN.md section 2: "Bounded containers never
truncate silently").  build(ora, e, scenario) fills a container of episode e of an OracleVecEnv to one below its capacity ('m1'), to exactly its
capacity ('cap') or to its capacity with the operation that overflows it ('over'), with cc4_edit_state ops where one exists and byte pokes into
the episode's rows (snapshot / restore; offsets from cc4o_layout) where none does.  No capacity is a literal here: cc4o_caps(steps).

A scenario is '<container>:<variant>'.  The operation -- what 'm1' and 'over' do and 'cap' does not -- is one of
  * edits applied after the crafted state has been copied wherever it goes (`Built.edits`: the same op on the oracle and on a device handle must
    return the same value, -1 where the engine refuses it);
  * actions submitted with the FIRST step (`Built.red` / `Built.green` records for step_ex, `Built.blue` raw blue actions for any step);
  * nothing: the crafted state itself carries it (a foreign session that the step's reassignment moves, a pending event that the step hands over).
So 'm1' ends exactly full and clean, 'cap' stays full and clean, 'over' raises exactly `Built.flag` -- by the end of the first step at the latest
(`Built.needs_ext`: only on a step that takes submitted red / green actions)."""
import ctypes
import json

import numpy as np

from oracle_binding import load

STEPS = 60                                   # episode length of the crafted batches: cold_povf_cap 160, cold_sus_cap 112
SE_ADD_SERVICE, SE_CLEAR_HOST, SE_DEPLOY_DECOY, SE_ADD_RED_SESSION, SE_SET_RED_ACTIVE = 1, 3, 4, 5, 9
K_SSHD, K_OT, K_SESS_RED, K_SHELL, K_PLAIN, K_DEC_VSFTPD = 0, 1, 11, 12, 13, 8            # process kinds (csrc/cc4_state.h)
RS_ABSTRACT, RS_ROOT, RS_ORIG, RS_CHILD = 1, 2, 4, 8
PB_22, PB_HAS = 1, 128
RA_EXPLOIT, XG_LOCAL, XF_RATE1, XF_SKIP_VALID = 4, 1, 2, 4
BA_MONITOR, BA_DECOY, BLUE_RAW_ACTION = 1, 5, 0x10000
RED_SUBNETS = [[4], [0], [1], [2], [3], [5, 6, 7]]            # allowed subnets of red agent r / blue agent b as subnet indices (host id = 17 * subnet + slot)
BLUE_SUBNETS = [[0], [1], [2], [3], [5, 6, 7]]
VARIANTS = ('m1', 'cap', 'over')
CONTAINERS = ('rs_add', 'rs_exploit', 'rs_reassign', 'pool0', 'pool1', 'pool2', 'pool3', 'pool_phish', 'known', 'known256',
              'proc_pin', 'proc_decoy_edit', 'proc_decoy', 'proc_exploit', 'proc_phish', 'sus0_end', 'sus4_end', 'sus0_monitor', 'sus4_monitor', 'pend')
SCENARIOS = tuple(f'{c}:{v}' for c in CONTAINERS for v in VARIANTS)


def caps(steps=STEPS):
    out = (ctypes.c_uint32 * 16)()
    load().cc4o_caps(int(steps), out)
    names = ('PIN', 'povf', 'sus', 'MAX_RS', 'RS_POOL', 'MAX_KS', 'MAX_OBS', 'MAX_PEND', 'povf_off', 'E_PROC', 'E_RSESS', 'E_KS', 'E_SUS', 'E_OBS',
             'E_PEND', 'cold_bytes')
    return dict(zip(names, (int(v) for v in out)))


def layout():
    buf = ctypes.create_string_buffer(8192)
    n = load().cc4o_layout(buf, 8192)
    return {k: int(v) for k, v in (ln.split() for ln in buf.raw[:n].decode().splitlines())}


class Built:
    """What build() did: the scenario, the flag its 'over' variant raises, the operation's parts and the list model of the adds performed."""
    def __init__(self, scenario):
        self.scenario = scenario
        self.container, self.variant = scenario.split(':')
        self.flag = 0                       # the E_* bit the operation raises in the 'over' variant
        self.edits = []                     # (op, a0, a1, a2, rc the engine must return)
        self.red, self.green, self.blue = [], [], None       # first-step submissions: (agent, type, host, session), (agent, type, host, rate1), [5]
        self.generated = {}                 # host -> length of its process list before the crafting
        self.sessions, self.procs = {}, {}  # list model: agent -> [(ident, host, index of its process in the host's list, flags)], host -> [[pid | None, kind, root]]
        self.watch = {}                     # what the operation must leave as it is when it is refused: ('sess', r) / ('proc', h) / ('known', r) / ('sus', b) / ('pend',)

    @property
    def needs_ext(self):
        return bool(self.red or self.green)

    @property
    def expect(self):
        return self.flag if self.variant == 'over' else 0


class _Ep:
    """One oracle episode being crafted: edits with the list model kept beside them, and pokes into its rows."""
    def __init__(self, ora, e, built):
        self.ora, self.e, self.b = ora, e, built
        self.ts = json.loads(ora.true_state_json(e))
        self.hosts = sorted(h['h'] for h in self.ts['hosts'])
        for h in self.ts['hosts']:
            built.procs[h['h']] = [[p[0], p[1], p[2] & 1] for p in h['procs']]
            built.generated[h['h']] = len(h['procs'])
        for r in range(6):
            built.sessions[r] = []
            for ident, host, pid, flags in self.ts['red'][r]['sessions']:
                built.sessions[r].append((ident, host, [p[0] for p in built.procs[host]].index(pid), flags))
        self.snap = None

    # ---- topology
    def zone(self, subnets, servers=None):
        return [h for h in self.hosts if h // 17 in subnets and h % 17 != 0 and h != 136 and (servers is None or (h % 17 >= 11) == servers)]

    def with_kind(self, hosts, kind):
        return [h for h in hosts if any(p[1] == kind for p in self.b.procs[h])]

    # ---- edits, mirrored in the list model
    def add_session(self, r, host, root=False, abstract=True, child=False):
        assert self.snap is None, 'an edit between a poke and its commit would be undone'
        ids = [s[0] for s in self.b.sessions[r]]
        want = max(ids) + 1 if ids else 0                                   # State.add_session: max + 1
        rc = self.ora.edit_state(self.e, SE_ADD_RED_SESSION, r, host, (1 if root else 0) | (2 if child else 0) | (4 if abstract else 0))
        assert rc == want, (self.b.scenario, r, host, rc, want)
        self.b.procs[host].append([None, K_SESS_RED if abstract else K_SHELL, int(root)])
        self.b.sessions[r].append((rc, host, len(self.b.procs[host]) - 1,
                                   (RS_ABSTRACT if abstract else 0) | (RS_ROOT if root else 0) | (RS_CHILD if child else 0)))
        return rc

    def fill_agent(self, r, total, hosts=None, salt=0):
        hosts = hosts or self.zone(RED_SUBNETS[r])
        j = salt
        while len(self.b.sessions[r]) < total:
            self.add_session(r, hosts[j % len(hosts)], root=(j % 4 == 1), abstract=(j % 3 != 0), child=(j % 5 == 2))
            j += 1
        # (no SE_SET_RED_ACTIVE: the first step's end activates an agent that holds sessions and lists them to it, as the controller does -- an FSM agent
        # switched on by hand would be asked for an action before it has seen a host: E_FSM_NO_HOST)

    def add_proc(self, host, decoy):
        assert self.snap is None, 'an edit between a poke and its commit would be undone'
        if decoy:
            assert self.ora.edit_state(self.e, SE_DEPLOY_DECOY, host, K_DEC_VSFTPD, 0) == 1
            self.b.procs[host].append([None, K_DEC_VSFTPD, 0])
        else:
            root = len(self.b.procs[host]) % 2
            pid = self.ora.edit_state(self.e, SE_ADD_SERVICE, host, K_OT, root)
            self.b.procs[host].append([pid, K_PLAIN, root])

    def fill_host(self, host, total):
        while len(self.b.procs[host]) < total:
            self.add_proc(host, decoy=(len(self.b.procs[host]) % 3 != 0))

    # ---- pokes
    def open(self):
        if self.snap is None:
            hot, cold = self.ora.snapshot(self.e)
            self.snap = [hot.copy(), cold.copy()]
        return self.snap

    def commit(self):
        if self.snap is not None:
            self.ora.restore(self.e, tuple(self.snap))
            self.snap = None

    def put(self, which, off, dtype, value):
        row = self.open()[which]
        row[off:off + np.dtype(dtype).itemsize].view(dtype)[0] = value

    def get(self, which, off, dtype):
        row = self.open()[which]
        return int(row[off:off + np.dtype(dtype).itemsize].view(dtype)[0])


L, _C = None, {}


def _layout():
    global L
    if L is None:
        L = layout()
    return L


def _caps(steps):
    if steps not in _C:
        _C[steps] = caps(steps)
    return _C[steps]


def _red_off(r, field):
    return _layout()['red'] + r * _layout()['sizeof.RedAgent'] + _layout()['red.' + field]


def _blue_off(b, field):
    return _layout()['blue'] + b * _layout()['sizeof.BlueAgent'] + _layout()['blue.' + field]


def _slot_of(ep, r, idx):
    return ep.get(0, _red_off(r, 'sord') + idx, np.uint8)


def _ssh_exploit(ep, r, targets):
    """A submitted ExploitRemoteService of agent r that succeeds whatever the draws: from its last abstract session, which is made to know port 22
    (and nothing else: SSHBruteForce is then the only option) of a target that runs sshd.  Returns the target."""
    cp = _caps(ep.ora.steps)
    idx = max(i for i, s in enumerate(ep.b.sessions[r]) if s[3] & RS_ABSTRACT)
    tgt = ep.with_kind(targets, K_SSHD)[-1]
    slot = _slot_of(ep, r, idx)
    row = (_layout()['cold.xrate'] - _layout()['cold.kports']) // cp['RS_POOL']
    ep.put(1, _layout()['cold.kports'] + slot * row + tgt, np.uint8, PB_HAS | PB_22)
    ep.b.red.append((r, RA_EXPLOIT, tgt, ep.b.sessions[r][idx][0]))
    return tgt


def _phish(ep, host_ok):
    """A submitted GreenLocalWork with phishing_error_rate 1 of a green agent on a host without red sessions that host_ok accepts.  Returns the host."""
    red_hosts = {s[1] for r in range(6) for s in ep.b.sessions[r]}
    for g, h in enumerate(ep.ts['green_hosts'][:ep.ts['n_green']]):
        if h not in red_hosts and host_ok(h):
            ep.b.green.append((g, XG_LOCAL, h, 1.0))
            return h
    raise AssertionError('no green host fits ' + ep.b.scenario)


def _fill_pool(ep, free, avoid=()):
    """Every agent gets sessions in its own zone until `free` records of the pool are left, none above MAX_RS."""
    cp = _caps(ep.ora.steps)
    want = cp['RS_POOL'] - free
    per = [cp['RS_POOL'] // 6] * 6
    k = 5
    while sum(per) > want:
        per[k] -= 1
        k = (k - 1) % 6
    for r in range(6):
        assert len(ep.b.sessions[r]) <= per[r] <= cp['MAX_RS']
        ep.fill_agent(r, per[r], hosts=[h for h in ep.zone(RED_SUBNETS[r]) if h not in avoid], salt=r)
    assert sum(len(ep.b.sessions[r]) for r in range(6)) == want


def _poke_sus(ep, b, count):
    """blue agent b's list of suspicious pids at `count` entries: pids no process carries, on hosts of its zone."""
    cp = _caps(ep.ora.steps)
    hosts = ep.zone(BLUE_SUBNETS[b])
    n0 = ep.get(0, _blue_off(b, 'nsus'), np.uint16)
    assert n0 == 0
    for k in range(count):
        h = hosts[k % len(hosts)]
        ep.put(1, _layout()['cold.sus'] + 4 * (b * cp['sus'] + k), np.uint32, (h << 16) | (60001 + k))
        w = _blue_off(b, 'sus_hosts') + 4 * (h >> 5)
        ep.put(0, w, np.uint32, ep.get(0, w, np.uint32) | (1 << (h & 31)))
    ep.put(0, _blue_off(b, 'nsus'), np.uint16, count)


def _poke_pend(ep, entries):
    for k, (h, pid) in enumerate(entries):
        ep.put(0, _layout()['pend'] + 4 * k, np.uint32, (h << 16) | pid)
    ep.put(0, _layout()['npend'], np.uint8, len(entries))


def build(ora, e, scenario):
    """Crafts episode e of `ora` (freshly reset, the FSM red agents and the green agents of the default configuration) for `scenario`."""
    cp = _caps(ora.steps)
    b = Built(scenario)
    ep = _Ep(ora, e, b)
    c, v = b.container, b.variant
    assert c in CONTAINERS and v in VARIANTS, scenario
    level = {'m1': -1, 'cap': 0, 'over': 0}[v]
    op = v != 'cap'
    full_host = cp['PIN'] + cp['povf']

    if c in ('rs_add', 'rs_exploit', 'rs_reassign'):
        b.flag = cp['E_RSESS']
        r = 1
        zone = ep.zone(RED_SUBNETS[r])
        b.watch = {('sess', r): None}
        if c == 'rs_reassign':                 # the operation is part of the crafted state: a foreign session the step's reassignment moves
            ep.fill_agent(r, cp['MAX_RS'] + level)
            if op:
                ep.add_session(0, zone[2], root=True, abstract=False)        # red_agent_0 on a host of red_agent_1's zone
        else:
            ep.fill_agent(r, cp['MAX_RS'] + level)
            if op and c == 'rs_add':
                b.edits.append((SE_ADD_RED_SESSION, r, zone[1], 1 | 4, max(s_[0] for s_ in b.sessions[r]) + 1 if v == 'm1' else -1))
            elif op:
                _ssh_exploit(ep, r, zone)
    elif c.startswith('pool'):
        b.flag = cp['E_RSESS']
        if c == 'pool_phish':                  # the phishing session takes the last record / finds none
            gh = ep.ts['green_hosts'][0]       # kept free of red sessions: PhishingEmail needs such a host
            _fill_pool(ep, 1 if v == 'm1' else 0, avoid=(gh,))
            if op:
                assert _phish(ep, lambda h: h == gh) == gh
        else:                                  # k free records and k exploiting agents ('cap'), k + 1 agents ('over'); k + 1 of both ('m1')
            k = int(c[4:])
            _fill_pool(ep, k + (1 if v == 'm1' else 0))
            for r in range(k + (1 if op else 0)):
                _ssh_exploit(ep, r + 1, ep.zone(RED_SUBNETS[r + 1]))
    elif c in ('known', 'known256'):
        b.flag = cp['E_KS']
        r = 2
        zone = ep.zone(RED_SUBNETS[r])
        b.watch = {('known', r): None}
        ep.fill_agent(r, 5)
        if c == 'known256':                    # the newest session's id past the bitmap: sid_known scans the list for it and for the next one
            ep.put(0, _layout()['spool'] + _slot_of(ep, r, 4) * _layout()['sizeof.RSess'] + _layout()['rsess.id'], np.uint16, 300)
            ident, host, pi, flags = b.sessions[r][4]
            b.sessions[r][4] = (300, host, pi, flags)
        # the ActionSpace keeps the ids of sessions long gone: ids 0 .. n-1 known, the list one short of / at its capacity
        n = cp['MAX_KS'] + level
        ids = list(range(n - 1)) + [300] if c == 'known256' else list(range(n))
        for k, ident in enumerate(ids):
            ep.put(1, _layout()['cold.known_sid'] + 2 * (r * cp['MAX_KS'] + k), np.uint16, ident)
            if ident < 256:
                w = _red_off(r, 'known_bm') + 4 * (ident >> 5)
                ep.put(0, w, np.uint32, ep.get(0, w, np.uint32) | (1 << (ident & 31)))
        ep.put(0, _red_off(r, 'nknown'), np.uint8, n)
        ep.commit()
        if op:                                 # a new abstract session (ident max + 1: new to the ActionSpace) that the step's RedSessionCheck lists
            if c == 'known':                   # ... with an ident no known id has: past the ids poked above
                for _ in range(3):
                    ep.add_session(r, zone[0], abstract=False)
                ep.put(0, _layout()['spool'] + _slot_of(ep, r, len(b.sessions[r]) - 1) * _layout()['sizeof.RSess'] + _layout()['rsess.id'], np.uint16, 200)
                ident, host, pi, flags = b.sessions[r][-1]
                b.sessions[r][-1] = (200, host, pi, flags)
                ep.commit()
            ep.add_session(r, zone[1], root=True, abstract=True)
    elif c.startswith('proc'):
        b.flag = cp['E_PROC']
        if c == 'proc_pin':                    # the boundary between the inline and the overflow part: PIN - 1, PIN, PIN + 1 -- all clean
            b.flag = 0
            for h in ep.zone([0, 1, 2, 3]):
                ep.fill_host(h, cp['PIN'] + {'m1': -1, 'cap': 0, 'over': 1}[v])
        elif c == 'proc_decoy_edit':
            h = ep.hosts[-2] if ep.hosts[-1] == 136 else ep.hosts[-1]          # the highest-numbered host of a subnet
            for hh in (h, 136):                                               # ... and the internet host: its overflow row closes the cold row
                ep.fill_host(hh, full_host + level)
                b.watch[('proc', hh)] = None
                if op:
                    b.edits.append((SE_DEPLOY_DECOY, hh, K_DEC_VSFTPD, 0, 1 if v == 'm1' else -1))
        elif c == 'proc_decoy':                # DeployDecoy of blue agents 0 and 4 on full hosts (4: the highest-numbered host a blue agent defends)
            b.blue = [-1] * 5
            for bl in (0, 4):
                h = ep.zone(BLUE_SUBNETS[bl])[-1]
                ep.fill_host(h, full_host + level)
                b.watch[('proc', h)] = None
                if op:
                    b.blue[bl] = BLUE_RAW_ACTION | (BA_DECOY << 8) | h | (1 << 20)      # duration 1: executed in the step it is submitted in
        elif c == 'proc_exploit':              # the shell of a successful exploit
            r = 3
            ep.fill_agent(r, 6)
            tgt = ep.with_kind(ep.zone(RED_SUBNETS[r]), K_SSHD)[-1]
            ep.fill_host(tgt, full_host + level)
            b.watch[('proc', tgt)] = None
            if op:
                assert _ssh_exploit(ep, r, [tgt]) == tgt
        else:                                  # proc_phish: the process of a phishing session
            ep.fill_agent(0, 3)
            greens = set(ep.ts['green_hosts'][:ep.ts['n_green']])
            reds = {s[1] for r in range(6) for s in b.sessions[r]}
            h = sorted(greens - reds)[-1]
            ep.fill_host(h, full_host + level)
            b.watch[('proc', h)] = None
            if op:
                assert _phish(ep, lambda g: g == h) == h
    elif c.startswith('sus'):
        b.flag = cp['E_SUS']
        bl = int(c[3])
        zone = ep.zone(BLUE_SUBNETS[bl])
        b.watch = {('sus', bl): None}
        _poke_sus(ep, bl, cp['sus'] + level)
        if op:                                 # one pid-carrying process_creation event of the zone waits for the agent
            _poke_pend(ep, [(zone[1], 60000)])
            if c.endswith('monitor'):          # ... and the agent's own Monitor action takes it (otherwise the end of the step does)
                b.blue = [-1] * 5
                b.blue[bl] = BLUE_RAW_ACTION | (BA_MONITOR << 8)
    elif c == 'pend':                          # MAX_PEND - 1 / MAX_PEND events wait (hosts no blue agent defends: they stay through Monitor actions)
        b.flag = cp['E_PEND']
        b.watch = {('pend',): None}
        con = ep.zone([4])
        if op:
            ep.fill_agent(1, 4)
        _poke_pend(ep, [(con[k % len(con)], 61000 + k) for k in range(cp['MAX_PEND'] + level)])
        if op:
            _ssh_exploit(ep, 1, ep.zone(RED_SUBNETS[1]))
    ep.commit()
    return b


def submissions(env, built_by_episode):
    """The record arrays and the blue rows of the first step: red / green for step_ex (None when no episode submits any), blue [n, 5] raw actions
    (-1: none, -2: not a crafted episode) to be laid over the step's blue actions with first_step_actions()."""
    n = env.num_envs
    red, green = env.agent_actions('red'), env.agent_actions('green')
    blue = np.full((n, 5), -2, np.int32)          # -2: not a crafted episode, the caller's own action stands
    any_ext = False
    for e, b in built_by_episode.items():
        for r, t, host, sid in b.red:
            rec = red[e, r]
            rec['type'] = t; rec['host'] = host; rec['session'] = sid; rec['ticks'] = 1; rec['flags'] = XF_SKIP_VALID
            any_ext = True
        for g, t, host, rate1 in b.green:
            rec = green[e, g]
            rec['type'] = t; rec['host'] = host; rec['flags'] = XF_RATE1 | XF_SKIP_VALID; rec['rate1'] = rate1
            any_ext = True
        blue[e] = b.blue if b.blue is not None else -1          # a crafted episode's first step: its operation and nothing else
    return (red, green) if any_ext else (None, None), blue


def apply_edits(env, e, built, lib_call=None):
    """The operation's edits on episode e of any handle; returns the values the engine gave (-1: refused).  OracleVecEnv and CC4VecEnv raise for a
    negative value: the call goes to the library itself."""
    out = []
    for op, a0, a1, a2, _want in built.edits:
        if hasattr(env.lib, 'cc4o_edit_state'):
            env.lib.cc4o_edit_state.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5
            out.append(int(env.lib.cc4o_edit_state(env._h, int(e), op, a0, a1, a2)))
        else:
            out.append(int(env.lib.cc4_edit_state(env._h, int(e), op, a0, a1, a2)))
    return out


def listed(ts, built, hot=None):
    """The content of the containers `built.watch` names, from a true-state document / the rows: what an overflowing operation must leave as it is."""
    out = {}
    for key in built.watch:
        if key[0] == 'sess':
            out[key] = [tuple(s) for s in ts['red'][key[1]]['sessions']]
        elif key[0] == 'proc':
            out[key] = [tuple(p) for h in ts['hosts'] if h['h'] == key[1] for p in h['procs']]
        elif key[0] == 'known':
            out[key] = list(ts['red'][key[1]]['known_sessions'])
        elif key[0] == 'sus':
            out[key] = [tuple(s) if isinstance(s, list) else s for s in ts['blue'][key[1]]['sus']]
        elif key[0] == 'pend' and hot is not None:
            n = int(hot[_layout()['npend']])
            out[key] = hot[_layout()['pend']:_layout()['pend'] + 4 * n].view(np.uint32).tolist()
    return out


def check_model(ts, built):
    """The session and process lists of the true-state document against the list model of the adds: idents max + 1, pids as returned (one more
    than the list's largest plus a draw below 9 where the op does not return it), insertion order."""
    hosts = {h['h']: h['procs'] for h in ts['hosts']}
    for h, model in built.procs.items():
        got = hosts[h]
        assert len(got) == len(model), (built.scenario, 'host', h, len(got), len(model))
        mx = 0
        for k, ((pid, kind, flags), (mpid, mkind, mroot)) in enumerate(zip(got, model)):
            assert kind == mkind and (flags & 1) == mroot, (built.scenario, 'host', h, k, (pid, kind, flags), (mpid, mkind, mroot))
            if mpid is not None:
                assert pid == mpid, (built.scenario, 'host', h, k, pid, mpid)
            if k >= built.generated[h]:
                assert mx < pid <= mx + 9, (built.scenario, 'host', h, k, pid, mx)
            mx = max(mx, pid)
    for r, model in built.sessions.items():
        got = ts['red'][r]['sessions']
        want = [(ident, host, hosts[host][pi][0], flags) for ident, host, pi, flags in model]
        assert [(s[0], s[1], s[2], s[3] & ~RS_ORIG) for s in got] == [(a, b_, c_, f & ~RS_ORIG) for a, b_, c_, f in want], (built.scenario, 'red', r, got[-3:], want[-3:])


def first_step_actions(actions, blue):
    """The blue actions of the first step: the crafted episodes' own rows (submissions()) over the caller's."""
    return np.where(blue > -2, blue, actions).astype(np.int32)


def live_cold(hot, cold, steps, rng_mode):
    """The live extents of a cold row (cold_live_span, csrc/cc4_state.h: what a device copy of an episode moves) as one byte string: the backup
    images, the tail of the fixed part (xrate .. rng2, with known_sid), the ephemeral-port maps in the numpy-stream mode, the port rows of the pool
    records in use, sus[b][0, nsus) and povf[h][0, nproc - PIN)."""
    cp, lay = _caps(steps), _layout()
    hot, cold = np.asarray(hot, np.uint8), np.asarray(cold, np.uint8)
    parts = [cold[:lay['cold.eph']], cold[lay['cold.xrate']:lay['sizeof.EnvCold']]]
    if rng_mode == 0:
        parts.append(cold[lay['cold.eph']:lay['cold.evlog']])
    row = (lay['cold.xrate'] - lay['cold.kports']) // cp['RS_POOL']
    used = np.unpackbits(hot[lay['spool_used']:lay['spool_used'] + cp['RS_POOL'] // 8], bitorder='little')
    for slot in np.nonzero(used)[0]:
        parts.append(cold[lay['cold.kports'] + slot * row:lay['cold.kports'] + (slot + 1) * row])
    for b in range(5):
        nsus = int(hot[_blue_off(b, 'nsus'):_blue_off(b, 'nsus') + 2].view(np.uint16)[0])
        parts.append(cold[lay['cold.sus'] + 4 * b * cp['sus']:lay['cold.sus'] + 4 * (b * cp['sus'] + min(nsus, cp['sus']))])
    nhosts = (lay['sizeof.EnvState'] - lay['hd']) // lay['sizeof.HostDyn']
    for h in range(nhosts):
        o = lay['hd'] + h * lay['sizeof.HostDyn'] + lay['hd.nproc']
        extra = max(0, int(hot[o:o + 2].view(np.uint16)[0]) - cp['PIN'])
        parts.append(cold[cp['povf_off'] + 4 * h * cp['povf']:cp['povf_off'] + 4 * (h * cp['povf'] + min(extra, cp['povf']))])
    return np.concatenate(parts).tobytes()
