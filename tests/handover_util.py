"""Cells of the plan-kernel hand-over tests (tests/test_plan_handover_cpu.py, tests/test_plan_handover.py).

A cell is one call of a persistent kernel on a fresh handle -- (batch, generator mode, episode length, earlier plan calls, the call under test, schedule
knobs) -- with every seed fixed, so its true trajectory is a constant: oracle_trajectory() steps the CPU oracle through it once, and the device may be asked
for it as often as one likes.  `base` is the call tests/test_plan.py's self-check child ends with, the one call that has been seen disagreeing; every other
cell differs from it in ONE factor (k62 in two: CELLS says which).  describe() says how the call is cut into runs (cc4_sched.h's run_split, through the oracle library) and where its
regenerations fall in them; check_premise() asserts that the cell still isolates what it claims to; locate() turns a mismatch's (episode, step) into
(run, position in the run, regeneration?, partition).

A regeneration: with autoreset a step call whose episode ended with the call before re-creates the episode instead of stepping it.  Where these fall is
read off the oracle's `done` rows, never computed here."""
import collections
import ctypes

import numpy as np

from oracle_binding import OracleVecEnv, load, random_actions
from plan_util import random_plan

PARTITIONS = 256            # the persistent schedule runs with one partition per compute unit or not at all (persist_setup); an MI355X has 256
OBS, OBS_PACKED = 578, 148  # values of an observation row; bytes of its packed form (2 bits a value, low bits first, the bits past value 577 zero)
RESET_SEED = 12             # as the self-check child: reset(seeds=12), plans from default_rng(batch size)
RANDOM_SEED0, RANDOM_T0 = 77, 5          # the stand-in policy's key and first action time of a `random` call
COLD_STRIDE = 256           # the cold rows compared: every 256th episode, and the last

Plan = collections.namedtuple('Plan', 'k msgs record')         # a plan call of k steps, with messages or without, recording the observations or not
Random = collections.namedtuple('Random', 'k')                  # cc4_run_random_steps of k steps
Cell = collections.namedtuple('Cell', 'id n rng_mode steps prefix call knobs R')

CHILD_CALLS = (Plan(12, True, True), Plan(45, False, False), Plan(10, False, True), Plan(70, True, True))   # test_plan._VERIFY_CHILD's (k, rec, m) rows


def _cell(id_, R, n=8192, rng_mode=1, steps=40, prefix=CHILD_CALLS[:3], call=CHILD_CALLS[3], **knobs):
    return Cell(id_, n, rng_mode, steps, tuple(prefix), call, tuple(sorted(knobs.items())), R)


def _prefix(second):
    return (CHILD_CALLS[0], CHILD_CALLS[1]._replace(k=second), CHILD_CALLS[2])


# R: repetitions of the GPU test (8 each: the count that was run and timed on an MI355X, 0.7 - 3.1 s a test; DESIGN 3.4b has the times and what a larger R would cost).
# Cells that share a trajectory (they differ in schedule knobs or in what is recorded) stand next to each other: the oracle steps it once for them.
CELLS = collections.OrderedDict((c.id, c) for c in (
    _cell('base', 8),
    _cell('no_record', 8, call=Plan(70, True, False)),
    _cell('steal_all', 8, CC4_PERSIST_THR='0'),
    _cell('steal_late', 8, CC4_PERSIST_THR='1000000'),      # (a partition hands out 448 tickets in this call: never that far ahead)
    _cell('every_step_a_run', 8, CC4_PERSIST_RUNS='1,1,0,0'),
    _cell('no_msgs', 8, call=Plan(70, False, True)),
    _cell('no_regen', 8, steps=1000),
    _cell('regen_first', 8, prefix=_prefix(41)),
    _cell('regen_last', 8, prefix=_prefix(42)),
    _cell('k64', 8, call=Plan(64, True, True)),
    _cell('k62', 8, call=Plan(62, True, True)),             # (two factors: runs of 4, and its regenerations fall on a run's first step)
    _cell('random_steps', 8, call=Random(70)),
    _cell('pcg', 8, n=6656, rng_mode=0),
))


def kernel_name(cell):
    """The persistent kernel the call under test is to take."""
    plan = isinstance(cell.call, Plan)
    if cell.rng_mode == 0:
        return 'k_run_pcgp' if plan else 'k_run_pcg'
    return 'k_run_philox1p' if plan else 'k_run_philox1'


def pack_obs(obs):
    """[n, 578] observation values -> [n, 148] packed bytes, as the kernels pack them (cc4_kernels.h pack_row_from_obs)."""
    obs = np.asarray(obs)
    assert obs.ndim == 2 and obs.shape[1] == OBS and not (obs >> 2).any(), 'an observation value outside 0 .. 3'
    u = obs.astype(np.uint8)
    out = np.zeros((obs.shape[0], OBS_PACKED), np.uint8)
    q = u[:, :OBS - OBS % 4].reshape(obs.shape[0], OBS // 4, 4)
    out[:, :OBS // 4] = q[:, :, 0] | (q[:, :, 1] << 2) | (q[:, :, 2] << 4) | (q[:, :, 3] << 6)
    for i in range(OBS % 4):
        out[:, OBS // 4] |= u[:, OBS - OBS % 4 + i] << (2 * i)
    return out


def unpack_obs(packed):
    """[..., 148] packed bytes -> [..., 578] uint8 values."""
    packed = np.asarray(packed, np.uint8)
    v = (packed[..., None] >> np.array([0, 2, 4, 6], np.uint8)) & np.uint8(3)
    return v.reshape(packed.shape[:-1] + (4 * OBS_PACKED,))[..., :OBS]


def cell_inputs(cell, n=None):
    """The inputs of the cell's calls, in order: (call, actions [k, n, 5], messages [k, n, 5, 8] or None) -- plans drawn as the child draws them, one
    generator seeded with the cell's batch size for the prefix and the call; a `random` call's actions are the stand-in policy's draws."""
    n = cell.n if n is None else n
    rng = np.random.default_rng(cell.n)
    out = []
    for c in cell.prefix + (cell.call,):
        if isinstance(c, Plan):
            out.append((c,) + random_plan(rng, c.k, n, c.msgs))
        else:
            out.append((c, np.stack([random_actions(RANDOM_SEED0, RANDOM_T0 + j, n) for j in range(c.k)]), None))
    return out


class Trajectory:
    """What the oracle says of the call under test.  obs_packed [K, n, 148] uint8 (obs: the same unpacked, [K, n, 578] uint8), rewards [K, n] float32,
    dones [K, n] bool, regen [K, n] bool (step j re-created episode e), err [n] (every flag a step of the call raised), obs_last / reward_last / done_last /
    err_last (the outputs after the last step), hot [n, state bytes], cold {episode: row}, rng [n, 7]; inputs: cell_inputs() of the same batch."""
    @property
    def obs(self):
        return unpack_obs(self.obs_packed)


_TRAJ = collections.OrderedDict()          # the last two trajectories (a full-batch one is ~300 MB)


def oracle_trajectory(cell, n=None):
    """The cell's true trajectory at n episodes (default: the cell's batch).  Cells whose inputs are the same share one Trajectory; nobody writes to it."""
    n = cell.n if n is None else n
    key = (n, cell.n, cell.rng_mode, cell.steps, tuple(c._replace(record=False) if isinstance(c, Plan) else c for c in cell.prefix + (cell.call,)))
    if key in _TRAJ:
        _TRAJ.move_to_end(key)
        return _TRAJ[key]
    ora = OracleVecEnv(n, steps=cell.steps, rng_mode=cell.rng_mode, autoreset=True)
    ora.reset_batch(RESET_SEED)
    t = Trajectory()
    t.inputs = cell_inputs(cell, n)
    for c, act, msg in t.inputs[:-1]:
        for j in range(c.k):
            ora.step_batch(act[j], None if msg is None else msg[j])
    c, act, msg = t.inputs[-1]
    t.obs_packed = np.zeros((c.k, n, OBS_PACKED), np.uint8)
    t.rewards, t.dones, t.regen = np.zeros((c.k, n), np.float32), np.zeros((c.k, n), bool), np.zeros((c.k, n), bool)
    t.err = np.zeros(n, np.uint32)
    for j in range(c.k):
        t.regen[j] = ora._done                  # the episode ended with the step call before this one: this call re-creates it
        o, r, d, info = ora.step_batch(act[j], None if msg is None else msg[j])
        t.obs_packed[j], t.rewards[j], t.dones[j] = pack_obs(o), r, d
        t.err |= info['err']
    t.obs_last, t.reward_last, t.done_last, t.err_last = o.copy(), r.copy(), d.copy(), info['err'].copy()
    t.hot = np.stack([ora.get_state(e) for e in range(n)])
    t.cold = {e: ora.get_cold(e) for e in sorted(set(range(0, n, COLD_STRIDE)) | {n - 1})}
    t.rng = ora.rng_state()
    ora.close()
    for a in (t.obs_packed, t.rewards, t.dones, t.regen, t.err, t.obs_last, t.reward_last, t.done_last, t.err_last, t.hot, t.rng) + tuple(t.cold.values()):
        a.setflags(write=False)
    _TRAJ[key] = t
    while len(_TRAJ) > 2:
        _TRAJ.popitem(last=False)
    return t


def run_config(cell):
    """CC4_PERSIST_RUNS as persist_setup reads it ("SA,SB,nB,single"; unset: 0,1,0,0)."""
    q = [0, 1, 0, 0]
    v = dict(cell.knobs).get('CC4_PERSIST_RUNS')
    if v is not None:
        for i, s in enumerate(v.split(',')[:4]):
            q[i] = int(s)
    return max(q[0], 0), max(q[1], 1), max(q[2], 0), max(q[3], 0)


Description = collections.namedtuple('Description', 'pattern runs regens')


def describe(cell, traj):
    """How the call under test is cut into runs, and where its regenerations fall.  pattern (SA, nA, SB, nB, singles); runs [(first step, length)];
    regens [(step, run, q, run length)] -- the steps that re-create an episode (any episode of traj; check_premise asserts they are every episode's)."""
    lib = load()
    K = cell.call.k
    i32 = ctypes.POINTER(ctypes.c_int32)
    split, k0, ln = np.zeros(5, np.int32), np.zeros(K, np.int32), np.zeros(K, np.int32)
    nph = lib.cc4o_sched_runs(K, *run_config(cell), 0, K, split.ctypes.data_as(i32), k0.ctypes.data_as(i32), ln.ctypes.data_as(i32))
    SA, nA, SB, nB = (int(v) for v in split[:4])
    runs = [(int(k0[r]), int(ln[r])) for r in range(nph)]
    regens = []
    for j in np.nonzero(traj.regen.any(axis=1))[0]:
        r, q = run_of(runs, int(j))
        regens.append((int(j), r, q, runs[r][1]))
    return Description((SA, nA, SB, nB, nph - nA - nB), runs, regens)


def run_of(runs, j):
    """(run, position in it) of step j of the call."""
    for r, (k0, ln) in enumerate(runs):
        if k0 <= j < k0 + ln:
            return r, j - k0
    raise ValueError(f'step {j} is in no run of {runs}')


def check_premise(cell, traj):
    """What the cell claims to isolate, asserted on the oracle's trajectory (at any batch size); returns its Description."""
    d = describe(cell, traj)
    SA, nA, SB, nB, singles = d.pattern
    K = cell.call.k
    where = f'{cell.id}: pattern {d.pattern}, regenerations (step, run, q, run length) {d.regens}'
    assert sum(ln for _, ln in d.runs) == K and all(k0 == sum(ln for _, ln in d.runs[:r]) for r, (k0, _) in enumerate(d.runs)), where
    assert (traj.regen == traj.regen[:, :1]).all(), f'{cell.id}: the episodes regenerate at different steps'
    assert not traj.err.any() and not traj.err_last.any(), f'{cell.id}: the oracle raises error flags'
    assert isinstance(cell.call, Random if cell.id == 'random_steps' else Plan), where
    assert (cell.rng_mode, cell.n) == ((0, 6656) if cell.id == 'pcg' else (1, 8192)), where
    assert all(c.k >= 10 for c in cell.prefix), where                   # (persist_min_k: every earlier call is a persistent one too)
    mid_run = [g for g in d.regens if g[3] == SA and 0 < g[2] < SA - 1]
    if cell.id == 'every_step_a_run':
        assert len(d.runs) == K and all(ln == 1 for _, ln in d.runs) and d.regens, where
    elif cell.id == 'k62':
        assert SA == 4 and nA >= 1 and nB == 0 and d.regens, where           # runs of 4 (its regenerations fall on a run's first step: DESIGN 3.4b says so)
    else:
        assert SA == 8 and nA >= 1 and nB == 0, where                        # runs of 8 ..
        assert (singles == 0) if cell.id == 'k64' else (singles >= 1), where      # .. then single steps (k64: none)
    if cell.id == 'no_regen':
        assert not d.regens, where
    elif cell.id == 'regen_first':
        assert d.regens and all(q == 0 for _, _, q, _ in d.regens) and any(ln == SA for _, _, _, ln in d.regens), where
    elif cell.id == 'regen_last':
        assert d.regens and all(q == ln - 1 for _, _, q, ln in d.regens) and any(ln == SA for _, _, _, ln in d.regens), where
    elif cell.id not in ('every_step_a_run', 'k62'):
        assert mid_run, where                                                # as the failing call: a regeneration strictly inside a run of 8
    return d


Location = collections.namedtuple('Location', 'episode step run q run_length regeneration partition')


def locate(cell, traj, e, j, partitions=PARTITIONS):
    """Where step j of episode e of the call under test sits in the schedule: its run, its position q in the run, whether the step re-creates the episode,
    and the partition (the compute unit whose waves normally run the episode: cc4_sched.h part_of)."""
    runs = describe(cell, traj).runs
    r, q = run_of(runs, int(j))
    return Location(int(e), int(j), r, q, runs[r][1], bool(traj.regen[j, e]), int(e) % partitions)


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a          # rewards compare as bit patterns


def first_mismatch(cell, traj, obs_packed=None, rewards=None, dones=None, final=None):
    """Everything a repetition produced against the trajectory, exactly.  obs_packed / rewards / dones: the recorded rows of every step (None: not
    recorded); final: {name: (got, want)} of per-episode arrays at the call's end, or (got, want, episodes) for rows of some episodes only.  None, or a message that names the first differing step's Location, the
    kinds that differ there, how many episodes differ at that step, and the final arrays that differ."""
    step, kinds, eps = None, [], None
    for kind, got, want in (('observations', obs_packed, traj.obs_packed), ('rewards', rewards, traj.rewards), ('dones', dones, traj.dones)):
        if got is None:
            continue
        got, want = _bits(got), _bits(want)
        assert got.shape == want.shape and got.dtype == want.dtype, (kind, got.shape, got.dtype, want.shape, want.dtype)
        if np.array_equal(got, want):
            continue
        j = next(j for j in range(want.shape[0]) if not np.array_equal(got[j], want[j]))
        bad = (got[j] != want[j]).reshape(want.shape[1], -1).any(axis=1)
        if step is None or j < step:
            step, kinds, eps = j, [kind], bad
        elif j == step:
            kinds.append(kind)
            eps = eps | bad
    parts = []
    if step is not None:
        e = int(np.nonzero(eps)[0][0])
        parts.append(f'first differing step: {locate(cell, traj, e, step)} ({" ".join(kinds)}); {int(eps.sum())} episode(s) differ at that step')
    for name, pair in (final or {}).items():
        got, want = _bits(pair[0]), _bits(pair[1])
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype, want.shape, want.dtype)
        if not np.array_equal(got, want):
            bad = np.nonzero((got != want).reshape(want.shape[0], -1).any(axis=1))[0]
            if len(pair) > 2:
                bad = np.asarray(pair[2])[bad]
            parts.append(f'{name} at the call\'s end differ in {bad.size} episode(s), first {bad[:8].tolist()} (partitions {[int(b) % PARTITIONS for b in bad[:8]]})')
    return '; '.join(parts) if parts else None
