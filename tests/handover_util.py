"""Cells of the plan-kernel hand-over tests (tests/test_plan_handover_cpu.py, tests/test_plan_handover.py).

A cell is one call of a persistent kernel on a fresh handle -- (batch, generator mode, episode length, earlier plan calls, the call under test, schedule
knobs) -- with every seed fixed, so its true trajectory is a constant: oracle_trajectory() steps the CPU oracle through it once, and the device may be asked
for it as often as one likes.  `base` is the call tests/test_plan.py's self-check child ends with, the one call that has been seen disagreeing; every other
cell differs from it in ONE factor (k62 in two: CELLS says which).  describe() says how the call is cut into runs (cc4_sched.h's run_split, through the oracle library) and where its
regenerations fall in them; check_premise() asserts that the cell still isolates what it claims to; locate() turns a mismatch's (episode, step) into
(run, position in the run, regeneration?, partition).

Six cells repeat `base`, `pcg` and `random_steps` with something on the device BESIDE the call (Cell.beside: the self-check's shadow handle, or a second
handle's per-step launches); they share their twins' inputs and trajectory.  For them the second half of this file drives the device: PlanCall /
run_plan_raw (cc4_run_plan_device on buffers the helper owns, downloaded whatever the call returned), fetch_final (a handle's rows at the call's end, the
shadow's too: cc4_debug_shadow_handle), self_check_verdict / neighbour_verdict (which side left the trajectory) and StreamTimes / overlap_share.

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
# What runs on the device BESIDE the call under test (Cell.beside; None: nothing).  It is no knob of the schedule: the call is cut and handed out as without it.
SelfCheck = collections.namedtuple('SelfCheck', 'env value')    # the handle is created with this self-check setting: checked calls run a shadow handle's per-step launches beside the kernel
Neighbour = collections.namedtuple('Neighbour', 'order')        # a second handle B takes the same plan in the per-step form, enqueued 'after' or 'before' A's call with no host wait between
Cell = collections.namedtuple('Cell', 'id n rng_mode steps prefix call knobs R beside', defaults=(None,))

CHILD_CALLS = (Plan(12, True, True), Plan(45, False, False), Plan(10, False, True), Plan(70, True, True))   # test_plan._VERIFY_CHILD's (k, rec, m) rows


def _cell(id_, R, n=8192, rng_mode=1, steps=40, prefix=CHILD_CALLS[:3], call=CHILD_CALLS[3], beside=None, **knobs):
    return Cell(id_, n, rng_mode, steps, tuple(prefix), call, tuple(sorted(knobs.items())), R, beside)


def _prefix(second):
    return (CHILD_CALLS[0], CHILD_CALLS[1]._replace(k=second), CHILD_CALLS[2])


# R: repetitions of the GPU test (the counts that were run and timed on an MI355X, 0.7 - 3.2 s a test: 8 for the single-factor cells, 24 / 16 for the cells with
# something beside the kernel; DESIGN 3.4b has the times).
# Cells that share a trajectory (they differ in schedule knobs or in what is recorded) stand next to each other: the oracle steps it once for them.
CELLS = collections.OrderedDict((c.id, c) for c in (
    _cell('base', 8),
    _cell('no_record', 8, call=Plan(70, True, False)),
    _cell('steal_all', 8, CC4_PERSIST_THR='0'),
    _cell('steal_late', 8, CC4_PERSIST_THR='1000000'),      # (a partition hands out 448 tickets in this call: never that far ahead)
    _cell('every_step_a_run', 8, CC4_PERSIST_RUNS='1,1,0,0'),
    # `base` with something beside the kernel (R as run and timed on an MI355X: DESIGN 3.4b)
    _cell('selfcheck_all', 24, beside=SelfCheck('CC4_PERSIST_VERIFY', '1')),             # base exactly as it failed: all four calls checked
    _cell('selfcheck_last', 24, beside=SelfCheck('CC4_PERSIST_VERIFY_EVERY', '4')),      # only the 70-step call of each repetition is checked
    _cell('neighbour_after', 16, beside=Neighbour('after')),
    _cell('neighbour_before', 16, beside=Neighbour('before')),
    _cell('no_msgs', 8, call=Plan(70, False, True)),
    _cell('no_regen', 8, steps=1000),
    _cell('regen_first', 8, prefix=_prefix(41)),
    _cell('regen_last', 8, prefix=_prefix(42)),
    _cell('k64', 8, call=Plan(64, True, True)),
    _cell('k62', 8, call=Plan(62, True, True)),             # (two factors: runs of 4, and its regenerations fall on a run's first step)
    _cell('random_steps', 8, call=Random(70)),
    _cell('selfcheck_random', 24, call=Random(70), beside=SelfCheck('CC4_PERSIST_VERIFY', '1')),
    _cell('pcg', 8, n=6656, rng_mode=0),
    _cell('selfcheck_pcg', 24, n=6656, rng_mode=0, beside=SelfCheck('CC4_PERSIST_VERIFY', '1')),
))
BATCH = {1: 8192, 0: 6656}          # the batch of a generator mode's cells (counter mode / numpy stream): the self-check child's two handles


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
    # by the cell's fields, not its id (tests/test_plan_handover_cpu.py asserts which ids carry which): the entry point, the mode's batch, and at most one of
    # the two changed -- the numpy-stream cells are plan calls
    assert type(cell.call) in (Plan, Random) and all(type(c) is Plan for c in cell.prefix), where
    assert cell.n == BATCH.get(cell.rng_mode), where
    assert cell.rng_mode == 1 or type(cell.call) is Plan, where
    assert all(c.k >= 10 for c in cell.prefix) and K >= 10, where       # (persist_min_k: every earlier call is a persistent one too)
    b = cell.beside
    assert b is None or (type(b) in (SelfCheck, Neighbour) and not cell.knobs), where          # what runs beside the kernel is the one factor changed
    if type(b) is SelfCheck:
        # every call checked, or every (calls of a repetition)-th persistent call: the call under test and no other (the count runs on over the repetitions)
        assert b == SelfCheck('CC4_PERSIST_VERIFY', '1') or (b.env == 'CC4_PERSIST_VERIFY_EVERY' and int(b.value) == len(cell.prefix) + 1 >= 2), where
    elif type(b) is Neighbour:
        assert b.order in ('after', 'before') and type(cell.call) is Plan, where
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


# ---------------------------------------------------------------------------------------------------------------- the device side (GPU tests only)
# A call under the self-check that disagrees returns -5, and CC4VecEnv.run_plan raises for it before it downloads anything: the evidence is freed.  PlanCall
# makes the same cc4_run_plan_device call on buffers it owns, can leave the call in flight (the neighbour cells enqueue a second handle's call behind it), and
# downloads what the call produced whatever it returned.
PlanResult = collections.namedtuple('PlanResult', 'rc error rewards dones obs_packed')       # obs_packed: None unless recorded; error: cc4_last_error where rc != 0


def hip_runtime():
    """The HIP runtime the library is linked against (vec_env._hip), with the event calls the overlap measurement needs."""
    from cage_challenge_4_amd import vec_env
    hip = vec_env._hip()
    if not getattr(hip, '_handover_events', False):
        vp = ctypes.c_void_p
        hip.hipEventCreate.argtypes, hip.hipEventCreate.restype = [ctypes.POINTER(vp)], ctypes.c_int
        hip.hipEventRecord.argtypes, hip.hipEventRecord.restype = [vp, vp], ctypes.c_int
        hip.hipEventSynchronize.argtypes, hip.hipEventSynchronize.restype = [vp], ctypes.c_int
        hip.hipEventElapsedTime.argtypes, hip.hipEventElapsedTime.restype = [ctypes.POINTER(ctypes.c_float), vp, vp], ctypes.c_int
        hip.hipEventDestroy.argtypes, hip.hipEventDestroy.restype = [vp], ctypes.c_int
        hip._handover_events = True
    return hip


def _hip_ok(rc, what):
    if rc != 0:
        raise RuntimeError(f'{what} failed (hipError_t {rc})')


class PlanCall:
    """One cc4_run_plan_device call of `env` on device buffers this object owns: the plan is uploaded here, enqueue() makes the call and does not wait for
    it, finish() waits, downloads rewards, dones and packed rows WHATEVER the call returned, frees the buffers and returns a PlanResult."""
    def __init__(self, env, actions, messages=None, record_obs=False):
        from cage_challenge_4_amd import _lib as L
        self.env, self.hip, vp = env, hip_runtime(), ctypes.c_void_p
        actions = np.ascontiguousarray(actions, dtype=np.int32)
        self.k, self.n = k, n = int(actions.shape[0]), env.num_envs
        assert actions.shape == (k, n, L.NUM_BLUE) and k >= 1, actions.shape
        staged = [actions.reshape(-1).view(np.uint8)]
        if messages is not None:
            messages = np.ascontiguousarray(messages, dtype=np.uint8)
            assert messages.shape == (k, n, L.NUM_BLUE, L.MSG_LEN), messages.shape
            staged.append(messages.reshape(-1))
        staged = np.concatenate(staged)
        self.b_act, self.with_msgs = actions.nbytes, messages is not None
        self.b_rew, self.b_pk, self.b_done = 4 * k * n, (OBS_PACKED * k * n if record_obs else 0), k * n
        self.d_in, self.d_out, self.rc, self.error = vp(), vp(), None, None
        _hip_ok(self.hip.hipSetDevice(env._dev), 'hipSetDevice')
        _hip_ok(self.hip.hipMalloc(ctypes.byref(self.d_in), staged.nbytes), 'hipMalloc')
        try:
            _hip_ok(self.hip.hipMalloc(ctypes.byref(self.d_out), self.b_rew + self.b_pk + self.b_done), 'hipMalloc')
            _hip_ok(self.hip.hipMemcpy(self.d_in, staged.ctypes.data_as(vp), staged.nbytes, 1), 'hipMemcpy')
        except Exception:
            self._free()
            raise

    def _free(self):
        for p in (self.d_in, self.d_out):
            if p:
                self.hip.hipFree(p)
        self.d_in = self.d_out = None

    def enqueue(self):
        vp, env = ctypes.c_void_p, self.env
        self.rc = int(env.lib.cc4_run_plan_device(env._h, self.k, self.d_in, vp(self.d_in.value + self.b_act) if self.with_msgs else None, self.d_out,
                                                  vp(self.d_out.value + self.b_rew + self.b_pk), vp(self.d_out.value + self.b_rew) if self.b_pk else None))
        if self.rc:
            msg = env.lib.cc4_last_error(env._h)
            self.error = msg.decode() if msg else ''
        return self.rc

    def finish(self):
        env = self.env
        try:
            assert self.rc is not None, 'finish() before enqueue()'
            rc2 = int(env.lib.cc4_synchronize(env._h))
            if rc2:
                msg = env.lib.cc4_last_error(env._h)
                raise RuntimeError(f'cc4_synchronize failed (rc={rc2}) behind a plan call that returned {self.rc}: {msg.decode() if msg else ""}')
            out = np.empty(self.b_rew + self.b_pk + self.b_done, np.uint8)
            _hip_ok(self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.d_out, out.nbytes, 2), 'hipMemcpy')
        finally:
            self._free()
        k, n = self.k, self.n
        return PlanResult(self.rc, self.error, out[:self.b_rew].view(np.float32).reshape(k, n).copy(), out[self.b_rew + self.b_pk:].reshape(k, n).astype(bool),
                          out[self.b_rew:self.b_rew + self.b_pk].reshape(k, n, OBS_PACKED) if self.b_pk else None)


def run_plan_raw(env, actions, messages=None, record_obs=False, wait=True):
    """cc4_run_plan_device through env.lib on buffers the helper owns.  wait: the PlanResult (return code and cc4_last_error with the rows, whatever the
    code); else the PlanCall in flight, whose finish() gives it."""
    call = PlanCall(env, actions, messages, record_obs)
    try:
        call.enqueue()
    except Exception:
        call._free()
        raise
    return call.finish() if wait else call


def shadow_handle(env):
    """The self-check's shadow handle of env (cc4_debug_shadow_handle) as a raw pointer for fetch_final, or None: the handle has none."""
    p = ctypes.c_void_p()
    rc = env.lib.cc4_debug_shadow_handle(env._h, ctypes.byref(p))
    assert rc == 0, rc
    return p if p else None


def fetch_final(lib, h, traj, plan=True):
    """What a handle (raw pointer: a CC4VecEnv's _h, or a shadow) holds at the call's end, paired with the trajectory's: first_mismatch's `final`.
    plan: the error words of a plan call hold every flag of the call, those of a `random` call the last step's."""
    n, vp = traj.hot.shape[0], ctypes.c_void_p

    def ok(rc, what):
        if rc != 0:
            msg = lib.cc4_last_error(h)
            raise RuntimeError(f'{what} failed (rc={rc}): {msg.decode() if msg else ""}')
    obs, rew, done, err = np.zeros((n, OBS), np.int32), np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    ok(lib.cc4_fetch(h, obs.ctypes.data_as(vp), rew.ctypes.data_as(vp), done.ctypes.data_as(vp), err.ctypes.data_as(vp)), 'cc4_fetch')
    hot = np.zeros((n, int(lib.cc4_state_bytes())), np.uint8)
    ok(lib.cc4_get_states(h, 0, n, hot.ctypes.data_as(vp)), 'cc4_get_states')
    rng = np.zeros((n, 7), np.uint64)
    ok(lib.cc4_get_rng_state(h, rng.ctypes.data_as(vp)), 'cc4_get_rng_state')
    cold = np.zeros((len(traj.cold), int(lib.cc4_cold_bytes(h))), np.uint8)
    for i, e in enumerate(traj.cold):
        ok(lib.cc4_get_cold(h, int(e), cold[i].ctypes.data_as(vp)), 'cc4_get_cold')
    return {'error words': (err, traj.err if plan else traj.err_last), 'last observations': (obs, traj.obs_last), 'last rewards': (rew, traj.reward_last),
            'last dones': (done.astype(bool), traj.done_last), 'hot rows': (hot, traj.hot), 'generator state': (rng, traj.rng),
            'cold rows': (cold, np.stack(list(traj.cold.values())), list(traj.cold))}


# ---------------------------------------------------------------------------------------------------------------- the verdict
Side = collections.namedtuple('Side', 'obs_packed rewards dones final', defaults=(None, None, None, None))     # first_mismatch's arguments: what one side produced
VERIFY_MISMATCH = -5                # a checked call that disagreed with its shadow (include/cc4.h cc4_verify_stats)


def self_check_verdict(cell, traj, rc, error, main, shadow=None):
    """A call under the self-check, arbitrated: None (the call returned 0 and the main handle's side equals the oracle's trajectory), or a message that
    names the side that left it.  main / shadow: Side (the shadow's recorded rows are freed inside the call: its final arrays only; None: not fetched)."""
    main_bad = first_mismatch(cell, traj, *main)
    shadow_bad = first_mismatch(cell, traj, *shadow) if shadow is not None else None
    shadow_says = ('the shadow was not fetched' if shadow is None else
                   'the shadow differs from the oracle too: ' + shadow_bad if shadow_bad else 'the shadow equals the oracle in everything fetched')
    if rc == 0:
        if main_bad is None:
            return None
        return f'the call returned 0 and the main side is off the oracle -- both sides wrong alike, or a difference the self-check does not look at: {main_bad}; {shadow_says}'
    if rc != VERIFY_MISMATCH:
        return f'the call failed (rc={rc}): {error}'
    said = f'the self-check said: "{error}"'
    if main_bad is None:
        where = ('the shadow against the oracle: ' + shadow_bad if shadow_bad else
                 'the shadow was not fetched' if shadow is None else 'the shadow\'s rows at the call\'s end equal the oracle too: the difference lies in its recorded trajectory rows alone')
        return f'SHADOW LEFT THE TRAJECTORY (rc=-5; the kernel\'s side equals the oracle in everything compared): {where}; {said}'
    return f'KERNEL LEFT THE TRAJECTORY (rc=-5): {main_bad}; {shadow_says}; {said}'


def neighbour_verdict(cell, traj, a, b):
    """Handle A (the persistent kernel) and handle B (the per-step launches beside it), each (rc, error, Side), each against the same trajectory: None, or a
    message that names which of them differs."""
    parts = []
    for name, (rc, error, side) in (('A (the persistent kernel)', a), ('B (the per-step launches beside it)', b)):
        if rc != 0:
            parts.append(f'{name}: the call failed (rc={rc}): {error}')
            continue
        bad = first_mismatch(cell, traj, *side)
        parts.append(f'{name} LEFT THE TRAJECTORY: {bad}' if bad else f'{name} equals the oracle')
    return None if all(p.endswith('equals the oracle') for p in parts) else '; '.join(parts)


def overlap_share(a0, a1, b0, b1):
    """The share of [a0, a1] (A's call on its stream) during which [b0, b1] (B's launches on theirs) was in flight; times on one clock.  None: A took no time."""
    if not a1 > a0:
        return None
    return max(0.0, min(a1, b1) - max(a0, b0)) / (a1 - a0)


class StreamTimes:
    """HIP events on the handles' main streams (cc4_group_info, group 0), read against one reference event recorded first: mark(name, env) records one,
    times() -- behind a synchronisation of everything marked -- gives {name: ms since the reference} (hipEventElapsedTime works across streams)."""
    def __init__(self, env):
        self.hip, self.ev = hip_runtime(), collections.OrderedDict()
        self.mark('ref', env)

    @staticmethod
    def stream(env):
        s = ctypes.c_void_p()
        rc = env.lib.cc4_group_info(env._h, 0, None, None, ctypes.byref(s))
        assert rc == 0, rc
        return s

    def mark(self, name, env):
        e = ctypes.c_void_p()
        _hip_ok(self.hip.hipEventCreate(ctypes.byref(e)), 'hipEventCreate')
        self.ev[name] = e
        _hip_ok(self.hip.hipEventRecord(e, self.stream(env)), 'hipEventRecord')

    def times(self):
        out = {}
        try:
            for name, e in self.ev.items():
                _hip_ok(self.hip.hipEventSynchronize(e), 'hipEventSynchronize')
                ms = ctypes.c_float(0.0)
                _hip_ok(self.hip.hipEventElapsedTime(ctypes.byref(ms), self.ev['ref'], e), 'hipEventElapsedTime')
                out[name] = float(ms.value)
        finally:
            self.close()
        return out

    def close(self):
        for e in self.ev.values():
            self.hip.hipEventDestroy(e)
        self.ev = collections.OrderedDict()
