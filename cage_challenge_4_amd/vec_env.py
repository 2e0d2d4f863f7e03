"""CC4VecEnv -- N independent CC4 episodes stepped by the HIP engine (libcc4.so) on one MI355X.

Vectorised counterpart of  BlueFlatWrapper(CybORG(EnterpriseScenarioGenerator(SleepAgent, FiniteStateRedAgent,
EnterpriseGreenAgent, steps), seed))  (reference: CybORG/env.py:53-123, CybORG/Agents/Wrappers/BlueFlatWrapper.py).
Observations are returned as one int32 array [N, 578] = agents 0..3 (92 each) then agent 4 (210);
`split_obs` gives the per-agent views.  Rewards are the team reward every blue agent receives."""
import ctypes
import numpy as np
from . import _lib as L
from . import _views as V
from ._tensors import NUMPY_CODES

RNG_PCG64 = 0    # numpy Generator(PCG64(SeedSequence(seed))): bit-exact with the reference under the same seed
RNG_PHILOX = 1   # Philox4x32-10 keyed by seed, counter (draw, stream, step, episode)
RED_FSM, RED_SLEEP, RED_DISCOVERY, RED_RANDOM = 0, 1, 2, 3   # red_agent_class: FiniteStateRedAgent / SleepAgent / DiscoveryFSRed / RandomSelectRedAgent
GREEN_ENTERPRISE, GREEN_SLEEP = 0, 1            # green_agent_class: EnterpriseGreenAgent / SleepAgent

ERR_NAMES = {0: 'PROC_OVERFLOW', 1: 'RSESS_OVERFLOW', 2: 'KNOWN_SID_OVERFLOW', 3: 'KNOWLEDGE_BLOCK_OVERFLOW',
             4: 'SUS_OVERFLOW', 5: 'OBS_OVERFLOW', 6: 'PENDING_EVENT_OVERFLOW', 7: 'STEP_PAST_END',
             8: 'UNREACHABLE_REFERENCE_PATH', 10: 'BLUE_GREEN_SESSION_KILLED', 11: 'FSM_NO_HOST'}


def pcg64_words(gen):
    """numpy Generator(PCG64) -> the six words cc4_set_rng_state takes."""
    st = gen.bit_generator.state
    if st.get('bit_generator') != 'PCG64':
        raise NotImplementedError(f"only numpy Generator(PCG64) streams can be adopted by the device RNG (got {st.get('bit_generator')})")
    m = (1 << 64) - 1
    return [st['state']['state'] >> 64, st['state']['state'] & m, st['state']['inc'] >> 64, st['state']['inc'] & m,
            int(st['has_uint32']), int(st['uinteger'])]


COPY_FAULT_NAMES = {0: 'INDEX_OUT_OF_RANGE', 1: 'DUPLICATED_DESTINATION', 2: 'SOURCE_IS_DESTINATION', 3: 'SLOT_NEVER_WRITTEN',
                    4: 'SLOT_OF_ANOTHER_CONFIGURATION'}     # cc4_copy_faults bits (include/cc4.h CC4_COPY_*)


class CC4EngineError(RuntimeError):
    """An episode left the part of the reference's behaviour the engine reproduces (a fixed-size container overflowed, or the
    reference itself would have crashed): its results can no longer be trusted to equal the reference's."""


def err_names(bits):
    return [ERR_NAMES.get(i, f'bit{i}') for i in range(32) if (int(bits) >> i) & 1]


def raise_on_copy_faults(bits):
    """bits: cc4_copy_faults.  The faulty entries of an episode copy were skipped (their destinations are unchanged); the others took effect."""
    if bits:
        names = [COPY_FAULT_NAMES.get(i, f'bit{i}') for i in range(32) if (int(bits) >> i) & 1]
        raise CC4EngineError(f"episode copy faults {names}: the faulty entries were skipped, the others applied (include/cc4.h CC4_COPY_*)")


def raise_on_engine_error(err):
    """err: uint32 flags per episode (cc4_get_err).  Bit 7 is the reference's own ValueError (State.py:539-540); any other bit
    raises CC4EngineError -- nothing is ever dropped silently."""
    err = np.asarray(err)
    if not err.any():
        return
    if (err & (1 << 7)).any():
        raise ValueError("Step number exceeds last mission phase step maximum. "
                         "Use step parameter in EnterpriseScenarioGenerator.")  # State.py:539-540
    bad = np.nonzero(err)[0]
    raise CC4EngineError(f"engine error flags on {bad.size} episode(s), first: episode {int(bad[0])} {err_names(err[bad[0]])} "
                         f"(see ERR_NAMES / include/cc4.h; results of a flagged episode may differ from the reference)")


# ---- the argument path of the host surface: whatever the caller holds -> a contiguous array of the entry point's dtype (None stays None), or a
# ValueError that names the argument and the shape it must have.  An array of that dtype, contiguous already, passes through without a copy.
def _shaped(x, dtype, shape, what):
    """shape: the extents; None: any extent of at least one."""
    a = np.ascontiguousarray(x, dtype=dtype)
    if a.shape != shape and (a.ndim != len(shape) or any(g < 1 if w is None else g != w for w, g in zip(shape, a.shape))):
        want = ', '.join('k' if w is None else str(w) for w in shape)
        raise ValueError(f'{what} must have shape [{want}]{" with k >= 1" if None in shape else ""}, got {list(a.shape)}')
    return a


def as_seeds(x, n, what='seeds'):
    """uint64 [n]; a scalar s stands for s, s + 1, ..."""
    if x is None:
        return None
    return _shaped(np.uint64(x) + np.arange(n, dtype=np.uint64) if np.isscalar(x) else x, np.uint64, (n,), what)


def as_env_mask(x, n):
    """uint8 [n]: nonzero selects the episode."""
    return None if x is None else _shaped(x, np.uint8, (n,), 'env_mask')


def _batch(x, dtype, n, k, tail, what):
    """[n, *tail]; with k a plan of them, [k, n, *tail] (k = 0: of any length k >= 1)."""
    return None if x is None else _shaped(x, dtype, (() if k is None else (k or None,)) + (n,) + tail, what)


def as_actions(x, n, k=None):
    """int32 [n, 5] wrapper indices, from any integer dtype; with k a plan [k, n, 5] (k = 0: of any length k >= 1)."""
    return _batch(x, np.int32, n, k, (L.NUM_BLUE,), 'actions')


def as_messages(x, n, k=None):
    """uint8 [n, 5, 8] of 0 / 1; with k the messages of a plan [k, n, 5, 8]."""
    return _batch(x, np.uint8, n, k, (L.NUM_BLUE, L.MSG_LEN), 'messages')


def as_ptr(x):
    """What ctypes takes for a void*: an array's data, a device address (int), a ctypes.c_void_p as it is, None."""
    if x is None or isinstance(x, ctypes.c_void_p):
        return x
    return x.ctypes.data_as(ctypes.c_void_p) if isinstance(x, np.ndarray) else ctypes.c_void_p(int(x))


def stage_layout(parts):
    """Where the parts of one staging allocation lie: parts are input arrays (placed at 16 bytes) or outputs (nbytes, alignment); returns
    (offsets, total) with every part at a multiple of its alignment, in the order given, none overlapping."""
    offsets, end = [], 0
    for p in parts:
        nbytes, align = (p.nbytes, 16) if isinstance(p, np.ndarray) else p
        offsets.append(-(-end // align) * align)
        end = offsets[-1] + nbytes
    return offsets, end


class Staged:
    """One device allocation laid out by stage_layout, for the host-array forms of calls that work on device memory.  The leading input arrays go
    up in one copy on entry, ptr(i) is part i's device address, down(i, out) copies output part i into the array `out`; freed on every path."""

    def __init__(self, device, parts):
        self.device, self.parts, self.d = device, parts, ctypes.c_void_p()
        self.offsets, self.total = stage_layout(parts)

    def __enter__(self):
        hip = _hip()
        _hip_chk(hip.hipSetDevice(self.device), 'hipSetDevice')
        _hip_chk(hip.hipMalloc(ctypes.byref(self.d), max(self.total, 1)), 'hipMalloc')
        try:
            ins = [p for p in self.parts if isinstance(p, np.ndarray)]
            if len(ins) > 1:                  # (several inputs: put together on the host as they will lie, so that one copy takes them up)
                up = np.zeros(self.offsets[len(ins) - 1] + ins[-1].nbytes, np.uint8)
                for a, o in zip(ins, self.offsets):
                    up[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
                ins = [up]
            if ins and ins[0].nbytes:
                _hip_chk(hip.hipMemcpy(self.d, as_ptr(ins[0]), ins[0].nbytes, 1), 'hipMemcpy')
        except BaseException:
            hip.hipFree(self.d)
            raise
        return self

    def __exit__(self, *exc):
        _hip().hipFree(self.d)

    def ptr(self, i):
        return ctypes.c_void_p(self.d.value + self.offsets[i])

    def down(self, i, out):
        _hip_chk(_hip().hipMemcpy(as_ptr(out), self.ptr(i), out.nbytes, 2), 'hipMemcpy')
        return out


class CC4VecEnv:
    def __init__(self, num_envs, steps=500, rng_mode=RNG_PCG64, device_id=0, autoreset=False, red_policy=0, green_policy=0,
                 topology_seed=0, strict=True, blue_policy=0):
        """topology_seed != 0 (RNG_PHILOX only): all episodes share the scenario drawn from that key (uniform topology).
        blue_policy 1: cc4BlueRandomAgent acts for every blue agent whose action index is negative (0: such an agent sleeps).
        red_policy / green_policy / blue_policy may be [N] arrays: a class per episode (set_policies), in place from the first reset on.
        strict: raise (ValueError for a step past the episode's end, as the reference does; CC4EngineError otherwise) as soon as
        any episode carries an error flag.  strict=False leaves the flags to the caller (`err`, `info['err']`)."""
        self.strict = bool(strict)
        self.lib = L.load()
        self.num_envs = int(num_envs)
        self.steps = int(steps)
        self._dev = int(device_id)
        # per-episode classes ([N] arrays): the handle is created with class 0 for them, and they are assigned before the first reset
        per_episode = {k: np.asarray(v) for k, v in (('red', red_policy), ('green', green_policy), ('blue', blue_policy)) if np.ndim(v) > 0}
        if per_episode:
            red_policy, green_policy, blue_policy = (0 if np.ndim(v) > 0 else v for v in (red_policy, green_policy, blue_policy))
            if int(green_policy) == 2:
                raise ValueError('green_policy 2 (the caller submits the green actions) cannot be combined with per-episode classes')
            # (an assignment is all three classes: the scalar ones are assigned to every episode beside the arrays)
            per_episode = {k: per_episode.get(k, v) for k, v in (('red', red_policy), ('green', green_policy), ('blue', blue_policy))}
        cfg = L.CC4Config(self.num_envs, self.steps, int(device_id), int(rng_mode), int(bool(autoreset)),
                          int(red_policy), int(green_policy), int(topology_seed), int(blue_policy))
        h = ctypes.c_void_p()
        rc = self.lib.cc4_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc != 0:
            msg = self.lib.cc4_last_error(h if h else None)
            if h:
                self.lib.cc4_destroy(h)
            raise L.CC4Error(f"cc4_create failed (rc={rc}): {msg.decode() if msg else ''}")
        self._h = h
        n = self.num_envs
        self._obs = np.zeros((n, L.OBS_PER_ENV), np.int32)
        self._rew = np.zeros(n, np.float32)
        self._done = np.zeros(n, np.uint8)
        self._mask = np.zeros((n, L.MASK_PER_ENV), np.uint8)
        self._err = np.zeros(n, np.uint32)
        self._err_seen = np.zeros(n, np.uint32)      # flags already raised for (strict mode raises once per flag and episode)
        self._any_seen = False
        vp = ctypes.c_void_p
        self._p_out = (self._obs.ctypes.data_as(vp), self._rew.ctypes.data_as(vp), self._done.ctypes.data_as(vp), self._err.ctypes.data_as(vp))
        if per_episode:
            try:
                self.set_policies(**per_episode)
            except Exception:
                self.close()
                raise

    # -- lifecycle
    def close(self):
        if getattr(self, '_h', None):
            self.lib.cc4_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        L.check(self.lib, self._h, rc, what)

    # -- API
    def reset(self, seeds=None, env_mask=None):
        """seeds: None (streams continue, == reference reset(seed=None)), int (seed+i per env) or array [N]."""
        seeds, env_mask = as_seeds(seeds, self.num_envs), as_env_mask(env_mask, self.num_envs)
        self._chk(self.lib.cc4_reset(self._h, as_ptr(seeds), as_ptr(env_mask)), 'cc4_reset')
        return self._fetch(mask=True)[0]

    def _policy_array(self, v, name):
        if v is None:
            return None
        a = np.asarray(v)
        if a.ndim == 0:
            a = np.full(self.num_envs, a)
        if a.shape != (self.num_envs,):
            raise ValueError(f'{name} must be a scalar or an array of {self.num_envs} classes')
        if ((a < -128) | (a > 127)).any():
            raise ValueError(f'{name}: class out of range')
        return np.ascontiguousarray(a, dtype=np.int8)

    def set_policies(self, red=None, green=None, blue=None):
        """Assign opponent classes per episode (cc4_set_policies, include/cc4.h): each of red (0..3), green (0..1), blue (0..1) a scalar or an [N]
        array, None = keep; an entry may be L.POLICY_KEEP or L.POLICY_DEFAULT (back to the handle's configuration).  An assignment takes effect
        at the episode's next regeneration (reset, autoreset), never mid-episode.  Refused entries (a class out of range) leave their
        episodes as they were and raise CC4EngineError after the others applied."""
        arrs = [self._policy_array(v, k) for k, v in (('red', red), ('green', green), ('blue', blue))]
        self._chk(self.lib.cc4_set_policies(self._h, *map(as_ptr, arrs)), 'cc4_set_policies')
        self._raise_copy_faults()

    def _raise_copy_faults(self):
        """Read (and clear) the faults the copies, views and assignments recorded since the last read; CC4EngineError if there are any."""
        faults = ctypes.c_uint32(0)
        self._chk(self.lib.cc4_copy_faults(self._h, ctypes.byref(faults)), 'cc4_copy_faults')
        raise_on_copy_faults(faults.value)

    def policies(self):
        """(live, assigned): two [N, 3] int8 arrays of (red, green, blue) classes -- what every episode runs now, and what it regenerates
        into (L.POLICY_DEFAULT where it carries no assignment: the handle's configuration)."""
        live = np.zeros((self.num_envs, 3), np.int8)
        assigned = np.zeros((self.num_envs, 3), np.int8)
        self._chk(self.lib.cc4_get_policies(self._h, live.ctypes.data_as(ctypes.c_void_p), assigned.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_policies')
        return live, assigned

    def step(self, actions=None, messages=None):
        """actions: int array [N,5] of wrapper indices (None / negative = no action -> Sleep)."""
        actions, messages = as_actions(actions, self.num_envs), as_messages(messages, self.num_envs)
        # cc4_step + cc4_fetch in one call: inputs up in one copy, the launch, the four results down in one copy, one host wait
        rc = self.lib.cc4_step_fetch(self._h, as_ptr(actions), as_ptr(messages), *self._p_out)
        if rc:
            self._chk(rc, 'cc4_step_fetch')
        obs, rew, done = self._check_err()
        return obs, rew, done, {'err': self._err}

    def agent_actions(self, kind):
        """An all-CC4_ACT_NONE array of cc4_agent_action records for step_ex: [N, 6] ('red') or [N, 80] ('green'); numpy
        structured dtype with the fields of include/cc4.h (type, host, arg, ticks, session, flags, rate0, rate1)."""
        a = np.zeros((self.num_envs, L.NUM_RED if kind == 'red' else L.MAX_GREEN), dtype=L.AGENT_ACTION_DTYPE)
        a['type'] = -1
        return a

    def step_ex(self, actions=None, messages=None, red=None, green=None):
        """cc4_step_ex: a step that also takes the red / green entries of the reference's `actions` dict (SimulationController.py:
        236-240) as agent_actions() arrays.  The blue indices may carry `action.duration` in bits 20..27."""
        n = self.num_envs
        args = (as_actions(actions, n), as_messages(messages, n), _batch(red, L.AGENT_ACTION_DTYPE, n, None, (L.NUM_RED,), 'red'),
                _batch(green, L.AGENT_ACTION_DTYPE, n, None, (L.MAX_GREEN,), 'green'))
        self._chk(self.lib.cc4_step_ex(self._h, *map(as_ptr, args)), 'cc4_step_ex')
        obs, rew, done = self._fetch()
        return obs, rew, done, {'err': self._err}

    def edit_state(self, env, op, a0=0, a1=0, a2=0):
        """cc4_edit_state: a direct edit of one episode between steps (what the reference's scripted tests do to
        env.environment_controller.state by hand): op 0 mission phase, 1 add service, 2 service reliability, 3 clear host,
        4 deploy one decoy kind, 5 add a red session, 6 block / allow a subnet pair, 7 step count, 8 add a host event, 9 a red
        agent's `active` flag (include/cc4.h).  Returns the op's result (>= 0)."""
        rc = int(self.lib.cc4_edit_state(self._h, int(env), int(op), int(a0), int(a1), int(a2)))
        if rc < 0:
            self._chk(rc, 'cc4_edit_state')
        return rc

    def _fetch(self, mask=False):
        self._chk(self.lib.cc4_fetch(self._h, *self._p_out), 'cc4_fetch')      # observations, reward, done, error flags: one copy
        if mask:
            self._chk(self.lib.cc4_get_action_mask(self._h, self._mask.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_action_mask')
        return self._check_err()

    def _check_err(self):
        if not self._any_seen and not self._err.any():      # the common case: no flag anywhere, none remembered
            return self._obs, self._rew, self._done.astype(bool)
        self._err_seen &= self._err                    # a regenerated episode (reset, autoreset) starts with a clean slate
        if self.strict:
            # a flag stays set in the episode's row until the episode is reset; it is raised ONCE -- a batch of thousands of
            # episodes is not taken hostage by one of them: the caller may reset that episode (env_mask) or carry on, `err` and
            # info['err'] keep showing the flag.  (A step past the episode's end raises on every call, as the reference does.)
            fresh = self._err & ~self._err_seen
            self._err_seen |= self._err
            self._any_seen = bool(self._err_seen.any())
            raise_on_engine_error(fresh | (self._err & np.uint32(1 << 7)))
        elif (self._err & (1 << 7)).any():
            raise ValueError("Step number exceeds last mission phase step maximum. "
                             "Use step parameter in EnterpriseScenarioGenerator.")  # State.py:539-540
        return self._obs, self._rew, self._done.astype(bool)

    @property
    def action_mask(self):
        return self._mask.astype(bool)

    @property
    def err(self):
        return self._err

    def topology(self, env=0):
        """cc4_get_topology: 9 cidr octets, 9 user counts, 9 server counts, 137 x (exists, ip octet)."""
        buf = np.zeros(L.TOPOLOGY_BYTES, np.uint8)
        self._chk(self.lib.cc4_get_topology(self._h, int(env), buf.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_topology')
        return buf

    def enable_event_log(self, on=True):
        """cc4_enable_event_log: record the HostEvents entries of every step (for decoded blue dict observations)."""
        self._chk(self.lib.cc4_enable_event_log(self._h, int(bool(on))), 'cc4_enable_event_log')

    def keep_previous(self, on=True):
        """cc4_keep_previous: keep the rows as they stood before every step, so that replay_logged() can produce the last step's event log on demand."""
        self._chk(self.lib.cc4_keep_previous(self._h, int(bool(on))), 'cc4_keep_previous')

    def replay_logged(self):
        """cc4_replay_logged: the last step once more on the kept rows with the event log on; true_state_json then carries its events."""
        self._chk(self.lib.cc4_replay_logged(self._h), 'cc4_replay_logged')

    def true_state_json(self, env=0):
        """cc4_get_true_state: the episode's packed state as the JSON document described in csrc/cc4_export.h."""
        need = int(self.lib.cc4_get_true_state(self._h, int(env), None, 0))
        self._chk(0 if need > 0 else need, 'cc4_get_true_state')
        buf = ctypes.create_string_buffer(need)
        self._chk(0 if self.lib.cc4_get_true_state(self._h, int(env), buf, need) > 0 else -1, 'cc4_get_true_state')
        return buf.value.decode()

    def set_seed(self, seeds):
        """cc4_set_seed: fresh generators (CybORG.set_seed) without touching the episodes."""
        if seeds is None:
            raise ValueError('seeds must be a scalar or have shape [N]')
        self._chk(self.lib.cc4_set_seed(self._h, as_ptr(as_seeds(seeds, self.num_envs))), 'cc4_set_seed')

    def set_generators(self, generators):
        """cc4_set_rng_state: adopt the streams of numpy Generator(PCG64) objects (one per episode).  The objects themselves are
        not advanced afterwards: the stream continues on the device."""
        w = np.zeros((self.num_envs, 6), np.uint64)
        for i, g in enumerate(generators):
            w[i] = pcg64_words(g)
        self._chk(self.lib.cc4_set_rng_state(self._h, w.ctypes.data_as(ctypes.c_void_p)), 'cc4_set_rng_state')

    @property
    def step_kernel(self):
        """cc4_step_kernel: the kernel this handle's steps launch ('k_step', 'k_step_philox' or 'k_step_philox1')."""
        return self.lib.cc4_step_kernel(self._h).decode()

    @property
    def run_kernel(self):
        """cc4_run_kernel: the kernel run_random_steps launches ('k_run_philox' = one launch for all k steps of a small batch)."""
        return self.lib.cc4_run_kernel(self._h).decode()

    def run_kernel_for(self, k):
        """cc4_run_kernel_for: the kernel a run_random_steps call of k steps launches."""
        return self.lib.cc4_run_kernel_for(self._h, int(k)).decode()

    @property
    def launches_per_step(self):
        """cc4_launches_per_step: a step of a large batch is several launches (episode groups on separate streams)."""
        return int(self.lib.cc4_launches_per_step(self._h))

    def host_stats(self):
        """cc4_host_stats as a dict."""
        out = np.zeros(5, np.float64)
        self._chk(self.lib.cc4_host_stats(self._h, out.ctypes.data_as(ctypes.c_void_p)), 'cc4_host_stats')
        return {'steps': int(out[0]), 'launch_us': float(out[1]), 'gather_us': float(out[2]), 'gathers': int(out[3]), 'gather_stalls': int(out[4])}

    def exchange_info(self):
        """cc4_exchange_info: the exchange inside the one-launch kernels (on / off, ring depth, steps per publish, calls served, watchdog firings)."""
        out = np.zeros(5, np.int32)
        self._chk(self.lib.cc4_exchange_info(self._h, out.ctypes.data_as(ctypes.c_void_p)), 'cc4_exchange_info')
        return {'in_kernel': bool(out[0]), 'ring': int(out[1]), 'chunk': int(out[2]), 'calls': int(out[3]), 'watchdog_timeouts': int(out[4])}

    def verify_stats(self):
        """cc4_verify_stats (CC4_PERSIST_VERIFY=1): (one-launch calls checked against per-step launches, calls that disagreed)."""
        out = (ctypes.c_int64 * 2)()
        self._chk(self.lib.cc4_verify_stats(self._h, out), 'cc4_verify_stats')
        return int(out[0]), int(out[1])

    def debug_digest(self):
        """cc4_debug_digest: the self-check's digest of every episode as it stands, [N, 3] uint64 (hot row, cold row, outputs: include/cc4_debug.h)."""
        out = np.zeros((self.num_envs, 3), np.uint64)
        self._chk(self.lib.cc4_debug_digest(self._h, out.ctypes.data_as(ctypes.c_void_p)), 'cc4_debug_digest')
        return out

    def debug_verify_plant(self, part, env=0, offset=0, step=0):
        """cc4_debug_verify_plant: arm one planted difference in the shadow's side of the next checked call (part -1 disarms); returns the hook's
        code (0, or -2: refused, nothing armed) instead of raising."""
        return int(self.lib.cc4_debug_verify_plant(self._h, int(part), int(env), int(offset), int(step)))

    def gather_log(self, steps):
        """cc4_debug_gather_log: keep the gathered rows of the next `steps` in-kernel-exchanged steps (0: free the log)."""
        self._chk(self.lib.cc4_debug_gather_log(self._h, int(steps)), 'cc4_debug_gather_log')

    def get_gather_log(self, world, first, count):
        """[count, world * N, 148] packed rows of steps first .. first + count - 1 of the log (distributed.unpack_obs decodes them)."""
        out = np.zeros((count, world * self.num_envs, 148), np.uint8)
        rc = self.lib.cc4_get_gather_log(self._h, out.ctypes.data_as(ctypes.c_void_p), int(first), int(count))
        if rc < 0:
            self._chk(rc, 'cc4_get_gather_log')
        return out

    def comm_info(self):
        """cc4_comm_info: RCCL's view of the communicator (ranks it spans, this rank, its device) + the identity of the handle's device."""
        out = np.zeros(8, np.int32)
        uuid = ctypes.create_string_buffer(33)
        self._chk(self.lib.cc4_comm_info(self._h, out.ctypes.data_as(ctypes.c_void_p), uuid), 'cc4_comm_info')
        return {'nccl_comm_count': int(out[0]), 'nccl_user_rank': int(out[1]), 'nccl_device': int(out[2]), 'hip_device': int(out[3]),
                'pci': f'{int(out[4]):04x}:{int(out[5]):02x}:{int(out[6]):02x}', 'compute_units': int(out[7]), 'device_uuid': uuid.value.decode()}

    def rng_state(self):
        out = np.zeros((self.num_envs, 7), np.uint64)
        self._chk(self.lib.cc4_get_rng_state(self._h, out.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_rng_state')
        return out

    def get_state(self, env):
        buf = np.zeros(self.lib.cc4_state_bytes(), np.uint8)
        self._chk(self.lib.cc4_get_state(self._h, int(env), buf.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_state')
        return buf

    def get_states(self):
        """The packed hot rows of ALL episodes, [num_envs][cc4_state_bytes] (checkpointing a batch, parity tests)."""
        nb = int(self.lib.cc4_state_bytes())
        out = np.zeros((self.num_envs, nb), np.uint8)
        self._chk(self.lib.cc4_get_states(self._h, 0, self.num_envs, out.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_states')
        return out

    def get_cold(self, env):
        cold = np.zeros(self.lib.cc4_cold_bytes(self._h), np.uint8)
        self._chk(self.lib.cc4_get_cold(self._h, int(env), cold.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_cold')
        return cold

    def set_state(self, env, buf):
        buf = _shaped(np.ravel(buf), np.uint8, (self.lib.cc4_state_bytes(),), 'a hot row')
        self._chk(self.lib.cc4_set_state(self._h, int(env), as_ptr(buf)), 'cc4_set_state')

    def snapshot(self, env):
        """Full episode snapshot (hot + cold row) for checkpointing / tree search / parity bisecting."""
        cold = np.zeros(self.lib.cc4_cold_bytes(self._h), np.uint8)
        self._chk(self.lib.cc4_get_cold(self._h, int(env), cold.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_cold')
        return self.get_state(env), cold

    def restore(self, env, snap):
        hot, cold = snap
        self.set_state(env, hot)
        cold = _shaped(np.ravel(cold), np.uint8, (self.lib.cc4_cold_bytes(self._h),), 'a cold row')
        self._chk(self.lib.cc4_set_cold(self._h, int(env), as_ptr(cold)), 'cc4_set_cold')

    def clone_episodes(self, src, dst, seeds=None):
        """Episode dst[i] becomes a copy of episode src[i] (cc4_clone_episodes: the device copy of cc4_copy_episodes_device, include/cc4.h);
        seeds: optional uint64 per entry, cc4_set_seed applied to the copy.  Faulty entries (an index out of range, a duplicated
        destination, a source that is also a destination) are skipped and raise CC4EngineError after the others applied.  Outputs and
        masks are fetched again; returns the observations.  A copied episode counts as a new one for strict mode."""
        src = np.ascontiguousarray(src, dtype=np.int32).ravel()
        dst = np.ascontiguousarray(dst, dtype=np.int32).ravel()
        if src.shape != dst.shape:
            raise ValueError('src and dst must have the same length')
        seeds = as_seeds(None if seeds is None else np.ravel(seeds), src.size, 'seeds (one entry per copy)')
        self._chk(self.lib.cc4_clone_episodes(self._h, int(src.size), as_ptr(src), as_ptr(dst), as_ptr(seeds)), 'cc4_clone_episodes')
        ok = dst[(dst >= 0) & (dst < self.num_envs)]
        self._err_seen[ok] = 0
        self._chk(self.lib.cc4_fetch(self._h, *self._p_out), 'cc4_fetch')
        self._chk(self.lib.cc4_get_action_mask(self._h, as_ptr(self._mask)), 'cc4_get_action_mask')
        self._raise_copy_faults()            # (of this copy: the outputs above are those of the entries that applied)
        return self._check_err()[0]

    def _view(self, view, ids, extra=(), max_edges=None, inp=None):
        """What the NumPy getters of the derived views share.  view: its name in _views.VIEWS, which says what its two arrays are, what an empty
        row holds and how the entry point wants them aligned; ids: episodes (None: all); inp: an input array that goes up with the ids; extra:
        the arguments in front of the two output pointers, or a function of inp's device address that gives them.  One staging block
        [ids | inp | first | second], the call, a synchronise like the other getters, two copies down.  An index out of range leaves the empty
        output in its row and raises CC4EngineError after the call."""
        ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ravel()
        n = self.num_envs if ids is None else int(ids.size)
        a, b = V.empty(view, (n,), max_edges)
        if n == 0:
            return a, b
        ins = [x for x in (ids, inp) if x is not None]
        with Staged(self._dev, ins + [(x.nbytes, o.align) for x, o in zip((a, b), V.VIEWS[view].outs)]) as st:
            if callable(extra):
                extra = extra(st.ptr(len(ins) - 1) if inp is not None else None)
            entry = V.VIEWS[view].device
            rc = getattr(self.lib, entry)(self._h, None, 0, st.ptr(0) if ids is not None else None, n, *extra, st.ptr(len(ins)), st.ptr(len(ins) + 1))
            rc2 = self.lib.cc4_synchronize(self._h)
            if rc or rc2:
                self._chk(rc or rc2, entry)
            st.down(len(ins), a), st.down(len(ins) + 1, b)
        if ids is not None and ((ids < 0) | (ids >= self.num_envs)).any():
            self._raise_copy_faults()
        return a, b

    def _view_device(self, view, d_a, d_b, n, d_ids, d_bank, capacity, *extra):
        """The *_device forms of the views: the entry point on device addresses of the caller's (int or ctypes.c_void_p).  Enqueued, no host wait."""
        entry = V.VIEWS[view].device
        rc = getattr(self.lib, entry)(self._h, as_ptr(d_bank), int(capacity), as_ptr(d_ids), self.num_envs if n is None else int(n), *extra, as_ptr(d_a), as_ptr(d_b))
        if rc:
            self._chk(rc, entry)

    def state_features(self, env_ids=None):
        """The privileged global state of the batch (cc4_state_features_device, include/cc4.h; columns and words: state_features.HOST_COLUMNS /
        GLOBAL_WORDS): (hosts [n, 137, 16] uint8, glob [n, 32] int32) of episodes env_ids (None: all), as NumPy arrays.  Synchronises, like
        the other getters.  An index out of range gives an all-zero row and raises CC4EngineError after the call."""
        return self._view('state_features', env_ids)

    def step_red_device(self, d_actions, d_messages, d_red):
        """cc4_step_red_device: a step with the blue indices [N, 5] int32, the messages [N, 5, 8] bytes (or None) and the red actions
        [N, 6, 4] int32 (red_view.ACTION_WORDS) all in device memory, given as device addresses (int or ctypes.c_void_p).  Enqueued, no host
        wait: fetch the outputs with the getters, or read them on the device."""
        rc = self.lib.cc4_step_red_device(self._h, as_ptr(d_actions), as_ptr(d_messages), as_ptr(d_red))
        if rc:
            self._chk(rc, 'cc4_step_red_device')

    def red_view_device(self, d_hosts, d_scalars=None, n=None, d_ids=None, d_bank=None, capacity=0):
        """cc4_red_view_device into device memory of the caller's (device addresses): hosts [n, 6, 137, 8] uint8, 16-byte aligned, scalars
        [n, 6, 16] int32 or None, of episodes d_ids (int32 [n] on the device; None: 0 .. n-1) of the env or of the slots of a snapshot bank.
        Enqueued, no host wait."""
        self._view_device('red_view', d_hosts, d_scalars, n, d_ids, d_bank, capacity)

    def red_view(self, env_ids=None):
        """What each red agent knows (cc4_red_view_device, include/cc4.h; columns and words: red_view.HOST_COLUMNS / SCALAR_WORDS):
        (hosts [n, 6, 137, 8] uint8, scalars [n, 6, 16] int32) of episodes env_ids (None: all), as NumPy arrays.  Synchronises, like the other
        getters.  An index out of range gives all-zero rows and raises CC4EngineError after the call."""
        return self._view('red_view', env_ids)

    def blue_view_device(self, d_hosts, d_scalars=None, n=None, d_ids=None, d_bank=None, capacity=0):
        """cc4_blue_view_device into device memory of the caller's (device addresses): hosts [n, 5, 137, 8] uint8, 8-byte aligned, scalars
        [n, 5, 16] int32 or None, of episodes d_ids (int32 [n] on the device; None: 0 .. n-1) of the env or of the slots of a snapshot bank.
        Enqueued, no host wait."""
        self._view_device('blue_view', d_hosts, d_scalars, n, d_ids, d_bank, capacity)

    def blue_view(self, env_ids=None):
        """Blue's own knowledge (cc4_blue_view_device, include/cc4.h; columns and words: blue_view.HOST_COLUMNS / SCALAR_WORDS):
        (hosts [n, 5, 137, 8] uint8, scalars [n, 5, 16] int32) of episodes env_ids (None: all), as NumPy arrays.  Synchronises, like the other
        getters.  The event columns need enable_event_log(); scalars[..., 10] says whether they are filled.  An index out of range gives
        all-zero rows and raises CC4EngineError after the call."""
        return self._view('blue_view', env_ids)

    def blue_edges_device(self, d_edges, d_counts=None, n=None, d_ids=None, d_bank=None, capacity=0, max_edges=L.BLUE_EDGES_MAX):
        """cc4_blue_edges_device into device memory of the caller's (device addresses): edges [n, max_edges, 8] int32, 16-byte aligned, counts
        [n, 8] int32 or None, of episodes d_ids (int32 [n] on the device; None: 0 .. n-1) of the env or of the slots of a snapshot bank.
        Enqueued, no host wait."""
        self._view_device('blue_edges', d_edges, d_counts, n, d_ids, d_bank, capacity, int(max_edges))

    def blue_edges(self, ids=None, max_edges=L.BLUE_EDGES_MAX):
        """The Monitor's connection entries of the step just taken as edge lists (cc4_blue_edges_device, include/cc4.h; columns and words:
        blue_edges.COLUMNS / WORDS): (edges [n, max_edges, 8] int32, counts [n, 8] int32) of episodes ids (None: all), as NumPy arrays.  Rows past
        an episode's edges are -1; counts[:, 5] > max_edges shows a truncated list.  Synchronises, like the other getters.
        The per-step log must be on (enable_event_log()) -- an env with the log on runs the full builds of its step kernel, one launch per step,
        and leaves the one-launch forms of run / plan calls; without it every row is -1 and counts[:, 6] is 0.  An index out of range gives
        -1 rows and zero counts and raises CC4EngineError after the call."""
        max_edges = V.check_max_edges(max_edges)
        return self._view('blue_edges', ids, (max_edges,), max_edges)

    def sample_actions_device(self, d_actions, d_stats=None, d_logits=None, logits_dtype=3, seed=0, t=0, temperature=1.0, flags=L.SAMPLE_BUSY,
                              n=None, d_ids=None, d_bank=None, capacity=0):
        """cc4_sample_actions_device on device memory of the caller's (device addresses): logits [n, 570] in logits_dtype (1 float16, 2 bfloat16,
        3 float32; None: uniform over the valid slots) -> actions [n, 5] int32 and stats [n, 5, 2] float32 (or None), of episodes d_ids (int32
        [n] on the device; None: 0 .. n-1) of the env or of the slots of a snapshot bank.  Enqueued, no host wait."""
        from .action_sampling import noise_words
        self._view_device('sample_actions', d_actions, d_stats, n, d_ids, d_bank, capacity, int(logits_dtype), as_ptr(d_logits),
                          *noise_words(seed, t), float(temperature), int(flags))

    def sample_actions(self, logits=None, ids=None, seed=0, t=0, temperature=1.0, greedy=False, busy_aware=True):
        """Valid blue actions drawn from policy logits (cc4_sample_actions_device, include/cc4.h; the definition: action_sampling):
        (actions [n, 5] int32, stats [n, 5, 2] float32 -- logp, entropy) of episodes ids (None: all), as NumPy arrays.  logits: [n, 570]
        float16 or float32 (float64 is cast to float32; uint16 is taken as bfloat16 bit patterns), row j for entry j; None: uniform over the valid
        slots.  The noise is a fixed function of (seed, t, episode, agent, slot).  A busy agent (busy_aware) gets -1: "submits nothing".
        Synchronises, like the other getters.  An index out of range gives -1 actions and zero stats and raises CC4EngineError after the call,
        as does an agent whose valid logits hold a NaN or +inf or are all -inf (only that agent is -1)."""
        from . import action_sampling as AS
        temperature = AS.check_temperature(temperature)
        n = self.num_envs if ids is None else int(np.asarray(ids).size)
        code, lg = 3, None
        if logits is not None:
            lg = np.asarray(logits)
            if lg.shape != (n, L.MASK_PER_ENV):
                raise ValueError(f'logits must have shape ({n}, {L.MASK_PER_ENV}), got {lg.shape}')
            if lg.dtype == np.float64:
                lg = lg.astype(np.float32)
            code = NUMPY_CODES.get(lg.dtype)
            if code is None:
                raise ValueError(f'logits must be float16, float32 (or uint16: bfloat16 bit patterns), got {lg.dtype}')
            lg = np.ascontiguousarray(lg)
        tail = (*AS.noise_words(seed, t), temperature, AS.flags_of(greedy, busy_aware))
        a, st = self._view('sample_actions', ids, lambda d_logits: (code, d_logits, *tail), inp=lg)       # (the logits go up with the ids)
        self._raise_copy_faults()
        return a, st

    def enable_reward_terms(self, on=True):
        """cc4_enable_reward_terms: record the pieces of every step's reward (reward_terms()).  The env then runs the full builds of its step
        kernel, one launch per step, and leaves the one-launch forms of run / plan calls and rollouts, as with submitted red / green actions;
        trajectories do not change.  on=False returns to the fast builds unless red or green actions were ever submitted on this env."""
        self._chk(self.lib.cc4_enable_reward_terms(self._h, int(bool(on))), 'cc4_enable_reward_terms')

    @property
    def reward_terms_enabled(self):
        return bool(self.lib.cc4_reward_terms_enabled(self._h))

    def reward_terms_device(self, d_terms, d_words=None, n=None, d_ids=None, d_bank=None, capacity=0):
        """cc4_reward_terms_device into device memory of the caller's (device addresses): terms [n, 9, 4] int32 and words [n, 16] int32 (or None),
        both 16-byte aligned, of episodes d_ids (int32 [n] on the device; None: 0 .. n-1) of the env or of the slots of a snapshot bank.
        Enqueued, no host wait."""
        self._view_device('reward_terms', d_terms, d_words, n, d_ids, d_bank, capacity)

    def reward_terms(self, ids=None):
        """Why the last step's reward was what it was (cc4_reward_terms_device, include/cc4.h; columns and words: reward_terms.TERM_COLUMNS /
        WORDS): (terms [n, 9, 4] int32, words [n, 16] int32) of episodes ids (None: all), as NumPy arrays.  Synchronises, like the other
        getters.  words[:, 0] says whether the last step recorded (enable_reward_terms(), or an env that steps with red / green actions).  An
        index out of range gives all-zero rows and raises CC4EngineError after the call."""
        return self._view('reward_terms', ids)

    def plan_kernel_for(self, k):
        """cc4_plan_kernel_for: the kernel a run_plan / step_plan call of k steps launches ('k_run_philox1p' / 'k_run_pcgp': one launch for the
        whole plan; else the step kernel, once per step)."""
        return self.lib.cc4_plan_kernel_for(self._h, int(k)).decode()

    def run_plan(self, actions, messages=None, record_obs=False):
        """k steps with the blue actions known in advance (cc4_run_plan_device, include/cc4.h): actions [k, N, 5] wrapper indices (any integer
        dtype; negative = no action), messages optional [k, N, 5, 8] of 0 / 1.  One upload of the plan, one call, one download of the trajectory.
        Returns (obs_last [N, 578], rewards [k, N] float32, dones [k, N] bool, info); info['obs_seq'] [k, N, 578] uint8 -- the observations
        after every step -- with record_obs.  The handle ends where k calls of step() would have left it; info['err'] holds every flag some
        step of the plan raised, and strict mode raises for them as step() does (a step past an episode's end raises ValueError in either
        mode); the exception's `plan_outputs` attribute is the tuple the call would have returned."""
        n = self.num_envs
        actions = as_actions(actions, n, 0)
        k = int(actions.shape[0])
        messages = as_messages(messages, n, k)
        ins = [actions] if messages is None else [actions, messages]             # [actions | messages]: one copy up
        b_rew, b_pk, b_done = 4 * k * n, (L.OBS_PACKED_BYTES * k * n if record_obs else 0), k * n
        with Staged(self._dev, ins + [(b_rew + b_pk + b_done, 16)]) as st:
            d_out = st.ptr(len(ins)).value
            rc = self.lib.cc4_run_plan_device(self._h, k, st.ptr(0), st.ptr(1) if messages is not None else None, as_ptr(d_out),
                                              as_ptr(d_out + b_rew + b_pk), as_ptr(d_out + b_rew) if record_obs else None)
            rc2 = self.lib.cc4_synchronize(self._h)
            if rc or rc2:
                self._chk(rc or rc2, 'cc4_run_plan_device')
            out = st.down(len(ins), np.empty(b_rew + b_pk + b_done, np.uint8))     # [rewards | packed observations | dones]: one copy down
        rewards = out[:b_rew].view(np.float32).reshape(k, n).copy()
        dones = out[b_rew + b_pk:].reshape(k, n).astype(bool)
        info = {}
        if record_obs:
            info['obs_seq'] = unpack_obs_rows(out[b_rew:b_rew + b_pk].reshape(k, n, L.OBS_PACKED_BYTES))
        self._chk(self.lib.cc4_fetch(self._h, *self._p_out), 'cc4_fetch')
        info['err'] = self._err
        try:
            obs = self._check_err()[0]
        except (ValueError, CC4EngineError) as e:       # (the plan has run: the exception carries what it produced)
            e.plan_outputs = (self._obs, rewards, dones, info)
            raise
        return obs, rewards, dones, info

    # device-resident loop used by bench.py
    def run_random_steps(self, seed0, t0, k, timed=True):
        ms = ctypes.c_float(0.0)
        self._chk(self.lib.cc4_run_random_steps(self._h, ctypes.c_uint64(seed0), ctypes.c_uint32(t0), int(k),
                                                ctypes.byref(ms) if timed else None), 'cc4_run_random_steps')
        return float(ms.value)

    def run_policy_steps(self, seed0, t0, k):
        """A learner's loop without the learner: per step a kernel writes the [N, 5] action indices into the handle's device buffer
        (cc4_random_actions_device -- k_random_actions standing in for a policy) and cc4_step_device consumes them; no host synchronisation,
        every step's observations stay readable on the device (cc4_obs_device).  Same draws as run_random_steps."""
        p = ctypes.c_void_p()
        self._chk(self.lib.cc4_actions_device(self._h, ctypes.byref(p)), 'cc4_actions_device')
        s0 = ctypes.c_uint64(seed0)
        for i in range(int(k)):
            rc = self.lib.cc4_random_actions_device(self._h, s0, ctypes.c_uint32(t0 + i)) or self.lib.cc4_step_device(self._h, p, None)
            if rc:
                self._chk(rc, 'cc4_step_device')
        return 0.0

    def run_policy_steps_grouped(self, seed0, t0, k):
        """The same loop with the policy applied per episode group on the group's own stream (cc4_group_info /
        cc4_random_actions_group_device / cc4_step_group_device): no cross-stream dependency, the groups' pipelines stay apart."""
        p = ctypes.c_void_p()
        self._chk(self.lib.cc4_actions_device(self._h, ctypes.byref(p)), 'cc4_actions_device')
        s0 = ctypes.c_uint64(seed0)
        groups = range(self.launches_per_step)
        for i in range(int(k)):
            for g in groups:
                rc = self.lib.cc4_random_actions_group_device(self._h, g, s0, ctypes.c_uint32(t0 + i)) or self.lib.cc4_step_group_device(self._h, g, p, None)
                if rc:
                    self._chk(rc, 'cc4_step_group_device')
        return 0.0

    def run_rollout(self, k, policy='random', seed0=0, t0=0, native=False):
        """A k-step rollout with the policy in the loop and ONE launch of the step engine (cc4_rollout_begin .. cc4_rollout_end, include/cc4.h): per step
        and policy group the gate on the last step's observations, the stand-in policy ('random': the draws of run_random_steps / run_policy_steps;
        'hash': action indices computed from each episode's packed observation row of the step before), the publish -- all enqueued behind the launch
        on the handle's policy stream.  A policy of the caller's takes the stand-in's place between cc4_rollout_wait_obs and cc4_rollout_publish."""
        lib, h = self.lib, self._h
        if native:       # the same sequence enqueued by the library itself (cc4_rollout_standin): no Python between the stream operations
            self._chk(lib.cc4_rollout_standin(h, int(k), 0 if policy == 'random' else 1, ctypes.c_uint64(seed0), ctypes.c_uint32(t0)), 'cc4_rollout_standin')
            return 0.0
        self._chk(lib.cc4_rollout_begin(h, int(k)), 'cc4_rollout_begin')
        G, blk = ctypes.c_int32(), ctypes.c_int32()
        rc = lib.cc4_rollout_groups(h, ctypes.byref(G), ctypes.byref(blk))
        s0 = ctypes.c_uint64(seed0)
        for j in range(int(k)):
            for g in range(G.value):
                # on the group's own policy stream: one operation for the publish of its last pass and the gate of this one (cc4_rollout_sync), then the policy
                rc = rc or lib.cc4_rollout_sync(h, g if j > 0 else -1, j - 1, g, j, None)
                rc = rc or (lib.cc4_rollout_random_policy(h, g, j, s0, ctypes.c_uint32(t0 + j), None) if policy == 'random' else lib.cc4_rollout_hash_policy(h, g, j, None))
        for g in range(G.value):
            rc = rc or lib.cc4_rollout_sync(h, g, int(k) - 1, -1, 0, None)
        end = lib.cc4_rollout_end(h)
        self._chk(rc or end, 'cc4_rollout')
        return 0.0

    def rollout_obs_packed(self, j):
        """Host copy of the packed observation rows the policy of step j of the last rollout read ([N, 148] bytes, 2 bits per value: the observations
        after step j - 1; the ring keeps the last 32 steps)."""
        p = ctypes.c_void_p()
        self._chk(self.lib.cc4_rollout_obs_packed(self._h, int(j), ctypes.byref(p)), 'cc4_rollout_obs_packed')
        out = np.zeros((self.num_envs, 148), np.uint8)
        self._chk(self.lib.cc4_debug_copy_from_device(self._h, out.ctypes.data_as(ctypes.c_void_p), p, out.nbytes), 'cc4_debug_copy_from_device')
        return out

    def rollout_actions(self, j):
        """Host copy of the action slot step j of the last rollout read ([N, 5]; slots alternate: valid for its last two steps)."""
        p = ctypes.c_void_p()
        self._chk(self.lib.cc4_rollout_actions(self._h, int(j), ctypes.byref(p)), 'cc4_rollout_actions')
        out = np.zeros((self.num_envs, L.NUM_BLUE), np.int32)
        self._chk(self.lib.cc4_debug_copy_from_device(self._h, out.ctypes.data_as(ctypes.c_void_p), p, out.nbytes), 'cc4_debug_copy_from_device')
        return out

    def device_actions(self):
        """cc4_get_actions: host copy of the handle's device action buffer ([N, 5]; after run_random_steps: the indices the last
        step drew in-kernel)."""
        out = np.zeros((self.num_envs, L.NUM_BLUE), np.int32)
        self._chk(self.lib.cc4_get_actions(self._h, out.ctypes.data_as(ctypes.c_void_p)), 'cc4_get_actions')
        return out

    def synchronize(self):
        self._chk(self.lib.cc4_synchronize(self._h), 'cc4_synchronize')


def unpack_obs_rows(packed):
    """[..., 148] packed observation rows (2 bits per value, low bits first: CC4_OBS_PACKED_BYTES) -> [..., 578] uint8 values."""
    packed = np.asarray(packed, dtype=np.uint8)
    vals = (packed[..., None] >> np.array([0, 2, 4, 6], np.uint8)) & np.uint8(3)
    return vals.reshape(packed.shape[:-1] + (4 * packed.shape[-1],))[..., :L.OBS_PER_ENV]


_hip_lib = None


def _hip():
    """The HIP runtime libcc4.so is linked against, reached through libcc4.so's own handle (a symbol lookup there searches its dependencies: no
    second search of the loader's path), for the host-array surface's staging block (Staged)."""
    global _hip_lib
    if _hip_lib is None:
        lib = ctypes.CDLL(L.LIB_PATH)
        vp = ctypes.c_void_p
        lib.hipSetDevice.argtypes, lib.hipSetDevice.restype = [ctypes.c_int], ctypes.c_int
        lib.hipMalloc.argtypes, lib.hipMalloc.restype = [ctypes.POINTER(vp), ctypes.c_size_t], ctypes.c_int
        lib.hipFree.argtypes, lib.hipFree.restype = [vp], ctypes.c_int
        lib.hipMemcpy.argtypes, lib.hipMemcpy.restype = [vp, vp, ctypes.c_size_t, ctypes.c_int], ctypes.c_int
        _hip_lib = lib
    return _hip_lib


def _hip_chk(rc, what):
    if rc != 0:
        raise L.CC4Error(f'{what} failed (hipError_t {rc})')


def split_obs(obs):
    """[N,578] -> list of 5 arrays [N,92|210] (agent order blue_agent_0..4)."""
    return [obs[:, o:o + n] for o, n in zip(L.OBS_OFF, L.OBS_LEN)]


def split_mask(mask):
    return [mask[:, o:o + n] for o, n in zip(L.ACT_OFF, L.ACT_LEN)]


def shard_range(num_envs, rank, world):
    """Static env sharding for multi-GPU runs: contiguous ranges [lo, hi)."""
    per = num_envs // world
    rem = num_envs % world
    lo = rank * per + min(rank, rem)
    return lo, lo + per + (1 if rank < rem else 0)
