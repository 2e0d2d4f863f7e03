"""CC4TorchVecEnv -- CC4VecEnv for a PyTorch learner on the same GPU: actions in, observations / masks / rewards / dones out, as torch
tensors on the device, with no host copy and no host synchronisation in step().

The engine's work runs on the handle's own (non-blocking) HIP streams; every call here is ordered against torch's current stream
in both directions (cc4_stream_wait / cc4_stream_signal, include/cc4.h), and one kernel (k_policy_outputs, cc4_policy_outputs) writes
the outputs straight into this object's tensors in the dtype the policy wants.  Importing this module imports torch; importing the
package does not."""
import ctypes
import numpy as np
import torch
from . import _lib as L
from . import _tensors as TS
from . import _views as V
from ._tensors import dptr as _dptr
from .vec_env import CC4VecEnv, as_env_mask, as_ptr, as_seeds, raise_on_copy_faults, split_obs, split_mask  # noqa: F401  (split_obs / split_mask slice tensors too)

_OBS_DTYPES = TS.torch_codes(torch, TS.OBS_DTYPE_CODES)
_LOGIT_DTYPES = TS.torch_codes(torch)      # the same codes: what sample_actions() takes
_TORCH_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}      # of the views' outputs


# ---- the tensor checks: a ValueError that names the argument, or the contiguous cast (on the current stream, as step() casts its actions)
def int_tensor(x, shape, device, what, *, to, saturate=False, bool_ok=False):
    """x as a contiguous tensor of dtype `to`: an integer tensor (bool_ok: or a bool one) of `shape` (None: any extent) on `device`.
    saturate: a value beyond `to` stays out of range instead of wrapping into it."""
    if (not torch.is_tensor(x) or x.dtype.is_floating_point or x.dtype.is_complex or (x.dtype == torch.bool and not bool_ok) or x.dim() != len(shape)
            or any(w is not None and w != g for w, g in zip(shape, x.shape)) or x.device != device):
        want = ', '.join('k' if w is None else str(w) for w in shape)
        raise ValueError(f'{what} must be an integer {"or bool " if bool_ok else ""}tensor [{want}] on {device}')
    if saturate and x.dtype != to:
        x = x.clamp(torch.iinfo(to).min, torch.iinfo(to).max)
    return x.to(to).contiguous()


def seed_tensor(x, n, device, what='seeds'):
    """Seeds as the int64 words the entry points read: a uint64 tensor is viewed, any other integer dtype cast."""
    if torch.is_tensor(x) and x.dtype == torch.uint64 and tuple(x.shape) == (n,) and x.device == device:
        return x.view(torch.int64).contiguous()
    return int_tensor(x, (n,), device, what, to=torch.int64)


def mask_tensor(x, n, device, what='env_mask'):
    """An episode mask as uint8: bool or uint8 only.  (A bool tensor -- the env's own `done`, which a reset's outputs rewrite -- is copied.)"""
    if torch.is_tensor(x) and x.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'{what} must be a bool or uint8 tensor [{n}] on {device}')
    return int_tensor(x, (n,), device, what, to=torch.uint8, bool_ok=True)


class _Ordered:
    """The stream bracket every call of CC4TorchVecEnv that orders against the caller's stream goes through.  On entry: the env's device, and the
    handle's streams wait for what torch's current stream holds at this moment (cc4_stream_wait) -- so argument checks, casts and staging copies
    come BEFORE the bracket: a refused call enqueues nothing, and a cast is waited for.  The body enqueues the library's work.  On exit the stream
    waits for the handle's: behind the kernel that writes the env's output tensors (outputs=True: _outputs), or as they stand
    (cc4_stream_signal).  Temporaries of the casts live on that stream, so the signal also orders their reuse behind their reader.  A body that
    raises leaves the stream unsignalled: nothing of that call is to be read.  (A plain class, not a generator: step() passes here every step.)"""
    __slots__ = ('env', 'outputs', 'guard', 's')

    def __init__(self, env, outputs=False):
        self.env, self.outputs = env, outputs

    def __enter__(self):
        env = self.env
        self.guard = torch.cuda.device(env.device)
        self.guard.__enter__()
        self.s = ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)
        rc = env.lib.cc4_stream_wait(env._h, self.s)
        if rc:
            self.guard.__exit__(None, None, None)
            env.venv._chk(rc, 'cc4_stream_wait')
        return self.s

    def __exit__(self, kind, exc, tb):
        try:
            if kind is None and self.outputs:
                self.env._outputs(self.s)
            elif kind is None:
                self.env.venv._chk(self.env.lib.cc4_stream_signal(self.env._h, self.s), 'cc4_stream_signal')
        finally:
            self.guard.__exit__(kind, exc, tb)


class CC4TorchVecEnv:
    """N episodes of CC4VecEnv stepped from device tensors.

    CC4TorchVecEnv(num_envs, *, obs_dtype=torch.uint8, **kw): kw are CC4VecEnv's keyword arguments (steps, rng_mode, device_id,
    autoreset, red_policy, green_policy, topology_seed, blue_policy, strict); the tensors live on cuda:<device_id>.

    reset(seeds=None, env_mask=None) -> (obs, info)             seeds / env_mask as CC4VecEnv.reset
    step(actions, messages=None, red_actions=None) -> (obs, reward, done, info)
        actions   integer tensor [N, 5] of wrapper action indices on the env's device (negative: no action), any integer dtype;
        messages  optional [N, 5, 8] tensor of 0 / 1 bytes;
        obs [N, 578] obs_dtype, reward [N] float32, done [N] bool, info {'action_mask': [N, 570] bool, 'err': [N] int32}.
    Everything runs on torch's current stream of the env's device as it stands at the call: whatever the caller enqueued there before (the policy that
    wrote `actions`) happens before the step, and whatever it enqueues after the call sees the step's outputs.  Callers that switch
    streams between calls order those streams themselves, as with any torch tensor.

    The returned tensors are this object's own and are REUSED: they hold the outputs of the last step / reset and stay valid until the
    next step() or reset() (clone what must outlive it).  `done` is terminated or truncated, as the reference's wrapper reports it
    (BlueFixedActionWrapper.py:177-178).  With autoreset=True, the call that follows a `done` regenerates that episode and takes no
    step in it (reward 0, the new scenario's first observation and action mask).  The action masks are refreshed for exactly the
    episodes a call (re)generated, on the device.

    Episode copies on the device (branching, undo, checkpoints; include/cc4.h cc4_copy_episodes_device):
    new_bank(capacity)                         -> uint8 tensor [capacity, snapshot_bytes] of never-written snapshot slots on the env's device
    clone_episodes(src, dst, seeds=None)       -> (obs, info)   episode dst[i] becomes a copy of episode src[i]
    save_episodes(env_ids, bank, slots)        -> (obs, info)   slot slots[i] of bank holds episode env_ids[i]
    load_episodes(bank, slots, env_ids, seeds=None) -> (obs, info)   episode env_ids[i] becomes the episode saved in slot slots[i]
        Index arguments are integer tensors on the device (any integer dtype), seeds an optional [n] int64 / uint64 tensor (cc4_set_seed applied
        to the copy).  A copy carries the episode's outputs: obs, reward, done, err and the action mask of a destination are its source's at
        once.  A slot holds no pointers: bank.cpu() and back, or into another env of the same steps and rng_mode, restores the episodes exactly.
        Faulty entries (an index out of range, a duplicated destination, a source that is also a destination, a slot never written or written
        by another configuration) are skipped; check_errors() raises CC4EngineError for them.

    The privileged global state for a centralised critic (include/cc4.h cc4_state_features_device; cage_challenge_4_amd.state_features):
    state_features(ids=None, bank=None, out=None) -> (hosts [n, 137, 16] uint8, glob [n, 32] int32)   of the env's episodes, or of the slots of a bank

    Red agents as learners (include/cc4.h cc4_step_red_device, cc4_red_view_device; cage_challenge_4_amd.red_view):
    step(actions, messages=None, red_actions=t)   t integer tensor [N, 6, 4] on the device: (type, host, arg, session) per red agent; type -1: the
                                                  agent's scripted policy acts; session -1: its first listed session.  A refused record (a type,
                                                  host or subnet out of range) becomes "no action", and check_errors() raises CC4EngineError for it.
                                                  Red's reward is -reward.  An env that has taken red actions runs the full builds of its step kernel.
    red_view(ids=None, bank=None, out=None) -> (hosts [n, 6, 137, 8] uint8, scalars [n, 6, 16] int32)   what each red agent knows

    Blue's own knowledge (include/cc4.h cc4_blue_view_device; cage_challenge_4_amd.blue_view):
    blue_view(ids=None, bank=None, out=None) -> (hosts [n, 5, 137, 8] uint8, scalars [n, 5, 16] int32)   busy, the outcome of the agent's own action,
                                                  what Analyse found, the deployed decoy, suspicious pids; with enable_event_log() the Monitor's
                                                  entries per host (counts, ports, remote hosts)
    enable_event_log(on=True)                     the per-step event log (full builds of the step kernel, one launch per step)
    blue_edges(ids=None, bank=None, out=None, max_edges=160) -> (edges [n, max_edges, 8] int32, counts [n, 8] int32)   the Monitor's connection
                                                  entries as a sorted, merged edge list: who talked to whom on which ports (needs the event log;
                                                  cage_challenge_4_amd.blue_edges, to_edge_index for a graph layer)

    Reward terms (include/cc4.h cc4_reward_terms_device; cage_challenge_4_amd.reward_terms):
    enable_reward_terms(on=True)                  record the pieces of every step's reward (full builds of the step kernel, one launch per step)
    reward_terms(ids=None, bank=None, out=None) -> (terms [n, 9, 4] int32, words [n, 16] int32)   per subnet the LocalWork / AccessService /
                                                  Impact penalties and the number of events; brm, action cost, each blue agent's share

    From policy logits to valid actions (include/cc4.h cc4_sample_actions_device; cage_challenge_4_amd.action_sampling):
    sample_actions(logits=None, *, seed=0, t=None, temperature=1.0, greedy=False, busy_aware=True, ids=None, bank=None, out=None)
                                                  -> (actions [n, 5] int32, stats [n, 5, 2] float32)   a policy's [n, 570] logits to the indices
                                                  step() takes in one launch: masked, busy agents -1, logp and entropy of the draw
    evaluate_actions(logits, mask, actions, temperature=1.0) -> (logp [..., 5], entropy [..., 5]) float32   the update's half: stored actions
                                                  under new logits, with the gradient back to the logits (cage_challenge_4_amd.action_logp)
    advantages(rewards, values, last_value, dones, *, gamma, lam, done0=None, actions=None, bootstrap=False, out=None)
                                                  -> (adv, ret, weight) in the shape of values   GAE of a stored rollout in one launch, in this
                                                  env's autoreset layout: skip rows and -1 actions get weight 0 (cage_challenge_4_amd.advantages)

    Mixed opponents in one batch (include/cc4.h cc4_set_policies_device, cc4_reset_device):
    set_opponents(red=None, green=None, blue=None)   integer tensors [N] on the device: the classes each episode regenerates into from its next
                                                     regeneration on (never mid-episode); None keeps
    opponents()                                      -> (live, assigned) two [N, 3] int8 tensors (red, green, blue)
    reset(seeds=tensor, env_mask=tensor)             seeds any integer dtype, env_mask bool or uint8 (env.reset(env_mask=env.done)): no host wait

    No call synchronises except check_errors(), which reads the error flags and raises what CC4VecEnv raises (ValueError for a step past
    the episode's end -- the reference's own error -- and CC4EngineError for any other flag; strict=False: the ValueError only), and raises
    CC4EngineError for the faults of the copies and state_features calls since the last call."""

    def __init__(self, num_envs, *, obs_dtype=torch.uint8, **kw):
        if obs_dtype not in _OBS_DTYPES:
            raise ValueError(f'obs_dtype must be one of {list(_OBS_DTYPES)}, got {obs_dtype}')
        self.venv = CC4VecEnv(num_envs, **kw)        # creates the handle (CC4Error without a HIP device) and keeps the error bookkeeping
        self.lib, self._h = self.venv.lib, self.venv._h
        self.num_envs = n = self.venv.num_envs
        self.obs_dtype = obs_dtype
        self._dt = _OBS_DTYPES[obs_dtype]
        self.device = torch.device('cuda', int(kw.get('device_id', 0)))
        self.autoreset = bool(kw.get('autoreset', False))
        with torch.cuda.device(self.device):
            z = dict(device=self.device)
            self.obs = torch.zeros((n, L.OBS_PER_ENV), dtype=obs_dtype, **z)
            self.action_mask = torch.zeros((n, L.MASK_PER_ENV), dtype=torch.bool, **z)
            self.reward = torch.zeros(n, dtype=torch.float32, **z)
            self.done = torch.zeros(n, dtype=torch.bool, **z)
            self.err = torch.zeros(n, dtype=torch.int32, **z)
            self._actions = torch.zeros((n, L.NUM_BLUE), dtype=torch.int32, **z)
            self._fresh = torch.zeros(n, dtype=torch.uint8, **z)     # episodes a copy overwrote since the last check_errors (strict mode: new episodes)
            self._messages = torch.zeros((n, L.NUM_BLUE, L.MSG_LEN), dtype=torch.uint8, **z)
            self._red = None         # [N, 6, 4] int32 staging of step(red_actions=...), allocated on first use
        self._sample_t = 0           # the counter word of sample_actions(t=None)
        vp = ctypes.c_void_p
        self._p_out = (vp(self.obs.data_ptr()), vp(self.action_mask.data_ptr()), vp(self.reward.data_ptr()), vp(self.done.data_ptr()),
                       vp(self.err.data_ptr()))
        self._p_act, self._p_msg = vp(self._actions.data_ptr()), vp(self._messages.data_ptr())

    def _info(self):
        return {'action_mask': self.action_mask, 'err': self.err}

    def _outputs(self, s):
        # (the handle's streams -> s behind the kernel that wrote this object's tensors)
        lib, h = self.lib, self._h
        rc = lib.cc4_policy_outputs(h, self._dt, *self._p_out)
        if rc:
            self.venv._chk(rc, 'cc4_policy_outputs')
        self.venv._chk(lib.cc4_stream_signal(h, s), 'cc4_stream_signal')

    def _call(self, entry, *args, outputs=False):
        """One entry point of the library inside the stream bracket."""
        with _Ordered(self, outputs):
            rc = getattr(self.lib, entry)(self._h, *args)
            if rc:
                self.venv._chk(rc, entry)

    def reset(self, seeds=None, env_mask=None):
        """seeds / env_mask as CC4VecEnv.reset (NumPy arrays, a scalar, None: cc4_reset, which waits for the device) -- or tensors on the env's
        device (seeds any integer dtype, env_mask bool or uint8, e.g. env.reset(env_mask=env.done)): cc4_reset_device on the current stream, no
        host wait; a NumPy array or scalar beside a tensor is moved to the device."""
        n = self.num_envs
        seeds, env_mask = (x if torch.is_tensor(x) else f(x, n) for x, f in ((seeds, as_seeds), (env_mask, as_env_mask)))
        if torch.is_tensor(seeds) or torch.is_tensor(env_mask):
            up = lambda a, dt: a if a is None or torch.is_tensor(a) else torch.from_numpy(a.view(dt)).to(self.device)      # noqa: E731
            seeds, env_mask = up(seeds, np.int64), up(env_mask, np.uint8)
            seeds = None if seeds is None else seed_tensor(seeds, n, self.device)
            env_mask = None if env_mask is None else mask_tensor(env_mask, n, self.device)
            self._call('cc4_reset_device', _dptr(seeds), _dptr(env_mask), outputs=True)
        else:
            # the reset rewrites rows the last step's kernels may still read, and the outputs go into tensors the caller's stream may
            # still read: everything on the stream first (cc4_reset itself waits for the device before it returns)
            self._call('cc4_reset', as_ptr(seeds), as_ptr(env_mask), outputs=True)
        return self.obs, self._info()

    def step(self, actions, messages=None, red_actions=None):
        if tuple(actions.shape) != (self.num_envs, L.NUM_BLUE) or (messages is not None and tuple(messages.shape) != tuple(self._messages.shape)):
            raise ValueError(f'actions must be [{self.num_envs}, {L.NUM_BLUE}] and messages [{self.num_envs}, {L.NUM_BLUE}, {L.MSG_LEN}]')
        if red_actions is not None:
            red_actions = int_tensor(red_actions, (self.num_envs, L.NUM_RED, L.RED_ACT_WORDS), self.device, 'red_actions (type, host, arg, session)',
                                     to=torch.int32, saturate=True)
            if self._red is None:
                self._red = torch.zeros_like(red_actions)
            self._red.copy_(red_actions)
        # staging copies on the current stream: any integer dtype cast, and the env no longer depends on the lifetime of the caller's tensors
        self._actions.copy_(actions)
        if messages is not None:
            self._messages.copy_(messages)
        mp = self._p_msg if messages is not None else None
        if red_actions is None:
            self._call('cc4_step_device', self._p_act, mp, outputs=True)
        else:
            self._call('cc4_step_red_device', self._p_act, mp, _dptr(self._red), outputs=True)
        return self.obs, self.reward, self.done, self._info()

    def step_plan(self, actions, messages=None, record_obs=False):
        """k steps with the blue actions known in advance (cc4_run_plan_device: one launch of the persistent kernel where it serves the batch,
        venv.plan_kernel_for(k)): actions integer tensor [k, N, 5] on the env's device, messages optional [k, N, 5, 8] of 0 / 1.
        Returns (obs, rewards [k, N] float32, dones [k, N] bool, info): obs, info['action_mask'], info['err'] are the env's reused tensors after the
        LAST step (masks refreshed for every episode the plan regenerated; err: every flag some step raised), rewards / dones fresh tensors,
        info['obs_seq'] [k, N, 578] obs_dtype -- the observations after every step -- with record_obs.  Ordered on the current stream both
        ways like step(); no host copy, no host wait."""
        n = self.num_envs
        # the casts (no copy when the plan is int32 / uint8 and contiguous already) and the trajectory's tensors, on the current stream
        plan = int_tensor(actions, (None, n, L.NUM_BLUE), self.device, 'actions', to=torch.int32)
        k = int(plan.shape[0])
        if k < 1:
            raise ValueError(f'actions must be an integer tensor [k, {n}, {L.NUM_BLUE}] with k >= 1')
        msgs = None if messages is None else int_tensor(messages, (k, n, L.NUM_BLUE, L.MSG_LEN), self.device, 'messages', to=torch.uint8, bool_ok=True)
        z = dict(device=self.device)
        rewards, dones = torch.empty((k, n), dtype=torch.float32, **z), torch.empty((k, n), dtype=torch.bool, **z)
        packed = torch.empty((k, n, L.OBS_PACKED_BYTES), dtype=torch.uint8, **z) if record_obs else None
        seq = torch.empty((k, n, L.OBS_PER_ENV), dtype=self.obs_dtype, **z) if record_obs else None
        info = self._info()
        with _Ordered(self, outputs=True):
            lib, h = self.lib, self._h
            rc = lib.cc4_run_plan_device(h, k, _dptr(plan), _dptr(msgs), _dptr(rewards), _dptr(dones), _dptr(packed))
            if rc:
                self.venv._chk(rc, 'cc4_run_plan_device')
            if record_obs:
                self.venv._chk(lib.cc4_unpack_rows_device(h, k * n, _dptr(packed), self._dt, _dptr(seq)), 'cc4_unpack_rows_device')
                info['obs_seq'] = seq
        return self.obs, rewards, dones, info

    @property
    def snapshot_bytes(self):
        """cc4_snapshot_bytes: bytes of one snapshot slot (header, hot row, cold row, the outputs of the last step)."""
        return int(self.lib.cc4_snapshot_bytes(self._h))

    def new_bank(self, capacity):
        return torch.zeros((int(capacity), self.snapshot_bytes), dtype=torch.uint8, device=self.device)

    def _index(self, x, what):
        return int_tensor(x, (None,), self.device, what, to=torch.int32)

    def _bank(self, bank):
        if (not torch.is_tensor(bank) or bank.dtype != torch.uint8 or bank.dim() != 2 or bank.shape[1] != self.snapshot_bytes
                or not bank.is_contiguous() or bank.device != self.device):
            raise ValueError(f'a bank is a contiguous uint8 tensor [capacity, {self.snapshot_bytes}] on {self.device} (new_bank)')
        return ctypes.c_void_p(bank.data_ptr()), int(bank.shape[0])

    def _copy(self, src, dst, src_bank=None, dst_bank=None, seeds=None):
        src, dst = self._index(src, 'source indices'), self._index(dst, 'destination indices')
        if src.shape != dst.shape:
            raise ValueError('source and destination indices must have the same length')
        sb, sc = self._bank(src_bank) if src_bank is not None else (None, 0)
        db, dc = self._bank(dst_bank) if dst_bank is not None else (None, 0)
        seeds = None if seeds is None else seed_tensor(seeds, int(src.numel()), self.device, 'seeds (one entry per copy)')
        self._call('cc4_copy_episodes_device', int(src.numel()), sb, sc, _dptr(src), db, dc, _dptr(dst), _dptr(seeds), outputs=True)
        if dst_bank is None and dst.numel():
            valid = (dst >= 0) & (dst < self.num_envs)
            self._fresh.scatter_reduce_(0, dst.clamp(0, self.num_envs - 1).long(), valid.to(torch.uint8), 'amax')
        return self.obs, self._info()

    def clone_episodes(self, src, dst, seeds=None):
        return self._copy(src, dst, seeds=seeds)

    def save_episodes(self, env_ids, bank, slots):
        return self._copy(env_ids, slots, dst_bank=bank)

    def load_episodes(self, bank, slots, env_ids, seeds=None):
        return self._copy(slots, env_ids, src_bank=bank, seeds=seeds)

    def _view(self, view, ids, bank, out, *extra, max_edges=None):
        """What the tensor methods of the derived views share.  view: its name in _views.VIEWS, which says what its two tensors are and how the
        entry point wants them aligned; ids, bank, out as state_features() documents them; extra: arguments in front of the two output pointers.
        Ordered on the current stream both ways like step(); no host copy, no host wait."""
        bp, cap = self._bank(bank) if bank is not None else (None, 0)
        ids = None if ids is None else self._index(ids, 'ids')
        n = int(ids.numel()) if ids is not None else (cap if bank is not None else self.num_envs)
        specs = [((n,) + o.tail, _TORCH_DTYPES[o.dtype], o.align) for o in V.outs(view, max_edges)]
        if out is None:
            a, b = (torch.empty(shp, dtype=dt, device=self.device) for shp, dt, _al in specs)
        else:
            a, b = out
            for k, (x, (shp, dt, al)) in enumerate(zip((a, b), specs)):
                if TS.check_tensor(torch, f'out[{k}]', x, shape=shp, dtypes=(dt,), device=self.device).data_ptr() % al:
                    raise ValueError(f'out[{k}] must be aligned to {al} bytes')
        self._call(V.VIEWS[view].device, bp, cap, _dptr(ids), n, *extra, _dptr(a), _dptr(b))
        return a, b

    def state_features(self, ids=None, bank=None, out=None):
        """The privileged global state (cc4_state_features_device, include/cc4.h; columns and words: state_features.HOST_COLUMNS / GLOBAL_WORDS)
        as tensors on the env's device: (hosts [n, 137, 16] uint8, glob [n, 32] int32).  ids: 1-D integer tensor on the device -- episodes of
        the env, or with bank= (a new_bank tensor) the slots of saved episodes, read where they lie; None: all episodes / all slots.
        out=(hosts, glob) reuses the caller's tensors.  Ordered on the current stream both ways like step(); no host copy, no host wait.  A
        faulty entry (an index out of range, a slot never written or written by another configuration) gives an all-zero row, and
        check_errors() raises CC4EngineError for it."""
        return self._view('state_features', ids, bank, out)

    def red_view(self, ids=None, bank=None, out=None):
        """What each red agent knows (cc4_red_view_device, include/cc4.h; columns and words: red_view.HOST_COLUMNS / SCALAR_WORDS) as tensors on
        the env's device: (hosts [n, 6, 137, 8] uint8, scalars [n, 6, 16] int32).  ids, bank, out and the ordering on the current stream as
        state_features(); no host copy, no host wait.  A faulty entry gives all-zero rows, and check_errors() raises CC4EngineError for it."""
        return self._view('red_view', ids, bank, out)

    def blue_view(self, ids=None, bank=None, out=None):
        """Blue's own knowledge (cc4_blue_view_device, include/cc4.h; columns and words: blue_view.HOST_COLUMNS / SCALAR_WORDS) as tensors on the
        env's device: (hosts [n, 5, 137, 8] uint8, scalars [n, 5, 16] int32) -- busy, the outcome of the agent's own action, what Analyse found,
        the deployed decoy, suspicious pids, and with enable_event_log() the Monitor's entries per host (scalars[..., 10]: whether they are
        filled).  ids, bank, out and the ordering on the current stream as state_features(); no host copy, no host wait.  A faulty entry gives
        all-zero rows, and check_errors() raises CC4EngineError for it."""
        return self._view('blue_view', ids, bank, out)

    def blue_edges(self, ids=None, bank=None, out=None, max_edges=L.BLUE_EDGES_MAX):
        """The Monitor's connection entries of the step just taken as edge lists (cc4_blue_edges_device, include/cc4.h; columns and words:
        blue_edges.COLUMNS / WORDS) as tensors on the env's device: (edges [n, max_edges, 8] int32, counts [n, 8] int32) -- agent, reporting
        host, local host, remote host, the two ports, how often, the slot within the agent's segment; sorted, merged, -1 past the last edge
        (edges[..., 0] >= 0 is the mask; counts[:, 5] > max_edges shows a truncated list).  blue_edges.to_edge_index() makes the [2, M] node
        pairs of a graph layer from it.  The per-step log must be on (enable_event_log(): the env then runs the full builds of its step kernel,
        one launch per step, and leaves the one-launch forms of run / plan calls); without it every row is -1 and counts[:, 6] is 0.
        ids, bank, out and the ordering on the current stream as state_features(); no host copy, no host wait.  A faulty entry gives -1 rows
        and zero counts, and check_errors() raises CC4EngineError for it."""
        max_edges = V.check_max_edges(max_edges)
        return self._view('blue_edges', ids, bank, out, max_edges, max_edges=max_edges)

    def sample_actions(self, logits=None, *, seed=0, t=None, temperature=1.0, greedy=False, busy_aware=True, ids=None, bank=None, out=None):
        """Valid blue actions drawn from policy logits in one launch (cc4_sample_actions_device, include/cc4.h; the definition:
        action_sampling) as tensors on the env's device: (actions [n, 5] int32, stats [n, 5, 2] float32 -- logp, entropy).  Per agent the slots
        this episode's topology does not have are masked out and one slot is drawn from softmax(logits / temperature) over the rest (greedy: the
        arg-max); a busy agent (busy_aware) gets -1, "submits nothing", and zero stats -- step() takes the actions as they are.  logits: a
        contiguous float16, bfloat16 or float32 tensor [n, 570] on the env's device, row j for entry j; None: uniform over the valid slots.
        The noise is a fixed function of (seed, t, the entry's id, agent, slot); t=None: a counter of the env that advances by one per call.
        ids, bank, out and the ordering on the current stream as state_features(); no host copy, no host wait.  A faulty entry gives -1 actions
        and zero stats, an agent whose valid logits hold a NaN or +inf or are all -inf gets -1 alone; check_errors() raises CC4EngineError for
        either."""
        from .action_sampling import check_temperature, flags_of, noise_words
        temperature = check_temperature(temperature)
        n = int(ids.numel()) if torch.is_tensor(ids) else (int(bank.shape[0]) if torch.is_tensor(bank) else self.num_envs)
        code, lp = 3, None
        if logits is not None:
            TS.check_tensor(torch, 'logits', logits, shape=(n, L.MASK_PER_ENV), dtypes=tuple(_LOGIT_DTYPES), device=self.device)
            code, lp = _LOGIT_DTYPES[logits.dtype], _dptr(logits)
        if t is None:
            t, self._sample_t = self._sample_t, self._sample_t + 1
        return self._view('sample_actions', ids, bank, out, code, lp, *noise_words(seed, t), temperature, flags_of(greedy, busy_aware))

    def evaluate_actions(self, logits, mask, actions, temperature=1.0):
        """action_logp.evaluate_actions: (logp, entropy) of stored actions under new logits, differentiable with respect to the logits -- the
        update's half of sample_actions().  A pure function of its tensors (the env is not read); action_logp.check_errors() reports refusals."""
        from .action_logp import evaluate_actions
        return evaluate_actions(logits, mask, actions, temperature)

    def advantages(self, rewards, values, last_value, dones, *, gamma, lam, done0=None, actions=None, bootstrap=False, out=None):
        """advantages.gae with autoreset taken from this env's configuration: (adv, ret, weight) of the rows a rollout stored -- done0 is
        env.done.clone() taken before the rollout's first call.  A pure function of its tensors (the env's state is not read)."""
        from .advantages import gae
        return gae(rewards, values, last_value, dones, gamma=gamma, lam=lam, done0=done0, actions=actions, autoreset=self.autoreset,
                   bootstrap=bootstrap, out=out)

    def enable_event_log(self, on=True):
        """CC4VecEnv.enable_event_log (cc4_enable_event_log): record the HostEvents entries of every step, which fills the event columns of
        blue_view() (entries per host, ports, remote hosts, the deployed decoy).  The log has a price: an env with the log on runs the full
        builds of its step kernel, one launch per step, and leaves the one-launch forms of run / plan calls.  Without it blue_view() still
        carries busy / success / what Analyse found / sus_pids."""
        self._call('cc4_enable_event_log', int(bool(on)))

    def reward_terms(self, ids=None, bank=None, out=None):
        """Why the last step's reward was what it was (cc4_reward_terms_device, include/cc4.h; columns and words: reward_terms.TERM_COLUMNS /
        WORDS) as tensors on the env's device: (terms [n, 9, 4] int32, words [n, 16] int32) -- per subnet the LocalWork-failed,
        AccessService-failed and Impact penalties and the number of charged events; valid, step_count, phase, brm, action cost, the five blue
        agents' shares, the unowned rest and the agents' own Restore costs.  words[:, 0] is 1 where the last step recorded
        (enable_reward_terms(), or an env that steps with red_actions); then words[:, 3] + words[:, 4] == reward.  ids, bank, out and the
        ordering on the current stream as state_features(); no host copy, no host wait.  A faulty entry gives all-zero rows, and
        check_errors() raises CC4EngineError for it."""
        return self._view('reward_terms', ids, bank, out)

    def enable_reward_terms(self, on=True):
        """CC4VecEnv.enable_reward_terms (cc4_enable_reward_terms): record the pieces of every step's reward, which reward_terms() turns into
        tensors.  The record has a price: the env runs the full builds of its step kernel, one launch per step, and leaves the one-launch
        forms of run / plan calls (after a plan only the last step's terms exist).  An env that steps with red_actions records anyway."""
        self._call('cc4_enable_reward_terms', int(bool(on)))

    def set_opponents(self, red=None, green=None, blue=None):
        """Assign opponent classes per episode from the device (cc4_set_policies_device, include/cc4.h): red (0..3), green (0..1), blue (0..1) each
        an integer tensor [N] on the env's device or None (keep); an entry may be L.POLICY_KEEP or L.POLICY_DEFAULT.  Takes effect at each
        episode's next regeneration (reset, autoreset), never mid-episode.  On the current stream, no host wait; a refused entry (a class out of
        range) leaves its episode as it was, and check_errors() raises CC4EngineError for it."""
        classes = [None if x is None else int_tensor(x, (self.num_envs,), self.device, what, to=torch.int8, saturate=True)
                   for x, what in ((red, 'red'), (green, 'green'), (blue, 'blue'))]
        self._call('cc4_set_policies_device', *map(_dptr, classes))

    def opponents(self):
        """(live, assigned): two fresh [N, 3] int8 tensors of (red, green, blue) classes -- what every episode runs now, and what it regenerates
        into (L.POLICY_DEFAULT where it carries no assignment).  On the current stream, no host wait."""
        live, assigned = (torch.empty((self.num_envs, 3), dtype=torch.int8, device=self.device) for _ in range(2))
        self._call('cc4_policies_device', _dptr(live), _dptr(assigned))
        return live, assigned

    def check_errors(self):
        """The one synchronising call: reads the error flags of the last step / reset and raises what CC4VecEnv.step would have raised
        (strict mode: each engine flag once per episode, a step past the end every time; an episode a copy overwrote counts as a new
        one); before that, CC4EngineError for the faults of the episode copies since the last call."""
        faults = ctypes.c_uint32(0)
        self.venv._chk(self.lib.cc4_copy_faults(self._h, ctypes.byref(faults)), 'cc4_copy_faults')
        fresh = self._fresh.cpu().numpy().astype(bool)
        if fresh.any():
            self.venv._err_seen[fresh] = 0
            self._fresh.zero_()
        raise_on_copy_faults(faults.value)
        self.venv._err[:] = self.err.cpu().numpy().view(np.uint32)
        self.venv._check_err()

    def close(self):
        if getattr(self, 'venv', None) is not None:
            self.venv.close()
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
