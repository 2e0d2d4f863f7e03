"""CC4TorchVecEnv -- CC4VecEnv for a PyTorch learner on the same GPU: actions in, observations / masks / rewards / dones out, as torch
tensors on the device, with no host copy and no host synchronisation in step().

The engine's work runs on the handle's own (non-blocking) HIP streams; every call here is ordered against torch.cuda.current_stream()
in both directions (cc4_stream_wait / cc4_stream_signal, include/cc4.h), and one kernel (k_policy_outputs, cc4_policy_outputs) writes
the outputs straight into this object's tensors in the dtype the policy wants.  Importing this module imports torch; importing the
package does not."""
import ctypes
import numpy as np
import torch
from . import _lib as L
from .vec_env import CC4VecEnv, raise_on_copy_faults, split_obs, split_mask  # noqa: F401  (split_obs / split_mask slice tensors too)

_OBS_DTYPES = {torch.uint8: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}
_LOGIT_DTYPES = {torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}      # the same codes: what sample_actions() takes


class CC4TorchVecEnv:
    """N episodes of CC4VecEnv stepped from device tensors.

    CC4TorchVecEnv(num_envs, *, obs_dtype=torch.uint8, **kw): kw are CC4VecEnv's keyword arguments (steps, rng_mode, device_id,
    autoreset, red_policy, green_policy, topology_seed, blue_policy, strict); the tensors live on cuda:<device_id>.

    reset(seeds=None, env_mask=None) -> (obs, info)             seeds / env_mask as CC4VecEnv.reset
    step(actions, messages=None, red_actions=None) -> (obs, reward, done, info)
        actions   integer tensor [N, 5] of wrapper action indices on the env's device (negative: no action), any integer dtype;
        messages  optional [N, 5, 8] tensor of 0 / 1 bytes;
        obs [N, 578] obs_dtype, reward [N] float32, done [N] bool, info {'action_mask': [N, 570] bool, 'err': [N] int32}.
    Everything runs on torch.cuda.current_stream() as it stands at the call: whatever the caller enqueued there before (the policy that
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

    def _reset_device(self, seeds, env_mask):
        """reset() from device tensors (cc4_reset_device): no upload, no host wait.  A NumPy array or scalar beside a tensor is moved to the device."""
        n = self.num_envs
        with torch.cuda.device(self.device):
            s = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            sp = mp = None
            if seeds is not None:           # (casts and uploads on s; the allocator keeps the temporaries on s, which cc4_stream_signal orders behind their reader)
                if not torch.is_tensor(seeds):
                    seeds = np.uint64(seeds) + np.arange(n, dtype=np.uint64) if np.isscalar(seeds) else np.ascontiguousarray(seeds, dtype=np.uint64)
                    seeds = torch.from_numpy(seeds.view(np.int64)).to(self.device)
                if tuple(seeds.shape) != (n,) or seeds.dtype.is_floating_point or seeds.dtype == torch.bool or seeds.device != self.device:
                    raise ValueError(f'seeds must be an integer tensor [{n}] on {self.device}')
                seeds = (seeds.view(torch.int64) if seeds.dtype == torch.uint64 else seeds.to(torch.int64)).contiguous()
                sp = ctypes.c_void_p(seeds.data_ptr())
            if env_mask is not None:
                if not torch.is_tensor(env_mask):
                    env_mask = torch.from_numpy(np.ascontiguousarray(env_mask, dtype=np.uint8)).to(self.device)
                if tuple(env_mask.shape) != (n,) or env_mask.dtype not in (torch.bool, torch.uint8) or env_mask.device != self.device:
                    raise ValueError(f'env_mask must be a bool or uint8 tensor [{n}] on {self.device}')
                env_mask = env_mask.to(torch.uint8).contiguous()        # (a bool tensor -- this object's own `done`, which the reset's outputs rewrite -- is copied)
                mp = ctypes.c_void_p(env_mask.data_ptr())
            rc = self.lib.cc4_stream_wait(self._h, s) or self.lib.cc4_reset_device(self._h, sp, mp)
            if rc:
                self.venv._chk(rc, 'cc4_reset_device')
            self._outputs(s)
        return self.obs, self._info()

    def reset(self, seeds=None, env_mask=None):
        """seeds / env_mask as CC4VecEnv.reset (NumPy arrays, a scalar, None: cc4_reset, which waits for the device) -- or tensors on the env's
        device (seeds any integer dtype, env_mask bool or uint8, e.g. env.reset(env_mask=env.done)): cc4_reset_device on the current stream, no
        host wait."""
        if torch.is_tensor(seeds) or torch.is_tensor(env_mask):
            return self._reset_device(seeds, env_mask)
        with torch.cuda.device(self.device):
            s = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            # the reset rewrites rows the last step's kernels may still read, and the outputs go into tensors the caller's stream may
            # still read: everything on s first (cc4_reset itself waits for the device before it returns)
            self.venv._chk(self.lib.cc4_stream_wait(self._h, s), 'cc4_stream_wait')
            sp = mp = None
            if seeds is not None:
                if np.isscalar(seeds):
                    seeds = np.uint64(seeds) + np.arange(self.num_envs, dtype=np.uint64)
                seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
                assert seeds.shape == (self.num_envs,)
                sp = seeds.ctypes.data_as(ctypes.c_void_p)
            if env_mask is not None:
                env_mask = np.ascontiguousarray(env_mask, dtype=np.uint8)
                assert env_mask.shape == (self.num_envs,)
                mp = env_mask.ctypes.data_as(ctypes.c_void_p)
            self.venv._chk(self.lib.cc4_reset(self._h, sp, mp), 'cc4_reset')
            self._outputs(s)
        return self.obs, self._info()

    def step(self, actions, messages=None, red_actions=None):
        with torch.cuda.device(self.device):
            if tuple(actions.shape) != (self.num_envs, L.NUM_BLUE) or (messages is not None and tuple(messages.shape) != tuple(self._messages.shape)):
                raise ValueError(f'actions must be [{self.num_envs}, {L.NUM_BLUE}] and messages [{self.num_envs}, {L.NUM_BLUE}, {L.MSG_LEN}]')
            if red_actions is not None:
                shape = (self.num_envs, L.NUM_RED, L.RED_ACT_WORDS)
                if (not torch.is_tensor(red_actions) or tuple(red_actions.shape) != shape or red_actions.dtype.is_floating_point
                        or red_actions.dtype == torch.bool or red_actions.device != self.device):
                    raise ValueError(f'red_actions must be an integer tensor {list(shape)} (type, host, arg, session) on {self.device}')
                if self._red is None:
                    self._red = torch.zeros(shape, dtype=torch.int32, device=self.device)
            s = torch.cuda.current_stream(self.device)
            # staging copies on s: any integer dtype cast, and the env no longer depends on the lifetime of the caller's tensors
            self._actions.copy_(actions)
            if messages is not None:
                self._messages.copy_(messages)
            lib, h, sp = self.lib, self._h, ctypes.c_void_p(s.cuda_stream)
            mp = self._p_msg if messages is not None else None
            if red_actions is None:
                rc = lib.cc4_stream_wait(h, sp) or lib.cc4_step_device(h, self._p_act, mp)
            else:
                if red_actions.dtype != torch.int32:     # (a value beyond int32 stays out of range instead of wrapping into it)
                    red_actions = red_actions.clamp(-2 ** 31, 2 ** 31 - 1)
                self._red.copy_(red_actions)
                rc = lib.cc4_stream_wait(h, sp) or lib.cc4_step_red_device(h, self._p_act, mp, ctypes.c_void_p(self._red.data_ptr()))
            if rc:
                self.venv._chk(rc, 'cc4_step_device' if red_actions is None else 'cc4_step_red_device')
            self._outputs(sp)
        return self.obs, self.reward, self.done, self._info()

    def step_plan(self, actions, messages=None, record_obs=False):
        """k steps with the blue actions known in advance (cc4_run_plan_device: one launch of the persistent kernel where it serves the batch,
        venv.plan_kernel_for(k)): actions integer tensor [k, N, 5] on the env's device, messages optional [k, N, 5, 8] of 0 / 1.
        Returns (obs, rewards [k, N] float32, dones [k, N] bool, info): obs, info['action_mask'], info['err'] are the env's reused tensors after the
        LAST step (masks refreshed for every episode the plan regenerated; err: every flag some step raised), rewards / dones fresh tensors,
        info['obs_seq'] [k, N, 578] obs_dtype -- the observations after every step -- with record_obs.  Ordered on the current stream both
        ways like step(); no host copy, no host wait."""
        n = self.num_envs
        if (not torch.is_tensor(actions) or actions.dim() != 3 or actions.shape[0] < 1 or tuple(actions.shape[1:]) != (n, L.NUM_BLUE)
                or actions.dtype.is_floating_point or actions.dtype == torch.bool or actions.device != self.device):
            raise ValueError(f'actions must be an integer tensor [k, {n}, {L.NUM_BLUE}] (k >= 1) on {self.device}')
        k = int(actions.shape[0])
        if messages is not None and (not torch.is_tensor(messages) or tuple(messages.shape) != (k, n, L.NUM_BLUE, L.MSG_LEN)
                                     or messages.dtype.is_floating_point or messages.device != self.device):
            raise ValueError(f'messages must be an integer or bool tensor [{k}, {n}, {L.NUM_BLUE}, {L.MSG_LEN}] on {self.device}')
        with torch.cuda.device(self.device):
            s = torch.cuda.current_stream(self.device)
            vp = ctypes.c_void_p
            # on s: casts (no copy when the plan is int32 / uint8 and contiguous already) and the trajectory's tensors; the allocator keeps them
            # on s, whose later work cc4_stream_signal orders behind the plan
            plan = actions.to(torch.int32).contiguous()
            msgs = messages.to(torch.uint8).contiguous() if messages is not None else None
            rewards = torch.empty((k, n), dtype=torch.float32, device=self.device)
            dones = torch.empty((k, n), dtype=torch.bool, device=self.device)
            packed = torch.empty((k, n, L.OBS_PACKED_BYTES), dtype=torch.uint8, device=self.device) if record_obs else None
            lib, h, sp = self.lib, self._h, vp(s.cuda_stream)
            rc = lib.cc4_stream_wait(h, sp) or lib.cc4_run_plan_device(h, k, vp(plan.data_ptr()), vp(msgs.data_ptr()) if msgs is not None else None,
                                                                       vp(rewards.data_ptr()), vp(dones.data_ptr()),
                                                                       vp(packed.data_ptr()) if record_obs else None)
            if rc:
                self.venv._chk(rc, 'cc4_run_plan_device')
            info = self._info()
            if record_obs:
                seq = torch.empty((k, n, L.OBS_PER_ENV), dtype=self.obs_dtype, device=self.device)
                self.venv._chk(lib.cc4_unpack_rows_device(h, k * n, vp(packed.data_ptr()), self._dt, vp(seq.data_ptr())), 'cc4_unpack_rows_device')
                info['obs_seq'] = seq
            self._outputs(sp)       # (signals s: what the caching allocator hands out on s once plan / msgs / packed die is ordered behind their readers)
        return self.obs, rewards, dones, info

    @property
    def snapshot_bytes(self):
        """cc4_snapshot_bytes: bytes of one snapshot slot (header, hot row, cold row, the outputs of the last step)."""
        return int(self.lib.cc4_snapshot_bytes(self._h))

    def new_bank(self, capacity):
        return torch.zeros((int(capacity), self.snapshot_bytes), dtype=torch.uint8, device=self.device)

    def _index(self, x, what):
        if not torch.is_tensor(x) or x.dim() != 1 or x.dtype.is_floating_point or x.dtype == torch.bool or x.device != self.device:
            raise ValueError(f'{what} must be a 1-D integer tensor on {self.device}')
        return x.to(torch.int32).contiguous()       # (on the current stream, as step() casts its actions)

    def _bank(self, bank):
        if (not torch.is_tensor(bank) or bank.dtype != torch.uint8 or bank.dim() != 2 or bank.shape[1] != self.snapshot_bytes
                or not bank.is_contiguous() or bank.device != self.device):
            raise ValueError(f'a bank is a contiguous uint8 tensor [capacity, {self.snapshot_bytes}] on {self.device} (new_bank)')
        return ctypes.c_void_p(bank.data_ptr()), int(bank.shape[0])

    def _copy(self, src, dst, src_bank=None, dst_bank=None, seeds=None):
        with torch.cuda.device(self.device):
            s = torch.cuda.current_stream(self.device)
            src, dst = self._index(src, 'source indices'), self._index(dst, 'destination indices')
            if src.shape != dst.shape:
                raise ValueError('source and destination indices must have the same length')
            sb, sc = self._bank(src_bank) if src_bank is not None else (None, 0)
            db, dc = self._bank(dst_bank) if dst_bank is not None else (None, 0)
            sd = None
            if seeds is not None:
                if not torch.is_tensor(seeds) or seeds.shape != src.shape or seeds.device != self.device:
                    raise ValueError('seeds must be a tensor with one entry per copy on the env\'s device')
                seeds = (seeds.view(torch.int64) if seeds.dtype == torch.uint64 else seeds.to(torch.int64)).contiguous()
                sd = ctypes.c_void_p(seeds.data_ptr())
            lib, h, sp = self.lib, self._h, ctypes.c_void_p(s.cuda_stream)
            rc = lib.cc4_stream_wait(h, sp) or lib.cc4_copy_episodes_device(h, int(src.numel()), sb, sc, ctypes.c_void_p(src.data_ptr()), db, dc,
                                                                               ctypes.c_void_p(dst.data_ptr()), sd)
            if rc:
                self.venv._chk(rc, 'cc4_copy_episodes_device')
            self._outputs(sp)
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

    def _view(self, entry, ids, bank, out, specs, *extra):
        """What the tensor methods of the derived views share.  entry: the cc4_*_device entry point; ids, bank, out as state_features() documents
        them; specs: (shape of one entry, dtype, required alignment in bytes) of the view's two tensors; extra: arguments in front of the two output
        pointers.  Ordered on the current stream both ways like step(); no host copy, no host wait."""
        with torch.cuda.device(self.device):
            s = torch.cuda.current_stream(self.device)
            vp = ctypes.c_void_p
            bp, cap = self._bank(bank) if bank is not None else (None, 0)
            if ids is not None:
                ids = self._index(ids, 'ids')
                n, ip = int(ids.numel()), vp(ids.data_ptr())
            else:
                n, ip = (cap if bank is not None else self.num_envs), None
            shapes = [(n,) + tuple(tail) for tail, _dt, _al in specs]
            if out is None:
                a, b = (torch.empty(shp, dtype=dt, device=self.device) for shp, (_tail, dt, _al) in zip(shapes, specs))
            else:
                a, b = out
                for x, shp, (_tail, dt, al) in zip((a, b), shapes, specs):
                    if (not torch.is_tensor(x) or tuple(x.shape) != shp or x.dtype != dt or x.device != self.device or not x.is_contiguous()
                            or x.data_ptr() % al):
                        want = ', '.join(f'{str(dt_).replace("torch.", "")} {list(shp_)} ({al_}-byte aligned)' for shp_, (_t, dt_, al_) in zip(shapes, specs))
                        raise ValueError(f'out must be contiguous tensors ({want}) on {self.device}')
            lib, h, sp = self.lib, self._h, vp(s.cuda_stream)
            rc = lib.cc4_stream_wait(h, sp) or getattr(lib, entry)(h, bp, cap, ip, n, *extra, vp(a.data_ptr()), vp(b.data_ptr()))
            if rc:
                self.venv._chk(rc, entry)
            self.venv._chk(lib.cc4_stream_signal(h, sp), 'cc4_stream_signal')
        return a, b

    def state_features(self, ids=None, bank=None, out=None):
        """The privileged global state (cc4_state_features_device, include/cc4.h; columns and words: state_features.HOST_COLUMNS / GLOBAL_WORDS)
        as tensors on the env's device: (hosts [n, 137, 16] uint8, glob [n, 32] int32).  ids: 1-D integer tensor on the device -- episodes of
        the env, or with bank= (a new_bank tensor) the slots of saved episodes, read where they lie; None: all episodes / all slots.
        out=(hosts, glob) reuses the caller's tensors.  Ordered on the current stream both ways like step(); no host copy, no host wait.  A
        faulty entry (an index out of range, a slot never written or written by another configuration) gives an all-zero row, and
        check_errors() raises CC4EngineError for it."""
        return self._view('cc4_state_features_device', ids, bank, out, (((L.FEAT_HOSTS, L.FEAT_PER_HOST), torch.uint8, 1), ((L.FEAT_GLOBAL,), torch.int32, 1)))

    def red_view(self, ids=None, bank=None, out=None):
        """What each red agent knows (cc4_red_view_device, include/cc4.h; columns and words: red_view.HOST_COLUMNS / SCALAR_WORDS) as tensors on
        the env's device: (hosts [n, 6, 137, 8] uint8, scalars [n, 6, 16] int32).  ids, bank, out and the ordering on the current stream as
        state_features(); no host copy, no host wait.  A faulty entry gives all-zero rows, and check_errors() raises CC4EngineError for it."""
        return self._view('cc4_red_view_device', ids, bank, out, (((L.NUM_RED, L.RED_VIEW_HOSTS, L.RED_VIEW_PER_HOST), torch.uint8, 1),
                                                                 ((L.NUM_RED, L.RED_VIEW_SCALARS), torch.int32, 1)))

    def blue_view(self, ids=None, bank=None, out=None):
        """Blue's own knowledge (cc4_blue_view_device, include/cc4.h; columns and words: blue_view.HOST_COLUMNS / SCALAR_WORDS) as tensors on the
        env's device: (hosts [n, 5, 137, 8] uint8, scalars [n, 5, 16] int32) -- busy, the outcome of the agent's own action, what Analyse found,
        the deployed decoy, suspicious pids, and with enable_event_log() the Monitor's entries per host (scalars[..., 10]: whether they are
        filled).  ids, bank, out and the ordering on the current stream as state_features(); no host copy, no host wait.  A faulty entry gives
        all-zero rows, and check_errors() raises CC4EngineError for it."""
        return self._view('cc4_blue_view_device', ids, bank, out, (((L.NUM_BLUE, L.BLUE_VIEW_HOSTS, L.BLUE_VIEW_PER_HOST), torch.uint8, 1),
                                                                  ((L.NUM_BLUE, L.BLUE_VIEW_SCALARS), torch.int32, 1)))

    def blue_edges(self, ids=None, bank=None, out=None, max_edges=L.BLUE_EDGES_MAX):
        """The Monitor's connection entries of the step just taken as edge lists (cc4_blue_edges_device, include/cc4.h; columns and words:
        blue_edges.COLUMNS / WORDS) as tensors on the env's device: (edges [n, max_edges, 8] int32, counts [n, 8] int32) -- agent, reporting
        host, local host, remote host, the two ports, how often, the slot within the agent's segment; sorted, merged, -1 past the last edge
        (edges[..., 0] >= 0 is the mask; counts[:, 5] > max_edges shows a truncated list).  blue_edges.to_edge_index() makes the [2, M] node
        pairs of a graph layer from it.  The per-step log must be on (enable_event_log(): the env then runs the full builds of its step kernel,
        one launch per step, and leaves the one-launch forms of run / plan calls); without it every row is -1 and counts[:, 6] is 0.
        ids, bank, out and the ordering on the current stream as state_features(); no host copy, no host wait.  A faulty entry gives -1 rows
        and zero counts, and check_errors() raises CC4EngineError for it."""
        max_edges = int(max_edges)
        if not 1 <= max_edges <= L.BLUE_EDGES_MAX:
            raise ValueError(f'max_edges must be 1 .. {L.BLUE_EDGES_MAX}, got {max_edges}')
        return self._view('cc4_blue_edges_device', ids, bank, out, (((max_edges, L.BLUE_EDGES_COLUMNS), torch.int32, 16), ((L.BLUE_EDGES_WORDS,), torch.int32, 1)),
                          max_edges)

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
        from .action_sampling import check_temperature, flags_of
        temperature = check_temperature(temperature)
        n = int(ids.numel()) if torch.is_tensor(ids) else (int(bank.shape[0]) if torch.is_tensor(bank) else self.num_envs)
        code, lp = 3, None
        if logits is not None:
            if (not torch.is_tensor(logits) or tuple(logits.shape) != (n, L.MASK_PER_ENV) or logits.dtype not in _LOGIT_DTYPES
                    or logits.device != self.device or not logits.is_contiguous()):
                raise ValueError(f'logits must be a contiguous float16, bfloat16 or float32 tensor [{n}, {L.MASK_PER_ENV}] on {self.device}')
            code, lp = _LOGIT_DTYPES[logits.dtype], ctypes.c_void_p(logits.data_ptr())
        if t is None:
            t, self._sample_t = self._sample_t, self._sample_t + 1
        return self._view('cc4_sample_actions_device', ids, bank, out, (((L.NUM_BLUE,), torch.int32, 4), ((L.NUM_BLUE, 2), torch.float32, 4)),
                          code, lp, int(seed) & (2 ** 64 - 1), int(t) & 0xFFFFFFFF, temperature, flags_of(greedy, busy_aware))

    def evaluate_actions(self, logits, mask, actions, temperature=1.0):
        """action_logp.evaluate_actions: (logp, entropy) of stored actions under new logits, differentiable with respect to the logits -- the
        update's half of sample_actions().  A pure function of its tensors (the env is not read); action_logp.check_errors() reports refusals."""
        from .action_logp import evaluate_actions
        return evaluate_actions(logits, mask, actions, temperature)

    def enable_event_log(self, on=True):
        """CC4VecEnv.enable_event_log (cc4_enable_event_log): record the HostEvents entries of every step, which fills the event columns of
        blue_view() (entries per host, ports, remote hosts, the deployed decoy).  The log has a price: an env with the log on runs the full
        builds of its step kernel, one launch per step, and leaves the one-launch forms of run / plan calls.  Without it blue_view() still
        carries busy / success / what Analyse found / sus_pids."""
        with torch.cuda.device(self.device):
            s = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self.venv._chk(self.lib.cc4_stream_wait(self._h, s), 'cc4_stream_wait')
            self.venv.enable_event_log(on)

    def reward_terms(self, ids=None, bank=None, out=None):
        """Why the last step's reward was what it was (cc4_reward_terms_device, include/cc4.h; columns and words: reward_terms.TERM_COLUMNS /
        WORDS) as tensors on the env's device: (terms [n, 9, 4] int32, words [n, 16] int32) -- per subnet the LocalWork-failed,
        AccessService-failed and Impact penalties and the number of charged events; valid, step_count, phase, brm, action cost, the five blue
        agents' shares, the unowned rest and the agents' own Restore costs.  words[:, 0] is 1 where the last step recorded
        (enable_reward_terms(), or an env that steps with red_actions); then words[:, 3] + words[:, 4] == reward.  ids, bank, out and the
        ordering on the current stream as state_features(); no host copy, no host wait.  A faulty entry gives all-zero rows, and
        check_errors() raises CC4EngineError for it."""
        return self._view('cc4_reward_terms_device', ids, bank, out, (((L.REWARD_SUBNETS, L.REWARD_COLS), torch.int32, 16), ((L.REWARD_WORDS,), torch.int32, 16)))

    def enable_reward_terms(self, on=True):
        """CC4VecEnv.enable_reward_terms (cc4_enable_reward_terms): record the pieces of every step's reward, which reward_terms() turns into
        tensors.  The record has a price: the env runs the full builds of its step kernel, one launch per step, and leaves the one-launch
        forms of run / plan calls (after a plan only the last step's terms exist).  An env that steps with red_actions records anyway."""
        with torch.cuda.device(self.device):
            s = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self.venv._chk(self.lib.cc4_stream_wait(self._h, s), 'cc4_stream_wait')
            self.venv.enable_reward_terms(on)
            self.venv._chk(self.lib.cc4_stream_signal(self._h, s), 'cc4_stream_signal')

    def set_opponents(self, red=None, green=None, blue=None):
        """Assign opponent classes per episode from the device (cc4_set_policies_device, include/cc4.h): red (0..3), green (0..1), blue (0..1) each
        an integer tensor [N] on the env's device or None (keep); an entry may be L.POLICY_KEEP or L.POLICY_DEFAULT.  Takes effect at each
        episode's next regeneration (reset, autoreset), never mid-episode.  On the current stream, no host wait; a refused entry (a class out of
        range) leaves its episode as it was, and check_errors() raises CC4EngineError for it."""
        n = self.num_envs
        with torch.cuda.device(self.device):
            s = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            ptrs, keep = [], []
            for x, what in ((red, 'red'), (green, 'green'), (blue, 'blue')):
                if x is None:
                    ptrs.append(None)
                    continue
                if not torch.is_tensor(x) or tuple(x.shape) != (n,) or x.dtype.is_floating_point or x.dtype == torch.bool or x.device != self.device:
                    raise ValueError(f'{what} must be an integer tensor [{n}] on {self.device}')
                x = x.clamp(-128, 127).to(torch.int8).contiguous()      # (a value beyond int8 stays out of range instead of wrapping into it)
                keep.append(x)
                ptrs.append(ctypes.c_void_p(x.data_ptr()))
            rc = self.lib.cc4_stream_wait(self._h, s) or self.lib.cc4_set_policies_device(self._h, *ptrs)
            if rc:
                self.venv._chk(rc, 'cc4_set_policies_device')
            self.venv._chk(self.lib.cc4_stream_signal(self._h, s), 'cc4_stream_signal')

    def opponents(self):
        """(live, assigned): two fresh [N, 3] int8 tensors of (red, green, blue) classes -- what every episode runs now, and what it regenerates
        into (L.POLICY_DEFAULT where it carries no assignment).  On the current stream, no host wait."""
        with torch.cuda.device(self.device):
            s = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            live = torch.empty((self.num_envs, 3), dtype=torch.int8, device=self.device)
            assigned = torch.empty((self.num_envs, 3), dtype=torch.int8, device=self.device)
            rc = self.lib.cc4_stream_wait(self._h, s) or self.lib.cc4_policies_device(self._h, ctypes.c_void_p(live.data_ptr()), ctypes.c_void_p(assigned.data_ptr()))
            if rc:
                self.venv._chk(rc, 'cc4_policies_device')
            self.venv._chk(self.lib.cc4_stream_signal(self._h, s), 'cc4_stream_signal')
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
