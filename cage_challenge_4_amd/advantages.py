"""Advantages, returns and loss weights of a STORED rollout (include/cc4.h, cc4_gae_device): the step of a PPO / A2C iteration between the rollout
and the update -- generalised advantage estimation in this env's own conventions, as a pure function of the tensors the rollout stored.

T rows, N episodes, A value heads per episode (values [T, N]: one, a team critic; values [T, N, A] with A <= 8: e.g. one per blue agent).
  autoreset=True   CC4TorchVecEnv(autoreset=True): the call that follows a `done` takes no step -- it regenerates the episode and returns reward 0
                   and the new scenario's first observation -- so the row stored for it is no transition (a skip row): adv 0, ret = its own
                   value, weight 0.  Which rows those are is read off the stored dones (and done0, the env's done before the first call).
  bootstrap=True   `done` here is always truncation (episodes end at the horizon only) and the observation returned with it is the old episode's
                   last one, which the skip row stores: the done row bootstraps from that row's value instead of 0 (needs autoreset=True).
  autoreset=False  the plain layout: a done cuts the trace, every row is a transition, done0 is ignored.
  weight           0 on skip rows and where the stored action is -1 ("submitted nothing": evaluate_actions gives it zero logp and no gradient).
Per column, backwards from A_next = 0, v_next = last_value:  delta = r + gamma vb - v,  adv = delta + gamma lam An,  ret = adv + v, with vb = v_next
(after a done row: 0, or v_next with bootstrap) and An = A_next (after a done row: 0); csrc/cc4_gae.h states it to the rounding.

Three ways to the same numbers:
  gae(rewards, values, last_value, dones, gamma=, lam=, ...)   the HIP kernel (k_gae), one launch on torch's current stream, float32
  from_arrays(...)                                              the same definition compiled for the host (cc4_gae_host) over NumPy arrays, no GPU
  reference(...)                                                a float64 NumPy restatement written another way: episode segments, explicit sums

Importing this module imports neither torch nor the library; gae() imports torch when it is called."""
import numpy as np
from . import _lib as L
from . import _tensors as TS

SKIP_AFTER_DONE, BOOTSTRAP_DONE, MAX_HEADS = L.GAE_SKIP_AFTER_DONE, L.GAE_BOOTSTRAP_DONE, L.GAE_MAX_HEADS
DTYPE_CODES = TS.DTYPE_CODES      # the codes of cc4_policy_outputs
launches = {'gae': 0}          # kernels this module has enqueued (what a caller's test counts)


def check_params(gamma, lam, autoreset=True, bootstrap=False):
    """(gamma, lam, flags) or ValueError: gamma and lam are numbers in [0, 1], bootstrap needs autoreset."""
    out = []
    for name, x in (('gamma', gamma), ('lam', lam)):
        if isinstance(x, (bool, str)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError(f'{name} must be a number in [0, 1], got {x!r}')
        x = float(x)
        if not 0.0 <= x <= 1.0:          # (a NaN fails the compare)
            raise ValueError(f'{name} must be in [0, 1], got {x}')
        out.append(x)
    if bootstrap and not autoreset:
        raise ValueError('bootstrap=True needs autoreset=True: only the autoreset layout stores the observation a done row ended on')
    return out[0], out[1], (SKIP_AFTER_DONE if autoreset else 0) | (BOOTSTRAP_DONE if bootstrap else 0)


def _shapes(shape_of, rewards, values, last_value, dones, done0, actions):
    """(T, N, A, reward_heads) from the shapes, or ValueError.  shape_of(x): the shape of an array or tensor as a tuple."""
    vs = shape_of(values)
    if len(vs) not in (2, 3) or (len(vs) == 3 and not 1 <= vs[2] <= MAX_HEADS):
        raise ValueError(f'values must have shape [T, N] or [T, N, A] with 1 <= A <= {MAX_HEADS}, got {list(vs)}')
    T, N = vs[:2]
    A = vs[2] if len(vs) == 3 else 1
    if shape_of(rewards) not in ((T, N), vs):
        raise ValueError(f'rewards must have shape {[T, N]} (shared by the heads) or {list(vs)}, got {list(shape_of(rewards))}')
    heads = 1 if shape_of(rewards) == (T, N) else A
    if shape_of(last_value) != vs[1:]:
        raise ValueError(f'last_value must have shape {list(vs[1:])}, got {list(shape_of(last_value))}')
    if shape_of(dones) != (T, N):
        raise ValueError(f'dones must have shape {[T, N]}, got {list(shape_of(dones))}')
    if done0 is not None and shape_of(done0) != (N,):
        raise ValueError(f'done0 must have shape {[N]}, got {list(shape_of(done0))}')
    if actions is not None and shape_of(actions) != vs:
        raise ValueError(f'actions must have shape {list(vs)}, got {list(shape_of(actions))}')
    if N * A > 2 ** 31 - 1:
        raise ValueError(f'N * A must not exceed {2 ** 31 - 1}, got {N * A}')
    return T, N, A, heads


def _arrays(rewards, values, last_value, dones, done0, actions):
    arrs = [np.asarray(x) for x in (rewards, values, last_value, dones)]
    done0 = None if done0 is None else np.asarray(done0)
    actions = None if actions is None else np.asarray(actions)
    for name, x, kinds in (('rewards', arrs[0], 'f'), ('values', arrs[1], 'f'), ('last_value', arrs[2], 'f'), ('dones', arrs[3], 'bu'),
                           ('done0', done0, 'bu'), ('actions', actions, 'iu')):
        if x is not None and x.dtype.kind not in kinds:
            raise ValueError(f'{name} must be {"floating point" if kinds == "f" else "bool or uint8" if kinds == "bu" else "integers"}, got {x.dtype}')
    dims = _shapes(lambda x: tuple(x.shape), *arrs, done0, actions)
    return arrs, done0, actions, dims


def reference(rewards, values, last_value, dones, *, gamma, lam, done0=None, actions=None, autoreset=True, bootstrap=False):
    """The definition in float64 NumPy, written from the prose of include/cc4.h WITHOUT the backward recurrence: every column is cut into episode
    segments at its done rows, the skip rows are dropped, and per segment delta_t = r_t + gamma vb_t - v_t and adv_t = sum over l of
    (gamma lam)^l delta_{t+l} as the explicit sum.  Arrays as from_arrays; the values are taken as they are carried.  Returns (adv, ret, weight)
    in the shape of values: float64, float64, bool."""
    gamma, lam, flags = check_params(gamma, lam, autoreset, bootstrap)
    (rw, vl, lv, dn), done0, actions, (T, N, A, heads) = _arrays(rewards, values, last_value, dones, done0, actions)
    g = float(np.float32(gamma))
    gl = g * float(np.float32(lam))
    v = vl.astype(np.float64).reshape(T, N, A)
    r = np.broadcast_to(rw.astype(np.float64).reshape(T, N, heads), (T, N, A))
    last = lv.astype(np.float64).reshape(N, A)
    d = dn.reshape(T, N) != 0
    first = np.zeros(N, bool) if done0 is None else done0 != 0
    prev = np.concatenate((first[None], d[:-1]), axis=0) if T else d
    skip = prev if autoreset else np.zeros((T, N), bool)
    adv, ret = np.zeros((T, N, A)), v.copy()
    for n in range(N):
        steps = np.nonzero(~skip[:, n])[0]                    # the rows that are transitions
        ends = np.nonzero(d[steps, n])[0]                      # ... and which of them end an episode
        bounds = np.concatenate(([0], ends + 1, [steps.size]))
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            seg = steps[lo:hi]                                 # one episode segment: consecutive rows, a done on the last one or none
            if seg.size == 0:
                continue
            assert (np.diff(seg) == 1).all()
            t_end = seg[-1]
            after = v[t_end + 1, n] if t_end + 1 < T else last[n]          # the value of the row after the segment's last
            if d[t_end, n] and not bootstrap:
                after = np.zeros(A)
            nxt = np.concatenate((v[seg[1:], n], after[None]), axis=0)
            with np.errstate(invalid='ignore', over='ignore'):
                delta = r[seg, n] + g * nxt - v[seg, n]
                pw = gl ** np.arange(seg.size)
                for k, t in enumerate(seg):
                    adv[t, n] = (pw[:seg.size - k, None] * delta[k:]).sum(axis=0)
                ret[seg, n] = adv[seg, n] + v[seg, n]
    weight = np.broadcast_to(~skip[:, :, None], (T, N, A)).copy()
    if actions is not None:
        weight &= actions.reshape(T, N, A) != -1
    shape = vl.shape
    return adv.reshape(shape), ret.reshape(shape), weight.reshape(shape)


def from_arrays(rewards, values, last_value, dones, *, gamma, lam, done0=None, actions=None, autoreset=True, bootstrap=False):
    """The host function over NumPy arrays (cc4_gae_host): rewards [T, N] or the shape of values, floating point; values [T, N] or [T, N, A] and
    last_value [N] or [N, A], floating point, taken as float32; dones [T, N] and done0 [N] bool or uint8; actions integers in the shape of values
    or None.  Returns (adv, ret, weight) in the shape of values: float32, float32, bool.  No GPU."""
    gamma, lam, flags = check_params(gamma, lam, autoreset, bootstrap)
    (rw, vl, lv, dn), done0, actions, (T, N, A, heads) = _arrays(rewards, values, last_value, dones, done0, actions)
    if T == 0 or N == 0:
        return np.zeros(vl.shape, np.float32), np.zeros(vl.shape, np.float32), np.zeros(vl.shape, np.bool_)
    lib = L.load()
    rw, vl, lv = (np.ascontiguousarray(x, np.float32) for x in (rw, vl, lv))
    dn = np.ascontiguousarray(dn).view(np.uint8)
    done0 = None if done0 is None else np.ascontiguousarray(done0).view(np.uint8)
    actions = None if actions is None else np.ascontiguousarray(actions.clip(-2 ** 31, 2 ** 31 - 1), np.int32)
    adv, ret, weight = np.zeros(vl.shape, np.float32), np.zeros(vl.shape, np.float32), np.zeros(vl.shape, np.uint8)
    from .vec_env import as_ptr as p
    rc = lib.cc4_gae_host(p(rw), heads, p(vl), p(lv), p(dn), p(done0), p(actions), T, N, A, gamma, lam, flags, p(adv), p(ret), p(weight))
    if rc != 0:
        raise L.CC4Error(f'cc4_gae_host failed (rc={rc})')
    return adv, ret, weight.view(np.bool_)


def _check_tensors(torch, rewards, values, last_value, dones, done0, actions, out):
    """(T, N, A, reward_heads, dtype code) or ValueError: kinds, shapes and dtypes first, then contiguity and devices."""
    given = [('rewards', rewards), ('values', values), ('last_value', last_value), ('dones', dones)]
    given += [(k, x) for k, x in (('done0', done0), ('actions', actions)) if x is not None]
    for name, x in given:
        TS.check_tensor(torch, name, x, contiguous=False)
    T, N, A, heads = _shapes(lambda x: tuple(x.shape), rewards, values, last_value, dones, done0, actions)
    codes = TS.torch_codes(torch)
    TS.check_tensor(torch, 'values', values, dtypes=tuple(codes), contiguous=False)
    if last_value.dtype != values.dtype:
        raise ValueError(f'last_value must have the dtype of values ({values.dtype}), got {last_value.dtype}')
    for name, x, dtypes in (('rewards', rewards, (torch.float32,)), ('dones', dones, (torch.bool, torch.uint8)), ('done0', done0, (torch.bool, torch.uint8)),
                            ('actions', actions, (torch.int32,))):
        if x is not None:
            TS.check_tensor(torch, name, x, dtypes=dtypes, contiguous=False)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 3 or not all(torch.is_tensor(o) for o in out):
            raise ValueError('out must be the (adv, ret, weight) triple an earlier call returned')
        for name, o, dt in zip(('out: adv', 'out: ret', 'out: weight'), out, (torch.float32, torch.float32, torch.bool)):
            given.append((name, TS.check_tensor(torch, name, o, shape=tuple(values.shape), dtypes=(dt,), contiguous=False)))
    for name, x in given:
        TS.check_tensor(torch, name, x, device='cuda')
    for name, x in given:
        if x.device != values.device:
            raise ValueError(f'{name} must be on the device of values ({values.device}), got {x.device}')
    return T, N, A, heads, codes[values.dtype]


def gae(rewards, values, last_value, dones, *, gamma, lam, done0=None, actions=None, autoreset=True, bootstrap=False, out=None):
    """(adv, ret, weight) of a stored rollout, in the shape of values: float32, float32, bool.  One launch on torch.cuda.current_stream() (k_gae),
    no host wait.  All inputs are contiguous CUDA tensors on one device:
      rewards     float32 [T, N] (shared by the heads) or the shape of values (per head, e.g. the agents' shares of reward_terms)
      values      float16, bfloat16 or float32 [T, N] or [T, N, A], A <= 8: the values the rollout STORED, detached -- they are read as data, and
                  the outputs do not require grad (the value loss is (new value - ret)^2 against the network's new output)
      last_value  [N] or [N, A] in the dtype of values: the value of the observation after the last row
      dones       bool or uint8 [T, N];  done0: [N], the env's done before the rollout's first call (done0 = env.done.clone()), None: all zero
      actions     int32 in the shape of values or None: the stored actions, -1 gives weight 0
      gamma, lam  in [0, 1];  autoreset, bootstrap: the layout (the module's docstring)
      out         the triple an earlier call returned: reused, and returned
    Wrong kinds, shapes, dtypes, devices and parameter ranges raise ValueError before anything is enqueued."""
    import torch
    gamma, lam, flags = check_params(gamma, lam, autoreset, bootstrap)
    T, N, A, heads, code = _check_tensors(torch, rewards, values, last_value, dones, done0, actions, out)
    dev = values.device
    if out is None:
        out = (torch.empty(values.shape, dtype=torch.float32, device=dev), torch.empty(values.shape, dtype=torch.float32, device=dev),
               torch.empty(values.shape, dtype=torch.bool, device=dev))
    adv, ret, weight = out
    if T == 0 or N == 0:          # nothing to do (and an empty tensor has no address to pass)
        return adv, ret, weight
    p = TS.dptr
    TS.pure_call('cc4_gae_device', dev, p(rewards), heads, p(values), code, p(last_value), p(dones), p(done0), p(actions), T, N, A, gamma, lam, flags,
                 p(adv), p(ret), p(weight), count=(launches, 'gae'))
    return adv, ret, weight
