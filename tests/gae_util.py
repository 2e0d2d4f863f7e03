"""What the tests of "advantages and returns of a stored rollout" share: crafted and random inputs, the error bound of a float32 evaluation against
the float64 restatement, and the definition as a learner writes it in PyTorch for the plain layout.

The bound is derived from float32 rounding with u = 2^-24, not from the code under test.  A row performs, in float32, gamma * vb, r + that, - v,
(gamma lam) * An, delta + that (and adv + v for ret); to first order each rounded operation adds u times the magnitude of its result, which the
sum of the magnitudes of the row's terms bounds, and the error of the row after it arrives scaled by gamma lam where the trace is not cut:
    E_t = 4 u (|r| + gamma |vb| + |v| + gamma lam |An| + |adv_t|) + gamma lam [not done] E_{t+1},     E_t = 0 on a skip row
evaluated in float64 along the reference; ret = adv + v adds one more rounding: E_t + u |ret_t|.  The 4 covers the row's rounded operations (and
the one rounding of gamma lam) to first order."""
import numpy as np

from bf16_util import to_bits as to_bf16_bits, upcast  # noqa: F401  (test_gae_device reads both from here)

U32 = 2.0 ** -24


def random_rollout(rng, T, N, A, done_rate=0.15, heads=1, none_rate=0.2, scale=50.0):
    """A stored rollout in the autoreset layout: values of scale `scale`, integer rewards in [-20, 0] (0 on skip rows, as the engine gives them),
    dones at done_rate per transition and 0 on skip rows, done0, actions in [-1, 50) with -1 at none_rate.  A dict of arrays; values float32."""
    dones = np.zeros((T, N), np.uint8)
    done0 = (rng.random(N) < done_rate).astype(np.uint8)
    prev = done0.copy()
    for t in range(T):
        dones[t] = np.where(prev != 0, 0, rng.random(N) < done_rate)
        prev = dones[t]
    rshape = (T, N) if heads == 1 else (T, N, A)
    rewards = -rng.integers(0, 21, rshape).astype(np.float32)
    skip = np.concatenate((done0[None], dones[:-1]), axis=0) != 0 if T else np.zeros((0, N), bool)
    rewards[skip] = 0.0
    values = (rng.standard_normal((T, N, A)) * scale).astype(np.float32)
    last = (rng.standard_normal((N, A)) * scale).astype(np.float32)
    actions = rng.integers(0, 50, (T, N, A)).astype(np.int32)
    actions[rng.random((T, N, A)) < none_rate] = -1
    return dict(rewards=rewards, values=values, last_value=last, dones=dones, done0=done0, actions=actions)


def force_events(rng, ro):
    """Make sure a rollout (T >= 1) holds at least one done, one skip row and one -1 action; T == 1: done0 gives the skip row."""
    T, N, A = ro['values'].shape
    n = int(rng.integers(0, N))
    ro['actions'][T - 1, n, int(rng.integers(0, A))] = -1
    if T >= 2:
        n = int(rng.integers(0, N))
        ro['dones'][T - 2, n], ro['dones'][T - 1, n] = 1, 0
        if T >= 3:
            ro['dones'][T - 3, n] = 0
        if T == 2:
            ro['done0'][n] = 0
    else:
        a, b = (0, 0) if N == 1 else (0, 1)
        ro['done0'][a], ro['dones'][0, b] = 1, 1
        if N > 1:
            ro['done0'][b] = 0
    return ro


def counts(ro):
    """(dones, skip rows, -1 actions) of a rollout in the autoreset layout."""
    T = ro['dones'].shape[0]
    prev = np.concatenate((ro['done0'][None], ro['dones'][:-1]), axis=0) if T else ro['dones']
    return int((ro['dones'] != 0).sum()), int((prev != 0).sum()), int((ro['actions'] == -1).sum())


def bound(ro, ref_adv, ref_ret, gamma, lam, autoreset, bootstrap, use_done0=True):
    """(E_adv, E_ret) in the shape [T, N, A]: the bound of the module's docstring along the reference's adv / ret (float64)."""
    v = upcast(ro['values']).astype(np.float64)
    T, N, A = v.shape
    r = np.broadcast_to(ro['rewards'].astype(np.float64).reshape(T, N, -1), (T, N, A))
    last = upcast(ro['last_value']).astype(np.float64)
    d = ro['dones'] != 0
    first = ro['done0'] != 0 if use_done0 and ro.get('done0') is not None else np.zeros(N, bool)
    prev = np.concatenate((first[None], d[:-1]), axis=0) if T else d
    skip = prev if autoreset else np.zeros((T, N), bool)
    adv = np.asarray(ref_adv, np.float64).reshape(T, N, A)
    ret = np.asarray(ref_ret, np.float64).reshape(T, N, A)
    g, gl = gamma, gamma * lam
    E = np.zeros((T, N, A))
    E_next = np.zeros((N, A))
    for t in range(T - 1, -1, -1):
        v_next = v[t + 1] if t + 1 < T else last
        a_next = adv[t + 1] if t + 1 < T else np.zeros((N, A))
        dt = d[t][:, None]
        vb = np.where(dt, v_next if bootstrap else 0.0, v_next)
        an = np.where(dt, 0.0, a_next)
        with np.errstate(invalid='ignore'):
            e = 4 * U32 * (np.abs(r[t]) + g * np.abs(vb) + np.abs(v[t]) + gl * np.abs(an) + np.abs(adv[t])) + gl * np.where(dt, 0.0, E_next)
        E[t] = np.where(skip[t][:, None], 0.0, e)
        E_next = E[t]
    return E, E + U32 * np.abs(ret)


def check(got_adv, got_ret, ro, gamma, lam, autoreset, bootstrap, what, ref=None, use_done0=True):
    """adv / ret within the bound of the reference; returns the worst |err| / E of adv (for the record)."""
    from cage_challenge_4_amd import advantages as AD
    if ref is None:
        ref = AD.reference(ro['rewards'], upcast(ro['values']), upcast(ro['last_value']), ro['dones'], gamma=gamma, lam=lam,
                           done0=ro['done0'] if use_done0 else None, autoreset=autoreset, bootstrap=bootstrap)
    ra, rr = ref[0], ref[1]
    Ea, Er = bound(ro, ra, rr, gamma, lam, autoreset, bootstrap, use_done0)
    ea = np.abs(np.asarray(got_adv, np.float64).reshape(Ea.shape) - ra.reshape(Ea.shape))
    er = np.abs(np.asarray(got_ret, np.float64).reshape(Ea.shape) - rr.reshape(Ea.shape))
    worst = float((ea / np.maximum(Ea, 1e-300)).max()) if ea.size else 0.0
    print(f'{what}: max |adv - ref| {ea.max() if ea.size else 0:.3g}, worst |err| / E {worst:.3g}')
    assert (ea <= Ea).all(), f'{what}: adv outside the bound, worst |err| / E {worst:.3g}'
    assert (er <= Er).all(), f'{what}: ret outside the bound'
    return worst


def learner_loop(torch, rewards, values, last_value, dones, gamma, lam):
    """The plain layout as a learner writes it in PyTorch: a reverse loop over T with torch.where, in the dtype and on the device of `values`
    (rewards broadcast over the heads).  Returns (adv, ret)."""
    T = values.shape[0]
    if rewards.dim() < values.dim():
        rewards = rewards[..., None]
    d = dones.bool()
    if d.dim() < values.dim():
        d = d[..., None]
    adv = torch.zeros_like(values)
    a_next, v_next = torch.zeros_like(last_value), last_value
    zero = torch.zeros_like(last_value)
    for t in range(T - 1, -1, -1):
        vb = torch.where(d[t], zero, v_next)
        an = torch.where(d[t], zero, a_next)
        delta = rewards[t] + gamma * vb - values[t]
        adv[t] = delta + gamma * lam * an
        a_next, v_next = adv[t], values[t]
    return adv, adv + values
