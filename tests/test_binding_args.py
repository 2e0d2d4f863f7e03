"""GPU: the Python binding's argument path on a device.  Every spelling of the same seeds, masks, actions and messages steps both envs to the
same bits; a view's out= tensors at an address the entry point would refuse are refused in Python, before anything is enqueued; a short reset
mask is refused instead of read; and CC4VecEnv.sample_actions, whose logits now travel in the view's own staging block, still equals the host
statement of the definition.  Counter mode, eight steps, 3 and 20 episodes: either side of the 16 episodes from which a handle stages its host
copies in pinned blocks.  No refusal here reaches the device: each is raised in Python before a launch."""
import numpy as np
import pytest

try:            # before libcc4.so opens the device: a torch imported behind it finds no GPU (torch brings a HIP runtime of its own)
    import torch
except ImportError:
    torch = None
import sample_util as U
from cage_challenge_4_amd import CC4VecEnv
from cage_challenge_4_amd import _lib as L
from cage_challenge_4_amd import _views as V
from cage_challenge_4_amd import action_sampling as AS

pytestmark = pytest.mark.gpu
KW = dict(steps=8, rng_mode=1, strict=False)
SIZES = (3, 20)


def _arguments(n):
    """The exact-dtype, contiguous spelling: (seeds, env_mask, [actions] * 3, [messages] * 3)."""
    rng = np.random.default_rng(n)
    seeds = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)        # (beyond int63: a cast through a signed dtype wraps back)
    mask = (np.arange(n) % 3 != 1).astype(np.uint8)
    acts = [np.stack([rng.integers(-1, r, n) for r in L.ACT_LEN], 1).astype(np.int32) for _ in range(3)]
    msgs = [rng.integers(0, 2, (n, L.NUM_BLUE, L.MSG_LEN)).astype(np.uint8) for _ in range(3)]
    return seeds, mask, acts, msgs


def _strided(a):
    big = np.zeros((2,) + a.shape, a.dtype).repeat(2, axis=-1)
    big[1, ..., ::2] = a
    out = big[1, ..., ::2]
    assert not out.flags.c_contiguous and np.array_equal(out, a)
    return out


SPELLINGS = {'exact': lambda a: a, 'list': lambda a: a.tolist(), 'int64': lambda a: a.astype(np.int64), 'strided': _strided}


def _host(x):
    return x.cpu().numpy().copy() if hasattr(x, 'cpu') else np.array(x, copy=True)


def _trajectory(env, n, spell, wrap=lambda a: a):
    """reset (all), reset (masked, fresh seeds), three steps; every output after every call.  wrap: what the env's step takes (tensors)."""
    seeds, mask, acts, msgs = _arguments(n)
    obs_of = lambda r: _host(r[0] if isinstance(r, tuple) else r)      # noqa: E731  (the torch env's reset returns (obs, info))
    out = [obs_of(env.reset(seeds=5)), obs_of(env.reset(seeds=spell(seeds), env_mask=spell(mask)))]
    for a, m in zip(acts, msgs):
        obs, rew, done, _info = env.step(wrap(spell(a)), wrap(spell(m)))
        out += [_host(obs), _host(rew), _host(done)]
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), f'{what}: output {k} differs'


@pytest.mark.parametrize('n', SIZES)
def test_every_spelling_steps_the_host_env_to_the_same_bits(n):
    env = CC4VecEnv(n, **KW)
    want = _trajectory(env, n, SPELLINGS['exact'])
    assert all(w.any() for w in want[:3])
    for name in ('list', 'int64', 'strided'):
        _same(_trajectory(env, n, SPELLINGS[name]), want, f'CC4VecEnv, N = {n}, {name}')
    with pytest.raises(ValueError, match='env_mask'):
        env.reset(env_mask=np.ones(n - 1, np.uint8))
    with pytest.raises(ValueError, match='seeds'):
        env.reset(seeds=np.arange(n + 1))
    with pytest.raises(ValueError, match='actions'):
        env.step(np.zeros((n, 4), np.int32))
    _same(_trajectory(env, n, SPELLINGS['exact']), want, f'CC4VecEnv, N = {n}, after the refusals')
    env.close()


@pytest.mark.parametrize('n', SIZES)
def test_every_spelling_steps_the_torch_env_to_the_same_bits(n):
    if torch is None:
        pytest.skip('no torch')
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    env = CC4TorchVecEnv(n, **KW)
    dev = env.device

    def tensor(a):          # (a list has no tensor spelling of its own: it goes up as the array it describes)
        a = np.asarray(a) if isinstance(a, list) else a
        if a.dtype == np.uint64:
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        big = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        if not a.flags.c_contiguous:                                  # strided on the device too
            wide = torch.zeros(big.shape[:-1] + (2 * big.shape[-1],), dtype=big.dtype, device=dev)
            wide[..., ::2] = big
            big = wide[..., ::2]
            assert not big.is_contiguous() or big.shape[-1] == 1
        return big
    # host arguments to reset (cc4_reset), tensors to step
    want = _trajectory(env, n, SPELLINGS['exact'], tensor)
    for name in ('list', 'int64', 'strided'):
        _same(_trajectory(env, n, SPELLINGS[name], tensor), want, f'CC4TorchVecEnv, N = {n}, {name}')
    # tensors to reset as well (cc4_reset_device): uint64 seeds viewed, int64 seeds of the same bits cast, a bool mask, a strided mask
    seeds, mask, acts, msgs = _arguments(n)
    variants = [(tensor(seeds), tensor(mask)), (tensor(seeds.view(np.int64)), tensor(mask).bool()), (tensor(seeds), tensor(_strided(mask))),
                (seeds, tensor(mask)), (tensor(seeds), mask.tolist())]
    for k, (s, m) in enumerate(variants):
        env.reset(seeds=5)
        got = [_host(env.reset(seeds=s, env_mask=m)[0])]
        for a, mm in zip(acts, msgs):
            got += [_host(x) for x in env.step(tensor(a), tensor(mm))[:3]]
        _same(got, want[1:], f'CC4TorchVecEnv, N = {n}, device reset variant {k}')
    with pytest.raises(ValueError, match='env_mask'):
        env.reset(env_mask=np.ones(n - 1, np.uint8))
    with pytest.raises(ValueError, match='env_mask'):
        env.reset(env_mask=torch.ones(n - 1, dtype=torch.bool, device=dev))
    env.check_errors()
    env.close()


def _misaligned_cases():
    """(view, which output, max_edges): every output whose entry point asks for more than its dtype's own alignment."""
    return [(name, i, 5 if name == 'blue_edges' else None) for name in V.VIEWS for i, o in enumerate(V.VIEWS[name].outs) if o.align > o.dtype.itemsize]


def test_the_table_has_outputs_to_misalign():
    assert {c[0] for c in _misaligned_cases()} == {'state_features', 'red_view', 'blue_view', 'blue_edges', 'reward_terms'}


@pytest.mark.parametrize('n', SIZES)
def test_a_misaligned_out_is_refused_before_anything_is_enqueued(n):
    if torch is None:
        pytest.skip('no torch')
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv, _TORCH_DTYPES
    env = CC4TorchVecEnv(n, **KW)
    env.enable_event_log()
    env.enable_reward_terms()
    env.reset(seeds=11)
    env.step(torch.zeros((n, 5), dtype=torch.int32, device=env.device))
    env.check_errors()
    calls = {'state_features': env.state_features, 'red_view': env.red_view, 'blue_view': env.blue_view,
             'blue_edges': lambda **kw: env.blue_edges(max_edges=5, **kw), 'reward_terms': env.reward_terms,
             'sample_actions': lambda **kw: env.sample_actions(None, seed=3, t=1, **kw)}
    assert set(calls) == set(V.VIEWS)

    def carve(o, offset):       # a tensor of the output's shape `offset` bytes into a fresh allocation (which the allocator aligns to 512 bytes)
        nbytes = n * int(np.prod(o.tail)) * o.dtype.itemsize
        raw = torch.zeros(nbytes + 64, dtype=torch.uint8, device=env.device)
        assert raw.data_ptr() % 64 == 0
        return raw[offset:offset + nbytes].view(_TORCH_DTYPES[o.dtype]).view((n,) + o.tail)
    for name, call in calls.items():
        e = 5 if name == 'blue_edges' else None
        outs = V.outs(name, e)
        want = call()
        got = call(out=tuple(carve(o, 0) for o in outs))
        assert all(torch.equal(g, w) for g, w in zip(got, want)), name
        assert want[0].shape == (n,) + outs[0].tail and want[1].shape == (n,) + outs[1].tail
        for _name, i, _e in (c for c in _misaligned_cases() if c[0] == name):
            off = outs[i].dtype.itemsize                   # aligned for the dtype, not for the entry point
            bad = tuple(carve(o, off if j == i else 0) for j, o in enumerate(outs))
            assert bad[i].data_ptr() % outs[i].align == off
            with pytest.raises(ValueError, match='out'):
                call(out=bad)
            assert not bad[i].any()                        # untouched
            env.check_errors()                             # nothing enqueued, no fault recorded
            # the same tensors where the entry point accepts them: one alignment further on
            ok = tuple(carve(o, outs[i].align if j == i else 0) for j, o in enumerate(outs))
            got = call(out=ok)
            assert got[0] is ok[0] and got[1] is ok[1] and all(torch.equal(g, w) for g, w in zip(got, want)), (name, i)
    env.check_errors()
    env.close()


def test_sample_actions_of_an_id_list_against_the_host_function():
    n, ids, seed, t = 3, [2, 0], 5, 11
    env = CC4VecEnv(n, **KW)
    env.reset(seeds=40)
    for _ in range(2):
        env.step(np.full((n, 5), 3, np.int32))
    hots, mask = env.get_states(), env.action_mask
    logits = U.random_logits(np.random.default_rng(1), (len(ids), 570))
    act, st = env.sample_actions(logits, ids=ids, seed=seed, t=t)
    assert act.shape == (2, 5) and act.dtype == np.int32 and st.shape == (2, 5, 2) and st.dtype == np.float32
    tally = U.Tally()
    for j, e in enumerate(ids):
        ha, hs, refused = AS.from_row(hots[e], logits[j], seed, t, e)
        busy = U.busy_of(hots[e], KW['steps'])
        ref = AS.reference(mask[e], busy, logits[j], seed, t, e, details=True)
        assert not refused
        tally.check(act[j], st[j], ref, f'entry {j} (episode {e})')
        sure = ref[3] >= 2.0 ** -12 * ref[4]['zmax']
        assert np.array_equal(act[j][sure], ha[sure]), (j, act[j], ha)
        same = act[j] == ha
        assert np.abs(st[j][same] - hs[same]).max(initial=0.0) <= 2.0 ** -12 * max(1.0, np.abs(hs).max()), j
    print(f'CC4VecEnv.sample_actions with ids: {tally.cases} cases, {tally.below} below tau, max |logp - ref| {tally.dlogp:.3g}')
    # without logits and without ids the same block carries the outputs alone
    act0, st0 = env.sample_actions(None, seed=seed, t=t)
    assert act0.shape == (n, 5) and (act0 >= -1).all()
    env.close()
