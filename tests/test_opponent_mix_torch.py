"""GPU: per-episode opponent classes and device-side resets through CC4TorchVecEnv, on a non-default current stream.
7. reset(seeds=, env_mask=) from tensors a kernel wrote just before the call (cc4_reset_device) == the host path (cc4_reset) on a twin;
8. a bank load into a SECOND env carries live classes and assignments; out-of-range classes are skipped and check_errors() raises for them;
9. set_opponents / opponents / tensor reset on a side stream == CC4VecEnv.set_policies / policies / reset on the twin."""
import contextlib
import ctypes

import numpy as np
import pytest

import mix_util as M

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
ACT_LEN = (82, 82, 82, 82, 242)


def _env(n, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, **kw)


def _twin(monkeypatch, n, **kw):
    """as tests/test_plan.py builds its twins: ONE stream (CC4_GROUPS=1), no sampled self-check shadow"""
    monkeypatch.setenv('CC4_GROUPS', '1')
    monkeypatch.setenv('CC4_PERSIST_VERIFY_EVERY', '0')
    try:
        return _env(n, **kw)
    finally:
        monkeypatch.delenv('CC4_GROUPS')
        monkeypatch.delenv('CC4_PERSIST_VERIFY_EVERY')


@contextlib.contextmanager
def _side_stream(dev):
    """A non-default current stream that leaves nothing behind.  torch.cuda.Stream() hands out streams of a pool that lives as long as the process, and
    every live stream takes part in the runtime's mapping of streams onto hardware queues (conftest.py: a rollout's policy streams must not come to
    share the queue of its persistent kernel) -- so this one is created here, wrapped, and destroyed when the test is over."""
    from cage_challenge_4_amd.vec_env import _hip
    hip, p = _hip(), ctypes.c_void_p()
    hip.hipStreamCreateWithFlags.argtypes, hip.hipStreamCreateWithFlags.restype = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint], ctypes.c_int
    hip.hipStreamDestroy.argtypes, hip.hipStreamDestroy.restype = [ctypes.c_void_p], ctypes.c_int
    with torch.cuda.device(dev):
        assert hip.hipStreamCreateWithFlags(ctypes.byref(p), 1) == 0          # hipStreamNonBlocking
    s = torch.cuda.ExternalStream(p.value, device=dev)
    try:
        with torch.cuda.stream(s):
            assert torch.cuda.current_stream(dev).cuda_stream == p.value != torch.cuda.default_stream(dev).cuda_stream
            yield s
    finally:
        torch.cuda.synchronize(dev)
        assert hip.hipStreamDestroy(p) == 0


def _random_actions(gen, n, dev):
    return torch.cat([torch.randint(-1, ACT_LEN[b] + 1, (n, 1), generator=gen, device=dev) for b in range(5)], 1)


def _outputs(env):
    return [env.obs.clone(), env.reward.clone(), env.done.clone(), env.action_mask.clone(), env.err.clone()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------- 7. cc4_reset_device == cc4_reset
@pytest.mark.parametrize('n', [64, 6656])
@pytest.mark.parametrize('rng_mode', [0, 1], ids=['pcg64', 'philox'])
def test_tensor_reset_equals_host_reset(rng_mode, n, monkeypatch):
    """Env `a` resets from device tensors written on the current (side) stream immediately before the call -- seeds = base + arange, a mask computed
    from the rewards, then env_mask = env.done with the streams continuing --, its twin `b` from the same values as NumPy arrays.  Outputs, masks and
    every hot row are equal after each reset and after a following step; episodes outside the mask keep their rows."""
    a = _env(n, steps=12, rng_mode=rng_mode, strict=False)
    b = _twin(monkeypatch, n, steps=12, rng_mode=rng_mode, strict=False)
    dev = a.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(n + rng_mode)
    a.reset(seeds=300), b.reset(seeds=300)
    with _side_stream(dev):
        acts = [_random_actions(gen, n, dev) for _ in range(14)]
        for t in range(5):
            a.step(acts[t]), b.step(acts[t])
        before = a.venv.get_states()
        # 1. seeds and a mask a kernel writes right here: int32 seeds (any integer dtype), a bool mask
        seeds = 9000 + torch.arange(n, device=dev, dtype=torch.int32)
        mask = (a.reward < a.reward.median()) | (torch.arange(n, device=dev) % 5 == 0)
        a.reset(seeds=seeds, env_mask=mask)
        m = mask.cpu().numpy()
        assert 0 < m.sum() < n
        b.reset(seeds=(9000 + np.arange(n)).astype(np.uint64), env_mask=m.astype(np.uint8))
        assert _same(_outputs(a), _outputs(b))
        rows = a.venv.get_states()
        assert np.array_equal(rows, b.venv.get_states())
        assert np.array_equal(rows[~m], before[~m]) and (rows[m] != before[m]).any(axis=1).all()      # unmasked episodes untouched
        a.step(acts[5]), b.step(acts[5])
        assert _same(_outputs(a), _outputs(b))
        # 2. to the end of the unmasked episodes (a 12-step episode is done after 11 steps), then env.reset(env_mask=env.done): uint8 mask variant on `b`'s values, streams continue
        for t in range(6, 11):
            a.step(acts[t]), b.step(acts[t])
        done = a.done.cpu().numpy()
        assert done.any() and not done.all() and np.array_equal(done, ~m)
        before = a.venv.get_states()
        a.reset(env_mask=a.done)
        b.reset(env_mask=done.astype(np.uint8))
        assert _same(_outputs(a), _outputs(b)) and not bool(a.done.any())
        rows = a.venv.get_states()
        assert np.array_equal(rows, b.venv.get_states()) and np.array_equal(rows[~done], before[~done])
        a.step(acts[12]), b.step(acts[12])
        assert _same(_outputs(a), _outputs(b))
        # 3. uint64 seeds beyond 2^63 as a uint8 mask picks them
        big = (torch.arange(n, device=dev, dtype=torch.int64) - (1 << 62)).view(torch.uint64)
        some = (torch.arange(n, device=dev) % 2).to(torch.uint8)
        a.reset(seeds=big, env_mask=some)
        b.reset(seeds=big.cpu().view(torch.int64).numpy().view(np.uint64), env_mask=some.cpu().numpy())
        a.step(acts[13]), b.step(acts[13])
        assert _same(_outputs(a), _outputs(b))
    assert np.array_equal(a.venv.get_states(), b.venv.get_states()) and np.array_equal(a.venv.rng_state(), b.venv.rng_state())
    a.check_errors(), b.check_errors()
    with pytest.raises(ValueError):
        a.reset(env_mask=torch.zeros(n, device=dev))                   # a float mask
    with pytest.raises(ValueError):
        a.reset(seeds=torch.zeros(n + 1, dtype=torch.int64, device=dev))
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 9. set_opponents on a stream
@pytest.mark.parametrize('rng_mode', [0, 1], ids=['pcg64', 'philox'])
def test_set_opponents_on_a_side_stream_equals_the_host_path(rng_mode, monkeypatch):
    """Classes computed on the device (all 16 combinations over the batch) and assigned on a side stream before the first reset, reassigned from
    tensors in mid-episode, a tensor reset of the episodes that are done: the twin takes the same values through CC4VecEnv.set_policies and NumPy
    resets.  30-step episodes with autoreset, 70 steps: outputs at every step, the class tensors, hot rows at the end."""
    n = 96
    a = _env(n, steps=30, rng_mode=rng_mode, autoreset=True, strict=False)
    b = _twin(monkeypatch, n, steps=30, rng_mode=rng_mode, autoreset=True, strict=False)
    dev = a.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    with _side_stream(dev):
        e = torch.arange(n, device=dev)
        red, green, blue = (e // 4) % 4, (e // 2) % 2, e % 2           # int64 tensors: any integer dtype
        a.set_opponents(red=red, green=green, blue=blue)
        b.venv.set_policies(red.cpu().numpy(), green.cpu().numpy(), blue.cpu().numpy())
        live, assigned = a.opponents()
        assert live.dtype == torch.int8 and tuple(live.shape) == (n, 3) and not bool(live.any())
        assert torch.equal(assigned, torch.stack([red, green, blue], 1).to(torch.int8))
        seeds = 70 + torch.arange(n, device=dev)
        a.reset(seeds=seeds)
        b.reset(seeds=seeds.cpu().numpy().astype(np.uint64))
        assert _same(_outputs(a), _outputs(b))
        assert torch.equal(a.opponents()[0], assigned)
        for t in range(70):
            if t == 12:                                                 # mid-episode: red classes rotate, green and blue stay (None = keep)
                red2 = (red + 1) % 4
                a.set_opponents(red=red2.to(torch.int16))
                b.venv.set_policies(red=red2.cpu().numpy())
            if t == 45:                                                 # a device criterion restarts some episodes early, the streams continue
                pick = a.reward < a.reward.median()
                a.reset(env_mask=pick)
                b.reset(env_mask=pick.cpu().numpy().astype(np.uint8))
                assert _same(_outputs(a), _outputs(b))
            act = _random_actions(gen, n, dev)
            a.step(act), b.step(act)
            assert _same(_outputs(a), _outputs(b)), t
            la, aa = a.opponents()
            lb, ab = b.venv.policies()
            assert np.array_equal(la.cpu().numpy(), lb) and np.array_equal(aa.cpu().numpy(), ab), t
            if 12 <= t < 29:
                assert torch.equal(la[:, 0], red.to(torch.int8)) and torch.equal(aa[:, 0], red2.to(torch.int8)), t      # not before the regeneration
        assert torch.equal(a.opponents()[0][:, 0], red2.to(torch.int8))
    assert np.array_equal(a.venv.get_states(), b.venv.get_states())
    a.check_errors(), b.check_errors()
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------------------- 8. banks and faults
def test_a_bank_load_into_a_second_env_carries_classes_and_assignments(monkeypatch):
    n = 16
    a = _env(n, steps=30, rng_mode=1, autoreset=True, strict=False)
    b = _twin(monkeypatch, n, steps=30, rng_mode=1, autoreset=True, strict=False, red_policy=1)
    dev = a.device
    e = torch.arange(n, device=dev)
    a.set_opponents(red=e % 4, green=(e // 4) % 2, blue=(e // 8) % 2)
    a.reset(seeds=11), b.reset(seeds=12)
    a.set_opponents(blue=1 - (e // 8) % 2)                              # live and assigned blue classes now differ
    live_a, asg_a = a.opponents()
    assert not torch.equal(live_a, asg_a)
    ids = torch.arange(n, device=dev)
    bank = a.new_bank(n)
    a.save_episodes(ids, bank, ids)
    half = ids[: n // 2]
    b.load_episodes(bank, half, half + n // 2)                          # slots 0..7 -> episodes 8..15 of the second env
    live_b, asg_b = b.opponents()
    assert torch.equal(live_b[n // 2:], live_a[: n // 2]) and torch.equal(asg_b[n // 2:], asg_a[: n // 2])
    assert bool((live_b[: n // 2] == torch.tensor([1, 0, 0], dtype=torch.int8, device=dev)).all()) and bool((asg_b[: n // 2] == M.DEFAULT).all())
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    for _ in range(32):                                                 # across the regeneration of call 30
        b.step(_random_actions(gen, n, dev))
    live_b, asg_b2 = b.opponents()
    assert torch.equal(asg_b2, asg_b) and torch.equal(live_b[n // 2:], asg_a[: n // 2])       # the destination regenerated into what it was given
    assert bool((live_b[: n // 2] == torch.tensor([1, 0, 0], dtype=torch.int8, device=dev)).all())
    a.check_errors(), b.check_errors()
    a.close(), b.close()


def test_out_of_range_opponents_leave_their_episodes_and_check_errors_raises():
    from cage_challenge_4_amd.vec_env import CC4EngineError
    n = 300                                                             # more than one block of the kernel
    env = _env(n, steps=30, rng_mode=0, strict=False)
    dev = env.device
    env.set_opponents(red=torch.full((n,), 3, device=dev), green=torch.zeros(n, dtype=torch.int64, device=dev), blue=torch.ones(n, dtype=torch.int64, device=dev))
    env.reset(seeds=1)
    env.check_errors()
    red = torch.full((n,), 1, device=dev)
    green = torch.full((n,), M.KEEP, device=dev)
    bad = {0: (4, M.KEEP), 63: (1, 2), 64: (300, M.KEEP), 257: (-129, M.KEEP), 299: (M.DEFAULT, 0)}      # 300 / -129: beyond int8, still out of range
    for i, (r, g) in bad.items():
        red[i], green[i] = r, g
    env.set_opponents(red=red, green=green)
    live, assigned = env.opponents()
    with pytest.raises(CC4EngineError, match='INDEX_OUT_OF_RANGE'):
        env.check_errors()
    env.check_errors()                                                  # reported once
    assert bool((live == torch.tensor([3, 0, 1], dtype=torch.int8, device=dev)).all())
    want = torch.tensor([[3, 0, 1] if i in bad else [1, 0, 1] for i in range(n)], dtype=torch.int8, device=dev)
    assert torch.equal(assigned, want)
    with pytest.raises(ValueError):
        env.set_opponents(red=torch.zeros(n, device=dev))              # a float tensor
    env.close()
