"""GPU: the torch surface of the masked action sampling.  CC4TorchVecEnv.sample_actions(): shapes and dtypes, out=, the refusals, determinism in
(seed, t) and the default counter; a learner's loop of sample_actions + step on the device, equal at every step -- actions, rewards, dones,
observations -- to the CPU oracle stepped with the host function's actions for the same seeds, which shows that -1 for a busy agent and the
drawn indices mean to step() what the definition says; check_errors() after a NaN logit on a valid slot."""
import numpy as np
import pytest

import sample_util as U
from cage_challenge_4_amd import action_sampling as AS
from oracle_binding import OracleVecEnv

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('torch sees no device', allow_module_level=True)

N, STEPS, SEED, K = 65, 30, 5100, 20


def _env(n=N, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, steps=STEPS, rng_mode=1, autoreset=True, **kw)


def test_shapes_out_refusals_determinism_and_check_errors():
    env = _env()
    dev = env.device
    env.reset(seeds=SEED)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        logits = (torch.randn((N, 570), generator=gen, device=dev) * 3).to(dt)
        actions, stats = env.sample_actions(logits)
        assert actions.shape == (N, 5) and actions.dtype == torch.int32 and stats.shape == (N, 5, 2) and stats.dtype == torch.float32
        assert actions.device == dev and stats.device == dev
        picked = env.action_mask.gather(1, (actions.long() + torch.tensor(AS.SEGMENTS[:5], device=dev)))
        assert bool(picked.all()) and bool((stats[..., 0] <= 0).all()) and bool((stats[..., 1] >= 0).all())
    ptrs = (actions.data_ptr(), stats.data_ptr())
    a2, s2 = env.sample_actions(logits, out=(actions, stats))
    assert a2 is actions and s2 is stats and (actions.data_ptr(), stats.data_ptr()) == ptrs
    # the same (seed, t) gives the same tensors; the default counter makes two consecutive calls differ
    x = env.sample_actions(logits, seed=3, t=8)
    y = env.sample_actions(logits, seed=3, t=8)
    z = env.sample_actions(logits, seed=3, t=9)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and not torch.equal(x[0], z[0])
    t0 = env._sample_t
    p = env.sample_actions(logits, seed=3)
    q = env.sample_actions(logits, seed=3)
    assert env._sample_t == t0 + 2 and not torch.equal(p[0], q[0])
    assert torch.equal(p[0], env.sample_actions(logits, seed=3, t=t0)[0]) and env._sample_t == t0 + 2
    g1, g2 = env.sample_actions(logits, greedy=True), env.sample_actions(logits, greedy=True)
    assert torch.equal(g1[0], g2[0])                  # no noise: the counter does not show
    u = env.sample_actions(None, seed=3, t=1)
    assert u[0].shape == (N, 5) and bool((u[0] >= 0).all())
    ids = torch.tensor([7, 64, 7], device=dev)
    sub = env.sample_actions(logits[[0, 1, 0]].contiguous(), seed=3, t=8, ids=ids)
    assert sub[0].shape == (3, 5) and torch.equal(sub[0][0], sub[0][2])
    # the ValueErrors
    f32 = logits.float()
    for bad in (f32[:-1], f32[:, :-1], f32.double(), f32.long(), f32.cpu(), f32.t().contiguous().t(), 'x', f32.view(N, 5, 114)):
        with pytest.raises(ValueError, match='logits'):
            env.sample_actions(bad)
    for T in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='temperature'):
            env.sample_actions(f32, temperature=T)
    for bad_out in ((actions[:-1], stats), (actions, stats.double()), (actions.long(), stats), (actions, stats[..., 0])):
        with pytest.raises(ValueError, match='out'):
            env.sample_actions(f32, out=bad_out)
    env.check_errors()
    # a NaN logit on a valid slot: that agent -1, the others as before, and check_errors() raises
    bad = f32.clone()
    bad[9, AS.SEGMENTS[2] + U.SLEEP[2]] = float('nan')
    got = env.sample_actions(bad, seed=3, t=8, busy_aware=False)
    ref = env.sample_actions(f32, seed=3, t=8, busy_aware=False)
    torch.cuda.synchronize(dev)
    assert int(got[0][9, 2]) == -1 and not got[1][9, 2].any()
    keep = torch.ones((N, 5), dtype=torch.bool, device=dev)
    keep[9, 2] = False
    assert torch.equal(got[0][keep], ref[0][keep]) and torch.equal(got[1][keep], ref[1][keep])
    from cage_challenge_4_amd.vec_env import CC4EngineError
    with pytest.raises(CC4EngineError):
        env.check_errors()
    env.check_errors()
    env.close()


def _oracle_episode(e, rng):
    """Episode e of the batch on the CPU oracle, stepped K steps with the host function's actions; its logits row is drawn again until no case of
    the run falls below tau, so that the device must reproduce the run exactly.  Returns (logits row, per step: actions, reward, done, obs)."""
    for _attempt in range(50):
        row = U.random_logits(rng)
        ora = OracleVecEnv(1, steps=STEPS, rng_mode=1, autoreset=True)
        ora.reset(seeds=np.array([SEED + e], np.uint64))
        mask = ora.mask()[0]
        trace, clear = [], True
        for t in range(K):
            hot = ora.get_state(0)
            a, _st, refused = AS.from_row(hot, row, 21, t, e, busy_aware=True)
            ref = AS.reference(mask, U.busy_of(hot, STEPS), row, 21, t, e, details=True)
            if refused or (ref[3] < 2.0 ** -12 * ref[4]['zmax']).any() or not np.array_equal(ref[0], a):
                clear = False
                break
            obs, rew, done, _ = ora.step(a[None, :])
            trace.append((a.copy(), float(rew[0]), bool(done[0]), obs[0].copy()))
        ora.close()
        if clear:
            return row, trace
    raise AssertionError(f'episode {e}: no logits row without a case below tau in 50 draws')


def test_loop_of_sample_and_step_equals_the_oracle_stepped_with_the_host_functions_actions():
    rng = np.random.default_rng(77)
    runs = [_oracle_episode(e, rng) for e in range(N)]
    assert all(len(tr) == K for _row, tr in runs)                     # the precondition: no case below tau anywhere in the oracle run
    assert any((a == -1).any() for _row, tr in runs for a, *_ in tr), 'no busy agent in the run'
    env = _env()
    dev = env.device
    env.reset(seeds=SEED)
    logits = torch.from_numpy(np.stack([row for row, _tr in runs])).to(dev)
    seen = []
    for t in range(K):                                                # enqueued; nothing here waits for the device
        actions, _stats = env.sample_actions(logits, seed=21, t=t, busy_aware=True)
        obs, reward, done, _info = env.step(actions)
        seen.append((actions.clone(), reward.clone(), done.clone(), obs.clone()))
    torch.cuda.synchronize(dev)
    for t, (a, r, d, o) in enumerate(seen):
        a, r, d, o = a.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy(), o.cpu().numpy()
        for e in range(N):
            wa, wr, wd, wo = runs[e][1][t]
            assert np.array_equal(a[e], wa), (t, e, a[e].tolist(), wa.tolist())
            assert r[e] == wr and bool(d[e]) == wd and np.array_equal(o[e].astype(np.int32), wo), (t, e)
    env.check_errors()
    env.close()
