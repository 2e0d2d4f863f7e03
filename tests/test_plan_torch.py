"""GPU: CC4TorchVecEnv.step_plan -- a plan produced and consumed on a side stream with nothing synchronised in between, against the numpy path;
the recorded observations; action masks of episodes regenerated inside the plan; argument checks; and README's search example as written."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
ACT_LEN = (82, 82, 82, 82, 242)


def _env(n, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, **kw)


def _np(t):
    return (t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy()


@pytest.mark.parametrize('n,mode,dtype', [(8192, 1, torch.bfloat16), (1024, 1, torch.uint8), (6656, 0, torch.float32)])
def test_step_plan_on_a_side_stream_equals_the_numpy_path(n, mode, dtype):
    from cage_challenge_4_amd import CC4VecEnv
    k, steps = 40, 30                       # every episode ends and regenerates inside the plan
    env = _env(n, obs_dtype=dtype, steps=steps, rng_mode=mode, autoreset=True, strict=False)
    ref = CC4VecEnv(n, steps=steps, rng_mode=mode, autoreset=True, strict=False)
    twin = _env(n, obs_dtype=dtype, steps=steps, rng_mode=mode, autoreset=True, strict=False)
    env.reset(seeds=21), ref.reset(seeds=21), twin.reset(seeds=21)
    dev = env.device
    mask0 = env.action_mask.clone()
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    with torch.cuda.stream(side):
        # the plan comes from kernels enqueued just before the call, the rewards go into one enqueued just behind it: no synchronise in between
        plan = torch.cat([torch.randint(-2, ACT_LEN[b] + 3, (k, n, 1), generator=gen, device=dev) for b in range(5)], 2)
        msgs = torch.randint(0, 2, (k, n, 5, 8), generator=gen, device=dev, dtype=torch.uint8)
        obs, rewards, dones, info = env.step_plan(plan, msgs, record_obs=True)
        ret = rewards.sum(0)
        n_done = dones.sum(0)
    side.synchronize()
    o2, r2, d2, i2 = ref.run_plan(plan.cpu().numpy(), msgs.cpu().numpy(), record_obs=True)
    assert np.array_equal(_np(rewards), r2) and np.array_equal(_np(dones), d2)
    assert np.array_equal(_np(ret), r2.sum(0, dtype=np.float32)) or np.allclose(_np(ret), r2.astype(np.float64).sum(0))   # (summation order is torch's)
    assert np.array_equal(_np(n_done), d2.sum(0)) and (d2.sum(0) >= 1).all()
    assert info['obs_seq'].dtype == dtype and np.array_equal(_np(info['obs_seq']).astype(np.uint8), i2['obs_seq'])
    assert torch.equal(info['obs_seq'][-1], obs)
    assert np.array_equal(_np(obs).astype(np.int32), o2)
    assert np.array_equal(_np(info['err']).astype(np.uint32), i2['err'])
    # the masks: a twin stepped one call at a time refreshes them at every regeneration
    for j in range(k):
        twin.step(plan[j], msgs[j])
    torch.cuda.synchronize(dev)
    assert torch.equal(info['action_mask'], twin.action_mask)
    assert (info['action_mask'] != mask0).any(dim=1).sum().item() > n // 2      # new scenarios: the rows did change
    assert torch.equal(obs, twin.obs) and torch.equal(env.reward, twin.reward) and torch.equal(env.done, twin.done)
    env.close(), ref.close(), twin.close()


def test_step_plan_argument_checks():
    n = 64
    env = _env(n, steps=20, rng_mode=1)
    env.reset(seeds=1)
    dev = env.device
    good = torch.zeros((3, n, 5), dtype=torch.int64, device=dev)
    for bad in (good[0], good[:, :-1], good[:, :, :4], good.float(), good.bool(), good.cpu(), good[:0], good.cpu().numpy()):
        with pytest.raises(ValueError):
            env.step_plan(bad)
    for bad in (torch.zeros((3, n, 5), dtype=torch.uint8, device=dev), torch.zeros((2, n, 5, 8), dtype=torch.uint8, device=dev),
                torch.zeros((3, n, 5, 8), dtype=torch.float32, device=dev), torch.zeros((3, n, 5, 8), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            env.step_plan(good, bad)
    before = env.obs.clone()
    obs, rewards, dones, info = env.step_plan(good, torch.zeros((3, n, 5, 8), dtype=torch.bool, device=dev))     # (nothing was enqueued by the refused calls)
    torch.cuda.synchronize(dev)
    twin = _env(n, steps=20, rng_mode=1)
    twin.reset(seeds=1)
    for j in range(3):
        twin.step(good[j])
    torch.cuda.synchronize(dev)
    assert torch.equal(obs, twin.obs) and rewards.shape == (3, n) and dones.dtype == torch.bool and before.shape == obs.shape
    env.close(), twin.close()


def test_readme_search_example_runs_as_written():
    """The example of README's plan section, executed verbatim; its best plan per root equals the one found by stepping the same candidates one
    step at a time on a second env."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    blocks = re.findall(r'```python\n(.*?)```', open(os.path.join(root, 'README.md')).read(), flags=re.S)
    code = [b for b in blocks if 'step_plan(' in b]
    assert len(code) == 1
    ns = {}
    exec(compile(code[0], 'README.md', 'exec'), ns)
    env, plans, best, best_plan, R, B, k = (ns[x] for x in ('env', 'plans', 'best', 'best_plan', 'R', 'B', 'k'))
    assert R * B == 8192 and env.venv.plan_kernel_for(k) == 'k_run_philox1p'
    other = _env(R * B, steps=500, rng_mode=1, autoreset=True)
    other.reset(seeds=0)
    other.clone_episodes(ns['roots'].repeat(B - 1), torch.arange(R, R * B, device=other.device))
    total = torch.zeros(R * B, dtype=torch.float64, device=other.device)
    rows = []
    for j in range(k):
        _, rew, _, _ = other.step(plans[j])
        rows.append(rew.clone())
        total += rew.double()
    torch.cuda.synchronize()
    assert torch.equal(torch.stack(rows), ns['rewards'])
    assert torch.equal(torch.stack(rows).sum(0).view(B, R).argmax(0), best)
    assert tuple(best_plan.shape) == (k, R, 5) and torch.equal(best_plan[:, 5], plans[:, int(best[5]) * R + 5])
    assert torch.equal(other.obs, ns['obs'])
    env.close(), other.close()
