"""GPU: the torch surface of the red agents as learners.  CC4TorchVecEnv.step(red_actions=...) and red_view() in a loop on a side stream with
no host wait -- a red policy on the device that reads the view and writes the next actions -- equal to the host path (cc4_step_ex) replayed
afterwards from the recorded actions; red_actions=None is the path of before."""
import numpy as np
import pytest

import red_util as RU
from cage_challenge_4_amd import red_view as RV

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('torch sees no device', allow_module_level=True)
ACT_LEN = (82, 82, 82, 82, 242)
from test_opponent_mix_torch import _side_stream  # noqa: E402  (after the skips above: that module imports torch)


def _env(n, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, **kw)


def _random_actions(gen, n, dev):
    return torch.cat([torch.randint(-1, ACT_LEN[b] + 1, (n, 1), generator=gen, device=dev) for b in range(5)], 1)


def _red_policy(hosts, scal, gen):
    """A stand-in red learner, on the device: a random action type per agent, aimed at what the view shows -- the first host whose ip it knows
    (scans, exploits), the first host it holds a session on (escalation, impact, degrade, withdraw), its lowest known subnet -- on SID_AUTO."""
    n, dev = hosts.shape[0], hosts.device
    typ = torch.randint(-1, 11, (n, 6), generator=gen, device=dev)
    known = hosts[..., 0].to(torch.int32).argmax(dim=2)
    held = (hosts[..., 3] > 0).to(torch.int32).argmax(dim=2)
    subnet = ((scal[..., 10].unsqueeze(-1) >> torch.arange(9, device=dev)) & 1).argmax(dim=2)
    host = torch.where(typ >= 5, held, known)
    arg = torch.where(typ == 0, subnet, torch.where(typ == 8, host, torch.zeros_like(host)))
    return torch.stack([typ, host, arg, torch.full_like(typ, RV.SID_AUTO)], dim=2)


def test_red_learner_loop_on_a_side_stream_equals_the_host_path():
    from cage_challenge_4_amd import CC4VecEnv
    n, K, seed = 48, 10, 930
    env = _env(n, steps=40, rng_mode=1, strict=False)
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(6)
    env.reset(seeds=seed)
    assert env.venv.run_kernel_for(12) != env.venv.step_kernel
    blue = [_random_actions(gen, n, dev) for _ in range(K)]
    rec = []
    with _side_stream(dev) as side:          # (a stream that is destroyed afterwards: a pooled torch stream would stay in the runtime's queue mapping)
        side.wait_stream(torch.cuda.default_stream(dev))
        hosts, scal = env.red_view()
        assert hosts.shape == (n, 6, 137, 8) and hosts.dtype == torch.uint8 and scal.shape == (n, 6, 16) and scal.dtype == torch.int32 and hosts.device == dev
        for t in range(K):
            red = _red_policy(hosts, scal, gen)                      # int64 [N, 6, 4]: any integer dtype
            obs, reward, done, info = env.step(blue[t], red_actions=red)
            env.red_view(out=(hosts, scal))
            rec.append((red.clone(), obs.clone(), reward.clone(), done.clone(), info['err'].clone(), hosts.clone(), scal.clone()))
    assert env.venv.run_kernel_for(12) == env.venv.step_kernel     # a handle that has taken red actions runs the full builds of its step kernel
    # the host path, from the recorded actions
    A = CC4VecEnv(n, steps=40, rng_mode=1, strict=False)
    A.reset(seeds=seed)
    types = set()
    for t, (red, obs, reward, done, err, hosts, scal) in enumerate(rec):
        docs = RU.parse([A.true_state_json(e) for e in range(n)])
        words = red.cpu().numpy().astype(np.int32)
        types |= set(np.unique(words[..., 0]).tolist())
        oa, ra, da, _ = A.step_ex(blue[t].cpu().numpy().astype(np.int32), None, red=RU.host_records(words, docs))
        assert np.array_equal(obs.cpu().numpy().astype(np.int32), oa) and np.array_equal(reward.cpu().numpy(), ra), t
        assert np.array_equal(done.cpu().numpy(), da) and np.array_equal(err.cpu().numpy().view(np.uint32), A.err), t
        views = [RV.from_row(r) for r in A.get_states()]
        assert np.array_equal(hosts.cpu().numpy(), np.stack([v[0] for v in views])) and np.array_equal(scal.cpu().numpy(), np.stack([v[1] for v in views])), t
        assert (scal[..., 15] == t + 1).all()
    assert types == set(range(-1, 11))
    assert np.array_equal(env.venv.get_states(), A.get_states())
    for e in range(0, n, 5):
        assert env.venv.true_state_json(e) == A.true_state_json(e), e
    env.check_errors()
    with pytest.raises(ValueError):
        env.step(blue[0], red_actions=torch.zeros((n, 6, 3), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        env.step(blue[0], red_actions=torch.zeros((n, 6, 4), dtype=torch.float32, device=dev))
    bad = torch.full((n, 6, 4), -1, dtype=torch.int64, device=dev)
    bad[3, 2] = torch.tensor([2 ** 32 + 3, 0, 0, 0], dtype=torch.int64, device=dev)      # beyond int32: refused, not wrapped into type 3
    env.step(blue[0], red_actions=bad)
    from cage_challenge_4_amd.vec_env import CC4EngineError
    with pytest.raises(CC4EngineError):
        env.check_errors()
    A.close()
    env.close()


def test_without_red_actions_the_step_is_the_one_of_before():
    n, K = 32, 8
    a, b = _env(n, steps=40, rng_mode=1), _env(n, steps=40, rng_mode=1)
    dev = a.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    a.reset(seeds=55); b.reset(seeds=55)
    for t in range(K):
        act = _random_actions(gen, n, dev)
        ra, rb = a.step(act), b.step(act, None, red_actions=None)
        for x, y in zip(ra[:3] + (ra[3]['action_mask'], ra[3]['err']), rb[:3] + (rb[3]['action_mask'], rb[3]['err'])):
            assert torch.equal(x, y), t
    torch.cuda.synchronize(dev)
    assert np.array_equal(a.venv.get_states(), b.venv.get_states())
    assert b.venv.run_kernel_for(12) == a.venv.run_kernel_for(12) != b.venv.step_kernel      # still on the one-launch forms: no record buffer, no full builds
    a.close(); b.close()
