"""GPU: the torch surface of blue's own knowledge.  CC4TorchVecEnv.blue_view() in a learner's loop on a side stream -- a busy-aware mask from the
view, a step, the view again into the same tensors -- with no host wait until the loop is over, equal to the host statement of the definition on
the rows the loop left; with observations as uint8 and as bfloat16; bank slots; and check_errors() for an id out of range."""
import numpy as np
import pytest

from cage_challenge_4_amd import blue_view as BV

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('torch sees no device', allow_module_level=True)
from test_opponent_mix_torch import _random_actions, _side_stream  # noqa: E402  (after the skips above: that module imports torch)


def _env(n, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, **kw)


def _host_views(env, steps, with_cold=True):
    v = env.venv
    hs = [BV.from_row(v.get_state(e), v.get_cold(e) if with_cold else None, steps) for e in range(env.num_envs)]
    return np.stack([h for h, _ in hs]), np.stack([s for _, s in hs])


@pytest.mark.parametrize('obs_dtype', ['uint8', 'bfloat16'])
def test_learner_loop_without_host_waits_and_out_reuse(obs_dtype):
    n, K, steps, seed = 48, 20, 60, 1210
    env = _env(n, steps=steps, rng_mode=1, strict=False, obs_dtype=getattr(torch, obs_dtype))
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    env.reset(seeds=seed)
    env.enable_event_log(True)
    busy_seen = torch.zeros((), dtype=torch.int64, device=dev)
    with _side_stream(dev) as side:
        side.wait_stream(torch.cuda.default_stream(dev))
        hosts, scal = env.blue_view()
        assert hosts.shape == (n, 5, 137, 8) and hosts.dtype == torch.uint8 and scal.shape == (n, 5, 16) and scal.dtype == torch.int32 and hosts.device == dev
        ptrs = (hosts.data_ptr(), scal.data_ptr())
        for t in range(K):                                   # twenty iterations enqueued; nothing here waits for the device
            act = _random_actions(gen, n, dev)
            busy = scal[..., 0] != 0                         # a busy agent's submission would be dropped: it submits nothing
            act = torch.where(busy, torch.full_like(act, -1), act)
            busy_seen += busy.sum()
            obs, reward, done, info = env.step(act)
            assert obs.dtype == getattr(torch, obs_dtype)
            h2, s2 = env.blue_view(out=(hosts, scal))
            assert h2 is hosts and s2 is scal and (hosts.data_ptr(), scal.data_ptr()) == ptrs
        side.synchronize()                                   # the one wait
    want_h, want_s = _host_views(env, steps)
    assert np.array_equal(hosts.cpu().numpy(), want_h) and np.array_equal(scal.cpu().numpy(), want_s)
    assert (want_s[..., 13] == K).all() and (want_s[..., 10] == 1).all() and want_h[..., 3].any()
    assert int(busy_seen) > 0
    env.check_errors()

    # bank slots: saved episodes read where they lie, after the env has moved on; the log off: the hot-row part
    ids = torch.tensor([5, 40, 11], device=dev)
    bank = env.new_bank(4)
    env.save_episodes(ids, bank, torch.tensor([2, 0, 3], device=dev))
    env.step(_random_actions(gen, n, dev))
    bh, bs = env.blue_view(ids=torch.tensor([2, 0, 3], device=dev), bank=bank)
    assert np.array_equal(bh.cpu().numpy(), want_h[[5, 40, 11]]) and np.array_equal(bs.cpu().numpy(), want_s[[5, 40, 11]])
    env.enable_event_log(False)
    env.step(_random_actions(gen, n, dev))
    oh, os_ = env.blue_view()
    off_h, off_s = _host_views(env, steps)
    assert np.array_equal(oh.cpu().numpy(), off_h) and np.array_equal(os_.cpu().numpy(), off_s)
    assert (off_s[..., 10] == 0).all() and not off_h[..., 3:7].any() and off_h[..., 0].any() and (off_s[..., 13] == K + 2).all()
    env.check_errors()

    # out= of another shape or dtype is refused; an id out of range gives zero rows and surfaces in check_errors()
    with pytest.raises(ValueError):
        env.blue_view(out=(hosts[:-1], scal))
    with pytest.raises(ValueError):
        env.blue_view(out=(hosts, scal.to(torch.int64)))
    zh, zs = env.blue_view(ids=torch.tensor([0, n, 3], device=dev))
    torch.cuda.synchronize(dev)
    assert not zh[1].any() and not zs[1].any() and np.array_equal(zh[2].cpu().numpy(), off_h[3]) and np.array_equal(zs[0].cpu().numpy(), off_s[0])
    from cage_challenge_4_amd.vec_env import CC4EngineError
    with pytest.raises(CC4EngineError):
        env.check_errors()
    env.check_errors()
    env.close()
