"""GPU: the torch surface of the reward terms.  CC4TorchVecEnv.enable_reward_terms() / reward_terms() in a learner's loop on a side stream -- a step,
the terms into the same tensors, both identities accumulated on the device against env.reward -- with no host wait until the loop is over, equal
to the host statement of the definition on the rows the loop left; an env that steps with red_actions records without the switch; bank slots;
the argument errors; check_errors() for an id out of range."""
import numpy as np
import pytest

from cage_challenge_4_amd import reward_terms as RT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('torch sees no device', allow_module_level=True)
from test_opponent_mix_torch import _random_actions, _side_stream  # noqa: E402  (after the skips above: that module imports torch)


def _env(n, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, **kw)


def _host(env, steps):
    v = env.venv
    tw = [RT.from_row(v.get_state(e), v.get_cold(e), steps) for e in range(env.num_envs)]
    return np.stack([t for t, _ in tw]), np.stack([w for _, w in tw])


def _loop(env, gen, K, red=None):
    """K steps on the current stream, nothing waits for the device: the number of valid rows, the rows that break an identity, the rows with a
    Restore cost and with a penalty, all as device scalars; the terms of the last step."""
    n, dev = env.num_envs, env.device
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    valid = torch.zeros_like(bad); costs = torch.zeros_like(bad); penalties = torch.zeros_like(bad)
    terms, words = env.reward_terms()
    assert terms.shape == (n, 9, 4) and terms.dtype == torch.int32 and words.shape == (n, 16) and words.dtype == torch.int32 and terms.device == dev
    ptrs = (terms.data_ptr(), words.data_ptr())
    for t in range(K):
        act = _random_actions(gen, n, dev)
        if red is None:
            obs, reward, done, info = env.step(act)
        else:
            obs, reward, done, info = env.step(act, red_actions=red)
        t2, w2 = env.reward_terms(out=(terms, words))
        assert t2 is terms and w2 is words and (terms.data_ptr(), words.data_ptr()) == ptrs
        v = words[:, 0] == 1
        first = (words[:, 3] + words[:, 4]).to(torch.float32) == reward
        second = words[:, 5:10].sum(1) + words[:, 10] == words[:, 3] + words[:, 4]
        brm = terms[:, :, :3].sum((1, 2)) == words[:, 3]
        bad += (v & ~(first & second & brm)).sum() + (~v & (terms.abs().sum((1, 2)) + words[:, 3:].abs().sum(1) != 0)).sum()
        valid += v.sum(); costs += (words[:, 4] != 0).sum(); penalties += (words[:, 3] != 0).sum()
    return terms, words, valid, bad, costs, penalties


def test_learner_loop_without_host_waits_out_reuse_and_the_identities_on_the_device():
    n, K, steps, seed = 48, 20, 60, 1310
    env = _env(n, steps=steps, rng_mode=1, strict=False)
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    env.reset(seeds=seed)
    env.enable_reward_terms()
    assert env.venv.reward_terms_enabled and env.venv.run_kernel_for(20) == env.venv.step_kernel
    with _side_stream(dev) as side:
        side.wait_stream(torch.cuda.default_stream(dev))
        terms, words, valid, bad, costs, penalties = _loop(env, gen, K)
        side.synchronize()                                   # the one wait
    assert int(bad) == 0 and int(valid) == n * K and int(costs) >= 10 and int(penalties) >= 50, (int(bad), int(valid), int(costs), int(penalties))
    want_t, want_w = _host(env, steps)
    assert np.array_equal(terms.cpu().numpy(), want_t) and np.array_equal(words.cpu().numpy(), want_w)
    assert (want_w[:, 1] == K).all() and (want_w[:, 0] == 1).all()
    env.check_errors()

    # the documented slices
    per_agent = words[:, 5:10].float()
    availability = terms[:, :, :2].sum((1, 2))
    compromise = terms[:, :, 2].sum(1)
    assert torch.equal(per_agent.sum(1) + words[:, 10], env.reward) and torch.equal((availability + compromise).to(torch.int32), words[:, 3])

    # bank slots: saved episodes read where they lie, after the env has moved on; then the switch off
    ids = torch.tensor([5, 40, 11], device=dev)
    bank = env.new_bank(4)
    env.save_episodes(ids, bank, torch.tensor([2, 0, 3], device=dev))
    env.step(_random_actions(gen, n, dev))
    bt, bw = env.reward_terms(ids=torch.tensor([2, 0, 3], device=dev), bank=bank)
    assert np.array_equal(bt.cpu().numpy(), want_t[[5, 40, 11]]) and np.array_equal(bw.cpu().numpy(), want_w[[5, 40, 11]])
    env.enable_reward_terms(False)
    assert not env.venv.reward_terms_enabled
    env.step(_random_actions(gen, n, dev))
    ot, ow = env.reward_terms()
    assert not ot.any() and (ow[:, 0] == 0).all() and (ow[:, 1] == K + 2).all() and not ow[:, 3:].any()
    env.check_errors()

    # out= of another shape, dtype or layout is refused; an id out of range gives zero rows and surfaces in check_errors()
    with pytest.raises(ValueError):
        env.reward_terms(out=(terms[:-1], words))
    with pytest.raises(ValueError):
        env.reward_terms(out=(terms, words.to(torch.int64)))
    with pytest.raises(ValueError):
        env.reward_terms(out=(terms.to(torch.uint8), words))
    with pytest.raises(ValueError):
        env.reward_terms(out=(terms, torch.zeros((16, n), dtype=torch.int32, device=dev).t()))
    with pytest.raises(ValueError):
        env.reward_terms(out=(terms.cpu(), words.cpu()))
    with pytest.raises(ValueError):
        env.reward_terms(ids=torch.tensor([0.5], device=dev))
    with pytest.raises(ValueError):
        env.reward_terms(bank=torch.zeros((2, 8), dtype=torch.uint8, device=dev))
    zt, zw = env.reward_terms(ids=torch.tensor([0, n, 3], device=dev))
    torch.cuda.synchronize(dev)
    assert not zt[1].any() and not zw[1].any() and zw[0, 1] == K + 2 and zw[2, 1] == K + 2
    from cage_challenge_4_amd.vec_env import CC4EngineError
    with pytest.raises(CC4EngineError):
        env.check_errors()
    env.check_errors()
    env.close()


def test_an_env_that_steps_with_red_actions_records_without_the_switch():
    n, K, steps, seed = 32, 12, 40, 1320
    env = _env(n, steps=steps, rng_mode=1, strict=False)
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(9)
    env.reset(seeds=seed)
    red = torch.full((n, 6, 4), -1, dtype=torch.int32, device=dev)          # every red agent: the scripted class acts
    with _side_stream(dev) as side:
        side.wait_stream(torch.cuda.default_stream(dev))
        terms, words, valid, bad, costs, penalties = _loop(env, gen, K, red=red)
        side.synchronize()
    assert not env.venv.reward_terms_enabled
    assert int(bad) == 0 and int(valid) == n * K and int(penalties) >= 20, (int(bad), int(valid), int(penalties))
    want_t, want_w = _host(env, steps)
    assert np.array_equal(terms.cpu().numpy(), want_t) and np.array_equal(words.cpu().numpy(), want_w)
    env.check_errors()
    env.close()
