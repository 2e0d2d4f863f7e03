"""GPU: the torch surface of "advantages and returns of a stored rollout".  advantages.gae on a real rollout of CC4TorchVecEnv(autoreset=True) --
65 episodes of 30 steps for 65 rows, so every episode ends twice; actions from sample_actions on random logits, so busy agents store -1; random
bfloat16 values of five heads: the skip rows (weight 0 for all five agents, in a call without actions) are exactly the rows whose previous done was
set, the engine returned reward 0 and done 0 on them (which pins the layout claim to the engine), adv and ret are within the rounding bound of the float64 restatement
with and without bootstrap, the weights agree with the -1 actions, one launch per call, out= reuses its storage.  The plain layout against the
definition as a learner writes it in PyTorch (gae_util.learner_loop, float64 on the CPU).  CC4TorchVecEnv.advantages forwards the env's autoreset;
the ValueErrors that need a device enqueue nothing."""
import numpy as np
import pytest

import gae_util as G
from cage_challenge_4_amd import advantages as AD

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('torch sees no device', allow_module_level=True)

N, STEPS, T, A = 65, 30, 65, 5
GAMMA, LAM = 0.99, 0.95


@pytest.fixture(scope='module')
def rollout():
    """The stored rollout, as tensors on the device, and the env that made it."""
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    env = CC4TorchVecEnv(N, steps=STEPS, rng_mode=1, autoreset=True)
    dev = env.device
    env.reset(seeds=3100)
    gen = torch.Generator(device=dev)
    gen.manual_seed(31)
    done0 = env.done.clone()
    rewards, dones = torch.zeros((T, N), device=dev), torch.zeros((T, N), dtype=torch.bool, device=dev)
    actions = torch.zeros((T, N, A), dtype=torch.int32, device=dev)
    for t in range(T):
        logits = torch.randn((N, 570), generator=gen, device=dev) * 3
        act, _stats = env.sample_actions(logits, seed=31, t=t)
        actions[t] = act
        _obs, reward, done, _info = env.step(act)
        rewards[t], dones[t] = reward, done
    env.check_errors()
    values = (torch.randn((T, N, A), generator=gen, device=dev) * 50).to(torch.bfloat16)
    last = (torch.randn((N, A), generator=gen, device=dev) * 50).to(torch.bfloat16)
    yield dict(env=env, rewards=rewards, dones=dones, done0=done0, actions=actions, values=values, last_value=last)
    env.close()


def _numpy(ro):
    return dict(rewards=ro['rewards'].cpu().numpy(), values=ro['values'].float().cpu().numpy(), last_value=ro['last_value'].float().cpu().numpy(),
                dones=ro['dones'].cpu().numpy().astype(np.uint8), done0=ro['done0'].cpu().numpy().astype(np.uint8), actions=ro['actions'].cpu().numpy())


def test_gae_on_a_real_autoreset_rollout(rollout):
    ro = rollout
    host = _numpy(ro)
    prev = np.concatenate((host['done0'][None], host['dones'][:-1])) != 0
    assert (host['dones'].sum(axis=0) == 2).all(), 'every episode ends twice'
    assert (host['actions'] == -1).any(), 'no busy agent in the rollout'
    for bootstrap in (False, True):
        before = dict(AD.launches)
        adv, ret, weight = AD.gae(ro['rewards'], ro['values'], ro['last_value'], ro['dones'], gamma=GAMMA, lam=LAM, done0=ro['done0'], actions=ro['actions'],
                                  autoreset=True, bootstrap=bootstrap)
        assert AD.launches['gae'] - before['gae'] == 1
        assert adv.shape == ret.shape == weight.shape == (T, N, A) and adv.dtype == ret.dtype == torch.float32 and weight.dtype == torch.bool
        assert not adv.requires_grad and not ret.requires_grad
        w = weight.cpu().numpy()
        # the skip rows -- weight 0 for all five agents; read off a call without actions, since a row on which all five agents are busy carries
        # five zero weights too -- are exactly the rows whose previous done was set, and on them the engine returned reward 0 and done 0
        bare = AD.gae(ro['rewards'], ro['values'], ro['last_value'], ro['dones'], gamma=GAMMA, lam=LAM, done0=ro['done0'], autoreset=True, bootstrap=bootstrap)
        assert torch.equal(bare[0], adv) and torch.equal(bare[1], ret)
        wb = bare[2].cpu().numpy()
        skip = ~wb.any(axis=2)
        assert np.array_equal(wb, np.broadcast_to(~skip[..., None], wb.shape))
        assert np.array_equal(skip, prev) and skip.sum() == 2 * N
        assert not w[skip].any()
        assert not host['rewards'][skip].any() and not host['dones'][skip].any()
        assert np.array_equal(w, ~skip[..., None] & (host['actions'] != -1))
        G.check(adv.cpu().numpy(), ret.cpu().numpy(), host, GAMMA, LAM, True, bootstrap, f'real rollout, bootstrap {bootstrap}')
        a = adv.cpu().numpy()
        assert not a[skip].any() and np.array_equal(ret.cpu().numpy()[skip], host['values'][skip])
        # out= reuses the triple
        ptrs = [x.data_ptr() for x in (adv, ret, weight)]
        keep = [x.clone() for x in (adv, ret, weight)]
        for x in (adv, ret):
            x.fill_(-1.0)
        before = dict(AD.launches)
        again = AD.gae(ro['rewards'], ro['values'], ro['last_value'], ro['dones'], gamma=GAMMA, lam=LAM, done0=ro['done0'], actions=ro['actions'],
                       autoreset=True, bootstrap=bootstrap, out=(adv, ret, weight))
        assert [x.data_ptr() for x in again] == ptrs and all(x is y for x, y in zip(again, (adv, ret, weight)))
        assert all(torch.equal(x, y) for x, y in zip(again, keep))
        assert AD.launches['gae'] - before['gae'] == 1
    # without done0 (None: all zero) nothing changes here: no episode was done before the first call
    assert not host['done0'].any()
    b = AD.gae(ro['rewards'], ro['values'], ro['last_value'], ro['dones'], gamma=GAMMA, lam=LAM, actions=ro['actions'], bootstrap=True)
    assert all(torch.equal(x, y) for x, y in zip(b, keep))


def test_no_rows_and_no_episodes_give_empty_outputs_and_no_launch(rollout):
    ro = rollout
    before = dict(AD.launches)
    for sl in ((slice(0, 0), slice(None)), (slice(None), slice(0, 0))):
        t, n = sl
        a, r, w = AD.gae(ro['rewards'][t, n].contiguous(), ro['values'][t, n].contiguous(), ro['last_value'][n].contiguous(), ro['dones'][t, n].contiguous(),
                         gamma=GAMMA, lam=LAM, done0=ro['done0'][n].contiguous(), actions=ro['actions'][t, n].contiguous())
        assert a.shape == r.shape == w.shape == ro['values'][t, n].shape and a.numel() == 0
        assert a.dtype == torch.float32 and w.dtype == torch.bool and a.device == ro['values'].device
    assert AD.launches == before


def test_env_advantages_forwards_the_envs_autoreset(rollout):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    ro = rollout
    args = (ro['rewards'], ro['values'], ro['last_value'], ro['dones'])
    kw = dict(gamma=GAMMA, lam=LAM, done0=ro['done0'], actions=ro['actions'])
    auto = AD.gae(*args, autoreset=True, **kw)
    plain = AD.gae(*args, autoreset=False, **kw)
    assert not torch.equal(auto[0], plain[0]) and not torch.equal(auto[2], plain[2])
    assert ro['env'].autoreset is True
    assert all(torch.equal(x, y) for x, y in zip(ro['env'].advantages(*args, **kw), auto))
    assert all(torch.equal(x, y) for x, y in zip(ro['env'].advantages(*args, bootstrap=True, **kw), AD.gae(*args, bootstrap=True, **kw)))
    env2 = CC4TorchVecEnv(4, steps=STEPS, rng_mode=1)
    assert env2.autoreset is False
    assert all(torch.equal(x, y) for x, y in zip(env2.advantages(*args, **kw), plain))
    with pytest.raises(ValueError, match='bootstrap'):
        env2.advantages(*args, bootstrap=True, **kw)
    env2.close()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
def test_plain_layout_against_the_learners_pytorch_loop(dtype):
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(17)
    for shape, heads in (((19, 65, 5), 1), ((19, 33, 2), 2), ((9, 64), 1)):
        Tn, Nn = shape[:2]
        An = shape[2] if len(shape) == 3 else 1
        ro = G.force_events(rng, G.random_rollout(rng, Tn, Nn, An, done_rate=0.2, heads=heads))
        vals = torch.from_numpy(ro['values']).to(dtype).reshape(shape)
        last = torch.from_numpy(ro['last_value']).to(dtype).reshape(shape[1:])
        rew = torch.from_numpy(ro['rewards'])
        if heads != 1 and len(shape) == 2:
            rew = rew[..., 0]
        dones = torch.from_numpy(ro['dones'])
        adv, ret, w = AD.gae(rew.to(dev), vals.to(dev), last.to(dev), dones.to(dev), gamma=GAMMA, lam=LAM, autoreset=False)
        assert adv.shape == shape and bool(w.all())
        g, l_ = float(np.float32(GAMMA)), float(np.float32(LAM))
        la, lr = G.learner_loop(torch, rew.double(), vals.double(), last.double(), dones, g, l_)
        seen = dict(ro, values=vals.float().numpy().reshape(Tn, Nn, An), last_value=last.float().numpy().reshape(Nn, An))
        G.check(adv.cpu().numpy(), ret.cpu().numpy(), seen, GAMMA, LAM, False, False, f'plain layout {dtype} {shape} heads {heads}',
                ref=(la.numpy().reshape(Tn, Nn, An), lr.numpy().reshape(Tn, Nn, An)))


def test_the_value_errors_that_need_a_device_enqueue_nothing(rollout):
    ro = rollout
    ok = {k: ro[k] for k in ('rewards', 'values', 'last_value', 'dones')}
    before = dict(AD.launches)

    def call(**kw):
        a = dict(ok, **{k: v for k, v in kw.items() if k in ok})
        rest = {k: v for k, v in kw.items() if k not in ok}
        return AD.gae(a['rewards'], a['values'], a['last_value'], a['dones'], gamma=GAMMA, lam=LAM, **rest)
    out = call()
    assert AD.launches['gae'] - before['gae'] == 1
    before = dict(AD.launches)
    nc = ro['values'].transpose(0, 1).contiguous().transpose(0, 1)          # the right shape, not contiguous
    assert nc.shape == ro['values'].shape and not nc.is_contiguous()
    for kw, match in ((dict(values=ro['values'].cpu()), 'values must be a contiguous CUDA tensor'), (dict(rewards=ro['rewards'].cpu()), 'rewards must be'),
                      (dict(dones=ro['dones'].cpu()), 'dones must be'), (dict(done0=ro['done0'].cpu()), 'done0 must be'),
                      (dict(actions=ro['actions'].cpu()), 'actions must be'), (dict(last_value=ro['last_value'].cpu()), 'last_value must be'),
                      (dict(values=nc), 'values must be a contiguous'), (dict(rewards=ro['rewards'].t().contiguous().t()), 'rewards must be a contiguous'),
                      (dict(out=tuple(x.cpu() for x in out)), 'out: adv must be a contiguous CUDA'),
                      (dict(out=(out[0], out[1], out[2].transpose(0, 1).contiguous().transpose(0, 1))), 'out: weight must be a contiguous')):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match='must be on the device of values'):
            call(dones=ro['dones'].to('cuda:1'))
    assert AD.launches == before
