"""GPU: the torch surface of "log-probabilities of stored blue actions".  action_logp.evaluate_actions() under autograd against the same loss
through a plain PyTorch float64 CPU chain (masked_fill, segment log_softmax, gather, entropy) and its autograd gradient, on the default stream and
on a side stream; an input that does not require grad builds no backward; the ValueErrors enqueue nothing; check_errors(); and the agreement with
the sampler: a loop of sample_actions + step stores (logits, mask, actions, stats), and evaluate_actions on the stored tensors gives the sampler's
own logp and entropy, zero for the -1 agents.  The tolerances: logp_util."""
import numpy as np
import pytest

import logp_util as LU
import sample_util as U
from cage_challenge_4_amd import action_logp as AL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('torch sees no device', allow_module_level=True)

N, STEPS = 65, 30
SEG = AL.SEGMENTS
CODES = {torch.float32: 3, torch.bfloat16: 2, torch.float16: 1}


def torch_chain(logits, mask, actions, temperature):
    """The definition as a learner writes it in PyTorch, float64 on the CPU: (logp [B, 5], entropy [B, 5]); an action of -1 gives zeros."""
    x = logits.double() * float(np.float32(1.0) / np.float32(temperature))
    x = x.masked_fill(~mask, float('-inf'))
    logp, ent = [], []
    for b in range(5):
        ls = torch.log_softmax(x[:, SEG[b]:SEG[b + 1]], dim=1)
        a = actions[:, b].long()
        on = a >= 0
        logp.append(torch.where(on, ls.gather(1, a.clamp(min=0)[:, None])[:, 0], torch.zeros_like(ls[:, 0])))
        p = ls.exp()
        h = -(p * ls.masked_fill(p == 0, 0.0)).sum(dim=1)
        ent.append(torch.where(on, h, torch.zeros_like(h)))
    return torch.stack(logp, 1), torch.stack(ent, 1)


@pytest.fixture(scope='module')
def stored():
    """65 rows: oracle masks, random logits, stored actions with some -1, the weights of the loss."""
    rng = np.random.default_rng(65)
    mask = LU.oracle_masks(N)
    return dict(mask=mask, logits=U.random_logits(rng, (N, 570)), actions=LU.stored_actions(rng, mask),
                w=rng.uniform(-1.0, 1.0, (N, 5, 2)).astype(np.float32))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('side_stream', [False, True])
def test_evaluate_actions_under_autograd_against_a_float64_cpu_chain(stored, dtype, side_stream):
    dev = torch.device('cuda', 0)
    T = 0.5 if side_stream else 1.0
    mask_c, act_c, w_c = torch.from_numpy(stored['mask']), torch.from_numpy(stored['actions']), torch.from_numpy(stored['w']).double()
    lg_c = torch.from_numpy(stored['logits']).to(dtype)            # the values the dtype carries
    ref_in = lg_c.double().requires_grad_(True)
    rl, rn = torch_chain(ref_in, mask_c, act_c, T)
    (w_c[..., 0] * rl + w_c[..., 1] * rn).sum().backward()
    before = dict(AL.launches)
    stream = torch.cuda.Stream(dev) if side_stream else torch.cuda.current_stream(dev)
    lg = lg_c.to(dev).requires_grad_(True)
    mask, act, w = mask_c.to(dev), act_c.to(dev), torch.from_numpy(stored['w']).to(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        logp, ent = AL.evaluate_actions(lg, mask, act, T)
        (w[..., 0] * logp + w[..., 1] * ent).sum().backward()
    torch.cuda.current_stream(dev).wait_stream(stream)
    assert logp.shape == (N, 5) and ent.shape == (N, 5) and logp.dtype == torch.float32 and ent.dtype == torch.float32 and logp.requires_grad
    assert lg.grad.shape == lg.shape and lg.grad.dtype == dtype
    assert {k: AL.launches[k] - before[k] for k in before} == {'fwd': 1, 'bwd': 1}
    what = f'{dtype} side_stream {side_stream}'
    a, b = LU.check_stats(logp.detach().cpu().numpy(), ent.detach().cpu().numpy(), rl.detach().numpy(), rn.detach().numpy(), what)
    c = LU.check_grad(lg.grad.float().cpu().numpy(), ref_in.grad.numpy(), T, CODES[dtype], what)
    print(f'{what}: max |logp - ref| {a:.3g}, |entropy - ref| {b:.3g}, |grad - ref| {c:.3g}')
    skipped = stored['actions'] == -1
    assert skipped.any() and not logp.detach().cpu().numpy()[skipped].any()
    AL.check_errors(dev)


def test_no_backward_without_requires_grad_leading_shapes_refusals_and_check_errors(stored):
    from cage_challenge_4_amd.vec_env import CC4EngineError
    dev = torch.device('cuda', 0)
    lg = torch.from_numpy(stored['logits']).to(dev)
    mask, act = torch.from_numpy(stored['mask']).to(dev), torch.from_numpy(stored['actions']).to(dev)
    before = dict(AL.launches)
    logp, ent = AL.evaluate_actions(lg, mask, act)
    assert not logp.requires_grad and logp.grad_fn is None and not ent.requires_grad
    assert {k: AL.launches[k] - before[k] for k in before} == {'fwd': 1, 'bwd': 0}
    # leading dimensions are flattened; a uint8 mask is a bool mask; float16 logits
    l3, e3 = AL.evaluate_actions(lg[:60].reshape(4, 15, 570), mask[:60].reshape(4, 15, 570).to(torch.uint8), act[:60].reshape(4, 15, 5))
    assert l3.shape == (4, 15, 5) and torch.equal(l3.reshape(60, 5), logp[:60]) and torch.equal(e3.reshape(60, 5), ent[:60])
    lh, _eh = AL.evaluate_actions(lg.half(), mask, act, 2.0)
    assert lh.shape == (N, 5) and lh.dtype == torch.float32
    # the ValueErrors, before anything is enqueued
    before = dict(AL.launches)
    for bad in (lg[:, :-1], lg.double(), lg.long(), lg.cpu(), lg.t().contiguous().t(), 'x', lg.reshape(N, 5, 114)):
        with pytest.raises(ValueError, match='logits'):
            AL.evaluate_actions(bad, mask, act)
    for bad in (mask[:-1], mask.float(), mask.cpu(), mask.t().contiguous().t(), None):
        with pytest.raises(ValueError, match='mask'):
            AL.evaluate_actions(lg, bad, act)
    for bad in (act[:-1], act.long(), act.cpu(), act[:, :4], None):
        with pytest.raises(ValueError, match='actions'):
            AL.evaluate_actions(lg, mask, bad)
    for T in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='temperature'):
            AL.evaluate_actions(lg, mask, act, T)
    assert AL.launches == before
    AL.check_errors(dev)
    # a NaN logit on a valid slot: that agent zero, the others as before, and check_errors() raises once
    bad = lg.clone().requires_grad_(True)
    with torch.no_grad():
        bad[9, SEG[2] + U.SLEEP[2]] = float('nan')
    keep = torch.from_numpy(stored['actions']).clone()
    keep[9, 2] = U.SLEEP[2]
    l2, e2 = AL.evaluate_actions(bad, mask, keep.to(dev))
    (l2.sum() + e2.sum()).backward()
    assert float(l2.detach()[9, 2]) == 0.0 and float(e2.detach()[9, 2]) == 0.0 and not bad.grad[9, SEG[2]:SEG[3]].any() and bool(torch.isfinite(bad.grad).all())
    same = torch.ones((N, 5), dtype=torch.bool, device=dev)
    same[9, 2] = False
    assert torch.equal(l2.detach()[same], logp[same]) and torch.equal(e2.detach()[same], ent[same])
    with pytest.raises(CC4EngineError, match='CC4_LOGP_REFUSED'):
        AL.check_errors(dev)
    AL.check_errors(dev)


def test_agreement_with_the_sampler_on_a_stored_rollout():
    """65 episodes, counter mode, 6 steps; some agents submit a Restore, so that later steps have busy agents (-1).  evaluate_actions on the stored
    (logits, mask, actions) gives the sampler's own stats bit for bit -- the two kernels run one reduction (csrc/cc4_row_wave.h) on the same x -- and so within 2^-12 max(1, |v|)."""
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    env = CC4TorchVecEnv(N, steps=STEPS, rng_mode=1, autoreset=True)
    dev = env.device
    env.reset(seeds=7300)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    first = torch.tensor([[int(U.valid_slots(m, b)[0]) for b in range(5)] for m in env.action_mask.cpu().numpy()], dtype=torch.int32, device=dev)
    restore = first + torch.tensor([2 * 16 + 1] * 4 + [2 * 48 + 1], dtype=torch.int32, device=dev)      # Restore of the agent's first valid host
    eb = torch.arange(N, device=dev)[:, None] + torch.arange(5, device=dev)[None, :]
    store = []
    for t in range(6):
        logits = (torch.randn((N, 570), generator=gen, device=dev) * 3).to(torch.bfloat16 if t % 2 else torch.float32)
        actions, stats = env.sample_actions(logits, seed=11, t=t)
        store.append((logits, env.action_mask.clone(), actions.clone(), stats.clone()))
        submit = torch.where(((eb + t) % 3 == 0) & (actions >= 0), restore, actions)
        env.step(submit)
    busy = differ = total = 0
    for t, (logits, mask, actions, stats) in enumerate(store):
        logp, ent = env.evaluate_actions(logits, mask, actions)
        got = torch.stack((logp, ent), dim=-1).cpu().numpy()
        want, a = stats.cpu().numpy(), actions.cpu().numpy()
        assert not got[a == -1].any() and not want[a == -1].any(), t
        assert (np.abs(got - want) <= 2.0 ** -12 * np.maximum(1.0, np.abs(want))).all(), t
        busy += int((a == -1).sum())
        differ += int((got.view(np.uint32) != want.view(np.uint32)).sum())
        total += got.size
    assert busy > 0, 'no busy agent in the rollout'
    print(f'evaluate_actions against the sampler: {total} values, {busy} agents busy, {differ} values not bit-equal')
    assert differ == 0, f'{differ} of {total} values of evaluate_actions are not bit-equal to the sampler\'s stats'
    AL.check_errors(dev)
    env.check_errors()
    env.close()
