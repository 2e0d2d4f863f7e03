"""GPU: CC4TorchVecEnv.state_features -- device tensors of the right shapes, equal to the NumPy surface; ordered on the caller's stream in both
directions inside a loop of steps with no synchronise; faults through check_errors()."""
import numpy as np
import pytest

from cage_challenge_4_amd import state_features as SF

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
ACT_LEN = (82, 82, 82, 82, 242)
SLOT_HDR = 64          # a snapshot slot: 64-byte header, then the hot row (include/cc4.h cc4_snapshot_bytes)


def _env(n, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, **kw)


def _random_actions(gen, n, dev):
    cols = [torch.randint(-1, ACT_LEN[b] + 1, (n, 1), generator=gen, device=dev) for b in range(5)]
    return torch.cat(cols, 1)


def _from_rows(rows):
    hg = [SF.from_row(r) for r in rows]
    return np.stack([h for h, _ in hg]), np.stack([g for _, g in hg])


def test_tensors_match_the_numpy_surface_and_banks_are_read_in_place():
    n = 64
    env = _env(n, steps=40, rng_mode=1)
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    env.reset(seeds=31)
    for _ in range(6):
        env.step(_random_actions(gen, n, dev))
    hosts, glob = env.state_features()
    assert hosts.shape == (n, 137, 16) and hosts.dtype == torch.uint8 and hosts.device == dev
    assert glob.shape == (n, 32) and glob.dtype == torch.int32 and glob.device == dev
    nh, ng = env.venv.state_features()
    assert np.array_equal(hosts.cpu().numpy(), nh) and np.array_equal(glob.cpu().numpy(), ng)
    want_h, want_g = _from_rows(env.venv.get_states())
    assert np.array_equal(nh, want_h) and np.array_equal(ng, want_g)
    ids = torch.tensor([9, 3, 3, 63, 0], device=dev, dtype=torch.int64)
    h2, g2 = env.state_features(ids=ids)
    assert torch.equal(h2, hosts[ids]) and torch.equal(g2, glob[ids])
    # out= reuses the caller's tensors
    oh, og = torch.full((5, 137, 16), 7, dtype=torch.uint8, device=dev), torch.full((5, 32), 7, dtype=torch.int32, device=dev)
    r = env.state_features(ids=ids.to(torch.int16), out=(oh, og))
    assert r[0] is oh and r[1] is og and torch.equal(oh, h2) and torch.equal(og, g2)
    with pytest.raises(ValueError):
        env.state_features(ids=ids, out=(oh[:4], og[:4]))
    # a search evaluates saved states without loading them
    bank = env.new_bank(8)
    env.save_episodes(torch.arange(10, 16, device=dev), bank, torch.arange(6, device=dev))
    for _ in range(3):
        env.step(_random_actions(gen, n, dev))
    bh, bg = env.state_features(ids=torch.tensor([5, 0, 2], device=dev), bank=bank)
    assert torch.equal(bh, hosts[[15, 10, 12]]) and torch.equal(bg, glob[[15, 10, 12]])
    assert not torch.equal(env.state_features()[1][:, 0], glob[:, 0])
    env.check_errors()
    env.close()


def test_loop_on_a_side_stream_is_ordered_both_ways_without_a_synchronise():
    """Ten times step() + state_features(out=...) on a non-default stream, and after every step the engine's own device snapshot of every
    episode (save_episodes into a fresh bank).  The `out` tensors (cloned on the same stream) match from_row of the snapshots' hot rows: the
    features saw the step before them, and the next step did not overtake the reader."""
    n, K = 64, 10
    env = _env(n, steps=40, rng_mode=1, autoreset=True)
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    env.reset(seeds=77)
    acts = [_random_actions(gen, n, dev) for _ in range(K)]
    ids = torch.arange(n, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    got, banks = [], []
    with torch.cuda.stream(side):
        oh = torch.zeros((n, 137, 16), dtype=torch.uint8, device=dev)
        og = torch.zeros((n, 32), dtype=torch.int32, device=dev)
        for a in acts:
            env.step(a)
            env.state_features(out=(oh, og))
            bank = env.new_bank(n)
            env.save_episodes(ids, bank, ids)
            got.append((oh.clone(), og.clone()))
            banks.append(bank)
    side.synchronize()
    nb = int(env.lib.cc4_state_bytes())
    for t in range(K):
        rows = banks[t].cpu().numpy()[:, SLOT_HDR:SLOT_HDR + nb]
        want_h, want_g = _from_rows(rows)
        assert (want_g[:, 0] == t + 1).all()
        assert np.array_equal(got[t][0].cpu().numpy(), want_h) and np.array_equal(got[t][1].cpu().numpy(), want_g), t
    env.check_errors()
    env.close()


def test_faulty_ids_surface_through_check_errors():
    from cage_challenge_4_amd.vec_env import CC4EngineError
    n = 64
    env = _env(n, steps=40, rng_mode=1)
    dev = env.device
    env.reset(seeds=1)
    hosts, glob = env.state_features()
    h2, g2 = env.state_features(ids=torch.tensor([4, n, 7], device=dev))
    with pytest.raises(CC4EngineError, match='INDEX_OUT_OF_RANGE'):
        env.check_errors()
    assert not h2[1].any() and not g2[1].any() and torch.equal(h2[0], hosts[4]) and torch.equal(h2[2], hosts[7]) and torch.equal(g2[2], glob[7])
    bank = env.new_bank(4)
    h3, _ = env.state_features(ids=torch.tensor([2], device=dev), bank=bank)      # a slot nobody wrote
    with pytest.raises(CC4EngineError, match='SLOT_NEVER_WRITTEN'):
        env.check_errors()
    assert not h3.any()
    env.check_errors()
    env.close()
