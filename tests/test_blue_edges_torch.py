"""GPU: the torch surface of the Monitor's connection edges.  CC4TorchVecEnv.blue_edges() in a learner's loop on a side stream -- a step, the edge
lists into the same tensors, their validity mask -- with no host wait until the loop is over, equal to the host statement of the definition
on the rows the loop left; max_edges=32; id lists and bank slots; to_edge_index against a NumPy construction; check_errors()."""
import numpy as np
import pytest

from cage_challenge_4_amd import blue_edges as BE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('torch sees no device', allow_module_level=True)
from test_opponent_mix_torch import _random_actions, _side_stream  # noqa: E402  (after the skips above: that module imports torch)


def _env(n, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, **kw)


def _host_edges(env, steps, E):
    v = env.venv
    ec = [BE.from_row(v.get_state(e), v.get_cold(e), steps, E) for e in range(env.num_envs)]
    return np.stack([e for e, _ in ec]), np.stack([c for _, c in ec])


def _edge_index_numpy(edges, agent=None):
    n, E, _ = edges.shape
    src, dst, rows = [], [], []
    for e in range(n):
        for k in range(E):
            r = edges[e, k]
            if r[0] >= 0 and (agent is None or r[0] == agent):
                src.append(e * 137 + r[3]); dst.append(e * 137 + r[1]); rows.append(e * E + k)
    return np.array([src, dst], np.int64).reshape(2, -1), np.array(rows, np.int64)


def test_learner_loop_without_host_waits_out_reuse_ids_banks_and_edge_index():
    n, K, steps, seed = 48, 20, 60, 1210
    env = _env(n, steps=steps, rng_mode=1, strict=False)
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(4)
    env.reset(seeds=seed)
    env.enable_event_log(True)
    edge_seen = torch.zeros((), dtype=torch.int64, device=dev)
    with _side_stream(dev) as side:
        side.wait_stream(torch.cuda.default_stream(dev))
        edges, counts = env.blue_edges()
        assert edges.shape == (n, 160, 8) and edges.dtype == torch.int32 and counts.shape == (n, 8) and counts.dtype == torch.int32 and edges.device == dev
        small = env.blue_edges(max_edges=32)
        assert small[0].shape == (n, 32, 8)
        ptrs = (edges.data_ptr(), counts.data_ptr(), small[0].data_ptr(), small[1].data_ptr())
        for t in range(K):                                   # twenty iterations enqueued; nothing here waits for the device
            obs, reward, done, info = env.step(_random_actions(gen, n, dev))
            e2, c2 = env.blue_edges(out=(edges, counts))
            s2 = env.blue_edges(out=small, max_edges=32)
            assert e2 is edges and c2 is counts and s2[0] is small[0] and (edges.data_ptr(), counts.data_ptr(), small[0].data_ptr(), small[1].data_ptr()) == ptrs
            edge_seen += (edges[..., 0] >= 0).sum()          # the validity mask, used on the same stream
        side.synchronize()                                   # the one wait
    want_e, want_c = _host_edges(env, steps, 160)
    got_e = edges.cpu().numpy()
    assert np.array_equal(got_e, want_e) and np.array_equal(counts.cpu().numpy(), want_c)
    assert np.array_equal(small[0].cpu().numpy(), want_e[:, :32]) and np.array_equal(small[1].cpu().numpy(), want_c)
    assert (want_c[:, 7] == K).all() and (want_c[:, 6] == 1).all() and want_c[:, 5].sum() > 0 and int(edge_seen) > 0
    env.check_errors()

    # to_edge_index against a NumPy construction: all agents, one agent, a single episode's list
    for agent in (None, 0, 4):
        ei, rows = BE.to_edge_index(edges, agent)
        w_ei, w_rows = _edge_index_numpy(got_e, agent)
        assert ei.dtype == torch.int64 and rows.dtype == torch.int64 and ei.device == dev and tuple(ei.shape) == (2, len(w_rows))
        assert np.array_equal(ei.cpu().numpy(), w_ei) and np.array_equal(rows.cpu().numpy(), w_rows), agent
    busiest = int(np.argmax(want_c[:, 5]))
    ei, rows = BE.to_edge_index(edges[busiest])
    w_ei, w_rows = _edge_index_numpy(got_e[busiest:busiest + 1])
    assert np.array_equal(ei.cpu().numpy(), w_ei) and np.array_equal(rows.cpu().numpy(), w_rows) and len(w_rows) == want_c[busiest, 5] > 0

    # an id list; bank slots: saved episodes read where they lie, after the env has moved on
    ids = torch.tensor([5, 40, 11], device=dev)
    ie, ic = env.blue_edges(ids=ids, max_edges=32)
    assert np.array_equal(ie.cpu().numpy(), want_e[[5, 40, 11], :32]) and np.array_equal(ic.cpu().numpy(), want_c[[5, 40, 11]])
    bank = env.new_bank(4)
    env.save_episodes(ids, bank, torch.tensor([2, 0, 3], device=dev))
    env.step(_random_actions(gen, n, dev))
    be, bc = env.blue_edges(ids=torch.tensor([2, 0, 3], device=dev), bank=bank)
    assert np.array_equal(be.cpu().numpy(), want_e[[5, 40, 11]]) and np.array_equal(bc.cpu().numpy(), want_c[[5, 40, 11]])
    env.check_errors()

    # out= of another shape or dtype and a max_edges out of range are refused; an id out of range gives -1 rows and surfaces in check_errors()
    with pytest.raises(ValueError):
        env.blue_edges(out=(edges[:-1], counts))
    with pytest.raises(ValueError):
        env.blue_edges(out=(edges, counts.to(torch.int64)))
    with pytest.raises(ValueError):
        env.blue_edges(out=(edges, counts), max_edges=32)
    with pytest.raises(ValueError):
        env.blue_edges(max_edges=0)
    now_e, now_c = _host_edges(env, steps, 160)
    ze, zc = env.blue_edges(ids=torch.tensor([0, n, 3], device=dev))
    torch.cuda.synchronize(dev)
    assert bool((ze[1] == -1).all()) and not zc[1].any() and np.array_equal(ze[2].cpu().numpy(), now_e[3]) and np.array_equal(zc[0].cpu().numpy(), now_c[0])
    from cage_challenge_4_amd.vec_env import CC4EngineError
    with pytest.raises(CC4EngineError):
        env.check_errors()
    env.check_errors()
    env.close()
