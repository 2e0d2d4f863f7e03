"""GPU: episode copies through CC4TorchVecEnv -- clone / save / load with device index tensors on the caller's stream: undo across an
autoreset, a checkpoint that goes through host memory into a fresh env, the outputs a copy carries (no step needed), the faults of slots
that were never written or come from another configuration, and the ordering against a side stream."""
import ctypes
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
ACT_LEN = (82, 82, 82, 82, 242)


def _env(n, **kw):
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    return CC4TorchVecEnv(n, **kw)


def _random_actions(gen, n, dev):
    cols = [torch.randint(-1, ACT_LEN[b] + 1, (n, 1), generator=gen, device=dev) for b in range(5)]
    return torch.cat(cols, 1)


def _outputs(env):
    return [env.obs.clone(), env.reward.clone(), env.done.clone(), env.action_mask.clone(), env.err.clone()]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('n', [96, 8192])
@pytest.mark.parametrize('rng_mode', [0, 1], ids=['pcg64', 'philox'])
def test_undo_across_an_autoreset(rng_mode, n):
    """save_episodes of the whole batch, k steps across an autoreset, load_episodes, the same k steps again: the same outputs at every step,
    the same generator words and hot rows at the end; right after the load the outputs are those of the moment of the save."""
    env = _env(n, steps=20, rng_mode=rng_mode, autoreset=True, strict=False)
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    env.reset(seeds=17)
    for _ in range(6):
        env.step(_random_actions(gen, n, dev))
    A = [_random_actions(gen, n, dev) for _ in range(30)]
    ids = torch.arange(n, device=dev)
    bank = env.new_bank(n)
    env.save_episodes(ids, bank, ids.flip(0))           # slot n-1-e holds episode e
    saved = _outputs(env)
    first = []
    for a in A:
        env.step(a)
        first.append(_outputs(env))
    assert bool(first[-1][2].any()) or any(bool(o[2].any()) for o in first), 'no episode ended: the autoreset was not crossed'
    rng1, hot1 = env.venv.rng_state(), env.venv.get_states()
    env.load_episodes(bank, ids.flip(0).to(torch.int16), ids)
    assert _same(_outputs(env), saved)
    for t, a in enumerate(A):
        env.step(a)
        assert _same(_outputs(env), first[t]), t
    assert np.array_equal(env.venv.rng_state(), rng1)
    assert np.array_equal(env.venv.get_states(), hot1)
    env.check_errors()
    env.close()


def test_a_checkpoint_resumes_in_a_fresh_env_and_refuses_other_configurations():
    """Save all of env A, take the bank through host memory, load it into a fresh B of the same configuration: A and B stay identical for 200
    steps.  The same bank into an env of another episode length (steps=499 has the cold layout of 500) or RNG mode is a fault and leaves the
    destination as it was."""
    from cage_challenge_4_amd.vec_env import CC4EngineError
    n = 256
    A = _env(n, steps=500, rng_mode=1, autoreset=True)
    B = _env(n, steps=500, rng_mode=1, autoreset=True)
    dev = A.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(8)
    A.reset(seeds=100)
    B.reset(seeds=5000)
    for _ in range(40):
        A.step(_random_actions(gen, n, dev))
    ids = torch.arange(n, device=dev)
    bank = A.new_bank(n)
    A.save_episodes(ids, bank, ids)
    host = bank.cpu()
    B.load_episodes(host.to(dev), ids, ids)
    assert _same(_outputs(A), _outputs(B))
    for t in range(200):
        a = _random_actions(gen, n, dev)
        A.step(a)
        B.step(a)
        assert _same(_outputs(A), _outputs(B)), t
    assert np.array_equal(A.venv.get_states(), B.venv.get_states())
    assert np.array_equal(A.venv.rng_state(), B.venv.rng_state())
    A.check_errors()
    B.check_errors()
    for kw in (dict(steps=499, rng_mode=1), dict(steps=500, rng_mode=0)):
        C = _env(n, autoreset=True, **kw)
        C.reset(seeds=9)
        assert C.snapshot_bytes == A.snapshot_bytes
        before, out0 = C.venv.get_states(), _outputs(C)
        C.load_episodes(host.to(dev), ids, ids)
        with pytest.raises(CC4EngineError, match='SLOT_OF_ANOTHER_CONFIGURATION'):
            C.check_errors()
        assert np.array_equal(C.venv.get_states(), before) and _same(_outputs(C), out0), kw
        C.close()
    A.close()
    B.close()


def test_never_written_slots_are_faults_and_the_written_ones_load():
    from cage_challenge_4_amd.vec_env import CC4EngineError
    n = 32
    env = _env(n, steps=100, rng_mode=1)
    env.reset(seeds=np.arange(n, dtype=np.uint64) + 40)
    dev = env.device
    bank = env.new_bank(8)
    env.save_episodes(torch.tensor([3, 4], device=dev), bank, torch.tensor([1, 6], device=dev))
    env.check_errors()
    before = env.venv.get_states()
    env.load_episodes(bank, torch.tensor([0, 1, 6, 7, 8], device=dev), torch.tensor([10, 11, 12, 13, 14], device=dev))
    with pytest.raises(CC4EngineError) as got:
        env.check_errors()
    assert 'SLOT_NEVER_WRITTEN' in str(got.value) and 'INDEX_OUT_OF_RANGE' in str(got.value)
    after = env.venv.get_states()
    want = before.copy()
    want[11], want[12] = before[3], before[4]
    assert np.array_equal(after, want)
    env.check_errors()                                   # cleared
    env.close()


@pytest.mark.parametrize('side', [True, False], ids=['side_stream', 'default_stream'])
def test_copies_carry_their_outputs_and_order_against_the_callers_stream(side):
    """Right after clone_episodes / load_episodes, obs, reward, done and the action mask of every destination are its source's (the
    destinations' scenarios, and so their masks, differed); the index tensors are written on the caller's stream behind a delay and dropped
    at once.  Then both envs step on: the torch env against CC4VecEnv driven through the host clone, every step."""
    from cage_challenge_4_amd import CC4VecEnv
    n, T = 1024, 10
    env = _env(n, steps=60, rng_mode=1, autoreset=True)
    ref = CC4VecEnv(n, steps=60, rng_mode=1, autoreset=True)
    dev = env.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(21)
    A = torch.stack([_random_actions(gen, n, dev) for _ in range(2 * T)])
    env.reset(seeds=300)
    ref.reset(seeds=300)
    for t in range(T):
        env.step(A[t])
        ref.step(A[t].cpu().numpy())
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2))
    src, dst = perm[:200].to(dev), perm[200:400].to(dev)
    pre = _outputs(env)
    s_, d_ = src.long(), dst.long()
    assert not torch.equal(pre[3][d_], pre[3][s_])
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev) if side else torch.cuda.default_stream(dev)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(2_000_000)
        s1, d1 = src * 1, dst * 1
        env.clone_episodes(s1, d1)
        del s1, d1
        got = _outputs(env)
    torch.cuda.synchronize(dev)
    for k in range(4):
        assert torch.equal(got[k][d_], pre[k][s_]), k
        keep = torch.ones(n, dtype=torch.bool, device=dev)
        keep[d_] = False
        assert torch.equal(got[k][keep], pre[k][keep]), k
    ref.clone_episodes(src.cpu().numpy(), dst.cpu().numpy())
    assert np.array_equal(env.obs.cpu().numpy().astype(np.int32), ref._obs)
    assert np.array_equal(env.action_mask.cpu().numpy(), ref.action_mask)
    # a save / load round trip of other episodes on the side stream
    bank = env.new_bank(64)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(1_000_000)
        env.save_episodes(perm[400:464].to(dev), bank, torch.arange(64, device=dev))
        env.load_episodes(bank, torch.arange(64, device=dev), perm[500:564].to(dev))
        got = _outputs(env)
    torch.cuda.synchronize(dev)
    ref.clone_episodes(perm[400:464].numpy(), perm[500:564].numpy())
    assert np.array_equal(got[0].cpu().numpy().astype(np.int32), ref._obs) and np.array_equal(got[3].cpu().numpy(), ref.action_mask)
    for t in range(T, 2 * T):
        obs, rew, done, info = env.step(A[t])
        o2, r2, d2, _ = ref.step(A[t].cpu().numpy())
        assert np.array_equal(obs.cpu().numpy().astype(np.int32), o2) and np.array_equal(rew.cpu().numpy(), r2) and np.array_equal(done.cpu().numpy(), d2), t
    env.check_errors()
    env.close()
    ref.close()


def test_torch_copies_are_refused_with_a_communicator():
    import os
    from cage_challenge_4_amd._lib import CC4Error
    env = _env(8, steps=50, rng_mode=1)
    env.reset(seeds=1)
    os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
    ident = (ctypes.c_uint8 * 128)()
    assert env.lib.cc4_comm_unique_id(ident) == 0
    env.venv._chk(env.lib.cc4_comm_init(env._h, 0, 1, ident), 'cc4_comm_init')
    with pytest.raises(CC4Error, match='communicator'):
        env.clone_episodes(torch.tensor([0], device=env.device), torch.tensor([1], device=env.device))
    env.close()
