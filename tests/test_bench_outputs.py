"""bench.py --dump-outputs without a GPU: the writer of the last step's outputs (bench.dump_outputs) on a stand-in handle -- float32 /
float64 files of the caller's arrays, and above the size cap a fixed seeded sample of the episodes with their indices."""
import os

import numpy as np

import bench

NAMES = ('observations', 'rewards', 'dones', 'error_flags', 'actions')


class _Handle:
    """What dump_outputs reads of a CC4VecEnv: the fetched host arrays and the device action buffer."""

    def __init__(self, n):
        rng = np.random.default_rng(n)
        self.num_envs = n
        self._obs = rng.integers(0, 4, (n, 578), dtype=np.int32)
        self._rew = rng.normal(size=n).astype(np.float32)
        self._done = rng.integers(0, 2, n, dtype=np.uint8)
        self._err = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        self._act = rng.integers(0, 242, (n, 5), dtype=np.int32)

    def device_actions(self):
        return self._act.copy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_the_whole_batch_as_float(tmp_path):
    h = _Handle(64)
    bench.dump_outputs(str(tmp_path), h)
    got = _load(tmp_path)
    assert sorted(got) == sorted(NAMES)
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert np.array_equal(got['observations'], h._obs) and np.array_equal(got['rewards'], h._rew) and np.array_equal(got['dones'], h._done)
    assert np.array_equal(got['error_flags'], h._err) and np.array_equal(got['actions'], h._act)       # (uint32 flags exact in float64)


def test_dump_above_the_cap_is_a_fixed_sample_of_episodes(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_MAX_BYTES', 600_000)
    h = _Handle(1000)
    bench.dump_outputs(str(tmp_path / 'a'), h)
    bench.dump_outputs(str(tmp_path / 'b'), h)
    a, b = _load(tmp_path / 'a'), _load(tmp_path / 'b')
    assert sorted(a) == sorted(NAMES + ('episode_index',))
    assert all(np.array_equal(a[k], b[k]) for k in a)                   # the same sample every time
    idx = a['episode_index'].astype(np.int64)
    assert 0 < idx.size < 1000 and np.all(np.diff(idx) > 0) and idx[-1] < 1000
    assert np.array_equal(a['observations'], h._obs[idx]) and np.array_equal(a['actions'], h._act[idx])
    assert np.array_equal(a['error_flags'], h._err[idx]) and np.array_equal(a['dones'], h._done[idx])
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a')) <= 600_000
