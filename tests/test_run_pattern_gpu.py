"""Long persistent calls take the run pattern of run_config_for_call (csrc/cc4_sched.h): runs of RUN_LONG_SA or RUN_LONGER_SA steps and ONE closing run for what they leave
over.  The schedule never affects results, so the calls at the thresholds -- and at threshold + SA - 1, whose closing run is SA - 1 steps long -- must leave
every episode exactly where per-step launches (CC4_PERSIST_VERIFY's shadow handle) and the CPU oracle leave it.  40-step episodes: regenerations fall
inside runs, the closing run included.  5121 episodes: the smallest batch the persistent path serves (partitions of 20 / 21 episodes for 24 waves: waves
idle and help out)."""
import os
import re

import numpy as np
import pytest
from oracle_binding import OracleVecEnv, random_actions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5121


def _sched_constants():
    txt = open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'cc4_sched.h')).read()
    return {k: int(v) for k, v in re.findall(r'\b(RUN_LONG_K|RUN_LONG_SA|RUN_LONGER_K|RUN_LONGER_SA) = (\d+)', txt)}


C = _sched_constants()


def _dev(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    return CC4VecEnv(n, **kw)


def _last_split(dev):
    import ctypes
    out = (ctypes.c_int32 * 5)()
    assert dev.lib.cc4_debug_last_run_split(dev._h, out) == 0
    return tuple(out)


def test_only_the_headline_kernel_takes_the_long_call_pattern(monkeypatch):
    """k_run_philox1 cuts a 500-step call into runs of RUN_LONGER_SA and one closing run; k_run_pcg -- like every build that is not the headline one: the
    builds with the exchange hold a run against the ring of 32 step slabs, where a run of 24 steps stalls (csrc/cc4_sched.h) -- keeps run_split's default
    of 62 runs of 8 and 4 single steps (tests/test_sched_cpu.py::test_default_split_known_cases)."""
    monkeypatch.delenv('CC4_PERSIST_RUNS', raising=False)
    monkeypatch.delenv('CC4_PERSIST_VERIFY', raising=False)
    K, SA = C['RUN_LONGER_K'], C['RUN_LONGER_SA']
    assert (K, SA) == (500, 24)
    for rng_mode, kernel, want in ((1, 'k_run_philox1', (SA, K // SA, K % SA, 1, K // SA + 1)), (0, 'k_run_pcg', (8, 62, 1, 0, 66))):
        dev = _dev(N, steps=500, rng_mode=rng_mode, autoreset=True); dev.reset(seeds=5)
        assert dev.run_kernel_for(K) == kernel
        assert _last_split(dev) == (0, 0, 0, 0, 0)
        dev.run_random_steps(5, 0, K, timed=False); dev.synchronize()
        assert _last_split(dev) == want, (kernel, _last_split(dev))
        dev.run_random_steps(5, K, 20, timed=False); dev.synchronize()
        assert _last_split(dev) == (4, 5, 1, 0, 5), kernel
        assert not dev.err.any()
        dev.close()


def test_calls_at_the_thresholds_agree_with_per_step_launches(monkeypatch):
    """The self-check repeats each call with per-step launches on a shadow handle and compares hot rows, cold rows and outputs of all episodes."""
    monkeypatch.setenv('CC4_PERSIST_VERIFY', '1')
    monkeypatch.delenv('CC4_PERSIST_RUNS', raising=False)
    dev = _dev(N, steps=40, rng_mode=1, autoreset=True, strict=False); dev.reset(seeds=77)
    calls = (C['RUN_LONG_K'] - 1, C['RUN_LONG_K'], C['RUN_LONG_K'] + C['RUN_LONG_SA'] - 1, C['RUN_LONG_K'] + 1,
             C['RUN_LONGER_K'], C['RUN_LONGER_K'] + C['RUN_LONGER_SA'] - 1, 12)
    assert all(dev.run_kernel_for(K) == 'k_run_philox1' for K in calls)
    t = 0
    for K in calls:
        dev.run_random_steps(77, t, K, timed=False); t += K
    assert dev.verify_stats() == (len(calls), 0)
    assert not dev.err.any()
    dev.close()


@pytest.mark.parametrize('thr', [None, '0', '1000000'], ids=['thr_default', 'every_run_stolen', 'none_stolen'])
def test_long_calls_leave_every_row_equal_to_the_oracle(thr, monkeypatch):
    """After a short call, a call at the threshold and one whose closing run is SA - 1 steps long: outputs, drawn actions, generator states, every hot
    row and every 256th cold row against the oracle; once each with every run taken from the partition that lags most and with none (CC4_PERSIST_THR)."""
    monkeypatch.delenv('CC4_PERSIST_RUNS', raising=False)
    monkeypatch.delenv('CC4_PERSIST_VERIFY', raising=False)
    if thr is None:
        monkeypatch.delenv('CC4_PERSIST_THR', raising=False)
    else:
        monkeypatch.setenv('CC4_PERSIST_THR', thr)
    seed0 = 9100
    dev = _dev(N, steps=40, rng_mode=1, autoreset=True)
    ora = OracleVecEnv(N, steps=40, rng_mode=1, autoreset=True)
    assert np.array_equal(dev.reset(seeds=seed0), ora.reset_batch(seed0))
    t = 0
    for K in (12, C['RUN_LONG_K'], C['RUN_LONG_K'] + C['RUN_LONG_SA'] - 1):
        assert dev.run_kernel_for(K) == 'k_run_philox1'
        dev.run_random_steps(seed0, t, K, timed=False)
        for k in range(K):
            a = random_actions(seed0, t + k, N)
            o = ora.step_batch(a)
        t += K
        dev.synchronize(); dev._fetch()
        bad = np.nonzero((dev._obs != o[0]).any(axis=1) | (dev._rew != o[1]) | (dev._done.astype(bool) != o[2]) | (dev._err != o[3]['err']))[0]
        assert bad.size == 0, (K, t, bad[:10].tolist())
        assert np.array_equal(dev.device_actions(), a), (K, t)
        assert np.array_equal(dev.rng_state(), ora.rng_state()), (K, t)
        rows = dev.get_states()
        want = np.stack([ora.get_state(i) for i in range(N)])
        bad = np.nonzero((rows != want).any(axis=1))[0]
        assert bad.size == 0, (K, t, bad[:8].tolist())
        for i in range(0, N, 256):
            assert np.array_equal(dev.get_cold(i), ora.get_cold(i)), (K, t, i)
    dev.close(); ora.close()
