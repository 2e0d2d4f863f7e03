"""CPU: the masked sampling of blue actions from policy logits -- its surface (header, exports, bindings, constants, the kernel's resource row as
committed in profiles/kernel_resources.txt), the host function (cc4_sample_actions_from_row, float32) against the float64 NumPy restatement
(action_sampling.reference) on rows of the CPU oracle, crafted logits, the distribution of the draws, the refusals of the Python entry points,
and the stand-alone check of the serial statement (csrc/cc4_sample.h: sample_from_row) against a double-precision formulation written without
the header's helpers: tests/cpp/sample_check.cpp is a program with its own main, built here with the host compiler at -O1 with the address and
undefined-behaviour sanitizers and run as a child process (never loaded into Python).  The tolerances: sample_util."""
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT
import sample_util as U
from cage_challenge_4_amd import action_sampling as AS
from cpp_check import build_and_run

SRC = os.path.join(ROOT, 'tests', 'cpp', 'sample_check.cpp')
STEPS = 30


def test_surface_header_exports_bindings_constants_and_resources():
    import ctypes
    from cage_challenge_4_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, nargs in (('cc4_sample_actions_device', 13), ('cc4_sample_actions_from_row', 9)):
        assert re.search(r'\bint\s+' + sym + r'\s*\(', code), sym
        assert hasattr(lib, sym), sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs, sym
    assert re.search(r'#define CC4_SAMPLE_GREEDY\s+1\n', txt) and re.search(r'#define CC4_SAMPLE_BUSY\s+2\n', txt)
    assert (_lib.SAMPLE_GREEDY, _lib.SAMPLE_BUSY) == (1, 2) == (AS.GREEDY, AS.BUSY)
    assert f'#define CC4_SAMPLE_TAG 0x{AS.TAG:04X}\n' in txt and AS.TAG != 0xB10E
    assert AS.SEGMENTS == (0, 82, 164, 246, 328, 570) and AS.SLOTS == 570 == _lib.MASK_PER_ENV and AS.NUM_BLUE == 5
    assert AS.SEGMENTS == tuple(_lib.ACT_OFF) + (570,)
    # the definition ties its constants to the header
    k_src = open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'cc4_k_sample.hip')).read()
    assert re.search(r'static_assert\(SA_GREEDY == CC4_SAMPLE_GREEDY && SA_BUSY == CC4_SAMPLE_BUSY && SA_TAG == CC4_SAMPLE_TAG', k_src)
    rows = [ln for ln in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')) if 'k_sample_actions' in ln]
    assert len(rows) == 1 and rows[0].rstrip().endswith('cc4_k_sample.hip'), rows
    assert re.search(r'scratch\s+0 vgpr_spill\s+0 sgpr_spill\s+0 ', rows[0]), rows[0]
    # at most one of LDS's 1280-byte granules, or none
    assert int(re.search(r'lds_static\s+(\d+)', rows[0]).group(1)) <= 1280, rows[0]


@pytest.fixture(scope='module')
def rows():
    """Hot rows, mask rows and busy flags of 4 oracle episodes (counter mode) after 0, 1 and 7 steps; the agents submit a Restore on some steps,
    so that some are busy.  Episode 0 has the segment-edge slots (sample_util.edge_seed)."""
    from oracle_binding import OracleVecEnv
    seed = U.edge_seed(1, STEPS)
    ora = OracleVecEnv(4, steps=STEPS, rng_mode=1)
    ora.reset(seeds=seed)
    mask = ora.mask()
    out = []
    for t in range(8):
        if t in (0, 1, 7):
            hots = [ora.get_state(e) for e in range(4)]
            out.append((t, hots, mask, [U.busy_of(h, STEPS) for h in hots]))
        act = np.zeros((4, 5), np.int32)
        for e in range(4):
            act[e] = AS.from_row(ora.get_state(e), None, 77, t, e)[0]
            for b in range(5):
                if (e + b + t) % 3 == 0:            # Restore of the agent's first valid host
                    first = U.valid_slots(mask[e], b)[0]
                    act[e, b] = 2 * (16 if b < 4 else 48) + 1 + first
        ora.step(act)
    ora.close()
    assert any(bz.any() for _t, _h, _m, busy in out for bz in busy), 'no busy agent in the fixture'
    return out


def test_host_function_against_the_numpy_restatement(rows):
    rng = np.random.default_rng(20240611)
    tally = U.Tally()
    saw_busy_minus_one = False
    for t, hots, mask, busy in rows:
        for e, hot in enumerate(hots):
            base = U.random_logits(rng)
            for code, (vals, _dev) in U.value_sets(base).items():
                for greedy in (False, True):
                    for T in (1.0, 0.5):
                        for busy_aware in (True, False):
                            a, st, refused = AS.from_row(hot, vals, 5, t, e, T, greedy, busy_aware)
                            ref = AS.reference(mask[e], busy[e], vals, 5, t, e, T, greedy, busy_aware, details=True)
                            assert not refused
                            tally.check(a, st, ref, f'step {t} episode {e} dtype {code} greedy {greedy} T {T} busy_aware {busy_aware}')
                            if busy_aware:
                                assert ((a == -1) == busy[e]).all() and not st[busy[e]].any()
                                saw_busy_minus_one |= bool(busy[e].any())
                            else:
                                assert (a >= 0).all()
                            ok = a >= 0
                            assert mask[e][np.array(AS.SEGMENTS[:5])[ok] + a[ok]].all(), 'a masked slot was drawn'
            for greedy in (False, True):
                a, st, refused = AS.from_row(hot, None, 5, t, e, 1.0, greedy, False)
                if not greedy:                  # (greedy without logits is all ties, margin 0 by construction: checked exactly below, not tallied)
                    tally.check(a, st, AS.reference(mask[e], busy[e], None, 5, t, e, 1.0, greedy, False, details=True), f'step {t} episode {e}: no logits')
                nvalid = np.array([U.valid_slots(mask[e], b).size for b in range(5)])
                assert np.allclose(st[:, 0], -np.log(nvalid), atol=2.0 ** -12 * 6) and np.allclose(st[:, 1], np.log(nvalid), atol=2.0 ** -12 * 6)
                if greedy:
                    assert [int(a[b]) for b in range(5)] == [int(U.valid_slots(mask[e], b)[0]) for b in range(5)]      # all equal: the lowest index
    assert saw_busy_minus_one
    tally.close('host function against the restatement')


def test_crafted_logits(rows):
    _t, hots, mask, _busy = rows[0]
    hot, m = hots[0], mask[0]
    seg = AS.SEGMENTS
    for name, lg, b, k in U.crafted_edge_rows(m):
        for t in range(4):
            a, st, refused = AS.from_row(hot, lg, 9, t, 0, 1.0, False, False)
            assert a[b] == k and not refused, (name, t, a)
            assert abs(st[b, 0]) < 2.0 ** -12      # p = 1 / (1 + (valid - 1) e^-40)
    rng = np.random.default_rng(3)
    base = U.random_logits(rng)
    want = AS.from_row(hot, base, 9, 1, 0)
    # 3e38 and NaN on invalid slots only: no effect, no fault
    lg = base.copy()
    inv = np.nonzero(~m)[0]
    lg[inv[::2]], lg[inv[1::2]] = 3e38, np.nan
    got = AS.from_row(hot, lg, 9, 1, 0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not got[2]
    # -inf on all valid slots but one: that one is drawn, with logp = 0 (and entropy 0)
    lg = base.copy()
    keep = [int(U.valid_slots(m, b)[-1]) for b in range(5)]
    lg[m] = -np.inf
    for b in range(5):
        lg[seg[b] + keep[b]] = base[seg[b] + keep[b]]
    for greedy in (False, True):
        a, st, refused = AS.from_row(hot, lg, 9, 1, 0, 0.5, greedy, False)
        assert a.tolist() == keep and not st.any() and not refused
    # NaN on a valid slot, and all valid slots -inf: action -1, zero stats, return code 1; the other agents are unaffected
    for b, poison in ((0, 'nan'), (4, 'nan'), (2, 'inf'), (3, '-inf')):
        lg = base.copy()
        v = U.valid_slots(m, b)
        if poison == '-inf':
            lg[seg[b] + v] = -np.inf
        else:
            lg[seg[b] + v[-1]] = np.nan if poison == 'nan' else np.inf
        a, st, refused = AS.from_row(hot, lg, 9, 1, 0, 1.0, False, False)
        assert refused and a[b] == -1 and not st[b].any(), (b, poison, a)
        others = [x for x in range(5) if x != b]
        assert np.array_equal(a[others], want[0][others]) and np.array_equal(st[others], want[1][others]), (b, poison)
        ra = AS.reference(m, [False] * 5, lg, 9, 1, 0, 1.0, False, False)[0]
        assert ra[b] == -1 and np.array_equal(ra[others], a[others])


def _draw_counts(hot, lg, slots, seed):
    counts = np.zeros(slots.shape, np.int64)
    for e in range(64):
        for t in range(32):
            a = AS.from_row(hot, lg, seed, t, e, 1.0, False, False)[0]
            for b in range(5):
                hit = np.nonzero(slots[b] == a[b])[0]
                assert hit.size == 1, f'agent {b} drew slot {a[b]}, not one of {slots[b]}'
                counts[b, hit[0]] += 1
    return counts


def test_distribution_of_the_draws(rows):
    """2048 draws per agent over (e, t) = 64 x 32: Pearson chi-square against the probabilities below the 1e-6 quantile.  The draw is a fixed
    function of the seed: the test is deterministic."""
    _t, hots, mask, _busy = rows[0]
    hot, m = hots[0], mask[0]
    lg, slots = U.four_slot_logits(m)
    counts = _draw_counts(hot, lg, slots, seed=1)
    expect = 2048 * np.array([0.4, 0.3, 0.2, 0.1])
    chi = ((counts - expect) ** 2 / expect).sum(axis=1)
    print('four slots: counts', counts.tolist(), 'chi-square', chi.round(2).tolist())
    assert (chi < U.chi2_bound(3)).all(), chi
    # no logits: uniform over the agent's valid slots
    for b in range(5):
        v = U.valid_slots(m, b)
        c = np.zeros(AS.SEGMENTS[b + 1] - AS.SEGMENTS[b], np.int64)
        for e in range(64):
            for t in range(32):
                c[AS.from_row(hot, None, 1, t, e, 1.0, False, False)[0][b]] += 1
        assert c.sum() == 2048 and not c[np.setdiff1d(np.arange(c.size), v)].any()
        chi_u = ((c[v] - 2048 / v.size) ** 2 / (2048 / v.size)).sum()
        print(f'uniform, agent {b}: {v.size} valid slots, chi-square {chi_u:.1f} (bound {U.chi2_bound(v.size - 1):.1f})')
        assert chi_u < U.chi2_bound(v.size - 1)


def test_refusals_of_the_python_entry_points():
    from cage_challenge_4_amd import _lib
    from cage_challenge_4_amd.vec_env import CC4VecEnv
    hot = np.zeros(_lib.load().cc4_state_bytes(), np.uint8)
    good = np.zeros(570, np.float32)
    for bad in (np.zeros(569, np.float32), np.zeros((2, 570), np.float32), np.zeros((570, 1), np.float32)):
        with pytest.raises(ValueError, match='shape'):
            AS.from_row(hot, bad, 0, 0, 0)
    for bad in (np.zeros(570, np.int32), np.zeros(570, bool), np.zeros(570, np.uint8)):
        with pytest.raises(ValueError, match='floating'):
            AS.from_row(hot, bad, 0, 0, 0)
    for T in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='temperature'):
            AS.from_row(hot, good, 0, 0, 0, T)
        with pytest.raises(ValueError, match='temperature'):
            AS.reference(np.ones(570, bool), [0] * 5, good, 0, 0, 0, T)
    with pytest.raises(ValueError, match='bytes'):
        AS.from_row(hot[:-1], good, 0, 0, 0)
    with pytest.raises(ValueError, match='shape'):
        AS.reference(np.ones(569, bool), [0] * 5, good, 0, 0, 0)
    # the C entry point itself
    lib, vp = _lib.load(), __import__('ctypes').c_void_p
    a, st = np.zeros(5, np.int32), np.zeros(10, np.float32)
    call = lambda h, T, fl, ap: lib.cc4_sample_actions_from_row(h, None, 0, 0, 0, T, fl, ap, st.ctypes.data_as(vp))      # noqa: E731
    assert call(hot.ctypes.data_as(vp), 1.0, 3, a.ctypes.data_as(vp)) == 0
    for args in ((None, 1.0, 0, a.ctypes.data_as(vp)), (hot.ctypes.data_as(vp), 1.0, 0, None), (hot.ctypes.data_as(vp), 0.0, 0, a.ctypes.data_as(vp)),
                 (hot.ctypes.data_as(vp), float('nan'), 0, a.ctypes.data_as(vp)), (hot.ctypes.data_as(vp), 1.0, 4, a.ctypes.data_as(vp))):
        assert call(*args) == -2, args
    # CC4VecEnv.sample_actions refuses before it touches the device (no env can be made here: the checks run on a stand-in for self)
    stand_in = types.SimpleNamespace(num_envs=2)
    for kw in (dict(logits=np.zeros((3, 570), np.float32)), dict(logits=np.zeros((2, 569), np.float32)), dict(logits=np.zeros(570, np.float32))):
        with pytest.raises(ValueError, match='shape'):
            CC4VecEnv.sample_actions(stand_in, **kw)
    for kw in (dict(logits=np.zeros((2, 570), np.int32)), dict(logits=np.zeros((2, 570), np.uint8))):
        with pytest.raises(ValueError, match='float16'):
            CC4VecEnv.sample_actions(stand_in, **kw)
    for T in (0.0, -0.5, float('nan')):
        with pytest.raises(ValueError, match='temperature'):
            CC4VecEnv.sample_actions(stand_in, logits=np.zeros((2, 570), np.float32), temperature=T)


def test_serial_statement_against_a_double_formulation_under_the_sanitizers(tmp_path):
    run = build_and_run(SRC, tmp_path, required=True, timeout=300, flags=['-ffp-contract=off'])
    assert ' 0 mismatches' in run.stdout, run.stdout
