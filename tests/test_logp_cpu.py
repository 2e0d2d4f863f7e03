"""CPU: log-probabilities of stored blue actions with gradients -- the surface (header, exports, bindings, the constant, the two kernels' resource
rows as committed in profiles/kernel_resources.txt); the float64 NumPy restatement (action_logp.reference) checked without the code under test,
its gradient against central differences of its own logp and entropy; the host functions (cc4_logp_actions_host, cc4_logp_actions_grad_host,
float32) against the restatement on mask rows of the CPU oracle and on the crafted rows; the refusals of the entry points; and the stand-alone check
of the serial statements (csrc/cc4_logp.h) against a double-precision formulation written without the header's helpers: tests/cpp/logp_check.cpp is
a program with its own main, built here with the host compiler at -O1 with the address and undefined-behaviour sanitizers and run as a child
process (never loaded into Python).  The tolerances: logp_util."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
import logp_util as LU
import sample_util as U
from cage_challenge_4_amd import action_logp as AL
from cpp_check import build_and_run

SRC = os.path.join(ROOT, 'tests', 'cpp', 'logp_check.cpp')
SEG = AL.SEGMENTS
NAMES = (('cc4_logp_actions_device', 9), ('cc4_logp_actions_grad_device', 10), ('cc4_logp_actions_host', 5), ('cc4_logp_actions_grad_host', 7))


def test_surface_header_exports_bindings_constant_and_resources():
    from cage_challenge_4_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, nargs in NAMES:
        assert re.search(r'\bint\s+' + sym + r'\s*\(', code), sym
        assert hasattr(lib, sym), sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs, sym
    assert re.search(r'#define CC4_LOGP_REFUSED\s+1\n', txt) and _lib.LOGP_REFUSED == 1 == AL.REFUSED
    assert AL.SEGMENTS == (0, 82, 164, 246, 328, 570) and AL.SLOTS == 570 and AL.NUM_BLUE == 5
    k_src = open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'cc4_k_logp.hip')).read()
    assert re.search(r'static_assert\(LP_REFUSED == CC4_LOGP_REFUSED', k_src)
    rows = [ln for ln in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')) if ln.rstrip().endswith('cc4_k_logp.hip')]
    assert len(rows) == 2 and sum('k_logp_fwd' in r for r in rows) == 1 and sum('k_logp_bwd' in r for r in rows) == 1, rows
    for row in rows:
        assert re.search(r'scratch\s+0 vgpr_spill\s+0 sgpr_spill\s+0 ', row), row
        assert int(re.search(r'lds_static\s+(\d+)', row).group(1)) <= 1280, row      # at most one of LDS's 1280-byte granules, or none
    # no kernel name of this unit matches the substrings other tests find their resource rows by
    for other in ('k_sample_actions', 'k_blue_view', 'k_red_view', 'k_red_submit', 'k_reward_terms', 'k_blue_edges', 'k_state_features'):
        assert not any(other in r for r in rows)


def test_importing_the_package_imports_neither_the_module_nor_torch():
    import subprocess
    prog = ('import sys; import cage_challenge_4_amd; assert "cage_challenge_4_amd.action_logp" not in sys.modules; '
            'import cage_challenge_4_amd.action_logp; assert "torch" not in sys.modules')
    run = subprocess.run([sys.executable, '-c', prog], cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


@pytest.fixture(scope='module')
def masks():
    return LU.oracle_masks(4)


def test_restatement_gradient_against_central_differences_of_itself(masks):
    """The formulas pinned without the code under test: d (sum g0 logp + g1 entropy) / d logits of reference() against central differences of
    reference()'s own logp and entropy in float64, step 1e-6, logits in [-5, 5], within 1e-7 max(1, |grad|)."""
    rng = np.random.default_rng(11)
    h = 1e-6
    worst = 0.0
    for e, T in ((0, 1.0), (1, 0.5), (2, 2.0)):
        mask = masks[e]
        lg = rng.uniform(-5.0, 5.0, 570)
        act = LU.stored_actions(rng, mask[None], skip=0.0)[0]
        if e == 2:
            act[1] = -1
        g = rng.uniform(-1.0, 1.0, (5, 2))
        grad = AL.reference(lg, mask, act, T, g)[3]
        slots = np.concatenate([np.nonzero(mask)[0][::7], (np.array(SEG[:5]) + act)[act >= 0], np.nonzero(~mask)[0][::9]])
        for f in slots:
            up, dn = lg.copy(), lg.copy()
            up[f] += h
            dn[f] -= h
            lu, eu, _ = AL.reference(up, mask, act, T)
            ld, ed, _ = AL.reference(dn, mask, act, T)
            num = ((g[:, 0] * (lu - ld)).sum() + (g[:, 1] * (eu - ed)).sum()) / (2 * h)
            assert abs(num - grad[f]) <= 1e-7 * max(1.0, abs(grad[f])), (e, T, int(f), num, grad[f])
            worst = max(worst, abs(num - grad[f]))
        assert not grad[~mask].any() and grad[SEG[1]:SEG[2]].any() == (e != 2)
    print(f'restatement against central differences: max difference {worst:.3g}')


def test_host_functions_against_the_restatement(masks):
    rng = np.random.default_rng(20250101)
    worst = [0.0, 0.0, 0.0]
    for rep in range(3):
        base = U.random_logits(rng, (4, 570))
        act = LU.stored_actions(rng, masks)
        g = rng.uniform(-1.0, 1.0, (4, 5, 2)).astype(np.float32)
        for code, (vals, _dev) in U.value_sets(base).items():
            for T in LU.TEMPERATURES:
                what = f'rep {rep} dtype {code} T {T}'
                aux, refused, grad = AL.from_rows(vals, masks, act, T, g)
                rl, rn, rr, rg = AL.reference(vals, masks, act, T, g)
                assert not refused.any() and not rr.any(), what
                a, b = LU.check_stats(aux[..., 0], aux[..., 1], rl, rn, what)
                c = LU.check_grad(grad, rg, T, 3, what)
                worst = [max(worst[0], a), max(worst[1], b), max(worst[2], c)]
                skipped = act == -1
                assert skipped.any() and not aux[skipped].any(), what
                for e in range(4):
                    for b_ in range(5):
                        if skipped[e, b_]:
                            assert not grad[e, SEG[b_]:SEG[b_ + 1]].any(), what
                assert not grad[~masks].any(), what
    print(f'host functions against the restatement: max |logp - ref| {worst[0]:.3g}, |entropy - ref| {worst[1]:.3g}, |grad - ref| {worst[2]:.3g}')


def test_crafted_rows_on_the_host(masks):
    rng = np.random.default_rng(5)
    rows = LU.crafted_rows(masks[0], rng)
    g = rng.uniform(-1.0, 1.0, (1, 5, 2)).astype(np.float32)
    for name, lg, mk, act, want_refused in rows:
        for T in LU.TEMPERATURES:
            what = f'{name}, T {T}'
            aux, refused, grad = AL.from_rows(lg[None], mk[None], act[None], T, g)
            rl, rn, rr, rg = AL.reference(lg[None], mk[None], act[None], T, g)
            assert tuple(np.nonzero(rr[0])[0]) == want_refused and refused[0] == len(want_refused), what
            LU.check_stats(aux[..., 0], aux[..., 1], rl, rn, what)
            LU.check_grad(grad, rg, T, 3, what)
            for b in range(5):
                if b in want_refused:
                    assert np.isnan(aux[0, b, 2]) and not aux[0, b, [0, 1, 3]].any() and not grad[0, SEG[b]:SEG[b + 1]].any(), what
                else:
                    assert not np.isnan(aux[0, b, 2]), what
            assert not grad[0][~mk].any(), what
            if want_refused:         # the other four agents: as without the cause
                _n, c_lg, c_mk, c_act, _r = rows[0]
                base_aux, base_ref, base_grad = AL.from_rows(c_lg[None], c_mk[None], c_act[None], T, g)
                for b in (b for b in range(5) if b not in want_refused):
                    assert np.array_equal(aux[0, b], base_aux[0, b]) and not base_ref[0], what
                    assert np.array_equal(grad[0, SEG[b]:SEG[b + 1]], base_grad[0, SEG[b]:SEG[b + 1]]), what
        if name == 'only the Sleep slot valid':
            assert not aux[0, :, :2].any() and not grad.any()                  # logp = 0, H = 0, the gradient exactly 0
        if name == 'the action on a valid -inf slot':
            assert np.isneginf(aux[0, :, 0]).all() and np.isfinite(grad).all()
        if name == 'every action -1':
            assert not aux.any() and not grad.any()
        if name == '-inf among the valid logits':
            assert np.isfinite(aux[..., :2]).all() and np.isfinite(grad).all()
    assert len(rows) >= 20


def test_refusals_of_the_entry_points():
    good = (np.zeros((2, 570), np.float32), np.ones((2, 570), bool), np.zeros((2, 5), np.int32))
    for fn in (AL.reference, AL.from_rows):
        for bad in ((good[0][:, :-1], good[1], good[2]), (good[0], good[1][:1], good[2]), (good[0], good[1], good[2][:, :4]),
                    (good[0].astype(np.int32), good[1], good[2]), (good[0], good[1], good[2].astype(np.float32))):
            with pytest.raises(ValueError):
                fn(*bad)
        with pytest.raises(ValueError, match='g must'):
            fn(*good, 1.0, np.zeros((2, 5), np.float32))
        for T in (0.0, -1.0, float('nan'), float('inf')):
            with pytest.raises(ValueError, match='temperature'):
                fn(*good, T)
    # the C entry points themselves: -2 for a null pointer or a bad temperature, on the host and -- before anything touches a device -- the device calls
    from cage_challenge_4_amd import _lib
    lib, vp = _lib.load(), ctypes.c_void_p
    lg, mk, ac = np.zeros(570, np.float32), np.ones(570, np.uint8), np.zeros(5, np.int32)
    aux, g, grad = np.zeros(20, np.float32), np.zeros(10, np.float32), np.zeros(570, np.float32)
    p = lambda a: a.ctypes.data_as(vp)      # noqa: E731
    assert lib.cc4_logp_actions_host(p(lg), p(mk), p(ac), 1.0, p(aux)) == 0
    assert lib.cc4_logp_actions_grad_host(p(lg), p(mk), p(ac), 1.0, p(aux), p(g), p(grad)) == 0
    for k in range(4):
        args = [p(lg), p(mk), p(ac), 1.0, p(aux)]
        args[k if k < 3 else 4] = None
        assert lib.cc4_logp_actions_host(*args) == -2
    for k in (0, 1, 2, 4, 5, 6):
        args = [p(lg), p(mk), p(ac), 1.0, p(aux), p(g), p(grad)]
        args[k] = None
        assert lib.cc4_logp_actions_grad_host(*args) == -2
    for T in (0.0, -1.0, float('nan'), float('inf')):
        assert lib.cc4_logp_actions_host(p(lg), p(mk), p(ac), T, p(aux)) == -2
        assert lib.cc4_logp_actions_grad_host(p(lg), p(mk), p(ac), T, p(aux), p(g), p(grad)) == -2
        assert lib.cc4_logp_actions_device(None, p(lg), 3, p(mk), p(ac), 1, T, p(aux), p(ac)) == -2
    for kw in (dict(dt=0), dict(dt=4), dict(n=-1), dict(lg=None), dict(aux=None), dict(fault=None)):
        a = dict(dt=3, n=1, lg=p(lg), aux=p(aux), fault=p(ac))
        a.update(kw)
        assert lib.cc4_logp_actions_device(None, a['lg'], a['dt'], p(mk), p(ac), a['n'], 1.0, a['aux'], a['fault']) == -2, kw
        assert lib.cc4_logp_actions_grad_device(None, a['lg'], a['dt'], p(mk), p(ac), a['n'], 1.0, a['aux'], p(g), p(grad) if a['fault'] else None) == -2, kw


def test_serial_statements_against_a_double_formulation_under_the_sanitizers(tmp_path):
    run = build_and_run(SRC, tmp_path, required=True, timeout=300, flags=['-ffp-contract=off'])
    assert ' 0 mismatches' in run.stdout, run.stdout
