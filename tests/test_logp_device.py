"""GPU: log-probabilities of stored blue actions on the device.  cc4_logp_actions_device (k_logp_fwd) and cc4_logp_actions_grad_device (k_logp_bwd)
against the float64 restatement (action_logp.reference, evaluated on the values the dtype carries) and against the host statement of the same
definition (action_logp.from_rows): 1, 5 and 65 rows -- one row, a partly filled workgroup, more than one workgroup -- the three dtypes, three
temperatures, logits and gradients that start at an odd element of their allocation and masks at an odd byte; the crafted rows, where the refused
ones set the fault word and only that bit; n == 0 and the refusals enqueue nothing.  The calls take plain device pointers and the null stream: no
env, no torch.  The tolerances: logp_util; device against host is two float32 results, each within its bound of the restatement: twice the bound."""
import ctypes

import numpy as np
import pytest

import logp_util as LU
import sample_util as U
from bf16_util import upcast
from cage_challenge_4_amd import action_logp as AL
from view_util import DevMem

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
SEG = AL.SEGMENTS
ITEM = {3: 4, 2: 2, 1: 2}


def _lib():
    from cage_challenge_4_amd import _lib
    return _lib.load()


def _run(dev_logits, code, mask, act, T, g, fill=0x5A):
    """Both kernels on n rows: (aux [n, 5, 4], grad [n, 570] as float32 values, the fault word).  The logits and the gradient start one element
    into their allocations, the mask one byte into its own; every output byte is `fill` before the calls."""
    lib = _lib()
    n, it = dev_logits.shape[0], ITEM[code]
    assert dev_logits.shape == (n, 570) and dev_logits.dtype.itemsize == it
    d_lg, d_mk, d_ac = DevMem(n * 570 * it + it), DevMem(n * 570 + 1), DevMem(n * 20)
    d_aux, d_g, d_grad, d_fault = DevMem(n * 80, fill), DevMem(n * 40), DevMem(n * 570 * it + it, fill), DevMem(4)
    d_lg.up(dev_logits, it)
    d_mk.up(np.ascontiguousarray(mask, np.uint8) * np.uint8(0xFF), 1)      # (any non-zero byte is "valid")
    d_ac.up(np.ascontiguousarray(act, np.int32))
    d_g.up(np.ascontiguousarray(g, np.float32))
    assert d_lg.hip.hipDeviceSynchronize() == 0
    f = ctypes.c_float(T)
    assert lib.cc4_logp_actions_device(None, d_lg.at(it), code, d_mk.at(1), d_ac.p, n, f, d_aux.p, d_fault.p) == 0
    assert lib.cc4_logp_actions_grad_device(None, d_lg.at(it), code, d_mk.at(1), d_ac.p, n, f, d_aux.p, d_g.p, d_grad.at(it)) == 0
    assert d_lg.hip.hipDeviceSynchronize() == 0
    aux = d_aux.down(np.float32, (n, 5, 4))
    raw = d_grad.down(np.uint8, d_grad.nbytes)
    assert (raw[:it] == fill).all(), 'the element in front of the gradient was written'
    grad = upcast(raw[it:].copy().view({3: np.float32, 2: np.uint16, 1: np.float16}[code]).reshape(n, 570))
    fault = int(d_fault.down(np.int32, 1)[0])
    for m in (d_lg, d_mk, d_ac, d_aux, d_g, d_grad, d_fault):
        m.free()
    return aux, grad, fault


@pytest.fixture(scope='module')
def masks():
    return LU.oracle_masks(65)


@pytest.mark.parametrize('n', [1, 5, 65])
def test_kernels_against_the_restatement_and_the_host_functions(masks, n):
    rng = np.random.default_rng(100 + n)
    mk = masks[:n]
    base = U.random_logits(rng, (n, 570))
    act = LU.stored_actions(rng, mk)
    if n == 1:
        act[0] = LU.edge_actions(mk[0])[3][0]              # slot 241 of agent 4, the Sleep slots of the others
        act[0, 2] = -1
    g = rng.uniform(-1.0, 1.0, (n, 5, 2)).astype(np.float32)
    worst = [0.0, 0.0, 0.0]
    for code, (vals, dev_arr) in U.value_sets(base).items():
        for T in LU.TEMPERATURES:
            what = f'n {n} dtype {code} T {T}'
            aux, grad, fault = _run(dev_arr, code, mk, act, T, g)
            rl, rn, rr, rg = AL.reference(vals, mk, act, T, g)
            assert fault == 0 and not rr.any(), what
            a, b = LU.check_stats(aux[..., 0], aux[..., 1], rl, rn, what)
            c = LU.check_grad(grad, rg, T, code, what)
            worst = [max(worst[0], a), max(worst[1], b), max(worst[2], c)]
            haux, hrefused, hgrad = AL.from_rows(vals, mk, act, T, g)
            assert not hrefused.any(), what
            assert (np.abs(aux - haux) <= 2 * 2.0 ** -12 * np.maximum(1.0, np.abs(haux))).all(), what
            tol = 2 * 2.0 ** -12 * max(1.0, 1.0 / T) * np.maximum(1.0, np.abs(hgrad)) + LU.out_tolerance(hgrad, code)
            assert (np.abs(grad - hgrad) <= tol).all(), what
            skipped = act == -1
            assert skipped.any() and not aux[skipped].any(), what
            for e, b_ in np.argwhere(skipped):
                assert not grad[e, SEG[b_]:SEG[b_ + 1]].any(), what
            assert not grad[~mk].any(), what
    print(f'kernels against the restatement, n = {n}: max |logp - ref| {worst[0]:.3g}, |entropy - ref| {worst[1]:.3g}, |grad - ref| {worst[2]:.3g}')


def test_crafted_rows_and_the_fault_word(masks):
    """The crafted rows of the CPU test as one batch per dtype: a refused agent leaves the other agents of its row and the other rows as they are,
    and the fault word carries CC4_LOGP_REFUSED and nothing else; without a refused row it stays zero."""
    rng = np.random.default_rng(5)
    rows = LU.crafted_rows(masks[0], rng)
    n = len(rows)
    lg = np.stack([r[1] for r in rows])
    mk = np.stack([r[2] for r in rows])
    act = np.stack([r[3] for r in rows])
    g = np.tile(rng.uniform(-1.0, 1.0, (1, 5, 2)).astype(np.float32), (n, 1, 1))      # (one g for every row: rows are compared with each other)
    clean = [k for k, r in enumerate(rows) if not r[4]]
    for code, (vals, dev_arr) in U.value_sets(lg).items():
        for T in (0.5, 1.0):
            what = f'dtype {code} T {T}'
            aux, grad, fault = _run(dev_arr, code, mk, act, T, g)
            assert fault == AL.REFUSED, what
            rl, rn, rr, rg = AL.reference(vals, mk, act, T, g)
            LU.check_stats(aux[..., 0], aux[..., 1], rl, rn, what)
            LU.check_grad(grad, rg, T, code, what)
            haux, hrefused, _hgrad = AL.from_rows(vals, mk, act, T, g)
            for k, (name, _l, m_, _a, want_refused) in enumerate(rows):
                assert tuple(np.nonzero(rr[k])[0]) == want_refused and hrefused[k] == len(want_refused), (what, name)
                assert tuple(np.nonzero(np.isnan(aux[k, :, 2]))[0]) == want_refused, (what, name)
                for b in want_refused:
                    assert not aux[k, b, [0, 1, 3]].any() and not grad[k, SEG[b]:SEG[b + 1]].any(), (what, name)
                assert not grad[k][~m_].any(), (what, name)
                if want_refused:                 # the other four agents: bit for bit what the row without the cause gives (row 0 of the batch)
                    for b in (b for b in range(5) if b not in want_refused):
                        assert np.array_equal(aux[k, b], aux[0, b]) and np.array_equal(grad[k, SEG[b]:SEG[b + 1]], grad[0, SEG[b]:SEG[b + 1]]), (what, name)
            by_name = {r[0]: k for k, r in enumerate(rows)}
            k = by_name['only the Sleep slot valid']
            assert not aux[k, :, :2].any() and not grad[k].any()
            k = by_name['the action on a valid -inf slot']
            assert np.isneginf(aux[k, :, 0]).all() and np.isfinite(grad[k]).all()
            k = by_name['every action -1']
            assert not aux[k].any() and not grad[k].any()
            # the rows without a refusal alone: no fault
            aux2, grad2, fault2 = _run(dev_arr[clean], code, mk[clean], act[clean], T, g[clean])
            assert fault2 == 0 and np.array_equal(aux2, aux[clean], equal_nan=True) and np.array_equal(grad2, grad[clean]), what


def test_no_rows_and_the_refusals_enqueue_nothing(masks):
    lib = _lib()
    n = 3
    rng = np.random.default_rng(9)
    lg = U.random_logits(rng, (n, 570))
    d_lg, d_mk, d_ac, d_g = DevMem(lg.nbytes), DevMem(n * 570), DevMem(n * 20), DevMem(n * 40)
    d_lg.up(lg)
    d_mk.up(masks[:n].astype(np.uint8))
    d_ac.up(np.tile(np.array(U.SLEEP, np.int32), (n, 1)))
    d_aux, d_grad, d_fault = DevMem(n * 80, 0xC3), DevMem(lg.nbytes, 0xC3), DevMem(4, 0xC3)
    assert d_lg.hip.hipDeviceSynchronize() == 0
    f = ctypes.c_float

    def fwd(n_=n, dt=3, T=1.0, lg_=d_lg.p, mk=d_mk.p, ac=d_ac.p, aux=d_aux.p, fault=d_fault.p):
        return lib.cc4_logp_actions_device(None, lg_, dt, mk, ac, n_, f(T), aux, fault)

    def bwd(n_=n, dt=3, T=1.0, lg_=d_lg.p, mk=d_mk.p, ac=d_ac.p, aux=d_aux.p, g=d_g.p, grad=d_grad.p):
        return lib.cc4_logp_actions_grad_device(None, lg_, dt, mk, ac, n_, f(T), aux, g, grad)
    bad = [dict(n_=-1), dict(dt=0), dict(dt=4), dict(T=0.0), dict(T=-1.0), dict(T=float('nan')), dict(T=float('inf')), dict(lg_=None), dict(mk=None),
           dict(ac=None), dict(aux=None)]
    for kw in bad + [dict(fault=None)]:
        assert fwd(**kw) == -2, kw
    for kw in bad + [dict(g=None), dict(grad=None)]:
        assert bwd(**kw) == -2, kw
    assert fwd(n_=0) == 0 and bwd(n_=0) == 0
    assert d_lg.hip.hipDeviceSynchronize() == 0
    for m in (d_aux, d_grad, d_fault):
        assert (m.down(np.uint8, m.nbytes) == 0xC3).all()
    for m in (d_lg, d_mk, d_ac, d_g, d_aux, d_grad, d_fault):
        m.free()
