"""CPU: advantages and returns of a stored rollout -- the surface (header, exports, bindings, constants, the kernel's resource row); the host
function (advantages.from_arrays: cc4_gae_host, float32) against the float64 restatement (advantages.reference: episode segments and explicit
sums, no backward recurrence) under the rounding bound of gae_util, for both layouts, bootstrap on and off, rewards shared and per head, with and
without actions; exact checks on crafted columns; every -2 of the two entry points' argument checks; and the ValueErrors of advantages.gae that
need no device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
import gae_util as G
from cage_challenge_4_amd import advantages as AD

VP = ctypes.c_void_p
LAYOUTS = [(True, False), (True, True), (False, False)]          # (autoreset, bootstrap)


def _lib():
    from cage_challenge_4_amd import _lib
    return _lib.load()


def test_surface_header_exports_bindings_constants_and_resources():
    from cage_challenge_4_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym, nargs in (('cc4_gae_device', 18), ('cc4_gae_host', 16), ('cc4_gae_rows', 0)):
        assert re.search(r'\bint(32_t)?\s+' + sym + r'\s*\(', code), sym
        assert hasattr(lib, sym), sym
        assert len(_lib.SIGNATURES[sym][1]) == nargs, sym
    assert re.search(r'#define CC4_GAE_SKIP_AFTER_DONE\s+1\n', txt) and re.search(r'#define CC4_GAE_BOOTSTRAP_DONE\s+2\n', txt)
    assert (_lib.GAE_SKIP_AFTER_DONE, _lib.GAE_BOOTSTRAP_DONE, _lib.GAE_MAX_HEADS) == (1, 2, 8) == (AD.SKIP_AFTER_DONE, AD.BOOTSTRAP_DONE, AD.MAX_HEADS)
    assert 1 <= _lib.load().cc4_gae_rows() <= 32
    k_src = open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'cc4_k_gae.hip')).read()
    assert 'fmaf' not in re.sub(r'//.*', '', k_src + open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'cc4_gae.h')).read())
    assert '-ffp-contract=off' in open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'Makefile')).read()
    rows = [ln for ln in open(os.path.join(ROOT, 'profiles', 'kernel_resources.txt')) if ln.rstrip().endswith('cc4_k_gae.hip')]
    assert len(rows) == 1 and 'k_gae' in rows[0]
    assert re.search(r'scratch\s+0\s+vgpr_spill\s+0\s', rows[0]) and re.search(r'lds_static\s+0\s', rows[0]), rows[0]


def test_importing_the_module_imports_neither_torch_nor_the_library():
    import subprocess
    code = ("import sys; import cage_challenge_4_amd.advantages as A, cage_challenge_4_amd._lib as L; "
            "assert 'torch' not in sys.modules and L._lib is None; print('ok')")
    pr = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert pr.returncode == 0 and pr.stdout.strip() == 'ok', pr.stderr


@pytest.fixture(scope='module')
def rollouts():
    """(T, N, A, heads) -> rollout: T = 1, a prime, more rows than columns, a long one at a low done rate."""
    rng = np.random.default_rng(31)
    out = {}
    for T, N, A, heads, rate in ((1, 5, 1, 1, 0.3), (17, 13, 5, 1, 0.15), (17, 13, 5, 5, 0.15), (65, 7, 8, 8, 0.1), (500, 4, 2, 1, 0.02), (500, 3, 1, 1, 0.0)):
        ro = G.random_rollout(rng, T, N, A, done_rate=rate, heads=heads)
        out[(T, N, A, heads)] = G.force_events(rng, ro) if rate else ro
    return out


@pytest.mark.parametrize('autoreset,bootstrap', LAYOUTS)
def test_host_function_against_the_restatement_under_the_bound(rollouts, autoreset, bootstrap):
    worst = 0.0
    for (T, N, A, heads), ro in rollouts.items():
        for gamma, lam in ((0.9, 0.5), (0.99, 0.95), (1.0, 1.0)):
            for with_actions in (False, True):
                for with_done0 in (False, True):
                    kw = dict(gamma=gamma, lam=lam, done0=ro['done0'] if with_done0 else None, autoreset=autoreset, bootstrap=bootstrap)
                    act = ro['actions'] if with_actions else None
                    adv, ret, w = AD.from_arrays(ro['rewards'], ro['values'], ro['last_value'], ro['dones'], actions=act, **kw)
                    ref = AD.reference(ro['rewards'], ro['values'], ro['last_value'], ro['dones'], actions=act, **kw)
                    assert adv.shape == ret.shape == w.shape == (T, N, A) and adv.dtype == ret.dtype == np.float32 and w.dtype == np.bool_
                    what = f'T {T} N {N} A {A} heads {heads} autoreset {autoreset} bootstrap {bootstrap} gamma {gamma} lam {lam}'
                    worst = max(worst, G.check(adv, ret, ro, gamma, lam, autoreset, bootstrap, what, ref=ref, use_done0=with_done0))
                    assert np.array_equal(w, ref[2]), what
                    prev = np.concatenate(((ro['done0'] if with_done0 else np.zeros(N, np.uint8))[None], ro['dones'][:-1])) != 0
                    skip = np.broadcast_to((prev & autoreset)[..., None], (T, N, A))
                    assert np.array_equal(w, ~skip & ((ro['actions'] != -1) | (not with_actions))), what
                    assert not adv[skip].any() and np.array_equal(ret[skip], ro['values'][skip]), what
    assert 0.0 < worst < 1.0
    print(f'host function against the restatement: worst |err| / E {worst:.3g}')


def test_no_rows_and_no_episodes_give_empty_outputs():
    for T, N, A in ((0, 3, 2), (4, 0, 2)):
        z = np.zeros
        for fn in (AD.from_arrays, AD.reference):
            a, r, w = fn(z((T, N), np.float32), z((T, N, A), np.float32), z((N, A), np.float32), z((T, N), np.uint8), gamma=0.9, lam=0.9,
                         done0=z(N, np.uint8), actions=z((T, N, A), np.int32))
            assert a.shape == r.shape == w.shape == (T, N, A) and w.dtype == np.bool_


def _col(r, v, last, d, done0=0, act=None, **kw):
    """One column (N = 1, A = 1) through the host function: (adv [T], ret [T], weight [T])."""
    T = len(v)
    a, rt, w = AD.from_arrays(np.asarray(r, np.float32).reshape(T, 1), np.asarray(v, np.float32).reshape(T, 1), np.asarray([last], np.float32),
                              np.asarray(d, np.uint8).reshape(T, 1), done0=np.asarray([done0], np.uint8),
                              actions=None if act is None else np.asarray(act, np.int32).reshape(T, 1), **kw)
    return a[:, 0], rt[:, 0], w[:, 0]


F = np.float32
R6, V6 = [-1, -2, -3, -4, -5, -6], [10, 20, 30, 40, 50, 60]


def _plain(r, v, after, gamma, lam):
    """One episode segment whose last row bootstraps from `after`, in float32 in the definition's order of operations."""
    g, gl = F(gamma), F(gamma) * F(lam)
    adv, a_next, v_next = [F(0)] * len(r), F(0), F(after)
    for t in range(len(r) - 1, -1, -1):
        adv[t] = ((F(r[t]) + g * v_next) - F(v[t])) + gl * a_next
        a_next, v_next = adv[t], F(v[t])
    return np.array(adv, F)


def test_crafted_done0_makes_row_0_a_skip_row():
    a, rt, w = _col(R6, V6, 70, [0] * 6, done0=1, gamma=0.9, lam=0.8, autoreset=True)
    assert a[0] == 0 and rt[0] == 10 and not w[0] and w[1:].all()
    assert np.array_equal(a[1:], _plain(R6[1:], V6[1:], 70, 0.9, 0.8))
    # ... and changes nothing in the plain layout
    a2, _r2, w2 = _col(R6, V6, 70, [0] * 6, done0=1, gamma=0.9, lam=0.8, autoreset=False)
    assert np.array_equal(a2, _plain(R6, V6, 70, 0.9, 0.8)) and w2.all()


def test_crafted_done_at_T_minus_2_and_at_T_minus_1_and_bootstrap():
    # done at T-2: the last row is a skip row; the done row bootstraps from that row's value with bootstrap, from 0 without; `last` is unused
    for boot in (False, True):
        a, rt, w = _col(R6, V6, 70, [0, 0, 0, 0, 1, 0], gamma=0.9, lam=0.8, autoreset=True, bootstrap=boot)
        assert a[5] == 0 and rt[5] == 60 and not w[5] and w[:5].all()
        assert np.array_equal(a[:5], _plain(R6[:5], V6[:5], 60 if boot else 0, 0.9, 0.8))
        b, _rt, _w = _col(R6, V6, -1234, [0, 0, 0, 0, 1, 0], gamma=0.9, lam=0.8, autoreset=True, bootstrap=boot)
        assert np.array_equal(a, b)
    # done at T-1: `last` is used only with bootstrap
    plain = _col(R6, V6, 70, [0, 0, 0, 0, 0, 1], gamma=0.9, lam=0.8, autoreset=True)[0]
    assert np.array_equal(plain, _plain(R6, V6, 0, 0.9, 0.8))
    assert np.array_equal(plain, _col(R6, V6, -5, [0, 0, 0, 0, 0, 1], gamma=0.9, lam=0.8, autoreset=True)[0])
    assert np.array_equal(plain, _col(R6, V6, 70, [0, 0, 0, 0, 0, 1], gamma=0.9, lam=0.8, autoreset=False)[0])
    boot = _col(R6, V6, 70, [0, 0, 0, 0, 0, 1], gamma=0.9, lam=0.8, autoreset=True, bootstrap=True)[0]
    assert np.array_equal(boot, _plain(R6, V6, 70, 0.9, 0.8)) and not np.array_equal(boot, plain)


def test_crafted_two_stored_dones_in_a_row_no_done_and_one_row():
    # rows 1 and 2 carry a done: rows 2 and 3 are skip rows (the byte of a skip row is taken as stored)
    a, rt, w = _col(R6, V6, 70, [0, 1, 1, 0, 0, 0], gamma=0.9, lam=0.8, autoreset=True, bootstrap=True)
    assert list(w) == [True, True, False, False, True, True]
    assert not a[2:4].any() and list(rt[2:4]) == [30, 40]
    assert np.array_equal(a[:2], _plain(R6[:2], V6[:2], 30, 0.9, 0.8)) and np.array_equal(a[4:], _plain(R6[4:], V6[4:], 70, 0.9, 0.8))
    # no done at all: one segment in either layout
    for ar in (True, False):
        assert np.array_equal(_col(R6, V6, 70, [0] * 6, gamma=0.99, lam=0.95, autoreset=ar)[0], _plain(R6, V6, 70, 0.99, 0.95))
    # T = 1
    a, rt, w = _col([-3], [5], 7, [0], gamma=0.5, lam=0.5, autoreset=True)
    assert a[0] == F(-3) + F(0.5) * F(7) - F(5) and rt[0] == a[0] + F(5) and w[0]
    a, rt, w = _col([-3], [5], 7, [0], done0=1, gamma=0.5, lam=0.5, autoreset=True)
    assert a[0] == 0 and rt[0] == 5 and not w[0]
    a, rt, w = _col([-3], [5], 7, [1], gamma=0.5, lam=0.5, autoreset=True)
    assert a[0] == -8 and rt[0] == -3 and w[0]


def test_crafted_gamma_0_lam_0_and_reward_to_go():
    d = [0, 0, 1, 0, 0, 0]
    a = _col(R6, V6, 70, d, gamma=0.0, lam=0.7, autoreset=False)[0]
    assert np.array_equal(a, np.array(R6, F) - np.array(V6, F))                     # gamma = 0: adv = r - v
    a = _col(R6, V6, 70, d, gamma=0.9, lam=0.0, autoreset=False)[0]
    nxt = np.array([20, 30, 0, 50, 60, 70], F)
    assert np.array_equal(a, (np.array(R6, F) + F(0.9) * nxt) - np.array(V6, F))     # lam = 0: adv = delta
    # gamma = lam = 1 with zero values: ret is the reward-to-go of the segment; the autoreset layout's skip row (row 3) carries reward 0
    _a, rt, _w = _col(R6, [0] * 6, 0, d, gamma=1.0, lam=1.0, autoreset=False)
    assert list(rt) == [-6, -5, -3, -15, -11, -6]
    _a, rt, w = _col([-1, -2, -3, 0, -5, -6], [0] * 6, 0, d, gamma=1.0, lam=1.0, autoreset=True)
    assert list(rt) == [-6, -5, -3, 0, -11, -6] and list(w) == [True, True, True, False, True, True]


def test_crafted_a_skip_rows_reward_and_action_change_nothing_elsewhere_and_the_weights():
    d = [0, 0, 1, 0, 0, 0]
    act = [3, -1, 4, 7, -1, 0]
    base = _col(R6, V6, 70, d, act=act, gamma=0.9, lam=0.8, autoreset=True)
    r2, act2 = list(R6), list(act)
    r2[3], act2[3] = -1000, -1
    other = _col(r2, V6, 70, d, act=act2, gamma=0.9, lam=0.8, autoreset=True)
    for x, y in zip(base, other):
        assert np.array_equal(x, y)
    a, rt, w = base
    assert a[3] == 0 and rt[3] == 40 and not w[3]
    assert list(w) == [True, False, True, False, False, True]                       # 0 exactly on the skip row and the -1 actions
    assert list(_col(R6, V6, 70, d, act=act, gamma=0.9, lam=0.8, autoreset=False)[2]) == [True, False, True, True, False, True]
    assert _col(R6, V6, 70, d, gamma=0.9, lam=0.8, autoreset=False)[2].all()
    # the -1 changes only the weight
    assert np.array_equal(a, _col(R6, V6, 70, d, gamma=0.9, lam=0.8, autoreset=True)[0])


@pytest.mark.parametrize('autoreset,bootstrap', LAYOUTS)
def test_crafted_a_nan_value_shows_only_in_its_own_episode_segment(autoreset, bootstrap):
    d = [0, 0, 1, 0, 0, 0, 0, 1, 0, 0]
    r = [-1] * 10
    v = [float(k) for k in range(10)]
    clean = _col(r, v, 11, d, gamma=0.9, lam=0.8, autoreset=autoreset, bootstrap=bootstrap)
    v[5] = float('nan')                 # the segment of rows 4 .. 7 (3 is its skip row in the autoreset layout)
    a, rt, w = _col(r, v, 11, d, gamma=0.9, lam=0.8, autoreset=autoreset, bootstrap=bootstrap)
    seg_lo = 4 if autoreset else 3
    assert np.isnan(a[seg_lo:6]).all() and np.isnan(rt[seg_lo:6]).all()
    rest = [t for t in range(10) if not seg_lo <= t <= 5]
    assert np.array_equal(a[rest], clean[0][rest]) and np.array_equal(rt[rest], clean[1][rest]) and np.array_equal(w, clean[2])
    ref = AD.reference(np.array(r, F).reshape(10, 1), np.array(v, F).reshape(10, 1), np.array([11], F), np.array(d, np.uint8).reshape(10, 1),
                       gamma=0.9, lam=0.8, autoreset=autoreset, bootstrap=bootstrap)
    assert np.array_equal(np.isnan(ref[0][:, 0]), np.isnan(a))


def test_the_restatement_on_a_column_worked_by_hand():
    """advantages.reference without the code under test: T = 4, gamma = 0.5, lam = 0.5 (exact in binary), a done on row 1."""
    r, v, d = [1.0, 2.0, 0.0, 4.0], [8.0, 4.0, 2.0, 6.0], [0, 1, 0, 0]
    kw = dict(gamma=0.5, lam=0.5)
    arr = lambda x, dt=np.float64: np.array(x, dt).reshape(4, 1)      # noqa: E731
    # autoreset, no bootstrap: segments {0, 1} (ends in 0) and {3} (ends in last = 10); row 2 is a skip row
    adv, ret, w = AD.reference(arr(r), arr(v), np.array([10.0]), arr(d, np.uint8), autoreset=True, **kw)
    d1 = 2.0 + 0.0 - 4.0
    d0 = 1.0 + 0.5 * 4.0 - 8.0
    assert list(adv[:, 0]) == [d0 + 0.25 * d1, d1, 0.0, 4.0 + 5.0 - 6.0] and list(ret[:, 0]) == [d0 + 0.25 * d1 + 8.0, d1 + 4.0, 2.0, 9.0]
    assert list(w[:, 0]) == [True, True, False, True]
    # bootstrap: row 1 ends on the skip row's value
    adv, _ret, _w = AD.reference(arr(r), arr(v), np.array([10.0]), arr(d, np.uint8), autoreset=True, bootstrap=True, **kw)
    assert list(adv[:, 0]) == [d0 + 0.25 * (d1 + 1.0), d1 + 1.0, 0.0, 3.0]
    # plain: segments {0, 1} and {2, 3}
    adv, _ret, w = AD.reference(arr(r), arr(v), np.array([10.0]), arr(d, np.uint8), autoreset=False, **kw)
    d3, d2 = 4.0 + 5.0 - 6.0, 0.0 + 3.0 - 2.0
    assert list(adv[:, 0]) == [d0 + 0.25 * d1, d1, d2 + 0.25 * d3, d3] and w.all()


def test_every_refusal_of_the_entry_points():
    """-2 from cc4_gae_host for every case of the ABI, and from cc4_gae_device for the same cases plus the dtype: the device call checks before it
    touches the runtime, so the plain host pointers it is given here are never used."""
    lib = _lib()
    T, N, A = 3, 2, 2
    f = lambda *s: np.zeros(s, np.float32)      # noqa: E731
    arrs = dict(r=f(T, N), v=f(T, N, A), last=f(N, A), d=np.zeros((T, N), np.uint8), d0=np.zeros(N, np.uint8), act=np.zeros((T, N, A), np.int32),
                adv=f(T, N, A) + 7, ret=f(T, N, A) + 7, w=np.zeros((T, N, A), np.uint8) + 7)
    P = {k: x.ctypes.data_as(VP) for k, x in arrs.items()}

    def host(heads=1, T_=T, N_=N, A_=A, gamma=0.9, lam=0.9, flags=1, **over):
        p = dict(P, **over)
        return lib.cc4_gae_host(p['r'], heads, p['v'], p['last'], p['d'], p['d0'], p['act'], T_, N_, A_, gamma, lam, flags, p['adv'], p['ret'], p['w'])

    def device(heads=1, dtype=3, T_=T, N_=N, A_=A, gamma=0.9, lam=0.9, flags=1, **over):
        p = dict(P, **over)
        return lib.cc4_gae_device(None, p['r'], heads, p['v'], dtype, p['last'], p['d'], p['d0'], p['act'], T_, N_, A_, gamma, lam, flags, p['adv'],
                                  p['ret'], p['w'])
    nan = float('nan')
    bad = [dict(r=None), dict(v=None), dict(last=None), dict(d=None), dict(adv=None), dict(ret=None), dict(T_=-1), dict(N_=-1), dict(A_=0), dict(A_=9),
           dict(A_=-1), dict(heads=0), dict(heads=3), dict(heads=A + 1), dict(gamma=-0.01), dict(gamma=1.01), dict(gamma=nan), dict(lam=-0.01),
           dict(lam=1.01), dict(lam=nan), dict(flags=4), dict(flags=-1), dict(flags=2), dict(flags=8 | 1), dict(N_=2 ** 30, A_=2), dict(N_=2 ** 31 - 1, A_=8)]
    for kw in bad:
        assert host(**kw) == -2, kw
        assert device(**kw) == -2, kw
    for kw in (dict(dtype=0), dict(dtype=4), dict(dtype=-1)):
        assert device(**kw) == -2, kw
    for x in ('adv', 'ret', 'w'):
        assert (arrs[x] == 7).all()
    # what is allowed: the optional pointers, both ends of the ranges, reward_heads = A, and no rows or no episodes
    assert host(d0=None, act=None, w=None) == 0 and host(gamma=0.0, lam=1.0) == 0 and host(gamma=1.0, lam=0.0, flags=3) == 0 and host(flags=0) == 0
    assert host(heads=A, r=arrs['v'].ctypes.data_as(VP)) == 0 and host(A_=1, heads=1) == 0
    before = arrs['adv'].copy()
    assert host(T_=0) == 0 and host(N_=0) == 0 and np.array_equal(arrs['adv'], before)
    assert device(T_=0) == 0 and device(N_=0) == 0


def test_value_errors_of_gae_that_need_no_device():
    torch = pytest.importorskip('torch')
    T, N, A = 4, 3, 5
    ok = dict(rewards=torch.zeros(T, N), values=torch.zeros(T, N, A), last_value=torch.zeros(N, A), dones=torch.zeros(T, N, dtype=torch.bool))
    before = dict(AD.launches)

    def call(gamma=0.9, lam=0.9, **kw):
        a = dict(ok, **{k: v for k, v in kw.items() if k in ok})
        rest = {k: v for k, v in kw.items() if k not in ok}
        return AD.gae(a['rewards'], a['values'], a['last_value'], a['dones'], gamma=gamma, lam=lam, **rest)
    for kw, match in ((dict(gamma=-0.1), 'gamma'), (dict(gamma=1.5), 'gamma'), (dict(gamma=float('nan')), 'gamma'), (dict(gamma='x'), 'gamma'),
                      (dict(gamma=None), 'gamma'), (dict(lam=-0.1), 'lam'), (dict(lam=2), 'lam'), (dict(lam=float('nan')), 'lam'),
                      (dict(autoreset=False, bootstrap=True), 'bootstrap'),
                      (dict(values=np.zeros((T, N, A), np.float32)), 'values must be a torch tensor'), (dict(rewards=None), 'rewards must be a torch tensor'),
                      (dict(values=torch.zeros(T)), 'values must have shape'), (dict(values=torch.zeros(T, N, 9), last_value=torch.zeros(N, 9)), 'values must have shape'),
                      (dict(values=torch.zeros(T, N, A, 1)), 'values must have shape'),
                      (dict(rewards=torch.zeros(T, N + 1)), 'rewards must have shape'), (dict(rewards=torch.zeros(T, N, 1)), 'rewards must have shape'),
                      (dict(last_value=torch.zeros(N)), 'last_value must have shape'), (dict(dones=torch.zeros(T, N, A, dtype=torch.bool)), 'dones must have shape'),
                      (dict(done0=torch.zeros(N + 1, dtype=torch.bool)), 'done0 must have shape'), (dict(actions=torch.zeros(T, N, dtype=torch.int32)), 'actions must have shape'),
                      (dict(values=torch.zeros(T, N, A, dtype=torch.float64), last_value=torch.zeros(N, A, dtype=torch.float64)), 'values must be float16'),
                      (dict(last_value=torch.zeros(N, A, dtype=torch.bfloat16)), 'last_value must have the dtype'),
                      (dict(rewards=torch.zeros(T, N, dtype=torch.float64)), 'rewards must be float32'), (dict(dones=torch.zeros(T, N)), 'dones must be bool or uint8'),
                      (dict(done0=torch.zeros(N, dtype=torch.int32)), 'done0 must be bool or uint8'),
                      (dict(actions=torch.zeros(T, N, A, dtype=torch.int64)), 'actions must be int32'),
                      (dict(out=(torch.zeros(T, N, A),)), 'out must be'), (dict(out=(torch.zeros(T, N, A), torch.zeros(T, N, A), torch.zeros(T, N, A))), 'out: weight'),
                      (dict(out=(torch.zeros(T, N), torch.zeros(T, N, A), torch.zeros(T, N, A, dtype=torch.bool))), 'out: adv'),
                      (dict(), 'rewards must be a contiguous CUDA tensor')):           # (everything else right: CPU tensors are refused last)
        with pytest.raises(ValueError, match=match):
            call(**kw)
    assert AD.launches == before
    # from_arrays and reference refuse the same parameters and shapes
    z = {k: v.numpy() for k, v in ok.items()}
    for fn in (AD.from_arrays, AD.reference):
        with pytest.raises(ValueError, match='gamma'):
            fn(z['rewards'], z['values'], z['last_value'], z['dones'], gamma=1.1, lam=0.5)
        with pytest.raises(ValueError, match='bootstrap'):
            fn(z['rewards'], z['values'], z['last_value'], z['dones'], gamma=0.9, lam=0.5, autoreset=False, bootstrap=True)
        with pytest.raises(ValueError, match='dones must have shape'):
            fn(z['rewards'], z['values'], z['last_value'], z['dones'][:-1], gamma=0.9, lam=0.5)
        with pytest.raises(ValueError, match='actions must be integers'):
            fn(z['rewards'], z['values'], z['last_value'], z['dones'], gamma=0.9, lam=0.5, actions=z['values'])
