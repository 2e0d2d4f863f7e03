"""GPU: advantages and returns of a stored rollout on the device.  cc4_gae_device (k_gae) is bit-equal to cc4_gae_host in all three outputs for
float32 values, and for bfloat16 and float16 values bit-equal to the host function fed the exactly upcast values: the library is built without
contraction, and the kernel and the host function are one statement (csrc/cc4_gae.h).  The shapes are the smallest at which the block loop, its
short block and the lane mapping can go wrong: T in {1, R-1, R, R+1, 2R+3} with R = cc4_gae_rows(), the rows the kernel of this build loads
ahead, and (N, A) a single column, exactly one wave, a wave and one lane, two heads, the largest A, several waves; per shape both layouts (and
the bootstrap), rewards shared and per head, done0 / actions / d_weight present and NULL.  Every output sits inside a larger allocation filled
with a sentinel: nothing outside its T * N * A elements is written.  A call on a side stream; T == 0, N == 0 and the refusals enqueue nothing.
The calls take plain device pointers: no env, and torch only for the stream test."""
import ctypes

import numpy as np
import pytest

import gae_util as G
from view_util import DevMem

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p
SHAPES = [(1, 1), (64, 1), (13, 5), (33, 2), (7, 8), (65, 5)]          # (N, A)
GUARD, FILL = 64, 0xA5                                                   # bytes in front of and behind every output, and what they hold
ITEM = {3: 4, 2: 2, 1: 2}


def _lib():
    from cage_challenge_4_amd import _lib
    return _lib.load()


def _rows():
    R = _lib().cc4_gae_rows()
    return sorted({1, max(R - 1, 1), R, R + 1, 2 * R + 3})


@pytest.fixture(scope='module')
def rollouts():
    """(T, N, A) -> a rollout with rewards per head (the shared form takes head 0), with at least one done, one skip row and one -1: asserted
    here, so that an empty case cannot pass silently."""
    rng = np.random.default_rng(3131)
    out = {}
    for T in _rows():
        for N, A in SHAPES:
            ro = G.force_events(rng, G.random_rollout(rng, T, N, A, done_rate=0.25, heads=A))
            dones, skips, nones = G.counts(ro)
            assert dones >= 1 and skips >= 1 and nones >= 1, (T, N, A, dones, skips, nones)
            out[(T, N, A)] = ro
    return out


def _device_values(values, code):
    """(what goes to the device, the float32 values it carries)."""
    if code == 3:
        return values, values
    if code == 2:
        bits = G.to_bf16_bits(values)
        return bits, G.upcast(bits)
    h = values.astype(np.float16)
    return h, h.astype(np.float32)


class Guarded:
    """An output of nbytes inside an allocation with GUARD sentinel bytes on either side (the output itself starts as the sentinel too)."""

    def __init__(self, nbytes):
        self.n, self.mem = nbytes, DevMem(nbytes + 2 * GUARD, FILL)

    @property
    def p(self):
        return self.mem.at(GUARD)

    def down(self, dtype, shape):
        raw = self.mem.down(np.uint8, self.n + 2 * GUARD)
        assert (raw[:GUARD] == FILL).all() and (raw[GUARD + self.n:] == FILL).all(), 'bytes outside the output were written'
        return raw[GUARD:GUARD + self.n].copy().view(dtype).reshape(shape)


def _run(ro, code, heads, gamma, lam, flags, with_done0=True, with_actions=True, with_weight=True, stream=None):
    """cc4_gae_device on a rollout: (adv, ret, weight or None) and the float32 values the device saw."""
    lib = _lib()
    T, N, A = ro['values'].shape
    dv, vals = _device_values(ro['values'], code)
    dl, last = _device_values(ro['last_value'], code)
    rw = ro['rewards'] if heads == A else np.ascontiguousarray(ro['rewards'][..., 0])
    ins = [DevMem(x.nbytes) for x in (rw, dv, dl, ro['dones'], ro['done0'], ro['actions'])]
    for m, x in zip(ins, (rw, dv, dl, ro['dones'], ro['done0'], ro['actions'])):
        m.up(x)
    adv, ret, w = Guarded(T * N * A * 4), Guarded(T * N * A * 4), Guarded(T * N * A)
    assert ins[0].hip.hipDeviceSynchronize() == 0
    rc = lib.cc4_gae_device(stream, ins[0].p, heads, ins[1].p, code, ins[2].p, ins[3].p, ins[4].p if with_done0 else None,
                            ins[5].p if with_actions else None, T, N, A, gamma, lam, flags, adv.p, ret.p, w.p if with_weight else None)
    assert rc == 0
    assert ins[0].hip.hipDeviceSynchronize() == 0
    out = adv.down(np.float32, (T, N, A)), ret.down(np.float32, (T, N, A)), w.down(np.uint8, (T, N, A))
    if not with_weight:
        assert (out[2] == FILL).all(), 'a NULL d_weight was written somewhere'
    for m in ins + [adv.mem, ret.mem, w.mem]:
        m.free()
    return out, vals, last, rw


def _host(ro, vals, last, rw, heads, gamma, lam, flags, with_done0=True, with_actions=True):
    lib = _lib()
    T, N, A = vals.shape
    adv, ret, w = np.zeros((T, N, A), np.float32), np.zeros((T, N, A), np.float32), np.zeros((T, N, A), np.uint8)
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(VP)      # noqa: E731
    vals, last, rw = (np.ascontiguousarray(x, np.float32) for x in (vals, last, rw))
    rc = lib.cc4_gae_host(p(rw), heads, p(vals), p(last), p(ro['dones']), p(ro['done0']) if with_done0 else None,
                          p(ro['actions']) if with_actions else None, T, N, A, gamma, lam, flags, p(adv), p(ret), p(w))
    assert rc == 0
    return adv, ret, w


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('N,A', SHAPES)
def test_device_is_bit_equal_to_the_host_function(rollouts, N, A):
    cases = 0
    for T in _rows():
        ro = rollouts[(T, N, A)]
        for code in (3, 2, 1):
            for flags in (1, 3, 0):
                for heads in sorted({1, A}):
                    # the three optional pointers: all present, all NULL, and one at a time on the float32 pass
                    opts = [(True, True, True), (False, False, False)]
                    if code == 3:
                        opts += [(False, True, True), (True, False, True), (True, True, False)]
                    for d0, act, wt in opts:
                        gamma, lam = (0.99, 0.95) if flags != 0 else (1.0, 0.9)
                        what = f'T {T} N {N} A {A} dtype {code} flags {flags} heads {heads} done0 {d0} actions {act} weight {wt}'
                        (adv, ret, w), vals, last, rw = _run(ro, code, heads, gamma, lam, flags, d0, act, wt)
                        hadv, hret, hw = _host(ro, vals, last, rw, heads, gamma, lam, flags, d0, act)
                        assert _same_bits(adv, hadv), what
                        assert _same_bits(ret, hret), what
                        if wt:
                            assert np.array_equal(w, hw) and set(np.unique(w)) <= {0, 1}, what
                        cases += 1
    print(f'N {N} A {A}: {cases} calls bit-equal to the host function, T in {_rows()}')


def test_device_against_the_restatement_under_the_bound(rollouts):
    """The kernel's numbers are the definition's: one shape, the three dtypes, against advantages.reference on the values the dtype carries."""
    T = _rows()[-1]
    ro = rollouts[(T, 65, 5)]
    for code in (3, 2, 1):
        for autoreset, bootstrap in ((True, False), (True, True), (False, False)):
            flags = (1 if autoreset else 0) | (2 if bootstrap else 0)
            (adv, ret, _w), vals, last, _rw = _run(ro, code, 5, 0.99, 0.95, flags)
            seen = dict(ro, values=vals, last_value=last)
            G.check(adv, ret, seen, 0.99, 0.95, autoreset, bootstrap, f'dtype {code} autoreset {autoreset} bootstrap {bootstrap}')


def test_a_call_on_a_side_stream_ordered_against_the_default_stream():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.skip('torch sees no device')
    lib = _lib()
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(77)
    T, N, A = 2 * lib.cc4_gae_rows() + 3, 65, 5
    ro = G.force_events(rng, G.random_rollout(rng, T, N, A, done_rate=0.2))
    side = torch.cuda.Stream(dev)
    # the inputs are written on the default stream (a scale by 2 of what was uploaded), the kernel runs on the side stream behind them, and the
    # default stream reads the outputs behind the kernel
    t = {k: torch.from_numpy(v).to(dev) for k, v in ro.items()}
    values = t['values'] * 2.0
    adv, ret = torch.full((T, N, A), 7.0, device=dev), torch.full((T, N, A), 7.0, device=dev)
    w = torch.full((T, N, A), 7, dtype=torch.uint8, device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    p = lambda x: VP(x.data_ptr())      # noqa: E731
    rc = lib.cc4_gae_device(VP(side.cuda_stream), p(t['rewards']), 1, p(values), 3, p(t['last_value']), p(t['dones']), p(t['done0']), p(t['actions']),
                            T, N, A, 0.99, 0.95, 3, p(adv), p(ret), p(w))
    assert rc == 0
    torch.cuda.current_stream(dev).wait_stream(side)
    got = (adv + 0.0).cpu().numpy(), (ret + 0.0).cpu().numpy(), w.clone().cpu().numpy()
    hadv, hret, hw = _host(ro, ro['values'] * np.float32(2.0), ro['last_value'], ro['rewards'], 1, 0.99, 0.95, 3)
    assert _same_bits(got[0], hadv) and _same_bits(got[1], hret) and np.array_equal(got[2], hw)


def test_no_rows_no_episodes_and_the_refusals_enqueue_nothing():
    lib = _lib()
    rng = np.random.default_rng(5)
    T, N, A = 5, 3, 2
    ro = G.random_rollout(rng, T, N, A)
    ins = {k: DevMem(v.nbytes) for k, v in ro.items()}
    for k, v in ro.items():
        ins[k].up(v)
    outs = [DevMem(T * N * A * 4, 0xC3), DevMem(T * N * A * 4, 0xC3), DevMem(T * N * A, 0xC3)]
    assert outs[0].hip.hipDeviceSynchronize() == 0

    def call(heads=1, dtype=3, T_=T, N_=N, A_=A, gamma=0.9, lam=0.9, flags=1, **over):
        p = dict({k: m.p for k, m in ins.items()}, adv=outs[0].p, ret=outs[1].p, w=outs[2].p)
        p.update(over)
        return lib.cc4_gae_device(None, p['rewards'], heads, p['values'], dtype, p['last_value'], p['dones'], p['done0'], p['actions'], T_, N_, A_,
                                  gamma, lam, flags, p['adv'], p['ret'], p['w'])
    nan = float('nan')
    for kw in (dict(rewards=None), dict(values=None), dict(last_value=None), dict(dones=None), dict(adv=None), dict(ret=None), dict(dtype=0), dict(dtype=4),
               dict(T_=-1), dict(N_=-1), dict(A_=0), dict(A_=9), dict(heads=0), dict(heads=A + 1), dict(gamma=-0.5), dict(gamma=1.5), dict(gamma=nan),
               dict(lam=-0.5), dict(lam=1.5), dict(lam=nan), dict(flags=4), dict(flags=2), dict(N_=2 ** 30, A_=2)):
        assert call(**kw) == -2, kw
    assert call(T_=0) == 0 and call(N_=0) == 0
    assert outs[0].hip.hipDeviceSynchronize() == 0
    for m in outs:
        assert (m.down(np.uint8, m.nbytes) == 0xC3).all()
    assert call() == 0 and outs[0].hip.hipDeviceSynchronize() == 0          # (and the same call with nothing wrong does write)
    assert not (outs[0].down(np.uint8, outs[0].nbytes) == 0xC3).all()
    for m in list(ins.values()) + outs:
        m.free()
