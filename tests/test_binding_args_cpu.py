"""CPU: the Python binding's one table of views, one argument path and one staging layout (cage_challenge_4_amd/_views.py, the as_* functions and
stage_layout of vec_env.py, int_tensor and its siblings of torch_env.py).  None of it needs a device, and none of it loads libcc4.so."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT

from cage_challenge_4_amd import _lib as L
from cage_challenge_4_amd import _views as V
from cage_challenge_4_amd.vec_env import as_actions, as_env_mask, as_messages, as_ptr, as_seeds, stage_layout

MAX_EDGES = (1, 7, L.BLUE_EDGES_MAX)


def _defines():
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    return {k: int(v, 0) for k, v in re.findall(r'^#define (CC4_[A-Z_0-9]+)\s+(-?(?:0x[0-9A-Fa-f]+|\d+))\b', txt, flags=re.M)}


def test_the_normalisers_do_not_load_the_library():
    code = ("import sys, ctypes\n"
            "from cage_challenge_4_amd import _lib, _views\n"
            "from cage_challenge_4_amd.vec_env import as_seeds, as_env_mask, as_actions, as_messages, as_ptr, stage_layout\n"
            "as_seeds(3, 4), as_actions([[0] * 5] * 4, 4), _views.empty('blue_edges', (2,), 5)\n"
            "assert _lib._lib is None, 'libcc4.so was loaded'\n"
            "assert 'torch' not in sys.modules\n")
    pr = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr


def test_table_restates_the_header_and_view_check():
    d = _defines()
    E = 'max_edges'
    want = {'state_features': ((('CC4_FEAT_HOSTS', 'CC4_FEAT_PER_HOST'), np.uint8, 0), (('CC4_FEAT_GLOBAL',), np.int32, 0)),
            'red_view': ((('CC4_NUM_RED', 'CC4_RED_VIEW_HOSTS', 'CC4_RED_VIEW_PER_HOST'), np.uint8, 0), (('CC4_NUM_RED', 'CC4_RED_VIEW_SCALARS'), np.int32, 0)),
            'blue_view': ((('CC4_NUM_BLUE', 'CC4_BLUE_VIEW_HOSTS', 'CC4_BLUE_VIEW_PER_HOST'), np.uint8, 0), (('CC4_NUM_BLUE', 'CC4_BLUE_VIEW_SCALARS'), np.int32, 0)),
            'blue_edges': (((E, 'CC4_BLUE_EDGES_COLUMNS'), np.int32, -1), (('CC4_BLUE_EDGES_WORDS',), np.int32, 0)),
            'reward_terms': ((('CC4_REWARD_SUBNETS', 'CC4_REWARD_COLS'), np.int32, 0), (('CC4_REWARD_WORDS',), np.int32, 0)),
            'sample_actions': ((('CC4_NUM_BLUE',), np.int32, -1), (('CC4_NUM_BLUE', 2), np.float32, 0))}
    assert set(V.VIEWS) == set(want)
    # the alignments: the two numbers every entry point hands view_check (csrc/cc4_api_views.hip)
    src = open(os.path.join(ROOT, 'cage_challenge_4_amd', 'csrc', 'cc4_api_views.hip')).read()
    aligns = {m[0]: (int(m[1]), int(m[2])) for m in re.findall(r'view_check\(h, "cc4_(\w+)_device",.*?, n, \w+, (\d+), \w+, (\d+),', src)}
    assert set(aligns) == set(want), aligns
    for name, view in V.VIEWS.items():
        assert view.device == f'cc4_{name}_device' and view.from_row == f'cc4_{name}_from_row'
        assert view.device in L.SIGNATURES and view.from_row in L.SIGNATURES
        for e in MAX_EDGES:
            outs = V.outs(name, e if name == 'blue_edges' else None)
            for o, (tail, dtype, fill), al in zip(outs, want[name], aligns[name]):
                assert o.tail == tuple(e if k == E else d.get(k, k) for k in tail), (name, o)
                assert (o.dtype, o.fill, o.align) == (np.dtype(dtype), fill, al), (name, o)
                assert o.align % o.dtype.itemsize == 0
            a, b = V.empty(name, (3,), e if name == 'blue_edges' else None)
            for x, o in zip((a, b), outs):
                assert x.shape == (3,) + o.tail and x.dtype == o.dtype and (x == o.fill).all()
    # ... and what _lib.py restates of the header
    for k in ('FEAT_HOSTS', 'FEAT_PER_HOST', 'FEAT_GLOBAL', 'RED_VIEW_HOSTS', 'RED_VIEW_PER_HOST', 'RED_VIEW_SCALARS', 'BLUE_VIEW_HOSTS', 'BLUE_VIEW_PER_HOST',
              'BLUE_VIEW_SCALARS', 'BLUE_EDGES_MAX', 'BLUE_EDGES_COLUMNS', 'BLUE_EDGES_WORDS', 'REWARD_SUBNETS', 'REWARD_COLS', 'REWARD_WORDS', 'NUM_BLUE',
              'NUM_RED', 'MSG_LEN', 'MASK_PER_ENV'):
        assert getattr(L, k) == d['CC4_' + k], k
    for bad in (0, L.BLUE_EDGES_MAX + 1, -1):
        with pytest.raises(ValueError, match='max_edges'):
            V.outs('blue_edges', bad)


def test_view_modules_keep_their_constants():
    from cage_challenge_4_amd import action_sampling, blue_edges, blue_view, red_view, reward_terms, state_features
    assert (state_features.FEAT_HOSTS, state_features.FEAT_PER_HOST, state_features.FEAT_GLOBAL) == (137, 16, 32) and len(state_features.HOST_COLUMNS) == 16
    assert (red_view.NUM_RED, red_view.VIEW_HOSTS, red_view.VIEW_PER_HOST, red_view.VIEW_SCALARS) == (6, 137, 8, 16) and len(red_view.SCALAR_WORDS) == 16
    assert (blue_view.NUM_BLUE, blue_view.VIEW_HOSTS, blue_view.VIEW_PER_HOST, blue_view.VIEW_SCALARS) == (5, 137, 8, 16) and len(blue_view.HOST_COLUMNS) == 8
    assert (blue_edges.MAX_EDGES, blue_edges.EDGE_COLUMNS, blue_edges.EDGE_WORDS, blue_edges.HOSTS) == (160, 8, 8, 137) and len(blue_edges.WORDS) == 8
    assert (reward_terms.SUBNETS, reward_terms.COLS, reward_terms.NWORDS) == (9, 4, 16) and len(reward_terms.WORDS) == 16
    assert action_sampling.SEGMENTS == (0, 82, 164, 246, 328, 570) and action_sampling.SLOTS == 570
    assert action_sampling.noise_words(-1, 2 ** 32 + 5) == (2 ** 64 - 1, 5)
    # the dtype codes: one table (include/cc4.h: "1 float16, 2 bfloat16, 3 float32", 0 the observations' bytes), and the modules' names for it
    from cage_challenge_4_amd import _tensors, action_logp, advantages
    assert _tensors.DTYPE_CODES == {'float16': 1, 'bfloat16': 2, 'float32': 3} and _tensors.OBS_DTYPE_CODES == dict(_tensors.DTYPE_CODES, uint8=0)
    assert action_logp.DTYPE_CODES is _tensors.DTYPE_CODES and advantages.DTYPE_CODES is _tensors.DTYPE_CODES
    assert _tensors.NUMPY_CODES == {np.dtype(np.float16): 1, np.dtype(np.uint16): 2, np.dtype(np.float32): 3}
    by_code = sorted(_tensors.OBS_DTYPE_CODES.items(), key=lambda kc: kc[1])
    assert 'obs_dtype ' + ', '.join(f'{c} {k}' for k, c in by_code) in open(os.path.join(ROOT, 'include', 'cc4.h')).read()


def _check_layout(parts):
    offsets, total = stage_layout(parts)
    end = 0
    for p, off in zip(parts, offsets):
        nbytes, align = (p.nbytes, 4) if isinstance(p, np.ndarray) else p       # (an input: int32 ids or float logits, 4 bytes at the least)
        assert off % align == 0, (parts, offsets)
        assert off >= end, (parts, offsets)                                     # in order, no overlap
        end = off + nbytes
    assert total == end
    return offsets


def test_stage_layout_places_every_part_at_its_alignment():
    for name in V.VIEWS:
        for e in (MAX_EDGES if name == 'blue_edges' else (None,)):
            for n in (1, 3, 7):
                outs = [(n * int(np.prod(o.tail)) * o.dtype.itemsize, o.align) for o in V.outs(name, e)]
                _check_layout(outs)
                _check_layout([np.zeros(n, np.int32)] + outs)
                _check_layout([np.zeros(n, np.int32), np.zeros((n, L.MASK_PER_ENV), np.float16)] + outs)
    # a first output of odd size: laying the second right behind it -- what the views' sizes used to allow -- would misplace it
    odd = [np.zeros(3, np.int32), (7, 1), (64, 16)]
    offsets = _check_layout(odd)
    assert (offsets[1] + 7) % 16 != 0 and offsets[2] == 32
    assert stage_layout([]) == ([], 0) and stage_layout([(5, 8)]) == ([0], 5)
    assert stage_layout([np.zeros(5, np.int32), np.zeros(3, np.uint8)]) == ([0, 32], 35)


def _spellings(exact):
    """The same values as a list, as int64, as a strided slice of a larger array, and as the exact array itself."""
    big = np.zeros((2,) + exact.shape, exact.dtype).repeat(2, axis=-1)
    big[1, ..., ::2] = exact
    return [exact.tolist(), exact.astype(np.int64), big[1, ..., ::2], exact]


@pytest.mark.parametrize('fn, dtype, shape, name', [(as_seeds, np.uint64, (4,), 'seeds'), (as_env_mask, np.uint8, (4,), 'env_mask'),
                                                    (as_actions, np.int32, (4, 5), 'actions'), (as_messages, np.uint8, (4, 5, 8), 'messages')])
def test_normalisers(fn, dtype, shape, name):
    n = 4
    exact = (np.arange(int(np.prod(shape))).reshape(shape) % 2).astype(dtype)
    assert fn(None, n) is None
    for x in _spellings(exact):
        got = fn(x, n)
        assert got.dtype == dtype and got.shape == shape and got.flags.c_contiguous and np.array_equal(got, exact)
        assert as_ptr(got).value == got.ctypes.data
    assert fn(exact, n) is exact                                     # the entry point's own dtype, contiguous: no copy
    for bad in (exact[:-1], exact[None], exact[..., None], np.zeros((0,) + shape[1:], dtype)):
        with pytest.raises(ValueError, match=name):
            fn(bad, n)
    with pytest.raises(ValueError, match=name):
        fn(exact, n + 1)


def test_scalar_seeds_and_plans():
    s = as_seeds(7, 3)
    assert s.dtype == np.uint64 and s.tolist() == [7, 8, 9]
    assert as_seeds(np.int64(2 ** 40), 2).tolist() == [2 ** 40, 2 ** 40 + 1]
    plan = np.zeros((6, 3, 5), np.int32)
    assert as_actions(plan, 3, 0) is plan and as_actions(plan, 3, 6) is plan and as_actions(plan[::2], 3, 0).flags.c_contiguous
    assert as_messages(np.zeros((6, 3, 5, 8), np.int64), 3, 6).dtype == np.uint8
    for bad, k in ((plan, 5), (plan[:0], 0), (plan[0], 0), (plan, None)):
        with pytest.raises(ValueError, match='actions'):
            as_actions(bad, 3, k)
    with pytest.raises(ValueError, match='messages'):
        as_messages(np.zeros((5, 3, 5, 8), np.uint8), 3, 6)
    import ctypes
    p = ctypes.c_void_p(64)
    assert as_ptr(None) is None and as_ptr(p) is p and as_ptr(4096).value == 4096


def test_tensor_checks():
    torch = pytest.importorskip('torch')
    from cage_challenge_4_amd.torch_env import int_tensor, mask_tensor, seed_tensor
    cpu = torch.device('cpu')
    good = torch.arange(12, dtype=torch.int64).reshape(3, 4)
    for bad in ('x', good.numpy(), good.float(), good.bool(), good[0], good[None], good[:2], good[:, :3], good.to('meta')):
        with pytest.raises(ValueError, match='things'):
            int_tensor(bad, (3, 4), cpu, 'things', to=torch.int32)
    for dt in (torch.int8, torch.int64, torch.uint8, torch.int32):
        got = int_tensor(good.to(dt), (3, 4), cpu, 'things', to=torch.int32)
        assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got, good.int())
    exact = good.int()
    assert int_tensor(exact, (3, 4), cpu, 'things', to=torch.int32).data_ptr() == exact.data_ptr()       # nothing to cast: no copy
    wide = torch.arange(24, dtype=torch.int64).reshape(3, 8)[:, ::2]
    got = int_tensor(wide, (3, None), cpu, 'things', to=torch.int32)
    assert not wide.is_contiguous() and got.is_contiguous() and torch.equal(got, wide.int())
    assert int_tensor(good[:0], (None, 4), cpu, 'things', to=torch.int32).shape == (0, 4)
    big = torch.tensor([2 ** 31 + 1, -2 ** 40, 5])
    assert int_tensor(big, (3,), cpu, 'things', to=torch.int32, saturate=True).tolist() == [2 ** 31 - 1, -2 ** 31, 5]
    assert int_tensor(big, (3,), cpu, 'things', to=torch.int32).tolist() == [-2 ** 31 + 1, 0, 5]
    assert int_tensor(good.bool(), (3, 4), cpu, 'things', to=torch.uint8, bool_ok=True).dtype == torch.uint8
    # seeds: uint64 viewed, not cast; any other integer dtype cast
    u = torch.tensor([2 ** 63 + 3, 1, 2], dtype=torch.uint64)
    got = seed_tensor(u, 3, cpu)
    assert got.dtype == torch.int64 and got.data_ptr() == u.data_ptr() and got.tolist() == [-2 ** 63 + 3, 1, 2]
    assert seed_tensor(torch.tensor([1, 2, 3], dtype=torch.int16), 3, cpu).dtype == torch.int64
    for bad in (u[:2], torch.zeros(3), torch.zeros(3, dtype=torch.bool), [1, 2, 3], u.to('meta')):
        with pytest.raises(ValueError, match='seeds'):
            seed_tensor(bad, 3, cpu)
    # masks: bool (copied) or uint8 (as it is)
    b = torch.tensor([True, False, True])
    got = mask_tensor(b, 3, cpu)
    assert got.dtype == torch.uint8 and got.tolist() == [1, 0, 1] and got.data_ptr() != b.data_ptr()
    m8 = got.clone()
    assert mask_tensor(m8, 3, cpu).data_ptr() == m8.data_ptr()
    for bad in (b[:2], b.int(), b.float(), [1, 0, 1], b.to('meta')):
        with pytest.raises(ValueError, match='env_mask'):
            mask_tensor(bad, 3, cpu)
