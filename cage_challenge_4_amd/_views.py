"""The derived views in one table: for each, its two entry points and -- per output -- the shape of one entry, the NumPy dtype, the fill of an
empty row and the alignment the device entry point demands.  Everything in Python that allocates, checks or lays out a view's outputs reads it
here (CC4VecEnv._view, CC4TorchVecEnv._view, the from_row / from_true_state functions of the view modules).  No torch, and the library is not
loaded.  A new view is one entry here, a one-line method on each env and its module."""
from collections import namedtuple
import numpy as np
from . import _lib as L

Out = namedtuple('Out', 'tail dtype fill align')      # tail: the shape behind the entry axis -- for blue_edges a function of max_edges
View = namedtuple('View', 'device from_row outs')


def _view(name, *outs):
    return View(f'cc4_{name}_device', f'cc4_{name}_from_row', tuple(Out(t, np.dtype(d), f, a) for t, d, f, a in outs))


# The alignments are view_check's in csrc/cc4_api_views.hip (align0, align1 of each cc4_*_device entry point); tests/test_binding_args_cpu.py
# holds the shapes against include/cc4.h.
VIEWS = {
    'state_features': _view('state_features', ((L.FEAT_HOSTS, L.FEAT_PER_HOST), np.uint8, 0, 16), ((L.FEAT_GLOBAL,), np.int32, 0, 4)),
    'red_view': _view('red_view', ((L.NUM_RED, L.RED_VIEW_HOSTS, L.RED_VIEW_PER_HOST), np.uint8, 0, 16), ((L.NUM_RED, L.RED_VIEW_SCALARS), np.int32, 0, 4)),
    'blue_view': _view('blue_view', ((L.NUM_BLUE, L.BLUE_VIEW_HOSTS, L.BLUE_VIEW_PER_HOST), np.uint8, 0, 8), ((L.NUM_BLUE, L.BLUE_VIEW_SCALARS), np.int32, 0, 4)),
    'blue_edges': _view('blue_edges', (lambda max_edges: (max_edges, L.BLUE_EDGES_COLUMNS), np.int32, -1, 16), ((L.BLUE_EDGES_WORDS,), np.int32, 0, 4)),
    'reward_terms': _view('reward_terms', ((L.REWARD_SUBNETS, L.REWARD_COLS), np.int32, 0, 16), ((L.REWARD_WORDS,), np.int32, 0, 16)),
    'sample_actions': _view('sample_actions', ((L.NUM_BLUE,), np.int32, -1, 4), ((L.NUM_BLUE, 2), np.float32, 0, 4)),
}


def check_max_edges(max_edges):
    max_edges = int(max_edges)
    if not 1 <= max_edges <= L.BLUE_EDGES_MAX:
        raise ValueError(f'max_edges must be 1 .. {L.BLUE_EDGES_MAX}, got {max_edges}')
    return max_edges


def outs(view, max_edges=None):
    """The view's two outputs with their tails as tuples (blue_edges: for max_edges, checked)."""
    return tuple(o._replace(tail=o.tail(check_max_edges(max_edges))) if callable(o.tail) else o for o in VIEWS[view].outs)


def empty(view, lead=(), max_edges=None):
    """The view's two arrays as an episode that produced nothing fills them, [*lead, *tail]."""
    return tuple(np.full(tuple(lead) + o.tail, o.fill, o.dtype) for o in outs(view, max_edges))
