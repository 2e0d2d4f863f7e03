"""What the view modules (state_features, red_view, blue_view, blue_edges, reward_terms) share: the byte-row and document arguments of their
from_row / from_true_state functions, the call of a from_row entry point on outputs from the table of views, and the two facts about the per-step event log that blue_view and blue_edges both restate in NumPy."""
import ctypes
import json
import numpy as np
from . import _lib as L
from . import _views as V

MAX_EVENTS = 160                         # entries the per-step log holds (a larger total: truncated, not valid)
ZONE_OF_SUBNET = (0, 1, 2, 3, -1, 4, 4, 4, -1)      # the blue agent that defends the subnet; -1: nobody


def _bytes(x, size, what):
    if isinstance(x, (bytes, bytearray, memoryview)):
        x = np.frombuffer(x, np.uint8)
    x = np.ascontiguousarray(x, dtype=np.uint8).ravel()
    if size is not None and x.size != size:
        raise ValueError(f'{what} has {size} bytes, got {x.size}')
    return x


def _rows(hot, cold):
    """(hot row, cold row or None) as byte arrays: the hot row of cc4_state_bytes(), the cold row the whole cc4_cold_bytes() of its env."""
    return _bytes(hot, L.load().cc4_state_bytes(), 'a hot row'), None if cold is None else _bytes(cold, None, 'a cold row')


def call_from_row(view, *args, max_edges=None, ok=(0,)):
    """The view's cc4_*_from_row entry point (_views.VIEWS) on args -- arrays go as pointers -- in front of its two outputs, allocated from the
    table: (first, second, rc).  An rc outside `ok` raises CC4Error."""
    name = V.VIEWS[view].from_row
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p) if isinstance(x, np.ndarray) else x      # noqa: E731
    a, b = V.empty(view, max_edges=max_edges)
    rc = getattr(L.load(), name)(*map(ptr, args), ptr(a), ptr(b))
    if rc not in ok:
        raise L.CC4Error(f'{name} failed (rc={rc})')
    return a, b, rc


def _doc(doc):
    if isinstance(doc, (str, bytes)):
        return json.loads(doc)
    return doc if isinstance(doc, dict) else doc.raw


def events_valid(doc):
    """The document's event log describes the step just taken and is complete."""
    d = _doc(doc)
    return 'events' in d and d['step'] >= 1 and d['events_step'] + 1 == d['step'] and d['events_total'] <= MAX_EVENTS
