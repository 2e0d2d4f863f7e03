"""What the view modules (state_features, red_view, blue_view, blue_edges, reward_terms) share: the byte-row and document arguments of their
from_row / from_true_state functions, and the two facts about the per-step event log that blue_view and blue_edges both restate in NumPy."""
import json
import numpy as np

MAX_EVENTS = 160                         # entries the per-step log holds (a larger total: truncated, not valid)
ZONE_OF_SUBNET = (0, 1, 2, 3, -1, 4, 4, 4, -1)      # the blue agent that defends the subnet; -1: nobody


def _bytes(x, size, what):
    if isinstance(x, (bytes, bytearray, memoryview)):
        x = np.frombuffer(x, np.uint8)
    x = np.ascontiguousarray(x, dtype=np.uint8).ravel()
    if size is not None and x.size != size:
        raise ValueError(f'{what} has {size} bytes, got {x.size}')
    return x


def _doc(doc):
    if isinstance(doc, (str, bytes)):
        return json.loads(doc)
    return doc if isinstance(doc, dict) else doc.raw


def events_valid(doc):
    """The document's event log describes the step just taken and is complete."""
    d = _doc(doc)
    return 'events' in d and d['step'] >= 1 and d['events_step'] + 1 == d['step'] and d['events_total'] <= MAX_EVENTS
