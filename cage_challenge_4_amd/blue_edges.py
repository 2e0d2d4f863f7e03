"""The Monitor's connection entries as edge lists: who talked to whom in the step just taken (include/cc4.h, cc4_blue_edges_device).  blue_view
counts the connection entries per host; the reference's dict observation also says which remote host connected to which local host on which ports,
  Processes[..].Connections[..] = {local_address, local_port, remote_address, remote_port}
and graph / attention policies are built on those pairs.

Per episode  edges [E, 8] int32   E = max_edges (1 .. MAX_EDGES), columns COLUMNS; rows past the number of edges are -1 in every column, so
                                  edges[..., 0] >= 0 is the validity mask
             counts [8] int32     WORDS: distinct edges per agent (the agents' segments are contiguous, agent 0 first), their total, events_valid,
                                  step_count -- always the untruncated numbers: counts[5] > E shows truncation
An entry of the per-step event log qualifies iff it is a connection entry with a remote address, appended at least once, on an existing host of a
blue agent's zone.  Entries equal in (agent, host, remote, local, local_port, remote_port) merge into one edge whose count is the sum; the edges
are sorted by that tuple, so the list never depends on the order in which the step appended its entries.  Which agent acted and pids enter nowhere.
The per-step event log must be on (enable_event_log()): without a valid log every row is -1 and counts[6] is 0.

Three ways to the same numbers:
  CC4VecEnv.blue_edges() / CC4TorchVecEnv.blue_edges()   the HIP kernel over the batch (k_blue_edges)
  from_row(hot, cold, steps, max_edges)   the same definition compiled for the host (cc4_blue_edges_from_row), in a process without a GPU
  from_true_state(doc, max_edges)         a NumPy restatement from the true-state document only: independent of the packed rows
and to_edge_index(edges) turns a batch of lists into the [2, M] node-id pairs a PyG-style layer takes."""
from . import _lib as L
from . import _views as V
from ._views import check_max_edges
from ._view_util import MAX_EVENTS, ZONE_OF_SUBNET, _doc, _rows, call_from_row, events_valid  # noqa: F401  (MAX_EVENTS: part of this module's surface)

NUM_BLUE, MAX_EDGES, EDGE_COLUMNS, EDGE_WORDS = L.NUM_BLUE, L.BLUE_EDGES_MAX, L.BLUE_EDGES_COLUMNS, L.BLUE_EDGES_WORDS
HOSTS = 137
COLUMNS = {'agent': 0, 'host': 1, 'local': 2, 'remote': 3, 'local_port': 4, 'remote_port': 5, 'count': 6, 'slot': 7}
WORDS = {'edges_0': 0, 'edges_1': 1, 'edges_2': 2, 'edges_3': 3, 'edges_4': 4, 'total': 5, 'events_valid': 6, 'step_count': 7}


def from_row(hot, cold, steps=0, max_edges=MAX_EDGES):
    """(edges [max_edges, 8] int32, counts [8] int32) of one packed hot row (CC4VecEnv.get_state(e)) and its cold row (the second part of
    CC4VecEnv.snapshot(e); the whole cc4_cold_bytes() of that env).  cold=None: no edges, events_valid 0.  steps: the episode length of the
    env the rows come from; 0: the length the hot row itself records."""
    max_edges = check_max_edges(max_edges)
    return call_from_row('blue_edges', *_rows(hot, cold), int(steps), max_edges, max_edges=max_edges)[:2]


def from_true_state(doc, max_edges=MAX_EDGES):
    """The same arrays from a true-state document (the JSON text of cc4_get_true_state, its parsed form, or true_state.TrueState): from
    "events" / "events_step" / "events_total", "step" and the ids of "hosts" only, with a dictionary and a Python sort."""
    d = _doc(doc)
    edges, counts = V.empty('blue_edges', max_edges=max_edges)
    max_edges = len(edges)
    valid = events_valid(d)
    counts[6], counts[7] = int(valid), d['step']
    if not valid:
        return edges, counts
    exists = {hd['h'] for hd in d['hosts']}
    merged = {}
    for _order, _seq, host, kind, laddr, lport, raddr, rport, _pid, rep in d['events']:
        if kind != 0 or rep <= 0 or host >= HOSTS or host not in exists or raddr >= HOSTS:
            continue
        b = ZONE_OF_SUBNET[host // 17]
        if b < 0:
            continue
        key = (b, host, raddr, laddr, lport, rport)
        merged[key] = merged.get(key, 0) + rep
    slot = [0] * NUM_BLUE
    for i, key in enumerate(sorted(merged)):
        b, host, raddr, laddr, lport, rport = key
        if i < max_edges:
            edges[i] = (b, host, laddr if laddr < HOSTS else -1, raddr, lport, rport, merged[key], slot[b])
        slot[b] += 1
    counts[:NUM_BLUE], counts[5] = slot, len(merged)
    return edges, counts


def to_edge_index(edges, agent=None):
    """A batch of edge lists as a graph: edges [N, E, 8] (or [E, 8]) int32, a torch tensor on any device.  Returns (edge_index [2, M] int64,
    rows [M] int64): edge_index[0] the node id of the remote host, edge_index[1] that of the reporting host, node id = episode * 137 + host --
    the (source, target) pairs a PyG-style message-passing layer takes -- and rows the indices of the M valid edges into edges.reshape(-1, 8)
    (for edge features: ports, count).  agent: only the edges of that blue agent.  M is data: the call waits for the device."""
    import torch
    if edges.dim() == 2:
        edges = edges.unsqueeze(0)
    n, e, _ = edges.shape
    flat = edges.reshape(n * e, EDGE_COLUMNS)
    keep = flat[:, 0] >= 0 if agent is None else flat[:, 0] == int(agent)
    rows = torch.nonzero(keep, as_tuple=False).squeeze(1)
    base = torch.div(rows, e, rounding_mode='floor') * HOSTS
    sel = flat.index_select(0, rows).to(torch.int64)
    return torch.stack((base + sel[:, 3], base + sel[:, 1])), rows
