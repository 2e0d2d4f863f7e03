"""Masked sampling of the blue actions from policy logits (include/cc4.h, cc4_sample_actions_device): the step from a policy's [570] logits to the
[5] action indices step() takes -- the slots this episode's topology does not have masked out, busy agents left out (their submission would be
dropped), one slot per agent drawn from the five segments SEGMENTS, and the log-probability and entropy of the draw.

Per agent b with the valid slots of its segment: x = logits / temperature, action = arg-max over the valid slots of x + Gumbel noise (a draw
from softmax(x over the valid slots); greedy: of x alone), logp = log softmax(x)[action], entropy of that softmax.  The noise is a fixed function
of (seed, t, the entry's id e, agent, slot): Philox4x32-10, key seed + e, counter (t, b, 0x5A3B, slot >> 2), slot i takes word i & 3,
u = (2 (w >> 9) + 1) / 2^24, g = -log(-log(u)).  A busy agent (busy_aware) and an agent whose valid logits hold a NaN or +inf or are all -inf get
action -1 -- "submits nothing", which the step resolves like Sleep -- and zero stats.

Three ways to the same numbers:
  CC4VecEnv.sample_actions() / CC4TorchVecEnv.sample_actions()   the HIP kernel over the batch (k_sample_actions), float32
  from_row(hot, logits, seed, t, e, ...)     the same definition compiled for the host (cc4_sample_actions_from_row), float32, no GPU
  reference(mask, busy, logits, seed, t, e, ...)   a NumPy restatement in float64 from the mask row and the busy flags only, with a NumPy Philox"""
import math
import numpy as np
from . import _lib as L
from ._view_util import _bytes, call_from_row

NUM_BLUE = L.NUM_BLUE
SLOTS = L.MASK_PER_ENV
SEGMENTS = (0, 82, 164, 246, 328, 570)
GREEDY, BUSY, TAG = L.SAMPLE_GREEDY, L.SAMPLE_BUSY, L.SAMPLE_TAG
STATS = {'logp': 0, 'entropy': 1}


def check_temperature(temperature):
    temperature = float(temperature)
    if not (temperature > 0.0 and math.isfinite(temperature)):
        raise ValueError(f'temperature must be finite and positive, got {temperature}')
    return temperature


def flags_of(greedy, busy_aware):
    return (GREEDY if greedy else 0) | (BUSY if busy_aware else 0)


def noise_words(seed, t):
    """(seed, t) as the uint64 and uint32 words the entry points take: any Python integers, reduced modulo 2^64 and 2^32."""
    return int(seed) & (2 ** 64 - 1), int(t) & 0xFFFFFFFF


def _logits_row(logits):
    if logits is None:
        return None
    a = np.asarray(logits)
    if a.shape != (SLOTS,):
        raise ValueError(f'logits must have shape ({SLOTS},), got {a.shape}')
    if a.dtype.kind != 'f':
        raise ValueError(f'logits must be floating point, got {a.dtype}')
    return np.ascontiguousarray(a, dtype=np.float32)


def from_row(hot, logits, seed, t, e, temperature=1.0, greedy=False, busy_aware=True):
    """(actions [5] int32, stats [5, 2] float32 (logp, entropy), refused bool) of one packed hot row (CC4VecEnv.get_state(e)) and its [570]
    logits (float16 / float32 / float64 values, taken as float32; None: uniform over the valid slots).  e: the id of the entry -- the episode
    or bank slot the row belongs to.  refused: some agent's valid logits held a NaN or +inf or were all -inf (its action is -1)."""
    temperature = check_temperature(temperature)
    hot = _bytes(hot, L.load().cc4_state_bytes(), 'a hot row')
    seed, t = noise_words(seed, t)
    actions, stats, rc = call_from_row('sample_actions', hot, _logits_row(logits), seed, t, int(e), temperature, flags_of(greedy, busy_aware), ok=(0, 1))
    return actions, stats, bool(rc)


def philox4x32_10(counter, key):
    """Philox4x32-10 on arrays: counter four uint64 arrays holding 32-bit words, key (k0, k1) likewise.  Returns the four output words."""
    m0, m1, w0, w1, lo = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85), np.uint64(0xFFFFFFFF)
    c = [np.asarray(x, np.uint64) for x in counter]
    k0, k1 = (np.asarray(x, np.uint64) for x in key)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [((p1 >> s32) ^ c[1] ^ k0) & lo, p1 & lo, ((p0 >> s32) ^ c[3] ^ k1) & lo, p0 & lo]
        k0, k1 = (k0 + w0) & lo, (k1 + w1) & lo
    return c


def gumbel(seed, t, e):
    """g of the 570 slots of entry e for (seed, t), float64: the five agents' blocks in one Philox call."""
    key = (int(seed) + int(e)) & (2 ** 64 - 1)
    nb = [(SEGMENTS[b + 1] - SEGMENTS[b] + 3) // 4 for b in range(NUM_BLUE)]
    agent = np.repeat(np.arange(NUM_BLUE, dtype=np.uint64), nb)
    block = np.concatenate([np.arange(k, dtype=np.uint64) for k in nb])
    z = np.zeros(agent.size, np.uint64)
    c = philox4x32_10((z + np.uint64(int(t) & 0xFFFFFFFF), agent, z + np.uint64(TAG), block), (z + np.uint64(key & 0xFFFFFFFF), z + np.uint64(key >> 32)))
    w = np.stack(c, axis=1)                      # [blocks, 4]: slot i of an agent is word i & 3 of its block i >> 2
    at = np.cumsum([0] + nb)
    w = np.concatenate([w[at[b]:at[b + 1]].reshape(-1)[:SEGMENTS[b + 1] - SEGMENTS[b]] for b in range(NUM_BLUE)])
    u = (2.0 * (w >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24
    return -np.log(-np.log(u))


def reference(mask, busy, logits, seed, t, e, temperature=1.0, greedy=False, busy_aware=True, details=False):
    """The definition in float64 NumPy from the entry's mask row [570] (info['action_mask'], CC4VecEnv.action_mask) and busy flags [5]
    (blue_view scalars[..., 0]).  Returns (actions [5] int32, logp [5], entropy [5], margin [5]) -- margin: the winning score minus the
    second-best valid score (inf where there is no second, for -1 actions too): a float32 implementation may differ where it is tiny.
    details=True appends a dict: 'second' [5] the runner-up slot (-1: none), 'logp_second' [5] its log-probability, 'zmax' [5] the largest
    |score| among the agent's finite scores (at least 1)."""
    temperature = check_temperature(temperature)
    mask = np.asarray(mask).astype(bool)
    lg = None if logits is None else np.asarray(logits, dtype=np.float64)
    if mask.shape != (SLOTS,) or (lg is not None and lg.shape != (SLOTS,)):
        raise ValueError(f'mask and logits must have shape ({SLOTS},)')
    r = float(np.float32(1.0) / np.float32(temperature))
    actions = np.full(NUM_BLUE, -1, np.int32)
    logp, ent, margin = np.zeros(NUM_BLUE), np.zeros(NUM_BLUE), np.full(NUM_BLUE, np.inf)
    second, logp2, zmax = np.full(NUM_BLUE, -1, np.int32), np.zeros(NUM_BLUE), np.ones(NUM_BLUE)
    g = None if greedy else gumbel(seed, t, e)
    for b in range(NUM_BLUE):
        lo, hi = SEGMENTS[b], SEGMENTS[b + 1]
        if busy_aware and busy[b]:
            continue
        valid = np.nonzero(mask[lo:hi])[0]
        with np.errstate(invalid='ignore', over='ignore'):
            x = np.zeros(valid.size) if lg is None else lg[lo:hi][valid] * r
            x = np.where(np.abs(x) > float(np.finfo(np.float32).max), np.sign(x) * np.inf, x)      # x is a float32 product: it overflows where float32 does
        if np.isnan(x).any() or (x == np.inf).any() or (x == -np.inf).all():
            continue
        m = x.max()
        ex = np.exp(x - m)
        s = ex.sum()
        p = ex / s
        z = x if greedy else x + g[lo:hi][valid]
        order = np.lexsort((valid, -z))              # largest score first, the lowest index among equals
        a = order[0]
        actions[b] = valid[a]
        logp[b] = x[a] - m - math.log(s)
        pos = p > 0
        ent[b] = -(p[pos] * np.log(p[pos])).sum()
        finite = np.isfinite(z)
        zmax[b] = max(1.0, np.abs(z[finite]).max())
        if finite.sum() > 1:
            margin[b] = z[order[0]] - z[order[1]]
            second[b], logp2[b] = valid[order[1]], x[order[1]] - m - math.log(s)
    if details:
        return actions, logp, ent, margin, {'second': second, 'logp_second': logp2, 'zmax': zmax}
    return actions, logp, ent, margin
