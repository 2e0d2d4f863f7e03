"""Crafted PCG64 states (plain Python integers): a generator whose d-th 64-bit output from now is a chosen value.

PCG64 is an invertible 128-bit LCG (state' = state * M + inc mod 2^128) with the XSL-RR 128/64 output function
out = rotr(hi ^ lo, hi >> 58).  For a wanted output pick any high word, solve for the low word, and walk the state back d steps
with M^-1.  set_generators (CC4VecEnv and OracleVecEnv) places such a state into an episode on both sides, so the draws that chance
meets once in 2^32 -- a zero word in a bounded draw (Lemire's re-draw), a zero buffered half word, a uniform below 0.01 where it
also needs a port -- are met at a known offset of a known phase (tests/test_pcg_rare_draws*.py)."""
import numpy as np

M = 0x2360ED051FC65DA44385DF649FCCF645       # PCG_DEFAULT_MULTIPLIER_128 (numpy/random/src/pcg64/pcg64.h)
MASK128 = (1 << 128) - 1
MASK64 = (1 << 64) - 1
M_INV = pow(M, -1, 1 << 128)
P01_64 = (1 << 64) // 100                    # floor(0.01 * 2^64): (v >> 11) * 2^-53 < 0.01 for every v below it

KINDS = ('Z', 'L', 'H', 'T', 'F')
# the entry buffer of an episode (has_uint32, uinteger; None = random): nothing buffered, a zero half word, an all-ones one, a random one
BUFFERS = ((0, 0), (1, 0), (1, 0xFFFFFFFF), (1, None))

# the crafted batch of the rare-draw tests
SEED0, ACT_SEED, WARMUP, STEPS = 4242, 99, 25, 500
D = 192                                      # planted offsets 1 .. D: two steps consume at least that many outputs (test_pcg_rare_draws_cpu.py asserts it)
# the per-step cases: batch, constructor arguments, event log, steps behind the planting (enough for every episode to pass its planted output: with
# SleepAgent greens a step draws a third as much), blue actions of those steps (False: none, the built-in policy draws them), seed of the planting
CASES = {
    'k_step': dict(n=2 * 5 * D, kw={}, evlog=False, steps=2, actions=True, seed=1),
    'k_step-builtin-blue': dict(n=2 * 5 * D, kw={'blue_policy': 1}, evlog=False, steps=2, actions=False, seed=2),
    'k_step-event-log': dict(n=5 * D, kw={}, evlog=True, steps=2, actions=True, seed=3),
    'k_step-sleep-greens': dict(n=5 * D, kw={'green_policy': 1}, evlog=False, steps=6, actions=True, seed=4),
}


def _rotl64(v, r):
    r &= 63
    return ((v << r) | (v >> ((64 - r) & 63))) & MASK64


def state_for(output64, inc128, d, rng):
    """The 128-bit state whose d-th output from now (d >= 1: the d-th call of random_raw) is output64, for the stream with increment inc128."""
    assert d >= 0 and 0 <= output64 <= MASK64 and inc128 & 1
    hi = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    lo = hi ^ _rotl64(output64, hi >> 58)
    s = (hi << 64) | lo
    for _ in range(d):
        s = ((s - inc128) * M_INV) & MASK128
    return s


def generator(state, inc, has_uint32=0, uinteger=0):
    g = np.random.Generator(np.random.PCG64(0))
    g.bit_generator.state = {'bit_generator': 'PCG64', 'state': {'state': int(state), 'inc': int(inc)},
                             'has_uint32': int(has_uint32), 'uinteger': int(uinteger)}
    return g


def planted_output(kind, rng):
    """Z: 0 (both halves zero: every bounded draw that meets it draws again, every random() < 0.01 fires).  L / H: low / high half zero, the other
    random and non-zero.  T: below floor(0.01 * 2^64) with both halves non-zero (fires the 1 % events without a re-draw).  F: 2^64 - 1 (a
    bounded draw picks the last index; the shuffle's masked rejection rejects it for every i that is not 2^k - 1)."""
    nz32 = lambda: int(rng.integers(1, 1 << 32))     # noqa: E731
    if kind == 'Z':
        return 0
    if kind == 'L':
        return nz32() << 32
    if kind == 'H':
        return nz32()
    if kind == 'T':
        v = (int(rng.integers(1, P01_64 >> 32)) << 32) | nz32()
        assert v < P01_64
        return v
    assert kind == 'F'
    return MASK64


def entry_buffer(b, rng):
    has, u = BUFFERS[b]
    return has, (int(rng.integers(1, 0xFFFFFFFF)) if u is None else u)


def batch_cells(n, depth=D):
    """[n, 3] (kind index, offset d in 1 .. depth, entry buffer index) of the crafted batch: the 5 x depth (kind, offset) cells in order, repeated over
    the batch.  A batch of exactly two repeats takes the first with nothing buffered and the second with a buffered half word whose three values
    are spread evenly; any other size cycles the four buffers over cells and repeats, so that four repeats meet every (kind, offset, buffer)."""
    cells = np.zeros((n, 3), np.int64)
    per = len(KINDS) * depth
    for e in range(n):
        c, rep = e % per, e // per
        if n == 2 * per:
            b = 0 if rep == 0 else 1 + (c + c // 3) % 3
        else:
            b = (rep + c + c // 4) % 4
        cells[e] = (c // depth, c % depth + 1, b)
    return cells


def crafted_generators(rng_words, cells, seed):
    """One numpy Generator(PCG64) per episode: the increment the episode's stream has (rng_words: rows of rng_state()), a fresh random position
    on it, the planted output of the cell's kind at the cell's offset and the cell's entry buffer."""
    rng = np.random.default_rng(seed)
    gens = []
    for w, (k, d, b) in zip(rng_words, cells):
        inc = (int(w[2]) << 64) | int(w[3])
        out = planted_output(KINDS[k], rng)
        s = state_for(out, inc, int(d), rng)
        has, u = entry_buffer(int(b), rng)
        gens.append(generator(s, inc, has, u))
    return gens


def case_actions(case, t, n):
    """The blue actions of step t (counted from the reset) of a per-step case."""
    from oracle_binding import random_actions
    a = random_actions(ACT_SEED, t, n)
    if t >= WARMUP and not case['actions']:
        a[:] = -1
    return a
