"""Host reference of the library's random numbers: Philox4x32-10 and the maps from its words to uniforms, normals and Bernoullis.

Written from the definition of Philox (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and from the
keying include/ardae_hip.h describes; numpy only - no GPU, no library.  tests/test_philox.py pins `words` to the Random123 known-answer
vectors, so the reference stands on its own and the device code (csrc/philox.h) is compared against it, not the other way round.

Keying of a draw (seed, offset): counter number q (a uint64) gives four 32-bit words,
    counter = (q lo, q hi, offset lo, offset hi),  key = (seed lo, seed hi),
and element e of the draw is word e % 4 of counter e // 4.  All arithmetic is modulo 2^32 / 2^64.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two multipliers of a round
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the Weyl increments of the key (golden ratio, sqrt(3) - 1)
ROUNDS = 10
MASK32, MASK64 = (1 << 32) - 1, (1 << 64) - 1
TWO_M24 = 2.0 ** -24


def philox4x32(counter, key, rounds=ROUNDS):
    """counter: four uint32 arrays (or ints), key: two ints -> four uint32 arrays.  The bijection itself, for the known-answer vectors."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & np.uint64(MASK32) for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bit: never wraps
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return [w.astype(np.uint32) for w in c]


def words(seed, offset, idx):
    """The four words of each counter in `idx` (uint64 array, or anything np.asarray takes) -> uint32 array [len(idx), 4]."""
    seed, offset = int(seed) & MASK64, int(offset) & MASK64
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    counter = (idx & np.uint64(MASK32), idx >> np.uint64(32), offset & MASK32, offset >> 32)
    return np.stack(philox4x32(counter, (seed & MASK32, seed >> 32)), axis=1)


def counters(first_counter, count):
    """first_counter, first_counter + 1, ... modulo 2^64 as a uint64 array."""
    with np.errstate(over="ignore"):
        return np.uint64(int(first_counter) & MASK64) + np.arange(count, dtype=np.uint64)


def _elements(seed, offset, first_element, n):
    first_element = int(first_element)
    if first_element % 4:
        raise ValueError("first_element must be a multiple of 4 (one counter = 4 elements)")
    return words(seed, offset, counters(first_element >> 2, (int(n) + 3) // 4))


def uniform(seed, offset, n, first_element=0):
    """float32 [n] in [0, 1): (word >> 8) 2^-24, exact in fp32."""
    w = _elements(seed, offset, first_element, n).reshape(-1)[:n]
    return ((w >> np.uint32(8)).astype(np.float64) * TWO_M24).astype(np.float32)


def u01_open(w):
    """(0, 1]: ((word >> 8) + 1) 2^-24 in float64 (exact there and in fp32)."""
    return ((w >> np.uint32(8)).astype(np.float64) + 1.0) * TWO_M24


def normal(seed, offset, first_element, n):
    """float64 [n]: elements [first_element, first_element + n) of the normal draw (seed, offset).  Box-Muller on the exact words: per
    counter, words (0, 1) and (2, 3) give (rad cos, rad sin) with rad = sqrt(-2 ln u(word 0 | 2)), angle = 2 pi u(word 1 | 3)."""
    w = _elements(seed, offset, first_element, n)
    out = np.empty((w.shape[0], 4), dtype=np.float64)
    for h in (0, 1):
        rad = np.sqrt(-2.0 * np.log(u01_open(w[:, 2 * h])))
        ang = 2.0 * np.pi * u01_open(w[:, 2 * h + 1])
        out[:, 2 * h], out[:, 2 * h + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return out.reshape(-1)[:n]


def bernoulli(p, rows, cols, seed, offset):
    """float32 [rows, cols] of 0 / 1: uniform element e < p[e % cols], compared in float32 (strict)."""
    p = np.asarray(p, dtype=np.float32).reshape(-1)
    assert p.size == cols
    u = uniform(seed, offset, rows * cols).reshape(rows, cols)
    return (u < p[None, :]).astype(np.float32)


def step_offset(offset, rng_offset):
    """The offset a draw uses when a step state is given: (offset + state.rng_offset) mod 2^64."""
    return (int(offset) + int(rng_offset)) & MASK64


def find_edge_counters(seed, offset, stop, start=0, chunk=1 << 20):
    """Counters in [start, stop) with a word whose top 24 bits are all zero or all one - the ends of both word-to-uniform maps.
    -> list of (counter, word index, "zero" | "one") in counter order.  (About 3 s per 10 M counters; tests/test_philox.py only
    confirms the constants this found.)"""
    found = []
    for lo in range(int(start), int(stop), chunk):
        q = counters(lo, min(chunk, int(stop) - lo))
        top = words(seed, offset, q) >> np.uint32(8)
        for kind, hit in (("zero", top == 0), ("one", top == 0xFFFFFF)):
            for r, c in zip(*np.nonzero(hit)):
                found.append((int(q[r]), int(c), kind))
    return sorted(found)
