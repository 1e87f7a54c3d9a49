"""The host reference of the random numbers (oracle/philox_ref.py) pinned to what does not depend on this repository: the Random123
known-answer vectors of philox4x32_10.  tests/test_philox_gpu.py then pins the device draws to the reference."""
import numpy as np
import pytest

from oracle import philox_ref as P

# Random123 (kat_vectors): philox4x32 10 rounds - counter, key, expected output
KAT = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
# counters of the draw (EDGE_SEED, EDGE_OFFSET) that hit the ends of the word-to-uniform maps (found by P.find_edge_counters):
# (counter, word, the word's top 24 bits)
EDGE_SEED, EDGE_OFFSET = 0x5EED, (1 << 63) | 7
EDGES = [(101026, 0, 0x000000),      # u = 2^-24: the largest radius, sqrt(48 ln 2) = 5.768
         (2343065, 0, 0xFFFFFF),     # u = 1: radius 0
         (2554395, 2, 0xFFFFFF),     # u = 1: radius 0 (second pair)
         (1669379, 3, 0x000000),     # angle 2^-24 revolutions
         (6808754, 3, 0xFFFFFF)]     # angle exactly one revolution


def hexwords(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_known_answer_vectors(counter, key, want):
    c, k = hexwords(counter), hexwords(key)
    got = [int(w[0]) for w in P.philox4x32(c, k)]
    assert got == hexwords(want)
    # the same through the library's keying: counter = (idx lo, idx hi, offset lo, offset hi), key = (seed lo, seed hi)
    idx, offset, seed = c[0] | c[1] << 32, c[2] | c[3] << 32, k[0] | k[1] << 32
    assert P.words(seed, offset, [idx])[0].tolist() == hexwords(want)


def test_words_is_vectorised_and_wraps():
    seed, offset = 0x9E3779B97F4A7C15, (1 << 63) | 7
    idx = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    w = P.words(seed, offset, idx)
    assert w.shape == (6, 4) and w.dtype == np.uint32
    for i, q in enumerate(idx.tolist()):
        assert np.array_equal(P.words(seed, offset, [q])[0], w[i])
    assert len({tuple(r) for r in w.tolist()}) == 6                  # every 64-bit counter its own words: no half dropped
    assert P.counters(2 ** 64 - 2, 4).tolist() == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]
    assert P.step_offset(2 ** 64 - 1, 16) == 15 and P.step_offset(0xFFFFFFFF, 1) == 1 << 32
    for a, b in (((seed, offset), (seed, offset + 2 ** 32)), ((123, 5), (123 + 2 ** 32, 5))):
        assert not np.array_equal(P.words(*a, [0]), P.words(*b, [0]))
    # fewer rounds, swapped multipliers: not the same function
    assert [int(x[0]) for x in P.philox4x32([0, 0, 0, 0], [0, 0], rounds=9)] != hexwords(KAT[0][2])


@pytest.mark.parametrize("counter,word,top", EDGES)
def test_edge_counters_are_what_the_gpu_tests_take_them_for(counter, word, top):
    w = P.words(EDGE_SEED, EDGE_OFFSET, [counter])[0]
    assert int(w[word]) >> 8 == top
    assert P.find_edge_counters(EDGE_SEED, EDGE_OFFSET, counter + 1, start=counter) == [(counter, word, "zero" if top == 0 else "one")]
    z = P.normal(EDGE_SEED, EDGE_OFFSET, 4 * counter, 4)
    u = P.uniform(EDGE_SEED, EDGE_OFFSET, 4, first_element=4 * counter)
    assert np.isfinite(z).all() and (u >= 0).all() and (u < 1).all()
    if word in (0, 2) and top == 0xFFFFFF:            # u = 1: radius exactly 0
        assert (z[word:word + 2] == 0).all()
    if word == 0 and top == 0:                        # u = 2^-24
        assert abs(np.hypot(z[0], z[1]) - np.sqrt(48 * np.log(2.0))) < 1e-12 and 5.768 < np.hypot(z[0], z[1]) < 5.769
    if word == 3:                                     # angle 2^-24 rev / one rev: on the positive x axis (to 4e-7 rad / exactly)
        rad = np.hypot(z[2], z[3])
        assert abs(z[2] - rad) <= 1e-12 * rad and abs(z[3]) <= 4e-7 * rad
        assert u[3] == (0.0 if top == 0 else np.float32(1 - 2.0 ** -24))


def test_uniform_and_bernoulli_maps():
    seed, offset = 991, 12
    w = P.words(seed, offset, np.arange(3, dtype=np.uint64)).reshape(-1)
    u = P.uniform(seed, offset, 10)
    assert u.dtype == np.float32 and u.shape == (10,)
    assert np.array_equal(u.astype(np.float64) * 2.0 ** 24, (w[:10] >> 8).astype(np.float64))          # exact in fp32
    assert np.array_equal(P.uniform(seed, offset, 6, first_element=4), u[4:10])
    p = np.array([0.0, 1.0, u[2], np.nextafter(u[3], np.float32(1)), 0.5], dtype=np.float32)
    b = P.bernoulli(p, 2, 5, seed, offset)
    assert b.shape == (2, 5) and b[0].tolist()[:4] == [0.0, 1.0, 0.0, 1.0] and b[1, 0] == 0 and b[1, 1] == 1
    assert np.array_equal(b, (u.reshape(2, 5) < p[None, :]).astype(np.float32))
    with pytest.raises(ValueError):
        P.normal(seed, offset, 2, 4)


def test_normal_sanity():
    n = 1 << 20
    z = P.normal(123, 1 << 63, 0, n)
    assert z.dtype == np.float64 and z.shape == (n,) and np.isfinite(z).all()
    assert abs(z.mean()) < 4 / np.sqrt(n)                       # standard error of the mean: 1 / sqrt(n)
    assert abs(z.std() - 1) < 4 / np.sqrt(2 * n)                # standard error of the standard deviation: 1 / sqrt(2 n)
    assert np.array_equal(P.normal(123, 1 << 63, 4096, 1000), z[4096:5096])
    assert np.array_equal(P.normal(123, 1 << 63, 0, 7), z[:7])
