"""ardae_hist2d_wide on the device: tables wider than one workgroup's LDS, cut into bands of x-bin rows.  Every comparison is EXACT against
np.histogram2d(..., range=[[lo, hi]] * 2, bins=bins): there are no tolerances.  129 bins is the first table with two bands (127 + 2 rows), 257 does
not divide into equal bands (4 x 63 + 5 rows), 512 has the most (16 x 32 rows); 128 and 5 are one band, where the result must also be ardae_hist2d's."""
import numpy as np
import pytest
import torch

from ardae_amd import _lib as L

pytestmark = pytest.mark.gpu

RANGES = [(-4.0, 4.0, 256), (-6.0, 6.0, 256), (-4.0, 4.0, 129), (-3.0, 3.0, 257), (-6.0, 6.0, 512), (-4.0, 4.0, 128), (-4.0, 4.0, 5)]
BAND_CELLS = 16384                                                              # csrc/diag.hip: HIST_BAND_CELLS


def _hist(pts, n, row_stride, nslots, slot_stride, cx, cy, lo, hi, bins, counts=None, entry="ardae_hist2d_wide"):
    if counts is None:
        counts = torch.zeros(nslots, bins, bins, dtype=torch.int64, device="cuda")
    L.call(entry, pts, n, row_stride, nslots, slot_stride, cx, cy, lo, hi, bins, counts)
    return counts


def _numpy(x, y, lo, hi, bins):
    return np.histogram2d(x, y, range=[[lo, hi], [lo, hi]], bins=bins)[0].astype(np.int64)


def _normals(n, lo, hi, seed):
    g = np.random.default_rng(seed)
    return (g.standard_normal((n, 2)) * (hi - lo) / 5).astype(np.float32)       # a few per cent fall outside the range


def _crafted(lo, hi, bins):
    """Every edge as float32 and its two float32 neighbours, the range's ends from both sides, +-inf, NaN - on either axis (tests/test_diagnostics_gpu.py):
    points on both sides of every band boundary, and in x bins 0 and bins - 1."""
    e = np.linspace(lo, hi, bins + 1).astype(np.float32)
    inf32 = np.float32(np.inf)
    v = np.concatenate([e, np.nextafter(e, -inf32), np.nextafter(e, inf32),
                        np.array([lo, hi, -lo, -hi, -1e-30, 1e-30, 0.0, -0.0, -1.8, 0.6, 1.8, -0.6, np.inf, -np.inf, np.nan], dtype=np.float32)])
    inside = np.full_like(v, np.float32(0.1))
    return np.concatenate([np.stack([v, v], 1), np.stack([v, inside], 1), np.stack([inside, v], 1), np.stack([v, v[::-1]], 1)])


_POINTS = {}


def _case(lo, hi, bins, case):
    """float32 points [n, 2] of a case, built once and left unchanged."""
    key = (lo, hi, bins, case)
    if key not in _POINTS:
        if case == "crafted":
            p = np.concatenate([_normals(1000, lo, hi, 1), _crafted(lo, hi, bins)])
        elif case == "contention":
            p = np.tile(np.array([[0.3, -1.1]], dtype=np.float32), (50000, 1))   # one cell takes every add
        elif case == "dropped":
            p = _normals(3000, lo, hi, 2)
            g = np.random.default_rng(3)
            bad = np.array([np.nan, np.inf, -np.inf, 2 * hi, 2 * lo, np.nextafter(np.float32(hi), np.float32(np.inf)),
                            np.nextafter(np.float32(lo), -np.float32(np.inf))], dtype=np.float32)
            rows = g.choice(len(p), 900, replace=False)
            p[rows, g.integers(0, 2, 900)] = bad[g.integers(0, len(bad), 900)]
        else:
            p = _normals(case, lo, hi, case)
        _POINTS[key] = np.ascontiguousarray(p)
    return _POINTS[key]


@pytest.mark.parametrize("case", [1, "crafted", 70001, "contention", "dropped"])
@pytest.mark.parametrize("lo,hi,bins", RANGES)
def test_hist2d_wide_equals_numpy(lo, hi, bins, case):
    p = _case(lo, hi, bins, case)
    want = _numpy(p[:, 0], p[:, 1], lo, hi, bins)
    dev = torch.from_numpy(p).cuda()
    got = _hist(dev, len(p), 2, 1, 0, 0, 1, lo, hi, bins)[0].cpu().numpy()
    print(f"({lo}, {hi}, {bins}) {case}: {len(p)} points, {int(want.sum())} counted, {int((got != want).sum())} bins differ")
    assert np.array_equal(got, want)
    if case == "contention":
        assert got.max() == 50000 and (got != 0).sum() == 1
    if case == "dropped":
        assert 0 < want.sum() < len(p) - 600                                    # the bad values were dropped, point by point
    if case == "crafted":                                                       # the set does what it is for: both sides of every band boundary
        rows = min(bins, BAND_CELLS // bins)
        assert want[0].sum() > 0 and want[bins - 1].sum() > 0
        assert all(want[r - 1].sum() > 0 and want[r].sum() > 0 for r in range(rows, bins, rows))
    if bins <= 128:                                                             # one band: ardae_hist2d's table
        assert torch.equal(_hist(dev, len(p), 2, 1, 0, 0, 1, lo, hi, bins, entry="ardae_hist2d")[0].cpu(), torch.from_numpy(got))


@pytest.mark.parametrize("lo,hi,bins", RANGES)
def test_hist2d_wide_strided_layouts_and_slots(lo, hi, bins):
    n = 1000
    g = np.random.default_rng(7)
    # rows of 32 floats, the pair in columns 5 and 2
    rows = (g.standard_normal((n, 32)) * (hi - lo) / 5).astype(np.float32)
    dev = torch.from_numpy(rows).cuda()
    assert np.array_equal(_hist(dev, n, 32, 1, 0, 5, 2, lo, hi, bins)[0].cpu().numpy(), _numpy(rows[:, 5], rows[:, 2], lo, hi, bins))
    # five slots side by side in a row, [n, 5, zd], written into the middle of a buffer whose neighbouring slabs hold a sentinel
    zd = 2
    z = (g.standard_normal((n, 5, zd)) * (hi - lo) / 5 * np.array([1, .8, .5, .1, .01]).reshape(1, 5, 1)).astype(np.float32)
    guard = torch.full((7, bins, bins), 7, dtype=torch.int64, device="cuda")
    guard[1:6] = 0
    _hist(torch.from_numpy(z).cuda(), n, 5 * zd, 5, zd, 0, 1, lo, hi, bins, guard[1:6])
    got = guard.cpu().numpy()
    assert (got[0] == 7).all() and (got[6] == 7).all()                          # counts outside the addressed slots are untouched
    for s in range(5):
        assert np.array_equal(got[1 + s], _numpy(z[:, s, 0], z[:, s, 1], lo, hi, bins)), s
    # slot-major blocks [5, n, zd]
    zt = np.ascontiguousarray(z.transpose(1, 0, 2))
    assert torch.equal(_hist(torch.from_numpy(zt).cuda(), n, zd, 5, n * zd, 0, 1, lo, hi, bins), guard[1:6])


@pytest.mark.parametrize("lo,hi,bins", RANGES)
def test_hist2d_wide_adds_two_halves_like_one_whole(lo, hi, bins):
    p = _case(lo, hi, bins, 70001)
    dev = torch.from_numpy(p).cuda()
    whole = _hist(dev, len(p), 2, 1, 0, 0, 1, lo, hi, bins)
    h = 35001
    halves = _hist(dev, h, 2, 1, 0, 0, 1, lo, hi, bins)
    _hist(dev[h:], len(p) - h, 2, 1, 0, 0, 1, lo, hi, bins, halves)
    assert torch.equal(whole, halves)
    assert torch.equal(_hist(dev, len(p), 2, 1, 0, 0, 1, lo, hi, bins, whole.clone()), 2 * whole)       # it ADDS
