"""`ardae_wgrad_batch` held to EXACT results at the slice, tile and dispatch edges of its five kernels (wgrad_x9_kernel, wgrad_wide_kernel
<256x32> and <256x256>, wgrad_kernel, wgrad_small_kernel) and of wgrad_reduce_kernel.  tests/wgrad_cases.py has the two harnesses - dense
small integers (every row counted exactly once) and one-hot selection (every lane, plane and fragment in its place) - and the table of
the kernel each case must run on; no comparison in this file has a tolerance.

Slices: a tiled launch runs splits = min(256 / tiles in the launch, smallest p.splits) workgroups per tile, each over cps = ceil(chunks /
splits) chunks of the concatenated (pair, row) range - 16-row chunks on wgrad_x9_kernel, 32-row chunks on wgrad_wide_kernel.  The cps
values quoted below are wgrad_x9_kernel's; with ARDAE_WGRAD_X9=0 the same cases run on wgrad_wide_kernel<256x256> at half the chunks."""
import os
import subprocess
import sys

import pytest
import torch

from ardae_amd import _lib as L
from wgrad_cases import Case, knob_env, launch, make_inputs, run_exact

pytestmark = pytest.mark.gpu

DATA = ["int", "onehot_g", "onehot_x"]
BETAS = [0.0, 1.0, -2.0, 0.5]


# ---- wgrad_x9_kernel: prologue, the trip that re-loads two chunks ahead, its compile-time vmcnt counts, empty slices
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("splits,beta", [(256, 0.0), (64, 1.0), (43, -2.0), (0, 0.5)])
def test_x9_short_slices(splits, beta, data):
    """M = 2048 (the kernel's minimum: 128 chunks), one 256 x 256 tile: splits 256 -> cps 1 and 128 EMPTY slices (zero partials), 64 -> cps 2,
    43 -> cps 3 with a short last slice, ardae_wgrad_splits (32) -> cps 4."""
    if splits == 0:
        assert L.lib().ardae_wgrad_splits(2048, 256, 256, 1) == 32
    names = run_exact([Case(2048, 256, 256, "x9", bias_pair=0, rowscale=True, splits=splits, beta=beta)], data, seed=splits)
    if knob_env() == ("1", "1", "1"):
        assert names == {"wgrad_x9_kernel<256x256>"}


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("bias_pair,rowscale,phase", [(0, False, 0), (0, True, 1), (1, False, 1), (1, True, 0)])
def test_x9_slice_straddles_the_pair_boundary(bias_pair, rowscale, phase, data):
    """Two pairs of 2048 rows, splits 51: cps 6, slice 21 covers chunks 126 .. 131 across the pair boundary at 128 - the bias and sigma sums
    switch on or off inside the slice (bias_pair 0 / 1), the leading dimensions change with the pair (ldG 256 / 260, ldX 256 / 264)."""
    run_exact([Case(2048, 256, 256, "x9", npairs=2, bias_pair=bias_pair, rowscale=rowscale, splits=51, ldG=(256, 260), ldX=(256, 264),
                    beta=BETAS[phase + 2 * rowscale], phase=phase)], data, seed=10 + bias_pair)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("O,I", [(512, 256), (256, 512)])
def test_x9_tiles_off_the_origin(O, I, data):
    """M = 2080 (130 chunks).  512 x 256: the second o-tile's bias and sigma partials land at o0 = 256; 256 x 512: the i0 = 256 tile must
    write none."""
    run_exact([Case(2080, O, I, "x9", npairs=2, bias_pair=1, rowscale=True, beta=1.0)], data, seed=O)


@pytest.mark.parametrize("data", DATA)
def test_mixed_launch_and_mixed_batch(data):
    """Two square problems with different M (2048, 2560) and npairs in ONE tiled launch (cps 4 and 10 from the same split count), beside a
    256 x 32 problem, a generic one and a per-image one in the same batch; every split count from ardae_wgrad_splits."""
    run_exact([Case(2048, 256, 256, "x9", bias_pair=0, beta=-2.0), Case(2560, 256, 256, "x9", npairs=2, bias_pair=0, rowscale=True),
               Case(2048, 256, 32, "narrow", npairs=2, bias_pair=1, rowscale=True, beta=0.5), Case(1030, 96, 130, "generic", bias_pair=0, beta=1.0),
               Case(64, 80, 70, "small", npairs=2, bias_pair=0, rowscale=True)], data, seed=20)


def test_x9_at_the_recipes_rows():
    """M = 80000 = 128 x 625 rows (the shipped recipes' batch), two pairs, bias and sigma column: the largest sums of this file, 2 x 80000 x 12
    = 1.92e6 < 2^24."""
    run_exact([Case(80000, 256, 256, "x9", npairs=2, bias_pair=1, rowscale=True, beta=1.0)], "int", seed=21)


def test_x9_needs_sigma_on_a_16_byte_boundary():
    """wgrad_x9_kernel reads sigma four rows at a time (global_load_dwordx4): wgrad_x9_eligible refuses a rowscale off a 16-byte boundary, and
    the problem runs on wgrad_wide_kernel<256x256>, which reads it dword by dword.  (This test exists only together with that gate.)"""
    for data in ("int", "onehot_g"):
        names = run_exact([Case(2048, 256, 256, "square_fp32", bias_pair=0, rowscale=True, rowscale_off=1, beta=1.0)], data, seed=22)
        assert not any(n.startswith("wgrad_x9") for n in names), names


# ---- wgrad_wide_kernel<256x32>
@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("splits", [256, 32, 22])
def test_narrow_geometry_slices_and_tiles(splits, data):
    """M = 2048 = 64 chunks of 32 rows; I = 64 is two i-tiles per o-tile, of which only the first (i0 == 0) writes the bias partials.  splits 256
    -> cps 1 (with empty slices while the problem has fewer than four tiles), 32 -> cps 2, 22 -> cps 3 with a one-chunk last slice."""
    for k, (O, I) in enumerate([(256, 32), (256, 64), (512, 32), (512, 64)]):
        run_exact([Case(2048, O, I, "narrow", bias_pair=0, rowscale=k % 2 == 1, splits=splits, beta=BETAS[k])], data, seed=30 + k)


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("bias_pair", [0, 1])
def test_narrow_slice_straddles_the_pair_boundary(bias_pair, data):
    """Two pairs of 64 chunks, splits 22: cps 6, slice 10 covers chunks 60 .. 65 across the boundary at 64; ldX differs between the pairs."""
    run_exact([Case(2048, 256, 64, "narrow", npairs=2, bias_pair=bias_pair, rowscale=True, splits=22, ldG=(256, 260), ldX=(64, 72), phase=bias_pair)],
              data, seed=35)


# ---- wgrad_kernel
GENERIC = {
    "first_M_one_row_split": Case(1025, 129, 257, "generic", bias_pair=0, rowscale=True),            # 17 splits of 64 rows: the last has one row;
                                                                                                      # one-row and one-column edge tiles
    "vector_loads_ragged_tail": Case(1025, 98, 130, "generic", npairs=2, bias_pair=1, rowscale=True, ldG=(100, 100), ldX=(132, 132), beta=1.0),
    "scalar_reduce": Case(1030, 3, 5, "generic", npairs=2, bias_pair=0, rowscale=True, beta=-2.0),
    "two_columns": Case(2048, 256, 2, "generic", bias_pair=0, beta=0.5),
    "three_i_blocks": Case(2048, 256, 96, "generic", npairs=2, bias_pair=0, rowscale=True),
    "rows_off_the_tiled_kernels": Case(2064, 256, 256, "generic", bias_pair=0, rowscale=True, beta=1.0),   # M % 32 != 0
    "partial_off_16_bytes": Case(1025, 98, 130, "generic", bias_pair=0, partial_off=1, beta=1.0),           # O I % 4 == 0, scalar reduce all the same
}


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("name", list(GENERIC))
def test_generic_kernel_edges(name, data):
    names = run_exact([GENERIC[name]], data, seed=40)
    assert names == {"wgrad_kernel"}       # in every knob environment: none of these shapes may reach a tiled or the per-image kernel


# ---- wgrad_small_kernel: odd M, M below one register batch, O and I below / just over the 32-wide wave tiles and 64-wide workgroup tiles,
# ---- M = 1024 (the last on this kernel; 1025 is GENERIC's first case)
SMALL = [Case(1, 1, 1, "small", bias_pair=0, rowscale=True), Case(1, 65, 63, "small", npairs=2, bias_pair=1, splits=2, beta=1.0),
         Case(2, 31, 33, "small", bias_pair=0, beta=-2.0), Case(2, 256, 256, "small", npairs=2, bias_pair=0, rowscale=True),
         Case(3, 33, 2, "small", npairs=2, bias_pair=1, rowscale=True, splits=2, beta=0.5), Case(3, 65, 63, "small"),
         Case(17, 31, 33, "small", npairs=2, bias_pair=0, rowscale=True, splits=3, ldG=(31, 36), ldX=(35, 33), beta=1.0),
         Case(17, 256, 256, "small", bias_pair=0), Case(64, 65, 63, "small", npairs=2, bias_pair=1, rowscale=True, beta=-2.0),
         Case(64, 1, 1, "small", bias_pair=0, rowscale=True, splits=5), Case(1023, 33, 2, "small", bias_pair=0, rowscale=True, beta=0.5),
         Case(1023, 256, 256, "small", npairs=2, bias_pair=1, rowscale=True), Case(1024, 31, 33, "small", npairs=2, bias_pair=0, splits=7, beta=1.0),
         Case(1024, 65, 63, "small", bias_pair=0, rowscale=True)]


@pytest.mark.parametrize("data", DATA)
@pytest.mark.parametrize("k", range(len(SMALL)), ids=[f"{c.M}x{c.O}x{c.I}" for c in SMALL])
def test_small_kernel_rows_and_tiles(k, data):
    run_exact([SMALL[k]], data, seed=50 + k)


# ---- wgrad_reduce_kernel: the four-group split walk (sp = sg; sp + 12 < S; sp += 16, then the tails) on the float4 and the scalar path
@pytest.mark.parametrize("data", ["int", "onehot_g"])
@pytest.mark.parametrize("splits", [1, 2, 3, 4, 5, 13, 16, 17, 29])
def test_reduce_split_walk(splits, data):
    """464 rows: every one of up to 29 splits has rows on the per-image kernel.  8 x 12: float4 path; 7 x 9: O I % 4 != 0, scalar path; 8 x 12 with
    `partial` four bytes off a 16-byte boundary: scalar path."""
    for k, (O, I, off) in enumerate([(8, 12, 0), (7, 9, 0), (8, 12, 1)]):
        run_exact([Case(464, O, I, "small", npairs=2, bias_pair=1, rowscale=True, splits=splits, partial_off=off, beta=BETAS[(splits + k) % 4])],
                  data, seed=60 + k)


# ---- a full batch
def _twenty():
    return [Case(3 + 5 * k, 5 + 3 * k, 70 - 3 * k, "small", npairs=1 + k % 2, bias_pair=k % 2, rowscale=k % 3 == 0, beta=BETAS[k % 4]) for k in range(20)]


@pytest.mark.parametrize("data", ["int", "onehot_g"])
def test_full_batch_of_twenty(data):
    """ARDAE_WGRAD_MAX_PROBLEMS = 20 problems (the kernels' whole argument block) in one call, every one exact."""
    assert L.CONSTANTS["ARDAE_WGRAD_MAX_PROBLEMS"] == 20
    run_exact(_twenty(), data, seed=70)


def test_batch_of_twenty_one_is_refused_before_any_launch():
    gen = torch.Generator(device="cuda").manual_seed(71)
    inputs = [make_inputs(Case(8 + k, 8, 8, "small", bias_pair=0), "int", gen) for k in range(21)]
    written = []
    with pytest.raises(ValueError):
        launch(inputs, stash=written)
    assert L.profile_report(max_entries=64) == []                      # no kernel was logged (the log outlives launch()'s switch-off) ...
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in written)            # ... and no output or scratch buffer was touched


# ---- the fixed-order reduction: "reproducible"
def test_three_launches_are_bit_identical():
    """Gaussian data, one batch over four kernels (x9 with two pairs at M = 16384, 256 x 32, generic, per-image), three launches into fresh
    buffers: every output bit for bit the same."""
    cases = [Case(16384, 256, 256, "x9", npairs=2, bias_pair=1, rowscale=True), Case(16384, 256, 32, "narrow", npairs=2, bias_pair=0),
             Case(3000, 96, 130, "generic", npairs=2, bias_pair=1, rowscale=True), Case(600, 80, 70, "small", bias_pair=0, rowscale=True)]
    gen = torch.Generator(device="cuda").manual_seed(80)
    inputs = [make_inputs(c, "gauss", gen) for c in cases]
    runs = [launch(inputs)[1] for _ in range(3)]
    for again in runs[1:]:
        for first, second in zip(runs[0], again):
            for a, b in zip(first, second):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))      # (bit patterns: the NaN guards compare equal too)
    for out, ob, ors in runs[0]:
        assert not torch.isnan(out[1:-1, 1:-2]).any() and not torch.isnan(ob[1:-1]).any()


# ---- the kernels only a knob reaches, under the same cases
@pytest.mark.parametrize("knobs", [dict(ARDAE_WGRAD_X9="0"), dict(ARDAE_WGRAD_WIDE="0", ARDAE_WGRAD_SMALL="0")], ids=["x9_off", "generic_only"])
def test_knob_only_kernels_under_the_same_cases(knobs):
    """The library reads its knobs once per process: this file again, in a fresh child process, with ARDAE_WGRAD_X9=0 (the square cases on
    wgrad_wide_kernel<256x256>, 32-row chunks) and with ARDAE_WGRAD_WIDE=0 ARDAE_WGRAD_SMALL=0 (everything on wgrad_kernel).  The
    expected-kernel tables of wgrad_cases.py keep the name assertions meaningful there."""
    env = dict(os.environ, ARDAE_DEBUG_KNOBS="1", **knobs)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not knob_only"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
