"""`ardae_linear`, `ardae_linear_chain` and `ardae_linear_wide_layers` on every kernel path behind them - linear_kernel's three geometries, the
three per-image blocks, linear_narrow_kernel, linear_shortk_kernel, linear_wide_kernel for K = 32 / 256 / 512 / 1024, linear_chain_kernel and
linear_wide_layers_kernel - with strided operands in NaN-guarded buffers (tests/linear_cases.py has the harness, the case table and the
table of the kernel each case must run on).  "int" and "onehot_x" comparisons are torch.equal; "gauss" ones (softplus, CHAIN) use the
2e-5 of tests/test_linear_gpu.py plus bit equality with the tight twin / the per-layer launches.  Every case asserts the kernel that ran,
intact guards around every output and bit-identical read-only operands.

The pair forms (linear_small*_pair_kernel) are not here: no entry point of the C ABI launches them on caller-made arguments - only the
engines' cDAE passes do (launch_linear_pair) - so they stay with tests/test_cdae_gpu.py.  tests/test_linear_cases.py shows on the CPU that
this harness refuses wrong kernels."""
import os
import subprocess
import sys

import pytest

import linear_cases as C
from ardae_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", range(len(C.TABLE)), ids=C.IDS)
def test_case(k):
    c, kind = C.TABLE[k]
    C.run_case(c, kind)


def test_tile_counts_match_the_library():
    """colsum and tile_loss are sized by the harness's restatement of linear.hip::pick_geometry."""
    lib = L.lib()
    for M, N in sorted({(c.M, c.Nout) for c, _ in C.TABLE}):
        assert lib.ardae_linear_row_tiles(M, N) == -(-M // C.row_tile(M, N)), (M, N)
        assert lib.ardae_linear_col_panels(M, N) == C.col_panels(M, N), (M, N)


def test_default_environment_reaches_all_eleven_kernels():
    """In the default environment the table's name assertions cover every kernel of the issue's list (a knob environment is the child
    process of the last test, which meets linear_kernel's geometries instead)."""
    if C.knob_env() != ("1", "1", "1", "1"):
        return
    heads = {C.kernel_of(c) for c, _ in C.TABLE}
    assert len(heads) >= 14 + 2        # 12 single-launch paths, chain x2 / x3, wide layers x2 / x3


def test_profile_costs_of_the_engine_launches():
    """The launchers that ardae_linear does not reach - the small chain (the 64-row cDAE score pass at one row per image), the per-image
    pair (the same 64 rows at two rows per image: that pass is not chained), the sampler tail behind the short-K layer (forward_hidden on
    8192 rows) - report the (name, calls, flops, bytes) recorded from the commit before the cost model was written once; exact, like
    every case of the table."""
    if C.knob_env() != ("1", "1", "1", "1"):
        return
    reached = set()
    for scene, run in sorted(C.SCENES.items()):
        got, want = run(), C.recorded_costs()["scenes"][scene]
        assert got == want, f"{scene}: the profile log reports {got}, recorded {want}"
        reached |= {name.split("<")[0].split(" ")[0] for name, *_ in got}
    assert {"linear_small_pair_kernel", "linear_small_chain_kernel"} <= reached and any(n.startswith("sampler_tail") for n in reached), reached


def test_knob_only_generic_kernel_under_the_same_cases():
    """The library reads its knobs once per process: this file again in a fresh child process with the per-image, narrow, short-K and wide
    kernels switched off - every single launch on linear_kernel, in the geometry the table of linear_cases.py expects."""
    env = dict(os.environ, ARDAE_DEBUG_KNOBS="1", ARDAE_SMALL="0", ARDAE_NARROW="0", ARDAE_SHORTK="0", ARDAE_WIDE="0")
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "not knob_only"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
