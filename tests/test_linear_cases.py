"""tests/linear_cases.py checked on the CPU: every case of its table through the pure-PyTorch strided emulator (the harness's claims about
its own data hold - make_data asserts them - and check() passes), and check() against deliberately WRONG emulators, each of which must
trip the assertion meant for it.  This is the evidence that tests/test_linear_exact_gpu.py would catch a subtly wrong kernel; no kernel is
mutated for it."""
import functools

import pytest
import torch

import linear_cases as C
from linear_cases import Case


@pytest.mark.parametrize("k", range(len(C.TABLE)), ids=C.IDS)
def test_table_case_on_the_emulator(k):
    c, kind = C.TABLE[k]
    assert C.run_case(c, kind, backend=C.emulate, device="cpu") is None


def test_table_covers_every_path_in_every_layout():
    seen = {(c.path, c.layout) for c, _ in C.TABLE}
    for path in C._DEFAULT:
        for lay in C.LAYOUTS:
            assert (path, lay) in seen, (path, lay)
    assert set(C.KERNELS) == {("1", "1", "1", "1"), ("0", "0", "0", "0")} and all(set(t) == set(C._DEFAULT) for t in C.KERNELS.values())


def test_onehot_rows_reach_every_k_and_end_on_the_last():
    gen = torch.Generator().manual_seed(0)
    for M, Ks in ((512, (256,)), (100, (37,)), (64, (40, 12)), (8192, (100,)), (1024, (1024,))):
        Xs = C._onehot_rows(M, Ks, gen)
        assert bool(((torch.cat(Xs, 1) != 0).sum(1) == 1).all())
        assert bool((Xs[(M - 1) % len(Ks)][M - 1, -1] != 0))
        assert all(int(X.abs().sum(1).nonzero()[-1]) >= M - len(Ks) and bool(X[X.abs().sum(1).nonzero()[-1], -1] != 0) for X in Xs)
        for X, K in zip(Xs, Ks):
            if M // len(Ks) >= K:
                assert bool((X != 0).any(0).all()), (M, Ks)
        # every 32-row block spreads over the 32 chunks (of 8 k) of a 256-wide source: at least half of them
        if Ks == (256,):
            assert all(int((X[r:r + 32] != 0).any(0).view(32, 8).any(1).sum()) >= 16 for r in range(0, M, 32))


# ---- wrong kernels: (bug of the emulator, a case it shows on, what check() must say)
_FULL = dict(bias=True, rowbias=4, rowscale=True, seed=True)
WRONG = [
    ("S_with_ldY", Case(100, (37,), 70, "small", epi="dact", act="relu", q=True, layout="pad4"), "Y: .* values differ"),
    ("writes_row_M", Case(100, (37,), 70, "small", act="relu", layout="pad4", **_FULL), "Y has 7070 numbers, 7000 belong there"),
    ("writes_row_M", Case(48, (100,), 36, "b16", act="none", layout="tight"), "Y has 1764 numbers, 1728 belong there"),
    ("writes_column_Nout", Case(100, (37,), 70, "small", act="relu", layout="pad4", **_FULL), "Y has 7100 numbers, 7000 belong there"),
    ("writes_column_Nout", Case(100, (37,), 70, "small", act="relu", layout="odd", **_FULL), "Y has 7100 numbers, 7000 belong there"),
    ("rowbias_of_previous_group", Case(100, (37,), 70, "small", act="relu", layout="odd", **_FULL), "Y: .* values differ"),
    ("drops_Q", Case(352, (64,), 224, "lean", epi="dact", act="relu", q=True, inplace=True, layout="pad4"), "Y: .* values differ"),
    ("colsum_row_twice", Case(200, (256,), 256, "geo1", epi="dact", act="none", q=True, colsum=True, layout="pad4"), "colsum: .* values differ"),
    ("modifies_input", Case(100, (37,), 70, "small", act="none", layout="pad4", kinds=("int", "onehot_x")), "read-only operand X0 .* was modified"),
    ("modifies_input", Case(8192, (256,), 256, "chain", epi="dact", act="relu", nl=2, layout="pad4"), "read-only operand (X0|S) .* was modified"),
]


@pytest.mark.parametrize("bug,case,message", WRONG, ids=[f"{b}-{c.path}-{c.layout}" for b, c, _ in WRONG])
def test_check_refuses_a_wrong_kernel(bug, case, message):
    for kind in case.kinds:
        C.run_case(case, kind, backend=C.emulate, device="cpu")             # the control: the right emulator passes on this very case
        with pytest.raises(AssertionError, match=message):
            C.run_case(case, kind, backend=functools.partial(C.emulate, bug=bug), device="cpu")


def test_a_tight_store_to_column_Nout_is_a_wrong_value():
    """A tight operand has no column guards: the store lands in the next row's first element (overwritten by the right value in an
    emulator that writes Y afterwards, so here it is the LAST row's store that shows: in the guard row behind the view)."""
    c = Case(48, (100,), 36, "b16", act="none", layout="tight")
    with pytest.raises(AssertionError, match="Y has 1729 numbers, 1728 belong there"):
        C.run_case(c, "int", backend=functools.partial(C.emulate, bug="writes_column_Nout"), device="cpu")


def test_geometry_restates_the_library():
    """geometry() / row_tile() / col_panels() restate linear.hip::pick_geometry; the GPU tests compare them with the library's answers
    (tests/test_linear_exact_gpu.py::test_tile_counts_match_the_library).  Here: the values the table relies on."""
    assert [C.geometry(*s) for s in ((16500, 20), (300, 8), (200, 256), (8200, 256), (2048, 512), (8192, 128), (1024, 1024), (8192, 96))] == \
        [0, 0, 1, 2, 1, 2, 1, 2]
    assert C.row_tile(2048, 512) == 32 and C.col_panels(2048, 512) == 4 and C.col_panels(384, 32) == 1
