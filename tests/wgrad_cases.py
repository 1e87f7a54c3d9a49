"""Two EXACT harnesses for `ardae_wgrad_batch` (tests/test_wgrad_exact_gpu.py): data for which dW, the bias sums and the sigma column have
one representable value whatever the order of the additions, so every comparison is torch.equal - no tolerance.

  "int"       dense small integers: G in [-3, 3], X in [-4, 4], rowscale in [-2, 2], prefills |v| <= 1000 (even where beta = 0.5).  Every partial
              sum, in any order, is an integer below 2^24 (asserted here), so each row must be counted exactly once.
  "onehot_g"  G has ONE non-zero per column o, +-2^k (k in [-2, 2]) at row r(o); X is arbitrary fp32 with full significands,
              +-(1 + j 2^-23) 10^e, zeros sprinkled in: dW[o, :] = +-2^k X[r(o), :] bit for bit, bias = +-2^k, sigma sum = +-2^k rowscale[r(o)].
              Every other term of a sum is an exact zero and any subset sum of one value's three bf16 pieces is representable: exact on
              wgrad_x9_kernel too, for any product order, and all three planes of its cut carry bits.
  "onehot_x"  the mirror image: X selects one row per column i, G carries the full significands (bias sums are not exact: no bias_pair).
r(.) walks the 8-row k groups of the concatenated (pair, row) range evenly and ends on its last row: with M = 2048 and 256 columns every
slice, chunk and k group carries a non-zero (`phase` shifts the walk where a problem has more k groups than columns: two pairs).

Both fill `partial` / `partial_vec` and the padding columns of G and X with NaN, put NaN guard rows and columns around out, out_bias and
out_rowscale, and assert through the profile log that the kernels the cases are meant for are the ones that ran."""
from dataclasses import dataclass

import torch

from ardae_amd import _lib as L

NAN = float("nan")

_X9, _SQ, _NR, _SM, _GEN = ("wgrad_x9_kernel<256x256>", "wgrad_wide_kernel<256x256>", "wgrad_wide_kernel<256x32>", "wgrad_small_kernel",
                            "wgrad_kernel")
_KNOBS = ("ARDAE_WGRAD_X9", "ARDAE_WGRAD_WIDE", "ARDAE_WGRAD_SMALL")
# what a case's `path` runs on, by knob environment (the three switches above under ARDAE_DEBUG_KNOBS=1; "1" = on, the default).
#   x9: square tiles x9 can take;  square_fp32: square tiles it cannot (sigma off a 16-byte boundary);  narrow: 256 x 32 tiles;
#   small: M <= 1024;  generic: everything else
KERNELS = {
    ("1", "1", "1"): dict(x9=_X9, square_fp32=_SQ, narrow=_NR, small=_SM, generic=_GEN),
    ("0", "1", "1"): dict(x9=_SQ, square_fp32=_SQ, narrow=_NR, small=_SM, generic=_GEN),
    ("1", "0", "0"): dict(x9=_GEN, square_fp32=_GEN, narrow=_GEN, small=_GEN, generic=_GEN),
}


def knob_env():
    return tuple("0" if int(L.debug_knob(n, "1")) == 0 else "1" for n in _KNOBS)


def kernel_of(path):
    env = knob_env()
    assert env in KERNELS, f"no expected-kernel table for {dict(zip(_KNOBS, env))}"
    return KERNELS[env][path]


@dataclass
class Case:
    M: int
    O: int
    I: int
    path: str                  # key of the KERNELS tables
    npairs: int = 1
    bias_pair: int = -1        # >= 0: out_bias is asked for
    rowscale: bool = False     # with bias_pair >= 0: sigma and out_rowscale as well
    splits: int = 0            # 0: ardae_wgrad_splits(M, O, I, problems in the batch)
    ldG: tuple = ()            # per pair; default O
    ldX: tuple = ()            # per pair; default I
    beta: float = 0.0
    partial_off: int = 0       # floats between a 16-byte boundary and `partial`
    rowscale_off: int = 0      # ... and `rowscale`
    phase: int = 0             # one-hot harnesses: shift of the k-group walk


def _cuda(*shape, fill=NAN):
    return torch.full(shape, fill, device="cuda")


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=gen).float()


def _full_significands(shape, gen, emax, zeros=0.05):
    """+-(1 + j 2^-23) 10^e, j in [1, 2^23), e in [-emax, emax], rounded to fp32 once; a fraction `zeros` of exact zeros.  On the
    generator's device (tests/linear_cases.py draws on the CPU)."""
    dev = gen.device
    j = torch.randint(1, 1 << 23, shape, device=dev, generator=gen).double()
    e = torch.randint(-emax, emax + 1, shape, device=dev, generator=gen).double()
    s = torch.randint(0, 2, shape, device=dev, generator=gen).double() * 2 - 1
    v = (s * (1 + j * 2.0 ** -23) * torch.pow(torch.tensor(10.0, dtype=torch.float64, device=dev), e)).float()
    v[torch.rand(shape, device=dev, generator=gen) < zeros] = 0.0
    return v


def _onehot(total, ncols, phase, gen):
    """[total, ncols] with one non-zero +-2^k per column; column c sits in k group (c groups / ncols + phase) mod groups, at row c % 8 of
    it - the last column on the very last row."""
    groups = (total + 7) // 8
    c = torch.arange(ncols, device="cuda")
    rows = torch.clamp(8 * ((c * groups // ncols + phase) % groups) + c % 8, max=total - 1)
    rows[-1] = total - 1
    pow2 = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0], device="cuda")[torch.randint(0, 5, (ncols,), device="cuda", generator=gen)]
    sign = torch.randint(0, 2, (ncols,), device="cuda", generator=gen).float() * 2 - 1
    m = torch.zeros(total, ncols, device="cuda")
    m[rows, c] = sign * pow2
    return m


def _padded(mat, ld):
    """`mat` [M, n] as the leading columns of a [M, ld] buffer whose other columns are NaN; -> (buffer, view)."""
    buf = _cuda(mat.shape[0], ld)
    buf[:, :mat.shape[1]] = mat
    return buf, buf[:, :mat.shape[1]]


def make_inputs(c, data, gen):
    M, O, I, n = c.M, c.O, c.I, c.npairs
    bias_pair = -1 if data == "onehot_x" else c.bias_pair
    if data == "int":
        assert n * M * 12 + 2000 < 2 ** 24       # |G X| <= 12 per row (sigma G: 6), |beta prefill| <= 2000: any partial sum is an exact integer
        G, X, sig = _ints((n * M, O), -3, 3, gen), _ints((n * M, I), -4, 4, gen), _ints((M,), -2, 2, gen)
        pre = lambda *shape: _ints(shape, -500, 500, gen) * 2 if c.beta == 0.5 else _ints(shape, -1000, 1000, gen)
    elif data == "gauss":
        G, X = (torch.randn(n * M, k, device="cuda", generator=gen) for k in (O, I))
        sig, pre = torch.randn(M, device="cuda", generator=gen), None
        assert c.beta == 0.0
    else:
        if data == "onehot_g":
            G, X = _onehot(n * M, O, c.phase, gen), _full_significands((n * M, I), gen, 18)
        else:
            G, X = _full_significands((n * M, O), gen, 18), _onehot(n * M, I, c.phase, gen)
        sig = _full_significands((M,), gen, 3)
        pre = lambda *shape: _full_significands(shape, gen, 6)
    ldG, ldX = c.ldG or (O,) * n, c.ldX or (I,) * n
    inp = dict(case=c, data=data, bias_pair=bias_pair, ldG=ldG, ldX=ldX,
               G=[_padded(G[q * M:(q + 1) * M], ldG[q]) for q in range(n)], X=[_padded(X[q * M:(q + 1) * M], ldX[q]) for q in range(n)])
    sbuf = _cuda(M + c.rowscale_off)
    sbuf[c.rowscale_off:] = sig
    inp["sig"] = sbuf[c.rowscale_off:] if (c.rowscale and bias_pair >= 0) else None
    inp["sig_buf"] = sbuf
    if c.beta != 0.0:
        inp["pre"] = (pre(O, I), pre(O), pre(O))
    return inp


def launch(inputs, stash=None):
    """One ardae_wgrad_batch call into FRESH scratch (NaN) and outputs (NaN guards; the prefill where beta != 0); asserts that the kernels
    of the cases' paths, and no others, ran.  `stash`: a list that receives every buffer the call may write, before the call.
    -> (kernel names of the profile log, [(out buffer, bias buffer, sigma-column buffer)])"""
    lib = L.lib()
    probs = (L.WgradProblem * len(inputs))()
    bufs, keep = [], []
    for p, inp in zip(probs, inputs):
        c = inp["case"]
        M, O, I = c.M, c.O, c.I
        p.M, p.O, p.I, p.npairs = M, O, I, c.npairs
        for q in range(c.npairs):
            p.G[q], p.ldG[q], p.X[q], p.ldX[q] = inp["G"][q][1].data_ptr(), inp["ldG"][q], inp["X"][q][1].data_ptr(), inp["ldX"][q]
        p.bias_pair = inp["bias_pair"]
        p.rowscale = inp["sig"].data_ptr() if inp["sig"] is not None else None
        p.splits = c.splits or lib.ardae_wgrad_splits(M, O, I, len(inputs))
        part = _cuda(p.splits * O * I + 4)
        assert part.data_ptr() % 16 == 0
        pvec = _cuda(p.splits * 2 * O)
        p.partial, p.partial_vec = part[c.partial_off:].data_ptr(), pvec.data_ptr()
        # the [O, I] view sits at row 1, column 1 of `out`, the [O] bias at element 1, the sigma column at rows 1.., column 2 of 5
        out, ob, ors = _cuda(O + 2, I + 3), _cuda(O + 2), _cuda(O + 2, 5)
        if c.beta != 0.0:      # (only what the call is asked to write: the other buffers stay NaN throughout)
            out[1:O + 1, 1:I + 1] = inp["pre"][0]
            if p.bias_pair >= 0:
                ob[1:O + 1] = inp["pre"][1]
            if inp["sig"] is not None:
                ors[1:O + 1, 2] = inp["pre"][2]
        p.out, p.ldout = out[1:, 1:].data_ptr(), I + 3
        p.out_bias = ob[1:].data_ptr() if p.bias_pair >= 0 else None
        p.out_rowscale, p.ld_rowscale = (ors[1:, 2:].data_ptr(), 5) if inp["sig"] is not None else (None, 0)
        p.beta = c.beta
        bufs.append((out, ob, ors))
        keep += [part, pvec]
    if stash is not None:
        stash += keep + [t for b in bufs for t in b]
    lib.ardae_profile_enable(1)
    try:
        L.check(lib.ardae_wgrad_batch(probs, len(inputs), L.stream_ptr()), "ardae_wgrad_batch")
        names = {e["name"] for e in L.profile_report(max_entries=64)}
    finally:
        lib.ardae_profile_enable(0)
    want = {kernel_of(inp["case"].path) for inp in inputs}
    assert names == want, (sorted(names), sorted(want), knob_env())
    return names, bufs


def _same(got, want, what):
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        where = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ; first at {where[:4].tolist()}, last at "
                             f"{where[-1].tolist()}: got {got[bad][:4].tolist()}, want {want[bad][:4].tolist()}")


def _exact32(t64, what):
    """A float64 reference as fp32, after asserting that the conversion changes nothing (the harness's claim about its own data)."""
    t32 = t64.float()
    assert torch.equal(t32.double(), t64), f"{what}: the reference is not representable in fp32 - the harness's data is wrong"
    return t32


def check(inputs, bufs):
    for k, (inp, (out, ob, ors)) in enumerate(zip(inputs, bufs)):
        c = inp["case"]
        O, I, bp, tag = c.O, c.I, inp["bias_pair"], f"problem {k} {c}"
        G = [g.double() for _, g in inp["G"]]
        dW = _exact32(sum(G[q].T @ inp["X"][q][1].double() for q in range(c.npairs)), tag + " dW")
        bias = _exact32(G[bp].sum(0), tag + " bias") if bp >= 0 else None
        rsum = _exact32((inp["sig"].double()[:, None] * G[bp]).sum(0), tag + " sigma column") if inp["sig"] is not None else None
        if c.beta != 0.0:      # beta is a power of two (or 1): beta * prefill is exact and one rounding is left, fused or not
            dW = inp["pre"][0] * c.beta + dW
            bias = inp["pre"][1] * c.beta + bias if bias is not None else None
            rsum = inp["pre"][2] * c.beta + rsum if rsum is not None else None
        if inp["data"] == "int":
            for ref in (dW, bias, rsum):
                assert ref is None or float(ref.abs().max()) < 2 ** 24
        _same(out[1:O + 1, 1:I + 1], dW, tag + " dW")
        assert int(torch.isnan(out).sum()) == out.numel() - O * I, tag + ": written outside the [O, I] view"
        if bias is not None:
            _same(ob[1:O + 1], bias, tag + " bias")
        assert int(torch.isnan(ob).sum()) == ob.numel() - (O if bias is not None else 0), tag + ": written outside out_bias"
        if rsum is not None:
            _same(ors[1:O + 1, 2], rsum, tag + " sigma column")
        assert int(torch.isnan(ors).sum()) == ors.numel() - (O if rsum is not None else 0), tag + ": written outside out_rowscale"
        for buf, view in inp["G"] + inp["X"]:      # the operands' padding is still NaN (and the NaN never reached a sum, checked above)
            assert int(torch.isnan(buf).sum()) == buf.numel() - view.numel()


def run_exact(cases, data, seed=0):
    """The batch `cases` on `data` ("int", "onehot_g", "onehot_x"): every output exact, guards intact, the expected kernels ran.  -> names"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    inputs = [make_inputs(c, data, gen) for c in cases]
    names, bufs = launch(inputs)
    check(inputs, bufs)
    return names
