"""The harness of tests/test_linear_exact_gpu.py: `ardae_linear`, `ardae_linear_chain` and `ardae_linear_wide_layers` with STRIDED operands in
GUARDED buffers, on data for which most epilogues have one representable result (torch.equal, no tolerance), and with the kernel that ran
asserted through the profile log, together with the flops and bytes that log reports for it (tests/golden/linear_profile_costs.json).
tests/test_linear_cases.py runs the same cases through a pure-PyTorch emulator on the CPU (and through
deliberately wrong emulators, which check() must refuse).

Layouts, applied to every operand a case has:
  "tight"  ld = width, 16-byte aligned: the control, and the twin of the bit comparisons;
  "pad4"   16-byte aligned rows, another pad per operand (X K + 4, second source K2 + 8, S + 4, Q + 8, R + 12, Y + 16, Y2 + 20, rowbias + 4,
           eps + 8): the wrong operand's ld, or Nout for an ld, lands in NaN or in another element;
  "odd"    epilogue operands with ld = width + 1 / + 3 and the base one float behind a 16-byte boundary; X as well where the case's path is a
           kernel that takes such rows (the generic per-image block, linear_kernel), pad4 elsewhere so that the case stays on its kernel.
Buffers: an operand is a [rows, width] view with row stride ld of a flat NaN buffer, one guard row (ld floats, at least 4) in front of it and
one behind; the columns between width and ld are its column guards (a tight operand has none: a store to column Nout is a wrong value in the
next row there).  Vectors, colsum [row tiles, Nout] and tile_loss sit in such buffers too.  Read-only operands are compared with a clone bit
for bit after the call, guards included; an output has exactly M Nout numbers afterwards.

Data (CPU generator; the device gets copies, so the emulator sees the same numbers):
  "int"       X in [-4, 4], W in [-3, 3], bias / rowbias / rowscale / rowscale_w / seed vector / Q in [-2, 2], S a relu output (zeros and
              positive integers), scale a power of two: every partial sum is an integer of at most 12 x 1024 + 10 in magnitude, exact in any
              order.  Layer runs and DAE_LOSS use sparse W (4 / 2 non-zeros of +-1 per row; DAE_LOSS: X in [-2, 2], sigma in [-1, 1], eps in
              [-2, 2]) so that layer outputs and the tiles' sums of rho^2 stay far below 2^24.
  "onehot_x"  row m of X has ONE non-zero +-2^j (j in [-2, 2]) at k(m) = K - 1 - (M - 1 - m) p mod K (p coprime to K: a 32-row block spreads over the k chunks,
              M >= K rows reach every k; the last row has k = K - 1; with two sources the rows alternate between them); W carries full
              significands: Y[m, n] = +-2^j W[n, k(m)] bit for bit (relu: its positive part) - every fragment, lane and k chunk in its place.
  "gauss"     the float64 comparison of tests/test_linear_gpu.py at that file's 2e-5, plus bit equality with the "tight" twin launch where
              the profile log names the same kernel for both (the three per-image blocks: always - one k order is their stated rule)."""
import ctypes
import functools
import json
import math
import os
import zlib
from dataclasses import dataclass, replace

import torch

from ardae_amd import _lib as L
from wgrad_cases import _exact32, _full_significands, _same

NAN = float("nan")
TOL = 2e-5                      # tests/test_linear_gpu.py: max |err| / max |ref|
LAYOUTS = ("tight", "pad4", "odd")
_PAD4 = dict(X0=4, X1=8, S=4, Q=8, R=12, Y=16, Y2=20, rowbias=4, eps=8)
_ODD = dict(X0=1, X1=3, S=1, Q=3, R=1, Y=3, Y2=1, rowbias=3, eps=1)
_ODD_X_PATHS = ("small", "geo0", "geo1", "geo2")      # kernels that take rows off a 16-byte boundary

# ---- the kernel a case's `path` must run on: (what the logged name starts with, what it ends with), by knob environment
_G = ("linear_kernel<1, 1, 4, 1, 64, ", "linear_kernel<1, 1, 1, 4, 256, ", "linear_kernel<2, 2, 1, 4, 64, ")
_KNOBS = ("ARDAE_SMALL", "ARDAE_NARROW", "ARDAE_SHORTK", "ARDAE_WIDE")
_LAYER_RUNS = dict(chain=("linear_chain_kernel<", " x{nl}"), wide_layers=("linear_wide_layers_kernel<8, 4, 2, ", " x{nl}"))
_DEFAULT = dict(b16=("linear_small_kernel<", "> b16"), lean=("linear_small_kernel<", "> fast"), small=("linear_small_kernel<", ">"),
                narrow=("linear_narrow_kernel<", ">"), shortk=("linear_shortk_kernel<", ">"),
                wide256=("linear_wide_kernel<8, 4, 2, ", ">"), wide32=("linear_wide_kernel<4, 1, 2, ", ">"),
                wide512=("linear_wide_kernel<8, 8, 1, ", ">"), wide1024=("linear_wide_kernel<8, 16, 1, ", ">"),
                geo0=(_G[0], ">"), geo1=(_G[1], ">"), geo2=(_G[2], ">"), **_LAYER_RUNS)
# every single launch on linear_kernel, in the geometry its (M, Nout) selects ("geo"); the two layer-run entry points do not read these knobs
_GENERIC = dict({p: "geo" for p in _DEFAULT}, **_LAYER_RUNS)
KERNELS = {("1", "1", "1", "1"): _DEFAULT, ("0", "0", "0", "0"): _GENERIC}


def knob_env():
    return tuple("0" if int(L.debug_knob(n, "1")) == 0 else "1" for n in _KNOBS)


def geometry(M, Nout):
    """linear.hip::pick_geometry: 0 = 128 x 32 tiles (Nout <= 32), 1 = 32 x 128 (fewer than 128 tiles of 64 x 256), 2 = 64 x 256."""
    if Nout <= 32:
        return 0
    return 1 if -(-M // 64) * -(-Nout // 256) < 128 else 2


def row_tile(M, Nout):
    return (128, 32, 64)[geometry(M, Nout)]


def col_panels(M, Nout):
    g = geometry(M, Nout)
    return 1 if g == 0 else -(-Nout // (128 if g == 1 else 256))


def kernel_of(c):
    env = knob_env()
    assert env in KERNELS, f"no expected-kernel table for {dict(zip(_KNOBS, env))}"
    want = KERNELS[env][c.path]
    if want == "geo":
        want = (_G[geometry(c.M, c.Nout)], ">")
    return want[0], want[1].format(nl=c.nl)


@dataclass(frozen=True)
class Case:
    M: int
    Ks: tuple                  # one or two sources
    Nout: int
    path: str                  # key of the KERNELS tables
    epi: str = "act"           # act | dact | chain | dae_loss
    act: str = "none"          # none | relu | softplus
    layout: str = "tight"
    bias: bool = False
    rowbias: int = 0           # rows_per_group; 0: no row bias
    rowscale: bool = False
    seed: bool = False         # EPI_ACT: Y2 = -R[c] act'(Y)
    q: bool = False            # EPI_DACT: + Q
    inplace: bool = False      # ... with Y is Q
    colsum: bool = False
    y_null: bool = False       # EPI_DAE_LOSS without Y
    nl: int = 1                # layer runs (path "chain" / "wide_layers"): layers of 256 x 256, layer l reads layer l - 1's Y
    kinds: tuple = ("int",)    # the data this case is exact (or, "gauss", within tolerance) on

    @property
    def tag(self):
        ops = "".join(s for s, on in (("b", self.bias), (f"g{self.rowbias}", self.rowbias), ("s", self.rowscale), ("w", self.seed), ("q", self.q),
                                      ("i", self.inplace), ("c", self.colsum), ("n", self.y_null), (f"x{self.nl}", self.nl > 1)) if on)
        return f"{self.path}-{self.M}x{'+'.join(map(str, self.Ks))}x{self.Nout}-{self.epi}-{self.act}" + (f"-{ops}" if ops else "")


# ---------------------------------------------------------------------------------------------------------------- data
def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _sparse_w(nout, K, nnz, gen):
    """[nout, K] with `nnz` entries of +-1 per row."""
    W = torch.zeros(nout, K)
    cols = torch.rand(nout, K, generator=gen).argsort(1)[:, :nnz]
    W.scatter_(1, cols, torch.randint(0, 2, (nout, nnz), generator=gen).float() * 2 - 1)
    return W


def _onehot_rows(M, Ks, gen):
    """One non-zero +-2^j per row: row m in source m % len(Ks), p columns apart mod K from row to row, ending at its source's last k on its last row."""
    pow2 = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])[torch.randint(0, 5, (M,), generator=gen)]
    val = pow2 * (torch.randint(0, 2, (M,), generator=gen).float() * 2 - 1)
    m = torch.arange(M)
    Xs = []
    for s, K in enumerate(Ks):
        p = next(p for p in (37, 41, 43, 47) if math.gcd(p, K) == 1)
        mine = m % len(Ks) == s
        k = (K - 1 - (int(m[mine][-1]) // len(Ks) - m // len(Ks)) * p) % K        # walks back from K - 1 on the source's last row
        X = torch.zeros(M, K)
        X[m[mine], k[mine]] = val[mine]
        Xs.append(X)
    return Xs


@functools.lru_cache(maxsize=4)
def _base(M, Ks, Nout, kind, sparse, seed):
    """The sources, the first layer's weights and their float64 product: drawn and multiplied once for all cases of a shape."""
    gen = torch.Generator().manual_seed(seed * 1000003 + M * 7 + sum(Ks) * 3 + Nout)
    if kind == "int":
        assert sum(Ks) <= 1024 and 12 * 1024 + 10 < 2 ** 24      # |x w| <= 12 per k, |addends| <= 10: any partial sum is an exact integer
        lim = 2 if sparse == 2 else 4
        Xs = [_ints((M, K), -lim, lim, gen) for K in Ks]
        Ws = [_sparse_w(Nout, K, sparse, gen) if sparse else _ints((Nout, K), -3, 3, gen) for K in Ks]
    elif kind == "onehot_x":
        Xs, Ws = _onehot_rows(M, Ks, gen), [_full_significands((Nout, K), gen, 18) for K in Ks]
    else:
        Xs = [torch.randn(M, K, generator=gen) for K in Ks]
        Ws = [torch.randn(Nout, K, generator=gen) / sum(Ks) ** 0.5 for K in Ks]
    V = sum(x.double() @ w.double().T for x, w in zip(Xs, Ws))
    return Xs, Ws, V, {}


def _scale(c):
    return 2.0 ** -round(math.log2(c.M * c.Nout))        # ~ 1 / (M z), a power of two: the products with it are exact


def make_data(c, kind, seed=0):
    """Dense CPU tensors of every operand of every layer, and the float64 references."""
    assert kind in c.kinds, (kind, c.tag)
    sparse = 0 if kind != "int" else 2 if c.epi == "dae_loss" else 4 if c.nl > 1 else 0
    Xs, W0, V0, cache = _base(c.M, c.Ks, c.Nout, kind, sparse, seed)
    gen = torch.Generator().manual_seed(seed * 7919 + zlib.crc32(c.tag.encode()) % 100000)
    M, N, exact = c.M, c.Nout, kind != "gauss"
    small = (lambda *s: _ints(s, -2, 2, gen)) if exact else (lambda *s: torch.randn(*s, generator=gen))
    layers, x64 = [], None
    for l in range(c.nl):
        d = dict(W=W0 if l == 0 else [_sparse_w(N, N, 4, gen) if kind == "int" else torch.randn(N, N, generator=gen) / N ** 0.5])
        V = V0 if l == 0 else x64 @ d["W"][0].double().T
        first, last = l == 0, l == c.nl - 1
        if c.epi in ("act", "dae_loss") and c.bias:
            d["bias"] = small(N)
        if c.epi == "act":
            if c.rowbias and first:
                d["rowbias"] = small(-(-M // c.rowbias), N)
            if c.rowscale and first:
                d["rowscale"], d["rowscale_w"] = small(M), small(N)
            if c.seed and last:
                d["w"] = small(N)
            pre = V + (d["bias"].double() if "bias" in d else 0.0)
            if "rowbias" in d:
                pre = pre + d["rowbias"].double().repeat_interleave(c.rowbias, 0)[:M]
            if "rowscale" in d:
                pre = pre + d["rowscale"].double()[:, None] * d["rowscale_w"].double()
            d["pre"] = pre
            Y = _act(c.act, pre)
            ref = dict(Y=Y)
            if "w" in d:
                ref["Y2"] = -d["w"].double() * _d1(c.act, Y)
        elif c.epi in ("dact", "chain"):
            if exact:
                d["S"] = _ints((M, N), -3, 3, gen).clamp(min=0)                       # a relu output
            else:
                d["S"] = torch.nn.functional.softplus(torch.randn(M, N, generator=gen) * 3)
            s1 = _d1(c.act, d["S"].double())
            if c.epi == "dact":
                if c.q:
                    d["Q"] = small(M, N)
                ref = dict(Y=V * s1 + (d["Q"].double() if c.q else 0.0))
            else:
                d["R"] = small(M, N)
                ref = dict(Y=V * s1, Y2=V * d["R"].double() * (1 - s1 if c.act == "softplus" else 0.0))
        else:
            lo = (lambda a, *s: _ints(s, -a, a, gen)) if exact else (lambda a, *s: torch.randn(*s, generator=gen))
            d["sigma"], d["eps"], d["scale"] = lo(1, M), lo(2, M, N), _scale(c) if exact else 1.0 / (M * N)
            g = V + (d["bias"].double() if c.bias else 0.0)
            rho = d["sigma"].double()[:, None] * g + d["eps"].double()
            ref = dict(Y=g, Y2=2 * d["sigma"].double()[:, None] * rho * d["scale"], loss=(rho ** 2).sum())
            if exact:      # rho^2 are non-negative integers: every tile's sum, and their sum in any order, is an exact integer
                assert float(ref["loss"]) < 2 ** 24
        if c.colsum and last:
            rt = row_tile(M, N)
            pad = torch.zeros(-(-M // rt) * rt, N, dtype=torch.float64)
            pad[:M] = ref["Y"]
            ref["colsum"] = pad.view(-1, rt, N).sum(1)
        d["ref"] = ref
        x64 = ref["Y"]
        layers.append(d)
    data = dict(case=c, kind=kind, X=Xs, layers=layers, cache=cache)
    _assert_data_conditions(data)
    return data


def _act(act, pre):
    return {"none": pre, "relu": pre.clamp(min=0), "softplus": torch.nn.functional.softplus(pre)}[act]


def _d1(act, s):
    """act' from the saved OUTPUT."""
    return {"none": torch.ones_like(s), "relu": (s > 0).to(s.dtype), "softplus": -torch.expm1(-s)}[act]


def _assert_data_conditions(data):
    """What the harness claims about its own data (exact kinds): every reference is an fp32 number below 2^24 ("int"), at least a quarter of
    each checked output is non-zero, a relu has at least a quarter of its pre-activations on each side of zero."""
    c = data["case"]
    if data["kind"] == "gauss":
        return
    for l, d in enumerate(data["layers"]):
        for name, ref in d["ref"].items():
            what = f"{c.tag} layer {l} {name}"
            if name == "loss":
                continue
            _exact32(ref, what)
            if data["kind"] == "int":
                assert float(ref.abs().max()) < 2 ** 24, what
            if not (name == "Y2" and c.epi == "chain" and c.act != "softplus"):       # (relu's second derivative: all zeros)
                assert float((ref != 0).double().mean()) >= 0.25, f"{what}: only {float((ref != 0).double().mean()):.3f} non-zero"
        if c.epi == "act" and c.act == "relu":
            pos, neg = float((d["pre"] > 0).double().mean()), float((d["pre"] < 0).double().mean())
            assert pos >= 0.25 and neg >= 0.25, f"{c.tag} layer {l}: pre-activations {pos:.3f} above / {neg:.3f} below zero"


# ---------------------------------------------------------------------------------------------------------------- buffers
def _guarded(mat, ld, off, device):
    """`mat` ([rows, width] or a vector) as a view with row stride `ld` of a flat NaN buffer: one guard row in front (the view starts `off`
    floats behind a 16-byte boundary), one behind.  mat None: the view stays NaN (an output).  -> (buffer, view)"""
    rows, width = mat if isinstance(mat, tuple) else (mat.shape if mat.dim() == 2 else (1, mat.shape[0]))
    assert ld >= width
    lead = max(4, -(-ld // 4) * 4) + off
    buf = torch.full((lead + rows * ld + max(4, ld),), NAN, device=device)
    view = buf.as_strided((rows, width), (ld, 1), lead)
    if not isinstance(mat, tuple):
        view.copy_(mat.view(rows, width))
    assert device == "cpu" or view.data_ptr() % 16 == 4 * (off % 4)
    return buf, view


def _lds(c):
    """name -> (floats added to the width, floats behind a 16-byte boundary) for the case's layout."""
    if c.layout == "tight":
        return {k: (0, 0) for k in _PAD4}
    if c.layout == "pad4":
        return {k: (v, 0) for k, v in _PAD4.items()}
    lds = {k: (v, 1) for k, v in _ODD.items()}
    if c.path not in _ODD_X_PATHS:
        lds.update(X0=(_PAD4["X0"], 0), X1=(_PAD4["X1"], 0))
    return lds


def make_inputs(data, device, layout=None):
    """Every operand of every layer in guarded buffers on `device`, outputs all NaN (in place: the Y view holds Q).
    -> dict(case, layers=[{name: (buffer, view)}], clones of the read-only buffers)"""
    c = data["case"] if layout is None else replace(data["case"], layout=layout)
    lds, voff = _lds(c), 0 if c.layout != "odd" else 1
    M, N = c.M, c.Nout
    layers = []
    for l, d in enumerate(data["layers"]):
        o = {}
        if l == 0:
            for s, x in enumerate(data["X"]):
                o[f"X{s}"] = _guarded(x, x.shape[1] + lds[f"X{s}"][0], lds[f"X{s}"][1], device)
        for name in ("bias", "rowscale", "rowscale_w", "w", "sigma"):
            if name in d:
                o[name] = _guarded(d[name], d[name].shape[0], voff, device)
        for name in ("rowbias", "S", "R", "eps"):
            if name in d:
                o[name] = _guarded(d[name], N + lds[name][0], lds[name][1], device)
        if "Q" in d and not c.inplace:
            o["Q"] = _guarded(d["Q"], N + lds["Q"][0], lds["Q"][1], device)
        if not c.y_null:
            # (a layer run's inner Y is the next layer's X: it keeps 16-byte aligned rows under "odd")
            ypad, yoff = lds["Y"] if (l == c.nl - 1 or c.layout != "odd") else (_PAD4["Y"], 0)
            o["Y"] = _guarded(d["Q"] if c.inplace else (M, N), N + ypad, yoff, device)
        if "Y2" in d["ref"]:
            o["Y2"] = _guarded((M, N), N + lds["Y2"][0], lds["Y2"][1], device)
        if "colsum" in d["ref"]:
            o["colsum"] = _guarded((-(-M // row_tile(M, N)), N), N, voff, device)
        if c.epi == "dae_loss":
            o["tile_loss"] = _guarded((-(-M // row_tile(M, N)) * col_panels(M, N), 1), 1, voff, device)
        layers.append(o)
    outputs = ("Y", "Y2", "colsum", "tile_loss")
    clones = [{k: b.clone() for k, (b, _) in o.items() if k not in outputs} for o in layers]
    return dict(case=c, data=data, device=device, layers=layers, clones=clones)


# ---------------------------------------------------------------------------------------------------------------- backends
def _packed(data, l, device):
    """Packed weight images of layer l (library backend), made once per data set (and once per shape for the first layer)."""
    store = data["cache"] if l == 0 else data["layers"][l]
    if "wp" not in store:
        wps = []
        for W in data["layers"][l]["W"]:
            Wd = W.to(device)
            out = torch.empty(L.lib().ardae_packed_floats(W.shape[0], W.shape[1]), device=device)
            L.check(L.lib().ardae_pack_weight(L.ptr(Wd), Wd.stride(0), W.shape[0], W.shape[1], 0, L.ptr(out), L.stream_ptr()))
            wps.append(out)
        store["wp"] = wps
    return store["wp"]


_EPI = dict(act="EPI_ACT", dact="EPI_DACT", chain="EPI_CHAIN", dae_loss="EPI_DAE_LOSS")


def _args(inp, l):
    c, d, o = inp["case"], inp["data"]["layers"][l], inp["layers"][l]
    a = L.LinearArgs()
    a.M, a.Nout, a.act = c.M, c.Nout, L.ACT[c.act]
    srcs = [o[f"X{s}"][1] for s in range(len(c.Ks))] if l == 0 else [inp["layers"][l - 1]["Y"][1]]
    a.nsrc = len(srcs)
    for s, (x, wp) in enumerate(zip(srcs, _packed(inp["data"], l, inp["device"]))):
        a.src[s].x, a.src[s].ld, a.src[s].K, a.src[s].wp = x.data_ptr(), x.stride(0), x.shape[1], wp.data_ptr()
    ptr = lambda k: o[k][1].data_ptr() if k in o else None
    a.bias, a.rowscale, a.rowscale_w, a.sigma = ptr("bias"), ptr("rowscale"), ptr("rowscale_w"), ptr("sigma")
    if "rowbias" in o:
        a.rowbias, a.rowbias_ld, a.rows_per_group = ptr("rowbias"), o["rowbias"][1].stride(0), c.rowbias
    for k, ld in (("S", "ldS"), ("Q", "ldQ"), ("eps", "ldeps"), ("Y", "ldY"), ("Y2", "ldY2")):
        if k in o:
            setattr(a, k, ptr(k)); setattr(a, ld, o[k][1].stride(0))
    if c.inplace:
        a.Q, a.ldQ = a.Y, a.ldY
    if "R" in o:
        a.R, a.ldR = ptr("R"), o["R"][1].stride(0)
    if "w" in o:
        a.R = ptr("w")
    a.scale = d.get("scale", 0.0)
    a.colsum, a.tile_loss = ptr("colsum"), ptr("tile_loss")
    return a


def _library(inp, per_layer):
    c, lib, epi = inp["case"], L.lib(), getattr(L, _EPI[inp["case"].epi])
    arr = (L.LinearArgs * c.nl)(*[_args(inp, l) for l in range(c.nl)])
    lib.ardae_profile_enable(1)
    try:
        if c.nl == 1 or per_layer:
            for l in range(c.nl):
                L.check(lib.ardae_linear(ctypes.byref(arr[l]), epi, L.stream_ptr()), "ardae_linear")
        elif c.path == "chain":
            assert lib.ardae_linear_chain_eligible(arr, c.nl, epi) == 1, c.tag
            L.check(lib.ardae_linear_chain(arr, c.nl, epi, L.stream_ptr()), "ardae_linear_chain")
        else:
            assert lib.ardae_linear_wide_layers_eligible(arr, c.nl, epi) == 1, c.tag
            L.check(lib.ardae_linear_wide_layers(arr, c.nl, epi, L.stream_ptr()), "ardae_linear_wide_layers")
        return L.profile_report(max_entries=64)
    finally:
        lib.ardae_profile_enable(0)


# ---- the cost model: (name, calls, flops, bytes) of the profile log, recorded from a build of the commit BEFORE the launchers' cost
# expressions were written once (tools/gen_linear_profile_costs.py).  bench.py builds its roofline from these numbers.
COSTS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_profile_costs.json")
_LINEAR_FAMILY = ("linear_", "sampler_tail_")


@functools.lru_cache(maxsize=1)
def recorded_costs():
    with open(COSTS_PATH) as f:
        return json.load(f)


def costs(entries):
    """The linear family's entries of a profile report as sorted [name, calls, flops, bytes]; flops and bytes are integer-valued doubles
    far below 2^53 (sums of products of sizes), so the comparison with the fixture is exact whatever the order of summation."""
    out = []
    for e in entries:
        if e["name"].startswith(_LINEAR_FAMILY):
            assert e["flops"] == int(e["flops"]) and e["bytes"] == int(e["bytes"]) and max(e["flops"], e["bytes"]) < 2 ** 53, e
            out.append([e["name"], int(e["calls"]), int(e["flops"]), int(e["bytes"])])
    return sorted(out)


def profiled(fn):
    """fn() with the profile log on -> costs() of what it launched."""
    lib = L.lib()
    lib.ardae_profile_enable(1)
    try:
        fn()
        return costs(L.profile_report(max_entries=64))
    finally:
        lib.ardae_profile_enable(0)


def scene_score_pass(B=64, S=1):
    """The 64-row cDAE score pass of tests/test_cdae_gpu.py's chain-cap child.  One row per image (64 x 1): the whole pass is ONE launch of
    the small chain, its two encoders levels of two problems.  Two rows per image (32 x 2): no chain launch (csrc/cdae.hip), the
    encoders' levels go out as launches of the pair, the rest one launch per layer."""
    from oracle import ardae_oracle as O
    from test_cdae_gpu import CdaeHarness
    cc = O.CdaeCfg("grad", 32, 32, 256, 3, "softplus")
    pc = O.init_params(O.cdae_param_spec(cc), 3)
    H = CdaeHarness(cc, torch.cat([pc[n].reshape(-1) for n, _ in O.cdae_param_spec(cc)]))
    g = torch.Generator().manual_seed(64)
    x, ctx, sigma = torch.randn(B * S, 32, generator=g) * 30, torch.randn(B, 32, generator=g), torch.zeros(B * S)
    return profiled(lambda: H.score(x, sigma, ctx, B, S))


def scene_forward_hidden():
    """One forward_hidden of the mnist 784 / 100 / 256 / 32 model at 32 images x nz 256: 8192 rows, the fewest the short-K and tail kernels take."""
    import ardae_amd as net
    torch.manual_seed(3)
    model = net.MNISTIPVAE(input_dim=784, noise_dim=100, h_dim=256, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=32).to("cuda")
    x, noise = (torch.rand(32, 784) < 0.2).float().cuda(), torch.randn(32 * 256, 100).cuda()
    return profiled(lambda: model.forward_hidden(x, nz=256, noise=noise))


SCENES = dict(score_pass_64=scene_score_pass, score_pass_32x2=functools.partial(scene_score_pass, 32, 2), forward_hidden_8192=scene_forward_hidden)


def emulate(inp, bug=None):
    """The operator in ordinary tensor operations on the SAME guarded views (float64 arithmetic, rounded once).  `bug`: one of the wrong
    kernels tests/test_linear_cases.py shows check() to refuse."""
    c = inp["case"]
    M, N = c.M, c.Nout
    wider = lambda v, rows, cols: v.as_strided((v.shape[0] + rows, v.shape[1] + cols), v.stride(), v.storage_offset())
    for l, (d, o) in enumerate(zip(inp["data"]["layers"], inp["layers"])):
        v = {k: t for k, (_, t) in o.items()}
        srcs = [v[f"X{s}"] for s in range(len(c.Ks))] if l == 0 else [inp["layers"][l - 1]["Y"][1]]
        V = sum(x.double() @ w.double().T for x, w in zip(srcs, d["W"]))
        rows = torch.arange(M)
        S = v.get("S")
        if bug == "S_with_ldY" and S is not None:
            flat, idx = o["S"][0], S.storage_offset() + torch.arange(M)[:, None] * v["Y"].stride(0) + torch.arange(N)
            S = torch.where(idx < flat.numel(), flat[idx.clamp(max=flat.numel() - 1)], torch.tensor(NAN))      # (beyond the buffer: anything)
        Y2 = None
        if c.epi == "act":
            pre = V + (v["bias"][0].double() if "bias" in v else 0.0)
            if "rowbias" in v:
                g = rows // c.rowbias
                if bug == "rowbias_of_previous_group":
                    g = (rows - 1).clamp(min=0) // c.rowbias
                pre = pre + v["rowbias"].double()[g]
            if "rowscale" in v:
                pre = pre + v["rowscale"][0].double()[:, None] * v["rowscale_w"][0].double()
            Y = _act(c.act, pre)
            if "w" in v:
                Y2 = -v["w"][0].double() * _d1(c.act, Y.float().double())
        elif c.epi == "dact":
            Q = v["Y"] if c.inplace else v.get("Q")
            Y = V * _d1(c.act, S.double()) + (Q.double() if Q is not None and bug != "drops_Q" else 0.0)
        elif c.epi == "chain":
            s1 = _d1(c.act, S.double())
            Y, Y2 = V * s1, V * v["R"].double() * (1 - s1 if c.act == "softplus" else 0.0)
        else:
            sg = v["sigma"][0].double()[:, None]
            Y = V + (v["bias"][0].double() if "bias" in v else 0.0)
            rho = sg * Y + v["eps"].double()
            Y2 = 2 * sg * rho * d["scale"]
            rt = row_tile(M, N)
            pad = torch.zeros(-(-M // rt) * rt, dtype=torch.float64)
            pad[:M] = (rho ** 2).sum(1)
            v["tile_loss"][:, 0] = pad.view(-1, rt).sum(1).float()
        if "Y" in v:
            if bug == "writes_row_M":
                wider(v["Y"], 1, 0)[M] = 1.0
            if bug == "writes_column_Nout":
                wider(v["Y"], 0, 1)[:, N] = 1.0
            v["Y"].copy_(Y.float())
        if "Y2" in v:
            v["Y2"].copy_(Y2.float())
        if "colsum" in v:
            rt = row_tile(M, N)
            pad = torch.zeros(-(-M // rt) * rt, N, dtype=torch.float64)
            pad[:M] = Y.float().double()
            cs = pad.view(-1, rt, N).sum(1)
            if bug == "colsum_row_twice":
                cs[-1] += pad[M - 1]
            v["colsum"].copy_(cs.float())
        if bug == "modifies_input":
            v["X0" if l == 0 else "S"][M // 2, 0] += 1.0
    return None


def launch(case, inp, backend="lib"):
    """Run `case` (the one `inp` was made for, in any layout) on `backend`: "lib" (its entry point; asserts that the kernel of its `path`, and no other, ran), "per_layer" (a layer
    run as nl calls of ardae_linear), "twin" (any kernel), or an emulator callable.  -> the kernel names of the profile log (None: emulator)"""
    assert replace(inp["case"], layout=case.layout) == case
    if callable(backend):
        return backend(inp)
    entries = _library(inp, backend == "per_layer")
    names = {e["name"] for e in entries}
    if backend == "lib":
        head, tail = kernel_of(case)
        assert len(names) == 1 and all(n.startswith(head) and n.endswith(tail) for n in names), \
            f"{case.tag}: ran {sorted(names)}, meant for {head}...{tail} under {dict(zip(_KNOBS, knob_env()))}"
        if knob_env() == ("1", "1", "1", "1"):       # the fixture holds the default environment: a case's cost follows its tag, not its layout or data
            want = recorded_costs()["cases"][case.tag]
            assert costs(entries) == want, f"{case.tag}: the profile log reports {costs(entries)}, the recorded cost is {want}"
    return names


# ---------------------------------------------------------------------------------------------------------------- checks
def _bits(t):
    return t.view(torch.int32)


def check(inp):
    """Inputs unmodified (guards included), outputs' guards intact, every value exact ("int", "onehot_x") or within TOL of float64 ("gauss")."""
    c, data, dev = inp["case"], inp["data"], inp["device"]
    M, N, exact = c.M, c.Nout, inp["data"]["kind"] != "gauss"
    for l, (d, o, clones) in enumerate(zip(data["layers"], inp["layers"], inp["clones"])):
        tag = f"{c.tag} {c.layout} {data['kind']} layer {l}"
        for k, clone in clones.items():
            assert torch.equal(_bits(o[k][0]), _bits(clone)), f"{tag}: the read-only operand {k} (or its padding) was modified"
        want = dict(Y=M * N, Y2=M * N, colsum=-(-M // row_tile(M, N)) * N, tile_loss=-(-M // row_tile(M, N)) * col_panels(M, N))
        for k in ("Y", "Y2", "colsum", "tile_loss"):
            if k in o:
                nans = int(torch.isnan(o[k][0]).sum())
                assert nans == o[k][0].numel() - want[k], \
                    f"{tag}: {k} has {o[k][0].numel() - nans} numbers, {want[k]} belong there - written outside the view, or not everywhere inside"
        for k, ref in d["ref"].items():
            if k == "loss":
                got = float(o["tile_loss"][1].double().sum())
                if exact:
                    assert got == float(ref), f"{tag}: sum of tile_loss {got}, want {float(ref)}"
                else:
                    assert abs(got - float(ref)) / float(ref) < 1e-5, f"{tag}: sum of tile_loss {got}, want {float(ref)}"
            elif k == "Y" and c.y_null:
                continue
            elif exact:
                _same(o[k][1], ref.float().to(dev), f"{tag} {k}")
            else:
                err = float((o[k][1].double() - ref.to(dev)).abs().max() / (ref.abs().max() + 1e-30))
                assert err < TOL, f"{tag} {k}: max |err| / max |ref| = {err:.3e}"


def outputs_equal(a, b, what):
    """Two launches' outputs, bit for bit."""
    for l, (oa, ob) in enumerate(zip(a["layers"], b["layers"])):
        for k in ("Y", "Y2", "colsum", "tile_loss"):
            if k in oa:
                assert torch.equal(_bits(oa[k][1].contiguous()), _bits(ob[k][1].contiguous())), f"{what}: {k} of layer {l} differs"


def run_case(c, kind, backend="lib", device="cuda", seed=0):
    """One case on one kind of data: launch, check; "gauss" (library): also the tight twin / the per-layer launches, bit for bit where they
    ran the same kernel family member (see the module docstring)."""
    data = make_data(c, kind, seed)
    inp = make_inputs(data, device)
    names = launch(c, inp, backend)
    check(inp)
    if kind != "gauss" or callable(backend):
        return names
    if c.nl > 1:         # a layer run equals nl launches of the N-row kernel on the same strided operands (both documented bit-identical)
        twin = make_inputs(data, device)
        tnames = launch(c, twin, "per_layer")
        check(twin)
        if all(n.startswith("linear_wide_kernel<") for n in tnames):
            outputs_equal(inp, twin, f"{c.tag} {c.layout}: layer run against per-layer launches")
    elif c.layout != "tight":
        twin = make_inputs(data, device, layout="tight")
        tnames = launch(c, twin, "twin")
        check(twin)
        if tnames == names or all(n.startswith("linear_small_kernel<") for n in names | tnames):
            outputs_equal(inp, twin, f"{c.tag}: {c.layout} against tight")
    return names


# ---------------------------------------------------------------------------------------------------------------- the table
def _variants(path, M, Ks, N, rpg, seed=True, rowscale=True, q_forms=True, colsum=None, chain=True, softplus_only=False, dact=True):
    """The epilogue / activation / operand combinations of one (path, shape): exact ones on "int" (with addends) and "int" + "onehot_x"
    (without: +-2^j W plus a bias would round), softplus and CHAIN on "gauss".  colsum: True (three of them) or "all" (the shapes that
    reach their kernel only with it); a column sum of full significands is not exact, so those cases leave "onehot_x" out."""
    K = Ks if isinstance(Ks, tuple) else (Ks,)
    def mk(colsum=False, kinds=("int",), **kw):
        cs = bool(colsum) or all_cs
        return Case(M, K, N, path, colsum=cs, kinds=tuple(k for k in kinds if not (cs and k == "onehot_x")), **kw)
    all_cs, colsum = colsum == "all", bool(colsum)
    full = dict(bias=True, rowbias=rpg, rowscale=rowscale, seed=seed)
    out = []
    if not softplus_only:
        out += [mk(act="none", kinds=("int", "onehot_x")), mk(act="relu", kinds=("onehot_x",)),
                mk(act="none", **full), mk(act="relu", **full, colsum=colsum)]
        if dact:
            out += [mk(epi="dact", act="none", kinds=("int", "onehot_x")), mk(epi="dact", act="relu", kinds=("int", "onehot_x"))]
            if q_forms:
                out += [mk(epi="dact", act="none", q=True, colsum=colsum), mk(epi="dact", act="relu", q=True, inplace=True)]
    out.append(mk(act="softplus", **dict(full, seed=seed and not softplus_only), kinds=("gauss",)))
    if dact:
        out.append(mk(epi="dact", act="softplus", q=q_forms, inplace=q_forms, kinds=("gauss",)))
    if chain and dact and not softplus_only:
        out.append(mk(epi="chain", act="softplus", kinds=("gauss",), colsum=colsum))
    return [c for c in out if c.kinds]


def _layer_runs(path, M):
    mk = lambda **kw: Case(M, (256,), 256, path, **kw)
    out = []
    for nl in (2, 3):
        out += [mk(act="relu", bias=True, nl=nl), mk(epi="dact", act="relu", nl=nl), mk(epi="dact", act="relu", q=True, inplace=True, nl=nl),
                mk(act="softplus", bias=True, nl=nl, kinds=("gauss",)), mk(epi="dact", act="softplus", q=True, nl=nl, kinds=("gauss",)),
                mk(epi="chain", act="softplus", colsum=True, nl=nl, kinds=("gauss",))]
    if path == "chain":     # the energy stack's first and last layers: row bias + sigma term, score seed
        out += [mk(act="relu", bias=True, rowbias=64, rowscale=True, seed=True, nl=2),
                mk(act="softplus", bias=True, rowbias=128, rowscale=True, seed=True, nl=3, kinds=("gauss",))]
    return out


def _dae(path, M, K, z, **kw):
    return Case(M, (K,), z, path, epi="dae_loss", **kw)


def _table():
    t = []
    # 16 x 16 block: ragged columns (36), a partial last step of 16 k (100, 12), two sources
    t += _variants("b16", 48, 100, 36, 4) + _variants("b16", 16, 32, 48, 1) + _variants("b16", 64, (40, 12), 48, 8)
    # lean 32 x 32 block
    t += _variants("lean", 352, 64, 224, 4) + _variants("lean", 512, 256, 256, 3)
    # generic per-image block: ragged rows / K / columns (the lean shapes with X off a 16-byte boundary: ODD_ONLY below)
    t += _variants("small", 100, 37, 70, 7)
    # linear_narrow_kernel
    t += [Case(16512, (256,), z, "narrow", bias=b, kinds=("int", "onehot_x") if not b else ("int",)) for z in (32, 20) for b in (True, False)]
    t += [_dae("narrow", 384, 256, z, bias=z != 20, y_null=z == 2, kinds=("int", "gauss")) for z in (32, 20, 2)]
    # linear_shortk_kernel: row-bias groups aligned to its 128-row workgroups (128) and not (48)
    for (K, N), rpg in zip(((100, 96), (36, 128)), (128, 48)):
        t += _variants("shortk", 8192, K, N, rpg, seed=False, rowscale=False, dact=False)
    # linear_wide_kernel: one tile per workgroup (8192 rows), 257 tiles (16448: one workgroup carries deferred stores into a second tile)
    for M in (8192, 16448):
        t += _variants("wide256", M, 256, 256, 64, colsum=True) + _variants("wide32", M, 32, 256, 128, colsum=True)
    t += [Case(8256, (256,), 256, "wide256", act=a, bias=True, rowbias=96, rowscale=True, seed=True, kinds=k)      # group-tile mode
          for a, k in (("none", ("int",)), ("relu", ("int",)), ("softplus", ("gauss",)))]
    t += _variants("wide512", 2048, 512, 512, 64) + _variants("wide512", 8192, 512, 128, 128, colsum=True)
    # (2048, 512, 512) with colsum: linear_row_tiles() sizes colsum for 32-row tiles there - not the wide kernel's 64 (linear_wide_eligible)
    t += [Case(2048, (512,), 512, "geo1", epi="dact", act="relu", q=True, colsum=True)]
    t += _variants("wide1024", 1024, 1024, 1024, 64, softplus_only=True, q_forms=False)
    t += _layer_runs("chain", 8192) + _layer_runs("wide_layers", 8192)
    # linear_kernel's three geometries
    t += [Case(16500, (256,), 20, "geo0", bias=True), Case(16500, (256,), 20, "geo0", act="relu", kinds=("onehot_x",)),
          _dae("geo0", 300, 100, 8, bias=True), _dae("geo0", 300, 100, 8, kinds=("gauss",))]
    t += _variants("geo1", 200, 256, 256, 8, colsum="all")       # (without colsum: a per-image shape)
    t += _variants("geo2", 8200, 256, 256, 50, colsum=True)
    return t


# cases that reach their path only with X off a 16-byte boundary: the "odd" layout alone
ODD_ONLY = (_variants("small", 352, 64, 224, 4) + _variants("small", 512, 256, 256, 3) + _variants("geo2", 8192, 256, 256, 64, colsum=True))
TABLE = [(replace(c, layout=lay), kind) for c in _table() for lay in LAYOUTS for kind in c.kinds] + \
        [(replace(c, layout="odd"), kind) for c in ODD_ONLY for kind in c.kinds]
IDS = [f"{c.tag}-{c.layout}-{kind}" for c, kind in TABLE]
assert len(set(IDS)) == len(IDS)
