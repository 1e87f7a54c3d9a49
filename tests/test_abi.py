"""The C-ABI library loads and exports every symbol include/ardae_hip.h declares (no compute: runs without a GPU)."""
import ctypes
import os
import re

import pytest

import ardae_amd
from ardae_amd import _lib as L
from ardae_amd import layout
from ardae_amd.modules import KIND_IDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "ardae_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ardae_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound():
    syms = declared_symbols()
    assert len(syms) >= 30
    h = ctypes.CDLL(L.LIB_PATH)
    for s in syms:
        assert hasattr(h, s), f"{s} declared in include/ardae_hip.h but not exported by libardae_hip.so"
        assert s in L.EXPORTS, f"{s} has no ctypes binding in _lib.EXPORTS"
    assert sorted(L.EXPORTS) == syms


# ---- the binding is DERIVED from the header (ardae_amd/_lib.py::parse_header), so the header cannot vouch for it: what follows pins the
# derivation against the compiler, against signatures and constants written out here, and against inputs the parser must refuse
vp, i32, i64, u64, f32, f64, usize = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double,
                                      ctypes.c_size_t)


def test_struct_layout_matches_the_compiler():
    """The same literals as the static_asserts of csrc/api.hip: sizes of the six structs, offsets of the last fields of the two big ones."""
    sizes = {"ardae_lin_src": 24, "ardae_linear_args": 232, "ardae_wgrad_problem": 144, "ardae_cdae_desc": 24, "ardae_model_desc": 32,
             "ardae_profile_entry": 128}
    assert list(L.STRUCTS) == list(sizes)                                   # declaration order: ardae_lin_src before its user
    assert {n: ctypes.sizeof(c) for n, c in L.STRUCTS.items()} == sizes
    assert (L.LinearArgs.tile_loss.offset, L.WgradProblem.beta.offset) == (224, 140)
    assert [L.STRUCTS[n] for n in sizes] == [L.LinSrc, L.LinearArgs, L.WgradProblem, L.CdaeDesc, L.ModelDesc, L.ProfileEntry]
    # one field of every declaration form the header uses: `int M, Nout;`, two declarations on a line, arrays, a nested struct by value
    assert [f[0] for f in L.LinearArgs._fields_[:4]] == ["M", "Nout", "nsrc", "src"] and L.LinearArgs.src.size == 2 * 24
    assert (L.LinearArgs.S.offset + 8, L.LinearArgs.S.size) == (L.LinearArgs.ldS.offset, 8)
    assert (L.WgradProblem.G.size, L.WgradProblem.ldG.size, L.ProfileEntry.name.size, L.ProfileEntry.calls.offset) == (16, 8, 96, 96)
    assert [f[0] for f in L.ModelDesc._fields_] == ["kind", "input_dim", "noise_dim", "h_dim", "z_dim", "n_layers", "act", "flags"]


SIGNATURES = {      # every scalar type, data pointers, a struct pointer, an out-parameter; one (name, type) per parameter, in order
    "ardae_adam_ref_step": (i32, [("p", vp), ("g", vp), ("exp_avg", vp), ("exp_avg_sq", vp), ("max_exp_avg_sq", vp), ("n", i64), ("lr", f64),
                                  ("beta1", f64), ("beta2", f64), ("eps", f64), ("step", i32), ("stream", vp)]),
    "ardae_weight_avg": (i32, [("avg", vp), ("p", vp), ("n", i64), ("kind", i32), ("decay", f64), ("origin", i64), ("state", vp), ("t", i64),
                               ("stream", vp)]),
    "ardae_cdae_perturb_loss_grads": (i32, [("d", ctypes.POINTER(L.CdaeDesc)), ("params", vp), ("packed", vp), ("latent", vp), ("z0", vp),
                                            ("ctx", vp), ("B", i32), ("nz", i32), ("std_scale", f32), ("delta", f32), ("seed", u64),
                                            ("offset_xi", u64), ("offset_eps", u64), ("state", vp), ("first_row", u64), ("xbar", vp),
                                            ("sigma", vp), ("eps_out", vp), ("std_b", vp), ("workspace", vp), ("workspace_floats", usize),
                                            ("loss", vp), ("grads", vp), ("stream", vp)]),
    "ardae_dp_comm_create": (i32, [("host_id", vp), ("nranks", i32), ("rank", i32), ("comm_out", ctypes.POINTER(vp))]),
    "ardae_gather_rows": (i32, [("table", vp), ("idx", vp), ("B", i32), ("D", i32), ("out", vp), ("stream", vp)]),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_derived_signature_matches_the_literal_one(name):
    restype, params = SIGNATURES[name]
    assert L.EXPORTS[name] == (restype, [t for _, t in params])
    assert [p[0] for p in L.PROTOTYPES[name][1]] == [n for n, _ in params]
    fn = getattr(L.lib(), name)
    assert fn.restype is restype and list(fn.argtypes) == [t for _, t in params]


def test_other_return_types_and_out_parameters():
    assert L.EXPORTS["ardae_last_error"] == (ctypes.c_char_p, []) and L.EXPORTS["ardae_dp_backend"] == (ctypes.c_char_p, [])
    assert L.EXPORTS["ardae_cdae_workspace_floats"] == (usize, [ctypes.POINTER(L.CdaeDesc), i32, i32, i32])
    assert L.EXPORTS["ardae_dp_comm_query"] == (i32, [vp] + [ctypes.POINTER(i32)] * 3)
    assert L.EXPORTS["ardae_cdae_perturb_fused_ok"] == (i32, [ctypes.POINTER(L.CdaeDesc), i32, i32])
    assert L.EXPORTS["ardae_profile_report"] == (i32, [ctypes.POINTER(L.ProfileEntry), i32])
    assert L.EXPORTS["ardae_debug_stamp"] == (i32, [vp, i32, vp])
    pointees = lambda name: [p[2] for p in L.PROTOTYPES[name][1]]
    assert pointees("ardae_gather_rows") == ["float", "int64_t", None, None, "float", "void"]
    assert pointees("ardae_debug_stamp") == ["unsigned long long", None, "void"]


def test_derived_constants_have_todays_values():
    from ardae_amd import optim
    assert L.ACT == {"none": 0, None: 0, "relu": 1, "softplus": 2, "csoftplus": 2, "elu": 3, "tanh": 4, "leaky_relu": 5, "swish": 6}
    assert (L.EPI_ACT, L.EPI_DACT, L.EPI_CHAIN, L.EPI_DAE_LOSS) == (0, 1, 2, 3)
    assert (L.MODEL_NO_CENTER, L.MODEL_HEAD_SHIFT, L.MODEL_CLIPPED, L.MODEL_CLIP_Z0_SHIFT, L.MODEL_CLIP_Z_SHIFT) == (1, 1, 16, 8, 12)
    assert L.LOG_RECORD_FLOATS == 16
    assert optim.WEIGHT_AVG_KINDS == {"swa": 0, "polyak": 1}
    # the two expressions among the header's enumerators, and a #define
    assert (L.CONSTANTS["ARDAE_MODEL_HEAD_MASK"], L.CONSTANTS["ARDAE_MODEL_CLIP_MASK"], L.CONSTANTS["ARDAE_WGRAD_MAX_PROBLEMS"]) == (14, 0xff00, 20)


GOOD_HEADER = """#define ARDAE_N 3
enum { ARDAE_A = 0, ARDAE_B = 1 << 4 };
typedef struct ardae_s { int a, b; const float* p[2]; } ardae_s;
int ardae_f(const ardae_s* s, float* y, /* a comment */ void* stream);
"""


def test_parser_reads_what_the_header_uses():
    consts, structs, protos = L.parse_header(GOOD_HEADER)
    assert consts == {"ARDAE_N": 3, "ARDAE_A": 0, "ARDAE_B": 16}
    assert ctypes.sizeof(structs["ardae_s"]) == 24 and structs["ardae_s"].__name__ == "S"
    assert protos == {"ardae_f": (i32, [("s", ctypes.POINTER(structs["ardae_s"]), "ardae_s"), ("y", vp, "float"), ("stream", vp, "void")])}


BAD_DECLARATIONS = [
    ("int ardae_g(long double x);", "ardae_g"),                                       # an unknown type ...
    ("int ardae_g(int n, short k);", "ardae_g.*short k"),
    ("long ardae_g(int n);", "ardae_g"),                                              # ... also as the result
    ("int ardae_g(ardae_t* t);", "ardae_g.*ardae_t"),                                 # a pointer to an undeclared struct is not a void*
    ("int ardae_g(char** names);", "ardae_g"),
    ("int ardae_g(int (*callback)(int), int n);", "ardae_g"),                         # a function pointer
    ("typedef struct ardae_t { int a b; } ardae_t;", "ardae_t.*int a b"),              # fields it cannot split
    ("typedef struct ardae_t { void (*f)(void); } ardae_t;", "ardae_t"),
    ("typedef struct ardae_t { float* x, y; } ardae_t;", "ardae_t"),
    ("typedef struct ardae_t { long double x; } ardae_t;", "ardae_t"),
    ("typedef struct ardae_t { int a; } ardae_u;", "ardae_t"),
    ("enum { ARDAE_C = 1 + 1 };", "ARDAE_C"),
    ("int ardae_g(int n) { return n; }", "ardae_g"),                                  # not a declaration of this header's kind
    ("#define ARDAE_X 1.5", "ARDAE_X"),
]


@pytest.mark.parametrize("decl,names", BAD_DECLARATIONS, ids=[f"bad{i}" for i in range(len(BAD_DECLARATIONS))])
def test_parser_refuses_what_it_does_not_recognise(decl, names):
    """It raises and names the declaration; a symbol is never bound loosely (to c_void_p) or skipped."""
    with pytest.raises(ValueError, match=names):
        L.parse_header(GOOD_HEADER + decl + "\nint ardae_h(int n);\n")


def test_call_helper_checks_arguments_before_anything_runs(monkeypatch):
    """The converter's refusals, on CPU tensors: every check runs before the stream is fetched and before the library is entered."""
    import types
    import torch
    fetched = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: fetched.append(1) or types.SimpleNamespace(cuda_stream=0))
    f32, i64t = torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float64 on cpu"):
        L.call("ardae_gather_rows", f32.double(), None, 4, 2, None)
    with pytest.raises(TypeError, match="expected a float32 tensor on the GPU, got torch.float32 on cpu"):      # right dtype, wrong device
        L.call("ardae_gather_rows", f32, None, 4, 2, None)
    with pytest.raises(TypeError, match="expected a int64 tensor on the GPU, got torch.int32"):
        L.call("ardae_gather_rows", None, i64t.int(), 4, 2, None)
    with pytest.raises(TypeError, match="expected a int64 tensor on the GPU, got torch.int64 on cpu"):
        L.call("ardae_gather_rows", None, i64t, 4, 2, None)
    with pytest.raises(TypeError, match="ardae_gather_rows takes 6 arguments"):
        L.call("ardae_gather_rows", None, None, 4, 2, None, None, None)                  # one too many
    with pytest.raises(TypeError, match="ardae_gather_rows takes 6 arguments"):
        L.call("ardae_gather_rows", None, None, 4, 2)                                    # two too few
    with pytest.raises(TypeError, match="ardae_cdae_param_floats takes 1 arguments, got 0"):
        L.query("ardae_cdae_param_floats")                                               # no stream parameter: nothing is optional
    with pytest.raises(ctypes.ArgumentError, match="CdaeDesc"):
        L.query("ardae_cdae_param_floats", L.ModelDesc())                                # the wrong struct: argtypes holds a typed pointer
    assert not fetched
    # a missing trailing stream is NOT an error: the call goes through (to the library's own validation, which runs before any HIP call),
    # and its error carries the entry point's name
    with pytest.raises(ValueError, match="^ardae_pack_weight: "):
        L.call("ardae_pack_weight", None, 0, 0, 0, 0, None)
    assert fetched == [1]
    with pytest.raises(ValueError, match="^ardae_pack_weight: "):
        L.call("ardae_pack_weight", None, 0, 0, 0, 0, None, None)                        # ... and so does an explicit one
    assert fetched == [1]
    # values: a struct goes by reference, tensors without a dtype rule (the host-side RCCL id) go as their address, numbers as they are
    cd = L.CdaeDesc(0, 8, 8, 64, 3, 2)
    assert L.query("ardae_cdae_param_floats", cd) == L.lib().ardae_cdae_param_floats(ctypes.byref(cd)) > 0
    assert L.query("ardae_cdae_workspace_floats", cd, 4, 8, 1) == L.lib().ardae_cdae_workspace_floats(ctypes.byref(cd), 4, 8, 1) > 0
    assert L.query("ardae_abi_version") == 1
    with pytest.raises(ValueError, match="^ardae_dp_comm_create: "):
        L.call("ardae_dp_comm_create", torch.zeros(128, dtype=torch.uint8), 0, 0, ctypes.c_void_p())      # nranks 0


def test_abi_version_and_error_channel():
    lib = L.lib()
    assert lib.ardae_abi_version() == 1
    a = L.LinearArgs()
    assert lib.ardae_linear(ctypes.byref(a), 0, None) < 0          # argument validation happens before any HIP call
    assert b"empty problem" in lib.ardae_last_error()
    with pytest.raises(ValueError):
        L.check(lib.ardae_pack_weight(None, 0, 0, 0, 0, None, None))


def _linear_args(M, K, Nout, epi):
    """A valid call of ardae_linear for `epi` on arbitrary non-null, 16-byte aligned addresses (never launched: every use adds a defect)."""
    a = L.LinearArgs()
    a.M, a.Nout, a.nsrc, a.act = M, Nout, 1, L.ACT["softplus"]
    a.src[0].x, a.src[0].ld, a.src[0].K, a.src[0].wp = 1 << 20, K, K, 2 << 20
    a.Y, a.ldY = 3 << 20, Nout
    if epi in (L.EPI_DACT, L.EPI_CHAIN):
        a.S, a.ldS = 4 << 20, Nout
    if epi == L.EPI_CHAIN:
        a.R, a.ldR, a.Y2, a.ldY2 = 5 << 20, Nout, 6 << 20, Nout
    if epi == L.EPI_DAE_LOSS:
        a.sigma, a.eps, a.ldeps, a.tile_loss = 7 << 20, 8 << 20, Nout, 9 << 20
    return a


LINEAR_DEFECTS = {      # name -> (epilogue, the defect, the validator's message)
    "empty_M": (0, dict(M=0), "linear: empty problem (M=0"),
    "nsrc_0": (0, dict(nsrc=0), "linear: nsrc must be 1 or 2"),
    "nsrc_3": (0, dict(nsrc=3), "linear: nsrc must be 1 or 2"),
    "ld_below_K": (0, dict(ld=-1), "linear: bad source 0 (K="),
    "null_Y": (1, dict(Y=None), "linear: Y is null"),
    "dact_without_S": (1, dict(S=None), "linear: EPI_DACT needs S"),
    "chain_without_S": (2, dict(S=None), "linear: EPI_CHAIN needs S, R and Y2"),
    "chain_without_R": (2, dict(R=None), "linear: EPI_CHAIN needs S, R and Y2"),
    "chain_without_Y2": (2, dict(Y2=None), "linear: EPI_CHAIN needs S, R and Y2"),
    "chain_act_none": (2, dict(act=0), "linear: unsupported epilogue/activation combination (epi=2 act=0)"),
    "dae_loss_without_sigma": (3, dict(sigma=None), "linear: EPI_DAE_LOSS needs sigma and eps"),
    "act_99": (0, dict(act=99), "linear: unknown activation 99"),
    "dact_act_99": (1, dict(act=99), "linear: unknown activation 99"),
    "epi_99": (99, {}, "linear: unknown epilogue 99"),
    "rowbias_group_0": (0, dict(rowbias=10 << 20, rowbias_ld=256, rows_per_group=0), "linear: rows_per_group must be positive"),
}
# a per-image shape, a ragged one for linear_kernel, and two the wide kernel takes (whole 64-row tiles, K = Nout = 256, 128 and 256 tiles)
LINEAR_DEFECT_SHAPES = [(64, 64, 64), (300, 100, 70), (8192, 256, 256), (16384, 256, 256)]


@pytest.mark.parametrize("shape", LINEAR_DEFECT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("defect", sorted(LINEAR_DEFECTS))
def test_linear_validation_does_not_depend_on_the_kernel_path(defect, shape):
    """launch_linear validates once, before any eligibility rule (csrc/linear.hip::validate_linear): one defect at a time gives a negative
    status and the validator's message whichever kernel the shape would have selected; validation precedes every HIP call."""
    assert (L.EPI_ACT, L.EPI_DACT, L.EPI_CHAIN, L.EPI_DAE_LOSS) == (0, 1, 2, 3)
    epi, change, message = LINEAR_DEFECTS[defect]
    M, K, Nout = shape
    a = _linear_args(M, K, Nout, epi)
    for k, v in change.items():
        if k == "ld":
            a.src[0].ld = K + v
        else:
            setattr(a, k, v)
    lib = L.lib()
    assert lib.ardae_linear(ctypes.byref(a), epi, None) < 0
    assert message.encode() in lib.ardae_last_error(), lib.ardae_last_error()


# packed floats and workspace floats at (B, nz) = (8, 16) for modes 0 .. 3, as the C side gave them before the packed buffers were laid
# out from one pack list (the packed-buffer and workspace layouts are part of no interface, but a change of either is a change of every offset)
MODEL_SIZES = [("mnist", (784, 100, 256, 32, 2), 2, 0, 1656832, [66176, 1735232, 98304, 56256]),
               ("toy", (2, 10, 256, 2, 2), 2, 0, 584192, [73280, 692864, 65536, 76224]),
               ("mnist", (24, 10, 64, 8, 2), 2, 0, 62464, [13248, 124160, 24576, 12608]),
               ("conv", (784, 100, 800, 32, 1), 2, 0, 1450752, [476224, 16308992, 7104448, 476224]),
               ("auxmnist", (784, 100, 300, 32, 2), 2, 0, 2099200, [134016, 2191488, 76800, 134016]),
               ("auxmnist", (24, 10, 48, 8, 3), 2, 0, 58368, [27072, 130176, 18432, 27072]),
               ("auxconv", (784, 100, 800, 32, 1), 2, 0, 2873600, [853632, 18387072, 7481856, 853632]),
               ("resconv", (784, 100, 512, 32, 1), 3, 0, 10086208, [1506112, 77025792, 48908288, 1506112]),
               ("auxresconv", (784, 100, 450, 32, 1), 3, 0, 6869312, [1446592, 76021632, 48892416, 1446592]),
               ("auxtoy", (2, 2, 64, 2, 1), 4, 0, 23552, [4032, 28608, 8192, 4032]),
               # both log-variance clip codes set (z0 head 'hard', z head 'spm4'): two more workspace buffers, same parameters and panels
               ("auxmnist", (784, 100, 300, 32, 2), 2, (1 << L.MODEL_CLIP_Z0_SHIFT) | (6 << L.MODEL_CLIP_Z_SHIFT), 2099200, [138944, 2196416, 76800, 138944]),
               # the ends of the MLP families' layer loops, num_hidden_layers 1 and 4 (auxtoy at 1 is the row above): recorded from a build of
               # the commit BEFORE the stacks and the decoder of these four kinds were written once (csrc/mlp.h), not from that code
               ("mnist", (24, 10, 64, 8, 1), 2, 0, 46080, [12736, 94080, 16384, 12096]),
               ("mnist", (24, 10, 64, 8, 4), 2, 0, 95232, [14272, 184320, 40960, 13632]),
               ("toy", (2, 10, 64, 2, 1), 2, 0, 22528, [10816, 45824, 8192, 10176]),
               ("toy", (2, 10, 64, 2, 4), 2, 0, 99328, [36928, 215168, 32768, 37824]),
               ("auxmnist", (24, 10, 48, 8, 1), 2, 0, 21504, [14016, 55424, 6144, 14016]),
               ("auxmnist", (24, 10, 48, 8, 4), 2, 0, 76800, [33600, 167552, 24576, 33600]),
               ("auxtoy", (2, 2, 64, 2, 4), 4, 0, 97280, [11712, 143808, 32768, 11712])]
# kind 5 at (784, 100, 512, 32, nl): (packed floats, workspace floats at (4, 8), mode 1) per sampler head and nl = 1, 2, 3
RESCONV_HEAD_SIZES = {"res-wn-mlp": [(10086208, 22831104), (11660608, 23456000), (13235008, 24080896)],
                      "mlp": [(7447104, 22141504), (7971392, 22453376), (8495680, 22765248)],
                      "res-mlp": [(10086208, 22829184), (11660608, 23452928), (13235008, 24076672)],
                      "res-wn-mlp-lin": [(10017344, 22810240), (11591744, 23435136), (13166144, 24060032)],
                      "res-mlp-lin": [(10017344, 22808512), (11591744, 23432256), (13166144, 24056000)]}


@pytest.mark.parametrize("kind,args,act,flags,packed,workspace", MODEL_SIZES, ids=[f"{r[0]}-args{i}" for i, r in enumerate(MODEL_SIZES)])
def test_model_layout_matches_c_side(kind, args, act, flags, packed, workspace):
    spec = layout.model_spec(kind, *args)
    _, total = layout.offsets(spec)
    d = L.ModelDesc(KIND_IDS[kind], *args, act, flags)
    if kind == "resconv":       # every sampler head of ivae_ardae.py's --model resconv* choices, one to three hidden layers
        for et, code in layout.RESCONV_HEADS.items():
            for nl in (1, 2, 3):
                _, tot = layout.offsets(layout.model_spec(kind, *args[:4], nl, enc_type=et))
                dd = L.ModelDesc(5, *args[:4], nl, 3, code << L.MODEL_HEAD_SHIFT)
                assert L.lib().ardae_model_param_floats(ctypes.byref(dd)) == tot, (et, nl)
                assert (L.lib().ardae_model_packed_floats(ctypes.byref(dd)),
                        L.lib().ardae_model_workspace_floats(ctypes.byref(dd), 4, 8, 1)) == RESCONV_HEAD_SIZES[et][nl - 1], (et, nl)
    assert L.lib().ardae_model_param_floats(ctypes.byref(d)) == total
    assert L.lib().ardae_model_packed_floats(ctypes.byref(d)) == packed > total
    assert [L.lib().ardae_model_workspace_floats(ctypes.byref(d), 8, 16, mode) for mode in range(4)] == workspace


# packed floats and workspace floats at (B, S) = (4, 8) without / with gradients, recorded like MODEL_SIZES
@pytest.mark.parametrize("kind,args,packed,workspace", [("grad", (32, 32, 256, 3), 1081600, (104576, 753024)), ("res", (32, 32, 1024, 6), 35849216, (817280, 19596480)),
                                                        ("grad", (2, 2, 256, 3), 1069312, (102656, 735744)), ("grad", (32, 32, 512, 4), 5833216, (274560, 3477120))],
                         ids=["grad-args0", "res-args1", "grad-args2", "grad-args3"])
def test_cdae_layout_matches_c_side(kind, args, packed, workspace):
    spec = layout.cdae_spec(kind, *args)
    _, total = layout.offsets(spec)
    d = L.CdaeDesc(0 if kind == "grad" else 1, *args, 2)
    assert L.lib().ardae_cdae_param_floats(ctypes.byref(d)) == total
    assert L.lib().ardae_cdae_packed_floats(ctypes.byref(d)) == packed
    assert tuple(L.lib().ardae_cdae_workspace_floats(ctypes.byref(d), 4, 8, g) for g in (0, 1)) == workspace


# the unconditional kinds (2 / 3): parameter floats, packed floats and workspace floats at (B, S) = (4, 8) without / with gradients, recorded like
# MODEL_SIZES (these kinds share the layout, workspace and gradient-list code of kinds 0 / 1: what they do NOT take of it is pinned here)
DAE_SIZES = [("grad", (2, 64, 2), 4481, 10816, (8384, 21120)), ("grad", (2, 64, 3), 8641, 19008, (12480, 33536)),
             ("grad", (2, 256, 2), 67073, 141568, (32960, 133056)), ("grad", (2, 256, 3), 132865, 272640, (49344, 231872)),
             ("grad", (32, 64, 2), 6401, 12352, (10304, 24960)), ("grad", (32, 64, 3), 10561, 20544, (14400, 37376)),
             ("grad", (32, 256, 2), 74753, 147712, (34880, 142656)), ("grad", (32, 256, 3), 140545, 278784, (51264, 241472)),
             ("res", (2, 64, 2), 4546, 13376, (4288, 13056)), ("res", (2, 64, 3), 8706, 21568, (6336, 21376)),
             ("res", (2, 256, 2), 67330, 151808, (16576, 100608)), ("res", (2, 256, 3), 133122, 282880, (24768, 183040)),
             ("res", (32, 64, 2), 8416, 16448, (6208, 18816)), ("res", (32, 64, 3), 12576, 24640, (8256, 27136)),
             ("res", (32, 256, 2), 82720, 164096, (18496, 117888)), ("res", (32, 256, 3), 148512, 295168, (26688, 200320))]


@pytest.mark.parametrize("kind,args,params,packed,workspace", DAE_SIZES, ids=[f"{r[0]}-d{r[1][0]}-h{r[1][1]}-L{r[1][2]}" for r in DAE_SIZES])
def test_dae_layout_matches_c_side(kind, args, params, packed, workspace):
    d_in, h, nl = args
    _, total = layout.offsets(layout.dae_spec(kind, d_in, h, nl))
    d = L.CdaeDesc(2 if kind == "grad" else 3, d_in, 0, h, nl, 2)
    assert L.lib().ardae_cdae_param_floats(ctypes.byref(d)) == total == params
    assert L.lib().ardae_cdae_packed_floats(ctypes.byref(d)) == packed
    assert tuple(L.lib().ardae_cdae_workspace_floats(ctypes.byref(d), 4, 8, g) for g in (0, 1)) == workspace


def test_survey_parameter_counts():
    """839 472 / 543 489 (cfg #2), 271 386 / 528 129 (cfg #1), 2 923 521 (cfg #4 cDAE), 17 943 584 (cfg #5 cDAE)."""
    tot = lambda spec: layout.offsets(spec)[1]
    assert tot(layout.model_spec("mnist", 784, 100, 256, 32, 2)) == 839472
    assert tot(layout.cdae_spec("grad", 32, 32, 256, 3)) == 543489
    assert tot(layout.model_spec("toy", 2, 10, 256, 2, 2)) == 271386
    assert tot(layout.cdae_spec("grad", 2, 2, 256, 3)) == 528129
    assert tot(layout.cdae_spec("grad", 32, 32, 512, 4)) == 2923521
    assert tot(layout.model_spec("conv", 784, 100, 800, 32, 1)) == 757773
    assert tot(layout.cdae_spec("res", 32, 32, 1024, 6)) == 17943584
    # the reference's own parameter counts of the two residual-conv models (oracle/gen_golden.py asserts names and shapes against them)
    assert tot(layout.model_spec("resconv", 784, 100, 512, 32, 1)) == 2961487
    assert tot(layout.model_spec("auxresconv", 784, 100, 450, 32, 1)) == 2151637


def test_modules_refuse_cpu_execution():
    """No silent fallback: the HIP path is the only path."""
    import torch
    m = ardae_amd.MNISTIPVAE(input_dim=24, noise_dim=10, h_dim=64, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.encode(torch.zeros(2, 24), std=0)
    c = ardae_amd.MLPGradCARDAE(input_dim=8, context_dim=8, std=1., h_dim=64, num_hidden_layers=3, nonlinearity="softplus")
    with pytest.raises(RuntimeError, match="no CPU path"):
        c(torch.zeros(2, 3, 8), torch.zeros(2, 1, 8))
    with pytest.raises(NotImplementedError):
        ardae_amd.MLPGradCARDAE(input_dim=8, context_dim=8, h_dim=64, num_hidden_layers=3, nonlinearity="softplus", noise_type="laplace")
    with pytest.raises(NotImplementedError):
        ardae_amd.ToyIPVAE(enc_type="scale")


def test_state_dict_roundtrip_keeps_flat_views():
    import torch
    m = ardae_amd.MNISTIPVAE(input_dim=24, noise_dim=10, h_dim=64, num_hidden_layers=2, nonlinearity="softplus", enc_type="concat", z_dim=8)
    sd = {k: torch.randn_like(v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    off = 0
    for n, p in m.named_parameters():
        assert p.data_ptr() == m.flat_params().data_ptr() + 4 * off      # still views of the one flat buffer
        assert torch.equal(p, sd[n])
        off += p.numel()
    m2 = m.double().float()                                               # _apply keeps the views linked
    assert all(p.data_ptr() >= m2.flat_params().data_ptr() for p in m2.parameters())


def test_argument_validation_of_the_step_entry_points():
    """Error behaviour of the entry points a caller can misuse (all checks run before any HIP call, so no GPU is needed):
    negative status + a message on the error channel; nothing is launched, nothing is written."""
    lib = L.lib()
    md = L.ModelDesc(0, 24, 10, 64, 8, 2, 2)
    conv = L.ModelDesc(2, 784, 100, 800, 32, 1, 2)
    cd = L.CdaeDesc(0, 8, 8, 64, 3, 2)
    one = ctypes.c_void_p(64)                     # any non-null address: validation must fail before it is dereferenced
    big = ctypes.c_size_t(1 << 40)

    def fails(rc, fragment):
        assert rc < 0
        assert fragment.encode() in lib.ardae_last_error(), lib.ardae_last_error()

    # empty / oversized batches
    fails(lib.ardae_cdae_loss_grads(ctypes.byref(cd), one, one, one, one, one, one, 0, 8, one, big, one, one, None, None), "bad batch")
    fails(lib.ardae_cdae_loss_grads(ctypes.byref(cd), one, one, one, one, one, one, 1 << 20, 1 << 12, one, big, one, one, None, None), "bad batch")
    # workspace smaller than ardae_*_workspace_floats asks for
    fails(lib.ardae_cdae_loss_grads(ctypes.byref(cd), one, one, one, one, one, one, 4, 8, one, ctypes.c_size_t(16), one, one, None, None),
          "workspace too small")
    fails(lib.ardae_model_encode_pair(ctypes.byref(md), one, one, one, one, 4, 8, one, ctypes.c_size_t(16), one, one, 0, None), "workspace too small")
    # encode_pair: phase out of range, missing noise for the phases that need it
    fails(lib.ardae_model_encode_pair(ctypes.byref(md), one, one, one, one, 4, 8, one, big, one, one, 7, None), "phase")
    fails(lib.ardae_model_encode_pair(ctypes.byref(md), one, one, one, None, 4, 8, one, big, one, one, 2, None), "null pointer")
    # the split backward exists for the MLP models only
    fails(lib.ardae_model_vae_backward_decoder(ctypes.byref(conv), one, one, one, one, 4, 1, 1.0, 1.0, one, big, None), "conv model")
    fails(lib.ardae_model_vae_backward_sampler(ctypes.byref(conv), one, one, one, one, 4, 1, one, 1.0, one, big, one, 0.0, None), "conv model")
    # unknown network kinds / activations (0 = none and anything beyond swish)
    for bad_act in (0, 7):
        bad = L.CdaeDesc(0, 8, 8, 64, 3, bad_act)
        assert lib.ardae_cdae_workspace_floats(ctypes.byref(bad), 4, 8, 1) == 0
        fails(lib.ardae_cdae_pack(ctypes.byref(bad), one, one, None), "unknown activation")
    assert lib.ardae_cdae_workspace_floats(ctypes.byref(L.CdaeDesc(0, 8, 8, 64, 3, 1)), 4, 8, 1) > 0      # relu in mlp-grad: --cdae-nonlin's default
    assert lib.ardae_cdae_param_floats(ctypes.byref(L.CdaeDesc(5, 8, 8, 64, 3, 2))) == 0
    # weight-gradient batches: problem count and shapes
    probs = (L.WgradProblem * 1)()
    fails(lib.ardae_wgrad_batch(probs, 0, None), "problems per batch")
    fails(lib.ardae_wgrad_batch(probs, 1, None), "empty problem")


def test_engine_batch_validation_rules():
    """what ArdaeEngine.step / the phase entry points accept as a batch (checked before any pointer reaches a kernel).
    The rules are host logic, so they are exercised here on CPU tensors against a stand-in for the engine's fields."""
    import types
    import torch
    from ardae_amd.engine import ArdaeEngine
    eng = types.SimpleNamespace(B=4, dev=torch.device("cuda", 0), model=types.SimpleNamespace(input_dim=24))
    check = lambda x: ArdaeEngine._check_batch(eng, x, "step")
    good = torch.zeros(4, 24)
    with pytest.raises(ValueError, match="on cuda:0"):
        check(good)                                               # everything right but the device
    with pytest.raises(ValueError, match="batch_size=4"):
        check(torch.zeros(3, 24))                                 # ragged last batch of a loader without drop_last
    with pytest.raises(ValueError, match="batch_size=4"):
        check(torch.zeros(4, 25))
    with pytest.raises(ValueError, match="batch_size=4"):
        check(torch.zeros(1, 24).expand(4, 24)[:1])
    with pytest.raises(ValueError, match="contiguous"):
        check(torch.zeros(4, 48)[:, ::2])                         # strided view
    with pytest.raises(ValueError, match="contiguous"):
        check(torch.zeros(24, 4).t())
    with pytest.raises(ValueError, match="float32"):
        check(good.double())
    with pytest.raises(TypeError):
        check([[0.0] * 24] * 4)
    with pytest.raises(ValueError, match="on cuda:0"):
        check(torch.zeros(4, 1, 4, 6))                            # image-shaped batches pass the shape rule


def test_host_and_in_step_philox_offsets_are_disjoint():
    """host-side draws (rng.normal / uniform, data.*, model.generate / logprob) and the engine's in-step draws share one
    seed; their Philox offsets must never coincide.  In-step offsets are RNG_STRIDE * step + k < 2^63, host offsets have bit 63 set."""
    from ardae_amd import rng
    from ardae_amd.engine import ArdaeEngine
    rng.manual_seed(7, 0)
    host = [rng._next_offset() for _ in range(40)]
    assert all(o & rng.HOST_STREAM for o in host) and len(set(host)) == 40
    assert [o & ~rng.HOST_STREAM for o in host] == list(range(40))
    in_step = {ArdaeEngine.RNG_STRIDE * step + k for step in range(1, 10_000, 97) for k in range(ArdaeEngine.RNG_STRIDE)}
    assert max(in_step) < rng.HOST_STREAM and not (in_step & set(host))
    assert rng.get_state() == {"seed": 7, "offset": 40}           # the host counter itself (what the engine checkpoint stores)
    rng.manual_seed(7, 40)
    assert rng._next_offset() == rng.HOST_STREAM | 40


def test_activation_names_follow_get_nonlinear_func():
    """utils/models.py:14-32: relu, elu, tanh, softplus, csoftplus (= softplus; evaluated in the accurate form), leaky_relu, swish - every
    name get_nonlinear_func knows constructs; anything else is refused by the host classes."""
    import torch
    import ardae_amd as net
    assert L.ACT["csoftplus"] == L.ACT["softplus"] == 2 and L.ACT["relu"] == 1
    assert {L.ACT[k] for k in ("elu", "tanh", "leaky_relu", "swish")} == {3, 4, 5, 6}
    x = torch.linspace(-30, 30, 2001, dtype=torch.float64)
    from oracle import ardae_oracle as O
    # log(exp(x) + 1) is softplus; its literal fp32 evaluation only loses the tail below ~1e-7 (1 + e^x rounds to 1)
    assert torch.allclose(O.act("csoftplus")(x.float()), O.act("softplus")(x.float()), rtol=1e-6, atol=2e-7)
    net.MLPGradCARDAE(input_dim=2, context_dim=2, h_dim=16, num_hidden_layers=1, nonlinearity="swish")
    net.ToyIPVAE(input_dim=2, noise_dim=2, h_dim=16, z_dim=2, nonlinearity="swish", enc_type="concat")
    with pytest.raises(NotImplementedError):
        net.MLPGradCARDAE(input_dim=2, context_dim=2, h_dim=16, num_hidden_layers=1, nonlinearity="gelu")
    with pytest.raises(NotImplementedError):
        net.ToyIPVAE(input_dim=2, noise_dim=2, h_dim=16, z_dim=2, nonlinearity="gelu", enc_type="concat")
    # the reference's class defaults (tanh) construct
    net.MLPGradCARDAE(input_dim=2, context_dim=2, h_dim=16, num_hidden_layers=1)
    net.ToyIPVAE(input_dim=2, noise_dim=2, h_dim=16, z_dim=2, enc_type="concat")


def test_three_piece_cut_is_exact():
    """csrc/wgrad_x9.hip::cut3, restated in numpy: h = the top 16 bits of x, m = the top 16 bits of x - h, l = x - h - m.  Both subtractions are
    exact and h + m + l == x bit for bit for EVERY finite fp32 value (a million random bit patterns plus edge cases: all 24 significand bits
    set, powers of two, tiny and huge magnitudes, zeros).  For |x| >= 2^-100 the remainder l has at most 8 significand bits - its low half is
    zero by itself, i.e. it is a bf16 value as it stands and nothing is lost when the kernel keeps only its high half; below that (pieces in
    the denormal range, |x| < ~1e-30) the kernel's l loses its low half when it is a denormal: less than 2^-133 in absolute terms, far below an
    fp32 underflow."""
    import numpy as np
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    x = bits.view(np.float32)
    x = x[np.isfinite(x)]
    edge = np.array([0.0, -0.0, 1.0, -1.0, 1.9999999, -1.9999999, 3.4e38, -3.4e38, 1.2e-38, 1e-30, 16777215.0, 0.1, 1.0 / 3.0], dtype=np.float32)
    x = np.concatenate([x, edge])
    hi = lambda v: (v.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    h = hi(x)
    r1 = (x - h).astype(np.float32)
    assert np.array_equal(r1.astype(np.float64), x.astype(np.float64) - h.astype(np.float64))          # exact
    m = hi(r1)
    l = (r1 - m).astype(np.float32)
    assert np.array_equal(l.astype(np.float64), r1.astype(np.float64) - m.astype(np.float64))          # exact
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    normal = np.abs(x) >= np.float32(2.0 ** -100)
    assert np.all((l[normal].view(np.uint32) & np.uint32(0xffff)) == 0)                                 # l is a bf16 value as it stands
    lost = np.abs(l.astype(np.float64) - hi(l).astype(np.float64))                                     # what keeping only l's high half drops
    assert np.all(lost[normal] == 0) and np.all(lost < 2.0 ** -133)
