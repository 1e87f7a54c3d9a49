"""ctypes binding of libardae_hip.so, derived from the C ABI's only description: include/ardae_hip.h.

The HIP library is the product: there is no CPU or eager-PyTorch fallback.  Importing this module parses the header (no library, no
GPU needed); `lib()` raises without a built library; calling into it without a GPU raises from the HIP runtime.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARDAE_LIB") or os.path.join(_HERE, "libardae_hip.so")   # ARDAE_LIB: experiment builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ardae_hip.h")


def debug_knob(name, default=None):
    """Test / experiment switches (ARDAE_GRAPH, ARDAE_OVERLAP, ... and the kernel-selection switches of the library) are honoured
    only together with ARDAE_DEBUG_KNOBS=1: a stray ARDAE_* variable cannot change what a production process runs."""
    if os.environ.get("ARDAE_DEBUG_KNOBS") != "1":
        return default
    return os.environ.get(name, default)


# ---------------------------------------------------------------------------------------------------------------
# The header parser.  It reads THIS header, not C: enum blocks, integer #defines, `typedef struct X { ... } X;` and prototypes over
# the types below.  Anything else is an error that names the declaration - never a loosely bound symbol.
# ---------------------------------------------------------------------------------------------------------------
_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
_DATA_POINTEES = ("float", "int64_t", "void", "unsigned long long")      # pointers that are bound as c_void_p
_TYPE = r"(?:const\s+)?(unsigned long long|\w+)\s*"
_DECL = re.compile(r"\s*(?:enum\s*\{(?P<enum>[^{}]*)\}|typedef\s+struct\s+(?P<tag>\w+)\s*\{(?P<fields>[^{}]*)\}\s*(?P<alias>\w+)|(?P<proto>[^;{}]+?))\s*;")


def _int(expr, where):
    m = re.fullmatch(r"(\w+)(?:\s*<<\s*(\w+))?", expr.strip())
    try:
        return int(m.group(1), 0) << int(m.group(2) or "0", 0)
    except (AttributeError, ValueError):
        raise ValueError(f"ardae_hip.h: {where}: not an integer constant: {expr.strip()!r}") from None


def _struct(tag, body, structs):
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(_TYPE + r"(\*?)\s*(\w+(?:\[\d+\])?(?:\s*,\s*\w+(?:\[\d+\])?)*)", decl)
        if m is None or (m.group(2) and "," in m.group(3)):
            raise ValueError(f"ardae_hip.h: struct {tag}: cannot split the field declaration {decl!r}")
        base, star, names = m.groups()
        if star:
            ctype = ctypes.c_void_p if base in _DATA_POINTEES else None
        else:
            ctype = ctypes.c_char if base == "char" else _SCALARS.get(base) or structs.get(base)
        if ctype is None:
            raise ValueError(f"ardae_hip.h: struct {tag}: unknown type in the field declaration {decl!r}")
        fields += [(name, ctype * int(dim) if dim else ctype) for name, dim in re.findall(r"(\w+)(?:\[(\d+)\])?", names)]
    # ardae_linear_args -> LinearArgs
    return type("".join(w.title() for w in tag.split("_")[1:]), (ctypes.Structure,), {"_fields_": fields})


def _prototype(text, structs):
    """-> name, restype, [(parameter name, ctypes type, pointee or None)]"""
    m = re.fullmatch(_TYPE + r"(\*?)\s*(\w+)\s*\((.*)\)", text, re.S)
    if m is None:
        raise ValueError(f"ardae_hip.h: cannot split the declaration {' '.join(text.split())!r}")
    rbase, rptr, name, plist = m.groups()
    restype = ctypes.c_char_p if (rbase, rptr) == ("char", "*") else None if rptr else _SCALARS.get(rbase)
    if restype is None:
        raise ValueError(f"ardae_hip.h: {name}: unknown return type {rbase + rptr!r}")
    params = []
    for p in ([] if plist.strip() == "void" else plist.split(",")):
        pm = re.fullmatch(_TYPE + r"(\*{0,2})\s*(\w+)", p.strip())
        if pm is None:
            raise ValueError(f"ardae_hip.h: {name}: cannot split the parameter {' '.join(p.split())!r}")
        base, stars, pname = pm.groups()
        if not stars:
            ctype = _SCALARS.get(base)
        elif base in structs and stars == "*":
            ctype = ctypes.POINTER(structs[base])
        elif (base, stars) in (("void", "**"), ("int", "*")):
            ctype = ctypes.POINTER(ctypes.c_void_p if base == "void" else ctypes.c_int)
        else:
            ctype = ctypes.c_void_p if stars == "*" and base in _DATA_POINTEES else None
        if ctype is None:
            raise ValueError(f"ardae_hip.h: {name}: unknown type in the parameter {' '.join(p.split())!r}")
        params.append((pname, ctype, base + stars[1:] if stars else None))
    return name, restype, params


def parse_header(text):
    """-> (constants {name: int}, structs {C name: ctypes.Structure class, in declaration order}, prototypes {name: (restype, params)})"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", " ", text, flags=re.S)            # the extern "C" braces
    consts = {n: _int(v, f"#define {n}") for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    structs, protos, pos = {}, {}, 0
    while text[pos:].strip():
        m = _DECL.match(text, pos)
        if m is None:
            raise ValueError(f"ardae_hip.h: cannot split the declaration starting at {' '.join(text[pos:].split())[:80]!r}")
        pos = m.end()
        if m.group("enum") is not None:
            for item in filter(None, (i.strip() for i in m.group("enum").split(","))):
                n, _, v = item.partition("=")           # (an enumerator without a value is refused: the header numbers all of them)
                consts[n.strip()] = _int(v, f"enum constant {n.strip()}")
        elif m.group("tag"):
            if m.group("tag") != m.group("alias"):
                raise ValueError(f"ardae_hip.h: struct {m.group('tag')} is given the other name {m.group('alias')}")
            structs[m.group("tag")] = _struct(m.group("tag"), m.group("fields"), structs)
        else:
            name, restype, params = _prototype(m.group("proto"), structs)
            protos[name] = (restype, params)
    return consts, structs, protos


with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTS, PROTOTYPES = parse_header(_f.read())

LinSrc, LinearArgs, WgradProblem, CdaeDesc, ModelDesc, ProfileEntry = (STRUCTS["ardae_" + n] for n in (
    "lin_src", "linear_args", "wgrad_problem", "cdae_desc", "model_desc", "profile_entry"))
# every symbol include/ardae_hip.h declares: name -> (restype, argtypes)
EXPORTS = {name: (res, [ctype for _, ctype, _ in params]) for name, (res, params) in PROTOTYPES.items()}

MODEL_NO_CENTER = CONSTANTS["ARDAE_MODEL_NO_CENTER"]      # ardae_model_desc.flags (residual-conv kinds: do_center=False)
MODEL_HEAD_SHIFT = CONSTANTS["ARDAE_MODEL_HEAD_SHIFT"]    # kind 5: sampler-head type in flags bits 1-3 (layout.RESCONV_HEADS)
MODEL_CLIPPED = CONSTANTS["ARDAE_MODEL_CLIPPED"]          # kind 6: MNISTResConvAuxIPVAEClipped (no 'spm4' clip, z0 keeps an unscaled eps0)
# kinds 3 / 7: NormalDistribution.clip_logvar of the z0 / z heads (models/reparam.py:17-41; flags bits 8-11 / 12-15); the header gives
# these codes in a comment only
LOGVAR_CLIP = {None: 0, "none": 0, "hard": 1, "softplus": 2, "spm10": 3, "spm6": 4, "spm5": 5, "spm4": 6, "spm3": 7, "spm2": 8, "tanh": 9, "2tanh": 10}
MODEL_CLIP_Z0_SHIFT, MODEL_CLIP_Z_SHIFT = CONSTANTS["ARDAE_MODEL_CLIP_Z0_SHIFT"], CONSTANTS["ARDAE_MODEL_CLIP_Z_SHIFT"]

# utils/models.py:14-32 (get_nonlinear_func): all seven names; 'csoftplus' = log(exp(x) + 1) is softplus (evaluated in its accurate form)
ACT = {name: CONSTANTS["ARDAE_ACT_" + code] for name, code in (
    ("none", "NONE"), (None, "NONE"), ("relu", "RELU"), ("softplus", "SOFTPLUS"), ("csoftplus", "SOFTPLUS"), ("elu", "ELU"), ("tanh", "TANH"),
    ("leaky_relu", "LEAKY_RELU"), ("swish", "SWISH"))}
LOG_RECORD_FLOATS = CONSTANTS["ARDAE_LOG_RECORD_FLOATS"]
EPI_ACT, EPI_DACT, EPI_CHAIN, EPI_DAE_LOSS = (CONSTANTS["ARDAE_EPI_" + n] for n in ("ACT", "DACT", "CHAIN", "DAE_LOSS"))
WEIGHT_AVG_SWA, WEIGHT_AVG_POLYAK = CONSTANTS["ARDAE_WEIGHT_AVG_SWA"], CONSTANTS["ARDAE_WEIGHT_AVG_POLYAK"]

_lib = None


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                "(or `python -c 'import __graft_entry__ as g; g.build()'`). There is no fallback path.")
        h = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def check(rc, what="ardae call"):
    if rc != 0:
        msg = lib().ardae_last_error().decode("utf-8", "replace")
        if rc < 0:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what}: HIP error {rc}: {msg}")


_dtypes = {}      # "float32" -> torch.float32, filled at first use (torch stays a lazy import)


def _device_ptr(t, dtype):
    want = _dtypes.get(dtype)
    if want is None:
        import torch
        want = _dtypes[dtype] = getattr(torch, dtype)
    if not (t.is_cuda and t.dtype == want):
        raise TypeError(f"expected a {dtype} tensor on the GPU, got {t.dtype} on {t.device}")
    return t.data_ptr()


def ptr(t):
    """Device pointer of an fp32 CUDA(HIP) tensor (or None).  Layout is the caller's business (strided views are passed with their
    leading dimension); the engine validates its batches in ArdaeEngine._check_batch."""
    return None if t is None else ctypes.c_void_p(_device_ptr(t, "float32"))


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------
# call("ardae_X", ...) / query("ardae_X", ...): tensors, descs and numbers in the header's parameter order.  Only data pointers need
# a conversion of their own (None and ctypes objects pass; `argtypes` converts numbers and takes a struct, or a c_int / c_void_p
# out-parameter, by reference where the parameter is a pointer to one).  One plan per entry point, made here once.
# ---------------------------------------------------------------------------------------------------------------
def _typed(dtype):
    return lambda t: _device_ptr(t, dtype) if hasattr(t, "data_ptr") else t


_CONVERT = {"float": _typed("float32"), "int64_t": _typed("int64"),
            # the step state block, stamp slots, the host-side RCCL id: no dtype or device rule
            "void": lambda t: t.data_ptr() if hasattr(t, "data_ptr") else t}
_CONVERT["unsigned long long"] = _CONVERT["void"]
# name -> (per-parameter converter or None, whether the last parameter is `stream`)
_PLANS = {name: (tuple(_CONVERT.get(pointee) for _, _, pointee in params), bool(params) and params[-1][0] == "stream")
          for name, (_, params) in PROTOTYPES.items()}


def _invoke(name, args):
    plan, has_stream = _PLANS[name]
    missing = len(plan) - len(args)
    if missing and not (missing == 1 and has_stream):
        raise TypeError(f"{name} takes {len(plan)} arguments{' (the trailing stream is optional)' if has_stream else ''}, got {len(args)}")
    argv = [a if conv is None else conv(a) for conv, a in zip(plan, args)]
    if missing:
        import torch
        argv.append(torch.cuda.current_stream().cuda_stream)
    return getattr(_lib or lib(), name)(*argv)


def call(name, *args):
    """An entry point that returns a status: ValueError (status < 0) / RuntimeError (> 0) carrying its name and the library's message.
    A trailing `stream` parameter may be left out: PyTorch's current stream."""
    check(_invoke(name, args), name)


def query(name, *args):
    """An entry point that returns a value (*_floats, *_ok, *_eligible, ardae_wgrad_splits, ...)."""
    return _invoke(name, args)


def profile_report(max_entries=64):
    """Per-kernel (name, calls, total_ms, flops, bytes) since ardae_profile_enable(1); synchronises and clears the log."""
    buf = (ProfileEntry * max_entries)()
    n = query("ardae_profile_report", buf, max_entries)
    return [dict(name=buf[i].name.decode(), calls=buf[i].calls, total_ms=buf[i].total_ms, flops=buf[i].flops, bytes=buf[i].bytes)
            for i in range(min(n, max_entries))]
