"""ctypes binding of libsgan_hip.so, read from include/sgan_hip.h at import: the header is the one statement of the C ABI and
this module holds no second copy of it.  There is NO fallback: if the library is missing or a call fails, or the
header holds a declaration the reader does not understand, this raises."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# SGAN_HIP_LIB: diagnostics only (e.g. an -DSG_ABLATE build of the same sources, hence of the same header)
LIB_PATH = os.environ.get("SGAN_HIP_LIB") or os.path.join(_HERE, "csrc", "libsgan_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sgan_hip.h")      # csrc/Makefile: ../../include/sgan_hip.h


class SganError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_POINTEES = ("void", "char", "unsigned char")      # besides the scalars and the structs: what a pointer may point at
_RESTYPES = {"int": C.c_int, "int64_t": C.c_int64, "constchar*": C.c_char_p}      # keyed without white space
_FIELD_RENAMES = {"in": "inp"}      # the one Python keyword among the fields
# structs that live in device memory: the binding passes their address, so a pointer to one is a c_void_p like any device pointer
_DEVICE_STRUCTS = ("sgan_lbfgs_state", "sgan_diffaug_rec")
# (function, parameter) -> argtype, where the caller hands over a ctypes object of the host and the type says which
_ARG_OVERRIDES = {
    ("sgan_stream_device", "device_id"): C.POINTER(C.c_int32),      # byref(c_int32()): an out-parameter on the host
    ("sgan_profile_read", "name"): C.POINTER(C.c_char_p),           # likewise
    ("sgan_profile_read", "ms"): C.POINTER(C.c_float),              # likewise
    ("sgan_zero_multi", "ptrs"): C.POINTER(C.c_void_p),             # a host (c_void_p * n) array
    ("sgan_zero_multi", "bytes"): C.POINTER(C.c_int64),             # a host (c_int64 * n) array
    ("sgan_diffaug_draw", "shapes"): C.POINTER(C.c_int32),          # a host (c_int32 * 2 n) array
}
# bound by their return type alone, as they always were: no row in SIGNATURES
_RESTYPE_ONLY = ("sgan_version", "sgan_last_error", "sgan_last_kernel")

_PREPROCESSOR = re.compile(r"^[ \t]*#[^\n]*", re.M)
_DEFINE = re.compile(r"\s*#\s*define\s+(SGAN_\w+)(.*)")
_INT_EXPR = re.compile(r"(?:\s*(?:0[xX][0-9a-fA-F]+|\d+|<<|[()|+*-]))+\s*")      # all the header uses; C and Python agree on precedence
_TYPEDEF = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*;)\s*\}\s*(\w+)\s*;")
_PROTOTYPE = re.compile(r"(const\s+char\s*\*|int64_t|int)\s+(sgan_\w+)\s*\(([^()]*)\)\s*;")
_EXTERN_C = re.compile(r'extern\s+"C"\s*\{|\}')      # the two ends of the extern "C" bracket
_DECLARATION = re.compile(r"\s*([\w\s*]*[\s*])(\w+)\s*((?:\[\d+\])?)\s*")      # type, name, [N]
_DECLARATOR = re.compile(r"\s*(\w+)\s*((?:\[\d+\])?)\s*")
_SPACE = re.compile(r"\s*")


def read_header(text, name="sgan_hip.h"):
    """(defines, structs, prototypes) of a header in the style of include/sgan_hip.h.
    defines: {SGAN_X: int} for every `#define SGAN_X <integer constant expression>`; a define without a value (the include guard)
    is not a constant and is left out; any other value -- a float, a string, a macro with arguments -- is refused.
    structs: {C name: ctypes.Structure subclass}; prototypes: {function: (restype, [(parameter, argtype)])}, both in header order.
    The other preprocessor lines and the extern "C" bracket are skipped; everything else must be a typedef'd struct or a prototype
    of these forms, or SganError names the line."""
    def blank(m):
        return " " + "\n" * m.group().count("\n")
    code = re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)      # comments out, every line keeps its number
    defines, structs, prototypes = {}, {}, {}

    def fail(pos, what):
        line = code.count("\n", 0, pos) + 1
        raise SganError(f"{name}:{line}: cannot read this {what}: {text.splitlines()[line - 1].strip()!r}")

    def pieces(m, group, sep):
        """(piece, where its first word starts) of a match group split at `sep`."""
        at = m.start(group)
        for piece in m.group(group).split(sep):
            yield piece, at + len(piece) - len(piece.lstrip())
            at += len(piece) + len(sep)

    def declaration(decl, pos, typed, what):
        """'const float* w' -> ('w', c_void_p, ''): name, ctypes type and array suffix of a parameter or a field's first declarator.
        A pointer to one of the `typed` structs keeps its type; every other pointer is an address."""
        m = _DECLARATION.fullmatch(decl)
        if not m:
            fail(pos, what)
        words = [w for w in re.findall(r"\w+|\*", m.group(1)) if w != "const"]
        stars, base = words.count("*"), " ".join(w for w in words if w != "*")
        if stars == 0 and base in _SCALARS:
            return m.group(2), _SCALARS[base], m.group(3)
        if stars == 1 and base in typed:
            return m.group(2), C.POINTER(structs[base]), m.group(3)
        if stars >= 1 and (base in _SCALARS or base in _POINTEES or base in structs):
            return m.group(2), C.c_void_p, m.group(3)
        fail(pos, what + " (type)")

    for m in _PREPROCESSOR.finditer(code):
        d = _DEFINE.fullmatch(m.group())
        if d and d.group(2).strip():
            try:
                if not _INT_EXPR.fullmatch(d.group(2)):
                    raise ValueError
                defines[d.group(1)] = int(eval(d.group(2), {"__builtins__": {}}))      # digits, parentheses, | + * - << and nothing else
            except (ValueError, SyntaxError, ArithmeticError, TypeError):
                fail(m.start(), "integer define")
    code = _PREPROCESSOR.sub(blank, code)
    pos = _SPACE.match(code).end()
    while pos < len(code):
        m = _EXTERN_C.match(code, pos) or _TYPEDEF.match(code, pos) or _PROTOTYPE.match(code, pos)
        if not m:
            fail(pos, "declaration")
        if m.re is _TYPEDEF:
            if m.group(1) != m.group(3):
                fail(pos, "typedef")
            fields = []
            for decl, at in list(pieces(m, 2, ";"))[:-1]:
                first, *more = decl.split(",")
                fname, ftype, dim = declaration(first, at, structs, "field")
                if more and ftype is C.c_void_p:      # `float* a, b`: refused, not guessed
                    fail(at, "field")
                for d in [_DECLARATOR.fullmatch(fname + dim)] + [_DECLARATOR.fullmatch(x) for x in more]:
                    if not d:
                        fail(at, "field")
                    fields.append((_FIELD_RENAMES.get(d.group(1), d.group(1)), ftype * int(d.group(2)[1:-1]) if d.group(2) else ftype))
            structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
        elif m.re is _PROTOTYPE:
            typed = [s for s in structs if s not in _DEVICE_STRUCTS]
            args = []
            for decl, at in ([] if m.group(3).strip() == "void" else pieces(m, 3, ",")):
                pname, ptype, dim = declaration(decl, at, typed, "parameter")
                if dim:
                    fail(at, "parameter")
                args.append((pname, _ARG_OVERRIDES.get((m.group(2), pname), ptype)))
            prototypes[m.group(2)] = (_RESTYPES["".join(m.group(1).split())], args)
        pos = _SPACE.match(code, m.end()).end()
    return defines, structs, prototypes


with open(HEADER_PATH) as _f:
    DEFINES, STRUCTS, _PROTOTYPES = read_header(_f.read(), HEADER_PATH)
for _fn, _p in _ARG_OVERRIDES:
    if _p not in dict(_PROTOTYPES.get(_fn, (None, []))[1]):
        raise SganError(f"_ARG_OVERRIDES names {_fn}({_p}), which {HEADER_PATH} does not declare")

# name -> argtypes, and name -> restype for what does not return an int status
SIGNATURES = {n: [t for _, t in args] for n, (_, args) in _PROTOTYPES.items() if n not in _RESTYPE_ONLY}
RESTYPES = {n: res for n, (res, _) in _PROTOTYPES.items() if res is not C.c_int}

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = (DEFINES["SGAN_ACT_" + n] for n in ("NONE", "RELU", "LRELU", "TANH"))
MATH_F32, MATH_BF16X3, MATH_BF16X1 = (DEFINES["SGAN_MATH_" + n] for n in ("F32", "BF16X3", "BF16X1"))
FACTD_SIG1, FACTD_SIG2, FACTD_MSE = (DEFINES["SGAN_FACTD_" + n] for n in ("SIG1", "SIG2", "MSE"))
SEGHEAD_SOFTMAX, SEGHEAD_SIGMOID = DEFINES["SGAN_SEGHEAD_SOFTMAX"], DEFINES["SGAN_SEGHEAD_SIGMOID"]
CONV, CONVT = DEFINES["SGAN_CONV"], DEFINES["SGAN_CONVT"]

NormDesc, NormFinaliseJob, ConvDesc = STRUCTS["sgan_norm_desc"], STRUCTS["sgan_norm_finalise_job"], STRUCTS["sgan_conv_desc"]
GaussJob, ConvFwdJob, ConvDgradJob = STRUCTS["sgan_gauss_job"], STRUCTS["sgan_conv_fwd_job"], STRUCTS["sgan_conv_dgrad_job"]
WtSeg, ConvWgradJob, NormBwdJob = STRUCTS["sgan_wt_seg"], STRUCTS["sgan_conv_wgrad_job"], STRUCTS["sgan_norm_bwd_job"]
GanLossJob, FactdLossJob, BnRunningDesc = STRUCTS["sgan_gan_loss_job"], STRUCTS["sgan_factd_loss_job"], STRUCTS["sgan_bn_running_desc"]
AdamSeg, EmaSeg, DiffaugJob = STRUCTS["sgan_adam_seg"], STRUCTS["sgan_ema_seg"], STRUCTS["sgan_diffaug_job"]

_lib = None


def lib():
    """Load (once) and return the ctypes library; raise if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SganError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C supervised-gan_amd/csrc`.  There is no CPU/PyTorch fallback for this path.")
        # libsgan_hip.so needs libamdhip64.so.N.  PyTorch-ROCm ships its own copy (and its own HSA runtime); whichever copy is
        # mapped first serves the whole process.  If the system copy came first, torch's HSA runtime and the system HIP runtime
        # would be mixed and the first kernel launch fails with "no ROCm-capable device is detected" -- so torch goes first.
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = RESTYPES.get(name, C.c_int)
        for name in _RESTYPE_ONLY:
            getattr(l, name).restype = RESTYPES[name]
        _lib = l
    return _lib


def check(rc, what):
    if rc != 0:
        raise SganError(f"{what} failed ({rc}): {lib().sgan_last_error().decode()}")
