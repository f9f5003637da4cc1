"""The ctypes binding is read from include/sgan_hip.h (supervised-gan_amd/_lib.py); no GPU.  The C++ compiler judges
the structs and the defines -- sizes, offsets and values of a program that includes the header --, a second, cruder reading of the
prototypes judges SIGNATURES / RESTYPES, and doctored headers show that the reader refuses what it does not understand."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from supervised_gan_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")      # the compiler of tests/test_c_abi_example.py
with open(_lib.HEADER_PATH) as _f:
    HEADER = _f.read()
CODE = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)      # for the crude second readings below: comments out, nothing else done
C_FIELD = {v: k for k, v in _lib._FIELD_RENAMES.items()}


def test_header_is_the_one_the_library_is_built_from():
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "sgan_hip.h"))


def test_compiler_agrees_on_every_struct_and_define(tmp_path):
    """sizeof of every struct, offsetof and size of every field and the value of every SGAN_ define, printed by a program that
    includes the header, against ctypes.sizeof, the ctypes field offsets and DEFINES: exact, nothing left out."""
    struct_bodies = dict(re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}", CODE, flags=re.S))
    define_names = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SGAN_\w+)[ \t]+\S", CODE, flags=re.M)      # a define with a value
    assert list(struct_bodies) == list(_lib.STRUCTS) and len(struct_bodies) >= 17
    assert sorted(define_names) == sorted(_lib.DEFINES) and len(define_names) == len(set(define_names)) >= 80
    src = ['#include <cstddef>', '#include <cstdio>', '#include <type_traits>', '#include "sgan_hip.h"', 'int main() {']
    for name in define_names:
        src.append(f'  static_assert(std::is_integral<decltype({name})>::value, "{name} is not an integer");')
        src.append(f'  std::printf("define {name} %lld\\n", (long long)({name}));')
    for sname, cls in _lib.STRUCTS.items():
        # every declarator of the body is a field of the class: none dropped by the reader (a declarator ends in ',' or ';')
        assert len(cls._fields_) == len(re.findall(r"[,;]", struct_bodies[sname])), sname
        src.append(f'  std::printf("sizeof {sname} %zu\\n", sizeof({sname}));')
        for fname, _ in cls._fields_:
            c = C_FIELD.get(fname, fname)
            src.append(f'  std::printf("field {sname} {fname} %zu %zu\\n", offsetof({sname}, {c}), sizeof((({sname}*)0)->{c}));')
    src += ['  return 0;', '}']
    (tmp_path / "abi.cpp").write_text("\n".join(src) + "\n")
    cxx = next((c for c in (HIPCC, "c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path / "abi")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-I" + os.path.dirname(_lib.HEADER_PATH), str(tmp_path / "abi.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")[:-1]
    want = [f"define {n} {_lib.DEFINES[n]}" for n in define_names]
    for sname, cls in _lib.STRUCTS.items():
        want.append(f"sizeof {sname} {ctypes.sizeof(cls)}")
        want += [f"field {sname} {f} {getattr(cls, f).offset} {getattr(cls, f).size}" for f, _ in cls._fields_]
    assert out == want, [(a, b) for a, b in zip(out, want) if a != b][:10]
    assert ctypes.sizeof(_lib.STRUCTS["sgan_lbfgs_state"]) == 128 and ctypes.sizeof(_lib.STRUCTS["sgan_diffaug_rec"]) == 32


KIND = {ctypes.c_int32: "int32_t", ctypes.c_int64: "int64_t", ctypes.c_uint64: "uint64_t", ctypes.c_float: "float",
        ctypes.c_double: "double"}      # anything else in an argtypes row is a pointer


def test_prototypes_agree_with_a_cruder_reading():
    """Parameter count and scalar kind of every prototype, split at the commas and judged by the last type word, and the return
    type, against SIGNATURES and RESTYPES; the three getters that are bound by their return type alone have no parameters."""
    protos = re.findall(r"(const char\*|int64_t|int)\s+(sgan_\w+)\s*\(([^()]*)\)\s*;", CODE)
    assert len(protos) == len({n for _, n, _ in protos}) >= 130      # the ABI only grows
    assert {n for _, n, _ in protos} == set(_lib.SIGNATURES) | set(_lib._RESTYPE_ONLY)
    for ret, name, params in protos:
        kinds = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = re.findall(r"\w+|\*", p)
            kinds.append("pointer" if "*" in words else {"int": "int32_t"}.get(words[-2], words[-2]))
        if name in _lib._RESTYPE_ONLY:
            assert kinds == [], name
        else:
            assert [KIND.get(t, "pointer") for t in _lib.SIGNATURES[name]] == kinds, name
            assert all(t in KIND or issubclass(t, (ctypes._Pointer, ctypes.c_void_p)) for t in _lib.SIGNATURES[name]), name
        assert _lib.RESTYPES.get(name, ctypes.c_int) is {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}[ret]
    for (fn, param), t in _lib._ARG_OVERRIDES.items():      # an override types a pointer more closely, nothing else
        assert issubclass(t, ctypes._Pointer) and t in _lib.SIGNATURES[fn], (fn, param)


def test_struct_pointers_stay_typed_and_device_structs_are_addresses():
    S = _lib.STRUCTS
    assert _lib.SIGNATURES["sgan_conv_fwd"][0]._type_ is S["sgan_conv_desc"] and _lib.SIGNATURES["sgan_conv_fwd"][3]._type_ is S["sgan_norm_desc"]
    assert dict(S["sgan_conv_fwd_job"]._fields_)["d"]._type_ is S["sgan_conv_desc"] and "inp" in dict(S["sgan_conv_fwd_job"]._fields_)
    assert _lib.SIGNATURES["sgan_lbfgs_advance"][0] is ctypes.c_void_p and _lib.SIGNATURES["sgan_diffaug_multi_fwd"][2] is ctypes.c_void_p
    assert _lib.SIGNATURES["sgan_diffaug_multi_fwd"][0]._type_ is S["sgan_diffaug_job"]
    assert _lib.NormDesc is S["sgan_norm_desc"] and _lib.EmaSeg is S["sgan_ema_seg"]
    from supervised_gan_amd import lbfgs
    assert lbfgs.LbfgsState is S["sgan_lbfgs_state"] and dict(lbfgs.LbfgsState._fields_)["reserved"]._length_ == 8


@pytest.mark.parametrize("after, bad", [
    ("int sgan_stat_replicas(void);", "int sgan_bad(const float* x, size_t n, void* stream);"),      # a type the reader does not know
    ("typedef struct sgan_ema_seg {", "    int32_t flags : 3;"),                                      # a bit-field
    ("#define SGAN_STAT_REPLICAS 8", "#define SGAN_BAD_SCALE 0.5"),                                   # a float among the integer defines
    ("#define SGAN_STAT_REPLICAS 8", "#define SGAN_BAD_MACRO(x) ((x) + 1)"),
    ("int sgan_stat_replicas(void);", "typedef int32_t sgan_bad_t;"),
    ("int sgan_stat_replicas(void);", "void sgan_bad(void);"),
])
def test_reader_refuses_what_it_cannot_read(after, bad):
    """Nothing is skipped silently: the error names the header's line and quotes it.  A define with a float value is refused,
    not left out."""
    lines = HEADER.split("\n")
    k = next(i for i, l in enumerate(lines) if l.startswith(after)) + 1
    doctored = "\n".join(lines[:k] + [bad] + lines[k:])
    with pytest.raises(_lib.SganError) as e:
        _lib.read_header(doctored, "doctored.h")
    assert f"doctored.h:{k + 1}:" in str(e.value) and bad.strip() in str(e.value), str(e.value)
    defines, structs, protos = _lib.read_header(HEADER)      # and the header as it stands reads clean
    assert (defines, list(structs), list(protos)) == (_lib.DEFINES, list(_lib.STRUCTS), list(_lib._PROTOTYPES))
