"""The arithmetic-mode switch on the host side (no GPU): the one-plane mode "bf16x1" is known to the C ABI header, to the ctypes
binding, to ops.set_math / math_scope / get_math and to the trainers' --math option; the default stays "bf16x3"."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    with open(os.path.join(ROOT, "include", "sgan_hip.h")) as f:
        m = re.search(rf"#define {name} (\d+)", f.read())
    assert m, name
    return int(m.group(1))


def test_header_constants_match_binding():
    from supervised_gan_amd import _lib
    assert _header_define("SGAN_MATH_F32") == _lib.MATH_F32
    assert _header_define("SGAN_MATH_BF16X3") == _lib.MATH_BF16X3
    assert _header_define("SGAN_MATH_BF16X1") == _lib.MATH_BF16X1
    assert len({_lib.MATH_F32, _lib.MATH_BF16X3, _lib.MATH_BF16X1}) == 3


def test_set_get_scope_roundtrip():
    from supervised_gan_amd import _lib, ops
    prev = ops.get_math()
    try:
        for name, want in (("bf16x1", "bf16x1"), ("bf16", "bf16x1"), ("BF16X1", "bf16x1"), ("f32", "f32"), ("bf16x3", "bf16x3")):
            ops.set_math(name)
            assert ops.get_math() == want
            assert ops.uses_16bit() == (want != "f32")
        ops.set_math("f32")
        with ops.math_scope("bf16"):
            assert ops.get_math() == "bf16x1"
            assert ops.conv_desc(0, 4, 2, 1, 32, 32, 16, 16, 16, 32).math == _lib.MATH_BF16X1
            with ops.math_scope(None):
                assert ops.get_math() == "bf16x1"
        assert ops.get_math() == "f32"
        with pytest.raises(KeyError):
            ops.set_math("fp8")
    finally:
        ops.set_math(prev)


def _load(name, path, package=None):
    """A fresh, private copy of a module from its file (not registered in sys.modules, nothing else in the process changes)."""
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    if package:
        mod.__package__ = package
    spec.loader.exec_module(mod)
    return mod


def test_default_mode_is_still_bf16x3(monkeypatch):
    import supervised_gan_amd  # noqa: F401  (the package the copy's relative imports resolve in)
    monkeypatch.delenv("SGAN_MATH", raising=False)
    ops_default = _load("supervised_gan_amd._ops_default_copy", os.path.join(ROOT, "supervised-gan_amd", "ops.py"), "supervised_gan_amd")
    assert ops_default.get_math() == "bf16x3"


@pytest.mark.parametrize("which", ["TrainOptions", "TestOptions"])
def test_math_option_parses_and_sets_the_mode(which):
    from supervised_gan_amd import ops, options
    prev = ops.get_math()
    cls = getattr(options, which)
    try:
        ops.set_math("bf16x3")
        opt = cls().parse(["--name", "t", "--gpu_ids", "-1", "--math", "bf16x1"], save=False, verbose=False)
        assert opt.math == "bf16x1" and ops.get_math() == "bf16x1"
        ops.set_math("f32")
        opt = cls().parse(["--name", "t", "--gpu_ids", "-1"], save=False, verbose=False)      # unset: the current mode stays
        assert opt.math is None and ops.get_math() == "f32"
        with pytest.raises(SystemExit):
            cls().parse(["--name", "t", "--gpu_ids", "-1", "--math", "fp8"], save=False, verbose=False)
    finally:
        ops.set_math(prev)


def test_kernel_names_of_the_one_plane_instantiations():
    short = _load("_kernel_names_copy", os.path.join(ROOT, "tools", "kernel_names.py")).short
    assert short("void sg_igemm3_kernel<64, 64, 2, 2, false, true, true, true>(SgIgemmParams)") == "sg_igemm3_kernel<64,64,2,2,x1>"
    assert short("void sg_igemm3_kernel<64, 64, 2, 2, false, true, true, false>(SgIgemmParams)") == "sg_igemm3_kernel<64,64,2,2>"
    assert short("sg_igemm3p_kernel<64, 6, false, true, true, 1, true>(SgIgemmParams)") == "sg_igemm3p_kernel<64,s2,x1>"
    assert short("sg_igemm3p_kernel<64, 2, false, true, false, 2, false>(SgIgemmParams)") == "sg_igemm3p_kernel<64>"
    assert short("sg_wgrad3_kernel<64, 64, 2, 2, true, false, true>(SgWgradParams)") == "sg_wgrad3_kernel<64,64,2,2,x1>"
    assert short("sg_bwd_fused_kernel<3, 1, true, false, false, false>(SgIgemmParams, SgWgradParams, int)") == "sg_bwd_fused_kernel"
    assert short("sg_bwd_fused_kernel<3, 1, true, false, true, true>(SgIgemmParams, SgWgradParams, int)") == "sg_bwd_fused_kernel<x1>"
    assert short("sg_bwd_fused_kernel<6, 1, true, true, false, true>(SgIgemmParams, SgWgradParams, int)") == "sg_bwd_fused_kernel<wgrad x1>"
