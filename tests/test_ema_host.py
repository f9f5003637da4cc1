"""--ema_decay without a GPU: the fp64 reference of the averaging kernel (ema_ref.py) and two mutations of it, the options, the
exported symbol, and the arena ranges optim.WeightEMA pairs for two generators built on the CPU."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ema_ref import T_MAX, ema_bound, ema_decay_at, ema_ref  # noqa: E402


def _seq(k, n=7, seed=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), [rng.standard_normal(n) for _ in range(k)]


def test_decay_zero_gives_the_last_p():
    s0, ps = _seq(4)
    s, t = ema_ref(s0, ps, 0.0, False)
    assert np.array_equal(s, ps[-1]) and t == 4


def test_decay_one_gives_the_initial_shadow():
    s0, ps = _seq(4)
    s, t = ema_ref(s0, ps, 1.0, False)
    assert np.array_equal(s, s0) and t == 4


def test_constant_p_is_a_fixed_point():
    s0, _ = _seq(0)
    for warmup in (False, True):
        s, _ = ema_ref(s0, [s0] * 5, 0.75, warmup)
        assert np.array_equal(s, s0)


def test_counter_starts_at_t0_and_saturates():
    s0, ps = _seq(3)
    assert ema_ref(s0, ps, 0.5, True, t0=10)[1] == 13
    assert ema_ref(s0, ps, 0.5, True, t0=T_MAX - 1)[1] == T_MAX


@pytest.mark.parametrize("t", [1, 2, 10, 1000])
def test_warmup_schedule(t):
    for decay in (0.5, 0.999):
        assert ema_decay_at(t, decay, True) == min(decay, (1 + t) / (10 + t))
        assert ema_decay_at(t, decay, False) == decay
    # through the recurrence: one update from shadow 0 towards p 1 leaves 1 - d_t, at the count the update is made with
    s, _ = ema_ref(np.zeros(1), [np.ones(1)], 0.5, True, t0=t - 1)
    assert s[0] == 1.0 - min(0.5, (1 + t) / (10 + t))


def _mutant(off_by_one=False, drop_min=False):
    def decay_at(t, decay, warmup):
        t = t - 1 if off_by_one else t
        w = (1.0 + t) / (10.0 + t)
        return (w if drop_min else min(decay, w)) if warmup else decay
    return decay_at


def test_mutations_are_caught():
    """An off-by-one t fails the t = 1 case, a dropped min the t = 1000 case."""
    assert _mutant()(1, 0.999, True) == ema_decay_at(1, 0.999, True) and _mutant()(1000, 0.999, True) == ema_decay_at(1000, 0.999, True)
    assert _mutant(off_by_one=True)(1, 0.999, True) != ema_decay_at(1, 0.999, True)            # 1/10 against 2/11
    assert _mutant(drop_min=True)(1000, 0.5, True) != ema_decay_at(1000, 0.5, True)            # 1001/1010 against 0.5
    assert _mutant(drop_min=True)(1, 0.5, True) == ema_decay_at(1, 0.5, True)                  # ... which t = 1 would not show


def test_bound_scales_with_updates_and_magnitude():
    s0, ps = _seq(20)
    m = max(np.abs(s0).max(), max(np.abs(p).max() for p in ps))
    assert ema_bound(s0, ps) == 3 * 20 * 2.0 ** -24 * m


# ---- options -------------------------------------------------------------------------------------------------------------------
def _parse(argv):
    from supervised_gan_amd.options import TrainOptions
    return TrainOptions().parse(argv, save=False, verbose=False)


def test_options_default_is_off():
    opt = _parse([])
    assert opt.ema_decay is None and opt.ema_warmup is False and opt.ema_eval is False


def test_options_accept_a_decay():
    opt = _parse(["--ema_decay", "0.999", "--ema_warmup", "--ema_eval"])
    assert opt.ema_decay == 0.999 and opt.ema_warmup and opt.ema_eval
    assert _parse(["--ema_decay", "0"]).ema_decay == 0.0 and _parse(["--ema_decay", "1"]).ema_decay == 1.0


@pytest.mark.parametrize("argv,message", [(["--ema_eval"], "need --ema_decay"), (["--ema_decay", "1.5"], "a decay of 0 .. 1 (got 1.5)"),
                                          (["--ema_decay", "-0.1"], "a decay of 0 .. 1 (got -0.1)"), (["--ema_decay", "nan"], "a decay of 0 .. 1 (got nan)")],
                         ids=["eval_without_decay", "above_one", "negative", "nan"])
def test_options_refuse(argv, message, capsys):
    """Refused by check_ema_options, with its message (argparse's own `unrecognized arguments` would exit as well)."""
    with pytest.raises(SystemExit):
        _parse(argv)
    err = capsys.readouterr().err
    assert message in err and "unrecognized" not in err


def test_test_options_have_use_ema():
    from supervised_gan_amd.options import TestOptions
    assert TestOptions().parse([], save=False, verbose=False).use_ema is False
    assert TestOptions().parse(["--use_ema"], save=False, verbose=False).use_ema is True


# ---- library and plumbing ------------------------------------------------------------------------------------------------------
def test_library_exports_sgan_ema_multi(built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "sgan_ema_multi")
    from supervised_gan_amd import _lib
    assert "sgan_ema_multi" in _lib.SIGNATURES and ctypes.sizeof(_lib.EmaSeg) == 24


def test_merge_ranges():
    from supervised_gan_amd.optim import merge_ranges
    assert merge_ranges([(10, 5), (0, 10), (20, 1)]) == [(0, 15), (20, 1)]
    # with a twin offset two ranges merge only where the twins touch too
    assert merge_ranges([(4, 4, 104), (0, 4, 100), (8, 2, 200)]) == [(0, 8, 100), (8, 2, 200)]


@pytest.mark.parametrize("which,norm", [("unet_128", "batch"), ("deconv", "instance")])
def test_weight_ema_pairs_every_parameter_once(which, norm):
    """Two generators from one define_G call, on the CPU: the paired ranges cover every parameter's storage exactly once, with equal
    lengths on both sides, as the ranges FusedAdam works on; the shadow's parameters are frozen."""
    import torch
    from supervised_gan_amd import networks
    from supervised_gan_amd.optim import FusedAdam, WeightEMA
    mk = lambda: networks.define_G(2, 2, 8, which, norm, False, n_layers_G=5, use_fcn=True, noise_nc=8, gpu_ids=[])      # noqa: E731
    live, shadow = mk(), mk()
    ema = WeightEMA(live, shadow, 0.9, True)
    covered_live, covered_shadow = np.zeros(live._nflat, dtype=np.int64), np.zeros(shadow._nflat, dtype=np.int64)
    for (s, p), (la, loff, sa, soff, n) in zip(ema.segments(), ema._segs):
        assert s.numel() == p.numel() == n and la is live._flat and sa is shadow._flat
        covered_live[loff: loff + n] += 1
        covered_shadow[soff: soff + n] += 1
    want = np.zeros(live._nflat, dtype=np.int64)
    for prm in live.parameters():
        _, off, n = prm._sgan_seg
        want[off: off + n] += 1
    assert want.max() == 1 and np.array_equal(covered_live, want) and np.array_equal(covered_shadow, want)
    assert [(off, n) for _, _, off, n in FusedAdam(live.parameters())._segs] == [(loff, n) for _, loff, _, _, n in ema._segs]
    assert all(not p.requires_grad for p in shadow.parameters()) and all(p.requires_grad for p in live.parameters())
    assert ema._state.dtype == torch.int32 and ema._state.numel() == 4 and ema.count == 0
    with pytest.raises(ValueError):
        WeightEMA(live, shadow, 1.5)
