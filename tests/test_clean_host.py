"""CPU tests of the cleaning stage's host side: util.clean_wall, the yardstick of ops.clean_wall, against scipy restatements of its
three stages and against the properties of the definition; the --clean_* options; the two entry points in the header and the library.
Everything is a mask or an integer: equality, no tolerance."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import clean_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_RSQS = (1, 2, 4, 9, 25)
INPUTS = [("noise05", 23, 31), ("noise30", 40, 17), ("noise60", 33, 65), ("cell_map", 64, 64), ("cell_map", 97, 131), ("noise30", 1, 70),
          ("noise30", 70, 1), ("noise30", 1, 1), ("edge_values", 33, 65)]
EIGHT = np.ones((3, 3))


def _mask(name, H, W):
    return R.plane(name, H, W) > 0.5


@pytest.mark.parametrize("rsq", HOST_RSQS)
def test_closing_equals_the_two_scipy_calls(rsq):
    from supervised_gan_amd import util
    changed = 0
    for name, H, W in INPUTS:
        wall = _mask(name, H, W)
        got, counts = util.clean_wall(R.plane(name, H, W), rsq, 0, 0)
        want = R.scipy_close(wall, rsq)
        assert got.dtype == np.bool_ and np.array_equal(got, want), (name, H, W, rsq, int((got != want).sum()))
        assert counts.tolist() == [int((want & ~wall).sum()), 0, 0, 0, 0, 1]
        changed += counts[0]
    assert changed > 0


def _filter_restated(wall, min_wall, min_cell):
    """Stages 2 and 3 written out directly: label, count with bincount, flip the small components."""
    counts = [0, 0, 0, 0]
    if min_wall:
        lab, n = ndimage.label(wall, structure=EIGHT)
        area = np.bincount(lab.ravel(), minlength=n + 1)
        drop = [k for k in range(1, n + 1) if area[k] < min_wall]
        counts[0], counts[1] = len(drop), int(sum(area[k] for k in drop))
        wall = wall & ~np.isin(lab, drop)
    if min_cell:
        lab, n = ndimage.label(~wall, structure=EIGHT)
        area = np.bincount(lab.ravel(), minlength=n + 1)
        fill = [k for k in range(1, n + 1) if area[k] < min_cell]
        counts[2], counts[3] = len(fill), int(sum(area[k] for k in fill))
        wall = wall | np.isin(lab, fill)
    return wall, counts


@pytest.mark.parametrize("min_wall,min_cell", [(3, 0), (0, 5), (4, 10), (1, 1), (10 ** 6, 0), (0, 10 ** 6)])
def test_area_filters_equal_a_direct_restatement(min_wall, min_cell):
    from supervised_gan_amd import util
    changed = [0, 0]
    for name, H, W in INPUTS:
        wall = _mask(name, H, W)
        got, counts = util.clean_wall(wall, 0, min_wall, min_cell)
        want, want_counts = _filter_restated(wall, min_wall, min_cell)
        assert np.array_equal(got, want), (name, H, W)
        assert counts.tolist() == [0] + want_counts + [1]
        changed[0] += counts[2]
        changed[1] += counts[4]
    assert (changed[0] > 0) == (min_wall > 1) and (changed[1] > 0) == (min_cell > 1)      # a threshold of 1 removes nothing


def test_properties_of_the_three_stages():
    from supervised_gan_amd import util
    for name, H, W in INPUTS:
        wall = _mask(name, H, W)
        for rsq in HOST_RSQS:
            closed, c = util.clean_wall(wall, rsq, 0, 0)
            assert not (wall & ~closed).any()                                             # extensive
            assert np.array_equal(util.clean_wall(closed, rsq, 0, 0)[0], closed)          # idempotent for a fixed rsq
            assert c[0] == int(closed.sum()) - int(wall.sum())
        w2, c2 = util.clean_wall(wall, 0, 4, 0)
        assert not (w2 & ~wall).any() and c2[2] == int(wall.sum()) - int(w2.sum())        # stage 2 only removes wall
        w3, c3 = util.clean_wall(wall, 0, 0, 10)
        assert not (wall & ~w3).any() and c3[4] == int(w3.sum()) - int(wall.sum())        # stage 3 only adds wall
        # the stages run in the definition's order: the whole call is the three single calls chained, and the counts add up
        full, c = util.clean_wall(wall, 2, 4, 10)
        a, ca = util.clean_wall(wall, 2, 0, 0)
        b, cb = util.clean_wall(a, 0, 4, 0)
        d, cd = util.clean_wall(b, 0, 0, 10)
        assert np.array_equal(full, d) and c.tolist() == [ca[0], cb[1], cb[2], cd[3], cd[4], 1]
        assert int(full.sum()) == int(wall.sum()) + c[0] - c[2] + c[4]
    for H, W in ((1, 1), (5, 9), (33, 65)):
        for rsq in HOST_RSQS:
            for value in (False, True):                                                   # an empty and a full wall are fixed points
                m = np.full((H, W), value)
                got, c = util.clean_wall(m, rsq, 0, 0)
                assert np.array_equal(got, m) and c.tolist() == [0, 0, 0, 0, 0, 1]
    got, c = util.clean_wall(_mask("noise30", 33, 65), 0, 0, 0)                            # nothing asked for: the thresholded plane
    assert np.array_equal(got, _mask("noise30", 33, 65)) and c.tolist() == [0, 0, 0, 0, 0, 1]
    assert util.CLEAN_COUNTS == ('closed_pixels', 'wall_components_removed', 'wall_pixels_removed', 'cells_filled', 'cell_pixels_filled', 'images')


def test_the_closing_joins_a_punched_wall_and_the_border_is_kept():
    """What the stage is for: a one-pixel hole in a straight one-pixel wall merges two cells; the 3 x 3 box (rsq = 2) closes it
    and nothing else, the 4-neighbour plus (rsq = 1) fits through the hole sideways and leaves it; the wall's two ends at the image border
    survive the erosion."""
    from supervised_gan_amd import util
    wall = np.zeros((9, 11), dtype=bool)
    wall[:, 5] = True
    wall[4, 5] = False
    assert ndimage.label(~wall, structure=EIGHT)[1] == 1
    assert np.array_equal(util.clean_wall(wall, 1, 0, 0)[0], wall)
    closed, c = util.clean_wall(wall, 2, 0, 0)
    assert closed[4, 5] and c[0] == 1 and ndimage.label(~closed, structure=EIGHT)[1] == 2 and closed[:, 5].all()


def test_option_parsing():
    from supervised_gan_amd.options import TestOptions, TrainOptions, clean_params
    base = ["--name", "clean_opts", "--gpu_ids", "-1"]
    for options in (TrainOptions, TestOptions):
        opt = options().parse(base, save=False, verbose=False)
        assert (opt.clean_close, opt.clean_min_wall, opt.clean_min_cell) == (0, 0, 0) and clean_params(opt) == (0, 0, 0)
    opt = TestOptions().parse(base + "--clean_close 1.5 --clean_min_wall 4 --clean_min_cell 10".split(), save=False, verbose=False)
    assert clean_params(opt) == (2, 4, 10)
    for r, rsq in (("1", 1), ("2", 4), ("2.9", 8), ("64", 4096), ("0.5", 0)):
        assert clean_params(TrainOptions().parse(base + ["--clean_close", r], save=False, verbose=False))[0] == rsq
    for bad in (["--clean_close", "-1"], ["--clean_close", "64.5"], ["--clean_close", "nan"], ["--clean_min_wall", "-1"],
                ["--clean_min_cell", "-3"]):
        with pytest.raises(SystemExit):
            TrainOptions().parse(base + bad, save=False, verbose=False)
    import types
    assert clean_params(types.SimpleNamespace()) == (0, 0, 0)      # an options object from before the stage


def test_the_header_declares_and_the_library_exports_the_entries(built_lib):
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    assert re.search(r"\bint64_t sgan_clean_workspace\(int32_t H, int32_t W\);", header)
    assert re.search(r"\bint sgan_clean_wall\(const float\* plane, int64_t pix_stride, int32_t H, int32_t W, int32_t close_rsq, int32_t min_wall, "
                     r"int32_t min_cell,\s+float\* out, int64_t\* acc, void\* workspace, int64_t workspace_bytes, int32_t\* dev_err, void\* stream\);", header)
    assert "#define SGAN_CLEAN_COUNTS 6" in header
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "sgan_clean_wall") and hasattr(lib, "sgan_clean_workspace")
    from supervised_gan_amd import _lib, ops
    assert len(_lib.SIGNATURES["sgan_clean_wall"]) == 13 and _lib.RESTYPES["sgan_clean_workspace"] is ctypes.c_int64
    assert len(ops.CLEAN_COUNTS) == 6
    l = _lib.lib()
    # the size query and the refusals that need no device: nothing is launched before the arguments are checked
    assert l.sgan_clean_workspace(64, 64) >= l.sgan_edt_workspace(64, 64) + 3 * 4 * 64 * 64
    assert l.sgan_clean_workspace(0, 5) < 0 and l.sgan_clean_workspace(5, -1) < 0 and l.sgan_clean_workspace(32768, 32768) < 0
    assert l.sgan_clean_wall(None, 1, 4, 4, 1, 0, 0, None, None, None, 0, None, None) == 1 and b"null pointer" in l.sgan_last_error()
