"""CPU tests of util.split_cells, the host yardstick of the cell-splitting stage (include/sgan_hip.h, "splitting merged cells"), on
hand-built planes whose answers are known, and of the equivalence of its two definitions on random planes: the synchronous rounds
and the order-free form (geodesic distance to the cores, smallest label among the nearest)."""
import heapq
import os
import sys

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import split_ref as R  # noqa: E402
from supervised_gan_amd import util  # noqa: E402

EIGHT = np.ones((3, 3))
NB = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]


def _cells(wall):
    return ndimage.label(~wall, structure=EIGHT)[1]


def _core_labels(wall, rsq):
    """0 off the cores, else 1 + the smallest raster index of the pixel's core component (sgan_ccl_label's numbering)."""
    H, W = wall.shape
    comp, n = ndimage.label(~wall & (util.edt_sq(wall) >= rsq), structure=EIGHT)
    out = np.zeros((H, W), dtype=np.int64)
    for k in range(1, n + 1):
        out[comp == k] = 1 + int(np.flatnonzero(comp.ravel() == k)[0])
    return out


def rounds_form(wall, rsq, max_rounds):
    """The synchronous rounds, pixel by pixel: an unlabelled free pixel takes the smallest label among its 8 labelled neighbours of
    the round before."""
    H, W = wall.shape
    L = _core_labels(wall, rsq)
    for _ in range(max_rounds):
        new = L.copy()
        for y in range(H):
            for x in range(W):
                if not wall[y, x] and L[y, x] == 0:
                    near = [L[y + dy, x + dx] for dy, dx in NB if 0 <= y + dy < H and 0 <= x + dx < W and L[y + dy, x + dx] > 0]
                    if near:
                        new[y, x] = min(near)
        if (new == L).all():
            break
        L = new
    return L


def order_free_form(wall, rsq, max_rounds):
    """The order-free definition: per core component one breadth-first search through the free pixels gives its geodesic distance
    to every pixel; g(p) is the minimum over the components, L(p) the smallest label among those that attain it, 0 beyond the budget."""
    H, W = wall.shape
    cores = _core_labels(wall, rsq)
    far = 1 << 40
    g = np.full((H, W), far, dtype=np.int64)
    L = np.zeros((H, W), dtype=np.int64)
    for label in sorted(set(cores[cores > 0].tolist())):      # ascending: a later, larger label never replaces an equal distance
        dist = np.full((H, W), far, dtype=np.int64)
        heap = [(0, int(y), int(x)) for y, x in np.argwhere(cores == label)]
        for _, y, x in heap:
            dist[y, x] = 0
        heapq.heapify(heap)
        while heap:
            d, y, x = heapq.heappop(heap)
            if d > dist[y, x]:
                continue
            for dy, dx in NB:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and not wall[yy, xx] and d + 1 < dist[yy, xx]:
                    dist[yy, xx] = d + 1
                    heapq.heappush(heap, (d + 1, yy, xx))
        better = dist < g
        g[better], L[better] = dist[better], label
    L[g > max_rounds] = 0
    return L


def _no_two_labels_touch(L, out):
    """After the cut no two free 8-adjacent pixels carry different nonzero labels."""
    H, W = L.shape
    F = np.where(out, 0, L)
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        a = F[0:H - dy, max(0, -dx):W - max(0, dx)]
        b = F[dy:H, max(0, dx):W + min(0, dx)]
        if ((a > 0) & (b > 0) & (a != b)).any():
            return False
    return True


def test_two_discs_are_cut_at_the_neck_and_only_between_the_two_radii():
    """Two discs of radius 9, centres 14 apart: the neck is 11 pixels wide, its centre pixel exactly 6 from the wall.  split_rsq 37
    (the smallest radius^2 above the neck's 36, see split_ref.two_discs) gives two cores and exactly two cells; at 36 the neck's
    centre is still core under d >= split_rsq and joins them; 1 makes every free pixel core; 400 leaves no core at all."""
    wall = R.two_discs()
    assert _cells(wall) == 1 and wall[0].all() and wall[-1].all() and wall[:, 0].all() and wall[:, -1].all()
    d = util.edt_sq(wall)
    assert d[11, 18] == 36 and d[11, 11] >= 81 and d[11, 25] >= 81      # the neck's centre, the two discs' centres
    out, counts = util.split_cells(wall, 37)
    assert counts[0] == 2 and counts[1] > 0 and counts[4] == 0 and _cells(out) == 2, counts
    assert (out >= wall).all() and counts[1] == int((out & ~wall).sum()) and counts[2] == int((~wall).sum())
    sizes = np.bincount(ndimage.label(~out, structure=EIGHT)[0].ravel())[1:]
    assert abs(int(sizes[0]) - int(sizes[1])) <= counts[1], sizes      # cut down the middle
    for rsq, cores in ((36, 1), (1, 1), (400, 0)):
        out, counts = util.split_cells(wall, rsq)
        assert counts[0] == cores and counts[1] == 0 and (out == wall).all(), (rsq, counts)


def test_a_cell_without_a_core_is_untouched():
    wall = np.ones((12, 30), dtype=bool)
    wall[1:4, 1:29] = False              # three rows high: d <= 2 everywhere, no core at split_rsq 9
    wall[5:11, 1:29] = False
    wall[7:9, 14:16] = True              # a pillar in the lower cell; that cell keeps cores to its left and right
    out, counts = util.split_cells(wall, 9)
    L = util.split_labels(wall, 9)[0]
    assert (L[1:4] == 0).all() and (out[1:4] == wall[1:4]).all()
    assert counts[0] >= 2 and counts[1] > 0 and counts[2] == int((~wall[5:11]).sum())      # the lower cell is labelled, and cut


def test_planes_without_wall_and_without_free_pixels_come_back_unchanged():
    for wall in (np.zeros((9, 13), dtype=bool), np.ones((9, 13), dtype=bool)):
        for rsq in (1, 9):
            out, counts = util.split_cells(wall, rsq)
            assert (out == wall).all() and counts.tolist() == [0, 0, 0, 0, 0, 1]


def test_equal_distance_ties_go_to_the_smaller_label():
    wall = R.tie_plane()
    L, cores, rounds, last = util.split_labels(wall, 4)
    left, right = 1 + 3 * 15 + 2, 1 + 3 * 15 + 12      # the two rooms' centre pixels are their cores
    assert cores == 2 and sorted(set(L[L > 0].tolist())) == [left, right] and not last
    assert L[3, 7] == left and (L[3, 3:8] == left).all() and (L[3, 8:12] == right).all()      # (3, 7): 4 steps from either core
    out, counts = util.split_cells(wall, 4)
    assert np.argwhere(out & ~wall).tolist() == [[3, 7]] and counts[1] == 1      # cut seen from the left member of the pair


def test_a_short_budget_leaves_the_far_part_unlabelled_and_uncut():
    wall = R.corridor(40)
    L, cores, rounds, last = util.split_labels(wall, 4, 3)
    assert cores == 1 and rounds == 3 and last
    assert (L[2, 1:6] > 0).all() and (L[2, 6:45] == 0).all()      # the core, the room around it, then two corridor pixels
    out, counts = util.split_cells(wall, 4, 3)
    assert (out == wall).all() and counts.tolist() == [1, 0, 9 + 2, 3, 1, 1]
    out, counts = util.split_cells(wall, 4, 64)
    assert counts.tolist() == [1, 0, int((~wall).sum()), 42, 0, 1]
    two = np.concatenate([wall, wall[:, ::-1]], axis=1)      # a room at either end of one corridor of 82 pixels
    two[2, 44:48] = False
    out, counts = util.split_cells(two, 4, 3)
    assert counts[0] == 2 and counts[1] == 0 and counts[4] == 1 and (out == two).all()      # the floods have not met: no cut
    out, counts = util.split_cells(two, 4, 64)
    assert counts[1] == 1 and counts[4] == 0 and _cells(out) == 2


def test_the_spiral_and_the_lobes_behave_as_the_gpu_tests_assume():
    wall = R.plane("spiral", 97, 130) > 0.5
    assert _cells(wall) == 1
    L, cores, rounds, last = util.split_labels(wall, 9, 4096)
    assert cores == 1 and 64 < rounds < 4096 and not last and ((L > 0) == ~wall).all()
    assert util.split_cells(wall, 9, 64)[1][4] == 1 and util.split_cells(wall, 9, 9)[1][4] == 1
    wall = R.plane("lobes", 96, 112) > 0.5
    assert _cells(wall) == 1 and not wall[31, 47] and not wall[32, 48] and not wall[31, 48] and not wall[32, 47]
    out, counts = util.split_cells(wall, 25)
    assert counts[0] == 2 and _cells(out) == 2 and all(30 <= y <= 33 and 46 <= x <= 49 for y, x in np.argwhere(out & ~wall))


@pytest.mark.parametrize("seed", range(6))
def test_rounds_and_order_free_form_agree_on_random_planes(seed):
    rng = np.random.RandomState(300 + seed)
    H, W = (13, 17) if seed % 2 else (16, 11)
    density = (0.08, 0.2, 0.35)[seed % 3]
    wall = rng.rand(H, W) < density
    for rsq in (1, 2, 4, 5):
        for budget in (1, 2, 64):
            a, b = rounds_form(wall, rsq, budget), order_free_form(wall, rsq, budget)
            assert (a == b).all(), (seed, rsq, budget)
            L = util.split_labels(wall, rsq, budget)[0]
            assert (L == a).all(), (seed, rsq, budget)
            out, counts = util.split_cells(wall, rsq, budget)
            assert _no_two_labels_touch(L, out) and counts[1] == int((out & ~wall).sum()) and counts[2] == int((L > 0).sum())


def test_random_planes_cut_something():
    """The equivalence above is not about planes on which nothing happens."""
    cut = 0
    for seed in range(6):
        rng = np.random.RandomState(300 + seed)
        H, W = (13, 17) if seed % 2 else (16, 11)
        wall = rng.rand(H, W) < (0.08, 0.2, 0.35)[seed % 3]
        cut += sum(int(util.split_cells(wall, rsq)[1][1]) for rsq in (1, 2, 4, 5))
    assert cut > 0


def test_options_give_the_library_its_parameters():
    from supervised_gan_amd import options
    from types import SimpleNamespace as NS
    assert options.split_params(NS()) == (0, 64)
    assert options.split_params(NS(clean_split=3.0, clean_split_rounds=16)) == (9, 16)
    assert options.split_params(NS(clean_split=1.5, clean_split_rounds=64)) == (2, 64)
    assert options.clean_params(NS(clean_split=3.0)) == (0, 0, 0)
    ok = dict(clean_close=0.0, clean_min_wall=0, clean_min_cell=0, clean_split=3.0, clean_split_rounds=64)
    options.check_clean_options(NS(**ok))
    for bad in (dict(clean_split=-1.0), dict(clean_split=0.5), dict(clean_split=65.0), dict(clean_split=float("nan")),
                dict(clean_split_rounds=0), dict(clean_split_rounds=4097)):
        with pytest.raises(ValueError):
            options.check_clean_options(NS(**dict(ok, **bad)))
