"""What the tests of the cell-splitting stage share (test_split_host.py, test_hip_split.py): the hand-built planes, the shapes and
parameters, and the host yardstick's answers, each computed once per process and never written to.

Planes are float32 [H, W], wall where > 0.5.  The noise, cell-map and special planes are clean_ref's."""
import functools

import numpy as np

import clean_ref as C

# where the flood's 48 x 32 tiles, its 8-pixel halo, the labelling's 64 x 16 tiles and the waves end
SHAPES = ((1, 1), (1, 70), (70, 1), (31, 33), (33, 31), (64, 16), (65, 17), (97, 130))
RSQS = (1, 2, 9, 25)
ROUNDS = (1, 8, 9, 64)
NOISE = C.NOISE
SPECIAL = C.SPECIAL


def _ro(a):
    a.setflags(write=False)
    return a


def two_discs(radius=9, apart=14):
    """bool wall: two overlapping discs of free space (centres `apart` apart on one row) inside a one-pixel wall frame; everything
    outside the discs is wall.  On the column midway between the centres the free rows are dy = -5 .. 5 (49 + 36 > 81), so the
    centre pixel of the neck has distance^2 exactly 36 to the wall: with the contract's d >= split_rsq it is still core at 36, which
    joins the two discs' cores, and 37 is the smallest split_rsq that separates them."""
    H, W = 2 * radius + 5, 2 * radius + apart + 5
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = radius + 2, radius + 2
    free = ((yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius) | ((yy - cy) ** 2 + (xx - cx - apart) ** 2 <= radius * radius)
    return ~free


def corridor(length=40):
    """bool wall [5, length + 6]: a 3 x 3 room at the left end (one core at split_rsq 4) and a one-pixel corridor to the right."""
    wall = np.ones((5, length + 6), dtype=bool)
    wall[1:4, 1:4] = False
    wall[2, 4:length + 5] = False
    return wall


def tie_plane():
    """bool wall [7, 15]: two 3 x 3 rooms joined by a one-pixel corridor of 5 pixels on the middle row; the middle pixel of the
    corridor is reached by both cores in the same round."""
    wall = np.ones((7, 15), dtype=bool)
    wall[2:5, 1:4] = False
    wall[2:5, 11:14] = False
    wall[3, 4:11] = False
    return wall


def spiral(H, W, pitch=4):
    """bool wall [H, W]: a 7 x 7 room in the upper-left corner (the only core at split_rsq 5 .. 16) and, below it, a rectangular
    spiral corridor pitch - 1 = 3 pixels wide between walls one pixel thick, which starts under the room and winds inwards: the flood
    has to walk all of it, a few hundred rounds at 97 x 130."""
    wall = np.ones((H, W), dtype=bool)
    wall[1:8, 1:8] = False
    wall[8, 1:4] = False      # the door from the room to the start of the corridor
    sub = wall[8:]            # the spiral's own frame
    h = H - 8

    def carve(y, x):
        sub[y - 1:y + 2, x - 1:x + 2] = False

    y = x = t = l = 2
    b, r = h - 3, W - 3
    while r - x >= pitch:
        for x in range(x, r + 1):
            carve(y, x)
        if b - y < pitch:
            break
        for y in range(y, b + 1):
            carve(y, x)
        if x - l < pitch:
            break
        for x in range(x, l - 1, -1):
            carve(y, x)
        t += pitch
        if y - t < pitch:
            break
        for y in range(y, t - 1, -1):
            carve(y, x)
        l, r, b = l + pitch, r - pitch, b - pitch
    return wall


def lobes(H=96, W=112, cy=32, cx=48, radius=12):
    """bool wall [H, W]: two square free lobes that touch diagonally at (cy, cx), the corner of four flood tiles (48 x 32 cores),
    through a neck three pixels wide; everything else is wall."""
    wall = np.ones((H, W), dtype=bool)
    wall[cy - 2 * radius:cy, cx - 2 * radius:cx] = False      # the upper-left lobe ends at (cy - 1, cx - 1)
    wall[cy:cy + 2 * radius, cx:cx + 2 * radius] = False      # the lower-right lobe starts at (cy, cx)
    wall[cy - 1, cx] = wall[cy, cx - 1] = False               # the neck
    return wall


@functools.lru_cache(maxsize=None)
def plane(name, H, W, seed=0):
    if name == "spiral":
        return _ro(spiral(H, W).astype(np.float32))
    if name == "lobes":
        return _ro(lobes(H, W).astype(np.float32))
    return C.plane(name, H, W, seed)


@functools.lru_cache(maxsize=None)
def want(name, H, W, split_rsq, max_rounds, seed=0):
    """util.split_cells of the named plane: (bool [H, W], the six counts as a list)."""
    from supervised_gan_amd import util
    mask, counts = util.split_cells(plane(name, H, W, seed), split_rsq, max_rounds)
    return _ro(mask), counts.tolist()


def cuttable(H, W):
    """Whether any plane of this shape can be cut.  A cut needs two cores in one free component.  In a single row or column the
    distance to the wall is a tent over every free run, so the pixels of a run with d >= split_rsq are one interval, one core: the
    1 x 1, 1 x 70 and 70 x 1 shapes never cut, whatever the seed.  Every other shape of SHAPES cuts at seed 0 (found on the CPU; the
    tests assert it again)."""
    return min(H, W) >= 2


def inputs(H, W):
    """The named planes of one shape: noise at three densities, the cell map where the shape has room for cells, the special planes."""
    return NOISE + (("cell_map",) if min(H, W) >= 33 else ()) + SPECIAL
