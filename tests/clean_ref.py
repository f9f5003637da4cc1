"""What the tests of the cleaning stage share (test_clean_host.py, test_hip_clean.py): the input planes, the parameter sets and the
host yardstick's answers, each computed once per process and never written to.

Planes are float32 [H, W], wall where > 0.5.  cell_map is the flagship input: Voronoi walls two pixels thick with 1- to 3-pixel gaps
punched into them and a few specks inside the cells."""
import functools

import numpy as np

SHAPES = ((1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (97, 131))      # where tiles, column segments and waves end
BIG = (257, 255)                                                        # more than one EDT carry, several CCL tile rows
NOISE = ("noise05", "noise30", "noise60")
SPECIAL = ("empty", "full", "edge_values")
RSQS = (1, 2, 9, 100)


def _ro(a):
    a.setflags(write=False)
    return a


def cell_map(H, W, seed=0, sites=None, gaps=None, specks=None):
    """bool [H, W]: the walls between the Voronoi cells of random sites (a pixel is wall when one of its right / lower neighbours
    within two pixels belongs to another cell), `gaps` square holes of 1 .. 3 pixels cut into them, `specks` blobs of 1 .. 3 wall
    pixels added inside the cells."""
    rng = np.random.RandomState(1000 + seed)
    sites = max(2, H * W // 400) if sites is None else sites
    ys, xs = rng.randint(0, H, sites), rng.randint(0, W, sites)
    yy, xx = np.mgrid[0:H, 0:W]
    owner = ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).argmin(axis=-1)
    wall = np.zeros((H, W), dtype=bool)
    for dy, dx in ((0, 1), (0, 2), (1, 0), (2, 0)):
        a, b = owner[:H - dy, :W - dx], owner[dy:, dx:]
        wall[:H - dy, :W - dx] |= a != b
    on = np.argwhere(wall)
    for k in range(min(len(on), max(3, sites // 2) if gaps is None else gaps)):
        y, x = on[rng.randint(len(on))]
        g = 1 + k % 3
        wall[y:y + g, x:x + g] = False
    off = np.argwhere(~wall)
    for k in range(min(len(off), max(3, sites // 2) if specks is None else specks)):
        y, x = off[rng.randint(len(off))]
        wall[y, x:x + 1 + k % 3] = True
    return wall


@functools.lru_cache(maxsize=None)
def plane(name, H, W, seed=0):
    rng = np.random.RandomState(7919 * H + 31 * W + seed)
    if name.startswith("noise"):
        p = (rng.rand(H, W) < int(name[5:]) / 100.0).astype(np.float32)
    elif name == "cell_map":
        p = cell_map(H, W, seed).astype(np.float32)
    elif name == "empty":
        p = np.zeros((H, W), dtype=np.float32)
    elif name == "full":
        p = np.ones((H, W), dtype=np.float32)
    elif name == "edge_values":      # NaN and an exact 0.5 are not wall; the next float above 0.5 is
        values = np.array([np.nan, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 0.0, 1.0, -np.inf, np.inf, 0.49999997], dtype=np.float32)
        p = values[rng.randint(0, len(values), (H, W))]
    else:
        raise KeyError(name)
    return _ro(p)


@functools.lru_cache(maxsize=None)
def want(name, H, W, close_rsq, min_wall, min_cell, seed=0):
    """util.clean_wall of the named plane: (bool [H, W], the six counts as a list)."""
    from supervised_gan_amd import util
    mask, counts = util.clean_wall(plane(name, H, W, seed), close_rsq, min_wall, min_cell)
    return _ro(mask), counts.tolist()


def _areas(mask):
    """The distinct areas of the 8-connected components of a bool mask, ascending."""
    from scipy import ndimage
    labels, n = ndimage.label(mask, structure=np.ones((3, 3)))
    return np.unique(np.bincount(labels.ravel(), minlength=n + 1)[1:])


def _pick(areas):
    """(A, whether a threshold of exactly A removes something): the second-smallest distinct area, so that at A the smallest
    components go and those of area A stay, and at A + 1 those go too; with one distinct area only A + 1 removes anything."""
    return (int(areas[1]), True) if len(areas) > 1 else (int(areas[0]), False)


def scipy_close(wall, rsq):
    """The closing of the issue's definition as two scipy calls with the disk dy^2 + dx^2 <= rsq."""
    from scipy import ndimage
    r = int(np.floor(np.sqrt(rsq)))
    yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
    disk = yy * yy + xx * xx <= rsq
    return ndimage.binary_erosion(ndimage.binary_dilation(wall, structure=disk, border_value=0), structure=disk, border_value=1)


CLOSE_RSQ = 2      # --clean_close 1.5, the 3 x 3 box: the radius of the three-stage case


@functools.lru_cache(maxsize=None)
def cases(name, H, W, seed=0):
    """The cases a plane is cleaned with, as ((close_rsq, min_wall, min_cell), the stages that must change a pixel on the yardstick):
    every close_rsq alone; min_wall and min_cell alone at a component's area A and at A + 1, A taken from the yardstick's own
    labelling so that both sides of the `<` are hit; the three stages together, each area threshold one above the smallest area among
    the components the stage before it left.  A stage must change something whenever it can: the closing on anything but a single
    pixel, a threshold of A when a smaller component exists, a threshold of A + 1 always."""
    from supervised_gan_amd import util
    wall = plane(name, H, W, seed) > 0.5
    out = [((r, 0, 0), (H * W > 1, False, False)) for r in RSQS]
    if wall.any():
        a, below = _pick(_areas(wall))
        out += [((0, a, 0), (False, below, False)), ((0, a + 1, 0), (False, True, False))]
    if not wall.all():
        a, below = _pick(_areas(~wall))
        out += [((0, 0, a), (False, False, below)), ((0, 0, a + 1), (False, False, True))]
    wall1 = util.clean_wall(wall, CLOSE_RSQ, 0, 0)[0]
    if wall1.any():
        mw = int(_areas(wall1)[0]) + 1
        wall2 = util.clean_wall(wall1, 0, mw, 0)[0]
        mc = int(_areas(~wall2)[0]) + 1      # stage 2 removed something, so a free pixel exists
        out.append(((CLOSE_RSQ, mw, mc), (H * W > 1, True, True)))
    return tuple(out)


def stages_changed(counts):
    return (counts[0] > 0, counts[2] > 0, counts[4] > 0)


# The seed of a noise plane where seed 0 leaves a stage nothing to change (found on the CPU; the tests assert the condition again):
# at density 0.05 a row of 70 pixels rarely holds the `wall free wall` a closing of radius 1 needs.
SEEDS = {("noise05", 1, 70): 3, ("noise05", 70, 1): 1}


def seed_of(name, H, W):
    return SEEDS.get((name, H, W), 0)


def inputs(H, W):
    """The named planes of one shape: noise at three densities, the cell map where the shape has room for cells, the special planes."""
    return NOISE + (("cell_map",) if min(H, W) >= 33 else ()) + SPECIAL
