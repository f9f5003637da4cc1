"""Image and metric helpers of the drivers (util/util.py:15-28, :41-43, :86-128 of the reference): tensor -> uint8 image -> PNG,
the Rand F-score of a binary segmentation, the information score (VInfo) that goes with it, Guo-Hall thinning (the border
thinning both scores are ranked after: `thin`, `compute_thinned_scores`), and the shape statistics of the regions of a map
(`region_table`, the yardstick of the device's sgan_region_stats, and `region_props`, the features derived from its rows), and the
border term of the U-Net loss (`border_weight_map`, the yardstick of the device's sgan_border_weight), and the elastic deformation of
a training crop (`elastic_field`, `elastic_prep`, the yardsticks of the device's sgan_image_prep_elastic), and the geometry of
whole-image inference (`tile_plan`, `tile_window`, `prep_tile_ref`, `blend_tiles_ref`, the yardsticks of sgan_image_prep_tile /
sgan_tile_blend / sgan_tile_finish), and the augmentation of discriminator inputs (`diffaug_params`, `diffaug_ref`,
`diffaug_bwd_ref`, the yardsticks of sgan_diffaug_draw / sgan_diffaug_multi_fwd / sgan_diffaug_multi_bwd), and the photometric
augmentation of a training crop (`photo_draw`, the draw of the feeders; `photo_taps`, `photo_ref`, `photo_bounds`, the yardsticks of
sgan_image_photo)."""
import os
import random

import numpy as np


def tensor2im(image_tensor, imtype=np.uint8):
    """[1, C, H, W] in [-1, 1] -> [H, W, 3] uint8; 1 channel is repeated, 2 channels get a zero blue plane (util.py:15-24)."""
    image_numpy = image_tensor[0].detach().cpu().float().numpy()
    image_numpy = (image_numpy + 1) / 2.0 * 255.0
    if image_numpy.shape[0] == 1:
        image_numpy = image_numpy.repeat(3, 0)
    elif image_numpy.shape[0] == 2:
        image_numpy = np.concatenate((image_numpy, np.zeros((1,) + image_numpy.shape[1:], dtype=image_numpy.dtype)), axis=0)
    return np.transpose(image_numpy, (1, 2, 0)).clip(0, 255).astype(imtype)


def save_image(image_numpy, image_path):
    from PIL import Image
    os.makedirs(os.path.dirname(os.path.abspath(image_path)), exist_ok=True)
    Image.fromarray(image_numpy).save(image_path)


def _label_false_regions(mask):
    """skimage.measure.label(mask, background=1) for a boolean 2-D image: the 8-connected components of the FALSE pixels numbered
    from 1, true pixels = 0 (the reference labels the membrane-free regions of the thresholded maps, util.py:101-102)."""
    from scipy import ndimage
    lab, _ = ndimage.label(~mask, structure=np.ones((3, 3), dtype=np.int32))
    return lab


_THIN_WEIGHTS = np.array([[8, 4, 2], [16, 0, 1], [32, 64, 128]], dtype=np.uint8)      # E = 1, then counter-clockwise: NE N NW W SW S SE


def thin_tables():
    """The two 256-entry deletion tables of Guo-Hall thinning, indexed by the neighbour code (bit k = b[k], b0..b7 = E, NE, N, NW, W,
    SW, S, SE): table[s][code] is True when a set pixel with these neighbours is deleted in sub-iteration s + 1.
        G1: #{i in 0,2,4,6 : not b[i] and (b[i+1] or b[(i+2)%8])} == 1
        G2: min(N1, N2) in {2, 3},  N1 = #{k in 1,3,5,7 : b[k] or b[k-1]},  N2 = #{k in 1,3,5,7 : b[k] or b[(k+1)%8]}
        G3 (sub-iteration 1): not ((b1 or b2 or not b7) and b0);  G3' (sub-iteration 2): not ((b5 or b6 or not b3) and b4)"""
    tables = np.zeros((2, 256), dtype=bool)
    for code in range(256):
        b = [bool((code >> k) & 1) for k in range(8)]
        g1 = sum((not b[i]) and (b[i + 1] or b[(i + 2) % 8]) for i in (0, 2, 4, 6)) == 1
        n1 = sum(b[k] or b[k - 1] for k in (1, 3, 5, 7))
        n2 = sum(b[k] or b[(k + 1) % 8] for k in (1, 3, 5, 7))
        g12 = g1 and min(n1, n2) in (2, 3)
        tables[0, code] = g12 and not ((b[1] or b[2] or not b[7]) and b[0])
        tables[1, code] = g12 and not ((b[5] or b[6] or not b[3]) and b[4])
    return tables


def thin(mask, max_num_iter=None):
    """Guo-Hall thinning of a boolean [H, W] image to one-pixel lines, as skimage.morphology.thin performs it: an iteration is two
    sub-iterations, each of which decides every set pixel from one snapshot of its eight neighbours (outside the image = 0) by
    thin_tables() and then deletes; it stops after the first iteration that deletes nothing, or after max_num_iter iterations.
    Returns (thinned bool [H, W], n_changing = the number of iterations that deleted something).

    skimage is not installed where this was written, so "identical to skimage.morphology.thin" is unverified; what the tests claim
    is that the device kernel (sgan_thin) is identical to THIS function.  The host yardstick of ops.thin; the trainers do not call it."""
    from scipy import ndimage
    m = (np.asarray(mask) != 0).astype(np.uint8)
    assert m.ndim == 2, m.shape
    tables = thin_tables()
    n_changing, it = 0, 0
    while max_num_iter is None or it < max_num_iter:
        before = int(m.sum())
        for table in tables:
            code = ndimage.correlate(m, _THIN_WEIGHTS, mode='constant', cval=0)
            m = m & ~table[code]
        it += 1
        if int(m.sum()) == before:
            break
        n_changing += 1
    return m.astype(bool), n_changing


def border_weight_map(labels, radius, w0, sigma):
    """The border term of the U-Net loss (Ronneberger et al. 2015, eq. 2) of a label map [H, W] (0 = wall, > 0 = a cell id; a
    negative label counts as wall): returns (d1sq, d2sq, bmap), int64, int64 and float64 [H, W].  The host yardstick of
    ops.border_weight; the trainers do not call it.

    For a wall pixel p and a cell L, m_L(p) is the smallest dy^2 + dx^2 over the pixels of L inside the image with dy^2 + dx^2 <=
    radius^2; d1sq(p) <= d2sq(p) are the two smallest m_L(p) over distinct L, -1 where fewer than one / two cells are in range, and
        bmap(p) = w0 exp(-(sqrt(d1sq) + sqrt(d2sq))^2 / (2 sigma^2))
    where both exist, else 0.  Pixels that are not wall get (-1, -1, 0).

    Derivation of the method: the offsets of the disc are walked in ascending d = dy^2 + dx^2, each as one shifted copy of the map
    (padded with wall).  Because d never decreases along the walk, the first time a pixel sees a label L at all it sees it at m_L(p).
    So the first label a pixel sees is a nearest cell, l1, with d1sq = that d; the first label != l1 it sees later is a cell of
    the smallest m_L among the others, with d2sq = that d.  Offsets of equal d may come in any order: which of two equally near
    cells becomes l1 changes, the two numbers do not."""
    lab = np.asarray(labels).astype(np.int64)
    assert lab.ndim == 2 and radius >= 1 and sigma > 0, (lab.shape, radius, sigma)
    lab = np.where(lab < 0, 0, lab)
    H, W = lab.shape
    R = int(radius)
    wall = lab == 0
    pad = np.zeros((H + 2 * R, W + 2 * R), dtype=np.int64)
    pad[R:R + H, R:R + W] = lab
    offsets = sorted((dy * dy + dx * dx, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if 0 < dy * dy + dx * dx <= R * R)
    l1 = np.zeros((H, W), dtype=np.int64)
    d1sq = np.full((H, W), -1, dtype=np.int64)
    d2sq = np.full((H, W), -1, dtype=np.int64)
    for d, dy, dx in offsets:
        seen = pad[R + dy:R + dy + H, R + dx:R + dx + W]
        cell = wall & (seen > 0)
        second = cell & (d1sq >= 0) & (d2sq < 0) & (seen != l1)
        first = cell & (d1sq < 0)
        d2sq[second] = d
        l1[first] = seen[first]
        d1sq[first] = d
    both = d2sq >= 0
    bmap = np.zeros((H, W), dtype=np.float64)
    dist = np.sqrt(d1sq[both].astype(np.float64)) + np.sqrt(d2sq[both].astype(np.float64))
    bmap[both] = float(w0) * np.exp(-dist * dist / (2.0 * float(sigma) ** 2))
    return d1sq, d2sq, bmap


ELASTIC_CLAMP = 127.0      # source pixels: what a component of the elastic field is clamped to


def _catmull_rom_weights(rem, n, dtype):
    """[4, len(rem)] Catmull-Rom (a = -0.5) weights of the four control points around a cell at the fractional position rem / n,
    in `dtype`, operation for operation as the device forms them (csrc/sgan_elastic.hip): t = rem / n and s = (n - rem) / n are two
    correctly rounded divisions of exact integers, and every weight is a product of sums of positive terms:
        w0 = -t s^2 / 2,  w1 = s (s^2 + 3 s t + t^2 / 2),  w2 = t (t^2 + 3 s t + s^2 / 2),  w3 = -t^2 s / 2."""
    t = rem.astype(dtype) / dtype(n)
    s = (n - rem).astype(dtype) / dtype(n)
    ss, st, tt = s * s, s * t, t * t
    return np.stack([(dtype(-0.5) * t) * ss, s * ((ss + dtype(3) * st) + dtype(0.5) * tt), t * ((tt + dtype(3) * st) + dtype(0.5) * ss),
                     (dtype(-0.5) * tt) * s])


def elastic_field(ctrl, n, G, dtype=np.float32, return_abs=False):
    """The displacement field of the elastic deformation, [n, n, 2] in `dtype`, indexed (v, u) = (row, column) of the crop before flip
    and rotation, components (dx, dy) in source pixels.  The host yardstick of the field sgan_image_prep_elastic computes
    (ops.image_prep_elastic's field_out); the trainers do not call it.

    ctrl: [G + 3, G + 3, 2], control point (r, s) at crop coordinate ((s - 1) n / G, (r - 1) n / G).  Per axis, for coordinate u:
    a = u G, cell i = a // n, t = (a % n) / n -- integers and one rounded division.  The field is the Catmull-Rom tensor product of
    control points [j .. j + 3][i .. i + 3], summed row by row (((w0 c0 + w1 c1) + w2 c2) + w3 c3 along s, then the same along r) in
    `dtype`, each component clamped to +-ELASTIC_CLAMP.  float32 follows the device operation for operation (the device may contract
    a product and a sum into one rounding, so the two agree to a few units in the last place, not to the bit); float64 is the
    reference of the field test.  return_abs: also return sum_rs |w_r w_s c_rs| per pixel and component, in float64 from the
    float64 weights -- the magnitude the rounding of the fp32 field is proportional to."""
    dtype = np.dtype(dtype).type
    c = np.asarray(ctrl)
    assert 1 <= G <= 13 and c.shape == (G + 3, G + 3, 2) and n >= 1, (c.shape, G, n)
    a = np.arange(n, dtype=np.int64) * G
    cell, rem = a // n, a % n
    w = _catmull_rom_weights(rem, n, dtype)                                   # [4, n], the same along both axes
    c = c.astype(dtype)
    field = None
    for k in range(4):
        rows = c[cell + k]                                                    # [n(v), G + 3, 2]
        r = w[0][None, :, None] * rows[:, cell]                               # [n(v), n(u), 2]
        for m in range(1, 4):
            r = r + w[m][None, :, None] * rows[:, cell + m]
        field = w[0][:, None, None] * r if k == 0 else field + w[k][:, None, None] * r
    field = np.clip(field, dtype(-ELASTIC_CLAMP), dtype(ELASTIC_CLAMP))
    if not return_abs:
        return field
    w64, c64 = np.abs(_catmull_rom_weights(rem, n, np.float64)), np.abs(np.asarray(ctrl, dtype=np.float64))
    mag = np.zeros((n, n, 2))
    for k in range(4):
        for m in range(4):
            mag += (w64[k][:, None] * w64[m][None, :])[..., None] * c64[cell + k][:, cell + m]
    return field, mag


def _mirror_index(i, N):
    """i folded into [0, N) by reflection about the first and the last pixel, neither repeated (scipy's mode='mirror'); N == 1 -> 0."""
    if N == 1:
        return np.zeros_like(i)
    P = 2 * (N - 1)
    m = np.mod(i, P)
    return np.where(m < N, m, P - m)


def elastic_sample(img, X, Y, nearest_mask):
    """The integer stage of elastic_prep: img [H0, W0, 3] uint8 sampled at the 8.8 fixed-point positions X, Y (int arrays of one
    shape) -> uint8 of that shape + (3,).  A channel whose bit in nearest_mask is clear: bilinear,
        ((256 - fx)(256 - fy) p00 + fx (256 - fy) p01 + (256 - fx) fy p10 + fx fy p11 + 32768) >> 16,  ix = X >> 8, fx = X & 255;
    a channel whose bit is set: the pixel at ((X + 128) >> 8, (Y + 128) >> 8).  Indices are mirrored into the image."""
    img = np.asarray(img)
    H0, W0 = img.shape[:2]
    X, Y = np.asarray(X, dtype=np.int64), np.asarray(Y, dtype=np.int64)
    ix, iy, fx, fy = X >> 8, Y >> 8, X & 255, Y & 255
    xa, xb, ya, yb = _mirror_index(ix, W0), _mirror_index(ix + 1, W0), _mirror_index(iy, H0), _mirror_index(iy + 1, H0)
    num = (((256 - fx) * (256 - fy))[..., None] * img[ya, xa].astype(np.int64) + (fx * (256 - fy))[..., None] * img[ya, xb].astype(np.int64)
           + ((256 - fx) * fy)[..., None] * img[yb, xa].astype(np.int64) + (fx * fy)[..., None] * img[yb, xb].astype(np.int64))
    out = ((num + 32768) >> 16).astype(np.uint8)
    near = img[_mirror_index((Y + 128) >> 8, H0), _mirror_index((X + 128) >> 8, W0)]
    for ch in range(3):
        if (int(nearest_mask) >> ch) & 1:
            out[..., ch] = near[..., ch]
    return out


def elastic_positions(field, x0, y0):
    """(X, Y): the 8.8 fixed-point source positions of an [n, n, 2] fp32 field over the window at (x0, y0): q = rint(field * 256)
    (exact in fp32, ties to even as rintf), X = (x0 + u) 256 + qx, Y = (y0 + v) 256 + qy."""
    field = np.asarray(field)
    assert field.dtype == np.float32 and field.ndim == 3 and field.shape[0] == field.shape[1] and field.shape[2] == 2, (field.shape, field.dtype)
    n = field.shape[0]
    q = np.rint(field * np.float32(256.0)).astype(np.int64)
    v, u = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing='ij')
    return (x0 + u) * 256 + q[..., 0], (y0 + v) * 256 + q[..., 1]


def elastic_prep(img, x0, y0, n, flip, rot, ctrl, G, nearest_mask, field=None):
    """img [H0, W0, 3] uint8 -> float32 [3, n, n]: the crop window at (x0, y0) seen through the elastic field of `ctrl`, then flip,
    rot90, ToTensor and Normalize as the plain pipeline tail.  The host yardstick of ops.image_prep_elastic; the trainers do not
    call it.  `field`: an [n, n, 2] fp32 field to use instead of elastic_field(ctrl, n, G, float32) -- the device's own field read
    back, after which every step is integer and the two agree to the bit."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, (img.shape, img.dtype)
    assert 0 <= x0 and 0 <= y0 and x0 + n <= img.shape[1] and y0 + n <= img.shape[0], (x0, y0, n, img.shape)
    if field is None:
        field = elastic_field(ctrl, n, G, np.float32)
    X, Y = elastic_positions(field, x0, y0)
    c = elastic_sample(img, X, Y, nearest_mask)
    if flip:
        c = c[:, ::-1]
    c = np.rot90(c, rot, axes=(0, 1))                                         # counter-clockwise, as PIL's ROTATE_90
    t = c.astype(np.float32) / np.float32(255.0)                              # ToTensor
    t = (t - np.float32(0.5)) / np.float32(0.5)                               # Normalize((.5,.5,.5), (.5,.5,.5))
    return np.ascontiguousarray(t.transpose(2, 0, 1))


# ---- whole-image inference: overlap tiles, blended seams, D4 averaging.  The geometry every layer reads: the options
# check, the feeder, SegmentationModel.test() and the yardsticks of sgan_image_prep_tile / sgan_tile_blend / sgan_tile_finish ----------
TILE_MAX_RAMP = 64


def tile_geometry_error(L, T, M, R, S, axis='image'):
    """None, or why tiles of side T with margin M, ramp R and stride S cannot cover an axis of length L (L None: the conditions that
    do not involve the image)."""
    if T < 1 or M < 0:
        return "--tile T >= 1 and --tile_margin M >= 0 (got T %d, M %d)" % (T, M)
    if not 1 <= R <= TILE_MAX_RAMP:
        return "--tile_ramp: 1..%d pixels (got %d)" % (TILE_MAX_RAMP, R)
    if not 1 <= S <= T - 2 * M:
        return ("--tile_stride S must lie in 1 .. T - 2 M = %d, so that the non-margin parts of the tiles cover the image "
                "(got S %d with T %d, M %d)" % (T - 2 * M, S, T, M))
    if L is not None and M > L - 1:
        return "--tile_margin %d: a reflection reaches at most %s length - 1 = %d pixels" % (M, axis, L - 1)
    if L is not None and L + 2 * M < T:
        return "--tile %d does not fit the padded %s: length %d + 2 x margin %d = %d" % (T, axis, L, M, L + 2 * M)
    return None


def tile_window(T, M, R):
    """w(i) = clamp(min(i + 1, T - i) - M, 0, R), i = 0 .. T - 1, int64: zero in the margin, a ramp of R pixels, then flat; symmetric,
    so the 2-D weight w(y) w(x) is the same under all 8 flips and rotations."""
    i = np.arange(T, dtype=np.int64)
    return np.clip(np.minimum(i + 1, T - i) - M, 0, R)


def tile_origins(L, T, M, S):
    """Tile origins along an axis of length L: -M, -M + S, ... while the tile ends before L + M, then L + M - T (the last tile is
    shifted back, not padded further); duplicates removed."""
    err = tile_geometry_error(L, T, M, 1, S)
    if err is not None:
        raise ValueError(err)
    o, k = [], -M
    while k + T < L + M:
        o.append(k)
        k += S
    if not o or o[-1] != L + M - T:
        o.append(L + M - T)
    return o


def _tile_weight_sum(L, origins, win):
    s = np.zeros(L, dtype=np.int64)
    for o in origins:
        lo, hi = max(0, o), min(L, o + len(win))
        s[lo:hi] += win[lo - o: hi - o]
    return s


def tile_plan(H, W, T, M, R, S):
    """(oy, ox, Wy, Wx): the tile origins of the rows and of the columns (lists) and the per-axis weight sums Wy [H], Wx [W] (int64,
    > 0 everywhere): Wy(Y) = sum over the row origins o of w(Y - o).  The weight a pixel collects over all passes is the exact integer
    n_tta Wy(Y) Wx(X); it must stay below 2^24, where fp32 holds every integer."""
    err = tile_geometry_error(H, T, M, R, S, 'height') or tile_geometry_error(W, T, M, R, S, 'width')
    if err is not None:
        raise ValueError(err)
    win = tile_window(T, M, R)
    oy, ox = tile_origins(H, T, M, S), tile_origins(W, T, M, S)
    Wy, Wx = _tile_weight_sum(H, oy, win), _tile_weight_sum(W, ox, win)
    assert Wy.min() > 0 and Wx.min() > 0
    if 8 * int(Wy.max()) * int(Wx.max()) >= 1 << 24:
        raise ValueError("tiles overlap so often that a pixel's weight sum 8 x %d x %d is no exact fp32 integer: raise --tile_stride or "
                         "lower --tile_ramp" % (Wy.max(), Wx.max()))
    return oy, ox, Wy, Wx


def tile_passes(oy, ox, tta):
    """The passes of an image in the order they run: tile-row, tile-column, flip 0..1, rot 0..3 -> [(y0, x0, flip, rot)]."""
    d4 = [(f, r) for f in (0, 1) for r in range(4)] if tta else [(0, 0)]
    return [(y0, x0, f, r) for y0 in oy for x0 in ox for f, r in d4]


def _reflect_index(i, L):
    """Index of the padded domain -> the image, mirrored without repeating the edge (F.pad(mode='reflect')): one fold."""
    i = np.asarray(i, dtype=np.int64)
    assert i.min() > -L and i.max() <= 2 * (L - 1), "the window reaches more than length - 1 pixels outside the image"
    i = np.abs(i)
    return np.where(i >= L, 2 * (L - 1) - i, i)


def d4_apply(a, flip, rot):
    """[..., h, w] -> horizontal flip, then rot x 90 degrees counter-clockwise (sg_image_prep_kernel's convention)."""
    if flip:
        a = a[..., ::-1]
    return np.rot90(a, rot, axes=(-2, -1))


def d4_inverse(a, flip, rot):
    """Undoes d4_apply: what a pass computed on a transformed tile, back in the orientation of the window it was cut from."""
    a = np.rot90(a, -rot, axes=(-2, -1))
    return a[..., ::-1] if flip else a


def prep_tile_ref(img_u8, y0, x0, h, w, flip, rot):
    """img [H0, W0, 3] uint8 -> float32 [3, h, w] ([3, w, h] under an odd rot): the h x w window at (y0, x0) of the reflected image,
    the D4 element, ToTensor and Normalize in float32 with sgan_image_prep's operation order.  The host yardstick of
    ops.image_prep_tile, to the bit."""
    img = np.asarray(img_u8)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, (img.shape, img.dtype)
    ys = _reflect_index(y0 + np.arange(h), img.shape[0])
    xs = _reflect_index(x0 + np.arange(w), img.shape[1])
    c = d4_apply(img[ys][:, xs].transpose(2, 0, 1), flip, rot)
    t = c.astype(np.float32) / np.float32(255.0)                              # ToTensor
    t = (t - np.float32(0.5)) / np.float32(0.5)                               # Normalize((.5,.5,.5), (.5,.5,.5))
    return np.ascontiguousarray(t)


def blend_tiles_ref(logits, H, W, T, M, R, S, tta=False, sigmoid=False, return_count=False):
    """The whole-image prediction in float64:

        P[c, Y, X] = (sum over the passes of w(y) w(x) p_pass[c] at the tile pixel that shows (Y, X)) / (n_tta Wy(Y) Wx(X))

    `logits`: one [C, T, T] array per pass in tile_passes' order, or a callable (index, y0, x0, flip, rot) -> that array; p_pass is
    its softmax over the channels (sigmoid: the logistic function of each).  A pass saw its window under d4_apply, so its result goes
    through d4_inverse back to image orientation; what lands outside the image (mirrored territory) is dropped.  return_count: also
    the number of passes that reached each pixel with a non-zero weight, [H, W].  The host yardstick of ops.tile_blend +
    ops.tile_finish."""
    oy, ox, Wy, Wx = tile_plan(H, W, T, M, R, S)
    win = tile_window(T, M, R)
    w2 = np.outer(win, win).astype(np.float64)
    num, count = None, np.zeros((H, W), dtype=np.int64)
    for k, (y0, x0, flip, rot) in enumerate(tile_passes(oy, ox, tta)):
        z = np.asarray(logits(k, y0, x0, flip, rot) if callable(logits) else logits[k], dtype=np.float64)
        assert z.ndim == 3 and z.shape[1:] == (T, T), z.shape
        if sigmoid:
            p = 1.0 / (1.0 + np.exp(-z))
        else:
            e = np.exp(z - z.max(axis=0, keepdims=True))
            p = e / e.sum(axis=0, keepdims=True)
        p = d4_inverse(p, flip, rot)
        if num is None:
            num = np.zeros((z.shape[0], H, W), dtype=np.float64)
        ya, yb, xa, xb = max(0, y0), min(H, y0 + T), max(0, x0), min(W, x0 + T)
        wgt = w2[ya - y0: yb - y0, xa - x0: xb - x0]
        num[:, ya:yb, xa:xb] += wgt * p[:, ya - y0: yb - y0, xa - x0: xb - x0]
        count[ya:yb, xa:xb] += wgt > 0
    P = num / ((8 if tta else 1) * np.outer(Wy, Wx).astype(np.float64))
    return (P, count) if return_count else P


REGION_COLS =('area', 'xmin', 'xmax', 'ymin', 'ymax', 'sum_x', 'sum_y', 'sum_xx', 'sum_yy', 'sum_xy', 'boundary', 'root', 'image',
               'edges', 'zero14', 'zero15')
REGION_PROPS = ('area', 'centroid_x', 'centroid_y', 'equivalent_diameter', 'extent', 'mu20', 'mu02', 'mu11', 'major_axis_length',
                'minor_axis_length', 'eccentricity', 'orientation', 'compactness', 'touches_border')


def region_table(free_mask, image_ordinal=0):
    """One row of 16 exact int64 per 8-connected region of the TRUE pixels of `free_mask` [H, W], in scipy.ndimage.label's order
    (ascending smallest raster index): the host yardstick of ops.region_stats on ops.ccl_label's map of the same pixels.
    Columns (REGION_COLS), x = column, y = row: 0 area; 1..4 xmin, xmax, ymin, ymax (inclusive); 5..9 sum x, sum y, sum x^2,
    sum y^2, sum x y; 10 boundary pixels (at least one 4-neighbour not in the region, outside the image counts as not in it);
    11 root = smallest raster index; 12 image_ordinal; 13 exposed edges = (pixel, N/S/E/W) pairs whose neighbour is not in the
    region; 14, 15 zero.  All sums are taken in int64 (np.add.reduceat over the pixels sorted by region), never through floats."""
    from scipy import ndimage
    free = np.asarray(free_mask) != 0
    assert free.ndim == 2, free.shape
    H, W = free.shape
    lab, k = ndimage.label(free, structure=np.ones((3, 3), dtype=np.int32))
    table = np.zeros((k, 16), dtype=np.int64)
    if k == 0:
        return table
    ys, xs = np.nonzero(lab)                                   # raster order
    region = lab[ys, xs].astype(np.int64) - 1
    order = np.argsort(region, kind='stable')                  # within a region the raster order is kept
    starts = np.searchsorted(region[order], np.arange(k))
    x, y = xs[order].astype(np.int64), ys[order].astype(np.int64)
    pad = np.zeros((H + 2, W + 2), dtype=lab.dtype)
    pad[1:-1, 1:-1] = lab
    mine = pad[1:-1, 1:-1]
    exposed = sum((nb != mine).astype(np.int64) for nb in (pad[:-2, 1:-1], pad[2:, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:]))
    e = exposed[ys, xs][order]
    table[:, 0] = np.add.reduceat(np.ones_like(x), starts)
    table[:, 1], table[:, 2] = np.minimum.reduceat(x, starts), np.maximum.reduceat(x, starts)
    table[:, 3], table[:, 4] = np.minimum.reduceat(y, starts), np.maximum.reduceat(y, starts)
    for col, v in ((5, x), (6, y), (7, x * x), (8, y * y), (9, x * y), (10, (e > 0).astype(np.int64)), (13, e)):
        table[:, col] = np.add.reduceat(v, starts)
    table[:, 11] = (y * W + x)[starts]
    table[:, 12] = image_ordinal
    return table


def region_props(table, shape):
    """regionprops-style features in float64 from the integer rows of region_table / ops.region_stats; shape = (H, W) of the images.
    Returns a dict of [R] arrays (REGION_PROPS).  With A = area, Sx = sum x, ... and a pixel taken as the unit square around its centre:
      centroid_x = Sx / A, centroid_y = Sy / A
      equivalent_diameter = sqrt(4 A / pi): the diameter of the disc of the same area
      extent = A / ((xmax - xmin + 1) (ymax - ymin + 1))
      mu20 = (A Sxx - Sx^2) / A^2 + 1/12, mu02 = (A Syy - Sy^2) / A^2 + 1/12, mu11 = (A Sxy - Sx Sy) / A^2: the central second
        moments per pixel; 1/12 is the second moment of the unit square itself, so a single pixel has mu20 = mu02 = 1/12 and an
        a x b rectangle a^2 / 12 and b^2 / 12.  The three numerators are formed in Python integers, which are exact.
      l1 = (mu20 + mu02 + sqrt((mu20 - mu02)^2 + 4 mu11^2)) / 2 and l2 = (mu20 mu02 - mu11^2) / l1: the eigenvalues of
        [[mu20, mu11], [mu11, mu02]] (the second from the determinant, which does not cancel)
      major_axis_length = 4 sqrt(l1), minor_axis_length = 4 sqrt(l2): the axes of the ellipse with the same second moments
      eccentricity = sqrt(1 - l2 / l1)
      orientation = atan2(2 mu11, mu20 - mu02) / 2: the angle of the major axis from the +x axis towards +y (rows grow downwards),
        in (-pi/2, pi/2]; 0 for a region with mu20 == mu02 and mu11 == 0.  skimage measures its angle from the row axis instead.
      compactness = 4 pi A / edges^2, the exposed edges being the perimeter of the pixel polygon: pi / 4 for any square
      touches_border = xmin == 0 or ymin == 0 or xmax == W - 1 or ymax == H - 1 (bool)"""
    t = np.asarray(table)
    assert t.ndim == 2 and t.shape[1] == 16 and t.dtype == np.int64, (t.shape, t.dtype)
    H, W = shape
    o = t.astype(object)
    A, Sx, Sy, Sxx, Syy, Sxy = (o[:, c] for c in (0, 5, 6, 7, 8, 9))
    exact = lambda v: np.array([float(q) for q in v], dtype=np.float64)      # noqa: E731
    a = t[:, 0].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        mu20 = exact(A * Sxx - Sx * Sx) / (a * a) + 1.0 / 12.0
        mu02 = exact(A * Syy - Sy * Sy) / (a * a) + 1.0 / 12.0
        mu11 = exact(A * Sxy - Sx * Sy) / (a * a)
        l1 = (mu20 + mu02 + np.sqrt((mu20 - mu02) ** 2 + 4.0 * mu11 ** 2)) / 2.0
        l2 = np.maximum((mu20 * mu02 - mu11 * mu11) / l1, 0.0)
        edges = t[:, 13].astype(np.float64)
        props = {
            'area': a,
            'centroid_x': t[:, 5] / a,
            'centroid_y': t[:, 6] / a,
            'equivalent_diameter': np.sqrt(4.0 * a / np.pi),
            'extent': a / ((t[:, 2] - t[:, 1] + 1) * (t[:, 4] - t[:, 3] + 1)).astype(np.float64),
            'mu20': mu20, 'mu02': mu02, 'mu11': mu11,
            'major_axis_length': 4.0 * np.sqrt(l1),
            'minor_axis_length': 4.0 * np.sqrt(l2),
            'eccentricity': np.sqrt(np.maximum(1.0 - l2 / l1, 0.0)),
            'orientation': 0.5 * np.arctan2(2.0 * mu11, mu20 - mu02),
            'compactness': 4.0 * np.pi * a / (edges * edges),
            'touches_border': (t[:, 1] == 0) | (t[:, 3] == 0) | (t[:, 2] == W - 1) | (t[:, 4] == H - 1),
        }
    assert tuple(props) == REGION_PROPS
    return props


def compute_thinned_scores(S, T):
    """(Rand F-score [N], VInfo [N]) of the THINNED prediction against the truth: compute_Rand_F_scores and compute_VInfo_scores on
    thin(S > 0.5)[0] and T > 0.5 -- the reference's compute_Rand_F_scores(S, T, do_thin=True) (util/util.py:99-101), which thins the
    prediction only.  The regions are still labelled 8-connected, as in the reference, so a thinned DIAGONAL wall does not separate
    the regions on its two sides: that is the reference's do_thin=True convention, kept as it is.
    S, T: [N, 1, H, W] (or a single [H, W] pair)."""
    S, T = np.asarray(S), np.asarray(T)
    if S.ndim == 2:
        S, T = S.reshape((1, 1) + S.shape), T.reshape((1, 1) + T.shape)
    St = np.stack([thin(S[k].squeeze(axis=0) > 0.5)[0][None] for k in range(S.shape[0])]).astype(np.float64)
    Tt = (T > 0.5).astype(np.float64)
    return compute_Rand_F_scores(St, Tt), compute_VInfo_scores(St, Tt)


def compute_Rand_F_scores(S, T, do_thin=False):
    """Rand F-score of prediction S against ground truth T per image (util/util.py:86-128): both thresholded at 0.5, the regions
    between the (true) boundary pixels labelled by 8-connectivity, then  F = 2 / (1/prec + 1/rec)  with
    prec = sum_ij p_ij^2 / sum_j b_j^2,  rec = sum_ij p_ij^2 / sum_i a_i^2  over the joint label distribution p without the
    ground-truth background row; prediction-background pixels count as singletons (the `aux / n` terms).
    S, T: [N, 1, H, W] (or a single [H, W] pair).  The contingency table is one bincount instead of the reference's pixel loop."""
    S, T = np.asarray(S), np.asarray(T)
    if S.ndim == 2:
        S, T = S.reshape((1, 1) + S.shape), T.reshape((1, 1) + T.shape)
    if do_thin:
        raise NotImplementedError("do_thin needs skimage.morphology.thin, which this image does not carry")
    scores = np.zeros(T.shape[0])
    for k in range(T.shape[0]):
        t_label = _label_false_regions(T[k].squeeze(axis=0) > 0.5)
        s_label = _label_false_regions(S[k].squeeze(axis=0) > 0.5)
        t_max, s_max = int(t_label.max()), int(s_label.max())
        p = np.bincount((t_label.astype(np.int64) * (s_max + 1) + s_label).ravel(), minlength=(t_max + 1) * (s_max + 1))
        p = p.reshape(t_max + 1, s_max + 1).astype(np.float64)
        n = p.sum()
        p_ = p[1:, :] / n
        p__ = p_[:, 1:]
        aux = p_[:, 0].sum()
        sumA2 = np.power(p_.sum(axis=1), 2).sum()
        sumB2 = np.power(p__.sum(axis=0), 2).sum() + aux / n
        sumAB2 = np.power(p__, 2).sum() + aux / n
        prec, rec = sumAB2 / sumB2, sumAB2 / sumA2
        scores[k] = 2 / (1 / prec + 1 / rec)
    return scores


def _xlogx_sum(counts):
    """sum of c ln c over the nonzero entries of an integer array (fp64)."""
    c = np.asarray(counts, dtype=np.float64).ravel()
    c = c[c > 0]
    return float((c * np.log(c)).sum())


def compute_VInfo_parts(s, t):
    """The terms of compute_VInfo_scores for one [H, W] pair, as a dict: SA, SB, SAB, aux, m, H_S, H_T, I, VInfo, split, merge."""
    t_label = _label_false_regions(np.asarray(t) > 0.5).astype(np.int64)
    s_label = _label_false_regions(np.asarray(s) > 0.5).astype(np.int64)
    t_max, s_max = int(t_label.max()), int(s_label.max())
    p = np.bincount((t_label * (s_max + 1) + s_label).ravel(), minlength=(t_max + 1) * (s_max + 1)).reshape(t_max + 1, s_max + 1)
    p = p[1:, :]                                        # without the ground-truth wall row
    a, b, c, aux = p.sum(axis=1), p[:, 1:].sum(axis=0), p[:, 1:], int(p[:, 0].sum())
    m = int(a.sum())
    nan = float('nan')
    out = dict(SA=_xlogx_sum(a), SB=_xlogx_sum(b), SAB=_xlogx_sum(c), aux=float(aux), m=float(m), H_S=nan, H_T=nan, I=nan, VInfo=nan,
               split=nan, merge=nan)
    if m == 0:
        return out
    A2, B2 = int((a.astype(object) ** 2).sum()), int((b.astype(object) ** 2).sum())
    ht_zero, hs_zero = A2 == m * m, (aux == 0 and B2 == m * m) or m == 1
    ln_m = float(np.log(float(m)))
    h_t = 0.0 if ht_zero else ln_m - out['SA'] / m
    h_s = 0.0 if hs_zero else ln_m - out['SB'] / m
    h_st = ln_m - out['SAB'] / m
    info = min(max(h_s + h_t - h_st, 0.0), min(h_s, h_t))
    if ht_zero and hs_zero:
        v = 1.0
    elif ht_zero or hs_zero:
        v = 0.0
    else:
        v = 2.0 * info / (h_s + h_t)
    out.update(H_S=h_s, H_T=h_t, I=info, VInfo=v, split=nan if hs_zero else info / h_s, merge=nan if ht_zero else info / h_t)
    return out


def compute_VInfo_scores(S, T, do_thin=False):
    """Information-theoretic F-score (V^Info of the ISBI-2012 segmentation challenge) of prediction S against ground truth T per
    image, under the conventions of compute_Rand_F_scores: both thresholded at 0.5, regions = 8-connected non-wall components, the
    pixels on truth wall left out, a pixel of a truth region on prediction wall a segment of its own.  With a_i, b_j, c_ij the pixel
    counts of truth region i, prediction region j (inside some truth region) and their intersection, and m = sum_i a_i:
        H_T = ln m - sum_i a_i ln a_i / m,  H_S = ln m - sum_j b_j ln b_j / m,  H_ST = ln m - sum_ij c_ij ln c_ij / m
    (singletons add 1 ln 1 = 0),  I = H_S + H_T - H_ST clamped to [0, min(H_S, H_T)],  VInfo = 2 I / (H_S + H_T).
    Whether an entropy is exactly 0 is decided from the integer counts: m == 0 scores NaN, two single regions 1, one single region
    against a split 0.  S, T: [N, 1, H, W] (or a single [H, W] pair).  The host yardstick of the device path
    (sgan_vinfo_accumulate); the trainers do not call it."""
    S, T = np.asarray(S), np.asarray(T)
    if S.ndim == 2:
        S, T = S.reshape((1, 1) + S.shape), T.reshape((1, 1) + T.shape)
    if do_thin:
        raise NotImplementedError("do_thin needs skimage.morphology.thin, which this image does not carry")
    return np.array([compute_VInfo_parts(S[k].squeeze(axis=0), T[k].squeeze(axis=0))['VInfo'] for k in range(T.shape[0])])


OBJECT_METRICS = ('ObjF1', 'ObjAP', 'SEG', 'PQ')      # the --which_metric names object_scores derives, in the order they are reported


def object_match_counts(s, t, min_area=1):
    """The object-level match counts (include/sgan_hip.h, "object-level scores") of prediction s against truth t, one [H, W] pair of
    boundary maps thresholded at 0.5 and labelled 8-connected as region_table labels: (counts int64[16], sums float64[2]).
    With whole areas a_i, b_j, the overlap c_ij and u_ij = a_i + b_j - c_ij, and regions smaller than min_area treated as absent:
    counts[k] = TP_k = pairs with 20 c_ij > (10 + k) u_ij for k = 0 .. 9 (int64 arithmetic), counts[10] = N_t, counts[11] = N_s,
    counts[12] = 1 (images), counts[13] = SEGn = pairs with 2 c_ij > a_i, counts[14] = counts[15] = 0; sums[0] = SIoU = sum of
    c_ij / u_ij over the pairs of TP_0, sums[1] = SSEG = the same sum over the pairs of SEGn (math.fsum: correctly rounded).
    The host yardstick of ops.object_match_accumulate; the trainers do not call it."""
    import math
    assert min_area >= 1, min_area
    t_label = _label_false_regions(np.asarray(t) > 0.5).astype(np.int64)
    s_label = _label_false_regions(np.asarray(s) > 0.5).astype(np.int64)
    assert t_label.ndim == 2 and t_label.shape == s_label.shape, (t_label.shape, s_label.shape)
    area_t, area_s = np.bincount(t_label.ravel()), np.bincount(s_label.ravel())
    stride = int(s_label.max()) + 1
    both = (t_label > 0) & (s_label > 0)
    pair, c = np.unique(t_label[both] * stride + s_label[both], return_counts=True)      # the nonzero c_ij only
    a, b, c = area_t[pair // stride], area_s[pair % stride], c.astype(np.int64)
    keep = (a >= min_area) & (b >= min_area)
    a, b, c = a[keep], b[keep], c[keep]
    u = a + b - c
    counts, sums = np.zeros(16, dtype=np.int64), np.zeros(2, dtype=np.float64)
    for k in range(10):
        counts[k] = int((20 * c > (10 + k) * u).sum())
    counts[10], counts[11], counts[12] = int((area_t[1:] >= min_area).sum()), int((area_s[1:] >= min_area).sum()), 1
    found, seg = 20 * c > 10 * u, 2 * c > a
    counts[13] = int(seg.sum())
    iou = c.astype(np.float64) / u.astype(np.float64)
    sums[0], sums[1] = math.fsum(iou[found]), math.fsum(iou[seg])
    return counts, sums


def object_scores(counts, sums):
    """ObjF1, ObjAP, SEG and PQ (an OrderedDict in that order) from pooled object_match_counts / ops.object_match_accumulate numbers:
    ObjF1 = 2 TP_0 / (N_t + N_s); ObjAP = mean over the ten thresholds of TP_k / (N_t + N_s - TP_k); SEG = SSEG / N_t;
    PQ = SIoU / ((N_t + N_s) / 2).  A score whose denominator is 0 reads 0.  The one place the trainers and the tests derive them."""
    from collections import OrderedDict
    tp, n_t, n_s = [int(v) for v in counts[:10]], int(counts[10]), int(counts[11])
    siou, sseg = float(sums[0]), float(sums[1])
    n = n_t + n_s
    return OrderedDict([('ObjF1', 2.0 * tp[0] / n if n else 0.0),
                        ('ObjAP', sum(v / (n - v) if n - v else 0.0 for v in tp) / 10.0),
                        ('SEG', sseg / n_t if n_t else 0.0),
                        ('PQ', siou / (n / 2.0) if n else 0.0)])


BOUNDARY_METRICS = ('BoundF', 'HausD', 'ASSD')      # the --which_metric names boundary_scores derives, in the order they are reported
BOUNDARY_BINS = 32


def _wall_mask(m):
    m = np.asarray(m)
    return m if m.dtype == np.bool_ else m > 0.5      # a NaN and an exact 0.5 are not wall


def edt_sq(mask):
    """The exact squared Euclidean distance transform of a [H, W] wall mask (bool, or a map thresholded at > 0.5): int32 [H, W], the
    smallest dy^2 + dx^2 to a wall pixel, 0 on the wall, -1 everywhere when the mask is empty.  Two 1-D passes in integers: the
    distance to the nearest wall pixel of the column from two running "last wall row seen" sweeps, then per row the minimum over
    all columns of dx^2 + g^2.  The host yardstick of ops.edt_sq; O(H W^2), the trainers do not call it."""
    wall = _wall_mask(mask)
    assert wall.ndim == 2, wall.shape
    H, W = wall.shape
    if not wall.any():
        return np.full((H, W), -1, dtype=np.int32)
    far = np.int64(4 * (H + W))      # farther than any pixel of the plane: "no wall in this column"
    rows = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(wall, rows, -far), axis=0)                         # the last wall row at or above y
    below = np.minimum.accumulate(np.where(wall, rows, far)[::-1], axis=0)[::-1]              # the first wall row at or below y
    g = np.minimum(rows - above, below - rows)
    has = wall.any(axis=0)
    gsq = np.where(has[None, :], g * g, np.int64(1) << 40)
    cols = np.arange(W, dtype=np.int64)
    dxsq = (cols[:, None] - cols[None, :]) ** 2                                               # [x, x']
    out = np.empty((H, W), dtype=np.int64)
    for y in range(H):
        out[y] = (dxsq + gsq[y][None, :]).min(axis=1)
    return out.astype(np.int32)


def signed_edt_sq(mask):
    """The signed squared Euclidean distance map of a [H, W] mask (bool, or a map thresholded at > 0.5; a NaN and an exact 0.5 are
    outside), from two edt_sq: int32 [H, W], +(the smallest dy^2 + dx^2 to an inside pixel) on an outside pixel, -(the smallest
    dy^2 + dx^2 to an outside pixel) on an inside pixel, 0 everywhere when the mask has no inside or no outside pixel.  The host
    yardstick of ops.signed_edt_sq."""
    inside = _wall_mask(mask)
    assert inside.ndim == 2, inside.shape
    if not inside.any() or inside.all():
        return np.zeros(inside.shape, dtype=np.int32)
    return np.where(inside, -edt_sq(~inside), edt_sq(inside)).astype(np.int32)


CLEAN_COUNTS = ('closed_pixels', 'wall_components_removed', 'wall_pixels_removed', 'cells_filled', 'cell_pixels_filled', 'images')


def clean_wall(mask, close_rsq=0, min_wall=0, min_cell=0):
    """The cleaned wall map (include/sgan_hip.h, "cleaning the prediction") of a [H, W] wall mask (bool, or a map thresholded at
    > 0.5): (bool [H, W], counts int64[6] in CLEAN_COUNTS' order).  Three stages in this order, each skipped when its parameter is 0:
    a closing with the disk dy^2 + dx^2 <= close_rsq from two thresholds of edt_sq (the dilation counts the outside of the image as
    free, the erosion as wall); 8-connected wall components with fewer than min_wall pixels become free; 8-connected free components
    with fewer than min_cell pixels become wall.  The host yardstick of ops.clean_wall; the trainers do not call it."""
    from scipy import ndimage
    wall = np.array(_wall_mask(mask), dtype=bool)
    assert wall.ndim == 2 and close_rsq >= 0 and min_wall >= 0 and min_cell >= 0, (wall.shape, close_rsq, min_wall, min_cell)
    counts = np.zeros(len(CLEAN_COUNTS), dtype=np.int64)
    counts[5] = 1
    if close_rsq > 0:
        d = edt_sq(wall)
        dilated = (d >= 0) & (d <= close_rsq)
        e = edt_sq(~dilated)
        closed = (e < 0) | (e > close_rsq)      # e < 0: nothing is left outside the dilation
        counts[0] = int((closed & ~wall).sum())
        wall = closed
    for k, (min_area, of_wall) in enumerate(((min_wall, True), (min_cell, False))):
        if min_area > 0:
            labels, _ = ndimage.label(wall if of_wall else ~wall, structure=np.ones((3, 3)))
            area = np.bincount(labels.ravel())
            small = area < min_area
            small[0] = False                    # label 0: the other side
            counts[1 + 2 * k], counts[2 + 2 * k] = int(small.sum()), int(area[small].sum())
            wall = wall & ~small[labels] if of_wall else wall | small[labels]
    return wall, counts


SPLIT_COUNTS = ('core_components', 'cut_pixels', 'labelled_pixels', 'rounds', 'budget_hits', 'images')


def split_labels(mask, split_rsq, max_rounds=64):
    """The flood of split_cells: (L int64 [H, W], core components, rounds that labelled something, whether round max_rounds did).
    L is 0 on the wall and on the free pixels the budget did not reach, else 1 + the smallest raster index of the core component
    that reaches the pixel first (the smallest such label when several arrive in the same round)."""
    from scipy import ndimage
    wall = np.array(_wall_mask(mask), dtype=bool)
    assert wall.ndim == 2 and split_rsq >= 1 and max_rounds >= 1, (wall.shape, split_rsq, max_rounds)
    H, W = wall.shape
    d = edt_sq(wall)
    comp, n = ndimage.label(~wall & (d >= split_rsq), structure=np.ones((3, 3)))
    first = np.full(n + 1, H * W, dtype=np.int64)
    np.minimum.at(first, comp.ravel(), np.arange(H * W, dtype=np.int64))      # the smallest raster index of every component
    L = np.where(comp > 0, first[comp] + 1, 0).astype(np.int64)
    none = np.int64(1) << 40      # "no labelled neighbour"
    rounds, last = 0, False
    for r in range(max_rounds):
        padded = np.full((H + 2, W + 2), none, dtype=np.int64)
        padded[1:-1, 1:-1] = np.where(L > 0, L, none)
        best = np.full((H, W), none, dtype=np.int64)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                if (dy, dx) != (1, 1):
                    best = np.minimum(best, padded[dy:dy + H, dx:dx + W])
        take = ~wall & (L == 0) & (best < none)
        last = bool(take.any())
        if not last:
            break
        L[take] = best[take]
        rounds += 1
    return L, n, rounds, last


def split_cells(mask, split_rsq, max_rounds=64):
    """The wall map with merged cells cut apart (include/sgan_hip.h, "splitting merged cells") of a [H, W] wall mask (bool, or a map
    thresholded at > 0.5): (bool [H, W], counts int64[6] in SPLIT_COUNTS' order).  The cores of the free space, edt_sq >= split_rsq,
    are labelled with the 8-structure; max_rounds synchronous rounds give every unlabelled free pixel the smallest label among its
    eight labelled neighbours; a labelled free pixel whose E, SW, S or SE neighbour carries another nonzero label becomes wall.  The
    host yardstick of ops.split_cells; the trainers do not call it."""
    wall = np.array(_wall_mask(mask), dtype=bool)
    L, n, rounds, last = split_labels(wall, split_rsq, max_rounds)
    H, W = wall.shape
    P = np.zeros((H + 1, W + 2), dtype=np.int64)      # L with a column of zeros on either side and a row below
    P[:H, 1:W + 1] = L
    cut = np.zeros((H, W), dtype=bool)
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):      # E, SW, S, SE
        q = P[dy:dy + H, 1 + dx:1 + dx + W]
        cut |= (L > 0) & (q > 0) & (q != L)
    counts = np.array([n, int(cut.sum()), int((L > 0).sum()), rounds, int(last), 1], dtype=np.int64)
    return wall | cut, counts


def boundary_bin(d):
    """The bin of a distance^2 (include/sgan_hip.h, "boundary scores"): k = ceil(sqrt(d)) in integers for 0 <= d <= 900, 31 beyond
    and for -1 (the other map has no wall)."""
    import math
    d = int(d)
    if d < 0 or d > 900:
        return BOUNDARY_BINS - 1
    k = math.isqrt(d)
    return k if k * k == d else k + 1


def boundary_counts(s_wall, t_wall):
    """The boundary counts (include/sgan_hip.h, "boundary scores") of the predicted wall s_wall against the true wall t_wall, two
    [H, W] masks (bool, or maps thresholded at > 0.5): (counts int64[80], sums float64[4]).  counts[0:32] / counts[32:64]: the
    predicted / truth wall pixels by the bin of their distance^2 to the other map's wall; [64] N_s, [65] N_t, [66] 1 (images),
    [67] 1 when both maps have wall, [68] / [69] the predicted / truth wall pixels with a defined distance, [70] / [71] the largest
    distance^2 on either side, the rest 0.  sums[0] / sums[1]: the sums of the distances over the predicted / truth wall pixels with
    a defined distance, sums[2] the Hausdorff distance of the pair when both have wall (math.fsum of math.sqrt: correctly rounded).
    The host yardstick of ops.boundary_accumulate; the trainers do not call it."""
    import math
    s_wall, t_wall = _wall_mask(s_wall), _wall_mask(t_wall)
    assert s_wall.ndim == 2 and s_wall.shape == t_wall.shape, (s_wall.shape, t_wall.shape)
    s_dsq, t_dsq = edt_sq(s_wall), edt_sq(t_wall)
    counts, sums = np.zeros(80, dtype=np.int64), np.zeros(4, dtype=np.float64)
    for side, (own, other) in enumerate(((s_wall, t_dsq), (t_wall, s_dsq))):
        d = other[own].astype(np.int64)
        for v, n in zip(*np.unique(d, return_counts=True)):
            counts[32 * side + boundary_bin(v)] += n
        counts[64 + side] = d.size
        defined = d[d >= 0]
        counts[68 + side] = defined.size
        counts[70 + side] = int(defined.max()) if defined.size else 0
        sums[side] = math.fsum(math.sqrt(int(v)) for v in defined)
    counts[66] = 1
    if counts[64] and counts[65]:
        counts[67] = 1
        sums[2] = math.sqrt(int(max(counts[70], counts[71])))
    return counts, sums


def boundary_pr(counts, tolerance):
    """(BoundP, BoundR, BoundF) at an integer pixel tolerance 0 .. 30 from pooled boundary counts: the share of the predicted / truth
    wall pixels within `tolerance` of the other map's wall, and their harmonic mean.  A zero denominator reads 0."""
    assert 0 <= int(tolerance) <= 30, tolerance
    k = int(tolerance) + 1
    n_s, n_t = int(counts[64]), int(counts[65])
    p = int(np.sum(counts[0:k])) / n_s if n_s else 0.0
    r = int(np.sum(counts[32:32 + k])) / n_t if n_t else 0.0
    return p, r, (2.0 * p * r / (p + r) if p + r else 0.0)


def boundary_scores(counts, sums, tolerance):
    """BoundF, HausD and ASSD (an OrderedDict in that order) from pooled boundary_counts / ops.boundary_accumulate numbers: BoundF at
    `tolerance` pixels (boundary_pr); HausD = the mean over the images where both maps have wall of their Hausdorff distances,
    sums[2] / counts[67]; ASSD = (sums[0] + sums[1]) / (counts[68] + counts[69]).  A score whose denominator is 0 reads 0.  The one
    place the trainers and the tests derive them."""
    from collections import OrderedDict
    n_h, n_d = int(counts[67]), int(counts[68]) + int(counts[69])
    return OrderedDict([('BoundF', boundary_pr(counts, tolerance)[2]),
                        ('HausD', float(sums[2]) / n_h if n_h else 0.0),
                        ('ASSD', (float(sums[0]) + float(sums[1])) / n_d if n_d else 0.0)])


# ---- topology scores: windowed Betti errors and clDice (the yardsticks of sgan_topo.hip) -----------------------------------
TOPO_METRICS = ('Betti0Err', 'Betti1Err', 'clDice')      # the --which_metric names topo_scores derives, in the order they are reported
TOPO_COUNTS = ('windows', 'abs_d0', 'abs_d1', 'b0_s', 'b0_t', 'b1_s', 'b1_t', 'skel_s', 'skel_s_in_t', 'skel_t', 'skel_t_in_s', 'images')


def betti_window(wall):
    """(b0, b1) of one window, a [h, w] wall mask (bool, or a map thresholded at > 0.5) cut out of its image, so that everything
    outside it is free: b0 = the 8-connected components of the wall, b1 = the 4-connected components of the free pixels that touch no
    edge of the window -- the enclosed cells.  scipy.ndimage.label on the window padded with one ring of free pixels, whose component
    is the outside."""
    from scipy import ndimage
    wall = np.array(_wall_mask(wall), dtype=bool)
    assert wall.ndim == 2, wall.shape
    _, b0 = ndimage.label(wall, structure=np.ones((3, 3)))
    _, n_free = ndimage.label(~np.pad(wall, 1, constant_values=False))      # the default structure: 4-connected
    return int(b0), int(n_free) - 1


def euler_bitquads(wall):
    """The Euler number of a window for 8-connectivity from Gray's bit quads, (Q1 - Q3 - 2 Qd) / 4 over every 2 x 2 block of the
    window padded with one ring of free pixels: Q1 / Q3 the blocks with one / three wall pixels, Qd those with two on a diagonal.
    Equals b0 - b1 of betti_window."""
    p = np.pad(np.array(_wall_mask(wall), dtype=bool), 1, constant_values=False).astype(np.int64)
    a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    n = a + b + c + d
    q1, q3 = int((n == 1).sum()), int((n == 3).sum())
    qd = int(((n == 2) & (a == d)).sum())
    assert (q1 - q3 - 2 * qd) % 4 == 0
    return (q1 - q3 - 2 * qd) // 4


def topo_windows(H, W, window, stride):
    """(wh, ww, the origins in y, the origins in x) of the windows of an H x W map: wh = min(window, H) by ww = min(window, W) pixels
    at 0, stride, 2 stride, ... while the window lies inside the map.  A strip at the bottom or the right that no full window covers
    is not scored."""
    assert H >= 1 and W >= 1 and 8 <= window <= 64 and 1 <= stride <= window, (H, W, window, stride)
    wh, ww = min(window, H), min(window, W)
    return wh, ww, list(range(0, H - wh + 1, stride)), list(range(0, W - ww + 1, stride))


def topo_counts(s_wall, t_wall, window=64, stride=None, s_thin=None, t_thin=None):
    """The topology counts (include/sgan_hip.h, "topology scores") of the predicted wall s_wall against the true wall t_wall, two
    [H, W] masks (bool, or maps thresholded at > 0.5): int64[12] in TOPO_COUNTS' order.  Over topo_windows: the windows, the sums
    of |b0(S) - b0(T)| and |b1(S) - b1(T)| and the plain sums of betti_window.  s_thin / t_thin: the thinned maps (thin of s_wall /
    t_wall), for the skeleton pixels and how many of them are wall in the other map; a side that is None counts nothing.  The host
    yardstick of ops.topo_accumulate; the trainers do not call it."""
    s_wall, t_wall = _wall_mask(s_wall), _wall_mask(t_wall)
    assert s_wall.ndim == 2 and s_wall.shape == t_wall.shape, (s_wall.shape, t_wall.shape)
    H, W = s_wall.shape
    wh, ww, ys, xs = topo_windows(H, W, window, window if stride is None else stride)
    c = np.zeros(len(TOPO_COUNTS), dtype=np.int64)
    for oy in ys:
        for ox in xs:
            (b0s, b1s), (b0t, b1t) = (betti_window(m[oy:oy + wh, ox:ox + ww]) for m in (s_wall, t_wall))
            c[:7] += (1, abs(b0s - b0t), abs(b1s - b1t), b0s, b0t, b1s, b1t)
    if s_thin is not None:
        k = _wall_mask(s_thin)
        c[7], c[8] = int(k.sum()), int((k & t_wall).sum())
    if t_thin is not None:
        k = _wall_mask(t_thin)
        c[9], c[10] = int(k.sum()), int((k & s_wall).sum())
    c[11] = 1
    return c


def topo_scores(counts):
    """Betti0Err, Betti1Err and clDice (an OrderedDict in that order) from pooled topo_counts / ops.topo_accumulate integers: the mean
    over the windows of |b0(S) - b0(T)| and of |b1(S) - b1(T)|, and the harmonic mean of Tprec = skel_s_in_t / skel_s and
    Tsens = skel_t_in_s / skel_t.  A zero denominator reads 0, as in boundary_pr.  The one place the trainers and the tests derive
    them."""
    from collections import OrderedDict
    n, n_s, n_t = int(counts[0]), int(counts[7]), int(counts[9])
    p = int(counts[8]) / n_s if n_s else 0.0
    r = int(counts[10]) / n_t if n_t else 0.0
    return OrderedDict([('Betti0Err', int(counts[1]) / n if n else 0.0),
                        ('Betti1Err', int(counts[2]) / n if n else 0.0),
                        ('clDice', 2.0 * p * r / (p + r) if p + r else 0.0)])


# ---- differentiable augmentation of discriminator inputs (--diffaug; the yardsticks of sgan_diffaug.hip) -----------------
DIFFAUG_OPS = ('translation', 'cutout', 'brightness', 'contrast')


def _philox4x32_10(ctr, key):
    """The four 32-bit words of Philox4x32-10 (Salmon et al.) for the 64-bit block counter `ctr` (c2 = c3 = 0) under the 64-bit `key`,
    in Python integers."""
    c = [ctr & 0xFFFFFFFF, (ctr >> 32) & 0xFFFFFFFF, 0, 0]
    k0, k1 = key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def diffaug_params(seed, offset, shapes, policy, rt=0.125, rc=0.5):
    """The records sgan_diffaug_draw writes for images of shapes = [(H, W), ...]: one tuple (b, a, ty, tx, cy0, cy1, cx0, cx1) per
    image, b and a Python floats holding fp32 values (b exactly the formula's; a the formula's rounded to fp32, as the device's one
    addition rounds it), the rest integers.  Image j takes the Philox blocks at counters offset + 2 j
    (words w0..w3) and offset + 2 j + 1 (w4, w5) under the key `seed`, whatever `policy` (an iterable of DIFFAUG_OPS) switches on; the
    stream moves on by 2 len(shapes)."""
    policy = set(policy)
    assert policy <= set(DIFFAUG_OPS), policy
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    recs = []
    for j, (H, W) in enumerate(shapes):
        w = _philox4x32_10((offset + 2 * j) & (2 ** 64 - 1), seed) + _philox4x32_10((offset + 2 * j + 1) & (2 ** 64 - 1), seed)
        b = (w[0] >> 8) * 2.0 ** -24 - 0.5 if 'brightness' in policy else 0.0
        a = float(np.float32((w[1] >> 8) * 2.0 ** -24 + 0.5)) if 'contrast' in policy else 1.0      # one fp32 addition: 23 fraction bits from 1 up
        ty = tx = 0
        if 'translation' in policy:
            Sy, Sx = int(np.floor(H * rt + 0.5)), int(np.floor(W * rt + 0.5))
            ty, tx = -Sy + w[2] % (2 * Sy + 1), -Sx + w[3] % (2 * Sx + 1)
        cy0 = cy1 = cx0 = cx1 = 0
        if 'cutout' in policy:
            ch, cw = int(np.floor(H * rc + 0.5)), int(np.floor(W * rc + 0.5))
            oy, ox = w[4] % (H + 1 - ch % 2), w[5] % (W + 1 - cw % 2)
            cy0, cy1 = max(0, oy - ch // 2), min(H, oy - ch // 2 + ch)
            cx0, cx1 = max(0, ox - cw // 2), min(W, ox - cw // 2 + cw)
        recs.append((b, a, ty, tx, cy0, cy1, cx0, cx1))
    return recs


def _diffaug_visible(rec, H, W):
    """K [H, W] of a record: 0 inside the cutout and where the shifted source pixel lies outside the image."""
    _, _, ty, tx, cy0, cy1, cx0, cx1 = rec
    h, w = np.arange(H)[:, None], np.arange(W)[None, :]
    cut = (h >= cy0) & (h < cy1) & (w >= cx0) & (w < cx1)
    inside = (h + ty >= 0) & (h + ty < H) & (w + tx >= 0) & (w + tx < W)
    return (~cut & inside).astype(np.float64)


def _diffaug_shift(x, ty, tx):
    """out[h][w] = x[h + ty][w + tx], 0 where that lies outside (x: [H, W, C])."""
    H, W = x.shape[:2]
    out = np.zeros_like(x)
    h0, h1, w0, w1 = max(0, -ty), min(H, H - ty), max(0, -tx), min(W, W - tx)
    if h0 < h1 and w0 < w1:
        out[h0:h1, w0:w1] = x[h0 + ty:h1 + ty, w0 + tx:w1 + tx]
    return out


def diffaug_ref(x, rec, colour_mask):
    """DiffAugment of one image x [H, W, C] under one record, in float64: on the channels whose bit of `colour_mask` is set
    g(v) = a (v - m) + m + b with m the mean of x over all pixels and those channels, the other channels as they are; then
    y[h][w] = K(h, w) g(x[h + ty][w + tx])."""
    x = np.asarray(x, dtype=np.float64)
    H, W, C = x.shape
    b, a, ty, tx = rec[:4]
    col = np.array([(int(colour_mask) >> c) & 1 for c in range(C)], dtype=bool)
    g = x.copy()
    if col.any():
        m = x[:, :, col].mean()
        g[:, :, col] = a * (x[:, :, col] - m) + m + b
    return _diffaug_visible(rec, H, W)[:, :, None] * _diffaug_shift(g, ty, tx)


def diffaug_bwd_ref(dy, rec, colour_mask):
    """The adjoint of diffaug_ref at the same record, in float64: dx[p][c] = a_c K(p - t) dy[p - t][c], plus on the colour channels
    (1 - a) S / n with S the sum of K dy over them and n their element count (the gradient through the mean)."""
    dy = np.asarray(dy, dtype=np.float64)
    H, W, C = dy.shape
    b, a, ty, tx = rec[:4]
    col = np.array([(int(colour_mask) >> c) & 1 for c in range(C)], dtype=bool)
    kdy = _diffaug_visible(rec, H, W)[:, :, None] * dy
    dx = _diffaug_shift(kdy, -ty, -tx)
    if col.any():
        S = kdy[:, :, col].sum()
        dx[:, :, col] = a * dx[:, :, col] + (1.0 - a) * S / (int(col.sum()) * H * W)
    return dx


# ---- sliced Wasserstein distance over Laplacian-pyramid patches (swd.py; include/sgan_hip.h, "sliced Wasserstein distance") ----------
SWD_PATCH = 7
SWD_MAX_N = 16384      # descriptors per set the device sorts in one workgroup's LDS (sgan_swd_distances)
SWD_MIN_SIDE = 16      # a further pyramid level exists while half the smaller side is at least this
_LAP_B = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def _lap_correlate(x, scale):
    """5 x 5 correlation of the planes [C, H, W] with scale * outer(b, b) in float64, the border mirrored without repeating the edge
    (d c b | a b c d | c b a: numpy's 'reflect', scipy.ndimage's 'mirror')."""
    p = np.pad(np.asarray(x, dtype=np.float64), ((0, 0), (2, 2), (2, 2)), mode='reflect')
    H, W = x.shape[1:]
    out = np.zeros(x.shape, dtype=np.float64)
    for dy in range(5):
        for dx in range(5):
            out += (scale * _LAP_B[dy] * _LAP_B[dx]) * p[:, dy:dy + H, dx:dx + W]
    return out


def lap_down_ref(x):
    """[C, H, W] -> [C, H / 2, W / 2]: blur with g = outer(b, b), b = [1 4 6 4 1] / 16, keep the even sites."""
    return _lap_correlate(x, 1.0)[:, ::2, ::2]


def lap_up_ref(x):
    """[C, h, w] -> [C, 2 h, 2 w]: x on the even sites of a zero plane, blurred with 4 g."""
    z = np.zeros((x.shape[0], 2 * x.shape[1], 2 * x.shape[2]), dtype=np.float64)
    z[:, ::2, ::2] = x
    return _lap_correlate(z, 4.0)


def lap_level_sizes(H, W):
    """Sizes of the pyramid's levels, finest first: a further level while both sides are even and half the smaller is >= 16."""
    sizes = [(H, W)]
    while H % 2 == 0 and W % 2 == 0 and min(H, W) // 2 >= SWD_MIN_SIDE:
        H, W = H // 2, W // 2
        sizes.append((H, W))
    return sizes


def lap_pyramid_ref(img):
    """Laplacian pyramid of img [C, H, W] in float64, finest first: G_0 = img, G_{l+1} = down(G_l), L_l = G_l - up(G_{l+1}); the last
    level is G_last itself, so that the levels, each upsampled back to the image's size and added, give the image."""
    g = np.asarray(img, dtype=np.float64)
    levels = []
    for _ in lap_level_sizes(*g.shape[1:])[1:]:
        nxt = lap_down_ref(g)
        levels.append(g - lap_up_ref(nxt))
        g = nxt
    levels.append(g)
    return levels


def swd_descriptors_ref(levels_of_images, pos):
    """levels_of_images: one [C, H, W] level per image; pos: int32 [N, 3] of (image, y, x), the top-left corner of a 7 x 7 patch.
    Returns (desc [N, C * 49] in the order [c][dy][dx], in the level's dtype; mean [C]; population std [C]), the statistics in
    float64 over all N * 49 values of a channel."""
    pos = np.asarray(pos)
    C = levels_of_images[0].shape[0]
    desc = np.stack([np.asarray(levels_of_images[i])[:, y:y + SWD_PATCH, x:x + SWD_PATCH].reshape(C * SWD_PATCH * SWD_PATCH)
                     for i, y, x in pos])
    per_channel = desc.reshape(len(pos), C, -1).astype(np.float64).transpose(1, 0, 2).reshape(C, -1)
    return desc, per_channel.mean(axis=1), per_channel.std(axis=1)


def swd_stats_from_sums(sums, count):
    """(mean, std) per channel from the device's accumulators (float64 [2 C]: C sums, then C sums of squares) with the device's own
    roundings: mean = sum / count, var = max(sumsq / count - mean * mean, 0), std = sqrt(var), each step rounded once in float64."""
    sums = np.asarray(sums, dtype=np.float64)
    C = len(sums) // 2
    mean = sums[:C] / np.float64(count)
    var = sums[C:] / np.float64(count) - mean * mean
    return mean, np.sqrt(np.where(var > 0.0, var, 0.0))


def swd_normalise_ref(desc, mean, std):
    """The one yardstick that mirrors the device's roundings, in float32: n = float32(float32(x - m32) * r32) with m32 = float32(mean)
    and r32 = float32(1 / std), 0 where std == 0 (a constant level gives zero descriptors, not NaN).  No multiply-add can be
    contracted out of a subtract-then-multiply, so the device matches this bit for bit."""
    desc = np.asarray(desc, dtype=np.float32)
    mean, std = np.asarray(mean, dtype=np.float64), np.asarray(std, dtype=np.float64)
    C = len(mean)
    m32 = mean.astype(np.float32)
    r32 = np.where(std == 0.0, 0.0, 1.0 / np.where(std == 0.0, 1.0, std)).astype(np.float32)
    x = desc.reshape(len(desc), C, -1)
    d = (x - m32[None, :, None]).astype(np.float32)
    return (d * r32[None, :, None]).astype(np.float32).reshape(desc.shape)


def swd_ref(nA, nB, dirs):
    """Per-direction sliced Wasserstein distances in float64: nA, nB [N, K] float32 with equal N, dirs [J, K] float32; project in
    float64, sort both, mean |sA - sB|.  A level's score is the mean of the J values (printed x 1e3)."""
    nA, nB, dirs = (np.asarray(a, dtype=np.float64) for a in (nA, nB, dirs))
    assert nA.shape == nB.shape and dirs.shape[1] == nA.shape[1], (nA.shape, nB.shape, dirs.shape)
    pA, pB = np.sort(nA @ dirs.T, axis=0), np.sort(nB @ dirs.T, axis=0)
    return np.abs(pA - pB).mean(axis=0)


def swd_draw(seed, level, n_images, P, H_l, W_l, K, J, set_index=0):
    """The only source of randomness of the score.  Returns (pos int32 [n_images * P, 3] of (image, y, x) with 0 <= y <= H_l - 7,
    dirs float32 [J, K]).  The directions come from RandomState([seed, level]) -- randn, each row divided by its L2 norm in float64,
    then cast -- and are the same for both sets; the positions from RandomState([seed, level, 1 + set_index]), one stream per set."""
    d = np.random.RandomState([int(seed), int(level)]).randn(J, K)
    dirs = (d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(np.float32)
    rs = np.random.RandomState([int(seed), int(level), 1 + int(set_index)])
    pos = np.empty((n_images * P, 3), dtype=np.int32)
    pos[:, 0] = np.repeat(np.arange(n_images), P)
    pos[:, 1] = rs.randint(0, H_l - SWD_PATCH + 1, size=n_images * P)
    pos[:, 2] = rs.randint(0, W_l - SWD_PATCH + 1, size=n_images * P)
    return pos, dirs


# ---- precision / recall / density / coverage by k-nearest-neighbour balls (swd.py --prd_k; include/sgan_hip.h) -----------------------
PRD_MAX_K = 8          # neighbours a row keeps on the device (sgan_knn_radii)


def _prd_d2(X, Y, chunk=32):
    """All-pairs squared Euclidean distances [len(X), len(Y)] in float64, as sums of squared differences (never the Gram form: equal
    rows give exactly 0), `chunk` rows of X at a time."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    out = np.empty((len(X), len(Y)), dtype=np.float64)
    for i in range(0, len(X), chunk):
        d = X[i:i + chunk, None, :] - Y[None, :, :]
        out[i:i + chunk] = np.einsum('ijk,ijk->ij', d, d)
    return out


def knn_radii_ref(X, k, group=1, d2=None):
    """X [N, K]: normalised descriptors, the rows of one image contiguous, `group` rows each.  The in-set neighbours of row i are the
    rows j with j // group != i // group (group = 1: every other row).  Returns (rad, nn1) in float64: rad[i] the k-th smallest
    d2(x_i, x_j) over them (equal values each count), nn1[i] the smallest.  d2: the all-pairs matrix, if the caller has it."""
    N = len(X)
    assert 1 <= k <= N - group, (k, N, group)
    d2 = np.array(_prd_d2(X, X) if d2 is None else d2, dtype=np.float64)
    g = np.arange(N) // group
    d2[g[:, None] == g[None, :]] = np.inf
    s = np.sort(d2, axis=1)
    return s[:, k - 1].copy(), s[:, 0].copy()


def prd_rows_ref(Q, R, radR, d2=None):
    """Per row of Q against the balls of R: (cnt, nn_d2, nn_idx) with cnt[i] = #{j : d2(q_i, r_j) <= radR[j]} (int64), nn_d2[i] =
    min_j d2(q_i, r_j) (float64) and nn_idx[i] the smallest j that attains it."""
    d2 = _prd_d2(Q, R) if d2 is None else np.asarray(d2, dtype=np.float64)
    cnt = (d2 <= np.asarray(radR, dtype=np.float64)[None, :]).sum(axis=1).astype(np.int64)
    idx = d2.argmin(axis=1)      # the first of equal minima
    return cnt, d2[np.arange(len(d2)), idx], idx.astype(np.int64)


def prd_scores_ref(rows_B, rows_A, knn_A, knn_B, k):
    """The scores of a generated set B against a real set A, N rows each, both normalised by A's statistics.  rows_B = prd_rows_ref(B,
    A, radA), rows_A = prd_rows_ref(A, B, radB), knn_A = knn_radii_ref(A, k, group), knn_B = knn_radii_ref(B, k, group) (its radii are
    what rows_A was counted with).  precision = share of B's rows inside some ball of A; recall = share of A's rows inside some ball
    of B; density = sum of B's ball counts / (k N); coverage = share of A's rows whose nearest row of B lies inside their OWN ball;
    nn_fake_real = median over B of the squared distance to the nearest row of A, nn_real_real = median over A of the squared
    distance to the nearest row of another image of A, nn_ratio their quotient (far below 1: B sits closer to A than A to itself).
    Returns a dict; 'counts' holds the four integers the device's finish gives."""
    cntB, nnB = np.asarray(rows_B[0]), np.asarray(rows_B[1], dtype=np.float64)
    cntA, nnA = np.asarray(rows_A[0]), np.asarray(rows_A[1], dtype=np.float64)
    radA, nn1A = np.asarray(knn_A[0], dtype=np.float64), np.asarray(knn_A[1], dtype=np.float64)
    N = len(cntB)
    assert len(cntA) == N and len(radA) == N and len(knn_B[0]) == N, (len(cntA), N)
    counts = np.array([(cntB > 0).sum(), (cntA > 0).sum(), cntB.sum(), (nnA <= radA).sum()], dtype=np.int64)
    out = prd_from_counts(counts, N, k)
    fr, rr = float(np.median(nnB)), float(np.median(nn1A))
    out.update(nn_fake_real=fr, nn_real_real=rr, nn_ratio=prd_ratio(fr, rr), counts=counts)
    return out


def prd_from_counts(counts, N, k):
    """precision, recall, density, coverage from the four integers of sgan_prd_finish."""
    c = [int(v) for v in counts]
    return dict(precision=c[0] / N, recall=c[1] / N, density=c[2] / (k * N), coverage=c[3] / N)


def prd_ratio(fake_real, real_real):
    """nn_fake_real / nn_real_real; 0 / 0 (both sets the same single texture) reads as 1."""
    if real_real == 0.0:
        return 1.0 if fake_real == 0.0 else float('inf')
    return fake_real / real_real


# ---- soft-clDice (Shit et al., CVPR 2021): the host yardstick of ops.soft_skeleton / losses.soft_cldice ------------
CLDICE_ERODE_ORDER = ((0, 0), (-1, 0), (0, -1), (0, 1), (1, 0))                                      # centre, up, left, right, down
CLDICE_DILATE_ORDER = ((0, 0), (-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))      # centre, then row-major


def _cldice_select(X, order, pad, pick):
    """(value, position in `order`) of the extreme of X over the in-image pixels of the neighbourhood `order`, the first pixel in
    that order that attains it winning (np.argmin / argmax return the first occurrence); out-of-image neighbours hold `pad`."""
    H, W = X.shape
    Xp = np.full((H + 2, W + 2), pad, dtype=X.dtype)
    Xp[1:-1, 1:-1] = X
    stack = np.stack([Xp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in order])
    sel = pick(stack, axis=0)
    return np.take_along_axis(stack, sel[None], 0)[0], sel


def _cldice_scatter(g, sel, order):
    """Hands g(y) to the pixel y + order[sel(y)]: the transpose of the selection."""
    H, W = g.shape
    out = np.zeros((H, W), dtype=np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    off = np.asarray(order)
    np.add.at(out, (yy + off[sel, 0], xx + off[sel, 1]), g)
    return out


def soft_skeleton_ref(X, iters):
    """The soft skeleton of the fp32 plane X with K = iters: (S_K in fp64, [I_0 .. I_{K+1}] in fp32 (bits of X), [delta_j], [S_j],
    erode selections of I_0 .. I_K, dilate selections of I_1 .. I_{K+1}).  Selections are made on the fp32 values."""
    K = int(iters)
    assert 1 <= K <= 16, K
    I = [np.ascontiguousarray(X, dtype=np.float32)]
    esel, dsel, delta, S = [], [], [], []
    for j in range(K + 1):
        v, s = _cldice_select(I[j], CLDICE_ERODE_ORDER, np.float32(np.inf), np.argmin)
        I.append(v)
        esel.append(s)
    for j in range(K + 1):
        d, s = _cldice_select(I[j + 1], CLDICE_DILATE_ORDER, np.float32(-np.inf), np.argmax)
        dsel.append(s)
        delta.append(np.maximum(I[j].astype(np.float64) - d.astype(np.float64), 0.0))
        S.append(delta[0] if j == 0 else S[-1] + delta[j] * (1.0 - S[-1]))
    return S[-1], I, delta, S, esel, dsel


def soft_cldice_sums(SP, T, ST, P):
    """(A, B, C, D, L, gA, gB, gC) of the loss from the two skeletons: d L / d S(P) = gA T + gB, the direct term gC S(T)."""
    A, B, C, D = float((SP * T).sum()), float(SP.sum()), float((ST * P).sum()), float(ST.sum())
    tp, ts = (A + 1.0) / (B + 1.0), (C + 1.0) / (D + 1.0)
    L = 1.0 - 2.0 * tp * ts / (tp + ts)
    dLdp, dLds = -2.0 * ts * ts / (tp + ts) ** 2, -2.0 * tp * tp / (tp + ts) ** 2
    return A, B, C, D, L, dLdp / (B + 1.0), -dLdp * (A + 1.0) / (B + 1.0) ** 2, dLds / (D + 1.0)


def soft_cldice_ref(P, T, iters):
    """soft-clDice of the probability plane P against the binary truth T (both read as fp32 [H, W]) with K = iters, in fp64:
    (L, dL/dP, S(P), S(T), [I_j of P], M).  M is the same backward run with every contribution taken in absolute value: the scale
    against which a rounding of the fp32 backward is measured."""
    P32, T32 = np.ascontiguousarray(P, dtype=np.float32), np.ascontiguousarray(T, dtype=np.float32)
    K = int(iters)
    SP, I, delta, S, esel, dsel = soft_skeleton_ref(P32, K)
    ST = soft_skeleton_ref(T32, K)[0]
    P64, T64 = P32.astype(np.float64), T32.astype(np.float64)
    _, _, _, _, L, gA, gB, gC = soft_cldice_sums(SP, T64, ST, P64)
    grads = []
    for absolute in (False, True):
        gS = abs(gA) * T64 + abs(gB) if absolute else gA * T64 + gB
        E = [None] * (K + 1)
        for j in range(K, 0, -1):
            E[j] = gS * (1.0 - S[j - 1]) * (delta[j] > 0)
            gS = gS * (1.0 - delta[j])
        E[0] = gS * (delta[0] > 0)
        sign = 1.0 if absolute else -1.0
        G = _cldice_scatter(sign * E[K], dsel[K], CLDICE_DILATE_ORDER)                   # d L / d I_{K+1}
        for j in range(K, -1, -1):
            G = E[j] + _cldice_scatter(G, esel[j], CLDICE_ERODE_ORDER)
            if j >= 1:
                G = G + _cldice_scatter(sign * E[j - 1], dsel[j - 1], CLDICE_DILATE_ORDER)
        grads.append(G + (abs(gC) if absolute else gC) * ST)
    return L, grads[0], SP, ST, I, grads[1]


def lovasz_ref(P, label, classes):
    """Lovasz-softmax (Berman, Triki, Blaschko, CVPR 2018, with classes = 'present') of the prediction P [C, H, W] or [1, C, H, W],
    read as fp32, against the index label [H, W] over the listed `classes`, in the semantics of include/sgan_hip.h,
    "Lovasz-softmax": (L, dL/dP [C, H, W], pi [n, N] int32, g [n, N], L_c [n], M).  Per listed class: fg = (label == c); a class
    without foreground takes no part (its g and L_c are 0); e = |fg - p| in fp32; pi sorts e descending, ties by the pixel index
    ascending -- the unique key ((0xFFFFFFFF - bits(e)) << 32) | i; with c_k the foreground among the first k + 1 sorted pixels,
    I = G - c_k and U = G + (k + 1 - c_k) in exact integers, g_k = 1 / U on a foreground pixel and I / (U (U - 1)) elsewhere, one
    fp64 division; L_c = sum e g in fp64; L the mean over the m present classes; dL/dp_pi(k) = sign(p - fg) g_k / m.  M = |dL/dP|,
    the scale of a rounding of the gradient."""
    P32 = np.ascontiguousarray(P, dtype=np.float32)
    if P32.ndim == 4:
        assert P32.shape[0] == 1, P32.shape
        P32 = P32[0]
    C, H, W = P32.shape
    N = H * W
    lab = np.asarray(label).reshape(N)
    classes = [int(c) for c in classes]
    assert len(set(classes)) == len(classes) and all(0 <= c < C for c in classes), classes
    n = len(classes)
    perm, g, Lc = np.zeros((n, N), np.int32), np.zeros((n, N), np.float64), np.zeros(n, np.float64)
    present = np.zeros(n, bool)
    sign = np.zeros((n, N), np.float64)
    idx = np.arange(N, dtype=np.uint64)
    for a, c in enumerate(classes):
        fg = lab == c
        p = P32[c].reshape(N)
        e = np.abs(fg.astype(np.float32) - p)                                # one fp32 subtraction
        key = ((np.uint64(0xFFFFFFFF) - e.view(np.uint32).astype(np.uint64)) << np.uint64(32)) | idx
        pi = np.argsort(key, kind="stable")
        perm[a] = pi
        sign[a] = np.sign(p.astype(np.float64) - fg)[pi]
        G = int(fg.sum())
        present[a] = G > 0
        if G == 0:
            continue
        f = fg[pi]
        ck = np.cumsum(f, dtype=np.int64)
        k1 = np.arange(1, N + 1, dtype=np.int64)
        I, U = G - ck, G + (k1 - ck)
        den = np.where(f, U, U * (U - 1))
        g[a] = np.where(f, 1, I).astype(np.float64) / den.astype(np.float64)
        Lc[a] = float(np.sum(e[pi].astype(np.float64) * g[a]))
    m = int(present.sum())
    dP = np.zeros((C, N), np.float64)
    for a, c in enumerate(classes):
        if present[a]:
            dP[c, perm[a]] = sign[a] * g[a] / m
    L = float(Lc.sum() / m) if m else 0.0
    dP = dP.reshape(C, H, W)
    return L, dP, perm, g, Lc, np.abs(dP)


def seg_terms_ref(logits, label_or_target, mode, classes=(), alpha=0.5, beta=0.5, smooth=1.0, power=1.0, focal_gamma=None,
                  class_weights=None):
    """The Tversky (soft Dice, focal-Tversky) and focal loss terms on the logits in NumPy fp64, in the semantics of
    include/sgan_hip.h, "Segmentation loss terms": (L_T, L_F, state [68], dz_T [npix, C], dz_F [npix, C]).

    logits [npix, C] (read as fp32); mode 0 (softmax): label_or_target the integer label [npix], p = softmax(z), t_c = [y == c], a
    pixel with a label outside [0, C) takes no part; mode 1 (sigmoid): the target [npix, C] in [0, 1], p = sigmoid(z).
    Tversky over the n listed classes (none: term off, L_T = 0): TP = sum p t, FP = sum p (1 - t), FN = sum (1 - p) t,
    D = TP + alpha FP + beta FN + smooth, TI = (TP + smooth) / D, L_c = (1 - TI)^power, L_T = mean over n; D == 0: L_c = 0, no
    gradient; 1 - TI == 0: derivative 0; G_c(t) = -(power / n) (1 - TI)^(power - 1) [t / D - (TP + smooth) (t (1 - beta) +
    alpha (1 - t)) / D^2]; softmax dz_k = p_k (G'_k - sum_j p_j G'_j), sigmoid dz_c = p_c (1 - p_c) G_c(t_c).
    Focal (focal_gamma None: off, L_F = 0), class weights w (None: 1): softmax, lp = z_y - logsumexp(z), pt = exp(lp):
    L_F = sum w[y] (1 - pt)^gamma (-lp) / sum w[y], dz_k = w[y] / norm [gamma pt (1 - pt)^(gamma - 1) lp - (1 - pt)^gamma]
    (delta_ky - p_k), the first product left out where gamma == 0 or 1 - pt == 0; sigmoid: L_F = sum w_c [t (1 - p)^gamma
    softplus(-z) + (1 - t) p^gamma softplus(z)] / (C npix) and its analytic derivative.
    state: [8 j + 0 .. 7] TP, FP, FN, D, TI, L_c, G_c(0), G_c(1) of listed class j; [64] focal numerator, [65] norm, [66] L_T, [67] L_F."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    assert z.ndim == 2, z.shape
    npix, C = z.shape
    classes = [int(c) for c in classes]
    n = len(classes)
    assert n <= 8 and len(set(classes)) == n and all(0 <= c < C for c in classes), classes
    softmax = int(mode) == 0
    state = np.zeros(68, np.float64)
    dzT, dzF = np.zeros((npix, C), np.float64), np.zeros((npix, C), np.float64)
    if softmax:
        y = np.asarray(label_or_target).reshape(npix).astype(np.int64)
        ok = (y >= 0) & (y < C)
        ys = np.where(ok, y, 0)
        m = z.max(axis=1, keepdims=True)
        lse = m[:, 0] + np.log(np.exp(z - m).sum(axis=1))
        p = np.exp(z - lse[:, None])
        t = np.zeros((npix, C), np.float64)
        t[np.arange(npix)[ok], y[ok]] = 1.0
        valid = ok.astype(np.float64)[:, None]
    else:
        t = np.asarray(label_or_target, dtype=np.float32).astype(np.float64).reshape(npix, C)
        p = 1.0 / (1.0 + np.exp(-z))
        q = 1.0 / (1.0 + np.exp(z))      # 1 - p
        valid = np.ones((npix, 1), np.float64)
    LT = 0.0
    Gp = np.zeros((npix, C), np.float64)      # G'_c per pixel, zero on unlisted channels
    for j, c in enumerate(classes):
        pc, tc, v = p[:, c], t[:, c], valid[:, 0]
        TP = float(np.sum(pc * tc * v))
        FP = float(np.sum(pc * (1.0 - tc) * v))
        FN = float(np.sum((1.0 - pc) * tc * v))
        D = ((TP + alpha * FP) + beta * FN) + smooth
        TI = Lc = G0 = G1 = 0.0
        if D > 0.0:
            num = TP + smooth
            TI = num / D
            u = max(1.0 - TI, 0.0)
            if u > 0.0:
                Lc = u ** power
                k = -(power / n) * u ** (power - 1.0)
                G0 = k * (-(num * alpha) / (D * D))
                G1 = k * (1.0 / D - (num * (1.0 - beta)) / (D * D))
        state[8 * j:8 * j + 8] = (TP, FP, FN, D, TI, Lc, G0, G1)
        LT += Lc
        Gp[:, c] = G0 + tc * (G1 - G0)
    if n:
        LT /= n
        if softmax:
            dzT = p * (Gp - np.sum(p * Gp, axis=1, keepdims=True)) * valid
        else:
            dzT = p * q * Gp
    LF = 0.0
    if focal_gamma is not None:
        g = float(focal_gamma)
        w = np.ones(C, np.float64)
        if class_weights is not None:
            cw = np.asarray(class_weights, dtype=np.float32).astype(np.float64).reshape(-1)
            w[:min(C, cw.size)] = cw[:C]
        if softmax:
            lp = z[np.arange(npix), ys] - lse
            pt = np.exp(lp)
            om = -np.expm1(lp)      # 1 - pt
            wy = w[ys] * ok
            num, norm = float(np.sum(wy * om ** g * -lp)), float(np.sum(wy))
            k = -(om ** g)
            if g != 0.0:
                nz = om != 0.0
                k = k + np.where(nz, g * pt * np.where(nz, om, 1.0) ** (g - 1.0) * lp, 0.0)
            if norm > 0.0:
                dzF = (wy / norm * k)[:, None] * (t - p) * valid
        else:
            spn = np.maximum(-z, 0.0) + np.log1p(np.exp(-np.abs(z)))      # softplus(-z)
            spp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))       # softplus(z)
            num, norm = float(np.sum(w * (t * q ** g * spn + (1.0 - t) * p ** g * spp))), float(C) * float(npix)
            dzF = w / norm * ((1.0 - t) * p ** g * (g * q * spp + p) - t * q ** g * (g * p * spn + q))
        LF = num / norm if norm > 0.0 else 0.0
        state[64], state[65] = num, norm
    state[66], state[67] = LT, LF
    return LT, LF, state, dzT, dzF


def dist_level_set(sdsq):
    """Kervadec's level set from a signed squared distance map (signed_edt_sq): the distance outside, -(distance - 1) inside, 0
    where the map is 0; float64."""
    s = np.asarray(sdsq).astype(np.float64)
    return np.where(s > 0, np.sqrt(np.abs(s)), np.where(s < 0, 1.0 - np.sqrt(np.abs(s)), 0.0))


def dist_terms_ref(logits, label_or_target, mode, cls, t_sdsq, p_sdsq=None, boundary=True, hausdorff_alpha=None):
    """The boundary loss (Kervadec et al., MIDL 2019) and the distance-transform Hausdorff loss (Karimi & Salcudean, TMI 2019, HD_DT)
    of one class on the logits in NumPy fp64, in the semantics of include/sgan_hip.h, "Distance-map loss terms":
    (L_B, L_H, state [5], dz_B [npix, C], dz_H [npix, C]), dz_X = dL_X/dz.

    logits [npix, C] (read as fp32); mode 0 (softmax): label_or_target the integer label [npix], p = softmax(z)_cls, g = [y == cls],
    a pixel with a label outside [0, C) takes no part; mode 1 (sigmoid): the target [npix, C], p = sigmoid(z_cls), g = target_cls.
    t_sdsq, p_sdsq: the signed squared distance maps (signed_edt_sq) of the truth and of the thresholded prediction, [npix] integers,
    constants.  N = npix.  Boundary (boundary False: off, L_B = 0): phi = dist_level_set(t_sdsq), L_B = sum phi p / N.  Hausdorff
    (hausdorff_alpha None: off, L_H = 0): F = |t_sdsq|^(alpha / 2) + |p_sdsq|^(alpha / 2), L_H = sum (p - g)^2 F / N.  With
    G = dL/dp: softmax dz_k = G p (delta_k,cls - p_k), sigmoid dz_cls = G p (1 - p).  state: sum phi p, sum (p - g)^2 F, N, L_B, L_H."""
    z = np.asarray(logits, dtype=np.float32).astype(np.float64)
    assert z.ndim == 2, z.shape
    npix, C = z.shape
    cls = int(cls)
    assert 0 <= cls < C, (cls, C)
    t_s = np.asarray(t_sdsq).reshape(npix).astype(np.int64)
    if int(mode) == 0:
        y = np.asarray(label_or_target).reshape(npix).astype(np.int64)
        valid = ((y >= 0) & (y < C)).astype(np.float64)
        m = z.max(axis=1, keepdims=True)
        E = np.exp(z - m)
        P = E / E.sum(axis=1, keepdims=True)
        p = P[:, cls]
        g = (y == cls).astype(np.float64)
        dpdz = -p[:, None] * P
        dpdz[:, cls] = p * (np.delete(E, cls, axis=1).sum(axis=1) / E.sum(axis=1))      # 1 - p without the cancellation
    else:
        t = np.asarray(label_or_target, dtype=np.float32).astype(np.float64).reshape(npix, C)
        valid = np.ones(npix, np.float64)
        p = 1.0 / (1.0 + np.exp(-z[:, cls]))
        q = 1.0 / (1.0 + np.exp(z[:, cls]))      # 1 - p
        g = t[:, cls]
        dpdz = np.zeros((npix, C), np.float64)
        dpdz[:, cls] = p * q
    N = float(npix)
    state = np.zeros(5, np.float64)
    state[2] = N
    dzB, dzH = np.zeros((npix, C), np.float64), np.zeros((npix, C), np.float64)
    LB = LH = 0.0
    if boundary:
        phi = dist_level_set(t_s)
        state[0] = float(np.sum(phi * p * valid))
        LB = state[0] / N
        dzB = (phi * valid / N)[:, None] * dpdz
    if hausdorff_alpha is not None:
        a = float(hausdorff_alpha)
        assert 0.0 < a <= 4.0, a
        p_s = np.asarray(p_sdsq).reshape(npix).astype(np.int64)
        if a == 2.0:
            F = (np.abs(t_s) + np.abs(p_s)).astype(np.float64)
        else:
            F = np.abs(t_s).astype(np.float64) ** (a / 2.0) + np.abs(p_s).astype(np.float64) ** (a / 2.0)
        state[1] = float(np.sum((p - g) ** 2 * F * valid))
        LH = state[1] / N
        dzH = (2.0 * (p - g) * F * valid / N)[:, None] * dpdz
    state[3], state[4] = LB, LH
    return LB, LH, state, dzB, dzH


# ---- photometric augmentation of a training crop (--photo_aug): the parameter draw of the feeders and the yardsticks
# of sgan_image_photo --------------------------------------------------------------------------------------------------------------
PHOTO_STAGES = ('blur', 'gamma', 'contrast', 'brightness', 'noise', 'occlude')      # the order they are drawn and applied in
PHOTO_MAX_R, PHOTO_MAX_BOX = 12, 4      # SGAN_PHOTO_MAX_R, SGAN_PHOTO_MAX_BOX
PHOTO_POW_ULP = 4       # what the bounds allow powf, in ulps of its result (chosen before any run: DESIGN.md R38)
# one fp32 rounding, relative; the factor pays for the float64 evaluation of the end points themselves
PHOTO_U = 2.0 ** -24 * (1.0 + 2.0 ** -20)
_PHOTO_TINY = 2.0 ** -149


def _f32(v):
    return float(np.float32(v))


class PhotoRec:
    """The parameters of one sgan_image_photo call, as the fp32 values the device receives (sgan_photo_rec), and the 64-bit `seed`
    of the noise planes, which the caller of ops.normal_fill uses and the kernel never sees.  boxes: (y0, y1, x0, x1, value), rows
    [y0, y1) x columns [x0, x1).  The defaults are the neutral values: PhotoRec() is the bitwise copy."""

    def __init__(self, taps=(1.0,), gamma=1.0, contrast=1.0, brightness=0.0, sigma_n=0.0, boxes=(), seed=0):
        self.w = np.asarray(taps, dtype=np.float32).reshape(-1)
        assert 1 <= len(self.w) <= PHOTO_MAX_R + 1, len(self.w)
        self.gamma, self.contrast, self.brightness, self.sigma_n = _f32(gamma), _f32(contrast), _f32(brightness), _f32(sigma_n)
        self.boxes = [(int(y0), int(y1), int(x0), int(x1), _f32(v)) for y0, y1, x0, x1, v in boxes]
        self.seed = int(seed) & (2 ** 64 - 1)

    @property
    def R(self):
        return len(self.w) - 1

    def point_stages(self, noise):
        """(gamma, contrast / brightness, noise) run: the device's rule for skipping a neutral stage."""
        return self.gamma != 1.0, self.contrast != 1.0 or self.brightness != 0.0, noise is not None and self.sigma_n != 0.0

    def __repr__(self):
        return 'PhotoRec(R=%d, gamma=%r, contrast=%r, brightness=%r, sigma_n=%r, boxes=%r, seed=%d)' % (
            self.R, self.gamma, self.contrast, self.brightness, self.sigma_n, self.boxes, self.seed)


def photo_taps(sigma):
    """The fp32 taps w[0 .. R] of the blur: R = min(12, ceil(3 sigma)), w_k = exp(-k^2 / (2 sigma^2)) in float64, normalised so that
    w_0 + 2 sum_{k >= 1} w_k = 1, then rounded to fp32."""
    sigma = float(sigma)
    assert sigma > 0.0, sigma
    R = min(PHOTO_MAX_R, int(np.ceil(3.0 * sigma)))
    w = np.exp(-np.arange(R + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


def photo_draw(opt, n, rng=random):
    """The PhotoRec of one n x n training crop under --photo_aug, from Python's `random` (or `rng`: anything with random() and
    getrandbits(64)).  The six stages are visited in the order of PHOTO_STAGES.  A stage that --photo_aug does not list draws nothing.
    A listed stage draws its gate g = random() and fires when g < --photo_prob; a stage that does not fire draws nothing else.  A stage
    that fires then draws, with r = random() anew each time:
        blur        sigma = 0.5 + (SMAX - 0.5) r                                                   -> photo_taps(sigma)
        gamma       gamma = exp((2 r - 1) ln G)
        contrast    c = 1 - C + 2 C r
        brightness  b = (2 r - 1) B
        noise       sigma_n = S r, then seed = getrandbits(64)
        occlude     for each of the K boxes: h = int(1 + r (m - 1)), w = int(1 + r (m - 1)) with m = max(1, FRAC n), then
                    y0 = int(r (n - h + 1)), x0 = int(r (n - w + 1)), value = 2 r - 1              (five draws a box)
    so a call makes len(--photo_aug) gate draws and 1, 1, 1, 1, 2, 5 K further ones for the stages that fire."""
    stages, prob = opt.photo_aug, float(opt.photo_prob)
    kw = {}
    for stage in PHOTO_STAGES:
        if stage not in stages or not rng.random() < prob:
            continue
        if stage == 'blur':
            kw['taps'] = photo_taps(0.5 + (float(opt.photo_blur) - 0.5) * rng.random())
        elif stage == 'gamma':
            kw['gamma'] = float(np.exp((2.0 * rng.random() - 1.0) * np.log(float(opt.photo_gamma))))
        elif stage == 'contrast':
            kw['contrast'] = 1.0 - float(opt.photo_contrast) + 2.0 * float(opt.photo_contrast) * rng.random()
        elif stage == 'brightness':
            kw['brightness'] = (2.0 * rng.random() - 1.0) * float(opt.photo_brightness)
        elif stage == 'noise':
            kw['sigma_n'] = float(opt.photo_noise) * rng.random()
            kw['seed'] = rng.getrandbits(64)
        else:
            K, frac = int(opt.photo_occlude[0]), float(opt.photo_occlude[1])
            m, boxes = max(1.0, frac * n), []
            for _ in range(K):
                h, w = int(1.0 + rng.random() * (m - 1.0)), int(1.0 + rng.random() * (m - 1.0))
                y0, x0 = int(rng.random() * (n - h + 1)), int(rng.random() * (n - w + 1))
                boxes.append((y0, y0 + h, x0, x0 + w, 2.0 * rng.random() - 1.0))
            kw['boxes'] = boxes
    return PhotoRec(**kw)


def _photo_blur_pass(a, w, axis):
    """w[0] a + sum_k w[k] (a shifted by -k + a shifted by +k) along `axis` of a float64 array, indices mirrored into the array."""
    N = a.shape[axis]
    idx = np.arange(N)
    out = float(w[0]) * a
    for k in range(1, len(w)):
        out = out + float(w[k]) * (np.take(a, _mirror_index(idx - k, N), axis=axis) + np.take(a, _mirror_index(idx + k, N), axis=axis))
    return out


def _photo_rn(lo, hi, budget):
    """The interval after one fp32 rounding to nearest: rounding is monotone and moves x by at most 2^-24 |x|."""
    if not budget:
        return lo, hi
    return lo - PHOTO_U * np.abs(lo) - _PHOTO_TINY, hi + PHOTO_U * np.abs(hi) + _PHOTO_TINY


def _photo_channel(lo, hi, rec, nz, yy, xx, budget):
    """One masked channel through the six stages as the interval [lo, hi] of float64 [H, W] planes.  Every stage is monotone
    (non-negative taps, pow on [0, 1], contrast > 0, an added constant, clamps), so a stage maps end point to end point; with
    `budget` every device rounding then widens the interval (DESIGN.md R38 counts them), without it lo == hi is the float64 value."""
    R = rec.R
    if R > 0:
        for axis in (1, 0):      # rows first, then columns
            mag = max(1.0, float(np.abs(lo).max()), float(np.abs(hi).max()))
            lo, hi = _photo_blur_pass(lo, rec.w, axis), _photo_blur_pass(hi, rec.w, axis)
            if budget:      # (2 R + 2) roundings a pass, each of a value no larger than the largest input (the taps sum to 1)
                e = (2 * R + 2) * PHOTO_U * mag
                lo, hi = lo - e, hi + e
    do_gamma, do_cb, do_noise = rec.point_stages(nz)
    if do_gamma:
        lo, hi = _photo_rn(0.5 * lo + 0.5, 0.5 * hi + 0.5, budget)
        lo, hi = np.clip(lo, 0.0, 1.0) ** rec.gamma, np.clip(hi, 0.0, 1.0) ** rec.gamma
        if budget:      # powf: PHOTO_POW_ULP ulps of the result, an ulp being at most 2^-23 of it
            lo, hi = lo - PHOTO_POW_ULP * 2.0 * PHOTO_U * lo - _PHOTO_TINY, hi + PHOTO_POW_ULP * 2.0 * PHOTO_U * hi + _PHOTO_TINY
            lo = np.maximum(lo, 0.0)      # powf of a value in [0, 1] is not negative
        lo, hi = _photo_rn(2.0 * lo - 1.0, 2.0 * hi - 1.0, budget)
    if do_cb:
        lo, hi = _photo_rn(rec.contrast * lo + 2.0 * rec.brightness, rec.contrast * hi + 2.0 * rec.brightness, budget)
    if do_noise:
        lo, hi = _photo_rn(lo + rec.sigma_n * nz, hi + rec.sigma_n * nz, budget)
    if do_gamma or do_cb or do_noise:
        lo, hi = np.clip(lo, -1.0, 1.0), np.clip(hi, -1.0, 1.0)
    for y0, y1, x0, x1, value in rec.boxes:      # a later box wins
        inside = (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
        lo, hi = np.where(inside, value, lo), np.where(inside, value, hi)
    return lo, hi


def _photo_run(x, rec, mask, noise, budget):
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 3, (x.dtype, x.shape)
    H, W, C = x.shape
    chans = [c for c in range(C) if (int(mask) >> c) & 1]
    assert int(mask) >> C == 0 and 0 <= rec.R <= min(PHOTO_MAX_R, H - 1, W - 1) and len(rec.boxes) <= PHOTO_MAX_BOX, (mask, C, rec)
    if noise is not None:
        noise = np.asarray(noise)
        assert noise.dtype == np.float32 and noise.shape == (len(chans), H, W), (noise.dtype, noise.shape)
    yy, xx = np.mgrid[:H, :W]
    with np.errstate(invalid='ignore'):      # a channel that is only copied may hold any bits, a signalling NaN among them
        lo, hi = x.astype(np.float64), x.astype(np.float64)
    for j, c in enumerate(chans):
        plane = x[..., c].astype(np.float64)
        assert np.abs(plane).max() <= 1.0, "image channels hold values in [-1, 1]"
        nz = None if noise is None else noise[j].astype(np.float64)
        lo[..., c], hi[..., c] = _photo_channel(plane, plane.copy(), rec, nz, yy, xx, budget)
    return lo, hi


def photo_ref(x, rec, mask, noise=None):
    """The host yardstick of ops.image_photo (sgan_image_photo) in float64: x [H, W, C] fp32 with values in [-1, 1] in the channels
    whose bit is set in `mask`, rec a PhotoRec, noise [popcount(mask), H, W] fp32 or None -> float64 [H, W, C].  The six stages on the
    fp32 parameters, a neutral stage skipped as on the device; every other channel is x.  The trainers do not call it."""
    return _photo_run(x, rec, mask, noise, False)[0]


def photo_bounds(x, rec, mask, noise=None):
    """(lo, hi), float64 [H, W, C]: the interval every element of the device's result must lie in, lo <= got <= hi -- photo_ref with
    the device's fp32 roundings counted stage by stage, no tuned tolerance.  Channels outside the mask, and every
    channel of the all-neutral record, have lo == hi == x: the bits."""
    return _photo_run(x, rec, mask, noise, True)
