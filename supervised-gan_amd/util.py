"""Image and metric helpers of the drivers (util/util.py:15-28, :41-43, :86-128 of the reference): tensor -> uint8 image -> PNG,
the Rand F-score of a binary segmentation, and the information score (VInfo) that goes with it."""
import os

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
