"""Inputs and recorded results of the thinning tests (tests/test_thin_host.py on the host rule util.thin, tests/test_hip_thin.py on
the kernel): the fixed and the random cases of the thinning rule, each with the pixel count and the number of changing iterations
it must give.  The figures were produced by an independent restatement of Guo-Hall thinning (scipy ndimage.correlate over a
256-entry table) and are not regenerated from the code under test."""
import functools

import numpy as np


def _band():
    m = np.zeros((40, 200), bool)
    m[5:35, 3:197] = True
    return m


def _small_band():
    m = np.zeros((7, 9), bool)
    m[2:5, 1:8] = True
    return m


def _line():
    m = np.zeros((9, 40), bool)
    m[4, 3:30] = True
    return m


def _dot():
    m = np.zeros((9, 11), bool)
    m[4, 5] = True
    return m


def _frame():
    m = np.ones((20, 20), bool)
    m[3:17, 3:17] = False
    return m


# name -> (mask, kept pixels, changing iterations)
FIXED = {
    "ones64": (lambda: np.ones((64, 64), bool), 1, 32),
    "ones17x130": (lambda: np.ones((17, 130), bool), 114, 8),
    "band40x200": (_band, 165, 15),
    "band7x9": (_small_band, 5, 1),
    "line": (_line, 27, 0),
    "dot": (_dot, 1, 0),
    "frame20": (_frame, 62, 3),
}

# seed -> (H, W, density, kept, set pixels of the input, changing iterations, kept after max_num_iter = 1, 2, 3 or None)
RANDOM = {
    1: (7, 5, 0.7, 15, 24, 3, (17, 16, 15)),
    2: (33, 70, 0.9, 838, 2071, 12, (1826, 1564, 1350)),
    3: (64, 64, 0.5, 1537, 2047, 3, None),
    4: (65, 129, 0.9, 3112, 7513, 21, (6854, 6070, 5393)),
    5: (97, 131, 0.8, 5935, 10162, 14, None),
    6: (130, 67, 0.95, 2161, 8293, 32, None),
}


def fixed(name):
    return FIXED[name][0]()


def random_mask(seed):
    H, W, d = RANDOM[seed][:3]
    return np.random.default_rng(seed).random((H, W)) < d


@functools.lru_cache(maxsize=None)
def host_thin(name, max_num_iter=None):
    """util.thin of a case (a FIXED name or a RANDOM seed), computed once per session; do not modify the arrays it returns."""
    from supervised_gan_amd.util import thin
    m = fixed(name) if name in FIXED else random_mask(name)
    out, n = thin(m, max_num_iter)
    out.setflags(write=False)
    return out, n
