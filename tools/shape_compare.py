#!/usr/bin/env python3
"""Compare the region shape statistics of two runs of shape_stats.py (typically --shape_source fake against real):

    python tools/shape_compare.py a/shape_stats.npz b/shape_stats.npz [--all]

For every feature of util.region_props, and for the number of regions per image, prints the two-sample Kolmogorov-Smirnov statistic
and the 1-D Wasserstein distance between the two samples (scipy.stats.ks_2samp, wasserstein_distance): one line
`feature  ks  wasserstein  n_a  n_b` each.  Regions that touch the image border are cut by it and are left out unless --all is given.
Identical files give 0 everywhere."""
import argparse
import sys

import numpy as np
from scipy import stats


def load(path, keep_border):
    z = np.load(path, allow_pickle=False)
    names = [str(n) for n in z["prop_names"]]
    props, table = z["props"], z["table"]
    keep = np.ones(len(props), bool) if keep_border else props[:, names.index("touches_border")] == 0
    per_image = np.bincount(table[keep, 12], minlength=int(z["images"])).astype(np.float64)
    return names, props[keep], per_image


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--all", action="store_true", help="keep the regions that touch the image border")
    a = ap.parse_args(argv)
    names, pa, na = load(a.a, a.all)
    names_b, pb, nb = load(a.b, a.all)
    if names != names_b:
        print("shape_compare.py: the two files hold different features", file=sys.stderr)
        raise SystemExit(2)
    print("# %-20s %10s %14s %8s %8s" % ("feature", "ks", "wasserstein", "n_a", "n_b"))
    samples = [(n, pa[:, i], pb[:, i]) for i, n in enumerate(names) if n != "touches_border"] + [("regions_per_image", na, nb)]
    for name, x, y in samples:
        x, y = x[np.isfinite(x)], y[np.isfinite(y)]
        if len(x) == 0 or len(y) == 0:
            print("%-22s %10s %14s %8d %8d" % (name, "nan", "nan", len(x), len(y)))
            continue
        print("%-22s %10.6f %14.6f %8d %8d" % (name, stats.ks_2samp(x, y).statistic, stats.wasserstein_distance(x, y), len(x), len(y)))


if __name__ == "__main__":
    main()
