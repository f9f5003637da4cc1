#!/usr/bin/env python3
"""Sliced Wasserstein distance between two image sets over Laplacian-pyramid patches (Karras et al. 2018, "Progressive growing of
GANs", section 5): one number per scale that says how far the generated images' local statistics are from the real ones', from the
images alone -- no pretrained network.

`--swd_pair real_fake` (default): set A is the dataset's real images, set B what `model.test()` makes of a loaded checkpoint
(`--use_ema` as in test.py) -- `--model fcgan`: `model.fake` from noise; `--model cgan` / `cgan2`: `fake_B` rendered from the dataset's
own `real_A`, against its `real_B`.  `--swd_pair real_real`: the dataset split into its even and odd files, no generator involved --
the floor a real_fake score is read against.  Per image, on the device and without a synchronisation: the Laplacian pyramid
(ops.lap_pyramid; a further level while both sides are even and half the smaller is at least 16) and, per level, `--swd_patches`
7 x 7 patches copied into the set's descriptor matrix with their per-channel sums (ops.swd_gather).  After the loop one
ops.swd_distances call per level -- normalise, project onto `--swd_dirs` unit directions, sort, compare -- and one read-back.

Each set is normalised by its OWN per-channel mean and standard deviation, level by level, as in the paper: the score is blind to a
global brightness or contrast change of one set and measures structure only.  Positions and directions come from util.swd_draw
alone (`--swd_seed`); both sets share the directions.  In real_fake each set draws its own positions; in real_real both halves
use one draw, so that a set split against itself scores exactly 0 and the floor is the image-to-image variation alone.

N = how_many * swd_patches descriptors per set, at most 16384 (what one workgroup sorts in LDS), and every image of a run has one
size; anything else exits with status 2.

`--prd_k K` (default 0: off, and then nothing of the run or its files changes) adds, per level and in the same descriptor space,
improved precision / recall (Kynkaanniemi et al. 2019) and density / coverage (Naeem et al. 2020): balls around every descriptor
that reach its K-th nearest neighbour among the patches of OTHER images of its set (the patches of one image overlap, and repeat at
coarse levels, so they do not count as neighbours).  Here BOTH sets are normalised by set A's statistics -- the two sets must live
in one space -- unlike the distances above.  precision: share of set B's patches inside some ball of A ("share of generated local
textures that occur in real images" -- patch descriptors are not image features); recall: share of A's patches inside some ball of
B; density: B's ball hits / (K N); coverage: share of A's patches whose nearest patch of B lies inside their own ball; and, to tell
copying from fidelity, nn_fake_real (median squared distance of a patch of B to its nearest patch of A) beside nn_real_real (of a
patch of A to its nearest patch of another image of A) and their quotient nn_ratio: far below 1 means the generated patches sit
closer to training patches than training patches of different images sit to each other.  K is 1..8 and at most N - swd_patches
(every patch needs K neighbours in other images); anything else exits with status 2 before anything runs.  ops.knn_radii twice,
ops.prd_rows twice and ops.prd_finish once per level, read back with the distances; prd.txt and prd.npz are written beside swd.txt.

Written under results_dir/name/<phase>_<which_epoch>/: swd.npz (distances [levels,
dirs], sizes, scores, the options) and swd.txt (one line `<H>x<W>: <score x 1e3>` per level, and their average)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from supervised_gan_amd.options import TestOptions  # noqa: E402
from supervised_gan_amd.synthetic_data import SyntheticDataset  # noqa: E402
from supervised_gan_amd.util import PRD_MAX_K, SWD_MAX_N, SWD_PATCH, lap_level_sizes, prd_from_counts, prd_ratio, swd_draw  # noqa: E402

MODELS = ('fcgan', 'cgan', 'cgan2')
MAX_DIRS = 4096
PRD_KEYS = ('precision', 'recall', 'density', 'coverage', 'nn_fake_real', 'nn_real_real', 'nn_ratio')


def _swd_args(argv):
    """The driver's own flags, split off before TestOptions parses the rest."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--swd_pair', choices=('real_fake', 'real_real'), default='real_fake')
    p.add_argument('--swd_patches', type=int, default=128, help='patches per image and level')
    p.add_argument('--swd_dirs', type=int, default=512, help='projection directions per level')
    p.add_argument('--swd_seed', type=int, default=0)
    p.add_argument('--swd_channels', type=int, nargs='+', default=None,
                   help='indices into the generated side\'s channels of --which_channel (default: all of them)')
    p.add_argument('--prd_k', type=int, default=0,
                   help='> 0: precision / recall / density / coverage with k-th-nearest-neighbour balls (1..8); 0: off')
    return p.parse_known_args(argv)


def _refuse(msg):
    print('swd.py: ' + msg, file=sys.stderr)
    raise SystemExit(2)


def side_channels(opt, pair):
    """RGB indices of the channels that are scored before --swd_channels picks among them: the generated side of --which_channel
    (cgan 'rg_b': b), all of them for fcgan and for real_real."""
    parts = opt.which_channel.split('_')
    if pair == 'real_fake' and opt.model in ('cgan', 'cgan2'):
        if len(parts) != 2:
            _refuse('--model %s reads --which_channel as <input>_<output> (got %s)' % (opt.model, opt.which_channel))
        parts = parts[1:]
    return ['rgb'.index(c) for c in ''.join(parts)]


def summary_text(sizes, scores):
    lines = ['%dx%d: %.6f' % (h, w, s * 1e3) for (h, w), s in zip(sizes, scores)]
    lines.append('average: %.6f' % (float(np.mean(scores)) * 1e3))
    return '\n'.join(lines) + '\n'


def prd_summary_text(sizes, prd):
    """prd: {key: [levels]} of PRD_KEYS."""
    fmt = ' '.join('%s %%.6f' % key for key in PRD_KEYS)
    lines = ['%dx%d: ' % (h, w) + fmt % tuple(prd[key][l] for key in PRD_KEYS) for l, (h, w) in enumerate(sizes)]
    lines.append('average: ' + fmt % tuple(float(np.mean(prd[key])) for key in PRD_KEYS))
    return '\n'.join(lines) + '\n'


def _median64(x):
    """numpy's median of a float32 vector, on the device in float64: the mean of the two middle values of an even count."""
    s = x.double().sort().values
    n = s.numel()
    return (s[(n - 1) // 2] + s[n // 2]) * 0.5


class _Sets:
    """The two descriptor matrices per level, filled image by image.  Enqueues only."""

    def __init__(self, sargs, how_many, n_channels, dev, same_positions):
        self.sargs, self.how_many, self.C, self.dev, self.same = sargs, how_many, n_channels, dev, same_positions
        self.sizes = None
        self.count = [0, 0]

    def _setup(self, H, W):
        import torch
        P, J, K, N = self.sargs.swd_patches, self.sargs.swd_dirs, self.C * SWD_PATCH * SWD_PATCH, self.how_many * self.sargs.swd_patches
        self.sizes = lap_level_sizes(H, W)
        if min(self.sizes[-1]) < SWD_PATCH:
            _refuse('images of %d x %d are smaller than a %d x %d patch' % (H, W, SWD_PATCH, SWD_PATCH))
        self.pos, self.dirs = [[], []], []
        for l, (h, w) in enumerate(self.sizes):
            for s in (0, 1):
                pos, dirs = swd_draw(self.sargs.swd_seed, l, self.how_many, P, h, w, K, J, set_index=0 if self.same else s)
                self.pos[s].append(torch.from_numpy(pos).to(self.dev))
            self.dirs.append(torch.from_numpy(dirs).to(self.dev))
        self.desc = [[torch.zeros((N, K), dtype=torch.float32, device=self.dev) for _ in self.sizes] for _ in (0, 1)]
        self.acc = [[torch.zeros(2 * self.C, dtype=torch.float64, device=self.dev) for _ in self.sizes] for _ in (0, 1)]

    def add(self, s, img):
        """img: [C, H, W] float32 on the device, the next image of set s."""
        from supervised_gan_amd import ops
        H, W = img.shape[1:]
        if self.sizes is None:
            self._setup(H, W)
        if (H, W) != self.sizes[0]:
            _refuse('every image of a run has one size: %d x %d after %d x %d (at most %d descriptors of one level per set)'
                    % ((H, W) + self.sizes[0] + (SWD_MAX_N,)))
        i, P = self.count[s], self.sargs.swd_patches
        for l, level in enumerate(ops.lap_pyramid(img)):
            ops.swd_gather(level, self.pos[s][l][i * P:(i + 1) * P], self.desc[s][l], i * P, self.acc[s][l])
        self.count[s] = i + 1

    def distances(self):
        """[levels, J] float64 on the device: one call per level."""
        import torch
        from supervised_gan_amd import ops
        return torch.stack([ops.swd_distances(self.desc[0][l], self.desc[1][l], self.acc[0][l], self.acc[1][l], self.dirs[l])
                            for l in range(len(self.sizes))])

    def prd(self, k):
        """[levels, 6] float64 on the device: the four counts of ops.prd_finish (exact in float64) and the medians of the nearest
        fake-to-real and real-to-real squared distances.  Both sets in set A's normalisation; group = the patches of one image."""
        import torch
        from supervised_gan_amd import ops
        rows, P = [], self.sargs.swd_patches
        for l in range(len(self.sizes)):
            A, B, stats = self.desc[0][l], self.desc[1][l], self.acc[0][l]
            radA, nn1A = ops.knn_radii(A, stats, k, P)
            radB, _ = ops.knn_radii(B, stats, k, P)
            cntB, nnB, _ = ops.prd_rows(B, A, stats, radA)
            cntA, nnA, _ = ops.prd_rows(A, B, stats, radB)
            rows.append(torch.cat([ops.prd_finish(cntB, cntA, nnA, radA).double(), torch.stack([_median64(nnB), _median64(nn1A)])]))
        return torch.stack(rows)


def main(argv=None, keep=None):
    """keep: an optional dict that receives {'A': [...], 'B': [...]}, the planar images of the two sets as they were scored (device
    tensors; nothing is read back for it)."""
    argv = sys.argv[1:] if argv is None else list(argv)
    sargs, rest = _swd_args(argv)
    opt = TestOptions().parse(rest, save=False)
    opt.nThreads, opt.batchSize, opt.serial_batches, opt.no_flip, opt.no_rotate = 1, 1, True, True, True
    fake = sargs.swd_pair == 'real_fake'
    if fake and opt.model not in MODELS:
        _refuse('--swd_pair real_fake scores the generators of --model %s (got --model %s); --swd_pair real_real measures any dataset'
                % (' / '.join(MODELS), opt.model))
    if sargs.swd_patches < 1 or opt.how_many < 1 or not 1 <= sargs.swd_dirs <= MAX_DIRS:
        _refuse('--swd_patches and --how_many are at least 1 and --swd_dirs is 1..%d' % MAX_DIRS)
    N = opt.how_many * sargs.swd_patches
    if N > SWD_MAX_N:
        _refuse('N = how_many * swd_patches = %d * %d = %d descriptors per set; the limit is %d'
                % (opt.how_many, sargs.swd_patches, N, SWD_MAX_N))
    if sargs.prd_k and not 1 <= sargs.prd_k <= min(PRD_MAX_K, N - sargs.swd_patches):
        _refuse('--prd_k is 0 (off) or 1..%d and at most N - swd_patches = %d - %d = %d: every patch needs that many neighbours among '
                'the patches of other images (got %d); a level with fewer is refused, not scored'
                % (PRD_MAX_K, N, sargs.swd_patches, N - sargs.swd_patches, sargs.prd_k))
    side = side_channels(opt, sargs.swd_pair)
    picks = list(range(len(side))) if sargs.swd_channels is None else sargs.swd_channels
    if not 1 <= len(picks) <= 3 or any(not 0 <= c < len(side) for c in picks):
        _refuse('--swd_channels picks 1..3 of the %d channels of the generated side of --which_channel %s (got %s)'
                % (len(side), opt.which_channel, picks))
    if not opt.gpu_ids:
        _refuse('the measurement runs on the GPU (--gpu_ids 0)')

    import torch
    from supervised_gan_amd import ops
    dev = torch.device('cuda', opt.gpu_ids[0])
    sets = _Sets(sargs, opt.how_many, len(picks), dev, same_positions=not fake)
    if keep is not None:
        keep.update(A=[], B=[])

    def add(s, x):
        """x: [C, H, W] with any strides, the scored channels of the next image of set s."""
        x = x.detach().to(dev, dtype=torch.float32, non_blocking=True).contiguous()
        if keep is not None:
            keep['AB'[s]].append(x)
        sets.add(s, x)

    def dataset():
        if opt.dataroot == 'synthetic':
            return SyntheticDataset(opt, opt.how_many * (1 if fake else 2))
        from supervised_gan_amd.data import create_dataset
        return create_dataset(opt)

    if not fake:
        rgb = [side[c] for c in picks]
        which = 'B' if opt.which_direction in ('B', 'BtoA') and opt.dataset_mode != 'single' else 'A'
        for i, data in enumerate(dataset()):
            if i >= 2 * opt.how_many:
                break
            add(i & 1, data[which][0, rgb])
    elif opt.model == 'fcgan':
        from supervised_gan_amd.models import create_model
        model = create_model(opt)
        rgb = [side[c] for c in picks]
        which = 'A' if opt.which_direction == 'A' else 'B'
        for i, data in enumerate(dataset()):
            if i >= opt.how_many:
                break
            add(0, data[which][0, rgb])
            model.test()
            add(1, model.fake[0, picks])
    else:
        from supervised_gan_amd.models import create_model
        model = create_model(opt)
        for i, data in enumerate(dataset()):
            if i >= opt.how_many:
                break
            model.set_input(data)
            model.test()
            add(0, model.input_B[0, picks])
            add(1, model.fake_B[0, picks])
    if sets.count != [opt.how_many, opt.how_many]:
        _refuse('the dataset gave %d and %d images for the two sets; --how_many %d needs %d files'
                % (sets.count[0], sets.count[1], opt.how_many, opt.how_many * (1 if fake else 2)))

    if sargs.prd_k:
        L, J = len(sets.sizes), sargs.swd_dirs
        both = torch.cat([sets.distances().reshape(-1), sets.prd(sargs.prd_k).reshape(-1)]).cpu().numpy()      # the one read-back
        dist, prd_raw = both[:L * J].reshape(L, J), both[L * J:].reshape(L, 6)
    else:
        dist = sets.distances().cpu().numpy()      # the one read-back
    ops.check_metric_err(dev)
    scores = dist.mean(axis=1)
    out_dir = os.path.join(opt.results_dir, opt.name, '%s_%s' % (opt.phase, opt.which_epoch))
    os.makedirs(out_dir, exist_ok=True)
    npz, txt = os.path.join(out_dir, 'swd.npz'), os.path.join(out_dir, 'swd.txt')
    own = {k: v for k, v in vars(sargs).items() if k != 'prd_k' or v}      # without --prd_k, swd.npz is what it was before the flag existed
    options = {k: str(v) for k, v in sorted(list(vars(opt).items()) + list(own.items()))}
    np.savez(npz, distances=dist, sizes=np.array(sets.sizes, dtype=np.int64), scores=scores, channels=np.array(picks, dtype=np.int64),
             option_names=np.array(list(options)), option_values=np.array(list(options.values())))
    text = summary_text(sets.sizes, scores)
    with open(txt, 'w') as f:
        f.write(text)
    print(text, end='')
    if sargs.prd_k:
        counts = np.rint(prd_raw[:, :4]).astype(np.int64)
        prd = {key: [] for key in PRD_KEYS}
        for l in range(len(sets.sizes)):
            level = prd_from_counts(counts[l], N, sargs.prd_k)
            level.update(nn_fake_real=float(prd_raw[l, 4]), nn_real_real=float(prd_raw[l, 5]), nn_ratio=prd_ratio(prd_raw[l, 4], prd_raw[l, 5]))
            for key in PRD_KEYS:
                prd[key].append(level[key])
        np.savez(os.path.join(out_dir, 'prd.npz'), counts=counts, sizes=np.array(sets.sizes, dtype=np.int64), k=np.int64(sargs.prd_k),
                 N=np.int64(N), group=np.int64(sargs.swd_patches), channels=np.array(picks, dtype=np.int64),
                 option_names=np.array(list(options)), option_values=np.array(list(options.values())),
                 **{key: np.array(prd[key], dtype=np.float64) for key in PRD_KEYS})
        text = prd_summary_text(sets.sizes, prd)
        with open(os.path.join(out_dir, 'prd.txt'), 'w') as f:
            f.write(text)
        print(text, end='')
    return npz, txt


if __name__ == '__main__':
    main()
