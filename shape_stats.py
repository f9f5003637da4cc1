#!/usr/bin/env python3
"""Region shape statistics of generated or real images: the measurement the reference's paper judges a generator by (shape features
of the generated cells and mitochondria against the real ones; the reference ships only MATLAB that loads precomputed features).

`--shape_source fake` loads `<which_epoch>_net_G.pth` of an fcgan run and samples `model.test()` `--how_many` times, as test.py
does; `--shape_source real` walks the dataset (or `--dataroot synthetic`) and measures the images themselves, no generator involved.
Per image, on the device and without a synchronisation: channel `--shape_channel` of the model's channels (`--which_channel`) is
rescaled from [-1, 1] to [0, 1], its regions are labelled (ops.ccl_label: `--shape_objects free` labels the pixels <= 0.5, the cells
a membrane channel encloses; `wall` labels the complement 1 - x, the bright objects of a mitochondria channel) and measured into one
table (ops.region_stats).  The table is read back once after the loop.  Written under results_dir/name/<phase>_<which_epoch>/:
shape_stats.npz (table, props, prop_names, images, shape and the options) and shape_stats.txt (regions per image, and quantiles of
area, eccentricity and compactness over the regions that do not touch the border).  tools/shape_compare.py compares two such files."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from supervised_gan_amd.options import TestOptions  # noqa: E402
from supervised_gan_amd.synthetic_data import SyntheticDataset  # noqa: E402

QUANTILES = (0.05, 0.25, 0.5, 0.75, 0.95)


def _shape_args(argv):
    """The driver's own flags, split off before TestOptions parses the rest."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--shape_source', choices=('fake', 'real'), default='fake')
    p.add_argument('--shape_channel', type=int, default=0, help='index into the channels --which_channel selects')
    p.add_argument('--shape_objects', choices=('free', 'wall'), default='free')
    p.add_argument('--shape_capacity', type=int, default=1 << 18, help='rows of the region table (16 int64 each)')
    return p.parse_known_args(argv)


def selected_channels(which_channel):
    """RGB indices of the model's channels in order ('rg' -> [0, 1], 'b_rg' -> [2, 0, 1]), as the models parse --which_channel."""
    return ['rgb'.index(c) for c in which_channel.replace('_', '')]


def object_plane(x, objects, out=None):
    """[H, W] in [-1, 1] -> the plane ops.ccl_label labels: (x + 1) / 2, or 1 - that for `wall`; two exact fp32 steps on any device."""
    import torch
    out = torch.add(x, 1.0, out=out)
    out.mul_(0.5)
    if objects == 'wall':
        out.neg_().add_(1.0)
    return out


def summary_text(table, props, images, shape, sargs):
    interior = ~props['touches_border']
    per_image = np.bincount(table[:, 12], minlength=images) if images else np.zeros(0)
    lines = ['source %s, channel %d, objects %s, image size %d x %d' % ((sargs.shape_source, sargs.shape_channel, sargs.shape_objects) + tuple(shape)),
             'images: %d' % images,
             'regions: %d (%d do not touch the border)' % (len(table), int(interior.sum())),
             'regions per image: mean %.4f std %.4f' % ((per_image.mean(), per_image.std()) if images else (float('nan'),) * 2),
             'quantiles %s over the regions that do not touch the border:' % ' '.join('%g' % q for q in QUANTILES)]
    for name in ('area', 'eccentricity', 'compactness'):
        v = props[name][interior]
        q = np.quantile(v, QUANTILES) if len(v) else [float('nan')] * len(QUANTILES)
        lines.append('%s: %s' % (name, ' '.join('%.6g' % x for x in q)))
    return '\n'.join(lines) + '\n'


def main(argv=None):
    import torch
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import REGION_PROPS, region_props
    argv = sys.argv[1:] if argv is None else list(argv)
    sargs, rest = _shape_args(argv)
    opt = TestOptions().parse(rest, save=False)
    opt.nThreads, opt.batchSize, opt.serial_batches, opt.no_flip, opt.no_rotate = 1, 1, True, True, True
    if sargs.shape_source == 'fake' and opt.model != 'fcgan':
        print('shape_stats.py: --shape_source fake samples an fcgan generator (got --model %s); --shape_source real measures any dataset'
              % opt.model, file=sys.stderr)
        raise SystemExit(2)
    channels = selected_channels(opt.which_channel)
    if not 0 <= sargs.shape_channel < len(channels) or sargs.shape_capacity < 1:
        print('shape_stats.py: --shape_channel %d is not one of the %d channels of --which_channel %s, or --shape_capacity < 1'
              % (sargs.shape_channel, len(channels), opt.which_channel), file=sys.stderr)
        raise SystemExit(2)
    if not opt.gpu_ids:
        print('shape_stats.py: the measurement runs on the GPU (--gpu_ids 0)', file=sys.stderr)
        raise SystemExit(2)
    dev = torch.device('cuda', opt.gpu_ids[0])
    table = torch.zeros((sargs.shape_capacity, ops.REGION_COLS), dtype=torch.int64, device=dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)
    state = {}

    def measure(x):
        """x: [H, W] on the device.  Enqueues only."""
        if 'plane' not in state or state['plane'].shape != x.shape:
            assert 'plane' not in state, 'every image of a run has one size: %s after %s' % (tuple(x.shape), tuple(state['plane'].shape))
            state['plane'] = torch.empty(x.shape, dtype=torch.float32, device=dev)
            state['labels'] = torch.empty(x.shape, dtype=torch.int32, device=dev)
        ops.region_stats(ops.ccl_label(object_plane(x, sargs.shape_objects, out=state['plane']), state['labels']), table, cursor)

    if sargs.shape_source == 'fake':
        from supervised_gan_amd.models import create_model
        model = create_model(opt)
        for _ in range(opt.how_many):
            model.test()
            measure(model.fake.detach()[0, sargs.shape_channel])
    else:
        if opt.dataroot == 'synthetic':
            dataset = SyntheticDataset(opt, opt.how_many)
        else:
            from supervised_gan_amd.data import create_dataset
            dataset = create_dataset(opt)
        side = 'A' if opt.which_direction == 'A' else 'B'
        for i, data in enumerate(dataset):
            if i >= opt.how_many:
                break
            measure(data[side][0, channels[sargs.shape_channel]].to(dev, dtype=torch.float32, non_blocking=True))

    # the one read-back
    rows, images = (int(v) for v in cursor.cpu())
    ops.check_metric_err(dev)
    table = table[:rows].cpu().numpy()
    shape = tuple(state['plane'].shape) if state else (0, 0)
    props = region_props(table, shape)
    out_dir = os.path.join(opt.results_dir, opt.name, '%s_%s' % (opt.phase, opt.which_epoch))
    os.makedirs(out_dir, exist_ok=True)
    npz, txt = os.path.join(out_dir, 'shape_stats.npz'), os.path.join(out_dir, 'shape_stats.txt')
    options = {k: str(v) for k, v in sorted(list(vars(opt).items()) + list(vars(sargs).items()))}
    np.savez(npz, table=table, props=np.stack([props[n].astype(np.float64) for n in REGION_PROPS], axis=1).reshape(len(table), len(REGION_PROPS)),
             prop_names=np.array(REGION_PROPS), images=np.int64(images), shape=np.array(shape, dtype=np.int64),
             option_names=np.array(list(options)), option_values=np.array(list(options.values())))
    text = summary_text(table, props, images, shape, sargs)
    with open(txt, 'w') as f:
        f.write(text)
    print(text, end='')
    return npz, txt


if __name__ == '__main__':
    main()
