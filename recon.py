#!/usr/bin/env python3
"""Latent reconstruction driver with the reference's loop (recon.py): load `<which_epoch>_net_G.pth` of an fcgan run, fit latents to
`how_many` images by L-BFGS (FCGANModel.reconstruction: 3 trials x 50 step() calls, lr 0.1 by default), write the best reconstruction
and the image beside it as PNGs under results_dir/name/<phase>_<which_epoch>/images/ with an index.html, and print the summary line
`BCE: mean .. std ..; noise: mean .. std ..; noise init: mean .. std ..`.  `--use_ema` fits against the averaged generator
(`<which_epoch>_net_G_ema.pth` of a run with `--ema_decay`)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from supervised_gan_amd.options import TestOptions  # noqa: E402
from supervised_gan_amd.synthetic_data import SyntheticDataset  # noqa: E402
from supervised_gan_amd import html  # noqa: E402
from supervised_gan_amd.visualizer import Visualizer  # noqa: E402


def _recon_args(argv):
    """The reconstruction's own flags (defaults: the reference's constants), split off before TestOptions parses the rest."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument('--recon_trials', type=int, default=3)
    p.add_argument('--recon_steps', type=int, default=50, help='LBFGS step() calls per trial')
    p.add_argument('--recon_lr', type=float, default=0.1)
    p.add_argument('--recon_eager', action='store_true', help='launch every closure eagerly instead of replaying a captured graph')
    return p.parse_known_args(argv)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    rargs, rest = _recon_args(argv)
    opt = TestOptions().parse(rest, save=False)
    opt.nThreads, opt.batchSize, opt.serial_batches, opt.no_flip, opt.no_rotate = 1, 1, True, True, True
    if opt.model != 'fcgan':
        print('recon.py: only --model fcgan has a latent reconstruction (got --model %s)' % opt.model, file=sys.stderr)
        raise SystemExit(2)
    from supervised_gan_amd.models import create_model
    model = create_model(opt)
    visualizer = Visualizer(opt)
    web_dir = os.path.join(opt.results_dir, opt.name, '%s_%s' % (opt.phase, opt.which_epoch))
    webpage = html.HTML(web_dir, 'Experiment = %s, Phase = %s, Epoch = %s' % (opt.name, opt.phase, opt.which_epoch))
    if opt.dataroot == 'synthetic':
        dataset = SyntheticDataset(opt, opt.how_many)
    else:
        from supervised_gan_amd.data import create_dataset
        dataset = create_dataset(opt)

    l2_dist, ll_noise, ll_noise_init, written = [], [], [], []
    for i, data in enumerate(dataset):
        if i >= opt.how_many:
            break
        model.set_input(data)
        print('reconstruct image {}...'.format(i))
        e, ll, ll0 = model.reconstruction(num_trials=rargs.recon_trials, n_steps=rargs.recon_steps, lr=rargs.recon_lr,
                                          graph=not rargs.recon_eager)
        l2_dist.append(e)
        ll_noise.append(ll)
        ll_noise_init.append(ll0)
        stem = os.path.splitext(os.path.basename(model.get_image_paths()[0]))[0]
        written.extend(visualizer.save_images(webpage, model.get_current_visuals(True), [stem + '.png']))
    webpage.save()

    l2_dist, ll_noise, ll_noise_init = (np.array(v).squeeze() for v in (l2_dist, ll_noise, ll_noise_init))
    print('BCE: mean {0:0.4f} std {1:0.4f}; noise: mean {2:0.4f} std {3:0.4f}; noise init: mean {4:0.4f} std {5:0.4f}'.format(
        np.mean(l2_dist), np.std(l2_dist), np.mean(ll_noise), np.std(ll_noise), np.mean(ll_noise_init), np.std(ll_noise_init)))
    return written, (l2_dist, ll_noise, ll_noise_init)


if __name__ == '__main__':
    main()
