#!/usr/bin/env python3
"""Evaluation driver of the segmentation trainers with the loop of the reference's test_ss.py: load `<which_epoch>_net_*.pth`, run
every image of the dataset (at most --how_many) through `model.test()`, take its cross-entropy, accumulate the accuracies of
`--which_metric` on the device, write the visuals to the result page, and print the metrics and the mean / std of the loss."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from supervised_gan_amd.models import create_model  # noqa: E402
from supervised_gan_amd.options import TestOptions  # noqa: E402
from supervised_gan_amd.synthetic_data import SyntheticDataset  # noqa: E402
from supervised_gan_amd import html  # noqa: E402
from supervised_gan_amd.visualizer import Visualizer  # noqa: E402


def main(argv=None):
    opt = TestOptions().parse(argv, save=False)
    opt.nThreads, opt.batchSize, opt.serial_batches, opt.no_flip, opt.no_rotate = 1, 1, True, True, True
    if opt.dataroot == 'synthetic':
        dataset = SyntheticDataset(opt, opt.how_many)
    else:
        from supervised_gan_amd.data import create_dataset
        dataset = create_dataset(opt)
    print('#testing images = %d' % len(dataset))
    model = create_model(opt)
    if not hasattr(model, 'accum_accs'):
        raise ValueError("test_ss.py drives the segmentation trainers; --model %s has no accuracies (use test.py)" % opt.model)
    visualizer = Visualizer(opt)
    web_dir = os.path.join(opt.results_dir, opt.name, '%s_%s' % (opt.phase, opt.which_epoch))
    webpage = html.HTML(web_dir, 'Experiment = %s, Phase = %s, Epoch = %s' % (opt.name, opt.phase, opt.which_epoch))
    model.reset_accs()
    ce_loss = []
    for i, data in enumerate(dataset):
        if i >= opt.how_many:
            break
        model.set_input(data)
        model.test()
        ce_loss.append(model.compute_cross_entropy_loss().detach())
        model.accum_accs()
        print('process image... %s' % model.get_image_paths())
        visualizer.save_images(webpage, model.get_current_visuals(), model.get_image_paths())
    accs = model.get_current_accs()
    ce_loss = np.array([float(v) for v in ce_loss])
    print('Segmentation results:')
    for key, value in accs.items():
        print('%s: %s' % (key, value))
    print('cross entropy loss: mean %s, std %s' % (np.mean(ce_loss), np.std(ce_loss)))
    webpage.save()
    return accs, ce_loss


if __name__ == '__main__':
    main()
