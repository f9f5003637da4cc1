#!/usr/bin/env python3
"""Training driver of the segmentation trainers (`--model segmentation`, `segmentation_cycle`) with the loop of the reference's
train_ss.py: like train.py, plus the running accuracies (`--which_metric RandScore VInfo meanIU`, and the thinned,
object-level and boundary scores of the README) accumulated after EVERY optimizer step,
a validation pass over `<dataroot>/val` after every epoch, and a `best` checkpoint kept by `--best_metric`.

    python train_ss.py --dataroot synthetic --name sgan_ss --model segmentation --which_direction AtoB --dataset_mode aligned \
        --fineSize 512 --valSize 512 --which_model_netG unet_256 --ngf 32 --which_model_netD n_layers --n_layers_D 3 --ndf 32 \
        --scale_factor 1 --lambda_D 1.0 --norm instance --no_dropout --no_lsgan --which_channel b_rg --weights 1 2 \
        --which_metric RandScore meanIU --best_metric RandScore --graph

The accuracies are accumulated by kernels queued behind the step (supervised_gan_amd/csrc/sgan_metrics.hip); the host reads them at
the print interval and after the validation pass only, and writes them to acc_log.txt beside loss_log.txt (the reference plots them
in visdom panes, which this path does not carry).

`--ema_decay D [--ema_warmup]` keeps an exponential moving average of the generator (one launch after every generator update, inside
the graphed step) and saves it as `<label>_net_G_ema.pth` beside every `<label>_net_G.pth`; with `--ema_eval` the validation pass, and
so `--best_metric` and the `best` checkpoint, score the average (SegmentationModel.forward(val_mode=True))."""
import copy
import math
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from supervised_gan_amd.models import create_model  # noqa: E402
from supervised_gan_amd.options import TrainOptions  # noqa: E402
from supervised_gan_amd.synthetic_data import SyntheticDataset  # noqa: E402
from supervised_gan_amd.util import save_image, tensor2im  # noqa: E402
from supervised_gan_amd.visualizer import Visualizer  # noqa: E402


LOWER_IS_BETTER = ('HausD', 'ASSD', 'Betti0Err', 'Betti1Err')      # distances in pixels and Betti errors: reported, never the --best_metric


def improves(value, best):
    """Strictly better than the best so far; a NaN score never is."""
    value = float(value)
    return not math.isnan(value) and value > best


def should_save_best(best_metric, accs, best):
    """The `best` checkpoint rule after a validation pass: --best_metric 'None' (compared by value: the option is a parsed string,
    not the literal) keeps no best checkpoint; otherwise the metric has to improve on the best so far."""
    return best_metric != 'None' and improves(accs[best_metric], best)


def validation_options(opt):
    """The second option set of train_ss.py:33-42: phase val, batch 1, in order, no flip, no rotation, loaded and cropped at valSize;
    no elastic deformation and no photometric variation either (--elastic and --photo_aug augment the training crops only)."""
    val = copy.copy(opt)
    val.phase, val.nThreads, val.batchSize, val.serial_batches, val.no_flip, val.no_rotate = 'val', 1, 1, True, True, True
    val.elastic = val.photo_aug = None
    val.valSize = val.valSize or val.loadSize
    val.loadSize = val.fineSize = val.valSize
    return val


def validate(model, dataset_val, img_dir=None):
    """One pass over the validation set: forward(val_mode=True) without gradients, accuracies accumulated from zero."""
    model.reset_accs()
    averaged = model.averaged_generator()      # --ema_eval: prepared once, the weights do not change during the pass
    kw = {} if averaged is None else {'netG': averaged}
    for data in dataset_val:
        model.set_input(data)
        with torch.no_grad():
            model.forward(val_mode=True, **kw)
        model.accum_accs()
        if img_dir is not None:
            name = os.path.splitext(os.path.basename(model.get_image_paths()[0]))[0]
            for label, v in model.get_current_visuals().items():
                if 'image' not in label:          # the raw image is on disk already
                    save_image(tensor2im(v), os.path.join(img_dir, '%s_%s.png' % (name, label)))
    return model.get_current_accs()


def main(argv=None):
    to = TrainOptions()
    to.initialize()
    to.parser.add_argument('--max_steps', type=int, default=0, help='stop after this many optimizer steps (0 = run all epochs); the '
                                                                    'validation pass and the checkpoints of the cut epoch still run')
    to.parser.add_argument('--epoch_size', type=int, default=64, help='synthetic images per epoch')
    to.parser.add_argument('--val_epoch_size', type=int, default=4, help='synthetic images per validation pass')
    to.parser.add_argument('--graph', action='store_true', help='replay the step as hipGraphs (graph_step.GraphedStep), see train.py')
    opt = to.parse(argv)
    opt_val = validation_options(opt)
    if opt.manualSeed is None:
        opt.manualSeed = random.randint(1, 10000)
    print("Random Seed: ", opt.manualSeed)
    random.seed(opt.manualSeed)
    np.random.seed(opt.manualSeed)
    torch.manual_seed(opt.manualSeed)
    if opt.dataroot == 'synthetic':
        dataset, dataset_val = SyntheticDataset(opt, opt.epoch_size), SyntheticDataset(opt_val, opt.val_epoch_size)
    else:
        from supervised_gan_amd.data import create_dataset
        dataset, dataset_val = create_dataset(opt), create_dataset(opt_val)
    dataset_size = len(dataset)
    print('#training images = %d' % dataset_size)
    print('#validation images = %d' % len(dataset_val))
    if opt.graph and opt_val.valSize != opt.fineSize:
        raise ValueError("--graph: the captured step owns the trainer's input buffers, so --valSize (%d) must equal --fineSize (%d)"
                         % (opt_val.valSize, opt.fineSize))
    if opt.best_metric in LOWER_IS_BETTER:
        raise ValueError("--best_metric %s: a distance or an error count, lower is better, and the `best` checkpoint is kept by the highest "
                         "value; choose a score among --which_metric (BoundF is the boundary score that rises, clDice the topology score)" % opt.best_metric)
    if opt.best_metric != 'None' and opt.best_metric not in opt.which_metric:
        raise ValueError("--best_metric %s is not among --which_metric %s" % (opt.best_metric, ' '.join(opt.which_metric)))
    model = create_model(opt)
    if not hasattr(model, 'accum_accs'):
        raise ValueError("train_ss.py drives the segmentation trainers; --model %s has no accuracies (use train.py)" % opt.model)
    visualizer = Visualizer(opt)
    graphed = None
    if opt.graph:
        from supervised_gan_amd.graph_step import GraphedStep
        graphed = GraphedStep(model)
    chkpt_dir = os.path.join(opt.checkpoints_dir, opt.name)
    total_steps, best, stop, validated = 0, -1.0, False, False
    for epoch in range(1, opt.niter + opt.niter_decay + 1):
        epoch_start_time = time.time()
        model.reset_accs()
        for data in dataset:
            iter_start_time = time.time()
            total_steps += opt.batchSize
            epoch_iter = total_steps - dataset_size * (epoch - 1)
            if graphed is None:
                model.set_input(data)
                model.optimize_parameters()
                model.accum_accs()              # kernels behind the step; nothing is read here
            elif not graphed.captured:
                graphed.capture(data)           # warm-up steps, then the recording: the captured tensors hold no step's result yet,
            else:                               # so this one iteration stays out of the running accuracies
                if validated:                   # the validation pass left the trainer's attributes naming its own tensors
                    graphed.reinstall()
                    validated = False
                graphed.step(data)
                model.accum_accs()
            if total_steps % opt.display_freq == 0:
                visualizer.display_current_results(model.get_current_visuals(), epoch)
            if total_steps % opt.print_freq == 0:
                visualizer.print_current_errors(epoch, epoch_iter, model.get_current_errors(), (time.time() - iter_start_time) / opt.batchSize)
                visualizer.print_current_accs(epoch, epoch_iter, model.get_current_accs(), 'train')
            if total_steps % opt.save_latest_freq == 0:
                print('saving the latest model (epoch %d, total_steps %d)' % (epoch, total_steps))
                model.save('latest')
            if opt.max_steps and total_steps >= opt.max_steps:
                stop = True
                break
        img_dir = os.path.join(chkpt_dir, 'val', 'epoch%03d' % epoch) if opt.save_val_visuals else None
        accs = validate(model, dataset_val, img_dir)
        validated = True
        visualizer.print_current_accs(epoch, 0, accs, 'val')
        if should_save_best(opt.best_metric, accs, best):
            best = float(accs[opt.best_metric])
            print('saving the best model (epoch %d, %s %.6f)' % (epoch, opt.best_metric, best))
            model.save('best')
        if stop or epoch % opt.save_epoch_freq == 0:
            print('saving the model at the end of epoch %d, iters %d' % (epoch, total_steps))
            model.save('latest')
            if not stop:
                model.save(epoch)
        if stop:
            break
        print('End of epoch %d / %d \t Time Taken: %d sec' % (epoch, opt.niter + opt.niter_decay, time.time() - epoch_start_time))
        if epoch > opt.niter:
            model.update_learning_rate()
    return model, best


if __name__ == '__main__':
    main()
