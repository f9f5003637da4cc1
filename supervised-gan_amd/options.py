"""Option surface of the reference (options/base_options.py:11-144, options/train_options.py:4-66,
options/test_options.py) for the trainers on the MI355X path: same flag names, types, defaults and
`nargs='+'` list flags, same `parse()` protocol (gpu_ids string -> list, opt.txt dump).  Flags that only
steer out-of-scope subsystems (visdom, dataset folders) are accepted and ignored."""
import argparse
import math
import os

import torch


class BaseOptions:
    def __init__(self):
        self.parser = argparse.ArgumentParser()
        self.initialized = False
        self.isTrain = False

    def initialize(self):
        a = self.parser.add_argument
        a('--dataroot', default='synthetic', help='path to images, or "synthetic" (MI355X bench feeder)')
        a('--batchSize', type=int, default=1)
        a('--loadSize', type=int, default=286)
        a('--fineSize', type=int, default=256)
        a('--patchSize', type=int, default=70)
        a('--input_nc', type=int, default=3)
        a('--noise_nc', type=int, default=8)
        a('--noiseSize', type=int, default=1)
        a('--noiseSizeVal', type=int, default=1)
        a('--output_nc', type=int, default=3)
        a('--ngf', type=int, default=64)
        a('--ndf', type=int, default=64)
        a('--which_model_netD', type=str, default='basic')
        a('--which_model_netG', type=str, default='resnet_9blocks')
        a('--n_layers_D', type=int, default=[3], nargs='+')
        a('--n_layers_G', type=int, default=5)
        a('--scale_factor', type=int, default=[1], nargs='+')
        a('--gpu_ids', type=str, default='0')
        a('--name', type=str, default='experiment_name')
        a('--dataset_mode', type=str, default='unaligned')
        a('--model', type=str, default='cycle_gan')
        a('--which_direction', type=str, default='AtoB')
        a('--nThreads', default=2, type=int)
        a('--checkpoints_dir', type=str, default='./checkpoints')
        a('--norm', type=str, default='instance')
        a('--serial_batches', action='store_true')
        a('--display_winsize', type=int, default=256)
        a('--display_id', type=int, default=1)
        a('--display_port', type=int, default=8097)
        a('--display_single_pane_ncols', type=int, default=0)
        a('--identity', type=float, default=0.0)
        a('--no_dropout', action='store_true')
        a('--max_dataset_size', type=int, default=float("inf"))
        a('--resize_or_crop', type=str, default='resize_and_crop')
        a('--no_flip', action='store_true')
        a('--no_rotate', action='store_true')
        a('--use_residual', action='store_true')
        a('--add_gaussian_noise', action='store_true')
        a('--gaussian_sigma', type=float, default=0.1)
        a('--which_channel', type=str, default='rg')
        a('--manualSeed', type=int, default=None)
        a('--display_title', type=str, default='loss over time')
        a('--n_layers_G_skip', type=int, default=-1)
        a('--weights', type=float, default=None, nargs='+')
        a('--use_sigmoid_ss', action='store_true')            # segmentation: sigmoid instead of softmax (base_options.py:55)
        a('--which_metric', default=['None'], nargs='+')      # any of RandScore, VInfo, meanIU, RandScoreThin, VInfoThin, ObjF1, ObjAP, SEG, PQ, BoundF, HausD, ASSD, Betti0Err, Betti1Err, clDice (device accumulators, seg_metrics.py)
        a('--min_object_area', type=int, default=1)           # ObjF1 / ObjAP / SEG / PQ: regions with fewer pixels count as absent, on both sides
        a('--clean_close', type=float, default=0.0)           # clean the predicted wall before the label-based scores: close gaps with a disk of this radius, close_rsq = floor(R * R); 1 = the 4-neighbour plus, 1.5 = the 3 x 3 box; at most 64
        a('--clean_min_wall', type=int, default=0)            # ... then drop 8-connected wall components with fewer pixels than this
        a('--clean_min_cell', type=int, default=0)            # ... then fill 8-connected regions with fewer pixels than this (seg_metrics.py; all three off: the raw thresholded map)
        a('--clean_split', type=float, default=0.0)           # ... and, between the specks and the small cells, cut merged cells apart: cores where the distance to the wall is >= this radius, split_rsq = floor(R * R), flooded back, a wall where two meet; 0 = off, at most 64
        a('--clean_split_rounds', type=int, default=64)       # ... flood rounds of --clean_split (one per pixel of distance from a core): 1 .. 4096
        a('--boundary_tolerance', type=int, default=2, choices=range(31), metavar='0..30')      # BoundF: a wall pixel within this many pixels of the other map's wall is matched
        a('--boundary_thin', action='store_true')             # BoundF / HausD / ASSD: thin the predicted wall to one-pixel lines first, as BSDS does; the truth is not thinned
        a('--topo_window', type=int, default=64)              # Betti0Err / Betti1Err: the side of the windows the Betti numbers are taken in, 8 .. 64 (clamped to the image); a strip no full window covers is not scored
        a('--topo_stride', type=int, default=None)            # ... and the step between window origins, 1 .. --topo_window; default: the window, no overlap
        a('--add_background_onehot', action='store_true')
        a('--add_background_onehot_acc', action='store_true')
        a('--valSize', type=int, default=0)                   # train_ss.py: size of the validation images, 0 = loadSize (base_options.py:102)
        a('--save_val_visuals', action='store_true')          # train_ss.py: write val/epochNNN/<name>_<label>.png
        a('--best_metric', type=str, default='None')          # train_ss.py: keep a `best` checkpoint by this validation metric
        a('--upsample_mode', type=str, default='convt')
        a('--no_share_label_block_weights', action='store_true')
        a('--n_layers_CRN_block', type=int, default=1)
        a('--pretrained_model_dir', type=str, default='')
        a('--transform_1to2', type=str, default='None')
        # two-stage models (options/base_options.py:62-99)
        a('--scale_factor1', type=int, default=[1], nargs='+')
        a('--scale_factor2', type=int, default=[1], nargs='+')
        a('--which_model_netD1', type=str, default='n_layers')
        a('--which_model_netG1', type=str, default='fcgan')
        a('--which_model_netF1', type=str, default='fcgan')
        a('--ngf1', type=int, default=64)
        a('--ndf1', type=int, default=64)
        a('--nff1', type=int, default=64)
        a('--n_layers_D1', type=int, default=[3], nargs='+')
        a('--n_layers_G1', type=int, default=5)
        a('--n_layers_F1', type=int, default=5)
        a('--no_dropout1', action='store_true')
        a('--noise_nc1', type=int, default=256)
        a('--noiseSize1', type=int, default=1)
        a('--which_model_netD2', type=str, default='n_layers')
        a('--which_model_netG2', type=str, default='unet_128')
        a('--which_model_netF2', type=str, default='unet_128')
        a('--ngf2', type=int, default=64)
        a('--ndf2', type=int, default=64)
        a('--nff2', type=int, default=64)
        a('--n_layers_D2', type=int, default=[3], nargs='+')
        a('--n_layers_G2', type=int, default=5)
        a('--n_layers_F2', type=int, default=5)
        a('--no_dropout2', action='store_true')
        a('--noise_nc2', type=int, default=256)
        a('--noiseSize2', type=int, default=1)
        a('--use_residual1', action='store_true')
        a('--use_residual2', action='store_true')
        a('--upsample_mode1', type=str, default='convt')
        a('--no_share_label_block_weights1', action='store_true')
        a('--n_layers_CRN_block1', type=int, default=1)
        a('--upsample_mode2', type=str, default='convt')
        a('--no_share_label_block_weights2', action='store_true')
        a('--n_layers_CRN_block2', type=int, default=1)
        a('--n_layers_G1_skip', type=int, default=-1)
        a('--n_layers_G2_skip', type=int, default=-1)
        # MI355X path extras (not in the reference)
        a('--skip_wasted_D_wgrad', action='store_true',
          help='do not compute discriminator weight gradients during the G step (the reference computes and discards them)')
        a('--hip_graph', action='store_true', help='capture the training step into hipGraphs')
        a('--no_group', action='store_true', help='launch every discriminator chain on its own instead of grouped kernels')
        a('--no_d_streams', action='store_true', help='run the discriminator chains on one stream instead of one each')
        a('--math', type=str, default=None, choices=['f32', 'bf16x3', 'bf16x1'],
          help='arithmetic of the conv kernels: f32 (exact fp32 MFMA), bf16x3 (split 16-bit planes, fp32-equivalent) or bf16x1 '
               '(one 16-bit plane: faster, ~bf16 products, fp32 storage and accumulation).  Unset: SGAN_MATH, else bf16x3.  '
               'Set when the options are parsed, before the model is built; a captured step (--hip_graph) replays the mode '
               'that was current when it was captured')
        self.initialized = True

    def parse(self, args=None, save=True, verbose=True):
        if not self.initialized:
            self.initialize()
        self.opt = self.parser.parse_args(args)
        self.opt.isTrain = self.isTrain
        check_border_options(self.opt)
        check_cldice_options(self.opt)
        check_lovasz_options(self.opt)
        check_dice_options(self.opt)
        check_focal_options(self.opt)
        check_dist_options(self.opt)
        check_clean_options(self.opt, self.parser)
        check_topo_options(self.opt, self.parser)
        check_elastic_options(self.opt)
        check_photo_options(self.opt)
        check_tile_options(self.opt, self.parser)
        check_ema_options(self.opt, self.parser)
        check_diffaug_options(self.opt, self.parser)
        if self.opt.math is not None:
            from . import ops
            ops.set_math(self.opt.math)
        str_ids = self.opt.gpu_ids.split(',')
        self.opt.gpu_ids = [int(s) for s in str_ids if int(s) >= 0]
        if len(self.opt.gpu_ids) > 0 and torch.cuda.is_available():
            torch.cuda.set_device(self.opt.gpu_ids[0])
        args_ = vars(self.opt)
        if verbose:
            print('------------ Options -------------')
            for k, v in sorted(args_.items()):
                print('%s: %s' % (str(k), str(v)))
            print('-------------- End ----------------')
        if save:
            expr_dir = os.path.join(self.opt.checkpoints_dir, self.opt.name)
            os.makedirs(expr_dir, exist_ok=True)
            with open(os.path.join(expr_dir, 'opt.txt'), 'wt') as f:
                f.write('------------ Options -------------\n')
                for k, v in sorted(args_.items()):
                    f.write('%s: %s\n' % (str(k), str(v)))
                f.write('-------------- End ----------------\n')
        return self.opt


def check_border_options(opt):
    """--border_weight goes with the softmax cross-entropy of the discriminator-free segmentation trainer only; fills in the default
    radius min(32, ceil(4 SIGMA)), beyond which the term is below W0 e^-8."""
    if getattr(opt, 'border_weight', None) is None:
        return
    w0, sigma = opt.border_weight
    assert sigma > 0, "--border_weight W0 SIGMA: SIGMA must be positive (got %g)" % sigma
    assert opt.which_model_netD == 'None', \
        "--border_weight weights the cross-entropy of the supervised baseline: it needs --which_model_netD None (got '%s')" % opt.which_model_netD
    assert not opt.use_sigmoid_ss, "--border_weight weights the softmax cross-entropy: it cannot be combined with --use_sigmoid_ss"
    if opt.border_radius is None:
        opt.border_radius = min(32, int(math.ceil(4 * sigma)))
    assert 1 <= opt.border_radius <= 32, "--border_radius: 1..32 (got %d)" % opt.border_radius
    assert opt.border_class >= 0, "--border_class: a class index (got %d)" % opt.border_class


def check_cldice_options(opt):
    """--cldice_weight LAMBDA adds the soft-clDice term to the generator loss of --model segmentation (any head, with or without
    discriminators); LAMBDA >= 0 with 0 = off, --cldice_iters 1..16, --cldice_class a class index.  Another model refuses it.  With
    the weight at 0 nothing is looked at and nothing is changed."""
    weight = getattr(opt, 'cldice_weight', 0.0)
    if weight == 0.0:
        return
    assert weight > 0.0, "--cldice_weight LAMBDA: a weight >= 0, 0 = off (got %g)" % weight      # a NaN fails the comparison
    assert getattr(opt, 'model', None) == 'segmentation', \
        "--cldice_weight adds the soft-clDice term to the segmentation trainer's generator loss: it needs --model segmentation (got '%s')" % \
        getattr(opt, 'model', None)
    assert 1 <= opt.cldice_iters <= 16, "--cldice_iters: 1..16 (got %d)" % opt.cldice_iters
    assert opt.cldice_class >= 0, "--cldice_class: a class index (got %d)" % opt.cldice_class


def check_lovasz_options(opt):
    """--lovasz_weight LAMBDA adds the Lovasz-softmax term over --lovasz_classes to the generator loss of --model segmentation (any
    head, with or without discriminators); LAMBDA >= 0 with 0 = off, 1..8 distinct class indices.  Another model refuses it.  With
    the weight at 0 nothing is looked at and nothing is changed."""
    weight = getattr(opt, 'lovasz_weight', 0.0)
    if weight == 0.0:
        return
    assert weight > 0.0, "--lovasz_weight LAMBDA: a weight >= 0, 0 = off (got %g)" % weight      # a NaN fails the comparison
    assert getattr(opt, 'model', None) == 'segmentation', \
        "--lovasz_weight adds the Lovasz-softmax term to the segmentation trainer's generator loss: it needs --model segmentation (got '%s')" % \
        getattr(opt, 'model', None)
    classes = list(opt.lovasz_classes)
    assert 1 <= len(classes) <= 8, "--lovasz_classes: 1..8 classes (got %d)" % len(classes)
    assert all(c >= 0 for c in classes), "--lovasz_classes: class indices (got %s)" % classes
    assert len(set(classes)) == len(classes), "--lovasz_classes: distinct classes (got %s)" % classes


def check_dice_options(opt):
    """--dice_weight LAMBDA adds the Tversky term over --dice_classes to the generator loss of --model segmentation (any head, with
    or without discriminators): soft Dice at the default --tversky 0.5 0.5, focal-Tversky at --tversky_power below 1.  LAMBDA >= 0
    with 0 = off, 1..8 distinct class indices, A, B >= 0 with A + B > 0, S >= 0, 0 < E <= 4.  Another model refuses it.  With the
    weight at 0 nothing is looked at and nothing is changed."""
    weight = getattr(opt, 'dice_weight', 0.0)
    if weight == 0.0:
        return
    assert weight > 0.0, "--dice_weight LAMBDA: a weight >= 0, 0 = off (got %g)" % weight      # a NaN fails the comparison
    assert getattr(opt, 'model', None) == 'segmentation', \
        "--dice_weight adds the Dice / Tversky term to the segmentation trainer's generator loss: it needs --model segmentation (got '%s')" % \
        getattr(opt, 'model', None)
    classes = list(opt.dice_classes)
    assert 1 <= len(classes) <= 8, "--dice_classes: 1..8 classes (got %d)" % len(classes)
    assert all(c >= 0 for c in classes), "--dice_classes: class indices (got %s)" % classes
    assert len(set(classes)) == len(classes), "--dice_classes: distinct classes (got %s)" % classes
    a, b = opt.tversky
    assert a >= 0.0 and b >= 0.0, "--tversky A B: both >= 0 (got %g %g)" % (a, b)      # a NaN fails the comparison
    assert a + b > 0.0, "--tversky A B: A + B == 0 leaves no penalty on any error (got %g %g)" % (a, b)
    assert a < float('inf') and b < float('inf'), "--tversky A B: finite (got %g %g)" % (a, b)
    assert 0.0 <= opt.dice_smooth < float('inf'), "--dice_smooth S: S >= 0 (got %g)" % opt.dice_smooth
    assert 0.0 < opt.tversky_power <= 4.0, "--tversky_power E: 0 < E <= 4 (got %g)" % opt.tversky_power


def check_focal_options(opt):
    """--focal_weight LAMBDA adds the focal loss (Lin et al., ICCV 2017) with --focal_gamma G and the class weights of --weights to
    the generator loss of --model segmentation (any head, with or without discriminators); LAMBDA >= 0 with 0 = off, 0 <= G <= 8.
    Another model refuses it.  With the weight at 0 nothing is looked at and nothing is changed."""
    weight = getattr(opt, 'focal_weight', 0.0)
    if weight == 0.0:
        return
    assert weight > 0.0, "--focal_weight LAMBDA: a weight >= 0, 0 = off (got %g)" % weight      # a NaN fails the comparison
    assert getattr(opt, 'model', None) == 'segmentation', \
        "--focal_weight adds the focal loss to the segmentation trainer's generator loss: it needs --model segmentation (got '%s')" % \
        getattr(opt, 'model', None)
    assert 0.0 <= opt.focal_gamma <= 8.0, "--focal_gamma G: 0 <= G <= 8 (got %g)" % opt.focal_gamma


def check_dist_options(opt):
    """--boundary_loss_weight LAMBDA adds the boundary loss (Kervadec et al., MIDL 2019) and --hausdorff_weight LAMBDA the
    distance-transform Hausdorff loss (Karimi & Salcudean, TMI 2019) with exponent --hausdorff_alpha A of the --dist_class channel to
    the generator loss of --model segmentation (any head, with or without discriminators); LAMBDA >= 0 with 0 = off, 0 < A <= 4, a
    class index.  Another model refuses them.  With both weights at 0 nothing is looked at and nothing is changed."""
    wb, wh = getattr(opt, 'boundary_loss_weight', 0.0), getattr(opt, 'hausdorff_weight', 0.0)
    if wb == 0.0 and wh == 0.0:
        return
    assert wb >= 0.0, "--boundary_loss_weight LAMBDA: a weight >= 0, 0 = off (got %g)" % wb      # a NaN fails the comparison
    assert wh >= 0.0, "--hausdorff_weight LAMBDA: a weight >= 0, 0 = off (got %g)" % wh
    assert getattr(opt, 'model', None) == 'segmentation', \
        "--boundary_loss_weight / --hausdorff_weight add distance-map terms to the segmentation trainer's generator loss: they need " \
        "--model segmentation (got '%s')" % getattr(opt, 'model', None)
    if wh > 0.0:
        assert 0.0 < opt.hausdorff_alpha <= 4.0, "--hausdorff_alpha A: 0 < A <= 4 (got %g)" % opt.hausdorff_alpha
    assert opt.dist_class >= 0, "--dist_class: a class index (got %d)" % opt.dist_class


def check_clean_options(opt, parser=None):
    """--clean_close R, --clean_min_wall N, --clean_min_cell N: none negative, R at most 64 (close_rsq = floor(R R) <= 4096, the
    library's limit); --clean_split R: 0 or 1 .. 64, --clean_split_rounds N: 1 .. 4096; refused at parse time."""
    bad = None
    if not 0.0 <= opt.clean_close <= 64.0:      # a NaN fails both comparisons
        bad = "--clean_close: a radius of 0 .. 64 pixels (got %g)" % opt.clean_close
    elif opt.clean_min_wall < 0 or opt.clean_min_cell < 0:
        bad = "--clean_min_wall / --clean_min_cell: a pixel count, not negative (got %d / %d)" % (opt.clean_min_wall, opt.clean_min_cell)
    elif not 0.0 <= getattr(opt, 'clean_split', 0.0) <= 64.0:
        bad = "--clean_split: a radius of 0 .. 64 pixels (got %g)" % opt.clean_split
    elif 0.0 < getattr(opt, 'clean_split', 0.0) < 1.0:
        bad = "--clean_split: a radius below 1 has no core (split_rsq = floor(R R) = 0); 0 = off (got %g)" % opt.clean_split
    elif not 1 <= getattr(opt, 'clean_split_rounds', 64) <= 4096:
        bad = "--clean_split_rounds: 1 .. 4096 (got %d)" % opt.clean_split_rounds
    if bad is not None:
        if parser is not None:
            parser.error(bad)
        raise ValueError(bad)


def check_topo_options(opt, parser=None):
    """--topo_window N: 8 .. 64 (a window is labelled in one workgroup's LDS); --topo_stride S: 1 .. N, default N; refused at parse
    time.  Leaves opt.topo_stride filled in."""
    window, stride = topo_params(opt)
    bad = None
    if not 8 <= window <= 64:
        bad = "--topo_window: 8 .. 64 (got %d)" % window
    elif not 1 <= stride <= window:
        bad = "--topo_stride: 1 .. --topo_window = %d (got %d)" % (window, stride)
    if bad is not None:
        if parser is not None:
            parser.error(bad)
        raise ValueError(bad)
    opt.topo_stride = stride


def topo_params(opt):
    """(window, stride) of ops.topo_accumulate from --topo_window / --topo_stride; (64, 64) for an options object without them."""
    window = int(getattr(opt, 'topo_window', 64))
    stride = getattr(opt, 'topo_stride', None)
    return window, window if stride is None else int(stride)


def split_params(opt):
    """(split_rsq, max_rounds) of ops.split_cells from --clean_split / --clean_split_rounds; split_rsq 0 = off, also for an options
    object without them."""
    r = float(getattr(opt, 'clean_split', 0.0))
    return int(math.floor(r * r)), int(getattr(opt, 'clean_split_rounds', 64))


def clean_params(opt):
    """(close_rsq, min_wall, min_cell) of ops.clean_wall from the --clean_* options; (0, 0, 0) for an options object without them."""
    r = float(getattr(opt, 'clean_close', 0.0))
    return int(math.floor(r * r)), int(getattr(opt, 'clean_min_wall', 0)), int(getattr(opt, 'clean_min_cell', 0))


def check_tile_options(opt, parser=None, size=None):
    """--whole_image / --tile T / --tile_margin M / --tile_ramp R / --tile_stride S / --tta (test options): whole-image inference by
    overlapping tiles, averaged over the 8 flips and rotations under --tta d4 (util.tile_plan).  Fills in the defaults
    (T = --fineSize, S = max(1, T - 2 M - R)) and leaves opt.tiling = is any of it on.  --tta d4 without --whole_image runs the feeder's
    T x T crop as one tile: M = 0, R = 1, S = T.  Refuses what the geometry cannot cover, at parse time as far as the image is not
    involved and, with `size` = (H, W), for an image (the feeder asks per file).  An options object without the flags (the training
    drivers) has no tiling."""
    from .util import tile_geometry_error
    if not hasattr(opt, 'whole_image'):
        opt.tiling = False
        return
    opt.tiling = bool(opt.whole_image or opt.tta == 'd4')
    bad = None
    if opt.tiling:
        if opt.whole_image:
            if opt.tile is None:
                opt.tile = opt.fineSize
            if opt.tile_stride is None:
                opt.tile_stride = max(1, opt.tile - 2 * opt.tile_margin - opt.tile_ramp)
        else:
            opt.tile, opt.tile_margin, opt.tile_ramp, opt.tile_stride = opt.fineSize, 0, 1, opt.fineSize
        T, M, R, S = opt.tile, opt.tile_margin, opt.tile_ramp, opt.tile_stride
        if opt.dataroot == 'synthetic':
            bad = "--whole_image / --tta d4 cut their tiles from the decoded uint8 image of an image folder; the synthetic feeder has none"
        elif opt.dataset_mode != 'single':
            bad = "--whole_image / --tta d4 read the single-image feeder (--dataset_mode single), got '%s'" % opt.dataset_mode
        elif opt.model != 'segmentation':
            bad = ("--whole_image / --tta d4 are built into SegmentationModel.test() (--model segmentation); the test() of --model %s "
                   "runs another forward" % opt.model)
        else:
            bad = tile_geometry_error(None, T, M, R, S)
            if bad is None and size is not None:
                bad = tile_geometry_error(size[0], T, M, R, S, 'height') or tile_geometry_error(size[1], T, M, R, S, 'width')
    if bad is not None:
        if parser is not None:
            parser.error(bad)
        raise ValueError(bad)


def check_ema_options(opt, parser=None):
    """--ema_decay D (train options): 0 <= D <= 1, unset = no average; --ema_warmup and --ema_eval need it.  Refused at parse time.
    An options object without the flags (the test drivers, which have --use_ema) passes."""
    decay = getattr(opt, 'ema_decay', None)
    bad = None
    if decay is not None and not 0.0 <= decay <= 1.0:      # a NaN fails both comparisons
        bad = "--ema_decay: a decay of 0 .. 1 (got %g)" % decay
    elif decay is None and (getattr(opt, 'ema_eval', False) or getattr(opt, 'ema_warmup', False)):
        bad = "--ema_eval / --ema_warmup need --ema_decay: without it there is no averaged generator"
    if bad is not None:
        if parser is not None:
            parser.error(bad)
        raise ValueError(bad)


def check_diffaug_options(opt, parser=None):
    """--diffaug POLICY (train options; diffaug.check_options): known operations, a supported --model with discriminators, ratios of
    0 .. 1 and, for a colour operation, a colour channel in the discriminator input.  Refused at parse time; leaves opt.diffaug_policy."""
    from .diffaug import check_options
    try:
        check_options(opt)
    except ValueError as e:
        if parser is not None:
            parser.error(str(e))
        raise


def check_elastic_options(opt):
    """--elastic G SIGMA deforms the crops of the image-folder feeders (data.py): G cells a side, 1..13 (the device stages the (G + 3)^2
    control vectors, at most 256); SIGMA >= 0 source pixels.  Leaves opt.elastic as (int G, float SIGMA)."""
    if getattr(opt, 'elastic', None) is None:
        return
    g, sigma = opt.elastic
    assert float(g) == int(g) and 1 <= int(g) <= 13, "--elastic G SIGMA: G is a whole number of cells a side, 1..13 (got %g)" % g
    assert sigma >= 0, "--elastic G SIGMA: SIGMA must not be negative (got %g)" % sigma
    assert opt.dataroot != 'synthetic', \
        "--elastic deforms the decoded uint8 image of the image-folder feeders; the synthetic feeder has none (give --dataroot a folder)"
    assert set(opt.elastic_label_channels) <= set('rgb'), \
        "--elastic_label_channels: letters of r, g, b (got '%s')" % opt.elastic_label_channels
    opt.elastic = (int(g), float(sigma))


def elastic_nearest_mask(opt):
    """The nearest_mask of ops.image_prep_elastic for --elastic_label_channels: bit c set = channel c of RGB holds labels."""
    return sum(1 << 'rgb'.index(ch) for ch in set(opt.elastic_label_channels))


def check_photo_options(opt):
    """--photo_aug LIST varies the grey values of the crops of the image-folder feeders (data.py, util.photo_draw): a comma list of
    blur, gamma, contrast, brightness, noise, occlude.  Refuses unknown or repeated stage names and out-of-range parameters, and a
    --photo_blur whose largest radius min(12, ceil(3 SMAX)) the --fineSize cannot hold.  Leaves opt.photo_aug as a tuple of stage
    names in the order they are drawn and applied in, and opt.photo_occlude as (int K, float FRAC)."""
    if getattr(opt, 'photo_aug', None) is None:
        return
    import math
    from .util import PHOTO_MAX_BOX, PHOTO_MAX_R, PHOTO_STAGES
    names = [s.strip() for s in opt.photo_aug.split(',')] if isinstance(opt.photo_aug, str) else list(opt.photo_aug)
    assert names and all(s in PHOTO_STAGES for s in names) and len(set(names)) == len(names), \
        "--photo_aug: a comma list of %s, each at most once (got '%s')" % (', '.join(PHOTO_STAGES), opt.photo_aug)
    assert opt.dataroot != 'synthetic', \
        "--photo_aug varies the crops of the image-folder feeders; the synthetic feeder has none (give --dataroot a folder)"
    finite = all(math.isfinite(float(v)) for v in (opt.photo_prob, opt.photo_blur, opt.photo_gamma, opt.photo_contrast, opt.photo_brightness,
                                                   opt.photo_noise, *opt.photo_occlude))
    assert finite, "--photo_*: every value must be finite"
    assert 0.0 <= opt.photo_prob <= 1.0, "--photo_prob: a probability (got %g)" % opt.photo_prob
    assert 0.5 <= opt.photo_blur <= 4.0, "--photo_blur SMAX: sigma ~ U(0.5, SMAX), 0.5 <= SMAX <= 4 (got %g)" % opt.photo_blur
    assert 1.0 <= opt.photo_gamma <= 2.0, "--photo_gamma G: gamma = exp(U(-ln G, ln G)), 1 <= G <= 2 (got %g)" % opt.photo_gamma
    assert 0.0 <= opt.photo_contrast < 1.0, "--photo_contrast C: c ~ U(1 - C, 1 + C), 0 <= C < 1 (got %g)" % opt.photo_contrast
    assert opt.photo_brightness >= 0.0, "--photo_brightness B must not be negative (got %g)" % opt.photo_brightness
    assert opt.photo_noise >= 0.0, "--photo_noise S must not be negative (got %g)" % opt.photo_noise
    k, frac = opt.photo_occlude
    assert float(k) == int(k) and 1 <= int(k) <= PHOTO_MAX_BOX and 0.0 < frac <= 1.0, \
        "--photo_occlude K FRAC: K boxes, a whole number 1..%d, of sides up to FRAC of the crop, 0 < FRAC <= 1 (got %g %g)" % (PHOTO_MAX_BOX, k, frac)
    assert opt.photo_channels and set(opt.photo_channels) <= set('rgb') and len(set(opt.photo_channels)) == len(opt.photo_channels), \
        "--photo_channels: letters of r, g, b (got '%s')" % opt.photo_channels
    assert not set(opt.photo_channels) & set(opt.elastic_label_channels), \
        "--photo_channels '%s' and --elastic_label_channels '%s' share a channel: a label channel takes no grey value variation" % (
            opt.photo_channels, opt.elastic_label_channels)
    if 'blur' in names:
        r = min(PHOTO_MAX_R, int(math.ceil(3.0 * opt.photo_blur)))
        assert r <= opt.fineSize - 1, \
            "--photo_blur %g reaches %d pixels, more than a --fineSize %d crop can mirror (at most fineSize - 1)" % (opt.photo_blur, r, opt.fineSize)
    opt.photo_aug = tuple(s for s in PHOTO_STAGES if s in names)
    opt.photo_occlude = (int(k), float(frac))


def photo_channel_mask(opt):
    """The channel mask of ops.image_photo for --photo_channels: bit c set = channel c of RGB holds the image."""
    return sum(1 << 'rgb'.index(ch) for ch in set(opt.photo_channels))


class TrainOptions(BaseOptions):
    def initialize(self):
        BaseOptions.initialize(self)
        a = self.parser.add_argument
        a('--display_freq', type=int, default=100)
        a('--print_freq', type=int, default=100)
        a('--save_latest_freq', type=int, default=5000)
        a('--save_epoch_freq', type=int, default=5)
        a('--continue_train', action='store_true')
        a('--phase', type=str, default='train')
        a('--which_epoch', type=str, default='latest')
        a('--niter', type=int, default=100)
        a('--niter_decay', type=int, default=100)
        a('--beta1', type=float, default=0.5)
        a('--lr', type=float, default=0.0002)
        a('--no_lsgan', action='store_true')
        a('--lambda_A', type=float, default=10.0)
        a('--lambda_B', type=float, default=10.0)
        a('--n_update_G', type=int, default=1)
        a('--n_update_D', type=int, default=1)
        a('--lambda_D', type=float, default=[1.0], nargs='+')
        a('--pool_size', type=int, default=50)
        a('--no_html', action='store_true')
        a('--no_cgan', action='store_true')
        a('--noise_pool_size', type=int, default=100)
        a('--optimizer', type=str, default='adam')
        a('--pool_reject_prob', type=float, default=0.5)
        a('--train_D_on_fake_fake_pair', action='store_true')   # cgan2 (options/train_options.py:33-34)
        a('--train_G_on_fake_fake_pair', action='store_true')
        a('--no_logD_trick', action='store_true')
        a('--lambda_fake_cycle', type=float, default=1.0)
        a('--which_model_to_load', nargs='+', default=[''])
        # two-stage models (options/train_options.py:42-64)
        a('--lr1', type=float, default=0.0002)
        a('--lr2', type=float, default=0.0002)
        a('--lambda_D1', type=float, default=[1.0], nargs='+')
        a('--no_lsgan1', action='store_true')
        a('--n_update_D1', type=int, default=1)
        a('--lambda_D2', type=float, default=[1.0], nargs='+')
        a('--no_lsgan2', action='store_true')
        a('--n_update_D2', type=int, default=1)
        a('--sequential_train', action='store_true')
        a('--which_epoch_sequential', type=str, default='seq')
        a('--use_multi_class_GAN', action='store_true')
        a('--detach_G1_from_G2_x', action='store_true')
        a('--detach_G1_from_G2_y', action='store_true')
        a('--GAN_losses_D2', nargs='+', default=['real_fake'])
        a('--GAN_losses_G2', nargs='+', default=['real_fake'])
        a('--lambda_A_cycle', type=float, default=10.0)
        a('--lambda_B_cycle', type=float, default=10.0)
        a('--use_fixed_noise1', action='store_true')
        a('--lambda_G1', type=float, default=1)
        a('--lambda_G2', type=float, default=1)
        # the U-Net border term of the supervised segmentation baseline (not in the reference)
        a('--border_weight', type=float, default=None, nargs=2, metavar=('W0', 'SIGMA'),
          help='segmentation with --which_model_netD None: add the U-Net border term W0 exp(-(d1 + d2)^2 / (2 SIGMA^2)) to the '
               'cross-entropy weight of every wall pixel between two cells (not in the reference; default off)')
        a('--border_radius', type=int, default=None, help='search radius of --border_weight in pixels, 1..32; default min(32, ceil(4 SIGMA))')
        a('--border_class', type=int, default=0, help='the class whose pixels form the wall between objects (--border_weight)')
        # the soft-clDice term of the segmentation trainers (Shit et al., CVPR 2021; not in the reference)
        a('--cldice_weight', type=float, default=0.0, metavar='LAMBDA',
          help='--model segmentation: add LAMBDA * soft-clDice of the --cldice_class probability plane against the truth to the '
               'generator loss (with or without discriminators, softmax or sigmoid head); 0 = off')
        a('--cldice_iters', type=int, default=5, metavar='K', help='soft-skeleton iterations of --cldice_weight, 1..16')
        a('--cldice_class', type=int, default=0, help='the class whose plane the soft-clDice term reads (the wall, as the label-based scores)')
        # the Lovasz-softmax term of the segmentation trainers (Berman, Triki, Blaschko, CVPR 2018; not in the reference)
        a('--lovasz_weight', type=float, default=0.0, metavar='LAMBDA',
          help='--model segmentation: add LAMBDA * Lovasz-softmax (the Lovasz extension of the Jaccard loss, classes present in the '
               'crop only) of the --lovasz_classes planes to the generator loss (with or without discriminators, softmax or sigmoid '
               'head); 0 = off')
        a('--lovasz_classes', type=int, default=[0], nargs='+', metavar='C', help='the 1..8 classes of --lovasz_weight (default 0, the wall)')
        # the Dice / Tversky and focal terms of the segmentation trainers, on the logits (not in the reference)
        a('--dice_weight', type=float, default=0.0, metavar='LAMBDA',
          help='--model segmentation: add LAMBDA * Tversky loss (soft Dice at the default --tversky 0.5 0.5) of the --dice_classes '
               'channels to the generator loss (with or without discriminators, softmax or sigmoid head); 0 = off')
        a('--dice_classes', type=int, default=[0], nargs='+', metavar='C', help='the 1..8 classes of --dice_weight (default 0, the wall)')
        a('--tversky', type=float, default=[0.5, 0.5], nargs=2, metavar=('A', 'B'),
          help='--dice_weight: the weights of false positives (A) and false negatives (B) in the Tversky index; 0.5 0.5 = Dice')
        a('--dice_smooth', type=float, default=1.0, metavar='S', help='--dice_weight: added to numerator and denominator, >= 0')
        a('--tversky_power', type=float, default=1.0, metavar='E',
          help='--dice_weight: the loss is (1 - TI)^E, 0 < E <= 4; 0.75 = the focal-Tversky loss of Abraham & Khan')
        a('--focal_weight', type=float, default=0.0, metavar='LAMBDA',
          help='--model segmentation: add LAMBDA * focal loss of the logits (class weights from --weights) to the generator loss '
               '(with or without discriminators, softmax or sigmoid head); 0 = off')
        a('--focal_gamma', type=float, default=2.0, metavar='G', help='--focal_weight: the focusing exponent, 0 <= G <= 8 (0 = cross-entropy)')
        # the distance-map terms of the segmentation trainers, on the logits (Kervadec et al., MIDL 2019; Karimi & Salcudean, TMI 2019; not in the reference)
        a('--boundary_loss_weight', type=float, default=0.0, metavar='LAMBDA',
          help='--model segmentation: add LAMBDA * boundary loss (the --dist_class probability weighted by the signed distance to the '
               'true boundary) to the generator loss (with or without discriminators, softmax or sigmoid head); 0 = off')
        a('--hausdorff_weight', type=float, default=0.0, metavar='LAMBDA',
          help='--model segmentation: add LAMBDA * distance-transform Hausdorff loss ((p - g)^2 weighted by the distance maps of the '
               'truth and of the thresholded prediction, recomputed every step) of --dist_class to the generator loss; 0 = off')
        a('--hausdorff_alpha', type=float, default=2.0, metavar='A', help='--hausdorff_weight: the exponent of the distances, 0 < A <= 4')
        a('--dist_class', type=int, default=0, metavar='C',
          help='the class of --boundary_loss_weight / --hausdorff_weight (default 0, the wall)')
        # random elastic deformation of every training crop, on the device (not in the reference, which augments with crop, flip and rot90)
        a('--elastic', type=float, default=None, nargs=2, metavar=('G', 'SIGMA'),
          help='image-folder feeders: deform every training crop by a smooth random field -- (G + 3)^2 displacement vectors drawn from '
               'N(0, SIGMA^2) source pixels on a grid of G x G cells (1..13) over the crop, interpolated bicubically per pixel, fused '
               'into the crop / flip / rot90 kernel (not in the reference; default off)')
        a('--elastic_label_channels', type=str, default='rg',
          help='letters of the RGB channels that hold labels and are sampled at the nearest pixel under --elastic; the others are '
               'sampled bilinearly (default rg: the reference keeps labels in r and g and the image in b)')
        # photometric augmentation of every training crop, on the device (not in the reference): check_photo_options, DESIGN.md R38
        a('--photo_aug', type=str, default=None, metavar='LIST',
          help='image-folder feeders: vary the grey values of the image channels of every training crop -- a comma list of blur, '
               'gamma, contrast, brightness, noise, occlude; each listed stage fires with probability --photo_prob, and they apply '
               'in that order after the crop / flip / rot90 / --elastic kernel (not in the reference; default off)')
        a('--photo_prob', type=float, default=0.5, metavar='P', help='--photo_aug: the probability of each listed stage')
        a('--photo_blur', type=float, default=2.0, metavar='SMAX', help='--photo_aug blur: Gaussian blur of sigma ~ U(0.5, SMAX) pixels, SMAX <= 4')
        a('--photo_gamma', type=float, default=1.5, metavar='G', help='--photo_aug gamma: gamma = exp(U(-ln G, ln G)) on the [0, 1] grey value, G <= 2')
        a('--photo_contrast', type=float, default=0.25, metavar='C', help='--photo_aug contrast: c ~ U(1 - C, 1 + C) about mid-grey, C < 1')
        a('--photo_brightness', type=float, default=0.1, metavar='B', help='--photo_aug brightness: b ~ U(-B, B) in [0, 1] grey value units')
        a('--photo_noise', type=float, default=0.05, metavar='S', help='--photo_aug noise: additive N(0, sigma_n^2), sigma_n ~ U(0, S) in [-1, 1] units')
        a('--photo_occlude', type=float, default=(2, 0.25), nargs=2, metavar=('K', 'FRAC'),
          help='--photo_aug occlude: K <= 4 boxes of sides U(1, FRAC fineSize) filled with a value ~ U(-1, 1)')
        a('--photo_channels', type=str, default='b',
          help='letters of the RGB channels that hold the image and are varied by --photo_aug; must not share a letter with '
               '--elastic_label_channels (default b: the reference keeps labels in r and g and the image in b)')
        # exponential moving average of the generator's weights (not in the reference, which evaluates the last iterate)
        a('--ema_decay', type=float, default=None, metavar='D',
          help='fcgan / cgan / cgan2 / segmentation: keep an exponential moving average of the generator, shadow += (1 - D) (G - shadow) '
               'after every generator update (one launch, inside the graphed step), saved as <epoch>_net_G_ema.pth; 0 <= D <= 1, '
               'unset: off.  BatchNorm statistics are not averaged: the average takes the live ones')
        a('--ema_warmup', action='store_true', help='--ema_decay: use min(D, (1 + t) / (10 + t)) at update t, so that a short run is not '
                                                    'dominated by the initial weights')
        a('--ema_eval', action='store_true', help='--ema_decay: test() and the validation pass of train_ss.py (and so --best_metric) run '
                                                  'the averaged generator')
        # differentiable augmentation of the discriminator inputs (DiffAugment, Zhao et al. 2020; not in the reference)
        a('--diffaug', type=str, default=None, metavar='POLICY',
          help='fcgan / cgan / cgan2 / segmentation with discriminators: a comma list of translation, cutout, brightness, contrast '
               '(color = brightness,contrast); every tensor a discriminator sees, real and fake, goes through one random transform '
               'and the generator\'s gradient flows back through it (inside the graphed step).  Unset: off')
        a('--diffaug_translation', type=float, default=0.125, help='--diffaug translation: largest shift as a fraction of the side')
        a('--diffaug_cutout', type=float, default=0.5, help='--diffaug cutout: side of the zeroed square as a fraction of the side')
        a('--diffaug_color_channels', type=str, default='b',
          help='letters of the RGB channels that hold the image (letters as in --elastic_label_channels): brightness and contrast touch '
               'these channels of the discriminator input only (default b: the reference keeps labels in r and g and the image in b)')
        self.isTrain = True


class TestOptions(BaseOptions):
    def initialize(self):
        BaseOptions.initialize(self)
        a = self.parser.add_argument
        a('--ntest', type=int, default=float("inf"))
        a('--results_dir', type=str, default='./results/')
        a('--aspect_ratio', type=float, default=1.0)
        a('--phase', type=str, default='test')
        a('--which_epoch', type=str, default='latest')
        a('--how_many', type=int, default=50)
        a('--save_as_single_image', action='store_true')
        # whole-image inference of test_ss.py (not in the reference, which scores one crop per file): check_tile_options, DESIGN.md R21
        a('--whole_image', action='store_true',
          help='segmentation: predict the whole image (after the resize of --resize_or_crop, no crop) from overlapping tiles of the '
               'mirrored image, their margins dropped and their overlaps blended')
        a('--tile', type=int, default=None, help='side T of a tile (default --fineSize)')
        a('--tile_margin', type=int, default=16, help='M: pixels at every side of a tile that are predicted but not used')
        a('--tile_ramp', type=int, default=16, help='R: width of the linear ramp of the blending window behind the margin, 1..64')
        a('--tile_stride', type=int, default=None, help='S: distance between tile origins, 1 .. T - 2 M (default T - 2 M - R, at least 1)')
        a('--tta', type=str, default='none', choices=['none', 'd4'],
          help='d4: average the prediction over the 8 flips and rotations of every tile; without --whole_image, of the one --fineSize crop')
        a('--use_ema', action='store_true',
          help='load <which_epoch>_net_G_ema.pth, the averaged generator a run with --ema_decay saves, in place of <which_epoch>_net_G.pth '
               '(--model test, fcgan, cgan, cgan2, segmentation); everything downstream runs on the average')
        self.isTrain = False
