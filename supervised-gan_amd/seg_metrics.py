"""The accuracy half of the segmentation trainers (segm_model.py:265-341 of the reference): SegMetrics owns the device accumulators
of every `--which_metric` name and the planes the scores share; SegMetricsMixin gives a trainer the public methods over it.

accumulate() only enqueues kernels (sgan_metrics.hip and its neighbours) behind the step, so a training loop that accumulates
after every step never waits for the GPU; read() and counts() are the only places that synchronise and read.

The label-based scores are taken on CHANNEL 0 of fake_B and real_B: the first picked label channel, the boundary map (the background
class of --add_background_onehot comes last).  The reference (segm_model.py:299-307) asserts num_classes == 2 and then hands the
whole 2-channel maps to a function that squeezes a channel axis of size one, which cannot run; this is our reading of that call
("Segmentation metrics on the device").  Batch 1, like every kernel of this path.  An image whose truth map has no free
pixel scores NaN, and the NaN stays in the running sum until reset(), as in the reference's running mean; nothing on the host sees
it before read().

With --clean_close / --clean_min_wall / --clean_min_cell the predicted plane of every label-based score is the CLEANED wall map
(ops.clean_wall: gaps closed with a disk, wall specks dropped, small regions filled), made once per accumulate().  With
--clean_split the merged cells of that map are cut apart (ops.split_cells) between the specks and the small cells: the stages run in
the order close, specks, split, small cells -- splitting can shave slivers off a cell, which --clean_min_cell is there to fill -- as
clean_wall without min_cell, split_cells, and clean_wall with min_cell alone.  meanIU and the
confusion matrix stay on the logits: they are per-pixel class scores, and may be multi-class."""
from collections import OrderedDict
from functools import cached_property

import numpy as np
import torch

from . import ops, util
from .options import clean_params, split_params, topo_params

# Every device accumulator: name, dtype, shape (k: the classes of the confusion matrix).  Each is made the first time a score adds
# to it; reset(), read() and counts() walk this table.
ACCUMULATORS = (
    ('rand', torch.float64, (2,)),                                # sum of the Rand F-scores, images
    ('vinfo', torch.float64, (2,)),                               # sum of VInfo, images
    ('conf', torch.int64, lambda k: (k, k)),                      # [label, prediction]
    ('rand_thin', torch.float64, (2,)),                           # the same two sums after border thinning
    ('vinfo_thin', torch.float64, (2,)),
    ('obj_i', torch.int64, (len(ops.OBJECT_COUNTS),)),            # ops.object_match_accumulate's pooled counters
    ('obj_f', torch.float64, (len(ops.OBJECT_SUMS),)),
    ('bnd_i', torch.int64, (len(ops.BOUNDARY_COUNTS),)),          # ops.boundary_accumulate's pooled counters
    ('bnd_f', torch.float64, (len(ops.BOUNDARY_SUMS),)),
)
# The counters of the cleaning stage, made only when a --clean_* option is set; beside ACCUMULATORS, and walked with it.
CLEAN_ACCUMULATORS = (
    ('clean_i', torch.int64, (len(ops.CLEAN_COUNTS),)),           # ops.clean_wall's pooled counters
    ('clean_post_i', torch.int64, (len(ops.CLEAN_COUNTS),)),      # ... of the second call, small cells after --clean_split (its own image count)
    ('split_i', torch.int64, (len(ops.SPLIT_COUNTS),)),           # ops.split_cells' pooled counters
)
# The pooled integers of the topology scores, made only when Betti0Err, Betti1Err or clDice is asked for; beside ACCUMULATORS too.
TOPO_ACCUMULATORS = (
    ('topo_i', torch.int64, (len(ops.TOPO_COUNTS),)),             # ops.topo_accumulate's pooled counters
)
COUNTS = {'objects': ('obj_i', 'obj_f', ops.OBJECT_COUNTS, ops.OBJECT_SUMS),
          'boundary': ('bnd_i', 'bnd_f', ops.BOUNDARY_COUNTS, ops.BOUNDARY_SUMS)}
SCORES = ('RandScore', 'VInfo', 'meanIU', 'RandScoreThin', 'VInfoThin') + util.OBJECT_METRICS + util.BOUNDARY_METRICS + util.TOPO_METRICS      # as read() orders them
VALUES = ('confusion', 'numAveragedPixels', 'numAveragedImages', 'pixelAcc', 'meanAcc') + SCORES


class _Planes:
    """The intermediates the scores of one accumulate() call share, each enqueued the first time one of them asks for it and handed
    to whoever asks again: both maps are labelled once, and the prediction is thinned once, however many scores read them."""

    def __init__(self, metrics, fake_B, real_B):
        self.m, self.fake_B, self.real_B = metrics, fake_B, real_B

    def _store(self, name, dtype):
        return self.m._plane(name, dtype, tuple(self.t.shape))

    @cached_property
    def s(self):
        """The predicted plane every label-based score reads: channel 0 as it lies, or its cleaned wall map with a --clean_* option."""
        clean, (split_rsq, rounds) = clean_params(self.m.opt), split_params(self.m.opt)
        s = self.fake_B.detach()[0, 0]
        if not split_rsq:
            if not any(clean):
                return s
            return ops.clean_wall(s, *clean, out=self._store('cleaned', torch.float32), acc=self.m._acc('clean_i'))
        # close, specks | split | small cells: two planes are ping-ponged, the last stage that runs writes 'cleaned'
        close_rsq, min_wall, min_cell = clean
        last, other = ('cleaned', 'cleaned_mid') if not min_cell else ('cleaned_mid', 'cleaned')
        if close_rsq or min_wall:
            s = ops.clean_wall(s, close_rsq, min_wall, 0, out=self._store(other, torch.float32), acc=self.m._acc('clean_i'))
        s = ops.split_cells(s, split_rsq, rounds, out=self._store(last, torch.float32), acc=self.m._acc('split_i'))
        if min_cell:
            s = ops.clean_wall(s, 0, 0, min_cell, out=self._store('cleaned', torch.float32), acc=self.m._acc('clean_post_i'))
        return s

    @cached_property
    def t(self):
        return self.real_B.detach()[0, 0]

    @cached_property
    def truth_labels(self):
        return ops.ccl_label(self.t, self._store('truth_labels', torch.int32))

    @cached_property
    def pred_labels(self):
        return ops.ccl_label(self.s, self._store('pred_labels', torch.int32))

    @cached_property
    def thinned(self):
        """The prediction thinned to one-pixel lines (util.compute_thinned_scores, the reference's do_thin=True); the truth is not."""
        return ops.thin(self.s, out=self._store('thinned', torch.float32))

    @cached_property
    def thinned_truth(self):
        """The truth thinned by the same ops.thin: the skeleton clDice's sensitivity is taken on."""
        return ops.thin(self.t, out=self._store('thinned_truth', torch.float32))

    @cached_property
    def thinned_labels(self):
        return ops.ccl_label(self.thinned, self._store('thinned_labels', torch.int32))

    @cached_property
    def dsq(self):
        """The exact squared distance transforms of the true and the predicted wall; with --boundary_thin of the thinned one."""
        wall = self.thinned if self.m.opt.boundary_thin else self.s
        return ops.edt_sq(self.t, out=self._store('truth_dsq', torch.int32)), ops.edt_sq(wall, out=self._store('pred_dsq', torch.int32))


class SegMetrics:
    def __init__(self, opt, device, num_classes):
        self.opt, self.device, self.num_classes = opt, device, num_classes
        self.acc = {}          # name of ACCUMULATORS -> its device tensor, for the scores that were taken at least once
        self.planes = {}       # name -> the persistent [H, W] tensor behind an intermediate of _Planes
        self.reset()

    def reset(self):
        self.values = dict.fromkeys(VALUES, 0)      # what read() derived last; the trainers mirror it as attributes
        for t in self.acc.values():
            t.zero_()

    def _acc(self, name):
        if name not in self.acc:
            k = self.num_classes + 1 if self.opt.add_background_onehot_acc else self.num_classes
            dtype, shape = next((d, s(k) if callable(s) else s) for n, d, s in ACCUMULATORS + CLEAN_ACCUMULATORS + TOPO_ACCUMULATORS if n == name)
            self.acc[name] = torch.zeros(shape, dtype=dtype, device=self.device)
        return self.acc[name]

    def _plane(self, name, dtype, hw):
        """The one place a plane is (re-)made: train_ss.py validates at --valSize, so the size may change from call to call."""
        p = self.planes.get(name)
        if p is None or tuple(p.shape) != hw:
            p = self.planes[name] = torch.empty(hw, dtype=dtype, device=self.device)
        return p

    @property
    def truth_labels(self):
        """The label map of the truth as the last accumulate() that labelled it left it (int32 [H, W]), or None.  Read only."""
        return self.planes.get('truth_labels')

    @property
    def cleaned(self):
        """The cleaned predicted wall map as the last accumulate() left it (float32 [H, W] of 0.0 / 1.0; after every stage that is on,
        --clean_split included), or None without a --clean_* option.  Read only."""
        return self.planes.get('cleaned')

    def accumulate(self, fake_B, real_B, logit, label, which=None):
        """Adds the scores named by --which_metric (or `which`) for one prediction / truth pair to their accumulators:

        RandScore / VInfo: util.compute_Rand_F_scores / compute_VInfo_scores of the two label maps.  The counting pass is the
        expensive launch and both scores are functions of its counters, so asking for both costs one count; the Rand value added is
        rand_f_accumulate's, bit for bit.  RandScoreThin / VInfoThin: the same of the thinned prediction against the truth.
        ObjF1 .. PQ: which truth cell is found by which predicted cell at IoU > 0.5 .. 0.95 (ops.object_match_accumulate), regions
        below --min_object_area left out.  meanIU: conf[label, prediction] += 1 for every pixel (segm_model.py:309-331).
        BoundF .. ASSD: how far every predicted wall pixel lies from the true wall and every true wall pixel from the predicted one
        (ops.boundary_accumulate).
        Betti0Err / Betti1Err / clDice: the Betti numbers of every --topo_window window of both walls and, for clDice alone, the
        skeleton pixels of the thinned prediction and of the thinned truth (ops.topo_accumulate, one call for the three).
        With a --clean_* option all of these but meanIU read the cleaned prediction (ops.clean_wall, once per call; with
        --clean_split ops.split_cells between its specks and its small cells)."""
        o = self.opt
        which = o.which_metric if which is None else which
        if any(k in which for k in SCORES if k != 'meanIU'):      # the scores of the label maps and of the walls
            assert self.num_classes == 2      # binary segmentation only, as in the reference
            assert fake_B.shape[0] == 1, "the device metrics take batch 1, like every kernel of this path"
        p = _Planes(self, fake_B, real_B)
        if 'VInfo' in which or 'RandScore' in which:
            self._rand_vinfo(p.truth_labels, p.pred_labels, 'rand' if 'RandScore' in which else None, 'vinfo' if 'VInfo' in which else None)
        if any(k in which for k in util.OBJECT_METRICS):
            ops.object_match_accumulate(p.truth_labels, p.pred_labels, self._acc('obj_i'), self._acc('obj_f'), min_area=o.min_object_area)
        if 'RandScoreThin' in which or 'VInfoThin' in which:
            self._rand_vinfo(p.truth_labels, p.thinned_labels, 'rand_thin' if 'RandScoreThin' in which else None,
                             'vinfo_thin' if 'VInfoThin' in which else None)
        if 'meanIU' in which:
            assert logit.shape[0] == 1, "the device metrics take batch 1, like every kernel of this path"
            if o.add_background_onehot_acc:
                ops.confusion_accumulate(ops.as_nhwc(fake_B.detach()), self.num_classes, self._acc('conf'), y=ops.as_nhwc(real_B.detach()),
                                         add_background=True)
            else:
                ops.confusion_accumulate(ops.as_nhwc(logit.detach()), self.num_classes, self._acc('conf'), label=label)
        if any(k in which for k in util.BOUNDARY_METRICS):
            t_dsq, s_dsq = p.dsq
            ops.boundary_accumulate(t_dsq, s_dsq, self._acc('bnd_i'), self._acc('bnd_f'))
        if any(k in which for k in util.TOPO_METRICS):
            window, stride = topo_params(o)
            cl = 'clDice' in which
            ops.topo_accumulate(p.t, p.s, self._acc('topo_i'), t_thin=p.thinned_truth if cl else None, s_thin=p.thinned if cl else None,
                                window=window, stride=stride)

    def _rand_vinfo(self, t_labels, s_labels, rand, vinfo):
        if vinfo is not None:          # one counting pass feeds both scores
            ops.vinfo_accumulate(t_labels, s_labels, self._acc(vinfo), acc_rand=self._acc(rand) if rand is not None else None)
        else:
            ops.rand_f_accumulate(t_labels, s_labels, self._acc(rand))

    def counts(self, which):
        """'topology': the twelve pooled integers of ops.TOPO_COUNTS (windows, the summed Betti differences and Betti numbers, the
        skeleton pixels, images).  'split': the six pooled integers of ops.SPLIT_COUNTS (core components, cut pixels, labelled pixels, rounds, budget hits,
        images).  'clean': the six pooled integers of ops.CLEAN_COUNTS (pixels set by the closing, wall components / pixels removed, cells /
        cell pixels filled, images).  Otherwise the pooled numbers of 'objects' (the 16 integers of ops.OBJECT_COUNTS: TP_0 .. TP_9 at IoU > 0.5 .. 0.95, N_t, N_s, images,
        SEGn; the two sums of ops.OBJECT_SUMS) or 'boundary' (the 80 integers of ops.BOUNDARY_COUNTS: the two histograms by distance
        bin, N_s, N_t, images, ...; the four sums of ops.BOUNDARY_SUMS) since reset(), as a dict.  Synchronises, like read()."""
        if which == 'clean':
            if 'clean_i' in self.acc or 'clean_post_i' in self.acc:
                ops.check_metric_err(self.device)
            return OrderedDict(zip(ops.CLEAN_COUNTS, self._clean_counts()))
        if which == 'topology':
            ints = [0] * len(ops.TOPO_COUNTS)
            if 'topo_i' in self.acc:
                ops.check_metric_err(self.device)
                ints = self.acc['topo_i'].cpu().tolist()
            return OrderedDict(zip(ops.TOPO_COUNTS, ints))
        if which == 'split':
            ints = [0] * len(ops.SPLIT_COUNTS)
            if 'split_i' in self.acc:
                ops.check_metric_err(self.device)
                ints = self.acc['split_i'].cpu().tolist()
            return OrderedDict(zip(ops.SPLIT_COUNTS, ints))
        acc_i, acc_f, names_i, names_f = COUNTS[which]
        ints, sums = [0] * len(names_i), [0.0] * len(names_f)
        if acc_i in self.acc:
            ops.check_metric_err(self.device)
            ints, sums = self.acc[acc_i].cpu().tolist(), self.acc[acc_f].cpu().tolist()
        return OrderedDict(list(zip(names_i, ints)) + list(zip(names_f, sums)))

    def _clean_counts(self):
        """The pooled CLEAN_COUNTS: with --clean_split the two clean_wall calls of an image count into accumulators of their own, whose
        stage counters add up and whose image counts are the same number."""
        a, b = ([0] * len(ops.CLEAN_COUNTS) if n not in self.acc else self.acc[n].cpu().tolist() for n in ('clean_i', 'clean_post_i'))
        return [x + y for x, y in zip(a[:5], b[:5])] + [max(a[5], b[5])]

    def read(self):
        """Reads the accumulators and derives every score from them into self.values; returns the ones --which_metric names, in the
        order RandScore, VInfo, meanIU, RandScoreThin, VInfoThin, then ObjF1 / ObjAP / SEG / PQ (util.object_scores of the pooled
        counts), then BoundF / HausD / ASSD (util.boundary_scores at --boundary_tolerance).  Built for evaluation (test_ss.py) it also
        prints the pooled TP_k / N_t / N_s line when an object score was taken, and the boundary precision / recall / F at the
        tolerances 0 .. 5 with the dataset's worst distance when a boundary score was, and the pooled counts of the cleaning stage
        when a --clean_* option ran it, then those of --clean_split, then the `topology:` line (windows, the mean Betti numbers
        of either map, Tprec / Tsens) when a topology score was taken.  Betti0Err / Betti1Err / clDice (util.topo_scores of the pooled
        integers) come last."""
        o, v = self.opt, self.values
        if self.acc:
            ops.check_metric_err(self.device)
            k = self.num_classes + 1 if o.add_background_onehot_acc else self.num_classes
            a = {n: self.acc[n].cpu().numpy() if n in self.acc else np.zeros(s(k) if callable(s) else s) for n, _, s in ACCUMULATORS}
            obj_i, bnd_i = a['obj_i'], a['bnd_i']
            topo_i = self.acc['topo_i'].cpu().numpy() if 'topo_i' in self.acc else np.zeros(len(ops.TOPO_COUNTS), dtype=np.int64)
            oc, bc = ops.OBJECT_COUNTS.index, ops.BOUNDARY_COUNTS.index
            for key, n in (('RandScore', 'rand'), ('VInfo', 'vinfo'), ('RandScoreThin', 'rand_thin'), ('VInfoThin', 'vinfo_thin')):
                v[key] = a[n][0] / a[n][1] if a[n][1] else 0
            v['numAveragedImages'] = int(max(a['rand'][1], a['vinfo'][1], a['rand_thin'][1], a['vinfo_thin'][1],
                                             obj_i[oc('images')], bnd_i[bc('images')], topo_i[ops.TOPO_COUNTS.index('images')]))
            v.update(util.object_scores(obj_i, a['obj_f']))
            v.update(util.boundary_scores(bnd_i, a['bnd_f'], o.boundary_tolerance))
            v.update(util.topo_scores(topo_i))
            if not o.isTrain and 'obj_i' in self.acc and any(key in o.which_metric for key in util.OBJECT_METRICS):
                # the evaluation drivers read the accuracies once, after the dataset: the per-threshold table goes beside them
                print('objects: TP at IoU > 0.50 .. 0.95: %s, N_t %d, N_s %d (min area %d)'
                      % (' '.join(str(int(x)) for x in obj_i[:10]), obj_i[oc('N_t')], obj_i[oc('N_s')], o.min_object_area))
            if not o.isTrain and 'bnd_i' in self.acc and any(key in o.which_metric for key in util.BOUNDARY_METRICS):
                print('boundary: P/R/F at tolerance 0 .. 5: %s, worst distance %.3f (N_s %d, N_t %d%s)'
                      % (' '.join('%.4f/%.4f/%.4f' % util.boundary_pr(bnd_i, tol) for tol in range(6)),
                         float(np.sqrt(float(max(bnd_i[bc('max_dsq_s')], bnd_i[bc('max_dsq_t')])))), bnd_i[bc('N_s')], bnd_i[bc('N_t')],
                         ', prediction thinned' if o.boundary_thin else ''))
            if not o.isTrain and ('clean_i' in self.acc or 'clean_post_i' in self.acc):
                c = self._clean_counts()
                print('clean: closed %d pixels, removed %d wall components (%d pixels), filled %d cells (%d pixels) in %d images '
                      '(close_rsq %d, min wall %d, min cell %d)' % (tuple(c) + clean_params(o)))
            if not o.isTrain and 'split_i' in self.acc:
                c = self.acc['split_i'].cpu().tolist()
                print('split: %d cores, cut %d pixels, labelled %d pixels in %d rounds, budget hit in %d of %d images '
                      '(split_rsq %d, %d rounds)' % (tuple(c) + split_params(o)))
            if not o.isTrain and 'topo_i' in self.acc and any(key in o.which_metric for key in util.TOPO_METRICS):
                c = dict(zip(ops.TOPO_COUNTS, (int(x) for x in topo_i)))
                n = max(1, c['windows'])
                print('topology: %d windows of %d at stride %d, mean b0 / b1 of the prediction %.3f / %.3f, of the truth %.3f / %.3f, '
                      'Tprec %.4f, Tsens %.4f' % ((c['windows'],) + topo_params(o) + (c['b0_s'] / n, c['b1_s'] / n, c['b0_t'] / n, c['b1_t'] / n,
                                                   c['skel_s_in_t'] / max(1, c['skel_s']), c['skel_t_in_s'] / max(1, c['skel_t']))))
            conf = a['conf'].astype(np.float64)
            v['confusion'], v['numAveragedPixels'] = conf, int(conf.sum())
            rel, sel, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
            v['pixelAcc'] = tp.sum() / max(1, v['numAveragedPixels'])
            v['meanAcc'] = float(np.mean(tp / np.maximum(1, rel)))
            v['meanIU'] = float(np.mean(tp / np.maximum(1, rel + sel - tp)))
        return OrderedDict((key, v[key]) for key in SCORES if key in o.which_metric)


class SegMetricsMixin:
    """The accuracy methods of a segmentation trainer over its `seg_metrics`; what read() derived is mirrored on the trainer
    (confusion, numAveragedPixels, numAveragedImages, pixelAcc, meanAcc and the score names), where the drivers look for it."""

    def reset_accs(self):
        self.seg_metrics.reset()
        self.__dict__.update(self.seg_metrics.values)

    def accum_accs(self, which=None):
        self.seg_metrics.accumulate(self.fake_B, self.real_B, self.logit, self.label, which)

    def compute_current_Rand_score(self):
        self.accum_accs(('RandScore',))

    def compute_current_accuracy(self):
        self.accum_accs(('meanIU',))

    def get_current_accs(self):
        accs = self.seg_metrics.read()
        self.__dict__.update(self.seg_metrics.values)
        return accs

    def get_object_counts(self):
        return self.seg_metrics.counts('objects')

    def get_boundary_counts(self):
        return self.seg_metrics.counts('boundary')

    def get_clean_counts(self):
        return self.seg_metrics.counts('clean')

    def get_split_counts(self):
        return self.seg_metrics.counts('split')

    def get_topology_counts(self):
        return self.seg_metrics.counts('topology')

    def with_cleaned_visual(self, visuals):
        """Built for evaluation with a --clean_* option: adds the wall map the label-based scores of the last accum_accs() were taken
        on to the trainer's visuals as `fake_B_clean` ([1, 1, H, W] in [-1, 1]), so that test_ss.py's result page shows it."""
        cleaned = self.seg_metrics.cleaned
        if not self.opt.isTrain and (any(clean_params(self.opt)) or split_params(self.opt)[0]) and cleaned is not None:
            visuals['fake_B_clean'] = cleaned.detach()[None, None] * 2 - 1
        return visuals
