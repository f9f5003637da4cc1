"""Image-folder feeders with the reference's transforms (data/single_dataset.py, data/aligned_dataset.py, data/base_dataset.py:17-55,
data/image_folder.py): file listing and PIL decode on the host; the decoded uint8 image is uploaded once and everything after it
runs on the device -- Image.resize (`sgan_image_resize`, bit-exact with Pillow's two-pass resampler) and ONE kernel for
crop -> flip -> rot90 -> ToTensor -> Normalize (`sgan_image_prep`) -- so neither the resized nor the float image ever exists in
host memory and the trainers' set_input reads a device tensor.

Yields what the reference's DataLoader yields at batchSize 1: {'A': [1, 3, H, W] in [-1, 1], 'A_paths': [path]} (single) or
{'A', 'B', 'A_paths', 'B_paths'} (aligned, unaligned).  Random draws use Python's `random` like the reference; the aligned feeder makes them
in the reference's order (aligned_dataset.py:31-38), the single feeder's crop offsets are torchvision-internal there and drawn
here as x then y.

`--elastic G SIGMA` (train options; not in the reference) deforms every training crop: the feeder draws the (G + 3)^2 control vectors
of a smooth field after its other draws, uploads these few hundred floats, and the same single kernel gathers through the field
(`sgan_image_prep_elastic`).  One field for both halves of an aligned pair, one per image otherwise.

`--photo_aug LIST` (train options; not in the reference) varies the grey values of every training crop: after all the draws above the
feeder draws the parameters of blur, gamma, contrast, brightness, noise and occlusion boxes (util.photo_draw), and one more kernel
(`sgan_image_photo`) applies them to the image channels of the prepared crop.  One record for both halves of an aligned pair (each
half with noise planes of its own), one per image otherwise.  Withheld wherever `--elastic` is.

`--whole_image` / `--tta d4` (test options; not in the reference): the single-image feeder also yields the uint8 device image under
'A_u8', and under `--whole_image` 'A' is the whole resized image, not a crop (`sgan_image_prep_tile`)."""
import os
import random

import numpy as np
import torch

from . import ops

IMG_EXTENSIONS = ['.jpg', '.JPG', '.jpeg', '.JPEG', '.png', '.PNG', '.ppm', '.PPM', '.bmp', '.BMP']      # image_folder.py:14-17


def make_dataset(dir):
    """All image files under `dir`, subdirectories included (data/image_folder.py:24-35)."""
    assert os.path.isdir(dir), '%s is not a valid directory' % dir
    images = []
    for root, _, fnames in sorted(os.walk(dir)):
        for fname in fnames:
            if any(fname.endswith(e) for e in IMG_EXTENSIONS):
                images.append(os.path.join(root, fname))
    return images


def _scale_width_size(ow, oh, target_width):
    """(w, h) after __scale_width (base_dataset.py:43-50)."""
    if ow == target_width:
        return ow, oh
    return target_width, int(target_width * oh / ow)


class _FolderDataset:
    def __init__(self, opt, device=None):
        self.opt = opt
        self.device = device if device is not None else torch.device('cuda', opt.gpu_ids[0])
        self.paths = sorted(make_dataset(os.path.join(opt.dataroot, opt.phase)))
        if not self.paths:
            raise RuntimeError('no images under %s' % os.path.join(opt.dataroot, opt.phase))
        self.order = list(range(len(self.paths)))

    def __len__(self):
        return min(len(self.paths), self.opt.max_dataset_size) if getattr(self.opt, 'max_dataset_size', None) else len(self.paths)

    def _to_device(self, img):
        return torch.from_numpy(np.array(img, dtype=np.uint8)).to(self.device, non_blocking=True)      # [H, W, 3], a writable copy

    def _draw_elastic(self):
        """--elastic G SIGMA on a training feeder: the 2 (G + 3)^2 control displacements of one field, random.gauss(0, SIGMA) row-major
        with dx before dy, drawn on the calling thread AFTER the item's other draws (none of which moves) and uploaded as [G + 3,
        G + 3, 2] fp32.  None when the option is off or the feeder does not train: then no draw is made."""
        el = getattr(self.opt, 'elastic', None)
        if not self.opt.isTrain or el is None:
            return None
        g, sigma = int(el[0]), float(el[1])
        vals = [random.gauss(0.0, sigma) for _ in range(2 * (g + 3) * (g + 3))]
        return torch.tensor(vals, dtype=torch.float32).view(g + 3, g + 3, 2).to(self.device, non_blocking=True)

    def _image_prep(self, dev, x0, y0, n, flip, rot, ctrl):
        """crop -> flip -> rot90 -> ToTensor -> Normalize in one kernel; through the elastic field of `ctrl` when there is one."""
        if ctrl is None:
            return ops.image_prep(dev, x0, y0, n, flip, rot)
        from .options import elastic_nearest_mask
        return ops.image_prep_elastic(dev, x0, y0, n, flip, rot, ctrl, elastic_nearest_mask(self.opt))

    def _draw_photo(self):
        """--photo_aug on a training feeder: the util.PhotoRec of one crop (util.photo_draw documents the draws), drawn on the calling
        thread AFTER the item's other draws, the elastic field included (none of which moves).  None when the option is off or the
        feeder does not train: then no draw is made."""
        if not self.opt.isTrain or getattr(self.opt, 'photo_aug', None) is None:
            return None
        from .util import photo_draw
        return photo_draw(self.opt, self.opt.fineSize, rng=random)

    def _photo(self, crops, rec):
        """The prepared crops that share the record `rec` through sgan_image_photo.  The noise stage reads N(0, 1) planes that
        ops.normal_fill writes into a scratch buffer of the feeder from the record's seed: crop 0 from stream offset 0, crop 1 (the
        second half of an aligned pair) from the offset the first fill left behind."""
        if rec is None:
            return crops
        from .options import photo_channel_mask
        mask = photo_channel_mask(self.opt)
        planes = None
        if rec.sigma_n != 0.0:
            n, P = crops[0].shape[0], bin(mask).count('1')
            if getattr(self, '_photo_noise', None) is None or tuple(self._photo_noise.shape) != (2, P, n, n):
                self._photo_noise = torch.empty((2, P, n, n), dtype=torch.float32, device=self.device)
                self._photo_offset = torch.zeros(1, dtype=torch.int64, device=self.device)
            self._photo_offset.zero_()
            for i in range(len(crops)):
                ops.normal_fill(self._photo_noise[i], rec.seed, self._photo_offset, advance=True)
            planes = self._photo_noise
        return [ops.image_photo(c, rec, mask, noise=None if planes is None else planes[i]) for i, c in enumerate(crops)]

    # An item is made in two halves: _host(index) -- file read, decode, resize: no random draws, safe on worker threads (PIL drops
    # the GIL while it decodes) -- and _device(index, host) -- the random draws in the reference's order, the upload, the kernel.
    def __getitem__(self, index):
        return self._device(index, self._host(index))

    def __iter__(self):
        """--nThreads host decodes run ahead of the consumer (the reference's DataLoader workers, data/custom_dataset_data_loader.py:
        32-37); the random draws and the device work stay on the calling thread, so an epoch is the same with or without them."""
        if not self.opt.serial_batches:
            random.shuffle(self.order)
        order = self.order[:len(self)]
        workers = int(getattr(self.opt, 'nThreads', 0) or 0)
        if workers <= 0:
            for i in order:
                yield self[i]
            return
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=workers) as pool:
            ahead, todo = deque(), iter(order)
            for i in todo:
                ahead.append((i, pool.submit(self._host, i)))
                if len(ahead) >= 2 * workers:
                    break
            while ahead:
                i, fut = ahead.popleft()
                nxt = next(todo, None)
                if nxt is not None:
                    ahead.append((nxt, pool.submit(self._host, nxt)))
                yield self._device(i, fut.result())


class SingleFolderDataset(_FolderDataset):
    """SingleDataset (data/single_dataset.py:8-31) + get_transform (data/base_dataset.py:17-41)."""

    def _host(self, index):
        return self._decode(self.paths[index])

    def _device(self, index, img):
        path = self.paths[index]
        if getattr(self.opt, 'tiling', False):
            return self._device_tiled(img, path)
        draw = self._draw(img, path)
        A = self._prep(img, draw, self._draw_elastic())        # --elastic: the field after every other draw of the item
        A, = self._photo([A], self._draw_photo())              # --photo_aug: its draws after the field's
        return {'A': ops.logical_view(A, 3), 'A_paths': [path]}

    def _device_tiled(self, img, path):
        """Whole-image inference (test options, options.check_tile_options): 'A' as always, and under 'A_u8' the uint8 device image it
        was made from, out of which SegmentationModel.test() cuts its tiles.  --whole_image: the whole image after the resize -- no
        crop, no random draw, any aspect -- through image_prep_tile over the full window.  --tta d4 alone: today's crop, and its
        window of the uint8 image."""
        from .options import check_tile_options
        opt = self.opt
        if opt.whole_image:
            w, h = self._resized_size(*img.size)
            check_tile_options(opt, size=(h, w))
            dev = self._resized(img, w, h)
            return {'A': ops.logical_view(ops.image_prep_tile(dev, 0, 0, h, w, False, 0), 3), 'A_u8': dev, 'A_paths': [path]}
        w, h, x0, y0, flip, rot = self._draw(img, path)
        assert not flip and rot == 0, "--tta d4 makes the flips and rotations itself: an evaluation feeder draws none"
        n = opt.fineSize
        dev = self._resized(img, w, h)
        return {'A': ops.logical_view(ops.image_prep(dev, x0, y0, n, False, 0), 3), 'A_u8': dev[y0: y0 + n, x0: x0 + n].contiguous(),
                'A_paths': [path]}

    def _decode(self, path):
        from PIL import Image
        img = Image.open(path).convert('RGB')
        img.load()
        return img

    def _resized_size(self, ow, oh):
        opt = self.opt
        if opt.resize_or_crop == 'resize_and_crop':
            return opt.loadSize, opt.loadSize                  # transforms.Scale([loadSize, loadSize], BILINEAR)
        if opt.resize_or_crop == 'scale_width':
            return _scale_width_size(ow, oh, opt.fineSize)
        if opt.resize_or_crop == 'scale_width_and_crop':
            return _scale_width_size(ow, oh, opt.loadSize)
        if opt.resize_or_crop != 'crop':
            raise ValueError('--resize_or_crop %s' % opt.resize_or_crop)
        return ow, oh

    def _draw(self, img, path):
        """The random draws of one image in the reference's order -> (w, h, x0, y0, flip, rot); no device work."""
        opt, n = self.opt, self.opt.fineSize
        crop = opt.resize_or_crop != 'scale_width'
        w, h = self._resized_size(*img.size)
        if crop:
            if w < n or h < n:
                raise ValueError('image %s is %dx%d after resizing, smaller than --fineSize %d' % (path, w, h, n))
            x0, y0 = random.randint(0, w - n), random.randint(0, h - n)
        else:
            if w != h:
                raise NotImplementedError('scale_width of a non-square image gives a non-square tensor; the MI355X feeder crops squares')
            x0 = y0 = 0
        flip = opt.isTrain and not opt.no_flip and random.random() < 0.5
        rot = random.randint(0, 3) if (opt.isTrain and not opt.no_rotate) else 0
        return w, h, x0, y0, flip, rot

    def _resized(self, img, w, h):
        dev = self._to_device(img)
        if (w, h) != img.size:
            dev = ops.image_resize(dev, w, h, "bilinear")      # Image.resize((w, h), BILINEAR), on the device
        return dev

    def _prep(self, img, draw, ctrl=None):
        w, h, x0, y0, flip, rot = draw
        return self._image_prep(self._resized(img, w, h), x0, y0, self.opt.fineSize, flip, rot, ctrl)


class UnalignedFolderDataset(SingleFolderDataset):
    """UnalignedDataset (data/unaligned_dataset.py:10-41): <root>/<phase>A and <root>/<phase>B, the i-th file of each (modulo its
    length), each through its own draw of the single-image transform."""

    def __init__(self, opt, device=None):
        self.opt = opt
        self.device = device if device is not None else torch.device('cuda', opt.gpu_ids[0])
        self.A_paths = sorted(make_dataset(os.path.join(opt.dataroot, opt.phase + 'A')))
        self.B_paths = sorted(make_dataset(os.path.join(opt.dataroot, opt.phase + 'B')))
        if not self.A_paths or not self.B_paths:
            raise RuntimeError('no images under %s{A,B}' % os.path.join(opt.dataroot, opt.phase))
        self.paths = list(range(max(len(self.A_paths), len(self.B_paths))))
        self.order = list(self.paths)

    def _host(self, index):
        a, b = self.A_paths[index % len(self.A_paths)], self.B_paths[index % len(self.B_paths)]
        return self._decode(a), self._decode(b)

    def _device(self, index, imgs):
        a, b = self.A_paths[index % len(self.A_paths)], self.B_paths[index % len(self.B_paths)]
        da = self._draw(imgs[0], a)                  # A's draws first, then B's (unaligned_dataset.py:32-33)
        db = self._draw(imgs[1], b)
        ca, cb = self._draw_elastic(), self._draw_elastic()      # --elastic: one field per image, after every other draw of the item
        ra, rb = self._draw_photo(), self._draw_photo()          # --photo_aug: one record per image, after both fields
        A, = self._photo([self._prep(imgs[0], da, ca)], ra)
        B, = self._photo([self._prep(imgs[1], db, cb)], rb)
        return {'A': ops.logical_view(A, 3), 'B': ops.logical_view(B, 3), 'A_paths': [a], 'B_paths': [b]}


class AlignedFolderDataset(_FolderDataset):
    """AlignedDataset (data/aligned_dataset.py:10-46): A|B side by side in one file, bicubic resize to (2 loadSize, loadSize), the
    same crop offsets and flip for both halves, no rotation."""

    def __init__(self, opt, device=None):
        assert opt.resize_or_crop == 'resize_and_crop'      # aligned_dataset.py:17
        super().__init__(opt, device)

    def _host(self, index):
        from PIL import Image
        img = Image.open(self.paths[index]).convert('RGB')
        img.load()
        return img

    def _device(self, index, AB):
        opt, path = self.opt, self.paths[index]
        w, h, n = opt.loadSize, opt.loadSize, opt.fineSize
        w_offset = random.randint(0, max(0, w - n - 1))
        h_offset = random.randint(0, max(0, h - n - 1))
        flip = (not opt.no_flip) and random.random() < 0.5
        dev = self._to_device(AB)
        if AB.size != (2 * w, h):
            dev = ops.image_resize(dev, 2 * w, h, "bicubic")   # AB.resize((loadSize * 2, loadSize), Image.BICUBIC), on the device
        ctrl = self._draw_elastic()                            # --elastic: one field for both halves, after every other draw of the item
        A = self._image_prep(dev, w_offset, h_offset, n, flip, 0, ctrl)
        B = self._image_prep(dev, w + w_offset, h_offset, n, flip, 0, ctrl)
        A, B = self._photo([A, B], self._draw_photo())         # --photo_aug: one record for both halves, its draws after the field's
        return {'A': ops.logical_view(A, 3), 'B': ops.logical_view(B, 3), 'A_paths': [path], 'B_paths': [path]}


def create_dataset(opt, device=None):
    """CreateDataLoader / CreateDataset (data/custom_dataset_data_loader.py:6-25) at batchSize 1."""
    if opt.dataset_mode == 'single':
        return SingleFolderDataset(opt, device)
    if opt.dataset_mode == 'aligned':
        return AlignedFolderDataset(opt, device)
    if opt.dataset_mode == 'unaligned':
        return UnalignedFolderDataset(opt, device)
    raise ValueError("Dataset [%s] not recognized." % opt.dataset_mode)
