"""A device-resident training set: the reference's `data/` package with everything per step moved onto the GPU (csrc/data_ops.hip).

The reference's transform chain (data/base_dataset.py:85-129) is a deterministic prefix -- convert('RGB'), the A|B split, Grayscale, the
resize -- followed by what is random per step: crop position, flip, and the partner index of unaligned data.  DeviceImageSet runs the
prefix ONCE per image on the host, with PIL itself, and keeps the result on the device as uint8 (int32 for instance maps).  DeviceLoader
then produces each batch with one cat_data_batch launch: gather by sample index, crop, horizontal flip, ToTensor + Normalize, written as the
NHWC activation `set_input` passes through untouched (ops.is_act), so neither an H2D copy of pixels nor a layout launch is left per step.

The random draws stay on the host, in the reference's calls and order, and reach the kernel as int32 codes (the arrangement of
models/image_pool.py).  The sampler is not restated either: a stock torch.utils.data.DataLoader runs over a tiny *codes dataset* whose
__getitem__(index) makes exactly the reference dataset's draws and returns the integers, with the batch_size, shuffle and num_workers the
reference passes -- shuffle order, per-iter() base seed, worker seeding and the short last batch are the installed torch's own.

    loader = DeviceLoader.aligned(opt, sorted(paths))           # next to create_dataloader(opt)
    for batch in loader:                                        # {'A', 'B', 'A_paths', 'B_paths'}, as the reference's
        model.set_input(batch); model.optimize_parameters(step)

With a captured step, `loader.fill(codes, out=step.static)` writes the batch into the graph's static inputs and GraphedStep skips its copy.

Differences from the reference, all deliberate:
  * `instance` is int32 (the reference gives int64 for mode-'L' instance maps and int32 for mode-'I' ones); downstream only compares ids.
  * unaligned / single data draw RandomCrop's and RandomHorizontalFlip's numbers as torchvision 0.8.2 makes them -- torch.randint(0, h - th + 1,
    (1,)), torch.randint(0, w - tw + 1, (1,)), neither when the sizes are equal, then torch.rand(1) < 0.5.  That sequence is written from
    memory of torchvision's source: torchvision is not a dependency here and the sequence is NOT verified against it.
  * configurations the reference itself gets wrong are refused (NotImplementedError), see _param_geometry."""
import copy
import ctypes as C
import os
import random

import numpy as np
import torch
import torch.utils.data
from PIL import Image

from . import _lib as L
from . import ops

IMAGE, LABEL, INSTANCE = 'image', 'label', 'instance'
_KIND = {IMAGE: L.DATA_IMAGE, LABEL: L.DATA_LABEL, INSTANCE: L.DATA_INT32}


# ---------------------------------------------------------------------------------------------------------------- the reference's draws
def get_params(opt, size):
    """data/base_dataset.py:63-82: three `random` calls in this order, made even where the result goes unused (scale_width, none)."""
    w, h = size
    new_h, new_w = h, w
    crop_w, crop_h = 0, 0
    if opt.preprocess == 'resize_and_crop':
        new_h = new_w = opt.load_size
        crop_h = crop_w = opt.crop_size
    elif opt.preprocess == 'scale_width_and_crop':
        new_w = opt.load_size
        new_h = opt.load_size * h // w
        crop_w = opt.crop_size
        crop_h = opt.crop_size * h // w
    x = random.randint(0, max(0, new_w - crop_w))
    y = random.randint(0, max(0, new_h - crop_h))
    flip = random.random() > 0.5
    return {'crop_pos': (x, y), 'flip': flip, 'crop_size': (crop_w, crop_h)}


def _random_crop_draws(opt, w, h):
    """RandomCrop(crop_size) then RandomHorizontalFlip() on a w x h image, torchvision 0.8.2's draws as remembered (module docstring:
    unverified) -> (x, y, flip)."""
    x = y = 0
    if 'crop' in opt.preprocess:
        th = tw = opt.crop_size
        if not (w == tw and h == th):
            y = int(torch.randint(0, h - th + 1, size=(1,)).item())
            x = int(torch.randint(0, w - tw + 1, size=(1,)).item())
    flip = False
    if not opt.no_flip:
        flip = bool(torch.rand(1) < 0.5)
    return x, y, flip


# ---------------------------------------------------------------------------------------------------------------- the deterministic prefix
def _open(item, kind):
    if isinstance(item, (str, os.PathLike)):
        return Image.open(item)
    if isinstance(item, Image.Image):
        return item
    a = np.asarray(item)
    if kind == INSTANCE and a.dtype != np.uint8:
        if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError('DeviceImageSet: an instance map is a 2-D integer array (got %s %s)' % (a.dtype, a.shape))
        return Image.fromarray(a.astype(np.int32))
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError('DeviceImageSet: arrays are uint8 [H, W] or [H, W, 3] (got %s %s)' % (a.dtype, a.shape))
    return Image.fromarray(a)


def _resize(opt, img, method):
    """The size-changing steps of get_transform, base_dataset.py:94-111 (the crop between them is the kernel's)."""
    if 'resize' in opt.preprocess:
        img = img.resize((opt.load_size, opt.load_size), method)
    elif 'scale_width' in opt.preprocess:
        ow, oh = img.size
        if ow != opt.load_size:
            img = img.resize((opt.load_size, int(opt.load_size * oh / ow)), method)
    if opt.preprocess == 'none':
        ow, oh = img.size
        h, w = int(round(oh / 4) * 4), int(round(ow / 4) * 4)
        if (h, w) != (oh, ow):
            img = img.resize((w, h), method)
    return img


def host_prefix(opt, item, kind=IMAGE, grayscale=False, side=None):
    """One item through the deterministic part of the reference's chain -> (PIL image, the size get_params / the transform was handed).
    side 'A' / 'B': that half of an aligned pair (aligned_dataset.py:42-45)."""
    img = _open(item, kind)
    if kind == IMAGE:
        img = img.convert('RGB')
        if side is not None:
            w, h = img.size
            w2 = int(w / 2)
            img = img.crop((0, 0, w2, h)) if side == 'A' else img.crop((w2, 0, w, h))
        size = img.size
        if grayscale:
            img = img.convert('L')      # transforms.Grayscale(1)
        return _resize(opt, img, Image.BICUBIC), size
    return _resize(opt, img, Image.NEAREST), img.size


def _to_array(img, kind):
    if kind == IMAGE:
        a = np.asarray(img)
        out = np.zeros((img.size[1], img.size[0], 4), dtype=np.uint8)
        if a.ndim == 2:
            out[..., 0] = a
        else:
            out[..., :3] = a
        return out
    if kind == LABEL:
        if img.mode != 'L':
            raise ValueError("DeviceImageSet: a label map is a mode-'L' image (got mode %r)" % img.mode)
        return np.array(img)
    if img.mode not in ('L', 'I', 'I;16'):
        raise ValueError("DeviceImageSet: an instance map is a mode-'L', 'I' or 'I;16' image (got mode %r)" % img.mode)
    return np.asarray(img).astype(np.int32)


class DeviceImageSet:
    """One plane of a data set after the deterministic prefix, as a single tensor on `device`: uint8 [M, H, W, 4] (RGBx, one dword per pixel, as
    metric.images.DeviceImages keeps its set) for images, uint8 [M, H, W] for label maps, int32 [M, H, W] for instance maps.  `items` are
    paths, PIL images or uint8 arrays.  Every item must come out of the prefix at one size (the reference's default collate needs the same for
    batch > 1).  `sizes[i]` is the size item i had where the reference calls get_params."""

    def __init__(self, opt, items, kind=IMAGE, grayscale=False, side=None, device=None, max_bytes=None):
        items = list(items)
        if not items:
            raise ValueError('DeviceImageSet: no items')
        if kind not in _KIND:
            raise ValueError('DeviceImageSet: kind %r' % (kind,))
        self.kind, self.channels = kind, (1 if grayscale else 3) if kind == IMAGE else 1
        self.paths = [os.fspath(it) if isinstance(it, (str, os.PathLike)) else '<memory:%d>' % i for i, it in enumerate(items)]
        self.sizes, host = [], None
        for i, item in enumerate(items):
            img, size = host_prefix(opt, item, kind, grayscale, side)
            a = _to_array(img, kind)
            if host is None:
                self.width, self.height = img.size
                self.nbytes = len(items) * a.nbytes
                if max_bytes is not None and self.nbytes > max_bytes:
                    raise ValueError('DeviceImageSet: %d %s items of %d x %d take %d bytes on the device, more than max_bytes = %d'
                                     % (len(items), kind, self.width, self.height, self.nbytes, max_bytes))
                host = torch.empty((len(items),) + a.shape, dtype=torch.int32 if kind == INSTANCE else torch.uint8)
            elif img.size != (self.width, self.height):
                raise ValueError('DeviceImageSet: item %d (%s) is %d x %d after the resize, the items before it %d x %d: a set has one size'
                                 % (i, self.paths[i], img.size[0], img.size[1], self.width, self.height))
            host[i] = torch.from_numpy(a)
            self.sizes.append(tuple(size))
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self.data = host.to(self.device)
        self.device = self.data.device      # 'cuda' -> the device it resolved to

    def __len__(self):
        return self.data.shape[0]


# ---------------------------------------------------------------------------------------------------------------- crop geometry
def _param_geometry(opt, sizes, w, h):
    """Aligned / cityscapes data (get_params + __crop, base_dataset.py:156-166) on a set whose images are w x h after the resize and had
    `sizes` where get_params is called -> (out_w, out_h, crops).  Refused, because the reference itself leaves the image there:
      * --preprocess crop: get_params returns crop_size (0, 0) and __crop cuts an empty image
      * a crop window that can leave the resized image (scale_width_and_crop: get_params' integer new_h against __scale_width's float h);
        PIL pads such a crop with black."""
    if 'crop' not in opt.preprocess:
        return w, h, False
    if opt.preprocess == 'crop':
        raise NotImplementedError("--preprocess crop on aligned / cityscapes data: the reference's get_params gives crop_size (0, 0) there and "
                                  "its __crop returns an empty image")
    out = None
    for ow, oh in sorted(set(sizes)):
        if opt.preprocess == 'resize_and_crop':
            new_w = new_h = opt.load_size
            tw = th = opt.crop_size
        else:
            new_w, new_h = opt.load_size, opt.load_size * oh // ow
            tw, th = opt.crop_size, opt.crop_size * oh // ow
        if not (w > tw or h > th):
            geo = (w, h, False)          # __crop returns the image as it is
        else:
            if tw <= 0 or th <= 0 or max(0, new_w - tw) + tw > w or max(0, new_h - th) + th > h:
                raise NotImplementedError('--preprocess %s with load_size %d, crop_size %d on %d x %d sources: the crop window get_params draws '
                                          '(up to %d + %d x %d + %d) can leave the %d x %d image the resize gives; PIL would pad it with black'
                                          % (opt.preprocess, opt.load_size, opt.crop_size, ow, oh, max(0, new_w - tw), tw, max(0, new_h - th), th, w, h))
            geo = (tw, th, True)
        if out is not None and geo != out:
            raise ValueError('sources of %s give batches of more than one size under --preprocess %s' % (sorted(set(sizes)), opt.preprocess))
        out = geo
    return out


def _random_geometry(opt, w, h):
    """Unaligned / single data: RandomCrop(crop_size) on a w x h image."""
    if 'crop' not in opt.preprocess:
        return w, h, False
    if w < opt.crop_size or h < opt.crop_size:
        raise ValueError('RandomCrop(%d) on %d x %d images: the crop is larger than the image' % (opt.crop_size, w, h))
    return opt.crop_size, opt.crop_size, True


# ---------------------------------------------------------------------------------------------------------------- the codes datasets
class _Codes(torch.utils.data.Dataset):
    """index -> int32 row [index of slot 0, of slot 1, (x, y, flip) per plane]: the draws of the reference dataset's __getitem__(index)."""

    def __init__(self, opt, n):
        self.opt, self.n = opt, n

    def __len__(self):
        return self.n


class _ParamCodes(_Codes):
    """AlignedDataset / CityscapesDataset: one get_params per sample, shared by its planes."""

    def __init__(self, opt, n, sizes, crops, planes):
        super().__init__(opt, n)
        self.sizes, self.crops, self.planes = sizes, crops, planes

    def __getitem__(self, index):
        p = get_params(self.opt, self.sizes[index])
        x, y = p['crop_pos'] if self.crops else (0, 0)
        flip = int(bool(p['flip']) and not self.opt.no_flip)
        return torch.tensor([index, index] + [int(x), int(y), flip] * self.planes, dtype=torch.int32)


class _RandomCodes(_Codes):
    """UnalignedDataset (two planes) / SingleDataset (one): random.randint for the partner unless serial_batches, then the transform's own
    draws for A and afterwards for B."""

    def __init__(self, opt, n, dims):
        super().__init__(opt, n)
        self.dims = dims        # [(M, w, h)] per plane

    def __getitem__(self, index):
        row = [index % self.dims[0][0], 0]
        if len(self.dims) == 2:
            row[1] = index % self.dims[1][0] if self.opt.serial_batches else random.randint(0, self.dims[1][0] - 1)
        for _, w, h in self.dims:
            x, y, flip = _random_crop_draws(self.opt, w, h)
            row += [x, y, int(flip)]
        return torch.tensor(row, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------- the loader
class _Plane:
    def __init__(self, key, images, slot, out_w, out_h, crops):
        self.key, self.set, self.slot, self.out_w, self.out_h, self.crops = key, images, slot, out_w, out_h, crops


class DeviceLoader:
    """The surface of the reference's CustomDatasetDataLoader that Trainer and Profiler touch -- __iter__, __len__, .dataset, load_data() --
    over DeviceImageSets.  Built by the constructors below; `mode` is the reference dataset it stands for."""
    _RING = 4       # slots of the pinned codes buffer: a slot is rewritten only after the copy that read it has run

    def __init__(self, opt, mode, planes, codes, paths):
        self.opt, self.mode, self.planes, self.dataset, self.paths = opt, mode, planes, codes, paths
        self.device = planes[0].set.device
        if any(p.set.device != self.device for p in planes):
            raise ValueError('DeviceLoader: the planes of one loader live on one device')
        self.batch_size = int(opt.batch_size)
        self.width = 2 + 3 * len(planes)
        self.dataloader = torch.utils.data.DataLoader(codes, batch_size=self.batch_size, shuffle=not opt.serial_batches,
                                                      num_workers=int(opt.num_threads))
        self.unknown = float(getattr(opt, 'input_nc', 0))
        self._dev_codes = self._pinned = None
        self._slot, self._events = 0, [None] * self._RING

    # -- constructors ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _count(opt, n):
        m = getattr(opt, 'max_dataset_size', -1)
        if m in (-1, None) or m == float('inf'):
            return n
        if not 0 < m <= n:
            raise ValueError('max_dataset_size %s with %d items' % (m, n))
        return int(m)

    @classmethod
    def aligned(cls, opt, pairs, device=None, max_bytes=None):
        """AlignedDataset: `pairs` are the A|B images of opt.dataroot/opt.phase (sorted, as the reference sorts its paths)."""
        if opt.load_size < opt.crop_size:
            raise ValueError('aligned data: load_size %d < crop_size %d' % (opt.load_size, opt.crop_size))
        pairs = list(pairs)
        pairs = pairs[:cls._count(opt, len(pairs))]
        btoa = opt.direction == 'BtoA'
        nc_a, nc_b = (opt.output_nc, opt.input_nc) if btoa else (opt.input_nc, opt.output_nc)
        a = DeviceImageSet(opt, pairs, IMAGE, nc_a == 1, 'A', device, max_bytes)
        b = DeviceImageSet(opt, pairs, IMAGE, nc_b == 1, 'B', device, None if max_bytes is None else max_bytes - a.nbytes)
        planes = [_Plane(k, s, 0, *_param_geometry(opt, a.sizes, s.width, s.height)) for k, s in (('A', a), ('B', b))]
        if planes[0].crops != planes[1].crops:
            raise ValueError('aligned data: one side of the pairs is cropped and the other is not')
        codes = _ParamCodes(opt, len(pairs), a.sizes, planes[0].crops, 2)
        return cls(opt, 'aligned', planes, codes, {'A_paths': (0, a.paths), 'B_paths': (0, a.paths)})

    @classmethod
    def unaligned(cls, opt, A, B, device=None, max_bytes=None):
        """UnalignedDataset: the images of opt.dataroot/opt.phase + 'A' and + 'B' (sorted); its length is the larger set's."""
        btoa = opt.direction == 'BtoA'
        nc_a, nc_b = (opt.output_nc, opt.input_nc) if btoa else (opt.input_nc, opt.output_nc)
        a = DeviceImageSet(opt, A, IMAGE, nc_a == 1, None, device, max_bytes)
        b = DeviceImageSet(opt, B, IMAGE, nc_b == 1, None, device, None if max_bytes is None else max_bytes - a.nbytes)
        planes = [_Plane(k, s, i, *_random_geometry(opt, s.width, s.height)) for i, (k, s) in enumerate((('A', a), ('B', b)))]
        codes = _RandomCodes(opt, max(len(a), len(b)), [(len(s), s.width, s.height) for s in (a, b)])
        return cls(opt, 'unaligned', planes, codes, {'A_paths': (0, a.paths), 'B_paths': (1, b.paths)})

    @classmethod
    def single(cls, opt, A, device=None, max_bytes=None):
        """SingleDataset: batches hold 'A' and 'A_paths' only."""
        A = list(A)
        A = A[:cls._count(opt, len(A))]
        nc = opt.output_nc if opt.direction == 'BtoA' else opt.input_nc
        a = DeviceImageSet(opt, A, IMAGE, nc == 1, None, device, max_bytes)
        planes = [_Plane('A', a, 0, *_random_geometry(opt, a.width, a.height))]
        codes = _RandomCodes(opt, len(a), [(len(a), a.width, a.height)])
        return cls(opt, 'single', planes, codes, {'A_paths': (0, a.paths)})

    @classmethod
    def cityscapes(cls, opt, labels, images, instances=None, device=None, max_bytes=None):
        """CityscapesDataset: label / image / instance files in matching (naturally sorted) order; `instances` None = --no_instance, the
        batch's 'instance' is then the collated 0 of the reference."""
        labels, images = list(labels), list(images)
        if len(labels) != len(images) or (instances is not None and len(list(instances)) != len(labels)):
            raise ValueError('cityscapes data: as many images (and instance maps) as label maps')
        n = cls._count(opt, len(labels))
        left = max_bytes
        sets = []
        for kind, items in ((LABEL, labels), (IMAGE, images), (INSTANCE, instances)):
            if items is None:
                continue
            s = DeviceImageSet(opt, list(items)[:n], kind, False, None, device, left)
            left = None if left is None else left - s.nbytes
            sets.append((kind, s))
        lab = sets[0][1]
        geo = _param_geometry(opt, lab.sizes, lab.width, lab.height)
        for kind, s in sets:
            if (s.width, s.height) != (lab.width, lab.height):
                raise ValueError('cityscapes data: %s maps are %d x %d after the resize, label maps %d x %d' % (kind, s.width, s.height, lab.width, lab.height))
        planes = [_Plane(kind, s, 0, *geo) for kind, s in sets]
        codes = _ParamCodes(opt, n, lab.sizes, geo[2], len(planes))
        return cls(opt, 'cityscapes', planes, codes, {'path': (0, sets[1][1].paths)})

    # -- the reference loader's surface ------------------------------------------------------------------------------------------------
    def load_data(self):
        return self

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        for codes in self.dataloader:
            yield self.fill(codes)

    # -- one batch ---------------------------------------------------------------------------------------------------------------------
    def validate(self, codes):
        """The codes of one batch, checked on the host before they travel: the kernel never sees an index or a window outside a set."""
        codes = torch.as_tensor(codes, dtype=torch.int32)
        if codes.dim() != 2 or codes.shape[1] != self.width or codes.device.type != 'cpu':
            raise ValueError('DeviceLoader: codes are a host int32 [n, %d] tensor (got %s)' % (self.width, tuple(codes.shape)))
        for i, p in enumerate(self.planes):
            idx, (x, y, flip) = codes[:, p.slot], codes[:, 2 + 3 * i:5 + 3 * i].unbind(1)
            ok = (idx >= 0) & (idx < len(p.set)) & (x >= 0) & (x <= p.set.width - p.out_w) & (y >= 0) & (y <= p.set.height - p.out_h) & \
                (flip >= 0) & (flip <= 1)
            if not bool(ok.all()):
                raise ValueError('DeviceLoader: codes outside plane %r (%d images of %d x %d, crop %d x %d): %s'
                                 % (p.key, len(p.set), p.set.width, p.set.height, p.out_w, p.out_h, codes[~ok].tolist()))
        return codes

    def upload(self, codes):
        """Validate one batch's codes and send them to the loader's device buffer (what a captured launch reads) -> the validated codes.  One
        pinned host buffer, one non-blocking copy, no synchronisation: a slot of the pinned ring is only waited for if the copy issued _RING
        batches ago has not run yet."""
        codes = self.validate(codes)
        n = codes.shape[0]
        if n > self.batch_size:
            raise ValueError('DeviceLoader: %d samples in a batch of at most %d' % (n, self.batch_size))
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('DeviceLoader.upload: codes are uploaded before a replay, not inside a capture')
        if self._dev_codes is None:
            self._dev_codes = torch.zeros((self.batch_size, self.width), dtype=torch.int32, device=self.device)
            self._pinned = torch.zeros((self._RING, self.batch_size, self.width), dtype=torch.int32).pin_memory()
        k = self._slot
        self._slot = (k + 1) % self._RING
        if self._events[k] is not None:
            self._events[k].synchronize()
        self._pinned[k, :n].copy_(codes)
        with torch.cuda.device(self.device):
            self._dev_codes[:n].copy_(self._pinned[k, :n], non_blocking=True)
            ev = self._events[k] = self._events[k] or torch.cuda.Event()
            ev.record()
        return codes

    def _buffers(self, n, out):
        bufs = {}
        for p in self.planes:
            t = None if out is None else out.get(p.key)
            shape = (n, p.set.channels, p.out_h, p.out_w)
            if t is not None and torch.is_tensor(t) and tuple(t.shape) == shape and t.device == self.device:
                if p.set.kind == IMAGE and not ops.is_act(t):
                    raise ValueError('DeviceLoader.fill: out[%r] must be an NHWC float32 activation (strides %s)' % (p.key, t.stride()))
                if p.set.kind != IMAGE and not (t.is_contiguous() and t.dtype == (torch.float32 if p.set.kind == LABEL else torch.int32)):
                    raise ValueError('DeviceLoader.fill: out[%r] must be a contiguous %s tensor' % (p.key, 'float32' if p.set.kind == LABEL else 'int32'))
            elif p.set.kind == IMAGE:        # no buffer, or one of another batch size (the short last batch): a fresh tensor
                t = ops.empty_act(n, p.set.channels, p.out_h, p.out_w, self.device)
            else:
                t = torch.empty(shape, dtype=torch.float32 if p.set.kind == LABEL else torch.int32, device=self.device)
            bufs[p.key] = t
        return bufs

    def launch(self, n, out=None):
        """The one cat_data_batch launch of a batch of n samples from the codes `upload` left on the device -> {key: tensor}.  Capturable: a
        graph replays it with whatever codes were uploaded before the replay."""
        if self._dev_codes is None:
            raise RuntimeError('DeviceLoader.launch: no codes were uploaded yet (the first upload allocates; it cannot happen inside a capture)')
        bufs = self._buffers(n, out)
        t = L.DataBatch()
        t.planes, t.N, t.unknown = len(self.planes), n, self.unknown
        for i, p in enumerate(self.planes):
            d, dst = t.plane[i], bufs[p.key]
            d.src, d.dst = p.set.data.data_ptr(), dst.data_ptr()
            d.M, d.H, d.W, d.Hc, d.Wc = len(p.set), p.set.height, p.set.width, p.out_h, p.out_w
            d.kind, d.C, d.slot = _KIND[p.set.kind], p.set.channels, p.slot
            d.cs = ops.act_cs(dst) if p.set.kind == IMAGE else 0
        with torch.cuda.device(self.device):
            L.call('cat_data_batch', C.byref(t), ops._p(self._dev_codes), ops._stream())
        return bufs

    def fill(self, codes, out=None):
        """codes (host int32 [n, 2 + 3 * planes], a batch of the codes dataset) -> the batch dict with the reference's keys.  `out`: a dict of
        preallocated buffers (GraphedStep.static); a plane whose buffer has this batch's shape is written there and that tensor is returned,
        otherwise (no buffer, or the short last batch) a fresh one.  Inside a graph capture nothing is uploaded (a capture records and does not
        execute): the launch is recorded, and `upload` feeds every replay."""
        codes = self.validate(codes) if torch.cuda.is_current_stream_capturing() else self.upload(codes)
        n = codes.shape[0]
        batch = self.launch(n, out)
        for key, (slot, paths) in self.paths.items():
            batch[key] = [paths[i] for i in codes[:, slot].tolist()]
        if self.mode == 'cityscapes' and INSTANCE not in batch:
            batch[INSTANCE] = torch.zeros(n, dtype=torch.int64)      # the default collate of --no_instance's `0`
        return batch


def eval_loader(opt, *sources, **kw):
    """create_eval_dataloader (data/__init__.py:50-65): load_size = crop_size, no_flip, serial_batches, batch_size = eval_batch_size, and the
    `single` dataset for unaligned data (`sources` are then the images of val<direction[0]>).  Otherwise the sources of opt.dataset_mode's
    constructor."""
    opt = copy.deepcopy(opt)
    opt.load_size = opt.crop_size
    opt.no_flip = True
    opt.serial_batches = True
    opt.batch_size = opt.eval_batch_size
    opt.phase = 'val'
    if opt.dataset_mode == 'unaligned':
        opt.dataset_mode = 'single'
    make = {'aligned': DeviceLoader.aligned, 'single': DeviceLoader.single, 'cityscapes': DeviceLoader.cityscapes}.get(opt.dataset_mode)
    if make is None:
        raise NotImplementedError('eval_loader: dataset_mode %r' % (opt.dataset_mode,))
    return make(opt, *sources, **kw)
