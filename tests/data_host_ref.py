"""Test-local host data sets for tests/test_data_*.py: the reference's per-sample chain written out with PIL and torch on the CPU --
Image.crop, transpose(FLIP_LEFT_RIGHT), torch.from_numpy(...).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5) -- over synthetic images.
The draws come from cat_amd.data.get_params (pinned to the reference's by tests/test_data_host.py) and, for unaligned data, from the same
torch.randint / torch.rand sequence cat_amd.data documents (not verified against torchvision: no test claims that parity)."""
import random
from argparse import Namespace

import numpy as np
import torch
import torch.utils.data
from PIL import Image


def data_opt(**kw):
    """The data options the reference's loaders read, at their base_options defaults."""
    opt = Namespace(preprocess='resize_and_crop', load_size=286, crop_size=256, no_flip=False, serial_batches=False, batch_size=1, num_threads=0,
                    direction='AtoB', input_nc=3, output_nc=3, max_dataset_size=-1, eval_batch_size=1, dataset_mode='aligned', no_instance=False,
                    phase='train')
    opt.__dict__.update(kw)
    return opt


def rgb(w, h, seed):
    """A w x h RGB image of seeded noise (every pixel distinct enough that a wrong offset or a missed flip shows)."""
    return Image.fromarray(np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8))


def to_tensor(img):
    """ToTensor of an RGB or L image: uint8 HWC -> float32 CHW / 255"""
    a = np.array(img)
    a = a[:, :, None] if a.ndim == 2 else a
    return torch.from_numpy(a).permute(2, 0, 1).float().div(255)


def normalize(t):
    return t.sub(0.5).div(0.5)


def resize(opt, img, method):
    if 'resize' in opt.preprocess:
        return img.resize((opt.load_size, opt.load_size), method)
    if 'scale_width' in opt.preprocess:
        ow, oh = img.size
        return img if ow == opt.load_size else img.resize((opt.load_size, int(opt.load_size * oh / ow)), method)
    if opt.preprocess == 'none':
        ow, oh = img.size
        h, w = int(round(oh / 4) * 4), int(round(ow / 4) * 4)
        return img if (h, w) == (oh, ow) else img.resize((w, h), method)
    return img


def crop_flip(opt, img, params):
    """__crop and __flip of base_dataset.py with get_params' result"""
    if 'crop' in opt.preprocess:
        (x, y), (tw, th) = params['crop_pos'], params['crop_size']
        if img.size[0] > tw or img.size[1] > th:
            img = img.crop((x, y, x + tw, y + th))
    if not opt.no_flip and params['flip']:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return img


class HostAligned(torch.utils.data.Dataset):
    def __init__(self, opt, pairs, names):
        from cat_amd import data
        self.opt, self.pairs, self.names, self.get_params = opt, pairs, names, data.get_params

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, index):
        opt = self.opt
        AB = self.pairs[index].convert('RGB')
        w, h = AB.size
        w2 = int(w / 2)
        A, B = AB.crop((0, 0, w2, h)), AB.crop((w2, 0, w, h))
        params = self.get_params(opt, A.size)
        out = {}
        for key, img, nc in (('A', A, opt.input_nc), ('B', B, opt.output_nc)):
            img = img.convert('L') if nc == 1 else img
            out[key] = normalize(to_tensor(crop_flip(opt, resize(opt, img, Image.BICUBIC), params)))
        out['A_paths'] = out['B_paths'] = self.names[index]
        return out


class HostUnaligned(torch.utils.data.Dataset):
    def __init__(self, opt, A, B, names_a, names_b):
        self.opt, self.A, self.B, self.names_a, self.names_b = opt, A, B, names_a, names_b
        self.positions = []      # (index, (xA, yA), (xB, yB)) in draw order

    def __len__(self):
        return max(len(self.A), len(self.B))

    def _transform(self, img):
        opt = self.opt
        img = resize(opt, img.convert('RGB'), Image.BICUBIC)
        pos = (0, 0)
        if 'crop' in opt.preprocess:
            w, h = img.size
            t = opt.crop_size
            if not (w == t and h == t):
                y = int(torch.randint(0, h - t + 1, size=(1,)).item())
                x = int(torch.randint(0, w - t + 1, size=(1,)).item())
                pos = (x, y)
                img = img.crop((x, y, x + t, y + t))
        if not opt.no_flip and bool(torch.rand(1) < 0.5):
            img = img.transpose(Image.FLIP_LEFT_RIGHT)
        return normalize(to_tensor(img)), pos

    def __getitem__(self, index):
        ia = index % len(self.A)
        ib = index % len(self.B) if self.opt.serial_batches else random.randint(0, len(self.B) - 1)
        A, pa = self._transform(self.A[ia])
        out = {'A': A, 'A_paths': self.names_a[ia]}
        if self.B:
            out['B'], pb = self._transform(self.B[ib])
            out['B_paths'] = self.names_b[ib]
            self.positions.append((index, pa, pb))
        return out


class HostSingle(HostUnaligned):
    def __init__(self, opt, A, names):
        super().__init__(opt, A, [], names, [])

    def __len__(self):
        return len(self.A)

    def __getitem__(self, index):
        A, _ = self._transform(self.A[index])
        return {'A': A, 'A_paths': self.names_a[index]}


class HostCityscapes(torch.utils.data.Dataset):
    def __init__(self, opt, labels, images, instances, names):
        from cat_amd import data
        self.opt, self.labels, self.images, self.instances, self.names, self.get_params = opt, labels, images, instances, names, data.get_params

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, index):
        opt = self.opt
        label = self.labels[index]
        params = self.get_params(opt, label.size)
        lab = to_tensor(crop_flip(opt, resize(opt, label, Image.NEAREST), params)) * 255.0
        lab[lab == 255] = opt.input_nc
        image = normalize(to_tensor(crop_flip(opt, resize(opt, self.images[index].convert('RGB'), Image.BICUBIC), params)))
        inst = crop_flip(opt, resize(opt, self.instances[index], Image.NEAREST), params)
        inst = torch.from_numpy(np.asarray(inst).astype(np.int32))[None]      # ToTensor of a mode-'I' image: int32 [1, H, W]
        return {'label': lab, 'instance': inst, 'image': image, 'path': self.names[index]}


def host_batches(opt, dataset):
    """The reference's own loader construction (data/__init__.py:82-86) over a host data set"""
    return list(torch.utils.data.DataLoader(dataset, batch_size=opt.batch_size, shuffle=not opt.serial_batches, num_workers=int(opt.num_threads)))


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)


class Launches:
    """Profiler-free launch log, as in tests/test_pretrained_gpu.py: wraps cat_amd._lib.call (every module reaches it as an attribute of _lib)
    while active and records the entry-point names."""

    def __init__(self):
        from cat_amd import _lib
        _lib.load()
        self.lib, self.names = _lib, []

    def __enter__(self):
        real = self.real = self.lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.real
