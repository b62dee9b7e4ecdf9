"""What feeding a step costs: the host path (the reference's per-sample PIL chain under a stock DataLoader, the H2D copy and set_input's layout
launch -- the path at this commit's parent) against the device path (cat_amd.data.DeviceLoader: one cat_data_batch launch per batch).

Two configurations:
  pix2pix   the inception distillation step of bench.py (workload c2) at 256 x 256, batch 16, fed from 286 x 286 aligned pairs (resize_and_crop)
  gaugan    the GauGAN distillation step of bench.py (workload spade) at 512 x 256, batch 4, fed from 2048 x 1024 synthetic label / image /
            instance sources held in memory (scale_width 512), the reference's --load_in_memory arrangement
For each:
  (a) ms per batch of the feed ALONE (batch on the device and through set_input, no step): host path with num_workers 0 and 4, device path;
      median over three epochs of 48 batches
  (b) images/s of the captured step (cat_amd.graph.GraphedStep) when fed each way, the ways alternating in one process, median of three rounds
      of one epoch each.
Both are taken from the first batch of an epoch on and end in a device synchronise; the time to the first batch -- the DataLoader's start-up, which
with workers is the start of the worker processes, paid once per epoch -- is reported beside them (startup_ms).  The sources are 128 pairs / 16
label-image-instance triples, repeated to 48 batches per epoch.
The PIL chain is restated here (HostAligned / HostCityscapes); nothing is read from the reference.

    python tools/data_feed_bench.py [--configs pix2pix gaugan] [--workers 0 4] [--out FILE]

The driver starts one child process per configuration, each under its own `timeout`, and stops at the first one that fails; at most 8 loader
workers.  One JSON line per configuration, printed and written to --out."""
import argparse
import json
import os
import random
import statistics
import subprocess
import sys
import time
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.utils.data  # noqa: E402
from PIL import Image  # noqa: E402

MAX_WORKERS = 8
CHILD_LIMIT_S = {'pix2pix': 420, 'gaugan': 540}


def data_opt(**kw):
    opt = Namespace(preprocess='resize_and_crop', load_size=286, crop_size=256, no_flip=False, serial_batches=False, batch_size=1, num_threads=0,
                    direction='AtoB', input_nc=3, output_nc=3, max_dataset_size=-1, dataset_mode='aligned', no_instance=False, phase='train')
    opt.__dict__.update(kw)
    return opt


# ---------------------------------------------------------------------------------------------------------------- the host chain, restated
def _to_tensor(img):
    a = np.array(img)
    a = a[:, :, None] if a.ndim == 2 else a
    return torch.from_numpy(a).permute(2, 0, 1).float().div(255)


def _scale(opt, img, method):
    if 'resize' in opt.preprocess:
        return img.resize((opt.load_size, opt.load_size), method)
    ow, oh = img.size
    return img if ow == opt.load_size else img.resize((opt.load_size, int(opt.load_size * oh / ow)), method)


def _crop_flip(opt, img, p):
    if 'crop' in opt.preprocess:
        (x, y), (tw, th) = p['crop_pos'], p['crop_size']
        if img.size[0] > tw or img.size[1] > th:
            img = img.crop((x, y, x + tw, y + th))
    return img.transpose(Image.FLIP_LEFT_RIGHT) if (p['flip'] and not opt.no_flip) else img


class HostAligned(torch.utils.data.Dataset):
    def __init__(self, opt, pairs):
        self.opt, self.pairs = opt, pairs

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, index):
        from cat_amd.data import get_params
        AB = self.pairs[index].convert('RGB')
        w, h = AB.size
        A, B = AB.crop((0, 0, int(w / 2), h)), AB.crop((int(w / 2), 0, w, h))
        p = get_params(self.opt, A.size)
        f = lambda img: _to_tensor(_crop_flip(self.opt, _scale(self.opt, img, Image.BICUBIC), p)).sub(0.5).div(0.5)
        return {'A': f(A), 'B': f(B), 'A_paths': str(index), 'B_paths': str(index)}


class HostCityscapes(torch.utils.data.Dataset):
    def __init__(self, opt, labels, images, instances):
        self.opt, self.labels, self.images, self.instances = opt, labels, images, instances

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, index):
        from cat_amd.data import get_params
        opt = self.opt
        p = get_params(opt, self.labels[index].size)
        lab = _to_tensor(_crop_flip(opt, _scale(opt, self.labels[index], Image.NEAREST), p)) * 255.0
        lab[lab == 255] = opt.input_nc
        img = _to_tensor(_crop_flip(opt, _scale(opt, self.images[index].convert('RGB'), Image.BICUBIC), p)).sub(0.5).div(0.5)
        ins = torch.from_numpy(np.array(_crop_flip(opt, _scale(opt, self.instances[index], Image.NEAREST), p)).astype(np.int32))[None]
        return {'label': lab, 'instance': ins, 'image': img, 'path': str(index)}


def host_loader(opt, dataset, workers):
    return torch.utils.data.DataLoader(dataset, batch_size=opt.batch_size, shuffle=not opt.serial_batches, num_workers=workers)


# ---------------------------------------------------------------------------------------------------------------- sources and models
def _sources(cfg):
    rs = np.random.RandomState(7)
    if cfg == 'pix2pix':
        opt = data_opt(batch_size=16)
        pairs = [Image.fromarray(rs.randint(0, 256, size=(286, 572, 3), dtype=np.uint8)) for _ in range(128)] * 6
        return opt, (pairs,)
    opt = data_opt(dataset_mode='cityscapes', preprocess='scale_width', load_size=512, crop_size=512, batch_size=4, input_nc=35, direction='BtoA')
    up = lambda a: np.repeat(np.repeat(a, 64, 0), 64, 1)
    labels = [Image.fromarray(up(rs.randint(0, 35, size=(16, 32))).astype(np.uint8)) for _ in range(16)]
    instances = [Image.fromarray(up(rs.randint(0, 1000, size=(16, 32))).astype(np.int32)) for _ in range(16)]
    images = [Image.fromarray(rs.randint(0, 256, size=(1024, 2048, 3), dtype=np.uint8)) for _ in range(16)]
    return opt, (labels * 12, images * 12, instances * 12)


def _model(cfg):
    import bench
    if cfg == 'pix2pix':
        return bench.build_model(Namespace(workload='c2', target_flops=4.6e9, size=256, batch=16), 0)[0]
    return bench.build_spade_model(Namespace(workload='spade', target_flops=5.6e9, size=256, batch=4), 0)[0]


def _device_loader(cfg, opt, sources):
    from cat_amd.data import DeviceLoader
    return DeviceLoader.aligned(opt, *sources) if cfg == 'pix2pix' else DeviceLoader.cityscapes(opt, *sources)


def _host_set(cfg, opt, sources):
    return HostAligned(opt, *sources) if cfg == 'pix2pix' else HostCityscapes(opt, *sources)


def _epoch(batches, consume):
    """One pass over `batches` -> (ms until the first batch was consumed: the DataLoader's start-up, worker processes included; ms per batch over
    the rest, ending in a device synchronise; samples per second over the rest)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t1, k, n = None, 0, 0
    for b in batches:
        got = consume(b)
        if t1 is None:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        else:
            k, n = k + 1, n + got
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1) / k, n / (t2 - t1)


def child(cfg, workers, epochs, rounds):
    from cat_amd import _lib
    from cat_amd.graph import GraphedStep
    _lib.load()
    torch.cuda.set_device(0)
    random.seed(233)
    torch.manual_seed(233)
    opt, sources = _sources(cfg)
    host_set = _host_set(cfg, opt, sources)
    dev = _device_loader(cfg, opt, sources)
    row = {'config': cfg, 'batch': opt.batch_size, 'items': len(host_set), 'batches_per_epoch': len(dev),
           'device_set_bytes': sum(p.set.nbytes for p in dev.planes), 'feed': {}, 'step': {}}
    ways = ['host_w%d' % w for w in workers] + ['device']
    host_loaders = {'host_w%d' % w: host_loader(opt, host_set, w) for w in workers}
    size = lambda batch: len(batch['path' if cfg == 'gaugan' else 'A_paths'])

    # (a) the feed alone: every batch lands on the device and goes through set_input
    model = _model(cfg)

    def feed(batch):
        model.set_input(batch)
        return size(batch)
    for name in ways:
        batches = lambda: dev if name == 'device' else host_loaders[name]
        _epoch(batches(), feed)      # first epoch: allocator, lazy state
        runs = [_epoch(batches(), feed) for _ in range(epochs)]
        row['feed'][name] = {'startup_ms': [round(r[0], 1) for r in runs], 'ms_per_batch': [round(r[1], 3) for r in runs],
                             'median_ms_per_batch': round(statistics.median(r[1] for r in runs), 3)}
        print('[%s] feed %s: %s' % (cfg, name, row['feed'][name]), file=sys.stderr, flush=True)

    # (b) the captured step fed each way: one model and one capture per way (the static inputs differ: NCHW copies against in-place fills)
    host_model, dev_model = model, _model(cfg)
    example_host = next(iter(host_loader(opt, host_set, 0)))
    host_step = GraphedStep(host_model, {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in example_host.items()})
    dev_step = GraphedStep(dev_model, next(iter(dev)))

    def host_fed(batch):
        host_step(batch)
        return size(batch)

    def dev_fed(codes):
        dev_step(dev.fill(codes, out=dev_step.static))
        return codes.shape[0]
    one = lambda name: _epoch(dev.dataloader, dev_fed) if name == 'device' else _epoch(host_loaders[name], host_fed)
    got = {name: [] for name in ways}
    for name in ways:
        one(name)
    for _ in range(rounds):
        for name in ways:
            got[name].append(one(name))
    for name in ways:
        row['step'][name] = {'startup_ms': [round(r[0], 1) for r in got[name]], 'images_per_s': [round(r[2], 2) for r in got[name]],
                             'median_images_per_s': round(statistics.median(r[2] for r in got[name]), 2)}
    assert host_step.replays > 0 and dev_step.replays > 0
    for m in (host_model, dev_model):
        losses = m.get_current_losses()
        assert losses and all(v == v for v in losses.values()), losses
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', nargs='+', default=['pix2pix', 'gaugan'], choices=['pix2pix', 'gaugan'])
    ap.add_argument('--workers', type=int, nargs='+', default=[0, 4])
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'data_feed_bench.txt'))
    ap.add_argument('--child', default=None, choices=['pix2pix', 'gaugan'])
    args = ap.parse_args()
    if any(not 0 <= w <= MAX_WORKERS for w in args.workers):
        raise SystemExit('at most %d loader workers' % MAX_WORKERS)
    if args.child:
        return child(args.child, args.workers, args.epochs, args.rounds)
    lines = []
    for cfg in args.configs:
        cmd = ['timeout', '-k', '10', str(CHILD_LIMIT_S[cfg]), sys.executable, os.path.abspath(__file__), '--child', cfg, '--workers'] + \
              [str(w) for w in args.workers] + ['--epochs', str(args.epochs), '--rounds', str(args.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit('%s ended with status %d: nothing more is started' % (cfg, r.returncode))
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
