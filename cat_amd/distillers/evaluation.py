"""`evaluate_model` on the GPU (reference distillers/inception_distiller.py:204-281,
distillers/spade_distiller.py:96-180).

The generator passes run on the HIP kernels (`model.test()` with the student in eval mode: BatchNorm students take the frozen-block
fusion of cat_amd/frozen.py); images of the first 10 samples (or all) are written like the reference does.

FID (round 5): the InceptionV3 pool3 feature extractor runs on the HIP kernels too (cat_amd.metric.InceptionV3, cat_amd.metric.get_fid --
reference metric/inception.py, metric/fid_score.py:152-216, metric/__init__.py:11-21).  `attach_fid(model, checkpoint, real_stat_path)`
builds it exactly as the reference's __init__ does (base_inception_distiller.py:218-234: `InceptionV3([block_idx])`, `np.load(real_stat_path)`)
from the torchvision-keyed FID checkpoint the reference downloads; a model that carries `inception_model` + `npz` needs no `fid_fn`.
mIoU: the cityscapes segmentation network (DRN-D-105 + head) and the resize / argmax / confusion-matrix tail run on the HIP kernels as well
(cat_amd.metric.DRNSeg, cat_amd.metric.get_mIoU -- reference metric/drn.py, metric/mIoU_score.py, metric/__init__.py:24-46).
`attach_miou(model, checkpoint, table_path, data_dir)` does what the reference's __init__ does (base_inception_distiller.py:226-232,
base_spade_distiller.py:166-170: `DRNSeg('drn_d_105', 19, pretrained=False)` + `load_network(..., opt.drn_path)`); a model that carries
`drn_model` needs no `miou_fn`.  An attached

    model.miou_fn = lambda fakes, names: ...

(`fakes` is the reference's list of NCHW CPU tensors, one per eval batch) still wins.  Either way the reference's bookkeeping comes back:
`is_best`, `best_fid / best_mIoU`, the 3-evaluation running means and the `metric/*` dict that `Trainer` logs.

The teacher models evaluate through the same loop (models/pix2pix_model.py, models/cycle_gan_model.py: `evaluate`'s keyword arguments name
their loaders, attributes and metric keys).  `model.eval_images = 'device'` keeps the generated set on the GPU as uint8
(cat_amd.metric.DeviceImages, csrc/image_ops.hip) whenever every metric of the evaluation is the package's own; the image dumps then come
from the same quantise kernel (`image_of`) and only uint8 crosses to the host."""
import ntpath
import os

import numpy as np
import torch


def tensor2im(t):
    """[-1, 1] CHW tensor -> HWC uint8 (reference utils/util.py:58-88; truncating cast, like numpy's astype)."""
    a = t.detach().cpu().float().numpy()
    if a.ndim == 2:
        a = a[None]
    a = np.clip((np.transpose(a, (1, 2, 0)) + 1) / 2.0 * 255.0, 0, 255)
    if a.shape[2] == 1:
        a = a[:, :, 0]
    return a.astype(np.uint8)


def label_colormap(n):
    """The bit-interleaved colour table the reference uses for n != 35 labels (utils/util.py:176-188): label i -> id = i + 1, the
    low three bits of successive octal digits of id go to the high bits of r, g, b."""
    cmap = np.zeros((n, 3), dtype=np.uint8)
    for i in range(n):
        ident, r, g, b = i + 1, 0, 0, 0
        for j in range(7):
            r ^= (ident & 1) << (7 - j)
            g ^= ((ident >> 1) & 1) << (7 - j)
            b ^= ((ident >> 2) & 1) << (7 - j)
            ident >>= 3
        cmap[i] = (r, g, b)
    return cmap


def tensor2label(t, n_label):
    """One-hot (or index) CHW label tensor -> colour image (reference utils/util.py:90-115)."""
    t = t.detach().cpu().float()
    idx = t.max(0)[1] if t.shape[0] > 1 else t[0].long()
    cmap = label_colormap(n_label)
    out = np.zeros(tuple(idx.shape) + (3,), dtype=np.uint8)
    valid = (idx >= 0) & (idx < n_label)
    out[valid.numpy()] = cmap[idx[valid].numpy()]
    return out


def save_image(arr, path):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if arr.ndim == 2:
        arr = np.repeat(arr[:, :, None], 3, 2)
    Image.fromarray(arr).save(path.replace('.jpg', '.png'))


def _track(model, value, best_attr, hist_attr, better, is_best='is_best'):
    """best value + is_best + running mean of the last 3 evaluations (inception_distiller.py:251-256, 271-276)."""
    if better(value, getattr(model, best_attr)):
        setattr(model, is_best, True)
        setattr(model, best_attr, value)
    hist = getattr(model, hist_attr)
    hist.append(value)
    if len(hist) > 3:
        hist.pop(0)
    return sum(hist) / len(hist)


def attach_fid(model, state_dict, real_stat_path=None, npz=None, dims=2048, frechet='host'):
    """What the reference's distiller __init__ does for FID (base_inception_distiller.py:218-234), with the feature extractor on the HIP kernels:
    `state_dict` = the torchvision-keyed FID checkpoint (pt_inception-2015-12-05-6726825d.pth, or a path to it); `real_stat_path` = the
    dataset's precomputed {'mu', 'sigma'} file.  frechet='device' (opt-in): the Frechet distance runs on the GPU in float64 as well
    (metric.get_fid(..., frechet='device')); the real set's mu and sigma are uploaded here, once."""
    if frechet not in ('host', 'device'):
        raise ValueError("attach_fid: frechet must be 'host' or 'device' (got %r)" % (frechet,))
    from ..metric.features import load_inception
    if dims != 2048:      # metric.get_fid compares pool3 features with the dataset's 2048-wide {mu, sigma} (metric/__init__.py:11-21)
        raise ValueError('attach_fid: the FID path uses the 2048-wide pool3 features (dims=%r)' % (dims,))
    model.inception_model = net = load_inception(dims, state_dict, model.device, 'FID')
    model.npz = npz if npz is not None else np.load(real_stat_path)
    model.fid_frechet = frechet
    if frechet == 'device':
        model.npz_device = {k: torch.from_numpy(np.ascontiguousarray(model.npz[k], dtype=np.float64)).to(model.device) for k in ('mu', 'sigma')}
        model.fid_cache = {}
    return net


def attach_miou(model, state_dict, table_path=None, data_dir=None):
    """What the reference's distiller __init__ does for the cityscapes mIoU (base_inception_distiller.py:226-232, base_spade_distiller.py:166-170),
    with the network on the HIP kernels: `state_dict` = the reference's `--drn_path` checkpoint (DRNSeg('drn_d_105', 19) keys), or a path to
    it; table_path / data_dir default to `opt.table_path` / `opt.cityscapes_path` at evaluation time."""
    from ..metric import DRNSeg
    if isinstance(state_dict, (str, bytes, os.PathLike)):
        state_dict = torch.load(state_dict, map_location='cpu')
    net = DRNSeg('drn_d_105', 19, pretrained=False)
    net.load_state_dict(state_dict)
    model.drn_model = net.to(model.device).eval()
    model.miou_table_path, model.miou_data_dir = table_path, data_dir
    return net


def image_of(model, t):
    """tensor2im of one sample for the image dumps.  A model with eval_images == 'device' quantises a device tensor with the kernel that
    fills the DeviceImages set (cat_image_quantize: the same bytes), so only uint8 crosses to the host; everything else is tensor2im."""
    if getattr(model, 'eval_images', 'host') == 'device' and isinstance(t, torch.Tensor) and t.is_cuda:
        from ..metric import images
        return images.tensor2im(t)
    return tensor2im(t)


def _builtin(fn):
    fn.cat_builtin = True      # evaluate keeps its own callables in model.fid_fn / model.miou_fn: the mark tells them from an attached one
    return fn


def _fid_callable(model, npz):
    """(fid_fn, built_in): an attached model.fid_fn wins; otherwise the reference's own call get_fid(fakes, self.inception_model, self.npz,
    ...) (inception_distiller.py:246-249) on cat_amd.metric, `npz` naming the attribute that holds the real set's statistics."""
    fn = getattr(model, 'fid_fn', None)
    if fn is not None and not getattr(fn, 'cat_builtin', False):
        return fn, False
    if getattr(model, 'inception_model', None) is None or getattr(model, npz, None) is None:
        raise RuntimeError('evaluate_model: call evaluation.attach_fid(model, fid_checkpoint, real_stat_path) or attach model.fid_fn '
                           '(cat_amd/distillers/evaluation.py)')
    from .. import metric
    if getattr(model, 'fid_frechet', 'host') == 'device':
        cache = model.fid_cache if npz == 'npz' else model.fid_cache.setdefault(npz, {})
        fn = lambda fakes: metric.get_fid(fakes, model.inception_model, getattr(model, npz + '_device'), device=model.device,      # noqa: E731
                                          batch_size=getattr(model.opt, 'eval_batch_size', 1), use_tqdm=False, frechet='device', cache=cache)
    else:
        fn = lambda fakes: metric.get_fid(fakes, model.inception_model, getattr(model, npz), device=model.device,      # noqa: E731
                                          batch_size=getattr(model.opt, 'eval_batch_size', 1), use_tqdm=False)
    model.fid_fn = _builtin(fn)
    return fn, True


def _miou_callable(model):
    """(miou_fn, built_in): an attached model.miou_fn wins; otherwise get_mIoU(fakes, names, self.drn_model, ...) (inception_distiller.py:263-270)."""
    fn = getattr(model, 'miou_fn', None)
    if fn is not None and not getattr(fn, 'cat_builtin', False):
        return fn, False
    if getattr(model, 'drn_model', None) is None:
        raise RuntimeError('evaluate_model: call evaluation.attach_miou(model, drn_checkpoint, table_path, data_dir) or attach model.miou_fn = '
                           'lambda fakes, names: ... (cat_amd/distillers/evaluation.py)')
    from .. import metric
    table_path = getattr(model, 'miou_table_path', None) or model.opt.table_path
    data_dir = getattr(model, 'miou_data_dir', None) or model.opt.cityscapes_path
    fn = lambda fakes, names: metric.get_mIoU(fakes, names, model.drn_model, model.device, table_path=table_path, data_dir=data_dir,      # noqa: E731
                                              batch_size=getattr(model.opt, 'eval_batch_size', 1), num_workers=getattr(model.opt, 'num_threads', 8),
                                              use_tqdm=False)
    model.miou_fn = _builtin(fn)
    return fn, True


def evaluate(model, step, student, feed, images, want_fid, want_miou, save_all=False, *, loader='eval_dataloader', run=None, fake='Sfake_B',
             subdir='', npz='npz', is_best='is_best', best_fid='best_fid', fids='fids', fid_key='metric/fid', best_miou='best_mIoU',
             mious='mIoUs', miou_key='metric/mIoU'):
    """feed(batch): set_input / set_single_input; images(j): {'input'|'real'|'Tfake'|'Sfake': HWC uint8} of sample j of the batch.
    student: the generator, or the generators, that run in eval mode during the loop.  The keyword arguments name what differs between the
    models, and their defaults are the distillers': `loader` the attribute holding the dataloader, `run` the function of one test pass
    (model.test), `fake` the attribute holding the generated batch, `subdir` the directory under eval/<step> the image kinds go to, `npz` the
    attribute with the real statistics, `is_best` / `best_*` / `fids` / `mious` the bookkeeping attributes and `*_key` the metric names.

    model.eval_images == 'device' (the default is 'host', the reference's list of CPU float tensors): the generated batches are quantised
    into a metric.DeviceImages where they lie and the package's own metrics read that set.  An attached fid_fn / miou_fn has the
    reference's contract and forces the host path for the evaluation."""
    if getattr(model, loader, None) is None:
        raise RuntimeError('evaluate_model: attach model.%s (the reference builds it from --dataroot in __init__; '
                           'cat_amd does not own datasets)' % loader)
    mode = getattr(model, 'eval_images', 'host')
    if mode not in ('host', 'device'):
        raise ValueError("evaluate_model: model.eval_images must be 'host' or 'device' (got %r)" % (mode,))
    fid_fn, fid_own = _fid_callable(model, npz) if want_fid else (None, True)
    miou_fn, miou_own = _miou_callable(model) if want_miou else (None, True)
    on_device = mode == 'device' and fid_own and miou_own
    setattr(model, is_best, False)
    save_dir = os.path.join(model.opt.log_dir, 'eval', str(step), subdir)
    os.makedirs(save_dir, exist_ok=True)
    students = list(student) if isinstance(student, (list, tuple)) else [student]
    run = model.test if run is None else run
    for net in students:
        net.eval()
    names, cnt = [], 0
    if on_device:
        from ..metric import DeviceImages
        fakes = DeviceImages()
    else:
        fakes = []
    try:
        batches = getattr(model, loader)
        for batch in batches:
            feed(batch)
            run()
            out = getattr(model, fake)
            if on_device and len(fakes) == 0 and hasattr(batches, '__len__'):
                fakes = DeviceImages(capacity=out.shape[0] * len(batches))      # sized once where the loader tells: no growth copies
            fakes.append(out if on_device else out.detach().cpu().contiguous())
            for j in range(len(model.image_paths)):
                name = os.path.splitext(ntpath.basename(model.image_paths[j]))[0]
                names.append(name)
                if cnt < 10 or save_all:
                    for kind, arr in images(j).items():
                        save_image(arr, os.path.join(save_dir, kind, '%s.png' % name))
                cnt += 1
    finally:
        for net in students:
            net.train()
    ret = {}
    if want_fid:
        fid = float(fid_fn(fakes))
        ret[fid_key] = fid
        ret[fid_key + '-mean'] = _track(model, fid, best_fid, fids, lambda a, b: a < b, is_best)
        ret[fid_key + '-best'] = getattr(model, best_fid)
    if want_miou:
        miou = float(miou_fn(fakes, names))
        ret[miou_key] = miou
        ret[miou_key + '-mean'] = _track(model, miou, best_miou, mious, lambda a, b: a > b, is_best)
        ret[miou_key + '-best'] = getattr(model, best_miou)
    return ret


