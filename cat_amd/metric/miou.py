"""Cityscapes mIoU with the segmentation network and the whole tail on the HIP kernels.

Reference: metric/mIoU_score.py:66-108 (SegList), :111-112 (per_class_iu), :174-247 (fast_hist, resize_4d_tensor, test) and
metric/cityscapes_mIoU.py (the same arithmetic with a `tqdm_position`).  The reference copies every [1, 19, h, w] log-probability map to
the host, enlarges it to 2048 x 1024 with PIL in 19 threads, takes the argmax and bins it with numpy.  Here the normalised image batch
goes to the device once, DRNSeg (cat_amd/metric/drn.py) runs on it batch by batch, per batch only the uint8 labels go up, and
cat_seg_confusion resizes + argmaxes + bins on the device into one 19 x 19 matrix of 64-bit counters that comes down once, at the end.
Host code (PIL, numpy): the table / name matching, label loading, the uint8 image -> `/ 255` -> mean / std normalisation, and the final
per-class IoU arithmetic."""
import ctypes as C
import os

import numpy as np
import torch

from .. import _lib as L
from .. import ops

# SegList's normalisation (metric/mIoU_score.py:75-81)
MEAN = [0.29010095242892997, 0.32808144844279574, 0.28696394422942517]
STD = [0.1829540508368939, 0.18656561047509476, 0.18447508988480435]
IGNORE = 255


def read_label_list(names, table_path):
    """The label file of every name, by the rule of SegList.read_lists (:96-108).  A table line is `<id> <label path> <image path>`; a name
    selects the first line whose id it equals or whose image path, without its '.png', ends with it.  A name without a line is an error (the
    reference asserts that both lists have one length)."""
    rows = []
    with open(table_path) as f:
        for line in f:
            ident, label_path, image_path = line.strip().split(' ')[:3]
            rows.append((ident, image_path[:-4], label_path))

    def lookup(name):
        return next((label for ident, stem, label in rows if ident == name or stem.endswith(name)), None)
    found = [lookup(name) for name in names]
    missing = [name for name, label in zip(names, found) if label is None]
    assert not missing, 'mIoU: no table line for %s' % ', '.join(missing[:5])
    return found


def normalize_images(ims):
    """uint8 [N, H, W, 3] (util.tensor2im's output) -> float32 [N, 3, H, W]: ToTensor's `/ 255`, then `(x - mean) / std` per channel in
    float32, as Normalize does it in place (:28-35, 42-51)."""
    x = torch.from_numpy(np.ascontiguousarray(ims)).permute(0, 3, 1, 2).contiguous().float() / 255
    mean, std = torch.FloatTensor(MEAN), torch.FloatTensor(STD)
    for c in range(3):
        x[:, c].sub_(mean[c]).div_(std[c])
    return x


def load_labels(paths, data_dir):
    """Label images as uint8 [N, Hl, Wl]; values outside [0, 255) can never be a class (fast_hist keeps 0 <= label < n) and become 255."""
    from PIL import Image
    out = []
    for p in paths:
        a = np.array(Image.open(os.path.join(data_dir, p)), dtype=np.int64)
        if a.ndim != 2:
            raise ValueError('mIoU: label image %s is not single-channel' % p)
        out.append(np.where((a >= 0) & (a < IGNORE), a, IGNORE).astype(np.uint8))
    return np.stack(out)


def per_class_iu(hist):
    """metric/mIoU_score.py:111-112; a class that is never labelled and never predicted gives 0 / 0 = NaN (dropped by nanmean)."""
    hist = np.asarray(hist, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))


def miou_from_hist(hist):
    """`round(np.nanmean(per_class_iu(hist) * 100), 2)` (:243-247)."""
    return round(np.nanmean(per_class_iu(hist) * 100), 2)


def confusion(logp, label, hist, n_classes, pred=None):
    """hist (int64 [n, n] on the device) += confusion matrix of argmax(resize(logp)) against `label` (uint8 [N, Hl, Wl] on the device);
    pred: optional uint8 [N, Hl, Wl] that receives the class map."""
    n, c, h, w = logp.shape
    if not ops.is_act(logp):
        raise ValueError('confusion: logp must be an NHWC activation')
    if label.dtype != torch.uint8 or not label.is_contiguous() or label.dim() != 3 or label.shape[0] != n:
        raise ValueError('confusion: label must be a contiguous uint8 [N, Hl, Wl] tensor')
    if hist.dtype != torch.int64 or not hist.is_contiguous() or hist.numel() != n_classes * n_classes:
        raise ValueError('confusion: hist must be a contiguous int64 [n, n] tensor')
    if pred is not None and (pred.dtype != torch.uint8 or not pred.is_contiguous() or pred.shape != label.shape):
        raise ValueError('confusion: pred must match label')
    L.call('cat_seg_confusion', ops._p(logp), ops.act_cs(logp), n, h, w, c, ops._p(label), label.shape[1], label.shape[2], n_classes, ops._p(hist),
           ops._p(pred), ops._stream())


def confusion_matrix(ims, names, model, device, table_path, data_dir, batch_size, num_classes, progress=None, preds=None):
    """The loop of `test` (:220-241) -> int64 [n, n] numpy matrix.  ims: uint8 [N, H, W, 3]; preds: optional list that receives the uint8
    class maps (one [B, Hl, Wl] array per batch).  ims may be a DeviceImages set (cat_amd/metric/images.py): every batch is then normalised
    from the bytes where they lie (cat_image_normalize: the values of normalize_images), and no float copy of the set exists."""
    from .images import DeviceImages
    labels = read_label_list(names, table_path)
    model.eval()
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if isinstance(ims, DeviceImages):
        def load(s):
            return ims.batch(s, s + batch_size, MEAN, STD)
    else:
        x = normalize_images(ims).to(device)      # the whole normalised set goes up once

        def load(s):
            return x[s:s + batch_size]
    hist = torch.zeros((num_classes, num_classes), dtype=torch.int64, device=device)
    batches = range(0, len(names), batch_size)
    with torch.no_grad():
        for s in (progress(batches) if progress is not None else batches):
            lab = torch.from_numpy(load_labels(labels[s:s + batch_size], data_dir)).to(device)
            final = model(load(s))[0]
            pred = torch.empty_like(lab) if preds is not None else None
            confusion(final, lab, hist, num_classes, pred)
            if preds is not None:
                preds.append(pred.cpu().numpy())
    return hist.cpu().numpy()


def test(fakes, names, model, device, table_path='datasets/table.txt', data_dir='database/cityscapes', batch_size=1, num_workers=8, num_classes=19,
         use_tqdm=True):
    """metric/mIoU_score.py:209-247 as get_mIoU calls it.  `num_workers` is accepted for the signature: there is no DataLoader (labels are
    read in the loop)."""
    progress = None
    if use_tqdm:
        from tqdm import tqdm
        progress = tqdm
    return miou_from_hist(confusion_matrix(fakes, names, model, device, table_path, data_dir, batch_size, num_classes, progress))


def test_cityscapes(fakes, names, model, device, table_path='datasets/table.txt', data_dir='database/cityscapes', batch_size=1, num_workers=8,
                    num_classes=19, tqdm_position=None):
    """metric/cityscapes_mIoU.py's `test`: the same arithmetic, progress bar at `tqdm_position`."""
    progress = None
    if tqdm_position:
        import tqdm
        progress = lambda it: tqdm.tqdm(it, desc='mIoU       ', position=tqdm_position, leave=False)  # noqa: E731
    return miou_from_hist(confusion_matrix(fakes, names, model, device, table_path, data_dir, batch_size, num_classes, progress))
