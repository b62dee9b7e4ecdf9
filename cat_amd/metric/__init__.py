"""Evaluation metrics of the distillers (reference metric/__init__.py): FID with its InceptionV3 feature extractor, the cityscapes mIoU
with its DRN-D-105 segmentation network and the kernel inception distance (metric/kid_score.py), all on the HIP kernels."""
import numpy as np
import torch

from .fid_score import _compute_statistics_of_ims, calculate_frechet_distance, get_activations_from_ims  # noqa: F401
from .drn import DRNSeg  # noqa: F401
from .images import DeviceImages  # noqa: F401
from .inception import InceptionV3  # noqa: F401
from .miou import miou_from_hist, per_class_iu  # noqa: F401


# get_fid, get_kid, get_mIoU and get_cityscapes_mIoU take a DeviceImages (cat_amd/metric/images.py: the generated set as uint8 on the device)
# wherever they take `fakes`, the reference's list of [B, 3, H, W] CPU tensors: the same bytes, batching and numbers, without a float copy
# of the set on either side.  With a list they do what the reference does.
def tensor2im_batch(t):
    """util.tensor2im on a [N, 3, H, W] batch in [-1, 1] (utils/util.py:58-88): [N, H, W, 3] uint8, truncating cast."""
    a = t.detach().cpu().float().numpy()
    return np.clip((np.transpose(a, (0, 2, 3, 1)) + 1) / 2.0 * 255.0, 0, 255).astype(np.uint8)


def get_fid(fakes, model, npz, device=None, batch_size=1, use_tqdm=True, frechet='host', cache=None):
    """metric/__init__.py:11-21: `fakes` = list of [B, 3, H, W] tensors in [-1, 1]; npz = {'mu', 'sigma'} of the real set.
    frechet='host' (the default): the reference's numpy + scipy tail.  frechet='device': the features stay on the GPU and the distance is
    float64 arithmetic on the f64 MFMA (fid_score.frechet_distance_from_features; no scipy); npz may then hold float64 device tensors, and
    `cache` is the dict that keeps what depends on the real set alone between calls."""
    if frechet not in ('host', 'device'):
        raise ValueError("get_fid: frechet must be 'host' or 'device' (got %r)" % (frechet,))
    m1, s1 = npz['mu'], npz['sigma']
    ims = fakes if isinstance(fakes, DeviceImages) else tensor2im_batch(torch.cat(fakes, dim=0)).astype(float)
    if frechet == 'device':
        from . import fid_score
        feats = fid_score.get_activations_device(ims, model, batch_size, 2048, device)
        return fid_score.frechet_distance_from_features(m1, s1, feats, device=device, cache=cache)
    m2, s2 = _compute_statistics_of_ims(ims, model, batch_size, 2048, device, use_tqdm=use_tqdm)
    return float(calculate_frechet_distance(m1, s1, m2, s2))


def get_kid(fakes, real_codes, model, device=None, batch_size=1, n_subsets=100, subset_size=100):
    """KID of `fakes` (list of [B, 3, H, W] tensors in [-1, 1], as get_fid takes them) against `real_codes`, the [n, 2048] pool3 features of
    the real set (kid_score.get_activations): (mean, std) of the subset estimates, as metric/kid_score.py:140-145 reports them.  The fakes
    become uint8 images first (tensor2im_batch), so the number equals the one of the same images saved as PNG files and read by
    calculate_kid_given_paths.  model = cat_amd.metric.InceptionV3([3]) on `device`."""
    from . import kid_score
    ims = fakes if isinstance(fakes, DeviceImages) else tensor2im_batch(torch.cat(fakes, dim=0))
    codes = kid_score._activations(kid_score._load_uint8(ims), len(ims), model, batch_size, real_codes.shape[1], device, False)
    mmds = kid_score.polynomial_mmd_averages(real_codes, codes, n_subsets=n_subsets, subset_size=subset_size, ret_var=False, device=device)
    return float(mmds.mean()), float(mmds.std())


def get_mIoU(fakes, names, model, device, table_path='datasets/table.txt', data_dir='database/cityscapes', batch_size=1, num_workers=8,
             num_classes=19, use_tqdm=True):
    """metric/__init__.py:24-46: `fakes` = list of [B, 3, H, W] tensors in [-1, 1], `names` = their image names (looked up in the table);
    model = cat_amd.metric.DRNSeg on `device`."""
    from . import miou
    ims = fakes if isinstance(fakes, DeviceImages) else tensor2im_batch(torch.cat(fakes, dim=0))
    return float(miou.test(ims, names, model, device, table_path=table_path, data_dir=data_dir, batch_size=batch_size, num_workers=num_workers,
                           num_classes=num_classes, use_tqdm=use_tqdm))


def get_cityscapes_mIoU(fakes, names, model, device, table_path='datasets/table.txt', data_dir='database/cityscapes', batch_size=1, num_workers=8,
                        num_classes=19, tqdm_position=None):
    """metric/__init__.py:49-71: the same arithmetic through metric/cityscapes_mIoU.py's `test`."""
    from . import miou
    ims = fakes if isinstance(fakes, DeviceImages) else tensor2im_batch(torch.cat(fakes, dim=0))
    return float(miou.test_cityscapes(ims, names, model, device, table_path=table_path, data_dir=data_dir, batch_size=batch_size,
                                      num_workers=num_workers, num_classes=num_classes, tqdm_position=tqdm_position))
