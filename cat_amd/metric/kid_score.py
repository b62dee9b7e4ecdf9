"""Kernel inception distance (reference metric/kid_score.py) with both halves on the HIP kernels.

Features come from cat_amd.metric.InceptionV3; the MMD tail -- three polynomial kernels per random subset and the sums `_mmd2_and_variance`
reads of them (:184-281) -- is one call of cat_kid_poly_sums for ALL subsets, float64 on the f64 MFMA (csrc/kid_ops.hip).  No kernel
matrix is ever stored and nothing of it crosses to the host but 6 * m + 4 sums per subset; the closed-form estimator on those sums
(`mmd2_and_variance_from_sums`) is float64 numpy, a few dozen flops per subset.  The reference uses sklearn's `polynomial_kernel` here; this
module needs neither sklearn nor a BLAS.

Names and semantics follow the reference file.  Differences: `cuda` flags are `device` arguments, there is no CPU path for the arithmetic,
and the Inception checkpoint is passed in (`--inception-path`), never downloaded.

    python -m cat_amd.metric.kid_score --real R --fake F [F ...] [--batch-size 2] [--dims 2048] [--gpu 0] --inception-path CKPT"""
import os
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np
import torch

from .features import add_inception_arguments, default_device as _default_device, feature_batches, load_inception

SUM_KEYS = ('rs_xx', 'dg_xx', 'rs_yy', 'dg_yy', 'rs_xy', 'cs_xy')      # [S, m] each, in the order of the kernel's output row
SCALAR_KEYS = ('tr_xy', 'sq_xx', 'sq_yy', 'sq_xy')                      # [S] each


# ---------------------------------------------------------------------------------------------------------------- features
def _activations(load, n, model, batch_size, dims, device, verbose):
    """The loop of get_activations (:51-97): `load(start, end)` returns the float32 [B, 3, H, W] batch in [0, 1]; a DeviceImages set in its
    place hands over its own `u8 / 255` batches, on the device."""
    from .images import DeviceImages
    if isinstance(load, DeviceImages):
        load = load.batch
    if n % batch_size != 0:
        print(('Warning: number of images is not a multiple of the '
               'batch size. Some samples are going to be ignored.'))
    if batch_size > n:
        print(('Warning: batch size is bigger than the data size. '
               'Setting batch size to data size'))
        batch_size = n
    n_batches = n // batch_size
    pred_arr = np.empty((n_batches * batch_size, dims))
    for start, end, feats in feature_batches(load, n, model, batch_size, _default_device(device), full_only=True):
        if verbose:
            print('\rPropagating batch %d/%d' % (end // batch_size, n_batches), end='', flush=True)
        pred_arr[start:end] = feats.cpu().numpy()
    if verbose:
        print(' done')
    return pred_arr


def _load_files(files):
    from PIL import Image

    def load(start, end):
        images = [np.array(Image.open(str(f))) for f in files[start:end]]
        images = np.stack(images).astype(np.float32) / 255.
        return images.transpose((0, 3, 1, 2))
    return load


def _load_uint8(ims):
    """uint8 [N, H, W, 3] images exactly as `_load_files` hands over the same images read back from PNG files (a DeviceImages set: itself)"""
    from .images import DeviceImages
    if isinstance(ims, DeviceImages):
        return ims

    def load(start, end):
        return (ims[start:end].astype(np.float32) / 255.).transpose((0, 3, 1, 2))
    return load


def get_activations(files, model, batch_size=50, dims=2048, device=None, verbose=False):
    """metric/kid_score.py:27-97.  files: a list of image paths, or an array [N, 3, H, W] in [-1, 1] (scaled `(x + 1) / 2`).  Images beyond
    the last full batch are DROPPED (the reference's behaviour, with its warning); returns float64 [n_used, dims]."""
    if type(files[0]) == np.ndarray:
        def load(start, end):
            images = np.copy(files[start:end]) + 1
            images /= 2.
            return images
    else:
        load = _load_files(files)
    return _activations(load, len(files), model, batch_size, dims, device, verbose)


def _compute_activations(path, model, batch_size, dims, device):
    """metric/kid_score.py:100-111: a directory is globbed for *.jpg, then *.png; more than 50 000 files are shuffled and cut."""
    if not type(path) == np.ndarray:
        import glob
        jpg = os.path.join(path, '*.jpg')
        png = os.path.join(path, '*.png')
        path = glob.glob(jpg) + glob.glob(png)
        if len(path) > 50000:
            import random
            random.shuffle(path)
            path = path[:50000]
    return get_activations(path, model, batch_size, dims, device)


def _inception_for(dims, inception, device):
    return load_inception(dims, inception, device, 'KID')


def calculate_kid_given_paths(paths, batch_size, device, dims, inception=None):
    """metric/kid_score.py:114-146: paths[0] is the real set, every further path a fake set; each a directory of images or a .npy array
    [N, 3, H, W] in [-1, 1].  inception: the torchvision-keyed FID checkpoint (path or state_dict) or a ready cat_amd.metric.InceptionV3.
    Returns [(path, mean, std)] of the 100 subset estimates per fake path."""
    pths = []
    for p in paths:
        if not os.path.exists(p):
            raise RuntimeError('Invalid path: %s' % p)
        if os.path.isdir(p):
            pths.append(p)
        elif p.endswith('.npy'):
            np_imgs = np.load(p)
            if np_imgs.shape[0] > 50000:
                np_imgs = np_imgs[np.random.permutation(np.arange(np_imgs.shape[0]))][:50000]
            pths.append(np_imgs)
    device = _default_device(device)
    model = _inception_for(dims, inception, device)
    act_true = _compute_activations(pths[0], model, batch_size, dims, device)
    pths = pths[1:]
    results = []
    for j, pth in enumerate(pths):
        print(paths[j + 1])
        actj = _compute_activations(pth, model, batch_size, dims, device)
        kid_values = polynomial_mmd_averages(act_true, actj, n_subsets=100, subset_size=100, device=device)
        results.append((paths[j + 1], kid_values[0].mean(), kid_values[0].std()))
    return results


# ---------------------------------------------------------------------------------------------------------------- the MMD tail
def _kernel_params(d, degree=3, gamma=None, coef0=1):
    """(degree, gamma, coef0) as the kernel takes them; gamma None = 1 / d (sklearn's polynomial_kernel).  Raises ValueError for what the
    kernel does not compute, before anything touches the device."""
    if isinstance(degree, bool) or int(degree) != degree or degree < 1:
        raise ValueError('KID: the polynomial degree must be an integer >= 1 (degree=%r)' % (degree,))
    if d % 4 != 0:
        raise ValueError('KID: the feature width must be a multiple of 4 (d=%d); the InceptionV3 widths 64, 192, 768, 2048 are' % d)
    return int(degree), (1.0 / d if gamma is None else float(gamma)), float(coef0)


def draw_subsets(n_g, n_r, n_subsets, subset_size):
    """The index tables of polynomial_mmd_averages (:167-170): per subset `np.random.choice(n_g, subset_size, replace=False)`, then the same
    for r -- the reference's order of draws from numpy's global generator, so a seed picks the reference's subsets.  int32 [n_subsets, m] x 2."""
    choice = np.random.choice
    gi = np.empty((n_subsets, subset_size), dtype=np.int32)
    ri = np.empty((n_subsets, subset_size), dtype=np.int32)
    for i in range(n_subsets):
        gi[i] = choice(n_g, subset_size, replace=False)
        ri[i] = choice(n_r, subset_size, replace=False)
    return gi, ri


def split_sums(out, m):
    """The kernel's [S, 6 * m + 4] output as a dict of [S, m] / [S] arrays (SUM_KEYS, SCALAR_KEYS)."""
    out = np.asarray(out)
    assert out.ndim == 2 and out.shape[1] == 6 * m + len(SCALAR_KEYS), out.shape
    sums = {k: out[:, i * m:(i + 1) * m] for i, k in enumerate(SUM_KEYS)}
    sums.update({k: out[:, 6 * m + i] for i, k in enumerate(SCALAR_KEYS)})
    return sums


def _features_to_device(codes, device):
    """float32 [n, d] on the device.  The features are float32 network outputs that the reference widens to float64: nothing is lost."""
    if isinstance(codes, torch.Tensor):
        t = codes.detach().to(device=device, dtype=torch.float32)
    else:
        t = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.float32)).to(device)
    if t.dim() != 2:
        raise ValueError('KID: features must be [n, d] (got %s)' % (tuple(t.shape),))
    return t.contiguous()


def poly_sums_device(x, y, gi, ri, degree, gamma, coef0, out=None, ws=None):
    """cat_kid_poly_sums on device tensors: x [nx, d], y [ny, d] float32 (may be the same tensor), gi / ri int32 [S, m] on the same device.
    Returns the float64 [S, 6 * m + 4] tensor of sums (layout: include/cat_hip.h).  out / ws: optional preallocated buffers."""
    from .. import _lib as L
    from .. import ops
    for t in (x, y, gi, ri):
        ops._require_cuda(t)
    if x.dtype != torch.float32 or y.dtype != torch.float32 or x.dim() != 2 or y.dim() != 2 or not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError('KID: features must be contiguous float32 [n, d] tensors')
    if x.shape[1] != y.shape[1]:
        raise ValueError('KID: feature widths differ (%d, %d)' % (x.shape[1], y.shape[1]))
    if gi.dtype != torch.int32 or ri.dtype != torch.int32 or gi.dim() != 2 or gi.shape != ri.shape or not (gi.is_contiguous() and ri.is_contiguous()):
        raise ValueError('KID: the index tables must be contiguous int32 [S, m] tensors of one shape')
    d = x.shape[1]
    degree, gamma, coef0 = _kernel_params(d, degree, gamma, coef0)
    n_sub, m = gi.shape
    if out is None:
        out = torch.empty((n_sub, 6 * m + len(SCALAR_KEYS)), dtype=torch.float64, device=x.device)
    nws = max(1, L.query('cat_kid_poly_sums_ws_bytes', n_sub, m) // 8)
    if ws is None:
        ws = torch.empty(nws, dtype=torch.float64, device=x.device)
    if out.dtype != torch.float64 or ws.dtype != torch.float64 or out.numel() != n_sub * (6 * m + 4) or ws.numel() < nws or \
            not (out.is_contiguous() and ws.is_contiguous()):
        raise ValueError('KID: out / ws must be contiguous float64 buffers of the documented sizes')
    with torch.cuda.device(x.device):
        L.call('cat_kid_poly_sums', ops._p(x), x.shape[0], ops._p(y), y.shape[0], d, ops._p(gi), ops._p(ri), n_sub, m, gamma, coef0, degree,
               ops._p(out), ops._p(ws), ops._stream())
    return out


def poly_sums(codes_g, codes_r, gi, ri, degree=3, gamma=None, coef0=1, device=None):
    """Host arrays in, dict of float64 numpy sums out (split_sums).  Index tables are checked against the feature counts here."""
    gi, ri = np.ascontiguousarray(gi, dtype=np.int32), np.ascontiguousarray(ri, dtype=np.int32)
    _kernel_params(np.shape(codes_g)[1], degree, gamma, coef0)
    if gi.ndim != 2 or gi.shape != ri.shape or gi.size == 0:
        raise ValueError('KID: the index tables must be [S, m] arrays of one shape')
    if gi.min() < 0 or gi.max() >= len(codes_g) or ri.min() < 0 or ri.max() >= len(codes_r):
        raise ValueError('KID: an index lies outside its feature matrix')
    device = _default_device(device)
    x = _features_to_device(codes_g, device)
    y = x if codes_r is codes_g else _features_to_device(codes_r, device)
    out = poly_sums_device(x, y, torch.from_numpy(gi).to(device), torch.from_numpy(ri).to(device), degree, gamma, coef0)
    return split_sums(out.cpu().numpy(), gi.shape[1])


def _sqn(arr):
    flat = np.ravel(arr)
    return flat.dot(flat)


def mmd2_and_variance_from_sums(sums, unit_diagonal=False, mmd_est='unbiased', var_at_m=None, ret_var=True):
    """metric/kid_score.py:205-281 from the sums it reads instead of the three m x m matrices.  sums: for ONE subset, a mapping with the row
    sums and diagonal of K_XX and K_YY ('rs_xx', 'dg_xx', 'rs_yy', 'dg_yy'), the row (axis=1) and column (axis=0) sums and the trace of K_XY
    ('rs_xy', 'cs_xy', 'tr_xy') and sum K^2 of each ('sq_xx', 'sq_yy', 'sq_xy').  Pure float64 numpy; needs no GPU."""
    rs_xx, rs_yy = np.asarray(sums['rs_xx'], dtype=np.float64), np.asarray(sums['rs_yy'], dtype=np.float64)
    m = rs_xx.shape[0]
    assert rs_xx.shape == (m,) and rs_yy.shape == (m,)
    if var_at_m is None:
        var_at_m = m
    if unit_diagonal:
        diag_X = diag_Y = 1
        sum_diag_X = sum_diag_Y = m
        sum_diag2_X = sum_diag2_Y = m
    else:
        diag_X = np.asarray(sums['dg_xx'], dtype=np.float64)
        diag_Y = np.asarray(sums['dg_yy'], dtype=np.float64)
        sum_diag_X = diag_X.sum()
        sum_diag_Y = diag_Y.sum()
        sum_diag2_X = _sqn(diag_X)
        sum_diag2_Y = _sqn(diag_Y)

    Kt_XX_sums = rs_xx - diag_X
    Kt_YY_sums = rs_yy - diag_Y
    K_XY_sums_0 = np.asarray(sums['cs_xy'], dtype=np.float64)
    K_XY_sums_1 = np.asarray(sums['rs_xy'], dtype=np.float64)

    Kt_XX_sum = Kt_XX_sums.sum()
    Kt_YY_sum = Kt_YY_sums.sum()
    K_XY_sum = K_XY_sums_0.sum()

    if mmd_est == 'biased':
        mmd2 = ((Kt_XX_sum + sum_diag_X) / (m * m) + (Kt_YY_sum + sum_diag_Y) / (m * m) - 2 * K_XY_sum / (m * m))
    else:
        assert mmd_est in {'unbiased', 'u-statistic'}
        mmd2 = (Kt_XX_sum + Kt_YY_sum) / (m * (m - 1))
        if mmd_est == 'unbiased':
            mmd2 -= 2 * K_XY_sum / (m * m)
        else:
            mmd2 -= 2 * (K_XY_sum - float(sums['tr_xy'])) / (m * (m - 1))

    if not ret_var:
        return mmd2

    Kt_XX_2_sum = float(sums['sq_xx']) - sum_diag2_X
    Kt_YY_2_sum = float(sums['sq_yy']) - sum_diag2_Y
    K_XY_2_sum = float(sums['sq_xy'])

    dot_XX_XY = Kt_XX_sums.dot(K_XY_sums_1)
    dot_YY_YX = Kt_YY_sums.dot(K_XY_sums_0)

    m1 = m - 1
    m2 = m - 2
    zeta1_est = (1 / (m * m1 * m2) * (_sqn(Kt_XX_sums) - Kt_XX_2_sum + _sqn(Kt_YY_sums) - Kt_YY_2_sum) - 1 / (m * m1)**2 *
                 (Kt_XX_sum**2 + Kt_YY_sum**2) + 1 / (m * m * m1) * (_sqn(K_XY_sums_1) + _sqn(K_XY_sums_0) - 2 * K_XY_2_sum) -
                 2 / m**4 * K_XY_sum**2 - 2 / (m * m * m1) * (dot_XX_XY + dot_YY_YX) + 2 / (m**3 * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum)
    zeta2_est = (1 / (m * m1) * (Kt_XX_2_sum + Kt_YY_2_sum) - 1 / (m * m1)**2 * (Kt_XX_sum**2 + Kt_YY_sum**2) + 2 / (m * m) * K_XY_2_sum -
                 2 / m**4 * K_XY_sum**2 - 4 / (m * m * m1) * (dot_XX_XY + dot_YY_YX) + 4 / (m**3 * m1) * (Kt_XX_sum + Kt_YY_sum) * K_XY_sum)
    var_est = (4 * (var_at_m - 2) / (var_at_m * (var_at_m - 1)) * zeta1_est + 2 / (var_at_m * (var_at_m - 1)) * zeta2_est)

    return mmd2, var_est


def _subset(sums, i):
    return {k: v[i] for k, v in sums.items()}


def polynomial_mmd_averages(codes_g, codes_r, n_subsets=50, subset_size=1000, ret_var=True, output=sys.stdout, device=None, **kernel_args):
    """metric/kid_score.py:154-181: the unbiased MMD^2 (and its variance estimate at m = min(len(codes_g), len(codes_r))) of `n_subsets` random
    subsets of `subset_size` features each.  The subsets are drawn from numpy's global generator in the reference's order; the features go to
    the device once and one kernel call covers all subsets.  `output` is where the reference's progress bar goes; there is no loop to show.
    kernel_args: degree, gamma, coef0 of polynomial_mmd."""
    m = min(codes_g.shape[0], codes_r.shape[0])
    _kernel_params(codes_g.shape[1], **kernel_args)
    gi, ri = draw_subsets(len(codes_g), len(codes_r), n_subsets, subset_size)
    sums = poly_sums(codes_g, codes_r, gi, ri, device=device, **kernel_args)
    mmds = np.zeros(n_subsets)
    if ret_var:
        vars = np.zeros(n_subsets)
    for i in range(n_subsets):
        o = mmd2_and_variance_from_sums(_subset(sums, i), var_at_m=m, ret_var=ret_var)
        if ret_var:
            mmds[i], vars[i] = o
        else:
            mmds[i] = o
    return (mmds, vars) if ret_var else mmds


def polynomial_mmd(codes_g, codes_r, degree=3, gamma=None, coef0=1, var_at_m=None, ret_var=True, device=None):
    """metric/kid_score.py:184-202 on two feature sets of one size: (mmd2, var_est), or mmd2 alone."""
    _kernel_params(codes_g.shape[1], degree, gamma, coef0)
    if len(codes_g) != len(codes_r):
        raise ValueError('polynomial_mmd: both sets must have one size (%d, %d)' % (len(codes_g), len(codes_r)))
    idx = np.arange(len(codes_g), dtype=np.int32)[None]
    sums = poly_sums(codes_g, codes_r, idx, idx, degree, gamma, coef0, device=device)
    return mmd2_and_variance_from_sums(_subset(sums, 0), var_at_m=var_at_m, ret_var=ret_var)


# ---------------------------------------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    parser = ArgumentParser(prog='python -m cat_amd.metric.kid_score', formatter_class=ArgumentDefaultsHelpFormatter)
    parser.add_argument('--real', type=str, required=True, help=('Path to the real images'))
    parser.add_argument('--fake', type=str, nargs='+', required=True, help=('Path to the generated images'))
    return add_inception_arguments(parser, batch_size=2).parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    print(args)
    if args.gpu == '':
        raise SystemExit('kid_score: --gpu must name a GPU; the kernels have no CPU path')
    device = torch.device('cuda', int(args.gpu))
    paths = [args.real] + args.fake
    results = calculate_kid_given_paths(paths, args.batch_size, device, args.dims, inception=args.inception_path)
    for p, m, s in results:
        print('KID (%s): %.3f (%.3f)' % (p, m, s))


if __name__ == '__main__':
    main()
