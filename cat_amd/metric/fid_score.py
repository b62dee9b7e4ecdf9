"""FID from pool3 features.  The feature half runs on the HIP kernels (cat_amd.metric.inception.InceptionV3); the
Frechet distance is host arithmetic on 2048 x 2048 matrices, as in the reference (metric/fid_score.py:217-275: numpy + scipy.linalg.sqrtm).

The `*_device` functions below are the same tail on the GPU in float64 (csrc/fid_ops.hip): the features stay on the device as one float32
tensor, mean and covariance come from cat_fid_stats, and Tr (S1 S2)^1/2 is the sum of the square roots of the eigenvalues of a symmetric
positive semi-definite M -- the Gram form M = Xc S1 Xc^T / (n - 1) when the fake set has n <= d features, the full form M = R S2 R with
R = S1^1/2 otherwise -- taken by the coupled Newton-Schulz iteration, which is nothing but cat_gemm_f64 calls (DESIGN section 3 "FID on the
device").  Opt-in: get_fid(..., frechet='device'); the host functions keep their behaviour.  The module is also the real-statistics writer:

    python -m cat_amd.metric.fid_score --images DIR_OR_NPY --output X.npz --inception-path CKPT [--batch-size 32] [--dims 2048] [--gpu 0]"""
import os

import numpy as np
import torch

from .features import add_inception_arguments, default_device, feature_batches, load_inception

NS_MAX_STEPS = 100          # cap of the Newton-Schulz iteration
NS_REL_STEP = 1e-14         # a step counts while the trace still grows by more than this, relative


def _scaled(ims):
    """load(start, end) over float images [N, H, W, 3] (or [N, 3, H, W]) in [0, 255]: the NCHW view of a slice, scaled IN PLACE.  A
    DeviceImages set (cat_amd/metric/images.py) hands over the same `u8 / 255` batch as a device activation; nothing of it is changed."""
    from .images import DeviceImages
    if isinstance(ims, DeviceImages):
        return ims.batch

    def load(start, end):
        images = ims[start:end] if ims.shape[1] == 3 else ims[start:end].transpose((0, 3, 1, 2))
        images /= 255
        return images
    return load


def get_activations_from_ims(ims, model, batch_size=50, dims=2048, device=None, verbose=False, use_tqdm=True):
    """metric/fid_score.py:152-216.  ims: float array [N, H, W, 3] (or [N, 3, H, W]) in [0, 255] -- it is scaled IN PLACE like the reference
    does (`images /= 255` on a view); returns [N, dims] float64 features.  Same batching (the last batch may be short)."""
    batches = feature_batches(_scaled(ims), len(ims), model, batch_size, default_device(device))
    if use_tqdm:
        try:
            from tqdm import tqdm
            batches = tqdm(batches, total=(len(ims) + batch_size - 1) // batch_size)
        except ImportError:
            pass
    pred_arr = np.empty((len(ims), dims))
    for start, end, feats in batches:
        pred_arr[start:end] = feats.cpu().numpy()
    if verbose:
        print(' done')
    return pred_arr


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + Tr(S1 + S2 - 2 sqrt(S1 S2)) (metric/fid_score.py:217-275): matrix square root by scipy, the near-singular retry
    with eps on the diagonals, imaginary parts below 1e-3 dropped."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    assert mu1.shape == mu2.shape, 'Training and test mean vectors have different lengths'
    assert sigma1.shape == sigma2.shape, 'Training and test covariances have different dimensions'
    diff = mu1 - mu2
    prod = sigma1.dot(sigma2)
    ok = True
    for _ in range(30):
        ok = True
        covmean, _ = linalg.sqrtm(prod, disp=False)
        if not np.isfinite(covmean).all():
            print('fid calculation produces singular product; adding %s to diagonal of cov estimates' % eps)
            offset = np.eye(sigma1.shape[0]) * eps
            covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
        if np.iscomplexobj(covmean):
            if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
                ok = False
            covmean = covmean.real
        if ok:
            break
    if not ok:
        print('Warning: the fid may be incorrect!')
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def _compute_statistics_of_ims(ims, model, batch_size, dims, device, use_tqdm=True):
    act = get_activations_from_ims(ims, model, batch_size, dims, device, verbose=False, use_tqdm=use_tqdm)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


# ---------------------------------------------------------------------------------------------------------------- the tail on the device
def get_activations_device(ims, model, batch_size=50, dims=2048, device=None):
    """The loop of get_activations_from_ims -- the same batching, the same in-place `/= 255` -- with the float32 [N, dims] features returned
    as ONE device tensor.  The network's outputs are float32, which the host path widens to float64: nothing is lost."""
    device = default_device(device)
    feats = torch.empty((len(ims), dims), dtype=torch.float32, device=device)
    for start, end, f in feature_batches(_scaled(ims), len(ims), model, batch_size, device):
        feats[start:end] = f
    return feats


def _check_features(feats):
    if not isinstance(feats, torch.Tensor) or feats.dim() != 2:
        raise ValueError('FID: features must be a [n, d] tensor (got %s)' % (type(feats).__name__,))
    if feats.dtype != torch.float32:
        raise ValueError('FID: features must be float32 (got %s)' % (feats.dtype,))
    n, d = feats.shape
    if n < 2:
        raise ValueError('FID: a covariance needs at least 2 features (n=%d)' % n)
    if d % 4 != 0:
        raise ValueError('FID: the feature width must be a multiple of 4 (d=%d); the InceptionV3 widths 64, 192, 768, 2048 are' % d)
    return n, d


def _check_stats(mu, sigma, d=None):
    """shapes and dtypes of a (mu, sigma) pair, numpy or tensor; returns d"""
    for name, a, nd in (('mu', mu, 1), ('sigma', sigma, 2)):
        if not isinstance(a, (np.ndarray, torch.Tensor)) or a.ndim != nd:
            raise ValueError('FID: %s must be a %d-dimensional array or tensor' % (name, nd))
        if a.dtype != (torch.float64 if isinstance(a, torch.Tensor) else np.float64):
            raise ValueError('FID: %s must be float64 (got %s)' % (name, a.dtype))
    if sigma.shape[0] != sigma.shape[1] or sigma.shape[0] != mu.shape[0]:
        raise ValueError('FID: mu %s and sigma %s do not belong together' % (tuple(mu.shape), tuple(sigma.shape)))
    if d is not None and mu.shape[0] != d:
        raise ValueError('FID: the statistics are %d wide, the features %d' % (mu.shape[0], d))
    if mu.shape[0] % 4 != 0:
        raise ValueError('FID: the feature width must be a multiple of 4 (d=%d)' % mu.shape[0])
    return mu.shape[0]


def _f64_device(a, device):
    if isinstance(a, torch.Tensor):
        return a.detach().to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _call(name, *args):
    """A library entry on the current stream, tensors as their pointers.  Imported on first use: the argument checks need no library."""
    from .. import _lib, ops
    _lib.call(name, *[ops._p(a) if isinstance(a, torch.Tensor) else a for a in args], ops._stream())


def _query(name, *args):
    from .. import _lib
    return _lib.query(name, *args)


def _require_cuda(t):
    from .. import ops
    ops._require_cuda(t)


def _gemm(a, b, trans_b=False, alpha=1.0, beta_eye=0.0, out=None):
    """cat_gemm_f64 on contiguous float64 device matrices: alpha * a @ (b.T if trans_b else b) + beta_eye * I"""
    m, k = a.shape
    n = b.shape[0] if trans_b else b.shape[1]
    assert (b.shape[1] if trans_b else b.shape[0]) == k and a.is_contiguous() and b.is_contiguous()
    if out is None:
        out = torch.empty((m, n), dtype=torch.float64, device=a.device)
    _call('cat_gemm_f64', a, a.shape[1], b, b.shape[1], int(trans_b), out, out.shape[1], m, n, k, float(alpha), float(beta_eye))
    return out


def _trace_sumsq(a, want_sumsq, out, ws):
    """(trace, sum of squares or NaN) of a square device matrix as two Python floats: a 16-byte copy"""
    _call('cat_f64_trace_sumsq', a, a.shape[0], a.shape[1], int(want_sumsq), out, ws)
    return tuple(out.tolist())


def _symmetrize(a, scale=1.0, out=None):
    out = a if out is None else out
    _call('cat_f64_symmetrize', a, a.shape[0], a.shape[1], float(scale), out, out.shape[1])
    return out


def statistics_device(feats):
    """(mu [d], sigma [d, d]) of float32 device features as float64 device tensors: np.mean(axis=0) and np.cov(rowvar=False) by cat_fid_stats"""
    n, d = _check_features(feats)
    _require_cuda(feats)
    feats = feats.contiguous()
    mu = torch.empty(d, dtype=torch.float64, device=feats.device)
    sigma = torch.empty((d, d), dtype=torch.float64, device=feats.device)
    with torch.cuda.device(feats.device):
        _call('cat_fid_stats', feats, n, d, mu, sigma)
    return mu, sigma


def compute_statistics_of_ims_device(ims, model, batch_size, dims, device):
    """_compute_statistics_of_ims with the features and both statistics on the device"""
    return statistics_device(get_activations_device(ims, model, batch_size, dims, device))


def _newton_schulz(m_sym):
    """The coupled Newton-Schulz iteration on a symmetric positive semi-definite device matrix M: Y0 = M / c, Z0 = I, c = |M|_F;
    T = 1.5 I - 0.5 Z Y, Y <- Y T, Z <- T Z; M^1/2 = sqrt(c) Y.  M is singular whenever it comes from centred features, and on a singular M
    the iteration is unstable once it has converged, so it stops at the first step whose trace is not finite or does not exceed the
    previous one by more than 1e-14 relative, and keeps the iterate with the larger finite trace.
    Returns (Y or None, c, Tr Y, steps, converged): converged is False at the cap or on a non-finite trace."""
    n = m_sym.shape[0]
    dev = m_sym.device
    out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = torch.empty(max(1, _query('cat_f64_trace_sumsq_ws_bytes', n) // 8), dtype=torch.float64, device=dev)
    _, ss = _trace_sumsq(m_sym, True, out, ws)
    if not np.isfinite(ss):
        return None, float('nan'), float('nan'), 0, False
    c = float(np.sqrt(ss))
    if c == 0.0:
        return torch.zeros_like(m_sym), 0.0, 0.0, 0, True
    y = _symmetrize(m_sym, 1.0 / c, torch.empty_like(m_sym))
    z = torch.eye(n, dtype=torch.float64, device=dev)
    t, y2, z2 = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
    best, _ = _trace_sumsq(y, False, out, ws)
    for step in range(1, NS_MAX_STEPS + 1):
        _gemm(z, y, alpha=-0.5, beta_eye=1.5, out=t)
        _gemm(y, t, out=y2)
        _gemm(t, z, out=z2)
        tr, _ = _trace_sumsq(y2, False, out, ws)
        if not np.isfinite(tr):
            return y, c, best, step, False
        if not tr > best * (1.0 + NS_REL_STEP):
            return (y2, c, tr, step, True) if tr > best else (y, c, best, step, True)
        best = tr
        y, y2, z, z2 = y2, y, z2, z
    return y, c, best, NS_MAX_STEPS, False


def sqrtm_trace_device(M):
    """Tr M^1/2 of a symmetric positive semi-definite float64 device matrix: (trace, steps, converged).  converged False (the cap of 100
    steps, or a non-finite value) means the trace must not be used."""
    if not isinstance(M, torch.Tensor) or M.dim() != 2 or M.shape[0] != M.shape[1] or M.dtype != torch.float64:
        raise ValueError('sqrtm_trace_device: a square float64 device matrix is required')
    _require_cuda(M)
    with torch.cuda.device(M.device):
        _, c, tr, steps, ok = _newton_schulz(M.contiguous())
    return float(np.sqrt(c) * tr) if ok else float('nan'), steps, ok


def _root_device(sigma):
    """(R = sigma^1/2 as a device matrix, steps) or (None, steps) if the iteration did not converge"""
    y, c, _, steps, ok = _newton_schulz(_symmetrize(sigma, 1.0, torch.empty_like(sigma)))
    if not ok:
        return None, steps
    return _symmetrize(y, float(np.sqrt(c))), steps


def _trace_device(a):
    out = torch.empty(2, dtype=torch.float64, device=a.device)      # without the sum of squares the workspace is not used
    return _trace_sumsq(a, False, out, out)[0]


def _real_side(cache, sigma1, device):      # (sigma1 on the device, its trace): uploaded and taken once per `cache`
    if 'sigma1' not in cache:
        cache['sigma1'] = _f64_device(sigma1, device)
        cache['tr1'] = _trace_device(cache['sigma1'])
    return cache['sigma1'], cache['tr1']


def _full_form(sigma1, sigma2, cache):
    """Tr (S1 S2)^1/2 through M = R S2 R, R = S1^1/2 (kept in `cache`): (trace, steps, converged)"""
    root = cache.get('root')
    steps0 = 0
    if root is None:
        root, steps0 = _root_device(sigma1)
        if root is None:
            return float('nan'), steps0, False
        cache['root'] = root
    m = _symmetrize(_gemm(_gemm(root, sigma2), root))
    tr, steps, ok = sqrtm_trace_device(m)
    return tr, steps0 + steps, ok


def _fall_back(mu1, sigma1, mu2, sigma2, steps):
    print('Warning: the device square root did not converge in %d steps; evaluating the Frechet distance on the host' % steps)
    return float(calculate_frechet_distance(_host(mu1), _host(sigma1), _host(mu2), _host(sigma2)))


def frechet_distance_from_features(mu1, sigma1, feats2, device=None, cache=None, info=None):
    """FID of the fake features `feats2` (float32 [n, d] device tensor) against the real statistics (mu1, sigma1), numpy arrays or float64
    device tensors.  n <= d (every launch script: 120 to 1100 images against 2048): the Gram form, sigma2 is never formed; n > d: the full
    form.  cache: a dict the caller keeps per real set -- the uploaded sigma1, its trace and, in the full form, its root are computed once.
    info: a dict that receives `form`, `steps`, `converged`.  Falls back to the host calculate_frechet_distance, with a warning, if the
    iteration does not converge."""
    n, d = _check_features(feats2)
    _check_stats(mu1, sigma1, d)
    _require_cuda(feats2)
    device = feats2.device if device is None else torch.device(device)
    cache = {} if cache is None else cache
    info = {} if info is None else info
    feats2 = feats2.contiguous()
    with torch.cuda.device(device):
        s1, tr1 = _real_side(cache, sigma1, device)
        if n <= d:
            info['form'] = 'gram'
            mu2 = torch.empty(d, dtype=torch.float64, device=device)
            _call('cat_fid_mean', feats2, n, d, mu2)
            xc = torch.empty((n, d), dtype=torch.float64, device=device)
            ss = torch.empty(1, dtype=torch.float64, device=device)
            ws = torch.empty(max(1, _query('cat_fid_center_ws_bytes', n) // 8), dtype=torch.float64, device=device)
            _call('cat_fid_center', feats2, mu2, n, d, xc, ss, ws)
            m = _symmetrize(_gemm(_gemm(xc, s1), xc, trans_b=True, alpha=1.0 / (n - 1)))
            tr2 = float(ss.item()) / (n - 1)
            tr, steps, ok = sqrtm_trace_device(m)
            sigma2 = None
        else:
            info['form'] = 'full'
            mu2, sigma2 = statistics_device(feats2)
            tr2 = _trace_device(sigma2)
            tr, steps, ok = _full_form(s1, sigma2, cache)
        info['steps'], info['converged'] = steps, ok
        if not ok:
            if sigma2 is None:
                mu2, sigma2 = statistics_device(feats2)
            return _fall_back(mu1, sigma1, mu2, sigma2, steps)
        diff = _host(mu1) - _host(mu2)
        return float(diff.dot(diff) + tr1 + tr2 - 2.0 * tr)


def calculate_frechet_distance_device(mu1, sigma1, mu2, sigma2, device=None, cache=None, info=None):
    """calculate_frechet_distance on the device in float64, full form: |mu1 - mu2|^2 + Tr S1 + Tr S2 - 2 Tr (R S2 R)^1/2, R = S1^1/2.
    Arguments are numpy arrays or float64 device tensors; cache / info as in frechet_distance_from_features."""
    d = _check_stats(mu1, sigma1)
    _check_stats(mu2, sigma2, d)
    tensors = [a for a in (mu1, sigma1, mu2, sigma2) if isinstance(a, torch.Tensor)]
    device = torch.device(device) if device is not None else (tensors[0].device if tensors else default_device(None))
    if device.type != 'cuda':
        raise ValueError('calculate_frechet_distance_device: a GPU device is required (got %s)' % (device,))
    cache = {} if cache is None else cache
    info = {} if info is None else info
    with torch.cuda.device(device):
        s1, tr1 = _real_side(cache, sigma1, device)
        s2 = _f64_device(sigma2, device)
        tr, steps, ok = _full_form(s1, s2, cache)
        info['form'], info['steps'], info['converged'] = 'full', steps, ok
        if not ok:
            return _fall_back(mu1, sigma1, mu2, sigma2, steps)
        diff = _host(mu1) - _host(mu2)
        return float(diff.dot(diff) + tr1 + _trace_device(s2) - 2.0 * tr)


# ---------------------------------------------------------------------------------------------------------------- the real-statistics writer
def load_images(path):
    """`path`: a directory of *.jpg / *.png of one size (sorted by name), or a .npy array [N, 3, H, W] in [-1, 1].  Returns (loader, N):
    loader(start, end) = float64 [B, H, W, 3] images in [0, 255], what get_real_stat.py hands over (tensor2im, then astype(float))."""
    if not os.path.exists(path):
        raise RuntimeError('Invalid path: %s' % path)
    if os.path.isdir(path):
        import glob
        files = sorted(glob.glob(os.path.join(path, '*.jpg')) + glob.glob(os.path.join(path, '*.png')))
        if not files:
            raise RuntimeError('no *.jpg / *.png under %s' % path)

        def load(start, end):
            from PIL import Image
            return np.stack([np.array(Image.open(f).convert('RGB')) for f in files[start:end]]).astype(float)
        return load, len(files)
    if not path.endswith('.npy'):
        raise RuntimeError('%s is neither a directory nor a .npy array' % path)
    arr = np.load(path, mmap_mode='r')
    if arr.ndim != 4 or arr.shape[1] != 3:
        raise RuntimeError('%s: expected an array [N, 3, H, W] in [-1, 1] (got %s)' % (path, arr.shape))

    def load(start, end):
        from . import tensor2im_batch
        return tensor2im_batch(torch.from_numpy(np.array(arr[start:end]))).astype(float)
    return load, arr.shape[0]


def real_statistics(path, model, batch_size=32, dims=2048, device=None, chunk_batches=16):
    """(mu, sigma) of an image set as float64 numpy arrays; the images are read `chunk_batches` batches at a time, the features and both
    statistics stay on the device"""
    load, n = load_images(path)
    device = default_device(device)
    feats = torch.empty((n, dims), dtype=torch.float32, device=device)
    step = batch_size * chunk_batches
    for start in range(0, n, step):
        end = min(start + step, n)
        feats[start:end] = get_activations_device(load(start, end), model, batch_size, dims, device)
    mu, sigma = statistics_device(feats)
    return mu.cpu().numpy(), sigma.cpu().numpy()


def parse_args(argv=None):
    from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
    parser = ArgumentParser(prog='python -m cat_amd.metric.fid_score', formatter_class=ArgumentDefaultsHelpFormatter,
                            description='Write the {mu, sigma} file of a real image set that --real_stat_path names')
    parser.add_argument('--images', type=str, required=True, help='a directory of *.jpg / *.png, or a .npy array [N, 3, H, W] in [-1, 1]')
    parser.add_argument('--output', type=str, required=True, help='the .npz file to write (keys mu, sigma; float64)')
    return add_inception_arguments(parser, batch_size=32).parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    print(args)
    if args.gpu == '':
        raise SystemExit('fid_score: --gpu must name a GPU; the kernels have no CPU path')
    device = torch.device('cuda', int(args.gpu))
    mu, sigma = real_statistics(args.images, load_inception(args.dims, args.inception_path, device, 'FID'), args.batch_size, args.dims, device)
    np.savez(args.output, mu=mu, sigma=sigma)
    print('wrote %s: mu %s, sigma %s' % (args.output, mu.shape, sigma.shape))


if __name__ == '__main__':
    main()
