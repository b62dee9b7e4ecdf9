"""GPU: FID's statistics and Frechet distance on the device (csrc/fid_ops.hip, cat_amd/metric/fid_score.py).

A: cat_fid_stats against np.mean / np.cov (tests/fid_numpy.stats): |d mu_j| <= 1e-13 max|F|, |d sigma_ij| <= 1e-12 sqrt(sigma_ii sigma_jj) +
   1e-13 max|sigma| -- a centred sum of n products in any order is within n 2^-53 of sum|a||b| <= (n - 1) sqrt(sigma_ii sigma_jj) on both
   sides, 6.7e-14 at n = 300, tenfold margin.  sigma equals its transpose bit for bit, two launches give the same bits, outputs pre-filled
   with NaN, n = 1 and d = 6 refused.
B: cat_gemm_f64 against numpy: |d C_ij| <= 4 k 2^-53 (|A||B|)_ij + tiny (gamma_k on each side; tiny = 2^-52 |beta_eye| for the epilogue's
   one addition on each side), both transB values, both (alpha, beta_eye) pairs, leading dimensions larger than the rows with NaN in the
   padding of every operand and of C.  The issue's shapes all take the 32 x 32 tile; (1030, 1029, 36) takes the 64 x 64 one.
C: frechet_distance_from_features and calculate_frechet_distance_device on every case of tests/golden/fid_frechet.npz.
   Bound T = (10 rho + d 2^-53) (Tr S1 + Tr S2): rho = the largest |fd - fd_eigh| / (Tr S1 + Tr S2) of the float64 numpy restatement of
   the same algorithm (tests/fid_numpy.nsqrt), measured on the CPU over the seven cases -- the algorithm's own distance to the yardstick,
   independent of the code under test -- and d 2^-53 the rounding of one product of length d.  Measured, per case in the fixture's order:
     frechet_ns (Gram form where n <= d, as frechet_distance_from_features):   0, 2.0e-16, 1.0e-15, 7.1e-17, 0, 2.1e-16, 7.2e-15
     full form throughout (as calculate_frechet_distance_device):              5.3e-15, 1.6e-15, 1.0e-15, 7.1e-17, 4.3e-16, 0, 4.4e-14
   so rho = 7.2e-15 and 4.4e-14.  Against the reference's own number: 2 ref_gap + T.  Against inception_fid.npz's recorded fd: 1e-9 |fd|.
   Measured on the MI355X, |fd - fd_eigh| per case in the fixture's order (absolute; T is 1.2e-12 to 3.7e-10):
     frechet_distance_from_features:       1.8e-14, 5.3e-15, 1.1e-13, 1.8e-14, 2.8e-13, 1.1e-13, 8.5e-14   in 15, 15, 13+15, 15+19, 12, 7, 21 steps
     calculate_frechet_distance_device:    5.7e-14, 2.3e-14, 1.1e-13, 1.8e-14, 1.1e-13, 1.1e-13, 8.5e-13   in 27 to 35 steps for both roots
   and |fd - fd_reference| = ref_gap to the printed digits in every case; inception_fid.npz's fd to 4.4e-15 relative.
D: get_fid(..., frechet='device') against frechet='host' on the seeded InceptionV3 (bound: the fixture's 2 ref_gap + T of the (64, 4, 2048)
   case, relative to that case's distance), and through attach_fid / evaluate_model.
E: the real-statistics writer in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fid_numpy as FN
import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
RHO_FEATURES, RHO_FULL = 7.2e-15, 4.4e-14

STATS_CASES = [(2, 64), (17, 64), (40, 16), (65, 192), (33, 68), (300, 2048)]
GEMM_CASES = [(16, 16, 4), (17, 15, 5), (64, 64, 32), (65, 63, 36), (130, 130, 200), (120, 2048, 2048), (1030, 1029, 36)]


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _nan(shape, dev, dtype=torch.float64):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _assert_stats_close(mu, sigma, want_mu, want_sigma, fmax, tag):
    dm = float(np.abs(mu - want_mu).max())
    sd = np.sqrt(np.diagonal(want_sigma))
    bound = 1e-12 * np.outer(sd, sd) + 1e-13 * np.abs(want_sigma).max()
    ds = np.abs(sigma - want_sigma)
    print('%s: |d mu| %.2e (bound %.2e), worst |d sigma| / bound %.3f' % (tag, dm, 1e-13 * fmax, float((ds / bound).max())))
    assert dm <= 1e-13 * fmax
    assert (ds <= bound).all()


# ---------------------------------------------------------------------------------------------------------------- A: statistics
_STATS = {}


def _stats_case(case):
    if case not in _STATS:
        n, d = case
        f = FN.features(3000 + n + d, n, d, shift=0.1)
        _STATS[case] = (f,) + FN.stats(f)
    return _STATS[case]


def _launch_stats(f, dev):
    from cat_amd import _lib as L, ops
    n, d = f.shape
    fd = torch.from_numpy(f.astype(np.float32)).to(dev)
    mu, sigma = _nan((d,), dev), _nan((d, d), dev)
    L.call('cat_fid_stats', ops._p(fd), n, d, ops._p(mu), ops._p(sigma), ops._stream())
    torch.cuda.synchronize()
    return mu, sigma


@pytest.mark.parametrize('case', STATS_CASES, ids=lambda c: 'n%d_d%d' % c)
def test_stats_against_numpy(dev, case):
    f, want_mu, want_sigma = _stats_case(case)
    mu, sigma = _launch_stats(f, dev)
    assert not bool(torch.isnan(mu).any()) and not bool(torch.isnan(sigma).any())          # every element was written
    assert torch.equal(sigma, sigma.t())
    _assert_stats_close(mu.cpu().numpy(), sigma.cpu().numpy(), want_mu, want_sigma, float(f.max()), 'stats n=%d d=%d' % case)
    mu2, sigma2 = _launch_stats(f, dev)
    assert torch.equal(mu, mu2) and torch.equal(sigma, sigma2)


def test_statistics_device_is_the_same_call(dev):
    from cat_amd.metric import fid_score as F
    f, _, _ = _stats_case((33, 68))
    mu, sigma = _launch_stats(f, dev)
    mu2, sigma2 = F.statistics_device(torch.from_numpy(f.astype(np.float32)).to(dev))
    assert mu2.dtype == torch.float64 and sigma2.shape == (68, 68) and torch.equal(mu, mu2) and torch.equal(sigma, sigma2)


def test_stats_refuse_what_they_do_not_compute(dev):
    from cat_amd import _lib as L, ops
    from cat_amd.metric import fid_score as F
    x = torch.zeros((8, 8), dtype=torch.float32, device=dev)
    out = torch.zeros(64, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match='at least 2'):
        L.call('cat_fid_stats', ops._p(x), 1, 8, ops._p(out), ops._p(out), ops._stream())
    with pytest.raises(RuntimeError, match='multiple of 4'):
        L.call('cat_fid_stats', ops._p(x), 8, 6, ops._p(out), ops._p(out), ops._stream())
    with pytest.raises(ValueError, match='at least 2'):
        F.statistics_device(x[:1])
    with pytest.raises(ValueError, match='multiple of 4'):
        F.statistics_device(x[:, :6].contiguous())


def test_center_writes_the_rows_and_their_sum_of_squares(dev):
    from cat_amd import _lib as L, ops
    f, want_mu, want_sigma = _stats_case((65, 192))
    n, d = f.shape
    fd = torch.from_numpy(f.astype(np.float32)).to(dev)
    mu = torch.from_numpy(want_mu).to(dev)
    xc, ss = _nan((n, d), dev), _nan((1,), dev)
    ws = _nan((L.query('cat_fid_center_ws_bytes', n) // 8,), dev)
    L.call('cat_fid_center', ops._p(fd), ops._p(mu), n, d, ops._p(xc), ops._p(ss), ops._p(ws), ops._stream())
    assert np.array_equal(xc.cpu().numpy(), f - want_mu)                                   # one subtraction per element: the same bits
    want = ((f - want_mu) ** 2).sum()
    assert abs(float(ss.item()) - want) <= n * d * U * want
    assert abs(float(ss.item()) / (n - 1) - np.trace(want_sigma)) <= 1e-12 * np.trace(want_sigma)


# ---------------------------------------------------------------------------------------------------------------- B: the product
_GEMM = {}


def _gemm_case(shape):
    """operands in [-1, 1) with padded leading dimensions, and the numpy products, once per shape"""
    if shape not in _GEMM:
        m, n, k = shape
        rs = np.random.RandomState(4000 + m + n + k)
        a, b = rs.uniform(-1, 1, (m, k)), rs.uniform(-1, 1, (k, n))
        _GEMM[shape] = (a, b, a.dot(b), np.abs(a).dot(np.abs(b)))
    return _GEMM[shape]


def _padded(x, pad, dev):
    t = _nan((x.shape[0], x.shape[1] + pad), dev)
    t[:, :x.shape[1]] = torch.from_numpy(x).to(dev)
    return t


def _launch_gemm(a, b, trans_b, alpha, beta_eye, dev):
    from cat_amd import _lib as L, ops
    m, k = a.shape
    n = b.shape[1]
    ad = _padded(a, 3, dev)
    bd = _padded(np.ascontiguousarray(b.T) if trans_b else b, 5, dev)
    cd = _nan((m, n + 1), dev)
    L.call('cat_gemm_f64', ops._p(ad), ad.shape[1], ops._p(bd), bd.shape[1], int(trans_b), ops._p(cd), cd.shape[1], m, n, k, alpha, beta_eye,
           ops._stream())
    torch.cuda.synchronize()
    return cd


@pytest.mark.parametrize('trans_b', [False, True], ids=['nn', 'nt'])
@pytest.mark.parametrize('shape', GEMM_CASES, ids=lambda s: 'm%d_n%d_k%d' % s)
def test_gemm_against_numpy(dev, shape, trans_b):
    a, b, prod, mag = _gemm_case(shape)
    m, n, k = shape
    for alpha, beta_eye in ((1.0, 0.0), (-0.5, 1.5)):
        cd = _launch_gemm(a, b, trans_b, alpha, beta_eye, dev)
        assert bool(torch.isnan(cd[:, n]).all()) and not bool(torch.isnan(cd[:, :n]).any())          # all of C and nothing beyond it
        got = cd[:, :n].cpu().numpy()
        want = alpha * prod + beta_eye * np.eye(m, n)
        bound = 4 * k * U * mag + 2 * U * abs(beta_eye) + 1e-300
        err = np.abs(got - want)
        print('gemm %s %s alpha %g: worst |d C| / bound %.3f' % (shape, 'nt' if trans_b else 'nn', alpha, float((err / bound).max())))
        assert (err <= bound).all()
    again = _launch_gemm(a, b, trans_b, -0.5, 1.5, dev)
    assert torch.equal(again[:, :n], cd[:, :n])


def test_gemm_and_small_kernels_refuse_bad_arguments(dev):
    from cat_amd import _lib as L, ops
    a = torch.zeros((8, 8), dtype=torch.float64, device=dev)
    c = torch.zeros((8, 8), dtype=torch.float64, device=dev)

    def gemm(A, lda, B, ldb, tb, Cm, ldc, m, n, k):
        L.call('cat_gemm_f64', ops._p(A), lda, ops._p(B), ldb, tb, ops._p(Cm), ldc, m, n, k, 1.0, 0.0, ops._stream())
    with pytest.raises(RuntimeError, match='alias'):
        gemm(a, 8, a, 8, 0, a, 8, 8, 8, 8)
    with pytest.raises(RuntimeError, match='leading'):
        gemm(a, 4, a, 8, 0, c, 8, 8, 8, 8)
    with pytest.raises(RuntimeError, match='geometry'):
        gemm(a, 8, a, 8, 0, c, 8, 0, 8, 8)
    with pytest.raises(RuntimeError, match='transB'):
        gemm(a, 8, a, 8, 2, c, 8, 8, 8, 8)
    with pytest.raises(RuntimeError, match='workspace'):
        L.call('cat_f64_trace_sumsq', ops._p(a), 8, 8, 1, ops._p(c), None, ops._stream())


def test_trace_sumsq_and_symmetrize(dev):
    from cat_amd import _lib as L, ops
    for n, pad in ((1, 0), (5, 2), (130, 1), (300, 0)):
        x = np.random.RandomState(50 + n).uniform(-1, 1, (n, n))
        xd = _padded(x, pad, dev)
        out = _nan((2,), dev)
        ws = _nan((L.query('cat_f64_trace_sumsq_ws_bytes', n) // 8,), dev)
        L.call('cat_f64_trace_sumsq', ops._p(xd), n, n + pad, 1, ops._p(out), ops._p(ws), ops._stream())
        tr, ss = out.tolist()
        assert abs(tr - np.trace(x)) <= n * U * np.abs(np.diagonal(x)).sum() and abs(ss - (x * x).sum()) <= n * n * U * (x * x).sum()
        assert not bool(torch.isnan(ws).any())
        out2 = _nan((2,), dev)
        L.call('cat_f64_trace_sumsq', ops._p(xd), n, n + pad, 0, ops._p(out2), None, ops._stream())
        assert out2[0].item() == tr and np.isnan(out2[1].item())
        sd = _nan((n, n + 3), dev)
        L.call('cat_f64_symmetrize', ops._p(xd), n, n + pad, 0.25, ops._p(sd), n + 3, ops._stream())
        got = sd[:, :n].cpu().numpy()
        assert np.array_equal(got, got.T) and np.array_equal(got, 0.25 * (0.5 * (x + x.T))) and bool(torch.isnan(sd[:, n:]).all())
        L.call('cat_f64_symmetrize', ops._p(xd), n, n + pad, 0.25, ops._p(xd), n + pad, ops._stream())          # in place
        assert np.array_equal(xd[:, :n].cpu().numpy(), got)


# ---------------------------------------------------------------------------------------------------------------- C: the distance
@pytest.fixture(scope='module')
def golden():
    g = H.load('fid_frechet.npz')
    assert json.loads(str(g['cases'])) == FN.CASES
    return g


_SETS = {}


def _case_sets(c):
    if c['name'] not in _SETS:
        f1, f2 = FN.case_features(c)
        _SETS[c['name']] = (f1, f2) + FN.stats(f1) + FN.stats(f2)
    return _SETS[c['name']]


def _check_distance(fd, info, golden, c, rho, tag):
    n = c['name']
    scale, fd_eigh, fd_ref, gap = (float(golden[n + k]) for k in ('_tr', '_fd_eigh', '_fd_reference', '_ref_gap'))
    T = (10 * rho + c['d'] * U) * scale
    print('%s %s: fd %.12g, |fd - fd_eigh| %.2e (T %.2e), |fd - fd_reference| %.2e (ref_gap %.2e), form %s, %d steps' % (
        tag, n, fd, abs(fd - fd_eigh), T, abs(fd - fd_ref), gap, info['form'], info['steps']))
    assert info['converged'] and info['steps'] < 100
    assert abs(fd - fd_eigh) <= T
    assert abs(fd - fd_ref) <= 2 * gap + T
    if n == 'identical':
        assert abs(fd) <= 1e-9 * scale


@pytest.mark.parametrize('case', FN.CASES, ids=lambda c: c['name'])
def test_frechet_distance_from_features(dev, golden, case):
    from cat_amd.metric import fid_score as F
    f1, f2, mu1, s1, _, _ = _case_sets(case)
    feats = torch.from_numpy(f2.astype(np.float32)).to(dev)
    info, cache = {}, {}
    fd = F.frechet_distance_from_features(mu1, s1, feats, cache=cache, info=info)
    assert info['form'] == ('gram' if case['n2'] <= case['d'] else 'full')
    _check_distance(fd, info, golden, case, RHO_FEATURES, 'from_features')
    # device statistics and the cache the first call filled: the same number, bit for bit
    again = F.frechet_distance_from_features(torch.from_numpy(mu1).to(dev), torch.from_numpy(s1).to(dev), feats, cache=cache)
    assert again == fd


@pytest.mark.parametrize('case', FN.CASES, ids=lambda c: c['name'])
def test_calculate_frechet_distance_device(dev, golden, case):
    from cat_amd.metric import fid_score as F
    _, _, mu1, s1, mu2, s2 = _case_sets(case)
    info = {}
    fd = F.calculate_frechet_distance_device(mu1, s1, mu2, s2, device=dev, info=info)
    assert info['form'] == 'full'
    _check_distance(fd, info, golden, case, RHO_FULL, 'full_form')


def test_recorded_host_distance_of_the_inception_fixture(dev):
    from cat_amd.metric import fid_score as F
    g = H.load('inception_fid.npz')
    info = {}
    fd = F.calculate_frechet_distance_device(*(FN.stats(g['fd_f1']) + FN.stats(g['fd_f2'])), device=dev, info=info)
    print('inception_fid.npz: fd %.15g, recorded %.15g, rel %.2e, %d steps' % (fd, float(g['fd']), abs(fd / float(g['fd']) - 1), info['steps']))
    assert info['converged'] and abs(fd - float(g['fd'])) <= 1e-9 * abs(float(g['fd']))


def test_sqrtm_trace_device(dev):
    from cat_amd.metric import fid_score as F
    c = FN.CASES[1]
    f1, f2, mu1, s1, _, _ = _case_sets(c)
    m, _ = FN.gram_matrix(s1, f2)
    want, want_steps, _ = FN.nsqrt_trace(m)
    tr, steps, ok = F.sqrtm_trace_device(torch.from_numpy(m).to(dev))
    assert ok and abs(steps - want_steps) <= 2 and abs(tr - want) <= (10 * RHO_FEATURES + c['d'] * U) * want
    assert F.sqrtm_trace_device(torch.zeros((8, 8), dtype=torch.float64, device=dev)) == (0.0, 0, True)


def test_no_convergence_falls_back_to_the_host_with_a_warning(dev, golden, monkeypatch, capsys):
    """a cap of 3 steps stands in for an iteration that does not converge"""
    from cat_amd.metric import fid_score as F
    c = FN.CASES[1]
    f1, f2, mu1, s1, mu2, s2 = _case_sets(c)
    monkeypatch.setattr(F, 'NS_MAX_STEPS', 3)
    want = float(F.calculate_frechet_distance(mu1, s1, mu2, s2))
    capsys.readouterr()
    info = {}
    fd = F.frechet_distance_from_features(mu1, s1, torch.from_numpy(f2.astype(np.float32)).to(dev), info=info)
    assert 'did not converge' in capsys.readouterr().out and info['converged'] is False
    # the host function on the device's statistics: scipy's sqrtm of a singular product answers a 1e-13 change of its input with a change
    # of the size of its own error, the fixture's ref_gap
    assert abs(fd - want) <= 2 * float(golden[c['name'] + '_ref_gap']) + 1e-9 * abs(want)
    info = {}
    fd = F.calculate_frechet_distance_device(mu1, s1, mu2, s2, device=dev, info=info)
    assert 'did not converge' in capsys.readouterr().out and info['converged'] is False and fd == want
    assert np.isnan(F.sqrtm_trace_device(torch.from_numpy(s1).to(dev))[0])


# ---------------------------------------------------------------------------------------------------------------- D: get_fid, evaluate_model
@pytest.fixture(scope='module')
def seeded():
    """(state_dict, InceptionV3([3]) on the GPU) with the seeded weights of tests/golden/inception_fid.npz"""
    from cat_amd.metric import InceptionV3
    from oracle import ref_inception_cpu as RI
    g = H.load('inception_fid.npz')
    sd = RI.seeded_state_dict(H.sd_from_shapes(g['shapes']), int(g['seed_w']))
    net = InceptionV3([3])
    net.load_fid_state_dict(sd)
    return sd, net.to(torch.device('cuda:0')).eval()


def _real_npz():
    """the recipe of test_evaluate_model_computes_fid_on_the_gpu: a seeded 64 x 2048 real set"""
    feats = np.random.default_rng(11).standard_normal((64, 2048))
    return {'mu': feats.mean(0), 'sigma': np.cov(feats, rowvar=False)}


def _relative_bound(golden):
    """the (64, 4, 2048) case's bound against the reference, 2 ref_gap + T, relative to that case's distance"""
    c = next(c for c in FN.CASES if c['name'] == 'gram_evaluate_model')
    n = c['name']
    T = (10 * RHO_FEATURES + c['d'] * U) * float(golden[n + '_tr'])
    return (2 * float(golden[n + '_ref_gap']) + T) / float(golden[n + '_fd_reference'])


def test_get_fid_on_the_device_equals_the_host_path(dev, seeded, golden):
    from cat_amd import metric
    from oracle import detfill
    _, net = seeded
    npz = _real_npz()
    fakes = [detfill.images((3, 3, 40, 56), 710)]
    host = metric.get_fid(fakes, net, npz, device=dev, batch_size=2, use_tqdm=False)
    device = metric.get_fid(fakes, net, npz, device=dev, batch_size=2, use_tqdm=False, frechet='device')
    rel = _relative_bound(golden)
    print('get_fid host %.10g, device %.10g, rel %.2e (bound %.2e)' % (host, device, abs(device / host - 1), rel))
    assert abs(device - host) <= rel * abs(host)


def test_evaluate_model_with_the_distance_on_the_device(dev, tmp_path, monkeypatch):
    from cat_amd import metric
    from cat_amd.distillers import evaluation as E
    from oracle import detfill, ref_inception_cpu as RI
    g = H.load('inception_fid.npz')
    sd = RI.seeded_state_dict(H.sd_from_shapes(g['shapes']), int(g['seed_w']))
    gs = H.load('step_in.npz')
    meta = json.loads(str(gs['meta']))
    opt = H.make_opt(norm='instance', track=False, ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                     lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16)
    opt.log_dir, opt.eval_batch_size = str(tmp_path), 2
    model = H.build_distiller(opt, gs['student_shapes'])
    npz = _real_npz()
    batches = [{'A': detfill.images((2, 3, 64, 64), 500 + i), 'B': detfill.images((2, 3, 64, 64), 600 + i),
                'A_paths': ['a%d_%d.png' % (i, j) for j in range(2)], 'B_paths': ['b%d_%d.png' % (i, j) for j in range(2)]} for i in range(2)]
    model.eval_dataloader = batches
    # without the argument the fid_fn that evaluate builds is today's call of get_fid (recorded here, not run: test_metric_inception.py runs it)
    E.attach_fid(model, sd, npz=npz)
    assert model.fid_frechet == 'host' and not hasattr(model, 'npz_device')
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(metric, 'get_fid', lambda *a, **k: calls.append((a, k)) or 10.0)
        model.best_fid, model.fids, model.is_best = 1e9, [], False
        assert model.evaluate_model(0)['metric/fid'] == 10.0
    (args, kwargs), = calls
    fakes = args[0]
    assert args[1] is model.inception_model and args[2] is npz and kwargs == dict(device=model.device, batch_size=2, use_tqdm=False)
    # opted in: get_fid(..., frechet='device') on the uploaded statistics, with the bookkeeping as before
    model.fid_fn = None
    E.attach_fid(model, sd, npz=npz, frechet='device')
    assert model.fid_frechet == 'device' and model.npz_device['sigma'].is_cuda and model.npz_device['sigma'].dtype == torch.float64
    model.best_fid, model.fids, model.is_best = 1e9, [], False
    ret = model.evaluate_model(0)
    want = metric.get_fid(fakes, model.inception_model, npz, device=model.device, batch_size=2, use_tqdm=False, frechet='device')
    print('evaluate_model FID on the device %.10g, get_fid on the same fakes %.10g' % (ret['metric/fid'], want))
    assert ret['metric/fid'] == want and np.isfinite(want) and want > 0
    assert model.is_best and ret['metric/fid-best'] == ret['metric/fid'] == ret['metric/fid-mean'] and 'sigma1' in model.fid_cache
    second = model.evaluate_model(1)
    assert second['metric/fid'] == ret['metric/fid'] and not model.is_best and second['metric/fid-mean'] == ret['metric/fid']


# ---------------------------------------------------------------------------------------------------------------- E: the command line
def test_real_statistics_writer_in_a_fresh_process(dev, seeded, tmp_path):
    from PIL import Image
    from cat_amd.metric import get_activations_from_ims
    sd, net = seeded
    ckpt = str(tmp_path / 'pt_inception_seeded.pth')
    torch.save(sd, ckpt)
    ims = np.random.RandomState(9).randint(0, 256, size=(4, 40, 56, 3)).astype(np.uint8)
    os.makedirs(str(tmp_path / 'real'))
    for i, im in enumerate(ims):
        Image.fromarray(im).save(str(tmp_path / 'real' / ('im%03d.png' % i)))
    out = str(tmp_path / 'real_stat.npz')
    cmd = [sys.executable, '-m', 'cat_amd.metric.fid_score', '--images', str(tmp_path / 'real'), '--output', out, '--batch-size', '2', '--gpu', '0',
           '--inception-path', ckpt]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    z = np.load(out)
    assert sorted(z.files) == ['mu', 'sigma'] and z['mu'].shape == (2048,) and z['sigma'].shape == (2048, 2048)
    assert z['mu'].dtype == np.float64 and z['sigma'].dtype == np.float64
    act = get_activations_from_ims(ims.astype(float), net, batch_size=2, dims=2048, device=dev, use_tqdm=False)
    _assert_stats_close(z['mu'], z['sigma'], np.mean(act, axis=0), np.cov(act, rowvar=False), float(act.max()), 'writer')
