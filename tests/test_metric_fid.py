"""CPU: the yardsticks and the fixture of FID's tail on the device (tests/fid_numpy.py, tests/golden/fid_frechet.npz), the argument checks
of cat_amd.metric.fid_score's device functions and its command line.  Nothing here touches a GPU."""
import json

import numpy as np
import pytest
import torch

import fid_numpy as FN
import helpers as H


@pytest.fixture(scope='module')
def golden():
    g = H.load('fid_frechet.npz')
    assert json.loads(str(g['cases'])) == FN.CASES
    return g


@pytest.fixture(scope='module')
def sets():
    """every small case's features and statistics, computed once"""
    out = {}
    for c in FN.CASES:
        f1, f2 = FN.case_features(c)
        out[c['name']] = (f1, f2) + FN.stats(f1)
    return out


@pytest.mark.parametrize('case', FN.CASES, ids=lambda c: c['name'])
def test_features_are_the_fixtures(golden, sets, case):
    f1, f2 = sets[case['name']][:2]
    assert f1.shape == (case['n1'], case['d']) and f2.shape == (case['n2'], case['d'])
    assert f1.min() >= 0 and np.array_equal(f1, f1.astype(np.float32).astype(np.float64))
    got = np.array([FN.checksum(f1), FN.checksum(f2)])
    assert np.allclose(got, golden[case['name'] + '_checksums'], rtol=1e-12, atol=0)


@pytest.mark.parametrize('case', FN.CASES, ids=lambda c: c['name'])
def test_iteration_agrees_with_the_eigenvalue_yardstick(golden, sets, case):
    """Tr M^1/2 by the Newton-Schulz restatement against the sum of sqrt(eigvalsh(M)) on the same M, through the distance: within
    1e-10 * (Tr S1 + Tr S2).  Measured here: 0 to 7.2e-15 of that scale, in 7 to 21 steps.  (With the yardstick's eigenvalues clipped at
    exactly 0 instead of at eigh's noise floor the gap is up to 8e-9 -- full_s1_singular -- and all of it is the yardstick's: see
    tests/fid_numpy.py.)"""
    f1, f2, mu1, s1 = sets[case['name']]
    steps = []

    def tr(m):
        v, s, ok = FN.nsqrt_trace(m)
        assert ok and s < FN.MAX_STEPS
        steps.append(s)
        return v
    fd_ns = FN._frechet(mu1, s1, f2, tr)
    fd_eigh = FN.frechet_eigh(mu1, s1, f2)
    scale = float(golden[case['name'] + '_tr'])
    assert abs(scale - (np.trace(s1) + np.trace(np.cov(f2, rowvar=False)))) <= 1e-12 * scale
    print('%s: |fd_ns - fd_eigh| / tr = %.2e in %s steps' % (case['name'], abs(fd_ns - fd_eigh) / scale, steps))
    assert abs(fd_ns - fd_eigh) <= 1e-10 * scale


@pytest.mark.parametrize('case', FN.CASES, ids=lambda c: c['name'])
def test_yardstick_is_the_references_number_up_to_its_own_gap(golden, sets, case):
    f1, f2, mu1, s1 = sets[case['name']]
    n = case['name']
    fd_eigh = FN.frechet_eigh(mu1, s1, f2)
    scale, gap = float(golden[n + '_tr']), float(golden[n + '_ref_gap'])
    assert abs(fd_eigh - float(golden[n + '_fd_eigh'])) <= 1e-10 * scale          # eigvalsh here and where the fixture was written
    assert abs(fd_eigh - float(golden[n + '_fd_reference'])) <= 2 * gap + 1e-10 * scale


def test_iteration_reproduces_the_recorded_host_distance():
    """inception_fid.npz's fd (the reference's calculate_frechet_distance on two 40 x 16 sets) through the full form and the iteration"""
    g = H.load('inception_fid.npz')
    f1, f2 = g['fd_f1'], g['fd_f2']
    mu1, s1 = FN.stats(f1)
    fd, steps = FN.frechet_ns(mu1, s1, f2)
    assert f2.shape[0] > f2.shape[1] and len(steps) == 2
    assert abs(fd - float(g['fd'])) <= 1e-9 * abs(float(g['fd']))


def test_zero_matrix_has_a_zero_root():
    assert FN.nsqrt_trace(np.zeros((4, 4))) == (0.0, 0, True)


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_raise_before_any_device_call(monkeypatch):
    from cat_amd import _lib
    from cat_amd.metric import fid_score as F

    def no_device(*a, **k):
        raise AssertionError('a device call was made')
    monkeypatch.setattr(_lib, 'call', no_device)
    monkeypatch.setattr(_lib, 'query', no_device)
    mu, sigma = np.zeros(8), np.eye(8)
    ok = torch.zeros((4, 8), dtype=torch.float32)
    with pytest.raises(ValueError, match='at least 2'):
        F.statistics_device(torch.zeros((1, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match='multiple of 4'):
        F.statistics_device(torch.zeros((4, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match='float32'):
        F.statistics_device(torch.zeros((4, 8), dtype=torch.float64))
    with pytest.raises(ValueError, match=r'\[n, d\]'):
        F.statistics_device(np.zeros((4, 8), dtype=np.float32))
    with pytest.raises(ValueError, match='at least 2'):
        F.frechet_distance_from_features(mu, sigma, ok[:1])
    with pytest.raises(ValueError, match='multiple of 4'):
        F.frechet_distance_from_features(np.zeros(6), np.eye(6), torch.zeros((4, 6), dtype=torch.float32))
    with pytest.raises(ValueError, match='8 wide'):
        F.frechet_distance_from_features(mu, sigma, torch.zeros((4, 12), dtype=torch.float32))
    with pytest.raises(ValueError, match='float64'):
        F.frechet_distance_from_features(mu.astype(np.float32), sigma, ok)
    with pytest.raises(ValueError, match='belong together'):
        F.frechet_distance_from_features(mu, np.eye(8)[:, :4], ok)
    with pytest.raises(ValueError, match='belong together'):
        F.calculate_frechet_distance_device(mu, sigma, np.zeros(12), np.eye(8))
    with pytest.raises(ValueError, match='12 wide'):
        F.calculate_frechet_distance_device(mu, sigma, np.zeros(12), np.eye(12))
    with pytest.raises(ValueError, match='multiple of 4'):
        F.calculate_frechet_distance_device(np.zeros(6), np.eye(6), np.zeros(6), np.eye(6))
    with pytest.raises(ValueError, match='float64'):
        F.calculate_frechet_distance_device(mu, sigma, mu, sigma.astype(np.float32))
    with pytest.raises(ValueError, match='square float64'):
        F.sqrtm_trace_device(torch.zeros((4, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match='square float64'):
        F.sqrtm_trace_device(torch.zeros((4, 4), dtype=torch.float32))


def test_get_fid_and_attach_fid_refuse_an_unknown_choice():
    from types import SimpleNamespace
    from cat_amd import metric
    from cat_amd.distillers import evaluation as E
    with pytest.raises(ValueError, match="'host' or 'device'"):
        metric.get_fid([], None, {}, frechet='gpu')
    with pytest.raises(ValueError, match="'host' or 'device'"):
        E.attach_fid(SimpleNamespace(), {}, npz={}, frechet='gpu')


def test_host_functions_keep_their_defaults():
    import inspect
    from cat_amd import metric
    from cat_amd.distillers import evaluation as E
    assert inspect.signature(metric.get_fid).parameters['frechet'].default == 'host'
    assert inspect.signature(E.attach_fid).parameters['frechet'].default == 'host'


# ---------------------------------------------------------------------------------------------------------------- command line
def test_command_line_parses():
    from cat_amd.metric import fid_score as F
    a = F.parse_args(['--images', 'real', '--output', 'x.npz', '--inception-path', 'ckpt.pth'])
    assert (a.images, a.output, a.inception_path, a.batch_size, a.dims, a.gpu) == ('real', 'x.npz', 'ckpt.pth', 32, 2048, '0')
    a = F.parse_args(['--images', 'r.npy', '--output', 'x.npz', '--inception-path', 'c', '--batch-size', '4', '--dims', '192', '--gpu', '1'])
    assert (a.batch_size, a.dims, a.gpu) == (4, 192, '1')
    for bad in (['--output', 'x.npz', '--inception-path', 'c'], ['--images', 'r', '--inception-path', 'c'], ['--images', 'r', '--output', 'x'],
                ['--images', 'r', '--output', 'x', '--inception-path', 'c', '--dims', '100']):
        with pytest.raises(SystemExit):
            F.parse_args(bad)


def test_image_loader_gives_what_the_reference_hands_over(tmp_path):
    """a folder of PNGs and a .npy array in [-1, 1] both become float64 [B, H, W, 3] in [0, 255] (tensor2im, then astype(float))"""
    from PIL import Image
    from cat_amd.metric import fid_score as F, tensor2im_batch
    ims = np.random.RandomState(3).randint(0, 256, size=(3, 8, 12, 3)).astype(np.uint8)
    for i, im in enumerate(ims):
        Image.fromarray(im).save(str(tmp_path / ('im%d.png' % i)))
    load, n = F.load_images(str(tmp_path))
    got = load(0, 3)
    assert n == 3 and got.dtype == np.float64 and np.array_equal(got, ims.astype(float))
    arr = np.random.RandomState(4).uniform(-1.2, 1.2, size=(5, 3, 8, 12)).astype(np.float32)
    np.save(str(tmp_path / 'a.npy'), arr)
    load, n = F.load_images(str(tmp_path / 'a.npy'))
    assert n == 5 and np.array_equal(load(1, 4), tensor2im_batch(torch.from_numpy(arr[1:4])).astype(float))
    with pytest.raises(RuntimeError, match='Invalid path'):
        F.load_images(str(tmp_path / 'missing'))
