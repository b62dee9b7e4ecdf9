"""CPU: the host half of the kernel inception distance (cat_amd/metric/kid_score.py) against the REFERENCE's own run.

tests/golden/kid.npz was written by tools/make_golden_kid.py from the reference's metric/kid_score.py (polynomial_mmd_averages and
_mmd2_and_variance under its three estimators) on the seeded features of tests/kid_numpy.py.  Here the sums the GPU kernel would deliver come
from numpy (kid_numpy.poly_sums); what is checked is everything around the kernel: the closed-form estimator on those sums, the order in
which the subsets are drawn, the image bookkeeping of get_activations, argument checks and the command line.

Bounds.  kid_numpy's kernels differ from sklearn's only in BLAS summation order: <= d * 2^-53 = 2.3e-13 relative per dot product of
non-negative features, three times that after the cube, kept by sums of positive terms.  mmd2 is a combination of means of K with
coefficients of order 1, so |d mmd2| <= 1e-11 * scale with scale = mean K_XX + mean K_YY + 2 mean K_XY has a tenfold margin; the variance
estimate is a combination of products of two such means, |d var| <= 1e-10 * scale^2."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H
import kid_numpy as KN


@pytest.fixture(scope='module')
def golden():
    g = H.load('kid.npz')
    assert json.loads(str(g['cases'])) == KN.CASES and tuple(json.loads(str(g['estimators']))) == KN.ESTIMATORS
    return g


@pytest.fixture(scope='module')
def case_sums():
    """per case: (x, y, gi, ri, numpy sums), computed once"""
    from cat_amd.metric import kid_score as K
    out = {}
    for c in KN.CASES:
        x, y = KN.features(c['seed'], c['nx'], c['ny'], c['d'])
        np.random.seed(c['draw_seed'])
        gi, ri = K.draw_subsets(len(x), len(y), c['S'], c['m'])
        out[c['name']] = (x, y, gi, ri, KN.poly_sums(x, y, gi, ri, **c['kernel']))
    return out


@pytest.mark.parametrize('case', KN.CASES, ids=lambda c: c['name'])
def test_estimator_on_numpy_sums_reproduces_the_reference(golden, case_sums, case):
    from cat_amd.metric import kid_score as K
    x, y, gi, ri, sums = case_sums[case['name']]
    m, m_all = case['m'], min(case['nx'], case['ny'])
    scale = KN.scale_of(sums, m)
    est = golden[case['name'] + '_est']
    for s in range(case['S']):
        one = {k: v[s] for k, v in sums.items()}
        for e, name in enumerate(KN.ESTIMATORS):
            mmd2, var = K.mmd2_and_variance_from_sums(one, mmd_est=name, var_at_m=m_all)
            assert abs(mmd2 - est[s, e, 0]) <= 1e-11 * scale[s], (name, mmd2, est[s, e, 0])
            assert abs(var - est[s, e, 1]) <= 1e-10 * scale[s] ** 2, (name, var, est[s, e, 1])
            assert K.mmd2_and_variance_from_sums(one, mmd_est=name, var_at_m=m_all, ret_var=False) == mmd2
        # what polynomial_mmd_averages reports is the 'unbiased' estimate at var_at_m = min(len(g), len(r))
        assert est[s, 1, 0] == golden[case['name'] + '_mmds'][s] and est[s, 1, 1] == golden[case['name'] + '_vars'][s]
    # var_at_m defaults to the subset size, and only scales the variance
    one = {k: v[0] for k, v in sums.items()}
    a, va = K.mmd2_and_variance_from_sums(one)
    b, vb = K.mmd2_and_variance_from_sums(one, var_at_m=m)
    assert (a, va) == (b, vb) and a == K.mmd2_and_variance_from_sums(one, var_at_m=m_all)[0]


def test_unit_diagonal_and_unknown_estimator(case_sums):
    from cat_amd.metric import kid_score as K
    one = {k: v[0] for k, v in case_sums['ragged'][4].items()}
    unit = dict(one, dg_xx=np.ones(37), dg_yy=np.ones(37))
    assert K.mmd2_and_variance_from_sums(one, unit_diagonal=True) == K.mmd2_and_variance_from_sums(unit)
    with pytest.raises(AssertionError):
        K.mmd2_and_variance_from_sums(one, mmd_est='median')


def test_subsets_are_drawn_in_the_reference_order(golden, case_sums):
    from cat_amd.metric import kid_score as K
    _, _, gi, ri, _ = case_sums['ragged']
    assert gi.dtype == np.int32 and gi.shape == (3, 37)
    assert np.array_equal(gi, golden['ragged_gi']) and np.array_equal(ri, golden['ragged_ri'])
    assert all(len(set(row)) == 37 for row in gi)                       # without replacement
    with pytest.raises(ValueError):                                     # numpy's own: a subset larger than the set
        K.draw_subsets(60, 30, 1, 37)
    with pytest.raises(ValueError):
        K.polynomial_mmd_averages(np.zeros((60, 64)), np.zeros((30, 64)), n_subsets=1, subset_size=37)


def test_split_sums_layout():
    from cat_amd.metric import kid_score as K
    m = 5
    out = np.arange(2 * (6 * m + 4), dtype=np.float64).reshape(2, -1)
    sums = K.split_sums(out, m)
    assert list(sums) == list(K.SUM_KEYS + K.SCALAR_KEYS)
    assert np.array_equal(sums['rs_xx'][1], out[1, :5]) and np.array_equal(sums['cs_xy'][0], out[0, 25:30])
    assert [float(sums[k][0]) for k in K.SCALAR_KEYS] == [30.0, 31.0, 32.0, 33.0]


def test_kernel_arguments():
    from cat_amd.metric import kid_score as K
    assert K._kernel_params(2048) == (3, 1.0 / 2048, 1.0)                # gamma None -> 1 / d, as sklearn
    assert K._kernel_params(64, 2, 0.01, 0.5) == (2, 0.01, 0.5)
    assert K._kernel_params(64, 3.0) == (3, 1.0 / 64, 1.0)
    f = np.zeros((8, 64))
    for bad in (2.5, 0, -1, True):
        with pytest.raises(ValueError, match='degree'):
            K.polynomial_mmd(f, f, degree=bad)
        with pytest.raises(ValueError, match='degree'):
            K.polynomial_mmd_averages(f, f, n_subsets=1, subset_size=4, degree=bad)
    with pytest.raises(ValueError, match='multiple of 4'):
        K.polynomial_mmd(np.zeros((8, 66)), np.zeros((8, 66)))
    with pytest.raises(ValueError, match='multiple of 4'):
        K.polynomial_mmd_averages(np.zeros((8, 30)), np.zeros((8, 30)), n_subsets=1, subset_size=4)
    with pytest.raises(ValueError, match='outside'):
        K.poly_sums(f, f, [[0, 8]], [[0, 1]])


def test_workspace_query_is_a_host_function():
    from cat_amd import _lib
    lib = _lib.load()
    assert lib.cat_kid_poly_sums_ws_bytes(3, 100) == 3 * 4 * 2 * 8       # ceil(100 / 64) panels x 4 scalars x S doubles
    assert lib.cat_kid_poly_sums_ws_bytes(1, 64) == 32 and lib.cat_kid_poly_sums_ws_bytes(1, 65) == 64
    assert lib.cat_kid_poly_sums_ws_bytes(0, 10) == 0


class _ChannelMeans(torch.nn.Module):
    """A stand-in for InceptionV3 on CPU tensors: one [B, 3, 1, 1] block of per-channel means, and a record of the batches it saw."""

    def __init__(self):
        super().__init__()
        self.batches = []

    def forward(self, x):
        assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3
        self.batches.append(x.shape[0])
        return [x.mean(dim=(2, 3), keepdim=True)]


def _write_images(folder, n, ext='png', seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    ims = rng.randint(0, 256, size=(n, 6, 8, 3)).astype(np.uint8)
    paths = []
    for i, im in enumerate(ims):
        paths.append(os.path.join(str(folder), '%s%02d.%s' % (ext[0], i, ext)))
        Image.fromarray(im).save(paths[-1])
    return ims, paths


def test_get_activations_drops_the_remainder(tmp_path, capsys):
    from cat_amd.metric import kid_score as K
    ims, paths = _write_images(tmp_path, 5)
    model = _ChannelMeans()
    act = K.get_activations(paths, model, batch_size=2, dims=3, device='cpu')
    text = capsys.readouterr().out
    assert 'not a multiple of the batch size' in text and 'bigger than the data size' not in text
    assert act.shape == (4, 3) and act.dtype == np.float64 and model.batches == [2, 2] and not model.training
    want = (ims[:4].astype(np.float32) / 255.).mean(axis=(1, 2))         # file path: / 255
    assert np.abs(act - want).max() < 1e-6
    # exact multiple: no warning
    K.get_activations(paths[:4], model, batch_size=2, dims=3, device='cpu')
    assert capsys.readouterr().out == ''


def test_get_activations_clamps_the_batch_size(tmp_path, capsys):
    from cat_amd.metric import kid_score as K
    ims, paths = _write_images(tmp_path, 3)
    model = _ChannelMeans()
    act = K.get_activations(paths, model, batch_size=8, dims=3, device='cpu')
    text = capsys.readouterr().out
    assert 'not a multiple of the batch size' in text and 'Setting batch size to data size' in text
    assert act.shape == (3, 3) and model.batches == [3]


def test_get_activations_scales_arrays_from_minus_one_one():
    from cat_amd.metric import kid_score as K
    rng = np.random.RandomState(3)
    arr = (rng.random_sample((4, 3, 6, 8)) * 2 - 1).astype(np.float32)
    keep = arr.copy()
    act = K.get_activations(arr, _ChannelMeans(), batch_size=2, dims=3, device='cpu')
    assert np.array_equal(arr, keep)                                    # the caller's array is not scaled in place
    assert np.abs(act - ((keep + 1) / 2).mean(axis=(2, 3))).max() < 1e-6


def test_compute_activations_globs_jpg_then_png(tmp_path, monkeypatch):
    from cat_amd.metric import kid_score as K
    _, pngs = _write_images(tmp_path, 2, 'png')
    _, jpgs = _write_images(tmp_path, 3, 'jpg')
    (tmp_path / 'notes.txt').write_text('not an image')
    seen = {}

    def fake(files, model, batch_size, dims, device):
        seen['files'] = list(files)
        return np.zeros((len(files), dims))
    monkeypatch.setattr(K, 'get_activations', fake)
    K._compute_activations(str(tmp_path), None, 2, 3, 'cpu')
    assert len(seen['files']) == 5
    assert sorted(seen['files'][:3]) == sorted(jpgs) and sorted(seen['files'][3:]) == sorted(pngs)
    arr = np.zeros((2, 3, 4, 4), dtype=np.float32)
    K._compute_activations(arr, None, 2, 3, 'cpu')                     # an array goes through as it is
    assert seen['files'][0].shape == (3, 4, 4)


def test_calculate_kid_given_paths_checks_its_inputs(tmp_path):
    from cat_amd.metric import kid_score as K
    with pytest.raises(RuntimeError, match='Invalid path'):
        K.calculate_kid_given_paths([str(tmp_path / 'missing')], 2, 'cpu', 2048)
    with pytest.raises(RuntimeError, match='does not download'):
        K.calculate_kid_given_paths([str(tmp_path), str(tmp_path)], 2, 'cpu', 2048, inception=None)


def test_command_line_arguments():
    from cat_amd.metric import kid_score as K
    a = K.parse_args(['--real', 'R', '--fake', 'F1', 'F2', '--inception-path', 'ckpt.pth'])
    assert (a.real, a.fake, a.batch_size, a.dims, a.gpu, a.inception_path) == ('R', ['F1', 'F2'], 2, 2048, '0', 'ckpt.pth')
    a = K.parse_args(['--real', 'R', '--fake', 'F', '--batch-size', '8', '--dims', '768', '-c', '3', '--inception-path', 'p'])
    assert (a.batch_size, a.dims, a.gpu) == (8, 768, '3')
    for argv in (['--fake', 'F', '--inception-path', 'p'], ['--real', 'R', '--inception-path', 'p'], ['--real', 'R', '--fake', 'F'],
                 ['--real', 'R', '--fake', 'F', '--inception-path', 'p', '--dims', '100']):
        with pytest.raises(SystemExit):
            K.parse_args(argv)


def test_get_kid_is_exported():
    import inspect
    from cat_amd import metric
    sig = inspect.signature(metric.get_kid)
    assert list(sig.parameters) == ['fakes', 'real_codes', 'model', 'device', 'batch_size', 'n_subsets', 'subset_size']
    assert [sig.parameters[k].default for k in ('device', 'batch_size', 'n_subsets', 'subset_size')] == [None, 1, 100, 100]
