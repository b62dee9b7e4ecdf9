"""GPU: the kernel inception distance on the HIP kernels (csrc/kid_ops.hip, cat_amd/metric/kid_score.py).

A: cat_kid_poly_sums against the float64 numpy restatement (tests/kid_numpy.py) over the tile edges of the kernel: exactly one 16 x 16 MFMA
   tile, one row over and under, a ragged panel, the evaluation scripts' own 100 x 2048, more than one 64-row panel, two rows, a feature
   width that is no multiple of the staging step.  Tables with rows shared between subsets and repeated inside one, nx != ny, Y aliasing X,
   outputs and workspace poisoned with NaN.  Every sum at 1e-11 relative: the bound for non-negative features is d * 2^-53 = 2.3e-13 on
   each dot product (both sides), about three times that after the cube, kept by sums of positive terms; 1e-11 leaves a tenfold margin.
B: two launches give the same bits; an index outside its matrix gives NaN, not a read; the entry point refuses what it does not compute.
C: polynomial_mmd_averages after np.random.seed(s) against tests/golden/kid.npz -- the reference's own run: |d mmd2| <= 1e-11 * scale,
   |d var| <= 1e-10 * scale^2 with scale = mean K_XX + mean K_YY + 2 mean K_XY (the sums' tolerance through the estimator's formula).
D: get_activations / get_kid / the command line on the seeded InceptionV3 of tests/golden/inception_fid.npz."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers as H
import kid_numpy as KN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_TOL = 1e-11

# (m, d, S, Y aliases X)
SUM_CASES = [(16, 64, 1, False), (17, 64, 2, False), (15, 192, 2, False), (37, 768, 2, True), (100, 2048, 3, False), (130, 64, 1, False),
             (2, 64, 1, False), (20, 36, 2, False)]


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _tables(rng, n, m, S):
    """[S, m] row numbers: a fresh permutation per subset, the first half of every later subset taken (shuffled) from subset 0"""
    t = np.stack([rng.permutation(n)[:m] for _ in range(S)]).astype(np.int32)
    for s in range(1, S):
        t[s, :m // 2] = rng.permutation(t[0])[:m // 2]
    return t


def _sum_case(m, d, S, alias):
    rng = np.random.RandomState(1000 + m + d)
    nx, ny = m + 7, (m + 7 if alias else m + 3)
    x, y = KN.features(2000 + m + d, nx, ny, d)
    if alias:
        y = x
    gi, ri = _tables(rng, nx, m, S), _tables(rng, ny, m, S)
    if alias:
        gi[0, 1] = gi[0, 0]                 # a row twice in one subset
        ri[0, :3] = gi[0, :3]               # and the same rows on both sides
    return x, y, gi, ri


_REF = {}


def _reference(case):
    """the numpy sums of a case, computed once"""
    if case not in _REF:
        x, y, gi, ri = _sum_case(*case)
        _REF[case] = (x, y, gi, ri, KN.poly_sums(x, y, gi, ri))
    return _REF[case]


def _launch(x, y, gi, ri, dev, alias, **kernel):
    from cat_amd import _lib as L
    from cat_amd.metric import kid_score as K
    xd = torch.from_numpy(x.astype(np.float32)).to(dev)
    yd = xd if alias else torch.from_numpy(y.astype(np.float32)).to(dev)
    S, m = gi.shape
    out = torch.full((S, 6 * m + 4), float('nan'), dtype=torch.float64, device=dev)
    ws = torch.full((L.query('cat_kid_poly_sums_ws_bytes', S, m) // 8,), float('nan'), dtype=torch.float64, device=dev)
    K.poly_sums_device(xd, yd, torch.from_numpy(gi).to(dev), torch.from_numpy(ri).to(dev), kernel.get('degree', 3), kernel.get('gamma'),
                       kernel.get('coef0', 1), out=out, ws=ws)
    torch.cuda.synchronize()
    return out, ws


@pytest.mark.parametrize('case', SUM_CASES, ids=lambda c: 'm%d_d%d_S%d%s' % (c[0], c[1], c[2], '_alias' if c[3] else ''))
def test_kernel_sums_against_numpy(dev, case):
    from cat_amd.metric import kid_score as K
    x, y, gi, ri, want = _reference(case)
    out, ws = _launch(x, y, gi, ri, dev, case[3])
    assert not bool(torch.isnan(out).any()) and not bool(torch.isnan(ws).any())      # every element of both buffers was written
    got = K.split_sums(out.cpu().numpy(), case[0])
    worst = 0.0
    for k in K.SUM_KEYS + K.SCALAR_KEYS:
        assert got[k].shape == want[k].shape, k
        err = float((np.abs(got[k] - want[k]) / np.abs(want[k])).max())
        worst = max(worst, err)
        assert err <= SUM_TOL, (k, err)
    print('kid sums m=%d d=%d S=%d: worst rel err %.2e' % (case[0], case[1], case[2], worst))


def test_kernel_sums_with_other_kernel_arguments(dev):
    from cat_amd.metric import kid_score as K
    case = (37, 768, 2, True)
    x, y, gi, ri, _ = _reference(case)
    for kernel in (dict(degree=2, gamma=0.01, coef0=0.5), dict(degree=1, gamma=0.5, coef0=0.0), dict(degree=5, gamma=None, coef0=2)):
        want = KN.poly_sums(x, y, gi, ri, **kernel)
        out, _ = _launch(x, y, gi, ri, dev, True, **kernel)
        got = K.split_sums(out.cpu().numpy(), 37)
        for k in K.SUM_KEYS + K.SCALAR_KEYS:
            assert float((np.abs(got[k] - want[k]) / np.abs(want[k])).max()) <= SUM_TOL, (kernel, k)


def test_two_launches_give_the_same_bits(dev):
    for case in ((100, 2048, 3, False), (130, 64, 1, False)):
        x, y, gi, ri, _ = _reference(case)
        a, wa = _launch(x, y, gi, ri, dev, False)
        b, wb = _launch(x, y, gi, ri, dev, False)
        assert torch.equal(a, b) and torch.equal(wa, wb)


def test_an_index_outside_the_matrix_poisons_its_row_only(dev):
    """Row numbers -1 and nx are not read (X is a view inside a larger buffer, so even a read would stay inside the allocation): the row's
    sums, and what crosses it, are NaN; the other product's sums are untouched."""
    from cat_amd.metric import kid_score as K
    m, d = 20, 64
    x, y = KN.features(77, m + 5, m + 3, d)
    buf = torch.zeros((m + 7, d), dtype=torch.float32, device=dev)
    buf[1:m + 6] = torch.from_numpy(x.astype(np.float32)).to(dev)
    xd = buf[1:m + 6]
    yd = torch.from_numpy(y.astype(np.float32)).to(dev)
    gi = np.arange(m, dtype=np.int32)[None].copy()
    ri = np.arange(m, dtype=np.int32)[None].copy()
    want = KN.poly_sums(x, y, gi, ri)
    gi[0, 3], gi[0, 11] = -1, m + 5
    out = K.poly_sums_device(xd, yd, torch.from_numpy(gi).to(dev), torch.from_numpy(ri).to(dev), 3, None, 1)
    got = K.split_sums(out.cpu().numpy(), m)
    bad = np.zeros(m, dtype=bool)
    bad[[3, 11]] = True
    assert np.isnan(got['rs_xx'][0]).all() and np.isnan(got['cs_xy'][0]).all()          # every row / column of K_XX, K_XY meets a bad row
    assert np.isnan(got['rs_xy'][0][bad]).all() and not np.isnan(got['rs_xy'][0][~bad]).any()
    assert np.isnan(got['dg_xx'][0][bad]).all() and not np.isnan(got['dg_xx'][0][~bad]).any()
    for k in ('rs_yy', 'dg_yy', 'sq_yy'):
        assert float((np.abs(got[k] - want[k]) / want[k]).max()) <= SUM_TOL
    with pytest.raises(ValueError, match='outside'):                                    # the host entry refuses such a table outright
        K.poly_sums(x, y, gi, ri, device=dev)


def test_entry_point_refuses_what_it_does_not_compute(dev):
    from cat_amd import _lib as L, ops
    from cat_amd.metric import kid_score as K
    x = torch.zeros((8, 6), dtype=torch.float32, device=dev)
    idx = torch.zeros((1, 4), dtype=torch.int32, device=dev)
    out = torch.zeros(28, dtype=torch.float64, device=dev)

    def call(d, degree):
        L.call('cat_kid_poly_sums', ops._p(x), 8, ops._p(x), 8, d, ops._p(idx), ops._p(idx), 1, 4, 1.0, 1.0, degree, ops._p(out), ops._p(out),
               ops._stream())
    with pytest.raises(RuntimeError, match='multiple of 4'):
        call(6, 3)
    with pytest.raises(RuntimeError, match='degree'):
        call(4, 0)
    with pytest.raises(ValueError, match='multiple of 4'):
        K.poly_sums_device(x, x, idx, idx, 3, None, 1)
    with pytest.raises(ValueError, match='int32'):
        K.poly_sums_device(x[:, :4].contiguous(), x[:, :4].contiguous(), idx.long(), idx.long(), 3, None, 1)


@pytest.mark.parametrize('case', KN.CASES, ids=lambda c: c['name'])
def test_polynomial_mmd_averages_matches_the_reference_run(dev, case):
    from cat_amd.metric import kid_score as K
    g = H.load('kid.npz')
    x, y = KN.features(case['seed'], case['nx'], case['ny'], case['d'])
    np.random.seed(case['draw_seed'])
    gi, ri = K.draw_subsets(len(x), len(y), case['S'], case['m'])
    scale = KN.scale_of(KN.poly_sums(x, y, gi, ri, **case['kernel']), case['m'])
    np.random.seed(case['draw_seed'])
    mmds, vars_ = K.polynomial_mmd_averages(x, y, n_subsets=case['S'], subset_size=case['m'], device=dev, **case['kernel'])
    np.random.seed(case['draw_seed'])
    only = K.polynomial_mmd_averages(x, y, n_subsets=case['S'], subset_size=case['m'], ret_var=False, device=dev, **case['kernel'])
    dm = np.abs(mmds - g[case['name'] + '_mmds']) / scale
    dv = np.abs(vars_ - g[case['name'] + '_vars']) / scale ** 2
    print('KID %s: |d mmd2| / scale %.2e, |d var| / scale^2 %.2e (scale %.3f)' % (case['name'], dm.max(), dv.max(), scale.mean()))
    assert (dm <= 1e-11).all() and (dv <= 1e-10).all()
    assert np.array_equal(only, mmds)
    # polynomial_mmd on one drawn subset is the same estimate, with the variance at the subset's own size unless told otherwise
    one, var_m = K.polynomial_mmd(x[gi[0]], y[ri[0]], var_at_m=min(len(x), len(y)), device=dev, **case['kernel'])
    assert abs(one - mmds[0]) <= 1e-11 * scale[0] and abs(var_m - vars_[0]) <= 1e-10 * scale[0] ** 2


# ---------------------------------------------------------------------------------------------------------------- features, get_kid, CLI
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


def _write_pngs(folder, ims):
    from PIL import Image
    os.makedirs(str(folder), exist_ok=True)
    paths = []
    for i, im in enumerate(ims):
        paths.append(os.path.join(str(folder), 'im%03d.png' % i))
        Image.fromarray(im).save(paths[-1])
    return paths


def test_get_activations_on_a_folder_of_pngs(dev, seeded, tmp_path, capsys):
    from cat_amd.metric import get_activations_from_ims, kid_score as K
    _, net = seeded
    ims = np.random.RandomState(5).randint(0, 256, size=(5, 40, 56, 3)).astype(np.uint8)
    paths = _write_pngs(tmp_path, ims)
    act = K.get_activations(paths, net, batch_size=2, dims=2048, device=dev)
    assert 'not a multiple of the batch size' in capsys.readouterr().out
    assert act.shape == (4, 2048) and act.dtype == np.float64
    want = get_activations_from_ims(ims[:4].astype(np.float64), net, batch_size=2, dims=2048, device=dev, use_tqdm=False)
    err = H.rel_err(act, want)
    print('get_activations vs get_activations_from_ims: rel err %.2e' % err)
    assert err <= 1e-6
    # a block below pool3 is averaged over its plane
    from cat_amd.metric import InceptionV3
    low = InceptionV3([0])
    low.load_fid_state_dict(seeded[0])
    a64 = K.get_activations(paths[:2], low.to(dev).eval(), batch_size=2, dims=64, device=dev)
    assert a64.shape == (2, 64) and np.isfinite(a64).all() and a64.min() >= 0


def test_get_kid_equals_the_folder_route(dev, seeded, tmp_path):
    """Four fakes as tensors against the same four images saved as PNG and globbed back (in whatever order the file system lists them): with
    subsets of the whole set the estimate does not depend on the order, so both routes agree to the sums' tolerance."""
    from cat_amd.metric import get_kid, kid_score as K, tensor2im_batch
    from oracle import detfill
    _, net = seeded
    fakes = [detfill.images((2, 3, 32, 40), 700 + i) for i in range(2)]
    real = np.random.RandomState(6).randint(0, 256, size=(4, 32, 40, 3)).astype(np.uint8)
    real_codes = K.get_activations(_write_pngs(tmp_path / 'real', real), net, batch_size=2, dims=2048, device=dev)
    np.random.seed(21)
    mean, std = get_kid(fakes, real_codes, net, device=dev, batch_size=2, n_subsets=3, subset_size=4)
    _write_pngs(tmp_path / 'fake', tensor2im_batch(torch.cat(fakes, 0)))
    codes = K._compute_activations(str(tmp_path / 'fake'), net, 2, 2048, dev)
    np.random.seed(21)
    mmds = K.polynomial_mmd_averages(real_codes, codes, n_subsets=3, subset_size=4, ret_var=False, device=dev)
    idx = np.arange(4, dtype=np.int32)[None]
    scale = float(KN.scale_of(KN.poly_sums(real_codes, codes, idx, idx), 4)[0])
    print('get_kid %.6f (%.2e), folder route %.6f, scale %.3f' % (mean, std, mmds.mean(), scale))
    assert np.isfinite(mean) and abs(mean - mmds.mean()) <= 1e-11 * scale and abs(std - mmds.std()) <= 1e-11 * scale
    assert std <= 1e-11 * scale                                          # every subset is the whole set


def test_command_line_in_a_fresh_process(dev, seeded, tmp_path):
    sd, _ = seeded
    ckpt = str(tmp_path / 'pt_inception_seeded.pth')
    torch.save(sd, ckpt)
    rng = np.random.RandomState(8)
    real = rng.randint(0, 256, size=(100, 16, 16, 3)).astype(np.uint8)
    fake = (rng.randint(0, 256, size=(100, 16, 16, 3)) // 2).astype(np.uint8)
    _write_pngs(tmp_path / 'real', real)
    _write_pngs(tmp_path / 'fake', fake)
    cmd = [sys.executable, '-m', 'cat_amd.metric.kid_score', '--real', str(tmp_path / 'real'), '--fake', str(tmp_path / 'fake'),
           str(tmp_path / 'real'), '--batch-size', '50', '--gpu', '0', '--inception-path', ckpt]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('KID (')]
    print('\n'.join(lines))
    assert len(lines) == 2
    for ln, folder in zip(lines, ('fake', 'real')):
        mt = re.fullmatch(r'KID \((.+)\): (-?\d+\.\d{3}) \((\d+\.\d{3})\)', ln)
        assert mt and mt.group(1) == str(tmp_path / folder), ln
    assert 'Warning' not in r.stdout                                     # 100 images at batch 50: nothing dropped
