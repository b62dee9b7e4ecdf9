"""The depthwise tile kernels deal a tile's channel quads out over several workgroups (csrc/common.h: kDwGroup, dw_quad_groups): cat_dwm_fwd,
cat_dwm_bwd and the tile path of cat_dwconv2d_multi_fwd at the quad counts, kernel-size runs and planes where that split can go wrong.

Reference: float64 depthwise convolution on the CPU (F.conv2d, groups = C, explicit reflect / zero padding), statistics and filter gradient
in float64 too.  Tolerance: rel() < TOL of tests/test_kernels_gpu.py, as test_fused_kernels_gpu.py and test_streaming_kernels_gpu.py use for
the same entry points.  N = 2 throughout."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_fused_kernels_gpu import (ACT_LRELU, ACT_NONE, ACT_RELU, NAN, SENTINEL, _act, _cmp, _columns, _dwm_geom, _frame, _nchw, _nhwc_buffer, _pad,
                                    _sentinel, _tail, _tile_stats, _w25, cdiv)
from test_kernels_gpu import TOL, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2
G = 4                                    # csrc/common.h: CAT_DW_GROUP, channel quads per workgroup
DWM_MAXQ, DWM_MAXQ_BWD, DWMULTI_MAXQ = 24, 18, 64      # include/cat_hip.h
TILE_MIN_WG = 1024                       # csrc/dwconv.hip: DW_MULTI_TILE_MIN_WG, tiles x quad groups from which the teacher entry point takes the tile kernel
UNEVEN = (1, 1, 1, 3, 3, 5, 5, 5, 5, 1, 3)      # run boundaries off the group boundaries
COUNTS_FWD = (1, G - 1, G, G + 1, 2 * G + 1, DWM_MAXQ)
COUNTS_BWD = (1, G - 1, G, G + 1, 2 * G + 1, DWM_MAXQ_BWD)

# forward: name -> (ks, H, W, reflect, (x, y, table) strides beyond 4 * nq, per-image affine, statistics, act, bias)
FWD = {'count%d' % nq: ((3,) * nq, 9, 17, 1, (0, 0, 0), 0, 1, ACT_RELU, 1) for nq in COUNTS_FWD}
FWD.update({
    'uneven': (UNEVEN, 9, 17, 1, (0, 0, 0), 0, 1, ACT_RELU, 1), 'all5': ((5,) * 6, 9, 17, 0, (0, 0, 0), 0, 1, ACT_LRELU, 0),
    'all1': ((1,) * 6, 9, 17, 1, (0, 0, 0), 0, 1, ACT_NONE, 1),
    'ragged-reflect': (UNEVEN, 9, 17, 1, (0, 0, 0), 0, 1, ACT_RELU, 0), 'ragged-zero': (UNEVEN, 9, 17, 0, (0, 0, 0), 0, 1, ACT_RELU, 1),
    'minimal-reflect': (UNEVEN, 3, 3, 1, (0, 0, 0), 0, 1, ACT_RELU, 1), 'minimal-zero': (UNEVEN, 3, 3, 0, (0, 0, 0), 0, 1, ACT_RELU, 0),
    'strides': (UNEVEN, 16, 32, 1, (8, 4, 12), 0, 1, ACT_RELU, 1), 'per-image': (UNEVEN, 16, 32, 0, (4, 0, 4), 1, 1, ACT_LRELU, 1),
    'no-stats': (UNEVEN, 16, 32, 1, (0, 4, 0), 0, 0, ACT_RELU, 1),
})
# backward: name -> (ks, H, W, reflect); both `accumulate` values in every case
BWD = {'count%d' % nq: ((3,) * nq, 9, 17, 1) for nq in COUNTS_BWD}
BWD.update({'uneven': (UNEVEN, 9, 17, 1), 'all5': ((5,) * 6, 9, 17, 0), 'all1': ((1,) * 6, 9, 17, 1),
            'ragged-zero': (UNEVEN, 9, 17, 0), 'minimal-reflect': (UNEVEN, 3, 3, 1), 'minimal-zero': (UNEVEN, 3, 3, 0), 'two-tiles': (UNEVEN, 16, 32, 0)})
# teacher entry point: name -> (ks, H, W, reflect).  Groups: 44 quads = runs of 22 / 11 / 11 -> 6 + 3 + 3 = 12, 64 quads = 4 x 16 -> 16
KS44, KS64 = (1,) * 22 + (3,) * 11 + (5,) * 11, (1,) * 16 + (3,) * 16 + (5,) * 16 + (1,) * 16
MULTI = {'nq44-reflect': (KS44, 57, 96, 1), 'nq44-zero': (KS44, 57, 96, 0), 'nq64-reflect': (KS64, 33, 112, 1), 'nq64-zero': (KS64, 33, 112, 0),
         'below': (KS44, 56, 96, 0)}


def _groups(ks):
    """dw_quad_groups: the runs of equal kernel size cut into pieces of at most G quads"""
    ng, prev, fill = 0, None, 0
    for k in ks:
        if k == prev and fill < G:
            fill += 1
        else:
            ng, prev, fill = ng + 1, k, 1
    return ng


def _wgs(name):
    ks, h, w, _ = MULTI[name]
    return N * cdiv(h, 8) * cdiv(w, 16) * _groups(ks)


def _runs(ks):
    """[(first quad, quads, kernel size)] of the runs of equal kernel size"""
    runs = []
    for q, k in enumerate(ks):
        if runs and runs[-1][2] == k:
            runs[-1][1] += 1
        else:
            runs.append([q, 1, k])
    return runs


def _dwconv_ref(a, ws, ks, reflect, b=None):
    """a [N, C, H, W] float64, ws: one [4][k][k] filter block per quad -> the depthwise conv, quad by kernel size"""
    y = torch.zeros_like(a)
    for k in (1, 3, 5):
        idx = [4 * q + e for q in range(len(ks)) if ks[q] == k for e in range(4)]
        if idx:
            wt = torch.cat([ws[q] for q in range(len(ks)) if ks[q] == k]).to(a.dtype).unsqueeze(1)
            y[:, idx] = F.conv2d(_pad(a[:, idx], k // 2, reflect), wt, None if b is None else b[idx].to(a.dtype), padding=0, groups=len(idx))
    return y


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def test_the_cases_meet_the_constants():
    assert _groups((3,) * (G + 1)) == 2 and _groups(UNEVEN) == 5 and _groups(KS44) == 12 and _groups(KS64) == 16
    assert _wgs('below') < TILE_MIN_WG <= _wgs('nq44-zero') and _wgs('below') == 1008 and _wgs('nq44-zero') == 1152
    assert all(_wgs(k) >= TILE_MIN_WG for k in MULTI if k != 'below')
    src = open(os.path.join(ROOT, 'cat_amd', 'csrc', 'dwconv.hip')).read() + open(os.path.join(ROOT, 'cat_amd', 'csrc', 'common.h')).read()
    assert 'DW_MULTI_TILE_MIN_WG = %d;' % TILE_MIN_WG in src and '#define CAT_DW_GROUP %d\n' % G in src


# ------------------------------------------------------------------------------------------------ cat_dwm_fwd
@functools.lru_cache(maxsize=None)
def _fwd_inputs(name):
    ks, h, w, reflect, extra, per_image, stats, act, bias = FWD[name]
    c = 4 * len(ks)
    x = detfill.normal((N, c, h, w), 1400)
    rows = N if per_image else 1
    scale, shift = detfill.normal((rows, c), 1401).abs() + 0.5, detfill.normal((rows, c), 1402, 0.3)
    ws = [detfill.normal((4, k, k), 1410 + q, 1.0 / k) for q, k in enumerate(ks)]
    return x, scale, shift, ws, (detfill.normal((c,), 1403, 0.2) if bias else None)


@functools.lru_cache(maxsize=None)
def _fwd_ref(name):
    ks, h, w, reflect, extra, per_image, stats, act, bias = FWD[name]
    x, scale, shift, ws, b = _fwd_inputs(name)
    c = x.shape[1]
    a = _act(x.double() * scale.double().view(-1, c, 1, 1) + shift.double().view(-1, c, 1, 1), act)
    out = {'y': _dwconv_ref(a, ws, ks, reflect, b)}
    if stats:
        out['sum'], out['m2'], _ = _tile_stats(out['y'])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(FWD))
def test_dwm_fwd_quad_groups(dev, name):
    from cat_amd import _lib as L, ops
    ks, h, w, reflect, (xe, ye, se), per_image, stats, act, bias = FWD[name]
    x, scale, shift, ws, b = _fwd_inputs(name)
    c = 4 * len(ks)
    xcs, ycs, scs, sstride = c + xe, c + ye, c + se, (c + 4 if per_image else 0)
    xg = _nhwc_buffer(x, xcs, dev)
    rows = lambda v: F.pad(v, (0, 4), value=SENTINEL).to(dev) if per_image else v.reshape(-1).to(dev)
    scg, shg = rows(scale), rows(shift)
    g = _dwm_geom(N, h, w, len(ks), xcs, ycs, scs, sstride, reflect, act, ks)
    yflat, y = _sentinel((N, h, w, ycs), dev)
    tflat, tab = _sentinel((N * cdiv(h, 8) * cdiv(w, 16), 2, scs), dev)
    w25, bg = _w25(_frame(ws, ks), dev), (b.to(dev) if bias else None)
    L.call('cat_dwm_fwd', C.byref(g), ops._p(xg), ops._p(scg), ops._p(shg), ops._p(w25), ops._p(bg), ops._p(y), ops._p(tab) if stats else None,
           ops._stream())
    torch.cuda.synchronize()
    yc, tc = y.cpu(), tab.cpu()
    _columns(yc, range(c), range(c), (name, 'y'))
    _tail(yflat, (name, 'y'))
    _tail(tflat, (name, 'table'))
    got = {'y': _nchw(yc, 0, c)}
    if stats:
        _columns(tc, range(c), range(c), (name, 'table'))
        got['sum'], got['m2'] = tc[:, 0, :c], tc[:, 1, :c]
    else:
        assert bool((tc == SENTINEL).all())
    _cmp('dwq-fwd', name, got, _fwd_ref(name))


# ------------------------------------------------------------------------------------------------ cat_dwm_bwd
@functools.lru_cache(maxsize=None)
def _bwd_inputs(name):
    ks, h, w, reflect = BWD[name]
    c = 4 * len(ks)
    a, dz = F.relu(detfill.normal((N, c, h, w), 1500) + 0.3), detfill.normal((N, c, h, w), 1501)
    ws = [detfill.normal((4, k, k), 1510 + q, 1.0 / k) for q, k in enumerate(ks)]
    prev = [detfill.normal((4 * nq, k, k), 1560 + i, float(np.sqrt(N * h * w))) for i, (q0, nq, k) in enumerate(_runs(ks))]
    return a, dz, ws, prev


@functools.lru_cache(maxsize=None)
def _bwd_ref(name):
    ks, h, w, reflect = BWD[name]
    a32, dz, ws, prev = _bwd_inputs(name)
    a = a32.double().requires_grad_(True)
    wl = [wt.double().requires_grad_(True) for wt in ws]
    z = _dwconv_ref(a, wl, ks, reflect)
    grads = torch.autograd.grad([z], [a] + wl, [dz.double()])
    out = {'da': grads[0]}
    for i, (q0, nq, k) in enumerate(_runs(ks)):      # one branch per run, the parameters' [c][k][k] layout
        out['dw%d' % i] = torch.cat(grads[1 + q0:1 + q0 + nq])
        out['dwacc%d' % i] = prev[i].double() + out['dw%d' % i]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(BWD))
def test_dwm_bwd_quad_groups(dev, name):
    from cat_amd import _lib as L, ops
    ks, h, w, reflect = BWD[name]
    a, dz, ws, prev = _bwd_inputs(name)
    c = 4 * len(ks)
    acs, zcs, dacs = c + 4, c + 8, c + 12
    br = [(4 * nq, k) for q0, nq, k in _runs(ks)]
    c0s = [4 * q0 for q0, nq, k in _runs(ks)]
    w25 = _w25(_frame(ws, ks), dev)
    ag, zg = _nhwc_buffer(a, acs, dev), _nhwc_buffer(dz, zcs, dev)
    g = _dwm_geom(N, h, w, len(ks), acs, zcs, 0, 0, reflect, 0, ks)
    nb = len(br)
    IA = C.c_int * nb
    nbytes = int(L.query('cat_dwm_bwd_ws_bytes', C.byref(g)))
    assert nbytes >= N * cdiv(h, 8) * cdiv(w, 16) * 25 * c * 4
    got = {}
    for accumulate in (0, 1):
        dflat, da = _sentinel((N, h, w, dacs), dev)
        wsflat, wsbuf = _sentinel((nbytes // 4,), dev, NAN)
        dsts = [_sentinel((cb * k * k,), dev, NAN) for cb, k in br]
        if accumulate:
            for (flat, d), p in zip(dsts, prev):
                d.copy_(p.reshape(-1))
        L.call('cat_dwm_bwd', C.byref(g), ops._p(ag), ops._p(zg), ops._p(w25), ops._p(da), dacs, nb, IA(*c0s), IA(*[cb for cb, k in br]),
               IA(*[k for cb, k in br]), (C.c_void_p * nb)(*[d.data_ptr() for flat, d in dsts]), accumulate, ops._p(wsbuf), ops._stream())
        torch.cuda.synchronize()
        dc = da.cpu()
        _columns(dc, range(c), range(c), (name, 'da'))
        _tail(dflat, (name, 'da'))
        _tail(wsflat, (name, 'workspace'))
        assert bool(torch.isfinite(wsbuf[:N * cdiv(h, 8) * cdiv(w, 16) * 25 * c]).all()), 'every partial of the table is written'
        if not accumulate:
            got['da'] = _nchw(dc, 0, c)
        else:
            assert torch.equal(_nchw(dc, 0, c), got['da']), 'accumulate only concerns the filter gradient'
        for i, ((cb, k), (flat, d)) in enumerate(zip(br, dsts)):
            _tail(flat, (name, 'dw', i))
            got[('dwacc%d' if accumulate else 'dw%d') % i] = d.cpu().view(cb, k, k)
    _cmp('dwq-bwd', name, got, _bwd_ref(name))


# ------------------------------------------------------------------------------------------------ cat_dwconv2d_multi_fwd
@functools.lru_cache(maxsize=None)
def _multi_inputs(name):
    ks, h, w, reflect = MULTI[name]
    c = 4 * len(ks)
    ws = [detfill.normal((4, k, k), 1610 + q, 1.0 / k) for q, k in enumerate(ks)]
    return detfill.normal((N, c, h, w), 1600), ws, detfill.normal((c,), 1601, 0.2)


@functools.lru_cache(maxsize=None)
def _multi_ref(name):
    ks, h, w, reflect = MULTI[name]
    x, ws, b = _multi_inputs(name)
    return {'y': F.relu(_dwconv_ref(x.double(), ws, ks, reflect, b))}


def _multi_run(dev, name, x=None):
    """-> y [N, C, H, W] on the host; x / y strides wider than 4 * nq"""
    from cat_amd import _lib as L, ops
    ks, h, w, reflect = MULTI[name]
    x0, ws, b = _multi_inputs(name)
    x = x0 if x is None else x
    c = 4 * len(ks)
    xcs, ycs = c + 4, c + 8
    g = L.DwMulti()
    g.N, g.H, g.W, g.nq, g.xcs, g.ycs, g.reflect, g.act, g.slope = N, h, w, len(ks), xcs, ycs, reflect, ACT_RELU, 0.2
    for q, k in enumerate(ks):
        g.ks[q] = k
    xg, w25, bg = _nhwc_buffer(x, xcs, dev), _w25(_frame(ws, ks), dev), b.to(dev)
    yflat, y = _sentinel((N, h, w, ycs), dev)
    L.call('cat_dwconv2d_multi_fwd', C.byref(g), ops._p(xg), ops._p(w25), ops._p(bg), ops._p(y), ops._stream())
    torch.cuda.synchronize()
    yc = y.cpu()
    _tail(yflat, (name, 'y'))
    assert bool((yc[..., c:] == SENTINEL).all()), (name, 'beyond 4 * nq')
    return _nchw(yc, 0, c).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(MULTI))
def test_dwconv_multi_fwd_tile_path(dev, name):
    _cmp('dwq-multi', name, {'y': _multi_run(dev, name)}, _multi_ref(name))


def _old_path_child(out):
    """run by test_dwconv_multi_fwd_routing in a process of its own, where the switch forces the 1-D kernel"""
    assert os.environ.get('CAT_DWMULTI_TILE') == '0'
    from cat_amd import _lib
    _lib.load()
    d = torch.device('cuda:0')
    np.savez(out, below=_multi_run(d, 'below').numpy(), above=_multi_run(d, 'nq44-zero').numpy())


@pytest.mark.gpu
def test_dwconv_multi_fwd_routing(dev, tmp_path):
    """one plane just below and one just above the routing threshold, against the forced 1-D kernel (the switch is read once per process: a
    child process): bit-identical below, within the tolerance above"""
    out = str(tmp_path / 'old.npz')
    env = dict(os.environ, CAT_DWMULTI_TILE='0', PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'tests')]))
    r = subprocess.run([sys.executable, '-s', '-c', 'import sys, test_dw_quadgroups_gpu as t; t._old_path_child(sys.argv[1])', out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    old = np.load(out)
    below, above = _multi_run(dev, 'below'), _multi_run(dev, 'nq44-zero')
    assert torch.equal(below, torch.from_numpy(old['below'])), 'below the threshold both runs take the 1-D kernel'
    d = rel(above, torch.from_numpy(old['above']))
    print('tile kernel against the 1-D kernel: rel %.3g' % d)
    assert d < TOL
    _cmp('dwq-multi', 'old-path-above', {'y': torch.from_numpy(old['above'])}, _multi_ref('nq44-zero'))


@pytest.mark.gpu
def test_dwconv_multi_fwd_tile_path_keeps_a_non_finite_pixel_in_its_windows(dev):
    """zero padding, x[0, :, 0, 0] = inf in every channel: every output whose window does not hold that pixel is finite (out-of-plane taps are
    literal zeros in LDS, never x * 0)"""
    name = 'nq44-zero'
    ks = MULTI[name][0]
    x = _multi_inputs(name)[0].clone()
    x[0, :, 0, 0] = float('inf')
    y = _multi_run(dev, name, x)
    holds = torch.zeros_like(y, dtype=torch.bool)
    for q, k in enumerate(ks):
        holds[0, 4 * q:4 * q + 4, :k // 2 + 1, :k // 2 + 1] = True
    assert bool(torch.isfinite(y[~holds]).all()), (~torch.isfinite(y) & ~holds).nonzero()[:8].tolist()
    clean = _multi_run(dev, name)
    assert torch.equal(y[~holds], clean[~holds])
