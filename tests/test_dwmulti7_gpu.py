"""cat_dwconv2d_multi7_fwd (csrc/dwconv.hip): the frozen BatchNorm-folded teacher's depthwise stage with a kernel size in {1, 3, 5, 7} per
channel quad, filters in a 7 x 7 frame [49][C] -- both kernels behind the entry point (the 1-D walk; the 8 x 16 tile kernel on its
(8 + 6) x (16 + 6) patch from DW_MULTI_TILE_MIN_WG workgroups on) through the C ABI.

Reference: float64 depthwise convolution on the CPU (F.conv2d, groups = C, explicit reflect / zero padding) + bias + ReLU.  Bar: _cmp of
tests/test_dw_quadgroups_gpu.py (rel() < TOL of tests/test_kernels_gpu.py), the bar of cat_dwconv2d_multi_fwd.  N = 2 throughout; x and y have
pixel strides wider than 4 * nq, sentinels in the columns beyond and behind the buffer."""
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
from test_fused_kernels_gpu import ACT_RELU, SENTINEL, _cmp, _nchw, _nhwc_buffer, _pad, _sentinel, _tail, cdiv
from test_kernels_gpu import TOL, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2
G = 4                      # csrc/common.h: CAT_DW_GROUP, channel quads per workgroup of the tile kernel
TILE_MIN_WG = 1024         # csrc/dwconv.hip: DW_MULTI_TILE_MIN_WG
MAXRUN = 8                 # include/cat_hip.h: CAT_DWMULTI_MAXRUN
RUNS = (7, 5, 3, 1)                              # one quad per run
TEACHER = (3,) * 11 + (5,) * 11 + (7,) * 11      # the 3 5 7 teacher's three 42-channel depthwise branches in 44-channel slots
# name -> (ks, H, W, reflect)
CASES = {
    'runs-reflect-9x17': (RUNS, 9, 17, 1), 'runs-zero-9x17': (RUNS, 9, 17, 0),
    'runs-reflect-4x4': (RUNS, 4, 4, 1),          # the smallest plane a mirrored 7 x 7 window admits: k / 2 < H
    'runs-zero-3x5': (RUNS, 3, 5, 0),             # windows wider than the plane
    'teacher-reflect-9x17': (TEACHER, 9, 17, 1),  # one full tile + a one-pixel ragged row and column
    'teacher-reflect-4x4': (TEACHER, 4, 4, 1), 'teacher-zero-3x5': (TEACHER, 3, 5, 0),
    'above-reflect': (TEACHER, 57, 113, 1), 'above-zero': (TEACHER, 57, 113, 0),      # the tile kernel: 2 x 64 tiles x 9 groups = 1152 workgroups
}


def _groups(ks):
    ng, prev, fill = 0, None, 0
    for k in ks:
        if k == prev and fill < G:
            fill += 1
        else:
            ng, prev, fill = ng + 1, k, 1
    return ng


def _wgs(name):
    ks, h, w, _ = CASES[name]
    return N * cdiv(h, 8) * cdiv(w, 16) * _groups(ks)


def frame_row(k, ky, kx):
    return (ky + 3 - k // 2) * 7 + kx + 3 - k // 2


def _w49(ws, ks):
    """one [4][k][k] filter block per quad -> the kernels' [49][C] frame"""
    fr = torch.zeros(49, 4 * len(ks))
    for q, (wt, k) in enumerate(zip(ws, ks)):
        for ky in range(k):
            for kx in range(k):
                fr[frame_row(k, ky, kx), 4 * q:4 * q + 4] = wt[:, ky, kx]
    return fr


def _dwconv_ref(a, ws, ks, reflect, b):
    y = torch.zeros_like(a)
    for k in (1, 3, 5, 7):
        idx = [4 * q + e for q in range(len(ks)) if ks[q] == k for e in range(4)]
        if idx:
            wt = torch.cat([ws[q] for q in range(len(ks)) if ks[q] == k]).to(a.dtype).unsqueeze(1)
            y[:, idx] = F.conv2d(_pad(a[:, idx], k // 2, reflect), wt, b[idx].to(a.dtype), padding=0, groups=len(idx))
    return y


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def test_the_cases_meet_the_constants():
    assert _groups(TEACHER) == 9 and _groups(RUNS) == 4
    assert _wgs('above-zero') == 1152 >= TILE_MIN_WG and all(_wgs(k) < TILE_MIN_WG for k in CASES if not k.startswith('above'))
    src = open(os.path.join(ROOT, 'cat_amd', 'csrc', 'dwconv.hip')).read() + open(os.path.join(ROOT, 'include', 'cat_hip.h')).read()
    assert 'DW_MULTI_TILE_MIN_WG = %d;' % TILE_MIN_WG in src and '#define CAT_DWMULTI_MAXRUN %d ' % MAXRUN in src
    for k in (1, 3, 5, 7):      # the frame's index map: centred, distinct rows
        rows = [frame_row(k, ky, kx) for ky in range(k) for kx in range(k)]
        assert len(set(rows)) == k * k and min(rows) >= 0 and max(rows) < 49 and rows[k * k // 2] == 24


@functools.lru_cache(maxsize=None)
def _inputs(name):
    ks, h, w, reflect = CASES[name]
    c = 4 * len(ks)
    ws = [detfill.normal((4, k, k), 1710 + q, 1.0 / k) for q, k in enumerate(ks)]
    return detfill.normal((N, c, h, w), 1700), ws, detfill.normal((c,), 1701, 0.2)


@functools.lru_cache(maxsize=None)
def _ref(name):
    ks, h, w, reflect = CASES[name]
    x, ws, b = _inputs(name)
    return {'y': F.relu(_dwconv_ref(x.double(), ws, ks, reflect, b))}


def _geom(ks, h, w, xcs, ycs, reflect):
    from cat_amd import _lib as L
    g = L.DwMulti()
    g.N, g.H, g.W, g.nq, g.xcs, g.ycs, g.reflect, g.act, g.slope = N, h, w, len(ks), xcs, ycs, reflect, ACT_RELU, 0.2
    for q, k in enumerate(ks):
        g.ks[q] = k
    return g


def _run(dev, name, x=None):
    """-> y [N, C, H, W] on the host; x / y strides wider than 4 * nq"""
    from cat_amd import _lib as L, ops
    ks, h, w, reflect = CASES[name]
    x0, ws, b = _inputs(name)
    x = x0 if x is None else x
    c = 4 * len(ks)
    xcs, ycs = c + 4, c + 8
    g = _geom(ks, h, w, xcs, ycs, reflect)
    xg, w49, bg = _nhwc_buffer(x, xcs, dev), _w49(ws, ks).contiguous().to(dev), b.to(dev)
    yflat, y = _sentinel((N, h, w, ycs), dev)
    L.call('cat_dwconv2d_multi7_fwd', C.byref(g), ops._p(xg), ops._p(w49), ops._p(bg), ops._p(y), ops._stream())
    torch.cuda.synchronize()
    yc = y.cpu()
    _tail(yflat, (name, 'y'))
    assert bool((yc[..., c:] == SENTINEL).all()), (name, 'beyond 4 * nq')
    return _nchw(yc, 0, c).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_dwconv_multi7_fwd(dev, name):
    _cmp('dwmulti7', name, {'y': _run(dev, name)}, _ref(name))


def _walk_child(out):
    """run by test_dwconv_multi7_fwd_routing in a process of its own, where the switch forces the 1-D walk"""
    assert os.environ.get('CAT_DWMULTI_TILE') == '0'
    from cat_amd import _lib
    _lib.load()
    np.savez(out, above=_run(torch.device('cuda:0'), 'above-zero').numpy())


@pytest.mark.gpu
def test_dwconv_multi7_fwd_routing(dev, tmp_path):
    """the plane above the routing threshold against the forced 1-D walk (the switch is read once per process: a child process): both within
    the bar of the float64 reference and of each other"""
    out = str(tmp_path / 'walk.npz')
    env = dict(os.environ, CAT_DWMULTI_TILE='0', PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'tests')]))
    r = subprocess.run([sys.executable, '-s', '-c', 'import sys, test_dwmulti7_gpu as t; t._walk_child(sys.argv[1])', out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    walk = torch.from_numpy(np.load(out)['above'])
    d = rel(_run(dev, 'above-zero'), walk)
    print('dwmulti7 tile kernel against the 1-D walk: rel %.3g' % d)
    assert d < TOL
    _cmp('dwmulti7', 'walk-above', {'y': walk}, _ref('above-zero'))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['above-zero', 'teacher-zero-3x5'])
def test_dwconv_multi7_fwd_keeps_a_non_finite_pixel_in_its_windows(dev, name):
    """zero padding, x[0, :, 0, 0] = NaN in every channel: every output whose window does not hold that pixel is finite and unchanged
    (out-of-plane taps load zeros, never x * 0) -- on the tile kernel and on the 1-D walk"""
    ks = CASES[name][0]
    x = _inputs(name)[0].clone()
    x[0, :, 0, 0] = float('nan')
    y = _run(dev, name, x)
    holds = torch.zeros_like(y, dtype=torch.bool)
    for q, k in enumerate(ks):
        holds[0, 4 * q:4 * q + 4, :k // 2 + 1, :k // 2 + 1] = True
    assert bool(torch.isfinite(y[~holds]).all()), (~torch.isfinite(y) & ~holds).nonzero()[:8].tolist()
    assert torch.equal(y[~holds], _run(dev, name)[~holds])


@pytest.mark.gpu
def test_dwconv_multi7_fwd_refusals(dev):
    """k = 9, more runs than CAT_DWMULTI_MAXRUN, a mirrored 7 x 7 window on a 3-pixel plane: an error, nothing written; and the 5 x 5 entry
    point still refuses k = 7"""
    from cat_amd import _lib as L, ops
    h, w = 8, 16
    for entry, ks, hh in (('cat_dwconv2d_multi7_fwd', (7, 9), h), ('cat_dwconv2d_multi7_fwd', (1, 3) * 4 + (5,), h),
                          ('cat_dwconv2d_multi7_fwd', (7, 7), 3), ('cat_dwconv2d_multi_fwd', (5, 7), h)):
        c = 4 * len(ks)
        g = _geom(ks, hh, w, c, c, 1)
        xg = torch.zeros((N, hh, w, c), device=dev)
        fr, b = torch.zeros((49, c), device=dev), torch.zeros(c, device=dev)
        yflat, y = _sentinel((N, hh, w, c), dev)
        with pytest.raises(RuntimeError, match='dwconv multi'):
            L.call(entry, C.byref(g), ops._p(xg), ops._p(fr), ops._p(b), ops._p(y), ops._stream())
        torch.cuda.synchronize()
        assert bool((yflat == SENTINEL).all()), (entry, ks)
    assert len((1, 3) * 4 + (5,)) == MAXRUN + 1
