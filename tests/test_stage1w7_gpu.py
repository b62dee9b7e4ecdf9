"""cat_tstage1w7_fwd (csrc/conv_s1w7.hip) -- stage 1 of a frozen, BatchNorm-folded InvertedResidualChannels block with kernel sizes 3 5 7 in one
launch: the 7 x 7, 5 x 5 and 3 x 3 first convs and the concatenated 1 x 1 group from one staging of the input, bias + activation into four
buffers -- through the C ABI against float64 ATen on the host (F.conv2d with explicit reflect / zero padding, bias, activation).

Bar: _cmp of tests/test_fused_kernels_gpu.py (rel() < TOL of tests/test_kernels_gpu.py), the bar of the LDS-tile convolutions.  Every output
buffer has a pixel stride wider than its slot's tiles (48 / 144 columns): valid columns finite, the tiles' padding columns exactly 0, the
columns beyond and the 64 floats behind the buffer still the sentinel."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_fused_kernels_gpu import ACT_LRELU, ACT_RELU, SENTINEL, _act, _cmp, _columns, _nchw, _nhwc_buffer, _pad, _sentinel, _tail, cs4

N = 2
KS = (7, 5, 3, 1)
T, EDGE_A, EDGE_B = (42, 42, 42, 132), (33, 48, 42, 129), (48, 33, 48, 144)      # the teacher's widths; the edges of 33..48 and 129..144
# name -> (cin, extra pixel stride of x, widths (7, 5, 3, 1), H, W, reflect, act, bias)
CASES = {
    'teacher-9x17-reflect': (36, 4, T, 9, 17, 1, ACT_RELU, 1),      # ragged tiles in both directions; a one-quad last chunk
    'teacher-9x17-zero-lrelu': (36, 0, T, 9, 17, 0, ACT_LRELU, 1),
    'teacher-8x16-cin16': (16, 0, T, 8, 16, 0, ACT_RELU, 1),        # one tile, one chunk
    'teacher-8x16-cin20-nobias': (20, 4, T, 8, 16, 1, ACT_RELU, 0),      # a 4-channel tail chunk
    'edge-a-7x7-reflect': (20, 0, EDGE_A, 7, 7, 1, ACT_LRELU, 1),   # the smallest plane the 7 x 7 mirror admits
    'edge-b-3x5-zero': (16, 4, EDGE_B, 3, 5, 0, ACT_RELU, 1),       # windows wider than the plane
    'edge-a-3x5-zero-nobias': (36, 0, EDGE_A, 3, 5, 0, ACT_RELU, 0),
    'teacher-9x17-cin256': (256, 0, T, 9, 17, 1, ACT_RELU, 1),      # the teacher's depth: 16 chunks through both tile buffers
}
SLOPE = 0.2


def supported(w7, w5, w3, w1):
    """mirror of cat_tstage1w7_supported: 3 + 3 + 3 + 9 N tiles"""
    return all(32 < v <= 48 for v in (w7, w5, w3)) and 128 < w1 <= 144


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _inputs(name):
    cin, xpad, widths, h, w, reflect, act, bias = CASES[name]
    x = detfill.normal((N, cin, h, w), 1800)
    ws = [detfill.normal((m, cin, k, k), 1810 + i, 1.0 / (cin * k * k) ** 0.5) for i, (m, k) in enumerate(zip(widths, KS))]
    bs = [detfill.normal((m,), 1820 + i, 0.3) if bias else None for i, m in enumerate(widths)]
    return x, ws, bs


@functools.lru_cache(maxsize=None)
def _ref(name):
    cin, xpad, widths, h, w, reflect, act, bias = CASES[name]
    x, ws, bs = _inputs(name)
    out = {}
    for i, (wt, b, k) in enumerate(zip(ws, bs, KS)):
        z = F.conv2d(_pad(x.double(), k // 2, reflect), wt.double(), None if b is None else b.double())
        out['y%d' % k] = _act(z, act, SLOPE)
    return out


def _launch(dev, name, widths=None):
    from cat_amd import _lib as L, ops, tconv
    cin, xpad, case_widths, h, w, reflect, act, bias = CASES[name]
    x, ws, bs = _inputs(name)
    xcs = cs4(cin) + xpad
    xg = _nhwc_buffer(x, xcs, dev, pad_to=cs4(cin))
    keep, packs = [], []
    for wt in ws:
        wd = ops.padded_weight_like(tuple(wt.shape), dev)
        wd.copy_(wt.to(dev))
        keep.append(wd)
        packs.append(tconv.pack(wd, tconv.FWD))
    bgs = [None if b is None else b.to(dev) for b in bs]
    g = L.Stage1W7Geom()
    g.N, g.H, g.W, g.xcs, g.cin, g.reflect, g.act, g.slope = N, h, w, xcs, cin, reflect, act, SLOPE
    outs = []
    for k, m in enumerate(widths or case_widths):
        ycs = (144 if k == 3 else 48) + 4
        g.ycs[k], g.nvalid[k] = ycs, m
        outs.append(_sentinel((N, h, w, ycs), dev))
    arr = C.c_void_p * 4
    call = lambda: L.call('cat_tstage1w7_fwd', C.byref(g), ops._p(xg), arr(*[t.data_ptr() for t in packs]),
                          arr(*[None if b is None else b.data_ptr() for b in bgs]) if bias else None, arr(*[y.data_ptr() for flat, y in outs]),
                          ops._stream())
    return call, outs, (xg, keep, packs, bgs, g)


def test_the_cases_are_in_the_kernels_domain():
    assert all(supported(*CASES[k][2]) for k in CASES)
    assert {CASES[k][0] for k in CASES} >= {16, 20, 36} and any(CASES[k][1] for k in CASES)


@pytest.mark.gpu
def test_support_predicate_matches_its_mirror(dev):
    from cat_amd import _lib as L
    for w7 in (32, 33, 48, 49):
        for w5 in (0, 33, 48, 49):
            for w3 in (32, 42, 49):
                for w1 in (128, 129, 132, 144, 145, 176):
                    assert bool(L.query('cat_tstage1w7_supported', w7, w5, w3, w1)) == supported(w7, w5, w3, w1), (w7, w5, w3, w1)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_stage1w7_fwd(dev, name):
    cin, xpad, widths, h, w, reflect, act, bias = CASES[name]
    call, outs, keep = _launch(dev, name)
    call()
    torch.cuda.synchronize()
    got = {}
    for k, ((flat, y), m) in enumerate(zip(outs, widths)):
        yc = y.cpu()
        _columns(yc, range(144 if k == 3 else 48), range(m), (name, 'slot', k))
        _tail(flat, (name, 'slot', k))
        got['y%d' % KS[k]] = _nchw(yc, 0, m)
    _cmp('stage1w7', name, got, _ref(name))


@pytest.mark.gpu
def test_stage1w7_fwd_refuses_what_it_has_no_kernel_for(dev):
    """a width outside 3 + 3 + 3 + 9 N tiles, and a mirrored 7 x 7 window on a plane it does not fit in: an error, nothing launched"""
    from cat_amd import _lib as L
    assert not L.query('cat_tstage1w7_supported', 42, 42, 42, 176)      # the 1 3 5 teacher's 1 x 1 group
    call, outs, keep = _launch(dev, 'teacher-8x16-cin16', widths=(42, 42, 42, 176))
    with pytest.raises(RuntimeError, match='tstage1w7'):
        call()
    call, outs2, keep2 = _launch(dev, 'teacher-8x16-cin16', widths=(42, 32, 42, 132))
    with pytest.raises(RuntimeError, match='tstage1w7'):
        call()
    call, outs3, keep3 = _launch(dev, 'teacher-8x16-cin16')
    g = keep3[-1]
    g.reflect, g.H, g.W = 1, 6, 16
    with pytest.raises(RuntimeError, match='tstage1w7'):
        call()
    torch.cuda.synchronize()
    for flat, y in outs + outs2 + outs3:
        assert bool((flat == SENTINEL).all())
