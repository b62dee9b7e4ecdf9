"""cat_tstage1ws7_fwd (csrc/conv_s1ws7.hip) -- stage 1 of a wide InvertedResidualChannels block with kernel sizes 3 5 7 in one launch with
statistics: the 7 x 7, 5 x 5 and 3 x 3 first convs and the concatenated 1 x 1 group from one staging of the input, pre-norm slices of one
buffer + the per-tile statistics table -- through the C ABI against float64 ATen on the host (F.conv2d with explicit reflect / zero padding,
as tests/test_stage1w7_gpu.py), with the checks and the bar of tests/test_stage1ws_gpu.py (part B of tests/test_fused_kernels_gpu.py): every
slot's slice of the pre-norm buffer, zeros in the slices' padding columns, sentinels in every column of y and of the table outside the four
slices and behind the buffers, the per-tile sum and M2, then mean / variance out of cat_tnorm_finalize over that table (G = 1 with running
statistics, G = N).

Cases: N = 2; planes 9 x 17 (ragged tiles both ways: 128, 16, 16 and 1 valid pixels), 8 x 16 (one tile), 7 x 7 with reflect (the smallest
plane the mirror admits), 3 x 5 with zero padding (windows wider than the plane); cin 256 / 36 / 20 / 16 (16 chunks through both tile
buffers, a one-quad last chunk, a 4-channel tail chunk, one chunk); the teacher's slot widths (44, 44, 44, 132) with 42 valid channels per
branch and the domain's edges (36, 48, 44, 132) and (48, 36, 48, 144); with and without bias; an x pixel stride wider than cs4(cin)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_fused_kernels_gpu import (FWD, SENTINEL, _cmp, _columns, _concat_pack, _finalize_gpu, _host, _nchw, _nhwc_buffer, _norm_ref, _pad,
                                    _padded_weight, _profiled, _sentinel, _tail, _tile_stats, cdiv, cs4)

N = 2
KS = (7, 5, 3, 1)
# channels of the 7 x 7 / 5 x 5 / 3 x 3 residual branch and of the depthwise branches whose 1 x 1 first convs are N-concatenated
T = (42, 42, 42, (42, 42, 42))            # slot widths 44 / 44 / 44 / 132
EDGE_A = (33, 48, 42, (41, 43, 42))       # 36 / 48 / 44 / 132
EDGE_B = (48, 34, 46, (45, 47, 48))       # 48 / 36 / 48 / 144
# name -> (cin, extra pixel stride of x, branch channels, H, W, reflect, bias)
CASES = {
    'teacher-9x17-reflect-cin256': (256, 0, T, 9, 17, 1, 1),      # the teacher's depth: 16 chunks through both tile buffers; ragged tiles
    'teacher-9x17-zero-cin36': (36, 4, T, 9, 17, 0, 1),           # a one-quad last chunk
    'teacher-8x16-zero-cin16-nobias': (16, 0, T, 8, 16, 0, 0),    # one tile, one chunk
    'teacher-8x16-reflect-cin20': (20, 4, T, 8, 16, 1, 1),        # a 4-channel tail chunk
    'edge-a-7x7-reflect-cin20': (20, 0, EDGE_A, 7, 7, 1, 1),      # the smallest plane the 7 x 7 mirror admits
    'edge-b-3x5-zero-cin16': (16, 4, EDGE_B, 3, 5, 0, 1),         # windows wider than the plane
    'edge-a-3x5-zero-cin36-nobias': (36, 0, EDGE_A, 3, 5, 0, 0),
    'edge-b-9x17-reflect-cin36-nobias': (36, 0, EDGE_B, 9, 17, 1, 0),
}
DEEPEST, SHALLOWEST = 'teacher-9x17-reflect-cin256', 'edge-b-3x5-zero-cin16'      # K = 256 * 49 on 153 pixels; K = 16 on 15 pixels


def supported(w7, w5, w3, w1):
    """mirror of cat_tstage1ws7_supported: 3 + 3 + 3 + 9 N tiles"""
    return all(32 < v <= 48 for v in (w7, w5, w3)) and 128 < w1 <= 144


def _layout(name):
    """Z1 = [4 sentinel lanes | k = 1 slice | k = 3 slice | k = 5 slice | k = 7 slice | 4 sentinel lanes], the order of a plan -> slot widths,
    first columns (both by kernel size), pixel stride, branches (k, channels, first column)"""
    m7, m5, m3, m1c = CASES[name][2]
    width = {7: cs4(m7), 5: cs4(m5), 3: cs4(m3), 1: sum(cs4(m) for m in m1c)}
    col0, o = {}, 4
    for k in (1, 3, 5, 7):
        col0[k] = o
        o += width[k]
    ycs = o + 4
    branches, o = [], col0[1]
    for m in m1c:
        branches.append((1, m, o))
        o += cs4(m)
    branches += [(3, m3, col0[3]), (5, m5, col0[5]), (7, m7, col0[7])]
    return width, col0, ycs, branches


@functools.lru_cache(maxsize=None)
def _inputs(name):
    cin, xpad, chans, h, w, reflect, bias = CASES[name]
    ycs, branches = _layout(name)[2:]
    x = detfill.normal((N, cin, h, w), 1900)
    ws = [detfill.normal((m, cin, k, k), 1910 + i, 1.0 / (cin * k * k) ** 0.5) for i, (k, m, o) in enumerate(branches)]
    bs = [detfill.normal((m,), 1930 + i, 0.3) if bias else None for i, (k, m, o) in enumerate(branches)]
    gamma, beta = detfill.normal((ycs,), 1950).abs() + 0.5, detfill.normal((ycs,), 1951, 0.3)
    run = [(detfill.normal((m,), 1960 + i, 0.1), detfill.normal((m,), 1980 + i).abs() + 0.5) for i, (k, m, o) in enumerate(branches)]
    return x, ws, bs, gamma, beta, run


def _ref(name, dtype):
    cin, xpad, chans, h, w, reflect, bias = CASES[name]
    branches = _layout(name)[3]
    x, ws, bs, gamma, beta, run = _inputs(name)
    out = {}
    for i, (k, m, o) in enumerate(branches):
        z = F.conv2d(_pad(x.to(dtype), k // 2, reflect), ws[i].to(dtype), None if bs[i] is None else bs[i].to(dtype), padding=0)
        s, m2, _ = _tile_stats(z)
        out.update({'z%d' % i: z, 'sum%d' % i: s, 'm2%d' % i: m2})
        for tag, inst in (('b', 0), ('i', 1)):
            r = _norm_ref(z, inst, gamma[o:o + m], beta[o:o + m], None if inst else run[i][0], None if inst else run[i][1])
            out.update({'%s%s%d' % (tag, key, i): v for key, v in r.items()})
    return out


@functools.lru_cache(maxsize=None)
def _ref64(name):
    return _ref(name, torch.float64)


def test_cases_are_in_the_kernels_domain_and_the_bar_is_reachable():
    widths = {name: tuple(_layout(name)[0][k] for k in KS) for name in CASES}
    assert widths[DEEPEST] == (44, 44, 44, 132)
    assert {widths[n] for n in CASES} == {(44, 44, 44, 132), (36, 48, 44, 132), (48, 36, 48, 144)} and all(supported(*v) for v in widths.values())
    assert {CASES[n][0] for n in CASES} == {256, 36, 20, 16} and any(CASES[n][1] for n in CASES)
    assert {CASES[n][3:5] for n in CASES} == {(9, 17), (8, 16), (7, 7), (3, 5)} and {CASES[n][6] for n in CASES} == {0, 1}
    assert all(CASES[n][3] >= 7 and CASES[n][4] >= 7 for n in CASES if CASES[n][5])
    for name in (DEEPEST, SHALLOWEST):      # fp32 ATen within TOL / 10 of float64: a correct fp32 kernel has ten-fold room
        _host('B', name, lambda dt, name=name: _ref(name, dt))


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.mark.gpu
def test_support_predicate_matches_its_mirror(dev):
    from cat_amd import _lib as L
    for w7 in (32, 33, 48, 49):
        for w5 in (0, 32, 33, 48, 49):
            for w3 in (32, 33, 44, 48, 49):
                for w1 in (128, 129, 132, 144, 145, 176):
                    assert bool(L.query('cat_tstage1ws7_supported', w7, w5, w3, w1)) == supported(w7, w5, w3, w1), (w7, w5, w3, w1)


def _launch(dev, name):
    from cat_amd import _lib as L, ops
    cin, xpad, chans, h, w, reflect, bias = CASES[name]
    width, col0, ycs, branches = _layout(name)
    x, ws, bs, gamma, beta, run = _inputs(name)
    scs, tiles = ycs, N * cdiv(h, 8) * cdiv(w, 16)
    xg = _nhwc_buffer(x, cs4(cin) + xpad, dev, pad_to=cs4(cin))
    wgs = [_padded_weight(wt, dev) for wt in ws]
    # the filter streams as a plan builds them: one zeroed stream per slot, every branch packed at its column of the slot
    packs = {k: _concat_pack([(wgs[i], o - col0[k]) for i, (bk, m, o) in enumerate(branches) if bk == k], FWD, k, cin, width[k], dev) for k in KS}
    bvec = torch.zeros(ycs)
    for (k, m, o), b in zip(branches, bs):
        if b is not None:
            bvec[o:o + m] = b
    bg = bvec.to(dev) if bias else None
    gs = L.Stage1S7Geom()
    gs.N, gs.H, gs.W, gs.xcs, gs.cin, gs.reflect, gs.ycs, gs.scs = N, h, w, cs4(cin) + xpad, cin, reflect, ycs, scs
    pk = (C.c_void_p * 4)()
    for slot, k in enumerate(KS):
        gs.col0[slot], gs.width[slot], gs.nvalid[slot] = col0[k], width[k], sum(m for bk, m, o in branches if bk == k)
        pk[slot] = packs[k].data_ptr()
    zflat, z = _sentinel((N, h, w, ycs), dev)
    tflat, tab = _sentinel((tiles, 2, scs), dev)
    call = lambda: L.call('cat_tstage1ws7_fwd', C.byref(gs), ops._p(xg), pk, ops._p(bg), ops._p(z), ops._p(tab), ops._stream())
    return call, (zflat, z, tflat, tab), (gs, xg, pk, packs, wgs, bg)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(CASES))
def test_stage1ws7_fwd(dev, name):
    cin, xpad, chans, h, w, reflect, bias = CASES[name]
    width, col0, ycs, branches = _layout(name)
    x, ws, bs, gamma, beta, run = _inputs(name)
    call, (zflat, z, tflat, tab), keep = _launch(dev, name)
    _, fam = _profiled(call)
    assert fam.get('conv_tstage1ws7', 0) == 1, fam
    zc, tc = z.cpu(), tab.cpu()
    owned = [c for k in KS for c in range(col0[k], col0[k] + width[k])]
    valid = [c for k, m, o in branches for c in range(o, o + m)]
    _columns(zc, owned, valid, (name, 'Z1'))
    _columns(tc, owned, valid, (name, 'table'))
    _tail(zflat, (name, 'Z1'))
    _tail(tflat, (name, 'table'))
    got = {}
    for i, (k, m, o) in enumerate(branches):
        got.update({'z%d' % i: _nchw(zc, o, m), 'sum%d' % i: tc[:, 0, o:o + m], 'm2%d' % i: tc[:, 1, o:o + m]})
    pairs = [(o, m) for k, m, o in branches]
    for tag, inst in (('b', 0), ('i', 1)):
        r = _finalize_gpu(dev, tab, ycs, inst, N, h, w, gamma, beta, pairs, run, ycs)
        got.update({tag + key: v for key, v in r.items()})
    _cmp('B', name, got, _ref64(name))


@pytest.mark.gpu
def test_stage1ws7_fwd_refuses_what_it_has_no_kernel_for(dev):
    """widths outside 3 + 3 + 3 + 9 N tiles, and a reflect-padded plane smaller than the 7 x 7 window: an error, nothing written"""
    call, (zflat, z, tflat, tab), keep = _launch(dev, 'teacher-8x16-reflect-cin20')
    gs = keep[0]
    for slot, bad in ((3, 176), (3, 128), (0, 32), (1, 52)):
        good, gs.width[slot] = gs.width[slot], bad
        with pytest.raises(RuntimeError, match='tstage1ws7'):
            call()
        gs.width[slot] = good
    for hh, ww in ((6, 16), (8, 6)):
        gs.H, gs.W = hh, ww
        with pytest.raises(RuntimeError, match='tstage1ws7'):
            call()
    torch.cuda.synchronize()
    assert bool((zflat == SENTINEL).all()) and bool((tflat == SENTINEL).all())
