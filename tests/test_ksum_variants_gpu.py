"""The wide-tile convolution sum (csrc/conv_ksum.hip: ksum_kernel3 / 4 / 3n / 4n behind cat_conv2d_ksum_fwd and cat_conv2d_ksum_norm_fwd) through
the C ABI against float64 ATen on the host, at the edges of its own plan: the flat (tap, quad) walk with chunks that straddle a tap boundary,
the 1..3-quad remainder steps, both staging buffers, the 96- / 128-wide N-tile rule, the vector and the scalar epilogue, the prefetched
residual, the per-sample scale / shift table and the statistics reduced through LDS.

A (host): a Python mirror of ksum_launch (n96 rule, tile width, grid, kernel, profiler family) and of the chunk walk of issue(); the __global__
          kernels and the n96 expression parsed from conv_ksum.hip; a named list of regimes, each a predicate over (case, mirror output): every
          regime is declared by a case of B or C, every declaration is confirmed by the mirror, and every case is the only one to declare at least
          one regime (removing a case fails here, without a GPU); the float32 ATen twin of every reference within TOL / 10 of the float64 one;
          the two support predicates against Python mirrors over a grid of geometries (pure host functions of the library).
B (GPU):  cat_conv2d_ksum_fwd, one launch per case: family conv_ksum, columns [Cout, ycw) exactly 0, [ycw, ycs) and the tail still sentinel,
          rel() < TOL; one case twice, bit for bit.
C (GPU):  cat_conv2d_ksum_norm_fwd: the same on y, the raw table against _tile_stats on the kernel's lattice, cat_tnorm_finalize2 over that table
          against float64 instance statistics, the table's zero and sentinel columns.
D (GPU):  every clause of the two predicates and the CAT_REQUIREs of the launch: an error, nothing written.

Sources sit inside wider NHWC buffers whose neighbouring channels are NaN, filter lanes [c4, wcs) and scale / shift lanes outside a segment's
slice are NaN, the bias has NaN behind it, the residual NaN around it: a quad fetched from a neighbour poisons the output.  Channels [cin, c4)
of a source are 0 and meet zero filters (and scale = shift = 0), as include/cat_hip.h requires.

Bars: TOL = 1e-4 with rel() of test_kernels_gpu.py for every compared tensor, exact equality for zero lanes, sentinels and the repeated run.
Largest distances observed on an MI355X: KSUM_OBSERVED below (records, not thresholds)."""
import ctypes as C
import functools
import itertools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_fused_kernels_gpu import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_TANH, EPS, NAN, SENTINEL, _act, _cmp, _columns, _host, _nchw,
                                    _norm_ref, _pad, _profiled, _sentinel, _tail, _tile_stats, cdiv, cs4, dev)      # noqa: F401  (dev: fixture)
from test_kernels_gpu import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KSUM_SRC = os.path.join(ROOT, 'cat_amd', 'csrc', 'conv_ksum.hip')
MAXSEG, BM, NORM_TAB = 4, 128, 1024      # CAT_KSUM_MAXSEG; BM and kNormTab of conv_ksum.hip
KSUM_OBSERVED = 'B (plain) 1.6e-06, C (norm: y, table, finalize2) 9.9e-07'


# ================================================================================================ A1: mirrors
def ksum_launch(cout, ycw, m, norm):
    """ksum_launch of conv_ksum.hip: 96-wide N tiles where they pad less than 128-wide ones; N tiles up to max(ycw, Cout)"""
    n96 = cdiv(cout, 96) * 96 < cdiv(cout, 128) * 128
    bn = 96 if n96 else 128
    ntn = cdiv(max(ycw, cout), bn)
    return dict(n96=n96, bn=bn, ntn=ntn, grid=cdiv(m, BM) * ntn, kernel='ksum_kernel%d%s' % (3 if n96 else 4, 'n' if norm else ''),
                family='conv_ksum_norm' if norm else 'conv_ksum')


def ksum_walk(segs):
    """issue() of ksum_body: per segment (q quads per tap, k) the chunks it fetches, in order: nq quads starting at quad q0 of `tap`;
    `straddles`: the chunk ends with quads of tap + 1; `buf`: the staging buffer it lands in (the chunks of a launch alternate)"""
    out, index = [], 0
    for q, k in segs:
        taps, flat, tap, q0, seq = k * k, q >= 8, 0, 0, []
        while tap < taps:
            left = (taps - tap) * q - q0
            nq = min(8, left) if flat else q
            seq.append(dict(nq=nq, straddles=q0 + nq > q, tap=tap, q0=q0, buf=index & 1))
            index += 1
            q0 += nq
            if q0 >= q:
                q0, tap = q0 - q, tap + 1
        out.append(seq)
    return out


def lattice(h, w):
    if w <= BM and BM % w == 0 and h % (BM // w) == 0:
        return BM // w, w
    return (1, BM) if w % BM == 0 else None


# ================================================================================================ case tables
def S(cin, k, lo=4, hi=4, wpad=0, nrm=None):
    """one segment: cin valid channels in a slot of cs4(cin), a k x k filter; the source's channels sit at offset `lo` of a pixel of
    lo + c4 + hi floats, a filter tap holds c4 + wpad floats; nrm = (staging activation, slope, rows): rows 'wide' = per-image rows inside a
    wider row (pointer offset, sstride > c4), 'image' = per-image rows of c4 floats, 'batch' = one row (sstride 0); None = read as it is"""
    return dict(cin=cin, c4=cs4(cin), k=k, lo=lo, hi=hi, wpad=wpad, nrm=nrm)


def K(n, h, w, segs, cout, reflect, regimes, ycw=None, ycs=None, bias=True, res=None, act=ACT_NONE, slope=0.2, stats=False, norm=False):
    """res: None or (rcs, offset of the residual's first channel inside its pixel); ycw as passed to the launch (0: Cout)"""
    ycw = cs4(cout) if ycw is None else ycw
    ycs = max(ycw, cs4(cout)) + 8 if ycs is None else ycs
    return dict(n=n, h=h, w=w, segs=segs, cout=cout, reflect=reflect, regimes=tuple(regimes), ycw=ycw, ycs=ycs, bias=bias, res=res, act=act,
                slope=slope, stats=stats, norm=norm, scs=max(ycw, cout) + 4)


WIDE0, WIDE02, WIDE1 = (ACT_RELU, 0.0, 'wide'), (ACT_LRELU, 0.2, 'wide'), (ACT_LRELU, 1.0, 'wide')

B_CASES = {
    # the frozen teacher's tail on one 8 x 16 plane, K = 176 + 9 * 44 + 25 * 44 = 1672: 44 quads of a 1 x 1 (5 chunks + 4 quads), 11 quads
    # per tap of the 3 x 3 (13 chunks: the 5 x 5 starts in buffer 1) and of the 5 x 5; run twice
    'teacher-tail': K(1, 8, 16, [S(176, 1), S(42, 3), S(42, 5)], 256, 1,
                      ['cout-256', 'mix-k135', 'kx-wrap-straddle', 'last-r0', 'last-nfull1', 'seg-starts-buf0', 'seg-starts-buf1', 'res-cs4', 'cin<c4',
                       'act-none'], res=(256, 0)),
    # zero padding, 9 and 11 quads per tap: straddling chunks on the 1- and 2-pixel frame; 126 pixels
    'zero-frame': K(2, 7, 9, [S(36, 3), S(44, 5)], 64, 0, ['cout-64', 'zero-frame-k3', 'zero-frame-k5', 'M<128', 'last-r1', 'last-nfull0',
                                                          'res-none', 'bias-null'], bias=False),
    # 1, 2, 3 and 4 quads per tap: remainder-only chunks; four segments; the scalar epilogue with a residual of stride 79
    'small-quads': K(3, 9, 11, [S(4, 5), S(8, 3), S(12, 1), S(16, 3)], 77, 0,
                     ['q1', 'q2', 'q3', 'q4', 'nseg-max', 'cout-77', 'ycw-0', 'M-ragged-tiles', 'res-rcs%4', 'res-cout%4', 'act-relu'], ycw=0, ycs=88,
                     res=(79, 2), act=ACT_RELU),
    # 5 .. 8 quads per tap; 96-wide tiles with a ragged second one; the residual inside a wider NaN buffer
    'mid-quads': K(1, 12, 12, [S(20, 3), S(24, 1), S(28, 5), S(32, 3)], 130, 1,
                   ['q5', 'q6', 'q7', 'q8', 'cout-130', 'ycs>ycw>cout', 'res-wide-nan', 'act-lrelu'], ycw=136, ycs=144, res=(140, 4), act=ACT_LRELU),
    # 10 quads x 9 taps ends on 2 quads, 13 quads of a 1 x 1 on 4 + 1; a 5 x 5 on a plane one pixel wide
    'column-plane': K(2, 20, 1, [S(40, 3), S(52, 1), S(8, 5)], 96, 0, ['cout-96', 'last-r2', 'zero-5x5-thin', 'ycw=ycs', 'act-relu6'], ycw=96, ycs=96,
                      res=(96, 0), act=ACT_RELU6),
    'reflect-3x3': K(2, 3, 3, [S(44, 5)], 97, 1, ['cout-97', 'reflect-3x3-k5', 'nseg-1', 'last-r3', 'act-tanh', 'bias'], res=(100, 0), act=ACT_TANH),
    'reflect-2x2': K(3, 2, 2, [S(40, 3, wpad=4)], 129, 1, ['cout-129', 'reflect-2x2-k3', 'idle-wave', 'wcs>c4']),
    # a 128-pixel row tile over six samples of 25 pixels
    'span-reflect': K(6, 5, 5, [S(36, 3), S(8, 5)], 128, 1, ['cout-128', 'span-reflect']),
    'span-zero': K(7, 5, 5, [S(44, 5), S(12, 3)], 192, 0, ['cout-192', 'span-zero']),
    'two-128': K(1, 4, 8, [S(32, 1, lo=8)], 193, 0, ['cout-193', 'xcs-offset']),
    'three-96': K(1, 4, 8, [S(16, 1)], 257, 0, ['cout-257']),
    # the promise of include/cat_hip.h for columns beyond the last N tile of Cout
    'hole-128': K(1, 8, 16, [S(20, 3)], 128, 1, ['ycw-hole-128'], ycw=136, ycs=144),
    'hole-96': K(1, 8, 16, [S(20, 3)], 96, 1, ['ycw-hole-96'], ycw=100, ycs=108),
}

C_CASES = {
    # stage 2 of a wide InstanceNorm block as frozen_in._wide_segs calls it: slices of one wide row per sample, three samples of one tile each
    'wide-rows': K(3, 8, 16, [S(44, 1, nrm=WIDE0), S(132, 1, nrm=WIDE0), S(44, 3, nrm=WIDE0), S(44, 5, nrm=WIDE0)], 256, 1,
                   ['lat-16x8-n3', 'rows-wide', 'norm-straddle', 'norm-remainder', 'nslope-0'], stats=True, norm=True),
    'between': K(2, 64, 2, [S(20, 3, nrm=(ACT_LRELU, 0.2, 'image')), S(24, 1), S(12, 1, nrm=(ACT_LRELU, 0.2, 'batch'))], 72, 1,
                 ['lat-2x64', 'unnormalised-between', 'rows-batch', 'nslope-0.2', 'norm-bn96'], stats=True, norm=True),
    'w256': K(1, 2, 256, [S(44, 3, nrm=WIDE1)], 100, 1, ['lat-w128k', 'nslope-1', 'norm-bn128'], stats=True, norm=True, bias=False),
    # a plane one pixel wide admits no reflection: the normalised segment is a 1 x 1, the 3 x 3 is read as it is under zero padding
    'w1': K(2, 128, 1, [S(36, 1, nrm=(ACT_RELU, 0.0, 'image')), S(8, 3)], 64, 0, ['lat-1x128'], stats=True, norm=True),
    # ksum.run_norm(stats=False, res=...)
    'nostats-res': K(2, 8, 16, [S(44, 3, nrm=WIDE02), S(20, 1)], 130, 1, ['nostats-res-relu'], res=(132, 0), act=ACT_RELU, norm=True),
    'table-1024': K(1, 8, 16, [S(256, 1, nrm=(ACT_RELU, 0.0, 'image'))] * 4, 64, 0, ['table-1024'], stats=True, norm=True),
    'norm-hole-128': K(1, 8, 16, [S(16, 1, nrm=(ACT_RELU, 0.0, 'batch'))], 128, 0, ['norm-ycw-hole-128'], ycw=136, ycs=144, stats=True, norm=True),
    'norm-hole-96': K(1, 8, 16, [S(16, 1, nrm=(ACT_RELU, 0.0, 'batch'))], 96, 0, ['norm-ycw-hole-96'], ycw=100, ycs=108, stats=True, norm=True),
}
CASES = dict(B_CASES, **C_CASES)
TWICE = 'teacher-tail'


def plan(c):
    p = ksum_launch(c['cout'], c['ycw'], c['n'] * c['h'] * c['w'], c['norm'])
    p['walk'] = ksum_walk([(s['c4'] // 4, s['k']) for s in c['segs']])
    p['M'] = c['n'] * c['h'] * c['w']
    return p


# ================================================================================================ A3: regimes
def _qs(c):
    return [s['c4'] // 4 for s in c['segs']]


def _chunks(c, p, pred=lambda s, ch: True):
    return [(s, ch) for s, seq in zip(c['segs'], p['walk']) for ch in seq if pred(s, ch)]


def _last_short(c, p):
    """the short last chunks of the flat-walk segments"""
    return [seq[-1] for s, seq in zip(c['segs'], p['walk']) if s['c4'] >= 32 and seq[-1]['nq'] < 8]


def _frame(c, p, k):
    """zero padding, straddling chunks of a k x k segment: which of (current tap in the plane, next tap outside) / the reverse some pixel meets"""
    seen = set()
    if c['reflect']:
        return seen
    for s, ch in _chunks(c, p, lambda s, ch: s['k'] == k and ch['straddles']):
        inside = lambda tap, oy, ox: 0 <= oy + tap // k - k // 2 < c['h'] and 0 <= ox + tap % k - k // 2 < c['w']
        for oy, ox in itertools.product(range(c['h']), range(c['w'])):
            a, b = inside(ch['tap'], oy, ox), inside(ch['tap'] + 1, oy, ox)
            if a != b:
                seen.add('in-out' if a else 'out-in')
    return seen


def _normed(c):
    return [s for s in c['segs'] if s['nrm']]


def _nslope(s):
    act, slope, _ = s['nrm']
    return {ACT_RELU: 0.0, ACT_LRELU: slope, ACT_NONE: 1.0}[act]


def _res(c, pred=lambda rcs, off: True):
    return c['res'] is not None and pred(*c['res'])


REGIMES = {
    # ---- walk
    **{'q%d' % q: (lambda c, p, q=q: q in _qs(c)) for q in range(1, 9)},
    'kx-wrap-straddle': lambda c, p: any(_chunks(c, p, lambda s, ch: s['c4'] > 32 and s['k'] > 1 and ch['straddles'] and (ch['tap'] + 1) % s['k'] == 0)),
    **{'last-r%d' % r: (lambda c, p, r=r: any(ch['nq'] & 3 == r for ch in _last_short(c, p))) for r in range(4)},
    'last-nfull0': lambda c, p: any(ch['nq'] >> 2 == 0 for ch in _last_short(c, p)),
    'last-nfull1': lambda c, p: any(ch['nq'] >> 2 == 1 for ch in _last_short(c, p)),
    'seg-starts-buf0': lambda c, p: any(seq[0]['buf'] == 0 for seq in p['walk'][1:]),
    'seg-starts-buf1': lambda c, p: any(seq[0]['buf'] == 1 for seq in p['walk'][1:]),
    'nseg-1': lambda c, p: len(c['segs']) == 1,
    'nseg-max': lambda c, p: len(c['segs']) == MAXSEG,
    'mix-k135': lambda c, p: {s['k'] for s in c['segs']} == {1, 3, 5},
    # ---- borders
    'zero-frame-k3': lambda c, p: _frame(c, p, 3) == {'in-out', 'out-in'},
    'zero-frame-k5': lambda c, p: _frame(c, p, 5) == {'in-out', 'out-in'},
    'zero-5x5-thin': lambda c, p: not c['reflect'] and 1 in (c['h'], c['w']) and any(s['k'] == 5 for s in c['segs']),
    'reflect-3x3-k5': lambda c, p: c['reflect'] and (c['h'], c['w']) == (3, 3) and any(s['k'] == 5 for s in c['segs']),
    'reflect-2x2-k3': lambda c, p: c['reflect'] and (c['h'], c['w']) == (2, 2) and any(s['k'] == 3 for s in c['segs']),
    # ---- rows
    'M<128': lambda c, p: p['M'] < BM,
    'M-ragged-tiles': lambda c, p: p['M'] % BM and p['M'] > 2 * BM,
    'span-reflect': lambda c, p: c['h'] * c['w'] == 25 and c['n'] >= 6 and c['reflect'] and any(s['k'] > 1 for s in c['segs']),
    'span-zero': lambda c, p: c['h'] * c['w'] == 25 and c['n'] >= 6 and not c['reflect'] and any(s['k'] > 1 for s in c['segs']),
    # ---- columns
    **{'cout-%d' % n: (lambda c, p, n=n: c['cout'] == n) for n in (64, 96, 97, 128, 129, 192, 193, 256, 257, 77, 130)},
    'idle-wave': lambda c, p: (c['cout'] - 1) % p['bn'] + 1 <= p['bn'] // 2,
    # ---- output
    'ycs>ycw>cout': lambda c, p: c['ycs'] > c['ycw'] > c['cout'],
    'ycw-0': lambda c, p: c['ycw'] == 0 and c['cout'] % 4 != 0,
    'ycw=ycs': lambda c, p: c['ycw'] == c['ycs'],
    'ycw-hole-128': lambda c, p: not c['norm'] and (c['cout'], c['ycw'], c['ycs']) == (128, 136, 144) and p['ntn'] == 2 and not p['n96'],
    'ycw-hole-96': lambda c, p: not c['norm'] and (c['cout'], c['ycw']) == (96, 100) and p['ntn'] == 2 and p['n96'],
    'norm-ycw-hole-128': lambda c, p: c['stats'] and (c['cout'], c['ycw'], c['ycs']) == (128, 136, 144) and p['ntn'] == 2 and not p['n96'],
    'norm-ycw-hole-96': lambda c, p: c['stats'] and (c['cout'], c['ycw']) == (96, 100) and p['ntn'] == 2 and p['n96'],
    # ---- residual
    'res-none': lambda c, p: c['res'] is None,
    'res-cs4': lambda c, p: _res(c, lambda rcs, off: rcs == cs4(c['cout']) and off == 0),
    'res-wide-nan': lambda c, p: _res(c, lambda rcs, off: rcs % 4 == 0 and off > 0 and rcs > off + c['cout']),
    'res-rcs%4': lambda c, p: _res(c, lambda rcs, off: rcs % 4 != 0),
    'res-cout%4': lambda c, p: _res(c) and c['cout'] % 4 != 0,
    # ---- epilogue (each activation in front of a residual)
    'act-none': lambda c, p: c['act'] == ACT_NONE and _res(c),
    'act-relu': lambda c, p: c['act'] == ACT_RELU and _res(c),
    'act-lrelu': lambda c, p: c['act'] == ACT_LRELU and c['slope'] == 0.2 and _res(c),
    'act-relu6': lambda c, p: c['act'] == ACT_RELU6 and _res(c),
    'act-tanh': lambda c, p: c['act'] == ACT_TANH and _res(c),
    'bias-null': lambda c, p: not c['bias'],
    'bias': lambda c, p: c['bias'],
    # ---- strides
    'xcs-offset': lambda c, p: any(s['lo'] > 4 for s in c['segs']),
    'wcs>c4': lambda c, p: any(s['wpad'] > 0 for s in c['segs']),
    'cin<c4': lambda c, p: any(s['cin'] < s['c4'] for s in c['segs']),
    # ---- the normalising form
    'rows-wide': lambda c, p: c['n'] > 1 and any(s['nrm'][2] == 'wide' for s in _normed(c)),
    'rows-batch': lambda c, p: c['n'] > 1 and any(s['nrm'][2] == 'batch' for s in _normed(c)),
    'unnormalised-between': lambda c, p: any(a['nrm'] and not b['nrm'] and d['nrm'] for a, b, d in zip(c['segs'], c['segs'][1:], c['segs'][2:])),
    'norm-straddle': lambda c, p: any(_chunks(c, p, lambda s, ch: s['nrm'] and ch['straddles'])),
    'norm-remainder': lambda c, p: any(_chunks(c, p, lambda s, ch: s['nrm'] and ch['nq'] & 3)),
    'nostats-res-relu': lambda c, p: c['norm'] and not c['stats'] and _res(c) and c['act'] == ACT_RELU and p['family'] == 'conv_ksum_norm',
    'nslope-0': lambda c, p: any(_nslope(s) == 0.0 for s in _normed(c)),
    'nslope-0.2': lambda c, p: any(_nslope(s) == 0.2 for s in _normed(c)),
    'nslope-1': lambda c, p: any(_nslope(s) == 1.0 for s in _normed(c)),
    'lat-w128k': lambda c, p: c['stats'] and c['w'] % BM == 0 and lattice(c['h'], c['w']) == (1, BM),
    'lat-2x64': lambda c, p: c['stats'] and (c['w'], c['h']) == (2, 64),
    'lat-1x128': lambda c, p: c['stats'] and (c['w'], c['h']) == (1, 128),
    'lat-16x8-n3': lambda c, p: c['stats'] and (c['w'], c['h'], c['n']) == (16, 8, 3),
    'norm-bn96': lambda c, p: c['stats'] and _normed(c) and c['cout'] <= 96 and p['kernel'] == 'ksum_kernel3n',
    'norm-bn128': lambda c, p: c['stats'] and _normed(c) and 97 <= c['cout'] <= 128 and p['kernel'] == 'ksum_kernel4n',
    'table-1024': lambda c, p: sum(s['c4'] for s in _normed(c)) == NORM_TAB,
}


def test_mirror_of_the_launch_and_the_walk():
    """A1: the mirrors on the geometries the kernel's comments spell out"""
    assert [ch['nq'] for ch in ksum_walk([(11, 3)])[0]] == [8] * 12 + [3]
    w = ksum_walk([(11, 3)])[0]
    assert (w[1]['tap'], w[1]['q0'], w[1]['straddles']) == (0, 8, True) and not w[0]['straddles']      # 8, then 3 of this tap + 5 of the next
    assert [(ch['nq'], ch['tap'], ch['straddles']) for ch in ksum_walk([(3, 3)])[0]] == [(3, t, False) for t in range(9)]      # q < 8: one tap per chunk
    assert [ch['nq'] for ch in ksum_walk([(44, 1)])[0]] == [8] * 5 + [4] and [ch['nq'] for ch in ksum_walk([(13, 1)])[0]] == [8, 5]
    assert [ksum_walk([(q, k)])[0][-1]['nq'] for q, k in ((9, 3), (10, 3), (11, 3), (11, 5))] == [1, 2, 3, 3]
    assert [seq[0]['buf'] for seq in ksum_walk([(44, 1), (11, 3), (11, 5)])] == [0, 0, 1]
    for segs in ([(11, 3)], [(9, 5), (16, 3)], [(8, 3)], [(44, 1), (11, 5)]):      # every quad of every tap exactly once, at most one tap boundary per chunk
        for (q, k), seq in zip(segs, ksum_walk(segs)):
            flat = [(ch['tap'] + (ch['q0'] + i) // q, (ch['q0'] + i) % q) for ch in seq for i in range(ch['nq'])]
            assert flat == [(t, i) for t in range(k * k) for i in range(q)]
            assert all(ch['q0'] + ch['nq'] <= 2 * q and ch['straddles'] == (ch['q0'] + ch['nq'] > q) for ch in seq)
    assert ksum_launch(176, 176, 2 * 16 * 16, False) == dict(n96=True, bn=96, ntn=2, grid=8, kernel='ksum_kernel3', family='conv_ksum')
    assert ksum_launch(256, 256, 128, True) == dict(n96=False, bn=128, ntn=2, grid=2, kernel='ksum_kernel4n', family='conv_ksum_norm')
    for cout in range(1, 700):      # ycw = cs_for(Cout), as every model passes it: the zero columns never add a tile
        assert ksum_launch(cout, cs4(cout), BM, False)['ntn'] == cdiv(cout, ksum_launch(cout, 0, BM, False)['bn'])


def test_kernels_and_tile_rule_of_the_source_match_the_mirror():
    """A2: the __global__ kernels of conv_ksum.hip are the ones the case tables reach; its n96 and grid expressions are the mirror's"""
    src = open(KSUM_SRC).read()
    kernels = set(re.findall(r'__global__[^\n;{]*\bvoid\s+(\w+)\s*\(', src))
    assert kernels == {'ksum_kernel3', 'ksum_kernel4', 'ksum_kernel3n', 'ksum_kernel4n'}, kernels
    assert {plan(c)['kernel'] for c in CASES.values()} == kernels
    assert {(plan(c)['kernel'], plan(c)['family']) for c in B_CASES.values()} == {('ksum_kernel3', 'conv_ksum'), ('ksum_kernel4', 'conv_ksum')}
    assert {(plan(c)['kernel'], plan(c)['family']) for c in C_CASES.values()} == {('ksum_kernel3n', 'conv_ksum_norm'), ('ksum_kernel4n', 'conv_ksum_norm')}
    m = re.search(r'const bool n96 = ([^;]+);', src)
    assert m, 'the n96 rule of ksum_launch'
    expr = re.sub(r'cat::cdiv\(g->Cout, (\d+)\)', r'cdiv(cout, \1)', m.group(1))
    assert re.fullmatch(r'[\w\s(),*<]+', expr) and 'g->' not in expr, expr
    for cout in range(1, 700):
        assert bool(eval(expr, {'cdiv': cdiv, 'cout': cout})) == ksum_launch(cout, 0, 1, False)['n96'], cout
    assert re.search(r'const int bn = n96 \? 96 : 128;', src)
    assert re.search(r'grid = \(int64_t\)cat::cdiv\(M, cat_ks::BM\) \* cat::cdiv\(a\.ycw, bn\);', src), 'N tiles up to max(ycw, Cout)'
    assert re.search(r'a\.ycw = g->ycw > g->Cout \? g->ycw : g->Cout;', src)
    assert re.search(r'#define CAT_KSUM_MAXSEG %d\b' % MAXSEG, open(os.path.join(ROOT, 'include', 'cat_hip.h')).read())
    assert re.search(r'constexpr int kNormTab = %d;' % NORM_TAB, src) and re.search(r'constexpr int BM = %d\b' % BM, src)


def test_case_tables_reach_every_regime():
    """A3: every regime has a case that declares it, the mirror confirms every declaration, and every case stands alone for some regime"""
    declared = {}
    for name, c in CASES.items():
        p = plan(c)
        assert c['regimes'], name
        for r in c['regimes']:
            assert r in REGIMES, (name, r)
            assert REGIMES[r](c, p), (name, r, 'declared, but the mirror does not confirm it')
            declared.setdefault(r, []).append(name)
    assert sorted(set(REGIMES) - set(declared)) == [], 'regimes without a case'
    for name, c in CASES.items():
        assert any(declared[r] == [name] for r in c['regimes']), (name, 'declares no regime of its own')
    assert TWICE in B_CASES
    for name, c in CASES.items():      # what the tables promise beyond the regimes
        assert all(s['lo'] >= 4 and s['hi'] >= 4 and s['lo'] % 4 == 0 and s['hi'] % 4 == 0 for s in c['segs']), (name, 'NaN neighbours on both sides')
        assert c['ycs'] % 4 == 0 and c['ycs'] >= max(c['ycw'], c['cout']) and c['scs'] > max(c['ycw'], c['cout'])
        assert c['n'] * c['h'] * c['w'] <= 512 and sum(s['c4'] * s['k'] ** 2 for s in c['segs']) <= 1700, (name, 'a small launch')
        assert c['res'] is None or c['res'][0] >= c['res'][1] + c['cout']
        assert (name in C_CASES) == c['norm'] and (not c['stats'] or (c['norm'] and lattice(c['h'], c['w']) and c['act'] == ACT_NONE and c['res'] is None))
        assert all(not s['nrm'] or s['k'] == 1 or c['reflect'] for s in c['segs'])


# ================================================================================================ inputs and references
@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = CASES[name]
    n, h, w, cout = c['n'], c['h'], c['w'], c['cout']
    seed = 3000 + 50 * sorted(CASES).index(name)
    fan = sum(s['cin'] * s['k'] ** 2 for s in c['segs'])
    xs, ws, tabs = [], [], []
    for i, s in enumerate(c['segs']):
        xs.append(detfill.normal((n, s['cin'], h, w), seed + i))
        ws.append(detfill.normal((cout, s['cin'], s['k'], s['k']), seed + 10 + i, fan ** -0.5))
        G = 1 if s['nrm'] and s['nrm'][2] == 'batch' else n
        tabs.append((detfill.normal((G, s['cin']), seed + 20 + i).abs() + 0.5, detfill.normal((G, s['cin']), seed + 30 + i, 0.3)) if s['nrm'] else None)
    return dict(xs=xs, ws=ws, tabs=tabs, bias=detfill.normal((cout,), seed + 40, 0.2) if c['bias'] else None,
                res=detfill.normal((n, cout, h, w), seed + 41) if c['res'] else None,
                gamma=detfill.normal((cout,), seed + 42).abs() + 0.5, beta=detfill.normal((cout,), seed + 43, 0.3))


def _ref(name, dtype):
    c, inp = CASES[name], _inputs(name)
    y = None
    for s, x, wt, tab in zip(c['segs'], inp['xs'], inp['ws'], inp['tabs']):
        a = x.to(dtype)
        if s['nrm']:
            sc, sh = (t.to(dtype).expand(c['n'], -1)[:, :, None, None] for t in tab)
            a = _act(a * sc + sh, s['nrm'][0], s['nrm'][1])
        t = F.conv2d(_pad(a, s['k'] // 2, c['reflect']), wt.to(dtype))
        y = t if y is None else y + t
    if c['bias']:
        y = y + inp['bias'].to(dtype).view(1, -1, 1, 1)
    out = {'y': _act(y, c['act'], c['slope'])}
    if c['res']:
        out['y'] = out['y'] + inp['res'].to(dtype)
    if c['stats']:      # of the sum in front of the epilogue, per lattice tile, and what cat_tnorm_finalize2 makes of them
        out['sum'], out['m2'], _ = _tile_stats(y, *lattice(c['h'], c['w']))
        out.update(_norm_ref(y, True, inp['gamma'], inp['beta']))
    return out


def test_fp32_twin_of_every_reference_is_within_a_tenth_of_the_bar():
    """A4: float32 ATen against float64 ATen on the host, <= TOL / 10 for every tensor a GPU case compares"""
    for name in CASES:
        _host('KB' if name in B_CASES else 'KC', name, functools.partial(_ref, name))


# ================================================================================================ the support predicates
def _i(v):
    return int(v or 0)


def supported(g):
    """cat_conv2d_ksum_supported over the ctypes struct"""
    if not (1 <= g.nseg <= MAXSEG) or min(g.N, g.H, g.W, g.Cout) <= 0:
        return False
    refl = None
    for s in range(g.nseg):
        sg = g.seg[s]
        if sg.ks not in (1, 3, 5) or sg.c4 <= 0 or sg.c4 % 4 or sg.xcs % 4 or sg.xcs < sg.c4 or sg.wcs % 4 or sg.wcs < sg.c4:
            return False
        if g.N * g.H * g.W * sg.xcs * 4 >= 2147483647 or g.Cout * sg.ks * sg.ks * sg.wcs * 4 >= 2147483647:
            return False
        if sg.ks > 1:
            if refl is not None and refl != bool(sg.reflect):
                return False
            refl = bool(sg.reflect)
            if sg.reflect and (sg.ks // 2 >= g.H or sg.ks // 2 >= g.W):
                return False
    return True


def norm_supported(g, nm):
    """cat_conv2d_ksum_norm_supported over the ctypes structs"""
    if not supported(g) or lattice(g.H, g.W) is None:
        return False
    ntab = 0
    for s in range(g.nseg):
        ns = nm.seg[s]
        if bool(ns.scale) != bool(ns.shift):
            return False
        if not ns.scale:
            continue
        if ns.sstride < 0 or (ns.sstride != 0 and ns.sstride < g.seg[s].c4):
            return False
        if ns.act not in (ACT_NONE, ACT_RELU, ACT_LRELU) or (ns.act == ACT_LRELU and not 0.0 <= ns.slope <= 1.0):
            return False
        if g.seg[s].ks > 1 and not g.seg[s].reflect:
            return False
        ntab += g.seg[s].c4
    if ntab > NORM_TAB:
        return False
    return not (nm.stats and (g.act != ACT_NONE or nm.scs < max(g.ycw, g.Cout)))


def _lib():
    from cat_amd import _lib as L
    L.load()
    return L


def _geoms(L, n, h, w, cout, segs, ycs=64, ycw=64, act=ACT_NONE, stats=16, scs=64):
    """segs: (ks, c4, xcs, wcs, reflect, normalised, sstride, staging act, slope); addresses are tokens, the predicates read no memory"""
    g, nm = L.KSum(), L.KSumNorm()
    g.N, g.H, g.W, g.Cout, g.ycs, g.ycw, g.rcs, g.act, g.slope, g.nseg = n, h, w, cout, ycs, ycw, 64, act, 0.2, len(segs)
    nm.stats, nm.scs = stats, scs
    for t, gs, (ks, c4, xcs, wcs, reflect, nrm, sstride, sact, slope) in zip(nm.seg, g.seg, segs):
        gs.src, gs.w, gs.xcs, gs.c4, gs.cin, gs.ks, gs.reflect, gs.wcs = 16, 16, xcs, c4, c4, ks, reflect, wcs
        if nrm:
            t.scale, t.shift, t.sstride, t.act, t.slope = (16 if nrm & 1 else None), (16 if nrm & 2 else None), sstride, sact, slope
    return g, nm


def test_support_predicates_match_their_mirrors():
    """both predicates are pure host functions: every clause on both sides, one and two segments"""
    L = _lib()
    seen = {True: 0, False: 0}

    def check(g, nm):
        a, b = supported(g), norm_supported(g, nm)
        assert bool(L.query('cat_conv2d_ksum_supported', C.byref(g))) == a, 'plain'
        assert bool(L.query('cat_conv2d_ksum_norm_supported', C.byref(g), C.byref(nm))) == b, 'norm'
        seen[a] += 1
        seen[b] += 1
    base = (3, 8, 8, 8, 1, 3, 8, ACT_RELU, 0.0)
    for ks, c4, xcs, wcs, reflect in itertools.product((1, 3, 5, 7), (0, 6, 8), (4, 8, 10, 12), (4, 8, 10, 12), (0, 1)):
        for h, w in ((8, 16), (2, 64), (1, 128), (3, 3), (2, 256), (12, 12), (8, 24)):
            check(*_geoms(L, 2, h, w, 64, [(ks, c4, xcs, wcs, reflect, 3, 8, ACT_RELU, 0.0)]))
    for k2, r2, nrm, sstride, sact, slope in itertools.product((1, 3), (0, 1), (0, 1, 2, 3), (-4, 0, 4, 8, 12), (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH),
                                                              (-0.5, 0.0, 1.0, 1.5)):
        check(*_geoms(L, 2, 8, 16, 64, [base, (k2, 8, 8, 8, r2, nrm, sstride, sact, slope)]))
    for act, stats, scs, ycw, cout in itertools.product((ACT_NONE, ACT_RELU), (None, 16), (60, 64, 68, 72), (0, 64, 72), (64, 66)):
        check(*_geoms(L, 1, 8, 16, cout, [base], ycs=72, ycw=ycw, act=act, stats=stats, scs=scs))
    for widths in ((256, 256, 256, 256), (260, 256, 256, 256), (256, 256, 256, 252), (512, 516)):
        g, nm = _geoms(L, 1, 8, 16, 64, [(1, c, c, c, 0, 3, 0, ACT_RELU, 0.0) for c in widths])
        assert norm_supported(g, nm) == (sum(widths) <= NORM_TAB)
        check(g, nm)
    g, nm = _geoms(L, 1, 8, 16, 64, [base])
    for nseg in (0, 1, MAXSEG + 1):
        g.nseg = nseg
        check(g, nm)
    for n, cout in ((1 << 20, 64), (1 << 22, 64), (1, 1 << 22), (1, 1 << 24), (0, 64), (1, 0)):      # tensors of 2 GB and more
        check(*_geoms(L, n, 8, 16, cout, [base]))
    assert seen[True] > 100 and seen[False] > 100, seen


# ================================================================================================ GPU plumbing
def _nan_tail(t, dev):
    """a host tensor on the device with four NaN behind it (what lies behind a bias)"""
    return torch.cat([t.reshape(-1).float(), torch.full((4,), NAN)]).to(dev)


def _device(dev, name):
    """-> (cat_ksum_t, cat_ksum_norm_t without the table, bias / residual addresses, tensors to keep alive)"""
    L = _lib()
    c, inp = CASES[name], _inputs(name)
    n, h, w, cout = c['n'], c['h'], c['w'], c['cout']
    g, nm, keep = L.KSum(), L.KSumNorm(), []
    g.N, g.H, g.W, g.Cout, g.ycs, g.ycw, g.act, g.slope, g.nseg = n, h, w, cout, c['ycs'], c['ycw'], c['act'], c['slope'], len(c['segs'])
    for i, (s, x, wt, tab) in enumerate(zip(c['segs'], inp['xs'], inp['ws'], inp['tabs'])):
        cin, c4, k, lo = s['cin'], s['c4'], s['k'], s['lo']
        xcs, wcs = lo + c4 + s['hi'], c4 + s['wpad']
        xb = torch.full((n, h, w, xcs), NAN)
        xb[..., lo:lo + c4] = 0.0
        xb[..., lo:lo + cin] = x.permute(0, 2, 3, 1)
        wb = torch.full((cout + 1, k, k, wcs), NAN)      # (one NaN row behind the last output channel's)
        wb[:cout, :, :, :c4] = 0.0
        wb[:cout, :, :, :cin] = wt.permute(0, 2, 3, 1)
        xg, wg = xb.to(dev), wb.to(dev)
        keep += [xg, wg]
        t = g.seg[i]
        t.src, t.w, t.xcs, t.c4, t.cin, t.ks, t.reflect, t.wcs = xg.data_ptr() + 4 * lo, wg.data_ptr(), xcs, c4, cin, k, int(c['reflect'] and k > 1), wcs
        if s['nrm']:
            act, slope, rows = s['nrm']
            G = tab[0].shape[0]
            off, roww = (4, c4 + 8) if rows == 'wide' else (0, c4)
            ptrs = []
            for v in tab:
                row = torch.full((G, roww), NAN)
                row[:, off:off + c4] = 0.0
                row[:, off:off + cin] = v
                rg = row.to(dev)
                keep.append(rg)
                ptrs.append(rg.data_ptr() + 4 * off)
            u = nm.seg[i]
            u.scale, u.shift, u.sstride, u.act, u.slope = ptrs[0], ptrs[1], 0 if rows == 'batch' else roww, act, slope
    bias = res = None
    if c['bias']:
        keep.append(_nan_tail(inp['bias'], dev))
        bias = keep[-1].data_ptr()
    if c['res']:
        rcs, off = c['res']
        rb = torch.full((n, h, w, rcs), NAN)
        rb[..., off:off + cout] = inp['res'].permute(0, 2, 3, 1)
        keep.append(_nan_tail(rb, dev))
        res, g.rcs = keep[-1].data_ptr() + 4 * off, rcs
    return g, nm, bias, res, keep


def _launch(dev, name):
    """one launch under the profiler -> (y, table or None on the host); families, columns and tails checked"""
    L = _lib()
    from cat_amd import ops
    c, p = CASES[name], plan(CASES[name])
    g, nm, bias, res, keep = _device(dev, name)
    n, h, w, cout, ycs, scs = c['n'], c['h'], c['w'], c['cout'], c['ycs'], c['scs']
    yflat, y = _sentinel((n, h, w, ycs), dev)
    tflat, tab = _sentinel((p['M'] // BM if c['stats'] else 1, 2, scs), dev)
    if c['norm']:
        nm.stats, nm.scs = (tab.data_ptr() if c['stats'] else None), scs
        assert L.query('cat_conv2d_ksum_norm_supported', C.byref(g), C.byref(nm)) == 1 and norm_supported(g, nm)
        call = lambda: L.call('cat_conv2d_ksum_norm_fwd', C.byref(g), C.byref(nm), bias, res, y.data_ptr(), ops._stream())
    else:
        assert L.query('cat_conv2d_ksum_supported', C.byref(g)) == 1 and supported(g)
        call = lambda: L.call('cat_conv2d_ksum_fwd', C.byref(g), bias, res, y.data_ptr(), ops._stream())
    _, fam = _profiled(call)
    assert fam.get(p['family'], 0) == 1 and len([f for f in fam if f.startswith('conv_')]) == 1, fam
    yc, tc = y.cpu(), tab.cpu()
    own = max(c['ycw'], cout)
    _columns(yc, range(own), range(cout), (name, 'y'))      # [Cout, ycw) exactly 0, [ycw, ycs) untouched
    _tail(yflat, (name, 'y'))
    _tail(tflat, (name, 'table'))
    if c['stats']:
        _columns(tc, range(own), range(cout), (name, 'table'))
    else:
        assert bool((tc == SENTINEL).all()), (name, 'no table asked for')
    return yc, (tc if c['stats'] else None)


# ================================================================================================ B: cat_conv2d_ksum_fwd
@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(B_CASES))
def test_ksum_fwd(dev, name):
    cout = CASES[name]['cout']
    yc, _ = _launch(dev, name)
    _cmp('KB', name, {'y': _nchw(yc, 0, cout)}, _ref(name, torch.float64))
    if name == TWICE:
        y2, _ = _launch(dev, name)
        assert torch.equal(yc, y2), 'two launches are bitwise equal'


# ================================================================================================ C: cat_conv2d_ksum_norm_fwd
def _finalize(dev, name, table):
    """cat_tnorm_finalize2 over the kernel's table on its lattice -> scale / shift / mean / rstd [N][Cout]"""
    L = _lib()
    from cat_amd import ops
    c, inp = CASES[name], _inputs(name)
    n, h, w, cout, scs = c['n'], c['h'], c['w'], c['cout'], c['scs']
    th, tw = lattice(h, w)
    sl = (L.NSlice * 1)()
    sl[0].c0, sl[0].c = 0, cout
    rows = [_sentinel((n, scs), dev) for _ in range(4)]
    gg, bg, tg = _nan_tail(inp['gamma'], dev), _nan_tail(inp['beta'], dev), table.to(dev)
    L.call('cat_tnorm_finalize2', ops._p(tg), scs, n, n, h, w, th, tw, 1, ops._p(gg), ops._p(bg), 1, sl, EPS, 0.1, *[r.data_ptr() for _, r in rows], scs,
           ops._stream())
    torch.cuda.synchronize()
    for flat, _ in rows:
        _tail(flat, (name, 'finalize2'))
    return {k: r.cpu()[:, :cout] for k, (_, r) in zip(('scale', 'shift', 'mean', 'rstd'), rows)}


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(C_CASES))
def test_ksum_norm_fwd(dev, name):
    c = CASES[name]
    cout = c['cout']
    want = _ref(name, torch.float64)
    yc, tc = _launch(dev, name)
    got = {'y': _nchw(yc, 0, cout)}
    if c['stats']:
        got['sum'], got['m2'] = tc[:, 0, :cout], tc[:, 1, :cout]
        got.update(_finalize(dev, name, tc))
    _cmp('KC', name, got, want)


# ================================================================================================ D: refusals
def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


# name -> (norm form, refused by the predicate (else by a CAT_REQUIRE of the launch), residual passed, edit of the two structs)
REFUSALS = {
    'nseg-5': (0, 1, 0, lambda g, nm: _set(g, nseg=MAXSEG + 1)),
    'ks-7': (0, 1, 0, lambda g, nm: _set(g.seg[0], ks=7)),
    'c4%4': (0, 1, 0, lambda g, nm: _set(g.seg[0], c4=6)),
    'xcs<c4': (0, 1, 0, lambda g, nm: _set(g.seg[0], xcs=4)),
    'wcs<c4': (0, 1, 0, lambda g, nm: _set(g.seg[0], wcs=4)),
    'two-paddings': (0, 1, 0, lambda g, nm: _set(g.seg[1], ks=3, reflect=0)),
    'reflect-pad>=H': (0, 1, 0, lambda g, nm: _set(g, H=1)),
    'ycs<cout': (0, 0, 0, lambda g, nm: _set(g, ycs=60, ycw=60)),
    'ycw>ycs': (0, 0, 0, lambda g, nm: _set(g, ycw=68)),
    'rcs<cout': (0, 0, 1, lambda g, nm: _set(g, rcs=60)),
    'scale-without-shift': (1, 1, 0, lambda g, nm: _set(nm.seg[0], shift=None)),
    'sstride<c4': (1, 1, 0, lambda g, nm: _set(nm.seg[0], sstride=4)),
    'slope-1.5': (1, 1, 0, lambda g, nm: _set(nm.seg[0], act=ACT_LRELU, slope=1.5)),
    'zero-padded-normalised-k3': (1, 1, 0, lambda g, nm: _set(g.seg[0], reflect=0)),
    'stats-with-activation': (1, 1, 0, lambda g, nm: _set(g, act=ACT_RELU)),
    'stats-with-residual': (1, 0, 1, lambda g, nm: None),
    'plane-off-the-lattice': (1, 1, 0, lambda g, nm: _set(g, H=12, W=12)),
    'table-1028': (1, 1, 0, lambda g, nm: ([_set(s, ks=1, c4=256, xcs=256, wcs=256) for s in g.seg], _set(g.seg[0], c4=260, xcs=260, wcs=260), _set(g, nseg=4),
                                           [_set(t, scale=nm.seg[0].scale, shift=nm.seg[0].shift, sstride=0, act=ACT_RELU) for t in nm.seg])),
}


def test_refusal_table_covers_every_clause():
    assert len(REFUSALS) == 18 and sum(1 for v in REFUSALS.values() if v[0]) == 8 and sum(1 for v in REFUSALS.values() if not v[1]) == 4


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_ksum_refuses_outside_its_domain(dev, name):
    """the base geometry (a reflect 3 x 3 over 8 channels + a 1 x 1 over 4, 64 output channels, one 8 x 16 plane) is accepted; with the edit the
    predicate answers 0 or the launch raises, and nothing is written"""
    L = _lib()
    from cat_amd import ops
    norm, by_predicate, with_res, edit = REFUSALS[name]
    big = torch.zeros(1 << 20, device=dev)      # every address points into 4 MB of zeros: whatever a wrong acceptance read would be mapped
    yflat, y = _sentinel((1, 16, 16, 72), dev)
    tflat, tab = _sentinel((2, 2, 72), dev)

    def structs():
        g, nm = _geoms(L, 1, 8, 16, 64, [(3, 8, 8, 8, 1, 3, 8, ACT_RELU, 0.0), (1, 4, 4, 4, 0, 0, 0, 0, 0.0)], stats=tab.data_ptr(), scs=72)
        for s in g.seg:
            s.src = s.w = big.data_ptr()
        nm.seg[0].scale = nm.seg[0].shift = big.data_ptr()
        return g, nm
    g, nm = structs()
    assert L.query('cat_conv2d_ksum_supported', C.byref(g)) == 1 and L.query('cat_conv2d_ksum_norm_supported', C.byref(g), C.byref(nm)) == 1
    edit(g, nm)
    assert bool(L.query('cat_conv2d_ksum_norm_supported', C.byref(g), C.byref(nm))) == norm_supported(g, nm) == (not by_predicate)
    if not norm:
        assert bool(L.query('cat_conv2d_ksum_supported', C.byref(g))) == supported(g) == (not by_predicate)
    res = big.data_ptr() if with_res else None
    with pytest.raises(RuntimeError, match='conv ksum'):
        if norm:
            L.call('cat_conv2d_ksum_norm_fwd', C.byref(g), C.byref(nm), None, res, y.data_ptr(), ops._stream())
        else:
            L.call('cat_conv2d_ksum_fwd', C.byref(g), None, res, y.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert bool((yflat == SENTINEL).all()) and bool((tflat == SENTINEL).all())
