"""Every compiled instantiation qconv_kernel<NQ, MAXIT> of the quad-granule LDS-tile convolution (csrc/conv_q.hip) and every plan cell on top
of it -- tile height 8 | 16, one or two staging buffers, N blocks over the grid, source stride 2, the four sub-pixel classes -- against the
formula of include/cat_hip.h evaluated directly in float64 on the host, through the C-ABI (qconv.geometry / plan_of / pack_conv / launch).

A (host): NQ_SET, the arms of CAT_Q_NQ and its three MAXIT branches are parsed from the source text; the instantiations must equal the keys of
          VARIANT_CASES, and cat_qconv_plan must send every case (and every feature launch of part C) to exactly the cell it declares, so a new
          instantiation without a case, or a plan rule that moves a case to another kernel, fails without a GPU.
B (GPU):  one launch per case into a sentinel-filled buffer between guard rows; every output element within the fp32 accumulation bound.
C (GPU):  the features on top of the cells: statistics table (raw entries, then cat_tnorm_finalize2), staging affine + activation, generic
          segments, channel-slice output, bias in front of NaNs, planes of pad + 1 rows, the Layer cache.

Bars.  An output with K products is held to (K + 4) * 2^-24 * (S + |res|), S = the same sum with every factor replaced by its absolute value
(|bias| included, |x * scale| + |shift| for a staged input): the bound of fp32 accumulation in any order, here K <= 1200.  One misplaced term is
about S / K, more than ten bars.  tanh / ReLU6 epilogues keep TOL = 1e-4 of the maximum (the device tanhf is not characterised).  A tile sum is
held to the sum of its elements' bars + (cnt + 1) * 2^-24 * sum |z|; M2 and the finalized rows to TOL of the largest entry; sentinel, zero
and NaN lanes are exact."""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QSRC = os.path.join(ROOT, 'cat_amd', 'csrc', 'conv_q.hip')
SENTINEL = 7.0
TOL = 1e-4
U = 2.0 ** -24
NAN = float('nan')

# A case is ('C', cin, cout, k, stride, N, H, W, min_tiles16, reflect, act) -- a "same" convolution, pad (k - 1) / 2 -- or
# ('T', cin, cout, N, H, W, min_tiles16, act) -- ConvTranspose2d(k 3, s 2, p 1, op 1) as four sub-pixel classes -- with the (th, nbuf, nblk) cell
# cat_qconv_plan must report for it.  Every case has a bias, ragged edge tiles and (but for the widths the table fixes) Nn % 4 != 0; padding
# mode and epilogue (0 none, 1 ReLU, 2 LeakyReLU 0.2) alternate down the rows.
VARIANT_CASES = {
    (1, 2): [(('C', 3, 3, 1, 1, 1, 9, 11, 1024, 0, 0), (8, 1, 1))],
    (2, 2): [(('C', 3, 5, 1, 1, 1, 9, 11, 1, 0, 1), (16, 1, 1)), (('T', 4, 8, 1, 5, 7, 1, 2), (16, 1, 1))],
    (3, 2): [(('C', 3, 9, 1, 1, 1, 9, 11, 1, 0, 2), (16, 1, 1))],
    (4, 2): [(('C', 3, 13, 1, 1, 1, 9, 11, 1, 0, 0), (16, 1, 1))],
    (5, 2): [(('C', 3, 17, 7, 1, 1, 20, 24, 1, 1, 1), (16, 1, 1))],
    (6, 2): [(('C', 3, 21, 7, 1, 1, 20, 24, 1, 0, 2), (16, 1, 1))],
    (8, 2): [(('C', 3, 25, 7, 1, 1, 20, 24, 1, 1, 0), (16, 1, 1)),          # the production stem's plan
             (('C', 3, 50, 7, 1, 1, 20, 24, 1024, 0, 1), (8, 1, 1))],
    (10, 2): [(('C', 4, 80, 3, 1, 1, 9, 11, 1024, 1, 2), (8, 1, 1))],
    (12, 2): [(('C', 3, 96, 7, 1, 1, 20, 24, 1024, 0, 0), (8, 1, 1))],
    (1, 4): [(('C', 12, 1, 1, 1, 1, 9, 11, 1, 0, 1), (16, 1, 1))],
    (2, 4): [(('C', 12, 5, 3, 1, 1, 9, 11, 1, 1, 2), (16, 1, 1))],
    (3, 4): [(('C', 12, 9, 3, 1, 1, 9, 11, 1, 0, 0), (16, 1, 1))],
    (4, 4): [(('C', 12, 13, 3, 1, 2, 18, 20, 1, 1, 1), (16, 1, 1))],
    (5, 4): [(('C', 12, 17, 3, 1, 2, 18, 20, 1, 0, 2), (16, 1, 1))],
    (6, 4): [(('C', 12, 21, 3, 1, 2, 18, 20, 1, 1, 0), (16, 1, 1))],
    (8, 4): [(('C', 12, 25, 3, 1, 2, 18, 20, 1, 0, 1), (16, 1, 1)),
             (('C', 4, 50, 3, 2, 1, 17, 19, 1024, 1, 2), (8, 1, 1)),         # S = 2
             (('T', 12, 25, 1, 9, 11, 1, 0), (16, 1, 1))],
    (10, 4): [(('C', 20, 65, 1, 1, 1, 9, 11, 1024, 0, 0), (8, 1, 1))],
    (12, 4): [(('C', 20, 81, 1, 1, 1, 9, 11, 1024, 0, 1), (8, 1, 1))],
    (1, 8): [(('C', 20, 1, 3, 1, 1, 9, 11, 1, 1, 2), (16, 1, 1))],
    (2, 8): [(('C', 20, 5, 3, 1, 1, 9, 11, 1, 0, 0), (16, 1, 1))],
    (3, 8): [(('C', 20, 9, 3, 1, 1, 9, 11, 1, 1, 1), (16, 1, 1))],
    (4, 8): [(('C', 20, 13, 3, 1, 1, 9, 11, 1, 0, 2), (16, 1, 1))],
    (5, 8): [(('C', 20, 17, 3, 1, 1, 9, 11, 1, 1, 0), (16, 1, 1))],
    (6, 8): [(('C', 20, 21, 3, 1, 1, 9, 11, 1, 0, 1), (16, 1, 1))],
    (8, 8): [(('C', 20, 25, 3, 1, 1, 9, 11, 1, 1, 2), (16, 1, 1)),
             (('T', 52, 100, 1, 9, 11, 1024, 1), (8, 2, 2))],
    (10, 8): [(('C', 8, 200, 3, 2, 1, 17, 19, 1024, 0, 0), (8, 1, 3))],      # S = 2, three N blocks
    (12, 8): [(('C', 42, 256, 3, 1, 1, 16, 16, 1024, 1, 1), (8, 1, 3))],
}

# The launches of part C that are a plain case: name -> (case, (nq, maxit, th, nbuf, nblk)).  Each feature below draws on rows with both tile
# heights, one and two staging buffers, one and several N blocks.
FEATURE_CASES = {
    'nq1': (('C', 3, 3, 1, 1, 2, 9, 11, 1024, 0, 0), (1, 2, 8, 1, 1)),
    'stem16': (('C', 3, 25, 7, 1, 2, 20, 24, 1, 1, 0), (8, 2, 16, 1, 1)),
    'wide12': (('C', 3, 96, 7, 1, 1, 20, 24, 1024, 0, 0), (12, 2, 8, 1, 1)),
    's2nblk': (('C', 8, 200, 3, 2, 2, 17, 19, 1024, 0, 0), (10, 8, 8, 1, 3)),
    's2chunks': (('C', 52, 37, 3, 2, 2, 17, 19, 1024, 0, 0), (5, 8, 8, 2, 1)),
    'chunks16': (('C', 52, 25, 3, 1, 2, 9, 11, 1, 0, 0), (8, 8, 16, 2, 1)),
    'chunks8': (('C', 52, 50, 3, 1, 2, 9, 11, 1024, 1, 0), (8, 8, 8, 2, 1)),
    'ct16': (('T', 12, 25, 2, 9, 11, 1, 0), (8, 4, 16, 1, 1)),
    'ctnblk': (('T', 52, 100, 2, 9, 11, 1024, 0), (8, 8, 8, 2, 2)),
    'head8': (('C', 16, 3, 7, 1, 1, 9, 11, 1024, 1, 3), (1, 8, 8, 1, 1)),
    'head16': (('C', 16, 3, 7, 1, 1, 9, 11, 1, 1, 4), (1, 8, 16, 1, 1)),
}
STATS_FEATURES = ('nq1', 'stem16', 'wide12', 's2nblk', 's2chunks', 'ct16', 'ctnblk')
AFFINE_FEATURES = ('chunks16', 'chunks8', 's2chunks', 'ct16', 'ctnblk')
SLICE_FEATURES = ('nq1', 'stem16', 's2nblk', 'chunks16', 'ctnblk')
BIAS_FEATURES = ('nq1', 'stem16', 's2nblk', 's2chunks', 'ct16', 'ctnblk')


def cs4(c):
    return (c + 3) // 4 * 4


def cdiv(a, b):
    return (a + b - 1) // b


def _ids(case):
    return '-'.join(str(v) for v in case)


# ------------------------------------------------------------------------------------------------ launches: host description
class Sg:
    """One K segment on the host: x [N, cin, H, W], w [Nn, cin, kh, kw] (fp32), tap (i, j) of lattice pixel (cy, cx) reads
    (cy * S + oy + i, cx * S + ox + j); optional staging affine rows [1 | N, cin] + activation."""

    def __init__(self, x, w, oy, ox, reflect=0, scale=None, shift=None, per_image=False, act=0, slope=0.0):
        self.x, self.w, self.oy, self.ox, self.reflect = x, w, oy, ox, int(reflect)
        self.scale, self.shift, self.per_image, self.act, self.slope = scale, shift, per_image, act, slope
        self.cin, self.kh, self.kw = w.shape[1], w.shape[2], w.shape[3]


class Launch:
    """What one cat_qconv_fwd call computes: segments, lattice, stride / classes, epilogue."""

    def __init__(self, segs, ho, wo, rule, stride=1, ncls=1, bias=None, act=0, slope=0.2, res=None, ctw=None):
        self.segs, self.ho, self.wo, self.rule, self.stride, self.ncls = segs, ho, wo, rule, stride, ncls
        self.bias, self.act, self.slope, self.res, self.ctw = bias, act, slope, res, ctw
        self.n, _, self.h, self.w = segs[0].x.shape
        self.nn = segs[0].w.shape[0]
        self.os = 2 if ncls == 4 else 1

    def geometry(self, ptrs=None, **kw):
        """cat_qconv_t; ptrs = per segment (src pointer, pixel stride, scale, shift) on the device, None = a host-only plan query"""
        from cat_amd import qconv
        qs = []
        for k, s in enumerate(self.segs):
            c4 = cs4(s.cin)
            ptr, xcs, sc, sh = ptrs[k] if ptrs else (0, c4, None, None)
            qs.append(qconv.Seg(None, s.kh, s.kw, s.oy, s.ox, reflect=s.reflect, scale=sc, shift=sh, sstride=c4 if s.per_image else 0, act=s.act,
                                slope=s.slope, c4=c4, cin=s.cin, xcs=xcs, ptr=ptr))
        return qconv.geometry(qs, self.n, self.h, self.w, self.ho, self.wo, self.nn, kw.pop('ycs', cs4(self.nn)), stride=self.stride,
                              ncls=self.ncls, act=self.act, slope=self.slope, **kw)


# output row 2a + py of ConvTranspose2d(k 3, s 2, p 1) = 2 (a + dy) - 1 + ky: filter row ky = py + 1 - 2 dy for the class's rows dy = 0 .. py
def _ct_class_weight(wt, py, px):
    ky = [py + 1 - 2 * d for d in range(1 + py)]
    kx = [px + 1 - 2 * d for d in range(1 + px)]
    return wt[:, :, ky][:, :, :, kx].permute(1, 0, 2, 3).contiguous()


@functools.lru_cache(maxsize=None)
def _case_launch(case, affine=None):
    """The launch of a table case on fixed inputs.  affine = (per_image, act, slope): a staging affine + activation on the source."""
    kw = {}
    if case[0] == 'C':
        _, cin, cout, k, stride, n, h, w, rule, reflect, act = case
    else:
        _, cin, cout, n, h, w, rule, act = case
    x = detfill.normal((n, cin, h, w), 1)
    if affine is not None:
        per_image, sact, sslope = affine
        rows = n if per_image else 1
        kw = dict(scale=detfill.normal((rows, cin), 5, 0.5) + 1.0, shift=detfill.normal((rows, cin), 6), per_image=per_image, act=sact, slope=sslope)
    b = detfill.normal((cout,), 3, 0.5)
    if case[0] == 'C':
        pad = (k - 1) // 2
        wt = detfill.normal((cout, cin, k, k), 2, 1.0 / np.sqrt(cin * k * k))
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        return Launch([Sg(x, wt, -pad, -pad, reflect, **kw)], ho, wo, rule, stride=stride, bias=b, act=act)
    wt = detfill.normal((cin, cout, 3, 3), 2, 1.0 / np.sqrt(cin * 9))
    segs = [Sg(x, _ct_class_weight(wt, c >> 1, c & 1), 0, 0, **kw) for c in range(4)]
    return Launch(segs, h, w, rule, ncls=4, bias=b, act=act, ctw=wt)


@contextlib.contextmanager
def _tile_rule(v):
    from cat_amd import _lib as L
    L.load()
    old = L.query('cat_qconv_min_tiles16', int(v))
    try:
        yield
    finally:
        L.query('cat_qconv_min_tiles16', old)


def _cell(plan):
    return (plan.nq, plan.maxit, plan.th, plan.nbuf, plan.nblk)


def _host_cell(launch):
    from cat_amd import qconv
    with _tile_rule(launch.rule):
        return _cell(qconv.plan_of(launch.geometry()))


# ------------------------------------------------------------------------------------------------ A: the table covers the dispatch
def _compiled_instantiations(text):
    nq_set = [int(v) for v in re.search(r'NQ_SET\[\]\s*=\s*\{([^}]*)\}', text).group(1).split(',')]
    lines = text.splitlines()
    start = [i for i, l in enumerate(lines) if l.startswith('#define CAT_Q_NQ(MAXIT)')]
    assert len(start) == 1
    body = []
    for l in lines[start[0]:]:
        body.append(l)
        if not l.rstrip().endswith('\\'):
            break
    arms = re.findall(r'(?:case\s+(\d+)|default)\s*:\s*CAT_Q_LAUNCH\((\d+),\s*MAXIT\)', '\n'.join(body))
    assert all(label in ('', nq) for label, nq in arms), arms      # `case N` launches NQ = N
    launched = sorted(int(nq) for _, nq in arms)
    assert launched == sorted(nq_set) and len(set(launched)) == len(launched), (launched, nq_set)
    rest = '\n'.join(lines[start[0] + len(body):])
    maxits = [int(v) for v in re.findall(r'\{\s*CAT_Q_NQ\((\d+)\)\s*\}', rest)]
    assert sorted(maxits) == [2, 4, 8], maxits
    for m in (2, 4):
        assert re.search(r'P\.maxit == %d\)\s*\{\s*CAT_Q_NQ\(%d\)' % (m, m), rest), m
    return {(nq, m) for nq in nq_set for m in maxits}


def test_variant_table_covers_the_instantiations():
    inst = _compiled_instantiations(open(QSRC).read())
    assert inst == set(VARIANT_CASES), (sorted(inst - set(VARIANT_CASES)), sorted(set(VARIANT_CASES) - inst))
    cells = set()
    for key, rows in VARIANT_CASES.items():
        assert rows, key
        for case, cell in rows:
            got = _host_cell(_case_launch(case))
            assert got == key + cell, (case, got, key + cell)
            cells.add((case[0], case[4] if case[0] == 'C' else 1) + got[2:])
    assert {c[2] for c in cells} == {8, 16} and {c[3] for c in cells} == {1, 2} and {c[4] for c in cells} == {1, 2, 3}
    assert ('C', 2, 8, 1, 3) in cells and ('T', 1, 16, 1, 1) in cells and ('T', 1, 8, 2, 2) in cells


def _meets_every_cell(names):
    cells = [FEATURE_CASES[n][1] for n in names]
    return {c[2] for c in cells} == {8, 16} and {c[3] for c in cells} == {1, 2} and 1 in {c[4] for c in cells} and max(c[4] for c in cells) > 1


def test_feature_launches_sit_on_their_cells():
    for name, (case, cell) in FEATURE_CASES.items():
        assert _host_cell(_case_launch(case)) == cell, name
    for names in (STATS_FEATURES, AFFINE_FEATURES, SLICE_FEATURES, BIAS_FEATURES):
        assert _meets_every_cell(names), names
    assert {FEATURE_CASES[n][1][0] for n in STATS_FEATURES} >= {1, 8, 12}
    for rule, cell in GENERIC_CELLS.items():
        assert _host_cell(_generic_launch(rule)) == cell, rule
    assert _host_cell(_generic_s2_launch()) == GENERIC_S2_CELL
    for k, plane, stride, reflect, rule in SMALL_PLANES:
        assert _host_cell(_small_plane_launch(k, plane, stride, reflect, rule))[2] == (16 if rule == 1 and stride == 1 else 8)


# ------------------------------------------------------------------------------------------------ the float64 reference
def _index(pos, size, reflect):
    if reflect:
        ok = (pos > -size) & (pos < 2 * size - 1)
        r = pos.abs()
        r = torch.where(r >= size, 2 * size - 2 - r, r)
    else:
        ok = (pos >= 0) & (pos < size)
        r = pos
    return r.clamp(0, size - 1), ok


def _staged(sg):
    """f_s(x) and the bound |x * scale| + |shift| >= |f_s(x)| of its magnitude"""
    x = sg.x.double()
    if sg.scale is None:
        a, mag = x, x.abs()
    else:
        rows = x.shape[0] if sg.per_image else 1
        sc, sh = sg.scale.double().view(rows, -1, 1, 1), sg.shift.double().view(rows, -1, 1, 1)
        a, mag = x * sc + sh, (x * sc).abs() + sh.abs()
    if sg.act == 1:
        a = a.clamp_min(0.0)
    elif sg.act == 2:
        a = torch.where(a > 0, a, a * sg.slope)
    return a, mag


def _seg_sum(sg, stride, ho, wo):
    """sum over the segment's taps and channels on the ho x wo lattice, and the same sum of absolute values"""
    a, mag = _staged(sg)
    n, cin, h, w = a.shape
    wd = sg.w.double()
    z = torch.zeros(n, wd.shape[0], ho, wo, dtype=torch.float64)
    s = torch.zeros_like(z)
    for i in range(sg.kh):
        iy, oky = _index(torch.arange(ho) * stride + sg.oy + i, h, sg.reflect)
        for j in range(sg.kw):
            ix, okx = _index(torch.arange(wo) * stride + sg.ox + j, w, sg.reflect)
            assert not sg.reflect or (bool(oky.all()) and bool(okx.all())), 'a reflect halo wider than the plane'
            m = (oky[:, None] & okx[None, :]).double()
            z += torch.einsum('nchw,oc->nohw', a[:, :, iy][:, :, :, ix] * m, wd[:, :, i, j])
            s += torch.einsum('nchw,oc->nohw', mag[:, :, iy][:, :, :, ix] * m, wd[:, :, i, j].abs())
    return z, s


@functools.lru_cache(maxsize=None)
def _reference(launch):
    """pre-activation z, output y, element bar -- all [N, Nn, Ho * OS, Wo * OS] float64"""
    L_ = launch
    if L_.ncls == 1:
        parts = [_seg_sum(s, L_.stride, L_.ho, L_.wo) for s in L_.segs]
        z, s = sum(p[0] for p in parts), sum(p[1] for p in parts)
        k = torch.full_like(z, float(sum(sg.kh * sg.kw * sg.cin for sg in L_.segs)))
    else:
        z = torch.zeros(L_.n, L_.nn, 2 * L_.ho, 2 * L_.wo, dtype=torch.float64)
        s, k = torch.zeros_like(z), torch.zeros_like(z)
        for c, sg in enumerate(L_.segs):
            py, px = c >> 1, c & 1
            z[:, :, py::2, px::2], s[:, :, py::2, px::2] = _seg_sum(sg, 1, L_.ho, L_.wo)
            k[:, :, py::2, px::2] = sg.kh * sg.kw * sg.cin
    assert float(k.max()) <= 1200
    if L_.bias is not None:
        z = z + L_.bias.double().view(1, -1, 1, 1)
        s = s + L_.bias.double().abs().view(1, -1, 1, 1)
    y = {0: z, 1: z.clamp_min(0.0), 2: torch.where(z > 0, z, z * L_.slope), 3: torch.tanh(z), 4: z.clamp(0.0, 6.0)}[L_.act]
    if L_.res is not None:
        y = y + L_.res.double()
        s = s + L_.res.double().abs()
    return z, y, (k + 4) * U * s


def test_reference_agrees_with_aten_float64():
    """the hand-written float64 formula against ATen's float64 convolutions (reflect and zero padding, stride 2, the transposed conv)"""
    for case in (('C', 3, 25, 7, 1, 1, 20, 24, 1, 1, 0), ('C', 4, 50, 3, 2, 1, 17, 19, 1024, 0, 0), ('T', 12, 25, 1, 9, 11, 1, 0)):
        la = _case_launch(case)
        z, _, _ = _reference(la)
        x, b = la.segs[0].x.double(), la.bias.double()
        if case[0] == 'T':
            want = F.conv_transpose2d(x, la.ctw.double(), b, stride=2, padding=1, output_padding=1)
        else:
            pad = (case[3] - 1) // 2
            xp = F.pad(x, (pad,) * 4, mode='reflect') if case[9] else x
            want = F.conv2d(xp, la.segs[0].w.double(), b, stride=case[4], padding=0 if case[9] else pad)
        assert tuple(z.shape) == tuple(want.shape) and float((z - want).abs().max()) < 1e-12, case


# ------------------------------------------------------------------------------------------------ launches: device side
@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


class Ran:
    pass


def _run(launch, dev, c0=0, extra=0, lead=0, stats=False, bias_behind_nan=False, rcs_extra=0):
    """One plan + pack + launch.  y is a channel slice [c0, c0 + ycw) of a sentinel-filled [N, Ho, Wo, c0 + ycw + extra] buffer between two
    guard rows on either side; a source is a slice at channel `lead` of a NaN-filled wider tensor; a residual carries NaNs in its padding lanes."""
    from cat_amd import ops, qconv
    la, r = launch, Ran()
    hout, wout, ycw = la.ho * la.os, la.wo * la.os, cs4(la.nn)
    ycs = c0 + ycw + extra
    guard, body = 2 * wout * ycs, la.n * hout * wout * ycs
    flat = torch.full((guard + body + guard,), SENTINEL, device=dev)
    keep, ptrs = [], []
    for sg in la.segs:
        c4 = cs4(sg.cin)
        xcs = lead + c4 + (4 if lead else 0)
        xh = torch.full((la.n, la.h, la.w, xcs), NAN)
        xh[..., lead:lead + c4] = 0.0
        xh[..., lead:lead + sg.cin] = sg.x.permute(0, 2, 3, 1)
        xd = xh.to(dev)
        sc = sh = None
        if sg.scale is not None:
            rows = sg.scale.shape[0]
            sc, sh = torch.zeros(rows, c4, device=dev), torch.zeros(rows, c4, device=dev)
            sc[:, :sg.cin], sh[:, :sg.cin] = sg.scale.to(dev), sg.shift.to(dev)
        keep += [xd, sc, sh]
        ptrs.append((xd.data_ptr() + 4 * lead, xcs, sc, sh))
    kw = {}
    if stats:
        r.scs = ycw
        r.entries = la.n * la.ncls * cdiv(la.ho, 8) * cdiv(la.wo, 16) + 3      # th >= 8: never fewer than the plan's count
        r.table = torch.full((r.entries * 2 * r.scs,), NAN, device=dev)
        kw = dict(stats=r.table, scs=r.scs)
    g = la.geometry(ptrs, ycs=ycs, ycw=ycw, **kw)
    if la.res is not None:
        rcs = ycw + rcs_extra
        rh = torch.full((la.n, la.ho, la.wo, rcs), NAN)
        rh[..., :la.nn] = la.res.permute(0, 2, 3, 1)
        resd = rh.to(dev)
        g.res, g.rcs = resd.data_ptr(), rcs
    bias = None
    if la.bias is not None:
        bias = torch.full((la.nn + 8,), NAN, device=dev) if bias_behind_nan else torch.empty(la.nn, device=dev)
        bias[:la.nn] = la.bias.to(dev)
    with _tile_rule(la.rule):
        plan = qconv.plan_of(g)
        pack = torch.zeros(int(plan.pack_floats), device=dev)
        if la.ncls == 4:
            wd = ops.padded_weight_like(la.ctw.shape, dev)
            wd.copy_(la.ctw)
            wcl, wcs = ops.weight_cl(wd)
            qconv.pack_conv_transpose(g, pack, wcl, wcs, la.nn)
        else:
            for k, sg in enumerate(la.segs):
                wd = ops.padded_weight_like(sg.w.shape, dev)
                wd.copy_(sg.w)
                wcl, wcs = ops.weight_cl(wd)
                assert wcl.data_ptr() == wd.data_ptr()
                qconv.pack_conv(g, k, pack, wcl, wcs, la.nn, sg.kh * sg.kw)
        qconv.launch(g, pack, bias, flat.data_ptr() + 4 * (guard + c0))
        torch.cuda.synchronize()
    r.cell, r.tiles, r.th = _cell(plan), plan.tiles, plan.th
    r.flat, r.guard, r.c0, r.ycw, r.ycs = flat.cpu(), guard, c0, ycw, ycs
    r.buf = r.flat[guard:guard + body].view(la.n, hout, wout, ycs)
    return r


WORST = {}


def _note(family, ratio, what):
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print('QCONV-RATIO %s %.4f worst %.4f %s' % (family, ratio, WORST[family], what))


def _check_output(launch, r, family, what, y=None, bar=None):
    """[c0, c0 + Nn) the result within its bar (TOL of the maximum behind a tanh / ReLU6 epilogue), [Nn, ycw) zeros, every other float of the
    buffer and of the guard rows the sentinel"""
    if y is None:
        _, y, bar = _reference(launch)
    nn, c0 = launch.nn, r.c0
    got = r.buf[..., c0:c0 + nn].permute(0, 3, 1, 2).double()
    assert tuple(got.shape) == tuple(y.shape) and bool(torch.isfinite(got).all()), what
    err = (got - y).abs()
    if launch.act in (3, 4):
        ratio = float(err.max() / (TOL * y.abs().max()))
    else:
        ratio = float(torch.where(err > 0, err / bar, torch.zeros_like(err)).max())
    _note(family, ratio, what)
    assert ratio <= 1.0, (what, ratio)
    assert bool((r.buf[..., c0 + nn:c0 + r.ycw] == 0.0).all()), what
    assert bool((r.buf[..., :c0] == SENTINEL).all()) and bool((r.buf[..., c0 + r.ycw:] == SENTINEL).all()), what
    assert bool((r.flat[:r.guard] == SENTINEL).all()) and bool((r.flat[-r.guard:] == SENTINEL).all()), what


# ------------------------------------------------------------------------------------------------ B: parity per instantiation
@pytest.mark.gpu
@pytest.mark.parametrize('key,case,cell', [(k, c, cell) for k, rows in VARIANT_CASES.items() for c, cell in rows],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_variant_parity(dev, key, case, cell):
    la = _case_launch(case)
    r = _run(la, dev)
    assert r.cell == key + cell, (case, r.cell)
    _check_output(la, r, 'variant', (key, case))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['head8', 'head16'])
def test_slow_epilogues(dev, name):
    """tanh (the image head) and ReLU6 through the out-of-line epilogue of the NQ = 1 kernel, both tile heights"""
    case, cell = FEATURE_CASES[name]
    la = _case_launch(case)
    r = _run(la, dev)
    assert r.cell == cell
    _check_output(la, r, 'tanh_relu6', name)


# ------------------------------------------------------------------------------------------------ C: features on top of the cells
def _tile_stats(launch, r, z, bar):
    """float64 (sum, M2) and the sum's bar for every entry (image * tiles + tile) * ncls + class of the plan's table"""
    la = launch
    tx, ty = cdiv(la.wo, 16), cdiv(la.ho, r.th)
    assert tx * ty * la.ncls == r.tiles
    sums, m2s, bars = [], [], []
    for img in range(la.n):
        for t in range(tx * ty):
            r0, c0 = (t // tx) * r.th, (t % tx) * 16
            r1, c1 = min(r0 + r.th, la.ho), min(c0 + 16, la.wo)
            for cls in range(la.ncls):
                py, px = cls >> 1, cls & 1
                sl = (img, slice(None), slice(r0 * la.os + py, r1 * la.os, la.os), slice(c0 * la.os + px, c1 * la.os, la.os))
                zt, cnt = z[sl], (r1 - r0) * (c1 - c0)
                assert zt.shape[1] * zt.shape[2] == cnt
                s = zt.sum((1, 2))
                sums.append(s)
                m2s.append(((zt - (s / cnt).view(-1, 1, 1)) ** 2).sum((1, 2)))
                bars.append(bar[sl].sum((1, 2)) + (cnt + 1) * U * zt.abs().sum((1, 2)))
    return torch.stack(sums), torch.stack(m2s), torch.stack(bars)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _check_stats(launch, r, dev, what):
    from cat_amd import _lib as L, ops
    la = launch
    z, _, bar = _reference(la)
    nn, scs, used = la.nn, r.scs, la.n * r.tiles
    tab = r.table.cpu().view(r.entries, 2, scs)
    assert used <= r.entries - 3
    assert bool(torch.isnan(tab[used:]).all()), what                       # entries beyond the plan's count: untouched
    assert bool(torch.isfinite(tab[:used]).all()), what
    assert bool((tab[:used, :, nn:] == 0.0).all()), what                    # channels [Nn, ycw)
    sums, m2s, sbar = _tile_stats(la, r, z, bar)
    err = (tab[:used, 0, :nn].double() - sums).abs()
    ratio = float((err / sbar).max())
    _note('stats_sum', ratio, what)
    assert ratio <= 1.0, (what, ratio)
    m2 = _rel(tab[:used, 1, :nn], m2s)
    _note('stats_m2', m2 / TOL, what)
    assert m2 < TOL, (what, m2)
    # the table through cat_tnorm_finalize2: nn.BatchNorm2d (with running statistics) and nn.InstanceNorm2d in training mode
    gamma, beta = detfill.normal((nn,), 14, 0.3) + 1.0, detfill.normal((nn,), 15)
    gd, bd = torch.zeros(scs, device=dev), torch.zeros(scs, device=dev)
    gd[:nn], bd[:nn] = gamma.to(dev), beta.to(dev)
    for groups in (1, la.n):
        rm, rv = torch.zeros(nn, device=dev), torch.ones(nn, device=dev)
        sl = (L.NSlice * 1)()
        sl[0].c0, sl[0].c = 0, nn
        if groups == 1:
            sl[0].running_mean, sl[0].running_var = rm.data_ptr(), rv.data_ptr()
        scale, shift, mean, rstd = (torch.empty(groups, scs, device=dev) for _ in range(4))
        L.call('cat_tnorm_finalize2', ops._p(r.table), scs, groups, la.n, la.ho, la.wo, r.th, 16, la.ncls, ops._p(gd), ops._p(bd), 1, sl, 1e-5, 0.1,
               ops._p(scale), ops._p(shift), ops._p(mean), ops._p(rstd), scs, ops._stream())
        torch.cuda.synchronize()
        dims = (0, 2, 3) if groups == 1 else (2, 3)
        m, v = z.mean(dims).reshape(groups, nn), z.var(dims, unbiased=False).reshape(groups, nn)
        sc_ref = gamma.double().view(1, -1) * (v + 1e-5).rsqrt()
        d = max(_rel(mean[:, :nn], m), _rel(rstd[:, :nn], (v + 1e-5).rsqrt()), _rel(scale[:, :nn], sc_ref),
                _rel(shift[:, :nn], beta.double().view(1, -1) - m * sc_ref))
        if groups == 1:
            cnt = z.numel() / nn
            d = max(d, _rel(rm, 0.1 * m[0]), _rel(rv, 0.9 + 0.1 * v[0] * cnt / (cnt - 1)))
        _note('stats_finalize', d / TOL, (what, groups))
        assert d < TOL, (what, groups, d)


@pytest.mark.gpu
@pytest.mark.parametrize('name', STATS_FEATURES)
def test_statistics_table(dev, name):
    """raw per-tile (sum, M2) of the pre-activation output at NQ 1 / 8 / 12, several N blocks, S = 2 and the four classes; then finalize2"""
    case, cell = FEATURE_CASES[name]
    la = _case_launch(case)
    assert la.act == 0
    r = _run(la, dev, stats=True)
    assert r.cell == cell
    _check_output(la, r, 'stats_y', name)
    _check_stats(la, r, dev, name)


@pytest.mark.gpu
@pytest.mark.parametrize('per_image,sact,sslope', [(False, 1, 0.0), (True, 2, 0.3), (False, 2, 0.3), (True, 1, 0.0)],
                         ids=['channel-relu', 'image-lrelu', 'channel-lrelu', 'image-relu'])
@pytest.mark.parametrize('name', AFFINE_FEATURES)
def test_staging_affine(dev, name, per_image, sact, sslope):
    """scale * x + shift and ReLU / LeakyReLU applied while the source is staged, on layers of several chunks and on the transposed conv; every
    shift is far from 0, so a zero-padded pixel that took the affine would show"""
    case, cell = FEATURE_CASES[name]
    la = _case_launch(case, (per_image, sact, sslope))
    r = _run(la, dev)
    assert r.cell == cell
    _check_output(la, r, 'staging_affine', (name, per_image, sact))


GENERIC_CELLS = {1: (8, 8, 16, 2, 1), 1024: (4, 8, 8, 2, 1)}
GENERIC_S2_CELL = (4, 8, 8, 2, 1)


@functools.lru_cache(maxsize=None)
def _generic_launch(rule):
    """Eight segments in one launch: 1 x 7 and 7 x 1 taps, a 3 x 3 off its centre, a reflect and a zero segment of different halos, one of 52
    channels (more than a staged chunk, between one-chunk neighbours), a 2 x 2 at offset 0, a staged affine; bias, ReLU and a residual."""
    n, h, w, nn = 2, 9, 11, 30
    spec = [(5, 1, 7, 0, -3, 0), (6, 7, 1, -3, 0, 1), (7, 3, 3, -2, 1, 0), (9, 3, 3, -1, -1, 1), (52, 1, 1, 0, 0, 0), (3, 5, 5, -2, -2, 0),
            (4, 2, 2, 0, 0, 0), (9, 1, 1, 0, 0, 0)]
    segs = []
    for k, (cin, kh, kw, oy, ox, reflect) in enumerate(spec):
        x = detfill.normal((n, cin, h, w), 40 + k)
        wt = detfill.normal((nn, cin, kh, kw), 60 + k, 1.0 / np.sqrt(cin * kh * kw))
        kw_ = dict(scale=detfill.normal((n, cin), 80, 0.5) + 1.0, shift=detfill.normal((n, cin), 81), per_image=True, act=2, slope=0.3) if k == 7 else {}
        segs.append(Sg(x, wt, oy, ox, reflect, **kw_))
    return Launch(segs, h, w, rule, bias=detfill.normal((nn,), 90, 0.5), act=1, res=detfill.normal((n, nn, h, w), 91))


@functools.lru_cache(maxsize=None)
def _generic_s2_launch():
    """source stride 2 with two segments of different halos (3 x 3 at -1 reflected, 1 x 1 at 0) over 52 and 5 channels"""
    n, h, w, nn = 1, 17, 19, 30
    segs = [Sg(detfill.normal((n, 52, h, w), 50), detfill.normal((nn, 52, 3, 3), 51, 1.0 / np.sqrt(52 * 9)), -1, -1, 1),
            Sg(detfill.normal((n, 5, h, w), 52), detfill.normal((nn, 5, 1, 1), 53, 1.0 / np.sqrt(5)), 0, 0, 0)]
    return Launch(segs, 9, 10, 1024, stride=2, bias=detfill.normal((nn,), 54, 0.5), act=2, res=detfill.normal((n, nn, 9, 10), 55))


@pytest.mark.gpu
@pytest.mark.parametrize('rule', [1, 1024], ids=['tiles16x16', 'tiles8x16'])
def test_generic_segments(dev, rule):
    """sources are channel slices of NaN-filled wider tensors; the residual's pixel stride exceeds the output's"""
    la = _generic_launch(rule)
    r = _run(la, dev, lead=4, rcs_extra=8)
    assert r.cell == GENERIC_CELLS[rule]
    _check_output(la, r, 'generic_segments', rule)


@pytest.mark.gpu
def test_generic_segments_stride2(dev):
    la = _generic_s2_launch()
    r = _run(la, dev, lead=4, rcs_extra=4)
    assert r.cell == GENERIC_S2_CELL
    _check_output(la, r, 'generic_segments', 'S2')


@pytest.mark.gpu
@pytest.mark.parametrize('name', SLICE_FEATURES)
def test_output_channel_slice(dev, name):
    """y = channels [8, 8 + ycw) of a wider buffer (ycw < ycs): [Nn, ycw) zeros, the neighbours on both sides and the guard rows untouched"""
    case, cell = FEATURE_CASES[name]
    la = _case_launch(case)
    r = _run(la, dev, c0=8, extra=12)
    assert r.cell == cell
    _check_output(la, r, 'channel_slice', name)


@pytest.mark.gpu
@pytest.mark.parametrize('name', BIAS_FEATURES)
def test_bias_in_front_of_nans(dev, name):
    """the last partial quad's bias load reads past Nn by design: what it reads must reach neither y nor the statistics table"""
    case, cell = FEATURE_CASES[name]
    la = _case_launch(case)
    r = _run(la, dev, stats=True, bias_behind_nan=True)
    assert r.cell == cell
    _check_output(la, r, 'bias_nan', name)
    tab = r.table.cpu().view(r.entries, 2, r.scs)
    assert bool(torch.isfinite(tab[:la.n * r.tiles]).all()) and bool(torch.isnan(tab[la.n * r.tiles:]).all())


# k, (H, W), stride, reflect, min_tiles16: reflect halos on planes of pad + 1 rows and columns; zero padding on planes below one tile, both S
SMALL_PLANES = [(3, (2, 2), 1, 1, 1), (5, (3, 3), 1, 1, 1024), (7, (4, 4), 1, 1, 1), (7, (4, 5), 1, 1, 1024), (3, (3, 5), 1, 0, 1), (3, (5, 3), 2, 0, 1),
                (3, (2, 2), 2, 0, 1024)]


@functools.lru_cache(maxsize=None)
def _small_plane_launch(k, plane, stride, reflect, rule):
    n, cin, cout, pad = 2, 5, 6, (k - 1) // 2
    h, w = plane
    x = detfill.normal((n, cin, h, w), 70)
    wt = detfill.normal((cout, cin, k, k), 71, 1.0 / np.sqrt(cin * k * k))
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    return Launch([Sg(x, wt, -pad, -pad, reflect)], ho, wo, rule, stride=stride, bias=detfill.normal((cout,), 72, 0.5))


@pytest.mark.gpu
@pytest.mark.parametrize('k,plane,stride,reflect,rule', SMALL_PLANES, ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_small_planes(dev, k, plane, stride, reflect, rule):
    la = _small_plane_launch(k, plane, stride, reflect, rule)
    r = _run(la, dev, stats=True)
    _check_output(la, r, 'small_planes', (k, plane, stride, reflect, rule))
    _check_stats(la, r, dev, ('small', k, plane, stride))


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['conv', 'convt'])
def test_layer_cache_follows_weight_and_tile_rule(dev, kind):
    """qconv.Layer re-packs when the weight's version moves and re-plans when cat_qconv_min_tiles16 moves: a changed weight under a flipped
    rule must give the current weight's result, never a stale stream or a stream of the other tiling"""
    from cat_amd import ops, qconv
    case = FEATURE_CASES['stem16' if kind == 'conv' else 'ct16'][0]
    la = _case_launch(case)
    sg = la.segs[0]
    w0 = sg.w if kind == 'conv' else la.ctw
    w1 = detfill.normal(tuple(w0.shape), 99, float(w0.std()))
    wd = ops.padded_weight_like(w0.shape, dev)
    wd.copy_(w0)
    layer = qconv.Layer(kind, wd, stride=1 if kind == 'conv' else 2, pad=-sg.oy if kind == 'conv' else 1, reflect=bool(sg.reflect))
    xd = ops.to_nhwc(sg.x.to(dev))
    bias = la.bias.to(dev)
    cells = []
    for wt, rule in ((w0, 1), (w1, 1024), (w0, 1024), (w1, 1)):
        version = wd._version
        wd.copy_(wt)
        assert wd._version > version
        if kind == 'conv':
            want = Launch([Sg(sg.x, wt, sg.oy, sg.ox, sg.reflect)], la.ho, la.wo, rule, bias=la.bias)
        else:
            want = Launch([Sg(sg.x, _ct_class_weight(wt, c >> 1, c & 1), 0, 0) for c in range(4)], la.ho, la.wo, rule, ncls=4, bias=la.bias, ctw=wt)
        _, y, bar = _reference(want)
        out = ops.empty_act(la.n, la.nn, la.ho * la.os, la.wo * la.os, dev)
        with _tile_rule(rule):
            plan = layer.run(xd, bias, out)
            torch.cuda.synchronize()
        cells.append(plan.th)
        err = (out.cpu().double() - y).abs()
        ratio = float((err / bar).max())
        _note('layer_cache', ratio, (kind, rule))
        assert ratio <= 1.0, (kind, rule, ratio)
    assert cells == [16, 8, 8, 16]


@pytest.mark.gpu
@pytest.mark.parametrize('column', ['adam_step', 'storage_move', 'data_swap'])
def test_layer_streams_follow_optimizer_steps_and_storage_moves(dev, column):
    """qconv.Layer's packed stream under the ways a TRAINED weight changes (test_layer_cache_follows_weight_and_tile_rule covers copy_): an
    eager FusedAdam.step after a real backward (raw pointers, no version bump: the optimizer epoch is the key), the storage move of
    FusedAdam's first zero_grad AFTER the layer has run (then a step), and `weight.data = new_tensor`.  The smallest stem16 case.  After the
    change the same Layer must give (a) bit for bit what a Layer that never ran gives on a copy of the new weight, (b) the fp64 result for
    the new weight within this file's element bar, (c) which the fp64 result for the old weight misses by > 100 bars (upper quartile over the elements); (d) one more
    run re-packs nothing."""
    from cat_amd import _lib as L
    from cat_amd import ops, qconv
    from cat_amd.optim import FusedAdam
    case = FEATURE_CASES['stem16'][0]
    la = _case_launch(case)
    sg = la.segs[0]
    pad, mode = -sg.oy, (L.PAD_REFLECT if sg.reflect else L.PAD_ZERO)
    w0 = ops.padded_weight_like(sg.w.shape, dev)
    w0.copy_(sg.w)
    weight, bias = torch.nn.Parameter(w0), torch.nn.Parameter(la.bias.to(dev))
    layer = qconv.Layer('conv', weight, stride=la.stride, pad=pad, reflect=bool(sg.reflect))
    xd = ops.to_nhwc(sg.x.to(dev))
    gy = ops.to_nhwc(detfill.normal((la.n, la.nn, la.ho, la.wo), 98).to(dev))
    packs = []
    real_call = L.call

    def counting(name, *args):
        if name == 'cat_qconv_pack':
            packs.append(name)
        return real_call(name, *args)

    def run(lay, b):
        out = ops.empty_act(la.n, la.nn, la.ho, la.wo, dev)
        with _tile_rule(la.rule):
            lay.run(xd, b.detach(), out, act=la.act, slope=la.slope)
            torch.cuda.synchronize()
        return out.cpu().double()

    def step(opt):
        """one training step of the layer the way nn._conv_norm_q drives it: forward on the quad-granule kernel, the general backward"""
        opt.zero_grad()
        with _tile_rule(la.rule):
            y = ops.Conv2dFn.apply(xd, weight, bias, la.stride, pad, mode, L.ACT_NONE, 0.0, {'layer': layer, 'stats': False})
            y.backward(gy)
        opt.step()

    def want(wt, b):
        return _reference(Launch([Sg(sg.x, wt, sg.oy, sg.ox, sg.reflect)], la.ho, la.wo, la.rule, stride=la.stride, bias=b, act=la.act, slope=la.slope))

    make = lambda: FusedAdam([weight, bias], lr=0.5, betas=(0.5, 0.999))
    if column == 'adam_step':
        opt = make()
        opt.zero_grad()
        y0 = run(layer, bias)
        step(opt)
    elif column == 'storage_move':
        y0 = run(layer, bias)                       # the first use is BEFORE the optimizer re-houses the weight
        ptr = weight.data_ptr()
        opt = make()
        opt.zero_grad()
        assert weight.data_ptr() != ptr and weight._cat_grad_view is not None
        step(opt)
    else:
        y0 = run(layer, bias)
        new = ops.padded_weight_like(sg.w.shape, dev)
        new.copy_(detfill.normal(tuple(sg.w.shape), 99, float(sg.w.std())))
        version = weight._version
        weight.data = new
        assert weight._version == version
    torch.cuda.synchronize()
    w1, b1 = weight.detach().cpu().clone().contiguous(), bias.detach().cpu().clone()
    _, r0, bar0 = want(sg.w, la.bias)
    assert float(((y0 - r0).abs() / bar0).max()) <= 1.0
    L.call = counting
    try:
        warm = run(layer, bias)
        assert len(packs) == 1                                                   # re-packed once
        _, r1, bar = want(w1, b1)
        ratio = float(((warm - r1).abs() / bar).max())
        sep = float(torch.quantile(((r0 - r1).abs() / bar).reshape(-1), 0.75))
        _note('layer_cache', ratio, (column,))
        print('qconv.Layer %s: warm vs fp64(W1) %.3g of the bar; (c) upper-quartile separation %.3g bars' % (column, ratio, sep))
        assert ratio <= 1.0, (column, ratio)                                      # (b)
        assert sep > 100.0, (column, sep)                                         # (c)
        from cat_amd import derived
        stream = derived.peek(layer, qconv.PK).value
        assert torch.equal(run(layer, bias), warm) and derived.peek(layer, qconv.PK).value is stream and len(packs) == 1      # (d)
    finally:
        L.call = real_call
    wc = ops.padded_weight_like(sg.w.shape, dev)
    wc.copy_(w1)
    cold = qconv.Layer('conv', wc, stride=la.stride, pad=pad, reflect=bool(sg.reflect))
    assert torch.equal(run(cold, b1.to(dev)), warm)                               # (a)
