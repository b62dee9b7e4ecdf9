"""Host side of the K-concatenated wide-tile convolution sum (csrc/conv_ksum.hip, cat_conv2d_ksum_* in include/cat_hip.h):

    y = act(bias + sum_s conv_{k_s x k_s, stride 1, "same"}(src_s, w_s)) + res

as ONE implicit GEMM on 128 x 128 tiles -- the tail of the frozen (eval-mode, BatchNorm-folded) teacher's InvertedResidualChannels block
(reference models/modules/inception_modules.py:230-236; cat_amd/frozen.py)."""
import ctypes as C
import os

import torch

from . import _lib as L
from . import ops

_ENABLED = os.environ.get('CAT_KSUM', '1') != '0'      # A/B switch: 0 keeps the LDS-tile launch (cat_tconv_fwd)
_MIN_WG = int(os.environ.get('CAT_KSUM_MIN_WG', '256'))


def set_min_workgroups(n):
    """Fewest 128 x 128 output tiles for which the wide-tile sum is chosen (tests lower it to drive small planes through the kernel)."""
    global _MIN_WG
    old, _MIN_WG = _MIN_WG, int(n)
    return old


class Segment:
    """src: NHWC activation [n, c, h, w] (or a channel slice of one); w: conv weight [Cout, c, k, k] in kernel layout."""
    __slots__ = ('src', 'w', 'ks', 'reflect')

    def __init__(self, src, w, reflect):
        self.src, self.w, self.ks, self.reflect = src, w, int(w.shape[2]), int(bool(reflect))


class NormSegment(Segment):
    """A segment read through f(v) = act(v * scale[n][c] + shift[n][c]) (cat_conv2d_ksum_norm_fwd): scale / shift are tensors or raw
    addresses of rows of cs_for(channels) floats, `sstride` floats apart per image (0: one row for the batch); scale None: read as it is.
    Padding channels of the slot must have scale = shift = 0 (cat_tseg_t's contract).  cin: valid channels, FLOP accounting only."""
    __slots__ = ('scale', 'shift', 'sstride', 'act', 'slope', 'cin')

    def __init__(self, src, w, reflect, scale=None, shift=None, sstride=0, act=L.ACT_NONE, slope=0.0, cin=None):
        super().__init__(src, w, reflect)
        self.scale, self.shift, self.sstride, self.act, self.slope, self.cin = scale, shift, int(sstride), int(act), float(slope), cin


def lattice(h, w):
    """(th, tw) of the statistics tiles cat_conv2d_ksum_norm_fwd leaves on an h x w plane -- its 128-pixel row tiles as lattice tiles of
    cat_tnorm_finalize2 --, or None where a row tile would straddle two samples or is no rectangle (the kernel declines such planes)."""
    if h <= 0 or w <= 0:
        return None
    if w <= 128 and 128 % w == 0 and h % (128 // w) == 0:
        return 128 // w, w
    if w % 128 == 0:
        return 1, 128
    return None


def _geom(segs, n, h, w, cout, ycs, ycw, rcs, act, slope):
    g = L.KSum()
    g.N, g.H, g.W, g.Cout, g.ycs, g.ycw, g.rcs, g.act, g.slope, g.nseg = n, h, w, cout, ycs, ycw, rcs, act, slope, len(segs)
    keep = []
    for k, s in enumerate(segs):
        wcl, wcs = ops.weight_cl(s.w)
        keep.append(wcl)
        t = g.seg[k]
        cin = s.src.shape[1]
        t.src, t.w = s.src.data_ptr(), wcl.data_ptr()
        t.xcs, t.c4, t.cin, t.ks, t.reflect, t.wcs = ops.act_cs(s.src), ops.cs_for(cin), getattr(s, 'cin', None) or cin, s.ks, s.reflect, wcs
    return g, keep


def applicable(segs, n, h, w, cout):
    if not _ENABLED or len(segs) > L.KSUM_MAXSEG or cout < 64:
        return False
    if ((n * h * w + 127) // 128) * ((cout + 127) // 128) < _MIN_WG:
        return False
    for s in segs:
        if s.w.shape[2] != s.w.shape[3] or s.w.shape[0] != cout or s.w.shape[1] != s.src.shape[1] or not ops.is_act(s.src):
            return False
        if ops.weight_wcs(s.w) is None or ops.weight_wcs(s.w) % 4:
            return False
    g, _ = _geom(segs, n, h, w, cout, ops.cs_for(cout), ops.cs_for(cout), 0, L.ACT_NONE, 0.0)
    return bool(L.query('cat_conv2d_ksum_supported', C.byref(g)))


def run(segs, bias, y, res=None, act=L.ACT_NONE, slope=0.0):
    """Enqueue the launch.  y: NHWC activation [n, cout, h, w]; res: optional residual of the same shape (added after the activation)."""
    n, cout, h, w = y.shape
    g, keep = _geom(segs, n, h, w, cout, ops.act_cs(y), ops.act_cs(y), 0 if res is None else ops.act_cs(res), act, slope)
    L.call('cat_conv2d_ksum_fwd', C.byref(g), None if bias is None else ops._p(bias), None if res is None else ops._p(res), ops._p(y), ops._stream())
    return y


# ---- the normalising, statistics-writing form (cat_conv2d_ksum_norm_fwd): stage 2 of a wide InstanceNorm block (cat_amd/frozen_in.py)
def _addr(t):
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def _norm_geom(segs, stats, scs):
    nm = L.KSumNorm()
    nm.stats, nm.scs = _addr(stats), scs
    for k, s in enumerate(segs):
        t = nm.seg[k]
        if getattr(s, 'scale', None) is not None:
            t.scale, t.shift, t.sstride, t.act, t.slope = _addr(s.scale), _addr(s.shift), s.sstride, s.act, s.slope
    return nm


def norm_applicable(segs, n, h, w, cout, stats=True, act=L.ACT_NONE):
    """The domain of cat_conv2d_ksum_norm_fwd (include/cat_hip.h) + this module's thresholds; the kernel never guesses: outside it the
    caller launches cat_tconv_fwd."""
    if not _ENABLED or len(segs) > L.KSUM_MAXSEG or cout < 64 or lattice(h, w) is None:
        return False
    if ((n * h * w + 127) // 128) * ((cout + 127) // 128) < _MIN_WG:
        return False
    for s in segs:
        if s.w.shape[2] != s.w.shape[3] or s.w.shape[0] != cout or s.w.shape[1] != s.src.shape[1] or not ops.is_act(s.src):
            return False
        if ops.weight_wcs(s.w) is None or ops.weight_wcs(s.w) % 4:
            return False
    cs = ops.cs_for(cout)
    g, _ = _geom(segs, n, h, w, cout, cs, cs, 0, act, 0.0)
    nm = _norm_geom(segs, 16 if stats else None, cs)      # (any non-NULL address: the predicate reads no memory)
    return bool(L.query('cat_conv2d_ksum_norm_supported', C.byref(g), C.byref(nm)))


def _tconv_norm(segs, bias, y, res, act, slope, stats):
    """The same sum on the LDS-tile kernel (cat_tconv_fwd), which stages through f_s and writes statistics on its 8 x 16 lattice: the
    fallback of run_norm.  The filters are packed per call -- a caller with a hot path keeps its own stream (fused_unit.Plan.pack2)."""
    from . import tconv
    n, cout, h, w = y.shape
    packs, tsegs, off = [], [], 0
    for s in segs:
        pk = tconv.pack(ops.weight_cl(s.w)[0], tconv.FWD)
        packs.append(pk)
        aff = {}
        if getattr(s, 'scale', None) is not None:
            aff = dict(scale=_addr(s.scale), shift=_addr(s.shift), sstride=s.sstride, act=s.act, slope=s.slope)
        tsegs.append(tconv.Segment(s.src, s.ks, s.ks // 2, s.reflect and s.ks > 1, off, **aff))
        off += pk.numel()
    part = torch.empty((n * ((h + 7) // 8) * ((w + 15) // 16), 2, ops.act_cs(y)), device=y.device, dtype=torch.float32) if stats else None
    # cat_tconv_fwd's statistics need a plain epilogue too: there the activation is one elementwise pass over y behind the launch
    late = stats and act != L.ACT_NONE
    tconv.run(tsegs, torch.cat(packs), bias, y, cout, n, h, w, h, w, act=L.ACT_NONE if late else act, slope=slope, res=res, stats=part,
              scs=ops.act_cs(y) if stats else 0)
    if late:
        L.call('cat_act_fwd', ops._p(y), ops._p(y), n * h * w * ops.act_cs(y), act, slope, ops._stream())
    return part


def run_norm(segs, bias, y, res=None, act=L.ACT_NONE, slope=0.0, stats=True):
    """Enqueue y = act(bias + sum_s conv(f_s(src_s), w_s)) + res and, with `stats`, the per-tile statistics of the sum for the norm behind it.
    -> (table [tiles][2][pixel stride of y] or None, th, tw): the tiles are th x tw lattice tiles for cat_tnorm_finalize2 -- this kernel's
    128-pixel rows inside its domain (norm_applicable), cat_tconv_fwd's 8 x 16 tiles outside it."""
    n, cout, h, w = y.shape
    if stats and res is not None:
        raise RuntimeError('ksum.run_norm: statistics are those of the sum, without a residual')
    if not norm_applicable(segs, n, h, w, cout, stats, act):
        return _tconv_norm(segs, bias, y, res, act, slope, stats), 8, 16
    th, tw = lattice(h, w)
    cs = ops.act_cs(y)
    part = torch.empty((n * h * w // 128, 2, cs), device=y.device, dtype=torch.float32) if stats else None
    g, keep = _geom(segs, n, h, w, cout, cs, cs, 0 if res is None else ops.act_cs(res), act, slope)
    nm = _norm_geom(segs, part, cs)
    L.call('cat_conv2d_ksum_norm_fwd', C.byref(g), C.byref(nm), None if bias is None else ops._p(bias), None if res is None else ops._p(res), ops._p(y),
           ops._stream())
    return part, th, tw
