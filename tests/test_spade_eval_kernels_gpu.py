"""The C-ABI entry points of csrc/spade.hip and csrc/eval_ops.hip, 19 that launch and 2 workspace queries (the GauGAN teacher's split-phase batch
norm, SPADE modulation, nearest resampling, poolings, one-hot + edges, spectral norm; the FID extractor's pooling and bilinear resize) through
L.call / L.query against float64 ATen on the host, at the shapes their launch plans switch on.  The plumbing is that of
test_streaming_kernels_gpu.py: workspaces and fresh-write outputs start as NaN, everything that must stay as the sentinel, 64 sentinels behind
every buffer, padding channels exactly 0, every case run twice and compared bit for bit.

A (host): mirrors of col_plan, ew_grid and the spectral-norm sizes held to cat_bn_ws_bytes / cat_spectral_norm_ws_bytes; every regime of B-F as
          an assertion over the case tables; the float32 ATen twin of every float64 reference within a tenth of its bar.  (D compares with
          float32 ATen itself, exactly; it has no twin.)
B (GPU):  cat_bn_stats_fwd -> cat_bn_finalize -> cat_affine_act_fwd -> cat_bn_stats_bwd -> cat_bn_apply_bwd: the sums per channel relative to
          that channel's sum of |terms|, then mean, rstd, a, b, scale, shift, running statistics, y, dx, dgamma, dbeta.
C (GPU):  cat_spade_fwd / cat_spade_bwd_stats / cat_spade_bwd_apply; the backward is handed the reference's y, so both share one mask.
D (GPU):  cat_interp_nearest_fwd, cat_upsample_nearest_bwd, cat_avgpool3x3s2_*, cat_maxpool2x2_*, cat_onehot_edges.
E (GPU):  cat_spectral_norm_fwd (two power iterations, then power_iter = 0) and cat_spectral_norm_bwd (accumulate 0 and 1).
F (GPU):  cat_pool2d_fwd, cat_global_avgpool_fwd, cat_resize_bilinear_fwd; then every CAT_REQUIRE of the 19 launching entry points.

Bars: TOL = 1e-4 with rel() (5 * TOL for gradients), TOL for everything of the origin pair, exact equality in D (TOL / 100 for the average
pooling and the upsample backward), 1e-6 for the evaluation poolings, 2e-6 absolute for the resize.

Inputs chosen by reasoning, not by result: a channel with var = 0 has rstd = eps^-1/2 = 316, and the fused map y = x * scale + shift then carries
|mean| * 316 * 2^-24 of absolute error (scale and shift round separately) against a y that is the constant beta, 0.1 * normal; such channels (the
constant channel, M == 1) hold powers of two of at most 2^-6, which keeps that error below 3e-7.  Two pixels (M == 2) have xhat = +-1 up to eps /
var, so dx is eps / (var + eps) times a difference of gradients: with var ~ 4 that is cancellation to 1e-6 of the terms, in float32 ATen as in the
kernel; the two-pixel cases use x = 0.004 * normal, var ~ eps.  With clamp = 1 a channel whose variance lies between 0 and eps is normalised by
eps^-1/2 while the kernel's dx keeps the variance term that autograd through clamp() drops (the comment at bn_bwd_apply_kernel says so): that
channel is tested forward only.  ReLU-like activations run only where no float64 pre-activation lies within 1e-4 of a kink (asserted in the
reference); the cases too large for that (P(no such value) = exp(-values * 8e-5)) run ACT_NONE / ACT_TANH.  The resize input is smooth: the kernel
and ATen form the source coordinate in float32, up to 4e-6 from the double's, which times a random image's pixel-to-pixel step would exceed the
2e-6 bar in float32 ATen as well.

Largest distances observed on an MI355X: B 1.5e-6 (y of the constant channel; the one-pixel case up to 1e-5 per channel, as reasoned above),
the origin pair 2.5e-6 with the first pixel 0 and 3.9e-6 as is (rstd, a, b, dx), sums 8.5e-8 of sum|term|; C 2.4e-7 (1.9e-7 where dx comes
from autograd); D 0 (the average pooling and the upsample backward bit for bit as well); E 5.9e-7 on dw, 2.3e-7 on v; F 5.1e-8 on the
poolings, 1.3e-7 absolute on the resize."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from oracle import ref_spade_cpu as R
from test_streaming_kernels_gpu import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_TANH, EPS, MAXREL, MOM, NAN, SENTINEL, SLOPE, TOL, _act, _cmp,
                                        _host, _in, _lib, _nchw, _nhwc, _out, _p, _same, _stream, _tail, cdiv, chan_rel, cs4, rel)

ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_RELU6)
KINKS = {ACT_RELU: (0.0,), ACT_LRELU: (0.0,), ACT_RELU6: (0.0, 6.0)}
KINK_MARGIN = 1e-4
EW_CAP = 16384                      # ew_grid of csrc/spade.hip, walk_grid of csrc/eval_ops.hip
SN_OSPLIT, SN_EPS = 16, 1e-12       # csrc/spade.hip; torch.nn.utils.spectral_norm's eps
POOL_MAX, POOL_AVG = 0, 1


# ================================================================================================ mirrors of the launch plans
def col_plan(m, cs):
    """col_plan() of csrc/spade.hip; `per` as col_stats_kernel derives it"""
    nq = cs // 4
    nz = cdiv(nq, 256)
    zq = cdiv(nq, nz)
    ppl = 256 // zq
    nb = max(1, min(cdiv(2048, nz), cdiv(m, ppl * 8)))
    return dict(nq=nq, nz=nz, zq=zq, ppl=ppl, nb=nb, per=cdiv(m, nb))


def ew_grid(n):
    return max(1, min(cdiv(n, 256), EW_CAP))


def sn_plan(o, i, k):
    """the sizes of cat_spectral_norm_fwd / _bwd"""
    taps, wcs = k * k, cs4(i)
    kp = taps * wcs
    n = o * kp
    return dict(taps=taps, wcs=wcs, Kp=kp, n=n, npart=min(1024, cdiv(n, 16384)), per=cdiv(o, SN_OSPLIT),
                ws_bytes=4 * ((SN_OSPLIT + 1) * kp + o + 1024))


# ================================================================================================ case tables
# B: (name, C, N, H, W, act, flags, seed).  flags: fwd (no backward), m1 (one pixel of powers of two), nogb (gamma / beta NULL), norun
# (running_mean / running_var NULL), nomap (scale / shift NULL: no y), nodx, nodgamma (dgamma alone NULL), acc, const (channel 0 constant),
# small (x = 0.004 * normal), lowvar (channel 1 with 0 < var < eps), clamp1, rank2 (sums doubled, count = 2M), origin0 / originraw
# (x = 8 + normal, first pixel 0 / as is)
BN_CASES = [
    ('few', 8, 1, 1, 2, ACT_RELU, 'small', 0),
    ('m1', 8, 1, 1, 1, ACT_NONE, 'fwd m1', 0),
    ('ragged', 10, 2, 33, 31, ACT_LRELU, '', 4),      # seeds 0..3 put a pre-activation within 1e-4 of the kink
    ('idle56', 400, 2, 9, 7, ACT_TANH, '', 0),
    ('trip2', 64, 1, 47, 49, ACT_NONE, '', 0),
    ('ppl1', 1024, 1, 4, 5, ACT_LRELU, '', 5),        # likewise seeds 0..4
    ('nz2', 1026, 2, 5, 5, ACT_TANH, '', 0),
    ('cap-none', 1024, 1, 100, 164, ACT_NONE, '', 0),
    ('cap-tanh', 1024, 1, 100, 164, ACT_TANH, '', 0),
    ('origin0', 8, 2, 128, 128, ACT_NONE, 'origin0', 0),
    ('originraw', 8, 2, 128, 128, ACT_NONE, 'originraw', 0),
] + [('act%d' % a, 10, 2, 9, 7, a, '', 0) for a in ACTS] + [
    ('nogb', 10, 2, 9, 7, ACT_RELU, 'nogb', 0),
    ('norun', 10, 2, 9, 7, ACT_LRELU, 'norun', 0),
    ('nomap', 10, 2, 9, 7, ACT_RELU, 'nomap', 0),
    ('nodx', 10, 2, 9, 7, ACT_RELU, 'nodx', 0),
    ('nodgamma', 10, 2, 9, 7, ACT_LRELU, 'nodgamma', 0),
    ('acc', 10, 2, 9, 7, ACT_RELU, 'acc', 0),
    ('const-clamp0', 10, 2, 9, 7, ACT_RELU, 'const', 0),
    ('const-clamp1', 10, 2, 9, 7, ACT_RELU, 'const clamp1', 0),
    ('lowvar-clamp0', 10, 2, 9, 7, ACT_NONE, 'fwd lowvar', 0),
    ('lowvar-clamp1', 10, 2, 9, 7, ACT_NONE, 'fwd lowvar clamp1', 0),
    ('rank2', 10, 2, 9, 7, ACT_RELU, 'rank2 clamp1', 0),
]
BN_BARS = {'dx': 5 * TOL}        # NORM_BARS of the streaming file
BN_ORIGIN_BARS = {}              # ORIGIN_BARS: TOL for everything

# C: (name, C, N, H, W, act, flags, seed).  flags: fwd, unit (a = 1, b = 0), rank2, gbslice (gb = channels 4.. of a buffer 8 floats wider),
# auto (the gradients by autograd; a, b are the batch's own statistics)
SP_CASES = [
    ('few', 8, 1, 1, 2, ACT_RELU, 'small', 0),
    ('m1', 8, 1, 1, 1, ACT_LRELU, 'unit', 0),
    ('ragged', 10, 2, 33, 31, ACT_LRELU, '', 0),
    ('idle56', 400, 2, 9, 7, ACT_RELU, '', 0),
    ('trip2', 64, 1, 47, 49, ACT_RELU6, '', 0),
    ('ppl1', 1024, 1, 4, 5, ACT_LRELU, '', 0),
    ('nz2', 1026, 2, 5, 5, ACT_LRELU, '', 0),
    ('cap', 1024, 1, 100, 164, ACT_LRELU, '', 0),
] + [('act%d-c%d' % (a, c), c, 2, 9, 7, a, '', 0) for c in (10, 8) for a in ACTS] + [
    ('unit', 8, 2, 9, 7, ACT_LRELU, 'unit', 0),
    ('unit-ragged', 10, 2, 9, 7, ACT_RELU, 'unit', 0),
    ('rank2', 10, 2, 9, 7, ACT_LRELU, 'rank2', 0),
    ('gbslice-vec', 8, 2, 9, 7, ACT_LRELU, 'fwd gbslice', 0),
    ('gbslice-ragged', 10, 2, 9, 7, ACT_RELU, 'fwd gbslice', 0),
    # odd C: gcs = cs4(2C) > 2C, so cat_spade_bwd_stats memsets dgb and its scalar stores dg[C + c + e] straddle the quads
    ('odd5', 5, 2, 9, 7, ACT_LRELU, '', 0),
    ('odd9', 9, 2, 9, 7, ACT_RELU, '', 0),
    ('odd7-tanh', 7, 2, 9, 7, ACT_TANH, '', 0),
    ('odd13-blocks', 13, 2, 33, 31, ACT_LRELU, '', 0),
    ('odd9-rank2', 9, 2, 9, 7, ACT_LRELU, 'rank2', 0),
    ('gbslice-odd', 9, 2, 9, 7, ACT_LRELU, 'fwd gbslice', 0),
    # auto: dx and dgb from float64 autograd through the batch statistics, not from the kernel's formulas
    ('auto-lrelu', 10, 2, 9, 7, ACT_LRELU, 'auto', 0),
    ('auto-relu-odd', 9, 2, 9, 7, ACT_RELU, 'auto', 0),
    ('auto-tanh', 8, 2, 9, 7, ACT_TANH, 'auto', 0),
    ('auto-relu6', 6, 2, 9, 7, ACT_RELU6, 'auto', 0),
]
SP_BARS = {'dgb': 5 * TOL, 'dxh': 5 * TOL, 'dx': 5 * TOL}

# D
INTERP_CASES = [      # (name, N, C, Hi, Wi, Ho, Wo, extra floats of xcs)
    ('up2', 2, 6, 5, 7, 10, 14, 0), ('up4', 1, 8, 3, 4, 12, 16, 0), ('down2', 2, 5, 16, 12, 8, 6, 0), ('down4', 1, 4, 16, 32, 4, 8, 0),
    ('frac-up', 2, 5, 7, 9, 16, 13, 0), ('frac-down', 2, 8, 12, 20, 5, 7, 0), ('to1x1', 2, 36, 16, 32, 1, 1, 0), ('identity', 2, 7, 6, 5, 6, 5, 0),
    ('xslice', 2, 6, 7, 9, 14, 18, 8), ('xslice-frac', 1, 4, 12, 20, 5, 7, 4), ('n3', 3, 5, 4, 6, 8, 12, 0),
]
UPS_FACTORS = (1, 2, 4)
AVG_SIZES = (1, 2, 3, 8, 9)
MAXPOOL_CASES = [('ties', 8, 8, 12), ('negative', 5, 6, 8), ('odd-both', 6, 7, 9), ('odd-h', 5, 7, 8), ('odd-w', 5, 8, 7), ('2x2', 9, 2, 2),
                 ('3x3', 4, 3, 3)]
ONEHOT_CASES = [(nc, True, kind) for nc in (4, 8, 35, 36) for kind in ('blocks', 'pixels')] + [(7, False, 'blocks')]

# E: (O, I, k)
SN_CASES = [(8, 5, 3), (35, 6, 4), (64, 67, 4), (1030, 3, 1), (520, 2048, 4)]
SN_BARS = {'dw': 5 * TOL, 'dw_acc': 5 * TOL}

# F
POOL_WINDOWS = [(3, 2, 0), (3, 1, 1), (2, 2, 0), (5, 2, 2), (7, 1, 3), (1, 1, 0)]
POOL_PLANES = [(13, 17), (6, 6)]
POOL_LAYOUTS = ('plain', 'xslice', 'yslice')
POOL_BAR = GAP_BAR = 1e-6
GAP_HW = (1, 35, 64, 289)
GAP_ITEMS = [(1, 4, 0), (3, 4, 0), (5, 4, 0), (1, 20, 0), (3, 8, 12)]      # (N, C4, extra floats of ycs): N * nq = 1, 3, 5, 5, 6
RESIZE_CASES = [      # (name, N, C, H, W, Ho, Wo, a, b, extra floats of xcs)
    ('up299', 2, 3, 40, 56, 299, 299, 2.0, -1.0, 0), ('down', 2, 4, 40, 56, 13, 9, 1.0, 0.0, 0), ('same', 2, 6, 40, 56, 40, 56, 2.0, -1.0, 0),
    ('to1x1', 2, 3, 40, 56, 1, 1, 1.0, 0.0, 4), ('h1', 2, 6, 1, 56, 5, 9, 2.0, -1.0, 4), ('grid-stride', 48, 3, 40, 56, 299, 299, 2.0, -1.0, 0),
]
RESIZE_BAR = 2e-6


def _id(case):
    return case[0]


def _pool_out(h, k, s, p):
    return (h + 2 * p - k) // s + 1


# ================================================================================================ references (any dtype)
def _act_grad(ym, act):
    """the derivative through the activation's OUTPUT, as cat::act_grad_from_out"""
    one = torch.ones_like(ym)
    if act in (ACT_RELU, ACT_LRELU):
        return torch.where(ym > 0, one, one * (SLOPE if act == ACT_LRELU else 0.0))
    if act == ACT_TANH:
        return 1.0 - ym * ym
    if act == ACT_RELU6:
        return ((ym > 0) & (ym < 6)).to(ym.dtype)
    return one


def _no_kink(pre, act, what):
    for k in KINKS.get(act, ()):
        d = float((pre.detach() - k).abs().min())
        assert d > KINK_MARGIN, (what, 'a pre-activation %.3g from the kink at %g: take another seed' % (d, k))


def _csum(t):
    return t.sum((0, 2, 3))


def _bn_inputs(case):
    name, c, n, h, w, act, flags, seed = case
    s = 900 + 20 * seed
    if 'origin' in flags:
        x = 8.0 + detfill.normal((n, c, h, w), s)
        if 'origin0' in flags:
            x[0, :, 0, 0] = 0.0      # the statistics pass shifts by the first pixel: here the shift is useless
    elif 'm1' in flags:
        x = torch.tensor([(-1.0) ** q * 2.0 ** -(8 + q % 4) for q in range(c)]).view(1, c, 1, 1)
    elif 'small' in flags:
        x = 0.004 * detfill.normal((n, c, h, w), s)      # see the module docstring: two pixels
    else:
        x = detfill.normal((n, c, h, w), s) * 2.0 + 3.0
    if 'const' in flags:
        x[:, 0] = 2.0 ** -6
    if 'lowvar' in flags:
        x[:, 1] = 0.002 * detfill.normal((n, h, w), s + 9)      # var 4e-6 < eps, mean ~ 0: the raw sums stay well conditioned
    ga = (3.0 if act == ACT_RELU6 else 1.0) * (1.0 + 0.2 * detfill.normal((c,), s + 1))
    be = 0.1 * detfill.normal((c,), s + 2)
    gy = detfill.normal((n, c, h, w), s + 3)
    rm0, rv0 = 0.1 * detfill.normal((c,), s + 4), 0.5 + detfill.normal((c,), s + 5).abs()
    pre = (0.5 * detfill.normal((c,), s + 6), 0.5 * detfill.normal((c,), s + 7))
    return dict(x=x, ga=ga, be=be, gy=gy, rm0=rm0, rv0=rv0, pre=pre)


def _bn_ref(case, dtype):
    """training-mode batch norm (+ activation) and its gradients; with rank2 on the gathered batch cat([x, x]), dgamma / dbeta half of that batch's
    (test_sync_batch_norm).  'sums' / 'bsums' are what ONE rank computes, '*_den' the sums of the absolute values of their terms."""
    name, c, n, h, w, act, flags, seed = case
    I = _bn_inputs(case)
    ranks = 2 if 'rank2' in flags else 1
    count = ranks * n * h * w
    rep = (lambda t: torch.cat([t] * ranks, 0))
    x = rep(I['x'].to(dtype)).requires_grad_(True)
    ga, be = ((torch.ones(c), torch.zeros(c)) if 'nogb' in flags else (I['ga'], I['be']))
    ga, be = ga.to(dtype).requires_grad_(True), be.to(dtype).requires_grad_(True)
    bc = lambda t: t[None, :, None, None]
    mean = x.mean((0, 2, 3))
    var = ((x - bc(mean)) ** 2).mean((0, 2, 3))
    rstd = var.clamp(min=EPS) ** -0.5 if 'clamp1' in flags else (var + EPS) ** -0.5
    xh = (x - bc(mean)) * bc(rstd)
    pre = xh * bc(ga) + bc(be)
    if dtype == torch.float64:
        _no_kink(pre, act, name)
    y = _act(pre, act)
    x1 = x.detach()[:n]
    out = {'mean': mean.detach(), 'rstd': rstd.detach(), 'a': rstd.detach(), 'b': (-mean * rstd).detach(),
           'sums': torch.stack([_csum(x1), _csum(x1 * x1)]), 'sums_den': torch.stack([_csum(x1.abs()), _csum(x1 * x1)])}
    if 'nomap' not in flags:
        out['scale'], out['shift'], out['y'] = (ga * rstd).detach(), (be - mean * ga * rstd).detach(), y.detach()[:n]
        if act == ACT_RELU6:
            assert bool((out['y'] == 0).any()) and bool((out['y'] == 6).any())
    if 'norun' not in flags:
        unb = var.detach() * (count / (count - 1.0) if count > 1 else 1.0)
        out['rm'] = (1 - MOM) * I['rm0'].to(dtype) + MOM * mean.detach()
        out['rv'] = (1 - MOM) * I['rv0'].to(dtype) + MOM * unb
    if 'fwd' in flags:
        return out
    gy = rep(I['gy'].to(dtype))
    g, = torch.autograd.grad(y, pre, gy, retain_graph=True)
    g1, xh1 = g.detach()[:n], xh.detach()[:n]
    out['bsums'] = torch.stack([_csum(g1), _csum(g1 * xh1)])
    out['bsums_den'] = torch.stack([_csum(g1.abs()), _csum((g1 * xh1).abs())])
    y.backward(gy)
    acc = 1.0 if 'acc' in flags else 0.0
    if 'nodx' not in flags:
        out['dx'] = x.grad[:n]
    if 'nogb' not in flags:
        out['dbeta'] = be.grad / ranks + acc * I['pre'][1].to(dtype)
        if 'nodgamma' not in flags:
            out['dgamma'] = ga.grad / ranks + acc * I['pre'][0].to(dtype)
    return out


def _sp_inputs(case):
    name, c, n, h, w, act, flags, seed = case
    s = 1100 + 20 * seed
    x = 0.004 * detfill.normal((n, c, h, w), s) if 'small' in flags else detfill.normal((n, c, h, w), s) * 1.5 + 0.3
    gb = 0.7 * detfill.normal((n, 2 * c, h, w), s + 1)
    if act == ACT_RELU6:
        gb[:, :c] += 4.0      # (1 + gamma) ~ 5: both bounds are hit
    dy = detfill.normal((n, c, h, w), s + 2)
    if 'unit' in flags:
        a, b = torch.ones(c), torch.zeros(c)
    else:
        x64 = x.double()
        mean = x64.mean((0, 2, 3))
        rstd = (((x64 - mean[None, :, None, None]) ** 2).mean((0, 2, 3)) + EPS) ** -0.5
        a, b = rstd.float(), (-mean * rstd).float()
    return dict(x=x, gb=gb, dy=dy, a=a, b=b)


def _sp_ref(case, dtype):
    """y = act(xhat * (1 + gamma) + beta), xhat = x * a + b from the GIVEN float32 a, b; the backward by its formulas, with the mask from y rounded
    to float32 (what the entry point is handed); in the 'auto' cases dx and dgb by autograd instead"""
    name, c, n, h, w, act, flags, seed = case
    I = {k: v.to(dtype) for k, v in _sp_inputs(case).items()}
    ranks = 2 if 'rank2' in flags else 1
    count = ranks * n * h * w
    bc = lambda t: t[None, :, None, None]
    xh = I['x'] * bc(I['a']) + bc(I['b'])
    gm, bt = I['gb'][:, :c], I['gb'][:, c:]
    y = _act(xh * (1.0 + gm) + bt, act)
    out = {'y': y}
    if act == ACT_RELU6:
        assert bool((y == 0).any()) and bool((y == 6).any())
    if 'fwd' in flags:
        return out
    g = I['dy'] * _act_grad(y.float().to(dtype), act)
    dxh = g * (1.0 + gm)
    s0, s1 = _csum(dxh), _csum(dxh * xh)
    out['dgb'] = torch.cat([g * xh, g], 1)
    out['dxh'] = dxh
    out['sums'], out['sums_den'] = torch.stack([s0, s1]), torch.stack([_csum(dxh.abs()), _csum((dxh * xh).abs())])
    out['dx'] = bc(I['a']) * (dxh - bc(ranks * s0 / count) - xh * bc(ranks * s1 / count))
    if 'auto' in flags:
        # independent of the formulas above: differentiate act(norm(x) * (1 + gamma) + beta) itself, the statistics included (a, b are
        # those statistics rounded to float32, 6e-8 from them)
        x, gb = I['x'].clone().requires_grad_(True), I['gb'].clone().requires_grad_(True)
        mean = x.mean((0, 2, 3))
        var = ((x - bc(mean)) ** 2).mean((0, 2, 3))
        pre = (x - bc(mean)) * bc((var + EPS) ** -0.5) * (1.0 + gb[:, :c]) + gb[:, c:]
        if dtype == torch.float64:
            _no_kink(pre, act, name)
        _act(pre, act).backward(I['dy'])
        out['dx'], out['dgb'] = x.grad, gb.grad
    return out


def _sn_inputs(case):
    o, i, k = case
    w = 0.2 * detfill.normal((o, i, k, k), 1300)
    # gw correlated with w: sum(gw * w_sn) * u v^T is then several times gw itself, and a wrong dot product cannot hide
    return dict(w=w, u=detfill.normal((o,), 1301), v=detfill.normal((i * k * k,), 1302), gw=detfill.normal((o, i, k, k), 1303) + 5.0 * w,
                pre=0.5 * detfill.normal((o, i, k, k), 1304))


def _sn_big(case):
    return sn_plan(*case)['n'] > 1 << 22


def _sn_ref(case, dtype):
    """torch.nn.utils.spectral_norm: two power iterations on the persistent u, v; sigma = u . W v; the gradient of weight_orig with u, v constant"""
    o, i, k = case
    I = {key: t.to(dtype) for key, t in _sn_inputs(case).items()}
    wm = I['w'].reshape(o, -1)
    u, v = I['u'], I['v']
    out = {}
    for it in (1, 2):
        v = F.normalize(wm.t() @ u, dim=0, eps=SN_EPS)
        s = wm @ v
        u = F.normalize(s, dim=0, eps=SN_EPS)
        vp = F.pad(v.view(i, k * k).t(), (0, cs4(i) - i)).reshape(-1)
        tag = '1' if it == 1 else ''
        out.update({'u' + tag: u, 'v' + tag: v, 'vp' + tag: vp, 'sigma' + tag: (u @ s).reshape(1)})
    sigma = out['sigma'][0]
    w_sn = I['w'] / sigma
    dw = (I['gw'] - (I['gw'] * w_sn).sum() * torch.outer(u, v).view_as(w_sn)) / sigma
    out.update({'w_sn': w_sn, 'dw': dw, 'dw_acc': dw + I['pre'], 'sigma_eval': out['sigma']})
    if not _sn_big(case):
        out['w_sn_eval'] = w_sn
    return out


def _pool_inputs(plane):
    """multiples of 2^-10: a window sum of up to 49 of them is exact in float32, and the average carries the one rounding of its division, so a
    float32 twin can stay within a tenth of the 1e-6 bar (with arbitrary normals ATen's own 3 x 3 average is 1.008e-7 from the double's)"""
    h, w = plane
    return torch.round(detfill.normal((2, 8, h, w), 1400 + h) * 1024.0) / 1024.0


def _pool_ref(mode, plane, dtype):
    x = _pool_inputs(plane).to(dtype)
    out = {}
    for k, s, p in POOL_WINDOWS:
        out['k%ds%dp%d' % (k, s, p)] = F.max_pool2d(x, k, s, p) if mode == POOL_MAX else F.avg_pool2d(x, k, s, p, count_include_pad=False)
    return out


def _gap_inputs(hw, n, c4):
    """multiples of 2^-10 as in _pool_inputs: sums of 289 of them are exact in float32 in any order"""
    return 0.5 + torch.round(detfill.normal((n, c4, hw, 1), 1500 + hw + n + c4) * 1024.0) / 1024.0


def _gap_ref(hw, dtype):
    return {'n%dc%d' % (n, c4): _gap_inputs(hw, n, c4).to(dtype).mean((2, 3)) for n, c4, ye in GAP_ITEMS}


def _resize_inputs(case):
    """a smooth image in [0.25, 0.45] (every float32 intermediate below 1: half the rounding of an image up to 1) with its own phase per
    (image, channel): neighbouring pixels differ by at most 0.002, so the 4e-6 by which the float32 source coordinate differs from the
    double's moves the value by 1e-8, and a wrong neighbour still by hundreds of bars"""
    name, n, c, h, w, ho, wo, a, b, xe = case
    ph = torch.arange(n * c, dtype=torch.float64).view(n, c, 1, 1)
    yy = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
    xx = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
    return (0.35 + 0.1 * torch.sin(0.017 * yy + 0.7 * ph) * torch.cos(0.013 * xx - 0.3 * ph)).float()


def _resize_ref(case, dtype):
    name, n, c, h, w, ho, wo, a, b, xe = case
    return {'y': a * F.interpolate(_resize_inputs(case).to(dtype), size=(ho, wo), mode='bilinear', align_corners=False) + b}


_REFS = {'B': _bn_ref, 'C': _sp_ref, 'E': _sn_ref, 'F-pool': _pool_ref, 'F-gap': _gap_ref, 'F-resize': _resize_ref}


@functools.lru_cache(maxsize=2)
def _ref(section, dtype, *key):
    """computed once per (case, dtype), shared by the tests that need it and never written to"""
    with torch.enable_grad():
        return _REFS[section](*key, dtype)


# ================================================================================================ comparisons
SUMS_KEYS = ('sums', 'bsums')


def _plain(d):
    return {k: v for k, v in d.items() if not k.startswith(SUMS_KEYS)}


def _sums_dist(got, want, den):
    """per channel, relative to the sum of the absolute values of that channel's terms: a sum near 0 is still a fair target"""
    return float(((got.double() - want.double()).abs() / (den.double() + 1e-300)).max())


def _check(section, what, got, want, bars=None, inst=False):
    for key in SUMS_KEYS:
        if key in want:
            d = _sums_dist(got[key], want[key], want[key + '_den'])
            MAXREL[section] = max(MAXREL.get(section, 0.0), d)
            print('%s %s %s per channel / sum|term| %.3g (bar %.3g)' % (section, what, key, d, TOL))
            assert d < TOL, (section, what, key, d)
    _cmp(section, what, _plain(got), _plain(want), bars, inst)


def _host_check(section, what, key, bars=None, inst=None):
    r64, r32 = _ref(section, torch.float64, *key), _ref(section, torch.float32, *key)
    for k in SUMS_KEYS:
        if k in r64:
            d = _sums_dist(r32[k], r64[k], r64[k + '_den'])
            print('host %s %s %s fp32-vs-fp64 %.3g' % (section, what, k, d))
            assert d <= TOL / 10, (section, what, k, d)
    _host(section, what, lambda dtype: _plain(_ref(section, dtype, *key)), bars, inst)


def _bn_bars(case):
    return BN_ORIGIN_BARS if 'origin' in case[6] else BN_BARS


# ================================================================================================ A: host
def test_plan_mirrors_match_the_workspace_queries():
    """cat_bn_ws_bytes and cat_spectral_norm_ws_bytes are pure host functions: nb follows from the byte count"""
    L = _lib()
    for case in BN_CASES + SP_CASES:
        name, c, n, h, w = case[:5]
        m, cs = n * h * w, cs4(c)
        nbytes = L.query('cat_bn_ws_bytes', m, cs)
        assert nbytes == 4 * col_plan(m, cs)['nb'] * 2 * cs, (case, nbytes, col_plan(m, cs))
    for case in SN_CASES:
        o, i, k = case
        p = sn_plan(o, i, k)
        assert L.query('cat_spectral_norm_ws_bytes', o, i, p['taps'], p['wcs']) == p['ws_bytes'], (case, p)
        assert p['ws_bytes'] >= 4 * (SN_OSPLIT * p['Kp'] + o) and p['ws_bytes'] >= 4 * p['npart']      # what _fwd and _bwd lay out in it
    assert ew_grid(1) == 1 and ew_grid(EW_CAP * 256) == EW_CAP == ew_grid(1 << 40)


def test_case_tables_reach_every_regime():
    """a table edit that loses a regime fails here, not silently on the GPU"""
    for table in (BN_CASES, SP_CASES):
        assert len({c[0] for c in table}) == len(table)
        plans = [(c, n * h * w, col_plan(n * h * w, cs4(c_))) for c in table for (c_, n, h, w) in [c[1:5]]]
        has = lambda pred: any(pred(c, m, p) for c, m, p in plans)
        bwd = lambda c: 'fwd' not in c[6]
        assert has(lambda c, m, p: p['nb'] == 1 and m < p['ppl'] and bwd(c))                                        # fewer pixels than pixel lanes
        assert has(lambda c, m, p: m == 1)                                                                          # count == 1
        # thread 255 idle; the last block holds 510 pixels
        assert has(lambda c, m, p: p == dict(nq=3, nz=1, zq=3, ppl=85, nb=4, per=512) and m == 2046 and c[1] % 4 and bwd(c))
        assert has(lambda c, m, p: (p['nq'], p['ppl'], p['nb']) == (100, 2, 8) and 256 - p['ppl'] * p['zq'] == 56 and bwd(c))
        assert has(lambda c, m, p: (p['ppl'], p['nb']) == (16, 18) and m == p['nb'] * p['per'] - 1 and bwd(c))      # b += 16: second, ragged trip
        assert has(lambda c, m, p: cs4(c[1]) == 1024 and (p['ppl'], p['nb'], p['per']) == (1, 3, 7) and m - 2 * p['per'] == 6 and bwd(c))
        assert has(lambda c, m, p: cs4(c[1]) == 1028 and c[1] % 4 == 2 and (p['nz'], p['zq'], p['nb']) == (2, 129, 7) and 2 * p['zq'] > p['nq']
                   and bwd(c))
        assert has(lambda c, m, p: p['nb'] == 2048 and p['per'] == 9 and cdiv(m, p['per']) == 1823 and m * p['nq'] == 4198400 > EW_CAP * 256
                   and bwd(c))
        assert has(lambda c, m, p: 256 % p['zq'] and p['ppl'] * p['zq'] < 256 and p['nb'] > 1)                      # zq does not divide 256
        assert has(lambda c, m, p: 'rank2' in c[6] and bwd(c))
        for act in ACTS:
            assert has(lambda c, m, p: c[5] == act and bwd(c) and c[1] % 4), act
    bn = {c[0]: c for c in BN_CASES}
    big = lambda c: c[1] * c[2] * c[3] * c[4] > 25000
    assert all(c[5] in (ACT_NONE, ACT_TANH) for c in BN_CASES if big(c))                    # the cap case among them
    assert {c[5] for c in BN_CASES if c[1] == 1024 and c[2] * c[3] * c[4] == 16400} == {ACT_NONE, ACT_TANH}
    flags = lambda f: [c for c in BN_CASES if set(f.split()) <= set(c[6].split())]
    for f in ('nogb', 'norun', 'nomap', 'nodx', 'nodgamma', 'acc', 'rank2', 'origin0', 'originraw', 'const clamp1', 'lowvar clamp1', 'm1 fwd'):
        assert flags(f), f
    assert any('clamp1' not in c[6] for c in flags('const')) and any('clamp1' not in c[6] for c in flags('lowvar'))
    assert all('fwd' in c[6] for c in flags('lowvar'))
    assert all(c[1:5] == (8, 2, 128, 128) for c in flags('origin0') + flags('originraw'))
    assert bn['acc'][5] != ACT_NONE and bn['nogb'][5] != ACT_NONE

    sp = {c[0]: c for c in SP_CASES}
    assert any(c[1] % 4 == 0 for c in SP_CASES if 'fwd' not in c[6]) and any(c[1] % 4 for c in SP_CASES if 'fwd' not in c[6])
    assert any('gbslice' in c[6] and c[1] % 4 == 0 for c in SP_CASES) and any('gbslice' in c[6] and c[1] % 4 for c in SP_CASES)
    assert any('unit' in c[6] for c in SP_CASES)
    spb = [c for c in SP_CASES if 'fwd' not in c[6]]
    padded = lambda c: cs4(2 * c[1]) - 2 * c[1]                                              # padding lanes of dgb: the memset of cat_spade_bwd_stats
    assert any(padded(c) and col_plan(c[2] * c[3] * c[4], cs4(c[1]))['nb'] == 1 for c in spb)
    assert any(padded(c) and col_plan(c[2] * c[3] * c[4], cs4(c[1]))['nb'] > 1 for c in spb)
    assert {padded(c) for c in spb} >= {0, 2} and any(padded(c) and 'rank2' in c[6] for c in spb)
    assert any(padded(c) and 'gbslice' in c[6] for c in SP_CASES)
    auto = [c for c in spb if 'auto' in c[6]]
    assert {c[5] for c in auto} >= {ACT_RELU, ACT_LRELU, ACT_TANH, ACT_RELU6} and any(padded(c) for c in auto) and any(c[1] % 4 == 0 for c in auto)
    assert not any('auto' in c[6] and ('unit' in c[6] or 'rank2' in c[6]) for c in SP_CASES)      # a, b must be the statistics, one rank
    assert sp['cap'][5] == ACT_LRELU and 'fwd' not in sp['cap'][6]                            # grid-stride trips of spade_fwd / spade_bwd_apply
    for c in (10, 8):
        assert {case[5] for case in SP_CASES if case[1] == c and case[2:5] == (2, 9, 7)} >= set(ACTS)

    ic = {c[0]: c for c in INTERP_CASES}
    up = lambda c: c[5] > c[3]
    assert any(up(c) and c[5] % c[3] == 0 for c in INTERP_CASES) and any(not up(c) and c[3] % c[5] == 0 and c[5] > 1 for c in INTERP_CASES)
    assert ic['frac-up'][3:7] == (7, 9, 16, 13) and ic['frac-down'][3:7] == (12, 20, 5, 7)
    assert any(c[5:7] == (1, 1) for c in INTERP_CASES) and any(c[3:5] == c[5:7] for c in INTERP_CASES)
    assert any(c[7] > 0 and up(c) for c in INTERP_CASES) and any(c[7] > 0 and c[5] % c[3] and c[3] % c[5] for c in INTERP_CASES)
    assert any(c[1] == 3 for c in INTERP_CASES) and set(UPS_FACTORS) == {1, 2, 4}
    div = lambda s, o: min(2 * o + 1, s - 1) - max(2 * o - 1, 0) + 1
    assert {(div(h, oy), div(w, ox)) for h in AVG_SIZES for w in AVG_SIZES for oy in range((h - 1) // 2 + 1) for ox in range((w - 1) // 2 + 1)} \
        == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    mp = {c[0]: c for c in MAXPOOL_CASES}
    assert {(c[2] % 2, c[3] % 2) for c in MAXPOOL_CASES} == {(0, 0), (0, 1), (1, 0), (1, 1)} and mp['2x2'][2:] == (2, 2)
    assert 'ties' in mp and 'negative' in mp and any(c[1] % 4 for c in MAXPOOL_CASES)
    assert {nc for nc, inst, kind in ONEHOT_CASES if inst} == {4, 8, 35, 36} and (7, False, 'blocks') in ONEHOT_CASES
    assert all(cs4(nc + 1) == nc + 4 for nc in (4, 8, 36)) and cs4(35 + 1) == 36      # the edge channel alone in its quad / last of a full one
    assert {kind for nc, inst, kind in ONEHOT_CASES if inst and nc % 4 == 0} == {'blocks', 'pixels'}

    snp = {c: sn_plan(*c) for c in SN_CASES}
    assert SN_CASES == [(8, 5, 3), (35, 6, 4), (64, 67, 4), (1030, 3, 1), (520, 2048, 4)]
    assert snp[(8, 5, 3)]['per'] == 1 and 8 < SN_OSPLIT                                          # empty row slices
    assert snp[(35, 6, 4)]['per'] == 3 and 12 * 3 > 35                                           # the last slices are empty
    assert (snp[(64, 67, 4)]['wcs'], snp[(64, 67, 4)]['Kp'], snp[(64, 67, 4)]['npart']) == (68, 1088, 5)
    assert snp[(1030, 3, 1)]['Kp'] == 4 and 1030 % SN_OSPLIT
    big = snp[(520, 2048, 4)]
    assert big['n'] == 17039360 and cdiv(big['n'], 16384) > 1024 == big['npart'] and big['n'] // 4 > EW_CAP * 256
    assert all(p['npart'] == 1 for c, p in snp.items() if p['n'] <= 16384) and any(1 < p['npart'] < 1024 for p in snp.values())
    assert any(i % 4 and k > 1 for o, i, k in SN_CASES) and any(o % SN_OSPLIT for o, i, k in SN_CASES)

    assert POOL_WINDOWS == [(3, 2, 0), (3, 1, 1), (2, 2, 0), (5, 2, 2), (7, 1, 3), (1, 1, 0)] and POOL_PLANES == [(13, 17), (6, 6)]
    assert (6 + 0 - 3) % 2 and {k for k, s, p in POOL_WINDOWS} >= {5, 7}
    assert all(_pool_out(d, k, s, p) > 0 and 2 * p <= k for d in (6, 13, 17) for k, s, p in POOL_WINDOWS)
    assert set(GAP_HW) == {1, 35, 64, 289} and {n * c4 // 4 for n, c4, ye in GAP_ITEMS} >= {1, 3, 5} and any(ye for n, c4, ye in GAP_ITEMS)
    assert any(n * c4 // 4 % 4 for n, c4, ye in GAP_ITEMS) and min(GAP_HW) < 64
    rc = {c[0]: c for c in RESIZE_CASES}
    assert {c[5:7] for c in RESIZE_CASES if c[3:5] == (40, 56)} >= {(299, 299), (13, 9), (40, 56), (1, 1)}
    assert rc['h1'][3] == 1 and {c[2] for c in RESIZE_CASES} == {3, 4, 6} and any(c[9] for c in RESIZE_CASES)
    assert {(c[7], c[8]) for c in RESIZE_CASES} == {(2.0, -1.0), (1.0, 0.0)}
    gs = rc['grid-stride']
    assert gs[1] * gs[5] * gs[6] * (cs4(gs[2]) // 4) == 4291248 > EW_CAP * 256 and gs[1:5] == (48, 3, 40, 56)


def test_fp32_twin_of_every_reference_is_within_a_tenth_of_the_bar():
    """B, C, E, F on the host: float32 ATen against float64 ATen, within a tenth of the bar each key is held to on the GPU"""
    for case in BN_CASES:
        _host_check('B', case[0], (case,), _bn_bars(case), inst=False)
    for case in SP_CASES:
        _host_check('C', case[0], (case,), SP_BARS, inst=False)
    for case in SN_CASES:
        _host_check('E', case, (case,), SN_BARS)
    for plane in POOL_PLANES:
        r64, r32 = _ref('F-pool', torch.float64, POOL_MAX, plane), _ref('F-pool', torch.float32, POOL_MAX, plane)
        assert all(torch.equal(r32[k].double(), r64[k]) for k in r64)
        _host_check('F-pool', plane, (POOL_AVG, plane), {k: POOL_BAR for k in r64})
    for hw in GAP_HW:
        _host_check('F-gap', hw, (hw,), {k: GAP_BAR for k in _ref('F-gap', torch.float64, hw)})
    for case in RESIZE_CASES:
        r64, r32 = _ref('F-resize', torch.float64, case)['y'], _ref('F-resize', torch.float32, case)['y']
        d = float((r32.double() - r64).abs().max())
        print('host F-resize %s fp32-vs-fp64 %.3g absolute' % (case[0], d))
        assert d <= RESIZE_BAR / 10, (case[0], d)


# ================================================================================================ GPU plumbing
@pytest.fixture(scope='module')
def dev():
    _lib()
    return torch.device('cuda:0')


class _Bufs:
    """the destinations of one run: every one is checked for its 64 sentinels at the end"""

    def __init__(self, dev, what):
        self.dev, self.what, self.flats = dev, what, []

    def out(self, name, shape, fill=NAN, init=None):
        flat, view = _out(shape, self.dev, fill)
        if init is not None:
            view.copy_(init.reshape(view.shape).to(self.dev))
        self.flats.append((name, flat))
        return view

    def tails(self):
        torch.cuda.synchronize()
        for name, flat in self.flats:
            _tail(flat, (self.what, name))


def _chan_vec(t, cs, dev):
    """[C] -> device [cs], zero on the padding"""
    return _in(F.pad(t, (0, cs - t.numel())), dev)


def _pad0(buf, c, what):
    assert bool((buf[..., c:] == 0.0).all()), (what, 'padding lanes')


def _twice(run, what):
    got = run()
    _same(got, run(), what)      # order-fixed sums: graph replays rely on it
    return got


# ================================================================================================ B: split-phase batch norm
def _bn_run(L, dev, case, T):
    name, c, n, h, w, act, flags, seed = case
    m, cs = n * h * w, cs4(c)
    ranks = 2 if 'rank2' in flags else 1
    count = float(ranks * m)
    nws = L.query('cat_bn_ws_bytes', m, cs) // 4
    assert nws == col_plan(m, cs)['nb'] * 2 * cs
    B = _Bufs(dev, name)
    ws, sums = B.out('ws', (nws,)), B.out('sums', (2, cs))
    L.call('cat_bn_stats_fwd', _p(T['x']), m, c, cs, _p(sums), _p(ws), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()), (name, 'every block, an empty one included, writes its partial')
    got = {'sums': sums.cpu()[:, :c]}
    _pad0(sums.cpu(), c, (name, 'sums'))
    if ranks == 2:
        sums.mul_(2.0)      # the all-reduce over two ranks that hold the same shard
    mean, rstd = B.out('mean', (c,)), B.out('rstd', (c,))
    a, b = B.out('a', (cs,)), B.out('b', (cs,))
    scale, shift = (None, None) if 'nomap' in flags else (B.out('scale', (cs,)), B.out('shift', (cs,)))
    rm, rv = (None, None) if 'norun' in flags else (B.out('rm', (c,), init=T['rm0']), B.out('rv', (c,), init=T['rv0']))
    gag, beg = (None, None) if 'nogb' in flags else (T['ga'], T['be'])
    L.call('cat_bn_finalize', _p(sums), count, c, cs, EPS, int('clamp1' in flags), MOM, _p(gag), _p(beg), _p(mean), _p(rstd), _p(rm), _p(rv), _p(a),
           _p(b), _p(scale), _p(shift), _stream())
    torch.cuda.synchronize()
    got.update({'mean': mean.cpu(), 'rstd': rstd.cpu()})
    for key, t in (('a', a), ('b', b), ('scale', scale), ('shift', shift)):
        if t is not None:
            _pad0(t.cpu(), c, (name, key))
            got[key] = t.cpu()[:c]
    if rm is not None:
        got['rm'], got['rv'] = rm.cpu(), rv.cpu()
    if scale is not None:
        y = B.out('y', (n, h, w, cs))
        L.call('cat_affine_act_fwd', _p(T['x']), _p(scale), _p(shift), _p(y), m, c, cs, act, SLOPE, _stream())
        torch.cuda.synchronize()
        yc = y.cpu()
        _pad0(yc, c, (name, 'y'))
        got['y'] = _nchw(yc, c)
    if 'fwd' in flags:
        B.tails()
        return got
    ws2, bs = B.out('bwd ws', (nws,)), B.out('bsums', (2, cs))
    L.call('cat_bn_stats_bwd', _p(T['x']), _p(T['dy']), _p(gag), _p(beg), _p(a), _p(b), m, c, cs, act, SLOPE, _p(bs), _p(ws2), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws2).all()), (name, 'bwd partials')
    got['bsums'] = bs.cpu()[:, :c]
    _pad0(bs.cpu(), c, (name, 'bsums'))
    local = B.out('local sums', (2, cs), init=bs)
    if ranks == 2:
        bs.mul_(2.0)
    acc = int('acc' in flags)
    dx = None if 'nodx' in flags else B.out('dx', (n, h, w, cs))
    db = None if 'nogb' in flags else B.out('dbeta', (c,), init=T['pre'][1] if acc else None)
    dg = None if ('nogb' in flags or 'nodgamma' in flags) else B.out('dgamma', (c,), init=T['pre'][0] if acc else None)
    L.call('cat_bn_apply_bwd', _p(T['x']), _p(T['dy']), _p(gag), _p(beg), _p(a), _p(b), _p(bs), count, _p(local), _p(dx), _p(dg), _p(db), acc, m, c,
           cs, act, SLOPE, _stream())
    B.tails()
    if dx is not None:
        dxc = dx.cpu()
        _pad0(dxc, c, (name, 'dx'))
        got['dx'] = _nchw(dxc, c)
    if db is not None:
        got['dbeta'] = db.cpu()
    if dg is not None:
        got['dgamma'] = dg.cpu()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('case', BN_CASES, ids=_id)
def test_split_phase_batch_norm_at_the_plan_edges(dev, case):
    """the whole chain against float64, every figure printed before it is asserted.  Origin pair (x = 8 + normal, TOL for every output): observed
    rstd 2.5e-6 with the first pixel 0 (the shifted sums shift by nothing) and 3.9e-6 as is (col_reduce_kernel converts the shifted sums back by
    M * x0 * x0): the float32 raw-sum formula itself, no finding."""
    L = _lib()
    name, c, n, h, w, act, flags, seed = case
    I = _bn_inputs(case)
    want = _ref('B', torch.float64, case)
    cs = cs4(c)
    T = {'x': _in(_nhwc(I['x'], cs), dev), 'dy': _in(_nhwc(I['gy'], cs), dev), 'ga': _in(I['ga'], dev), 'be': _in(I['be'], dev), 'rm0': I['rm0'],
         'rv0': I['rv0'], 'pre': I['pre']}
    got = _twice(lambda: _bn_run(L, dev, case, T), name)
    _check('B-origin' if 'origin' in flags else 'B', name, got, want, _bn_bars(case), inst=False)


# ================================================================================================ C: SPADE modulation
def _sp_run(L, dev, case, T):
    name, c, n, h, w, act, flags, seed = case
    m, cs, gcs = n * h * w, cs4(c), T['gcs']
    ranks = 2 if 'rank2' in flags else 1
    B = _Bufs(dev, name)
    y = B.out('y', (n, h, w, cs))
    L.call('cat_spade_fwd', _p(T['x']), _p(T['a']), _p(T['b']), _p(T['gb'], T['g0']), _p(y), m, c, cs, gcs, act, SLOPE, _stream())
    torch.cuda.synchronize()
    yc = y.cpu()
    _pad0(yc, c, (name, 'y'))
    got = {'y': _nchw(yc, c)}
    if 'fwd' in flags:
        B.tails()
        return got
    nws = L.query('cat_bn_ws_bytes', m, cs) // 4
    ws, sums = B.out('ws', (nws,)), B.out('sums', (2, cs))
    dgb, dxh = B.out('dgb', (n, h, w, gcs)), B.out('dxh', (n, h, w, cs))
    L.call('cat_spade_bwd_stats', _p(T['x']), _p(T['a']), _p(T['b']), _p(T['gb']), _p(T['y']), _p(T['dy']), _p(dgb), _p(dxh), _p(sums), m, c, cs, gcs,
           act, SLOPE, _p(ws), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()), (name, 'every block writes its partial')
    dgc, dxc, sc = dgb.cpu(), dxh.cpu(), sums.cpu()
    assert dgc[..., 2 * c:].shape[-1] == gcs - 2 * c == cs4(2 * c) - 2 * c
    _pad0(dgc, 2 * c, (name, 'dgb'))
    _pad0(dxc, c, (name, 'dxh'))
    _pad0(sc, c, (name, 'sums'))
    got.update({'dgb': _nchw(dgc, 2 * c), 'dxh': _nchw(dxc, c), 'sums': sc[:, :c]})
    if ranks == 2:
        sums.mul_(2.0)
    L.call('cat_spade_bwd_apply', _p(T['x']), _p(T['a']), _p(T['b']), _p(sums), float(ranks * m), _p(dxh), m, c, cs, _stream())
    B.tails()
    dxc = dxh.cpu()
    _pad0(dxc, c, (name, 'dx'))
    got['dx'] = _nchw(dxc, c)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('case', SP_CASES, ids=_id)
def test_spade_modulation_at_the_plan_edges(dev, case):
    L = _lib()
    name, c, n, h, w, act, flags, seed = case
    I = _sp_inputs(case)
    want = _ref('C', torch.float64, case)
    cs = cs4(c)
    sl = 'gbslice' in flags
    gcs, g0 = cs4(2 * c) + (8 if sl else 0), (4 if sl else 0)
    T = {'x': _in(_nhwc(I['x'], cs), dev), 'dy': _in(_nhwc(I['dy'], cs), dev), 'a': _chan_vec(I['a'], cs, dev), 'b': _chan_vec(I['b'], cs, dev),
         'gb': _in(_nhwc(I['gb'], gcs, fill=SENTINEL if sl else None, c0=g0), dev), 'gcs': gcs, 'g0': g0,
         'y': _in(_nhwc(want['y'].float(), cs), dev)}
    got = _twice(lambda: _sp_run(L, dev, case, T), name)
    _check('C', name, got, want, SP_BARS, inst=False)


# ================================================================================================ D: resampling, pooling, one-hot
def _exact(got, want, what):
    assert got.shape == want.shape and torch.equal(got, want), (what, float((got - want).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize('case', INTERP_CASES, ids=_id)
def test_interp_nearest(dev, case):
    L = _lib()
    name, n, c, hi, wi, ho, wo, xe = case
    ycs = cs4(c)
    xcs = ycs + xe
    x = detfill.normal((n, c, hi, wi), 1200)
    xg = _in(_nhwc(x, xcs, fill=SENTINEL if xe else None), dev)

    def run():
        B = _Bufs(dev, name)
        y = B.out('y', (n, ho, wo, ycs))
        L.call('cat_interp_nearest_fwd', _p(xg), _p(y), n, hi, wi, ho, wo, c, xcs, ycs, _stream())
        B.tails()
        return {'y': y.cpu()}
    yc = _twice(run, name)['y']
    _pad0(yc, c, name)
    _exact(_nchw(yc, c), F.interpolate(x, size=(ho, wo), mode='nearest'), name)


@pytest.mark.gpu
@pytest.mark.parametrize('f', UPS_FACTORS)
def test_upsample_nearest_bwd(dev, f):
    L = _lib()
    n, c, hi, wi = 2, 6, 5, 7
    cs = cs4(c)
    dy = detfill.normal((n, c, hi * f, wi * f), 1210 + f)
    x = torch.zeros(n, c, hi, wi, requires_grad=True)
    F.interpolate(x, scale_factor=f, mode='nearest').backward(dy)
    dyg = _in(_nhwc(dy, cs), dev)

    def run():
        B = _Bufs(dev, f)
        dx = B.out('dx', (n, hi, wi, cs))
        L.call('cat_upsample_nearest_bwd', _p(dyg), _p(dx), n, hi, wi, f, c, cs, _stream())
        B.tails()
        return {'dx': dx.cpu()}
    dxc = _twice(run, f)['dx']
    _pad0(dxc, c, f)
    _cmp('D', ('upsample bwd', f), {'dx': _nchw(dxc, c)}, {'dx': x.grad}, {'dx': TOL / 100})


@pytest.mark.gpu
def test_avgpool3x3s2_every_edge_divisor(dev):
    """F.avg_pool2d(3, 2, 1, count_include_pad=False) and its backward on every plane of AVG_SIZES x AVG_SIZES"""
    L = _lib()
    n, c = 2, 5
    cs = cs4(c)
    for h in AVG_SIZES:
        for w in AVG_SIZES:
            ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            x = detfill.normal((n, c, h, w), 1220 + 10 * h + w).requires_grad_(True)
            dy = detfill.normal((n, c, ho, wo), 1221 + 10 * h + w)
            yr = F.avg_pool2d(x, 3, 2, 1, count_include_pad=False)
            yr.backward(dy)
            xg, dyg = _in(_nhwc(x.detach(), cs), dev), _in(_nhwc(dy, cs), dev)

            def run():
                B = _Bufs(dev, (h, w))
                y, dx = B.out('y', (n, ho, wo, cs)), B.out('dx', (n, h, w, cs))
                L.call('cat_avgpool3x3s2_fwd', _p(xg), _p(y), n, h, w, c, cs, _stream())
                L.call('cat_avgpool3x3s2_bwd', _p(dyg), _p(dx), n, h, w, c, cs, _stream())
                B.tails()
                return {'y': y.cpu(), 'dx': dx.cpu()}
            got = _twice(run, (h, w))
            _pad0(got['y'], c, (h, w, 'y'))
            _pad0(got['dx'], c, (h, w, 'dx'))
            _cmp('D', ('avgpool', h, w), {'y': _nchw(got['y'], c), 'dx': _nchw(got['dx'], c)}, {'y': yr.detach(), 'dx': x.grad},
                 {'y': TOL / 100, 'dx': TOL / 100})


@pytest.mark.gpu
@pytest.mark.parametrize('case', MAXPOOL_CASES, ids=_id)
def test_maxpool2x2(dev, case):
    L = _lib()
    name, c, h, w = case
    n, cs = 2, cs4(c)
    x = detfill.normal((n, c, h, w), 1230)
    if name == 'ties':
        x = F.relu(x)
    elif name == 'negative':
        x = -1.0 - x.abs()
    x.requires_grad_(True)
    dy = detfill.normal((n, c, h // 2, w // 2), 1231)
    yr = F.max_pool2d(x, 2, 2)
    yr.backward(dy)
    if name == 'ties':
        assert bool((x.detach().unfold(2, 2, 2).unfold(3, 2, 2).reshape(n, c, h // 2, w // 2, 4) == 0).sum(-1).ge(2).any())
    xg, dyg = _in(_nhwc(x.detach(), cs), dev), _in(_nhwc(dy, cs), dev)

    def run():
        B = _Bufs(dev, name)
        y, dx = B.out('y', (n, h // 2, w // 2, cs)), B.out('dx', (n, h, w, cs))
        L.call('cat_maxpool2x2_fwd', _p(xg), _p(y), n, h, w, c, cs, _stream())
        L.call('cat_maxpool2x2_bwd', _p(xg), _p(dyg), _p(dx), n, h, w, c, cs, _stream())
        B.tails()
        return {'y': y.cpu(), 'dx': dx.cpu()}
    got = _twice(run, name)
    _pad0(got['y'], c, (name, 'y'))
    _pad0(got['dx'], c, (name, 'dx'))
    _exact(_nchw(got['y'], c), yr.detach(), (name, 'y'))
    _exact(_nchw(got['dx'], c), x.grad, (name, 'dx'))
    if h % 2:
        assert bool((got['dx'][:, h - 1] == 0.0).all()), (name, 'the last row of dx')
    if w % 2:
        assert bool((got['dx'][:, :, w - 1] == 0.0).all()), (name, 'the last column of dx')


def _onehot_inputs(nc, kind):
    n, h, w = 2, 6, 10
    rng = np.random.default_rng(1240 + nc)
    label = rng.integers(0, nc, (n, h, w)).astype(np.int32)
    label[0, 0, 0], label[0, 2, 3], label[1, 5, 9], label[1, 0, 4] = nc - 1, nc, 255, nc      # the last class; out of range: no class channel
    if kind == 'pixels':
        inst = rng.integers(0, 1000, (n, h, w)).astype(np.int32)
    else:
        # one instance per (image, half row): the last column of a row and the first of the next differ, and so do the last row of image 0
        # and the first of image 1; neither pair are neighbours.  Edges: the two columns at the middle, nothing else.
        inst = (np.arange(w)[None, None, :] >= w // 2).astype(np.int32) + 2 * np.arange(n, dtype=np.int32)[:, None, None]
        inst = inst + np.zeros((n, h, w), np.int32)
    return label, inst


def _onehot_ref(label, inst, nc):
    """numpy restatement of SPADEModel.preprocess_input / get_edges with labels >= nc giving no class"""
    n, h, w = label.shape
    out = np.zeros((n, nc + (inst is not None), h, w), np.float32)
    for k in range(nc):
        out[:, k] = label == k
    if inst is not None:
        e = np.zeros((n, h, w), bool)
        dh, dw = inst[:, 1:] != inst[:, :-1], inst[:, :, 1:] != inst[:, :, :-1]
        e[:, 1:] |= dh
        e[:, :-1] |= dh
        e[:, :, 1:] |= dw
        e[:, :, :-1] |= dw
        out[:, nc] = e
    return torch.from_numpy(out)


@pytest.mark.gpu
@pytest.mark.parametrize('nc,with_inst,kind', ONEHOT_CASES)
def test_onehot_edges(dev, nc, with_inst, kind):
    L = _lib()
    label, inst = _onehot_inputs(nc, kind)
    if not with_inst:
        inst = None
    n, h, w = label.shape
    cout = nc + int(with_inst)
    cs = cs4(cout)
    want = _onehot_ref(label, inst, nc)
    inr = label < nc
    lab_in = np.where(inr, label, 0)      # the oracle's scatter_ refuses labels >= nc: it vouches for the pixels that have a class
    ora = R.preprocess_input(torch.from_numpy(lab_in)[:, None], None if inst is None else torch.from_numpy(inst)[:, None], nc, False, inst is None)
    mask = torch.from_numpy(inr)[:, None].expand_as(want)
    assert torch.equal(ora[mask], want[mask]) and bool((want[:, :nc].sum(1)[torch.from_numpy(~inr)] == 0).all())
    if with_inst and kind == 'blocks':
        assert bool((want[:, nc, :, w // 2 - 1:w // 2 + 1] == 1).all()) and float(want[:, nc].sum()) == n * h * 2
    if with_inst and kind == 'pixels':
        assert float(want[:, nc].mean()) > 0.9

    def tail_i32(a):
        flat = torch.full((a.size + 64,), int(SENTINEL), dtype=torch.int32)
        flat[:a.size] = torch.from_numpy(a.reshape(-1))
        return flat.to(dev)
    lg, ig = tail_i32(label), None if inst is None else tail_i32(inst)

    def run():
        B = _Bufs(dev, (nc, kind))
        y = B.out('y', (n, h, w, cs))
        L.call('cat_onehot_edges', _p(lg), _p(ig), _p(y), n, h, w, nc, cs, _stream())
        B.tails()
        return {'y': y.cpu()}
    yc = _twice(run, (nc, kind))['y']
    _pad0(yc, cout, (nc, kind))
    _exact(_nchw(yc, cout), want, (nc, kind))


# ================================================================================================ E: spectral norm
def _sn_store(w, wcs):
    """[O][I][k][k] -> the kernels' [O][taps][wcs], zero on the padding lanes"""
    o, i, k, _ = w.shape
    return F.pad(w.permute(0, 2, 3, 1).reshape(o, k * k, i), (0, wcs - i)).contiguous()


def _sn_unstore(buf, i, k):
    o = buf.shape[0]
    return buf[:, :, :i].reshape(o, k, k, i).permute(0, 3, 1, 2)


def _sn_run(L, dev, case, T):
    o, i, k = case
    p = sn_plan(o, i, k)
    taps, wcs, kp = p['taps'], p['wcs'], p['Kp']
    B = _Bufs(dev, case)
    u, v = B.out('u', (o,), init=T['u']), B.out('v', (i * taps,), init=T['v'])
    vp, sigma, w_sn = B.out('vp', (kp,)), B.out('sigma', (1,)), B.out('w_sn', (o, taps, wcs))
    nws = L.query('cat_spectral_norm_ws_bytes', o, i, taps, wcs) // 4
    got = {}
    for it in (1, 2):
        for t in (vp, sigma, w_sn):
            t.fill_(NAN)
        ws = B.out('ws%d' % it, (nws,))
        L.call('cat_spectral_norm_fwd', _p(T['w']), o, i, taps, wcs, _p(u), _p(v), 1, SN_EPS, _p(sigma), _p(w_sn), _p(vp), _p(ws), _stream())
        torch.cuda.synchronize()
        tag = '1' if it == 1 else ''
        vpc = vp.cpu()
        _pad0(vpc.view(taps, wcs), i, (case, 'vp'))
        got.update({'u' + tag: u.cpu(), 'v' + tag: v.cpu(), 'vp' + tag: vpc, 'sigma' + tag: sigma.cpu()})
    wc = w_sn.cpu()
    _pad0(wc, i, (case, 'w_sn'))
    got['w_sn'] = _sn_unstore(wc, i, k)
    for acc, key in ((0, 'dw'), (1, 'dw_acc')):
        ws = B.out('bwd ws%d' % acc, (nws,))
        dw = B.out(key, (o, taps, wcs), init=T['pre'] if acc else None)
        L.call('cat_spectral_norm_bwd', _p(T['gw']), _p(w_sn), _p(u), _p(vp), _p(sigma), o, taps, wcs, _p(dw), acc, _p(ws), _stream())
        torch.cuda.synchronize()
        dwc = dw.cpu()
        _pad0(dwc, i, (case, key))
        got[key] = _sn_unstore(dwc, i, k)
    # eval mode: no power iteration, u and v stay
    vp2, sigma2, w2 = B.out('vp eval', (kp,)), B.out('sigma eval', (1,)), B.out('w_sn eval', (o, taps, wcs))
    ws = B.out('ws eval', (nws,))
    L.call('cat_spectral_norm_fwd', _p(T['w']), o, i, taps, wcs, _p(u), _p(v), 0, SN_EPS, _p(sigma2), _p(w2), _p(vp2), _p(ws), _stream())
    B.tails()
    same = torch.equal(u.cpu(), got['u']) and torch.equal(v.cpu(), got['v']) and torch.equal(vp2.cpu(), got['vp'])
    assert same, (case, 'power_iter = 0 moved u / v')
    got['sigma_eval'] = sigma2.cpu()
    if not _sn_big(case):
        got['w_sn_eval'] = _sn_unstore(w2.cpu(), i, k)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('case', SN_CASES, ids=lambda c: 'o%d-i%d-k%d' % c)
def test_spectral_norm_fwd_bwd(dev, case):
    L = _lib()
    o, i, k = case
    I = _sn_inputs(case)
    wcs = cs4(i)
    T = {'w': _in(_sn_store(I['w'], wcs), dev), 'gw': _in(_sn_store(I['gw'], wcs), dev), 'pre': _sn_store(I['pre'], wcs), 'u': I['u'], 'v': I['v']}
    got = _twice(lambda: _sn_run(L, dev, case, T), case)
    _check('E', case, got, _ref('E', torch.float64, case), SN_BARS, inst=None)


# ================================================================================================ F: evaluation kernels
@pytest.mark.gpu
@pytest.mark.parametrize('layout', POOL_LAYOUTS)
@pytest.mark.parametrize('plane', POOL_PLANES, ids=lambda p: '%dx%d' % p)
@pytest.mark.parametrize('mode', (POOL_MAX, POOL_AVG), ids=('max', 'avg'))
def test_pool2d(dev, mode, plane, layout):
    """every window of POOL_WINDOWS; xslice: the input is channels 4..12 of a 16-float pixel, yslice: the output channels 8..16 of a 20-float one"""
    L = _lib()
    h, w = plane
    x = _pool_inputs(plane)
    n, c4 = x.shape[:2]
    want = _ref('F-pool', torch.float64, mode, plane)
    xcs, x0 = (16, 4) if layout == 'xslice' else (c4, 0)
    ycs, y0 = (20, 8) if layout == 'yslice' else (c4, 0)
    xg = _in(_nhwc(x, xcs, fill=SENTINEL, c0=x0), dev)
    for k, s, p in POOL_WINDOWS:
        key = 'k%ds%dp%d' % (k, s, p)
        ho, wo = _pool_out(h, k, s, p), _pool_out(w, k, s, p)

        def run():
            B = _Bufs(dev, (mode, plane, layout, key))
            y = B.out('y', (n, ho, wo, ycs), fill=SENTINEL if ycs > c4 else NAN)
            L.call('cat_pool2d_fwd', _p(xg, x0), xcs, n, h, w, c4, k, s, p, mode, _p(y, y0), ycs, ho, wo, _stream())
            B.tails()
            return {'y': y.cpu()}
        yc = _twice(run, key)['y']
        if ycs > c4:
            assert bool((yc[..., :y0] == SENTINEL).all()) and bool((yc[..., y0 + c4:] == SENTINEL).all()), (key, 'outside the slice')
        got = _nchw(yc, c4, y0)
        if mode == POOL_MAX:
            _exact(got.double(), want[key], (plane, layout, key))
        else:
            _cmp('F', (plane, layout), {key: got}, {key: want[key]}, {key: POOL_BAR})


@pytest.mark.gpu
@pytest.mark.parametrize('hw', GAP_HW)
def test_global_avgpool(dev, hw):
    L = _lib()
    want = _ref('F-gap', torch.float64, hw)
    for n, c4, ye in GAP_ITEMS:
        key = 'n%dc%d' % (n, c4)
        ycs, y0 = c4 + ye, (4 if ye else 0)
        xg = _in(_nhwc(_gap_inputs(hw, n, c4), c4), dev)

        def run():
            B = _Bufs(dev, (hw, key))
            y = B.out('y', (n, ycs), fill=SENTINEL if ye else NAN)
            L.call('cat_global_avgpool_fwd', _p(xg), c4, n, hw, c4, _p(y, y0), ycs, _stream())
            B.tails()
            return {'y': y.cpu()}
        yc = _twice(run, key)['y']
        if ye:
            assert bool((yc[:, :y0] == SENTINEL).all()) and bool((yc[:, y0 + c4:] == SENTINEL).all()), (hw, key, 'outside the slice')
        _cmp('F', ('global avgpool', hw), {key: yc[:, y0:y0 + c4]}, {key: want[key]}, {key: GAP_BAR})


@pytest.mark.gpu
@pytest.mark.parametrize('case', RESIZE_CASES, ids=_id)
def test_resize_bilinear(dev, case):
    L = _lib()
    name, n, c, h, w, ho, wo, a, b, xe = case
    ycs = cs4(c)
    xcs = ycs + xe
    want = _ref('F-resize', torch.float64, case)['y']
    xg = _in(_nhwc(_resize_inputs(case), xcs, fill=SENTINEL if xe else None), dev)

    def run():
        B = _Bufs(dev, name)
        y = B.out('y', (n, ho, wo, ycs))
        L.call('cat_resize_bilinear_fwd', _p(xg), xcs, n, h, w, c, _p(y), ycs, ho, wo, a, b, _stream())
        B.tails()
        return {'y': y.cpu()}
    yc = _twice(run, name)['y']
    _pad0(yc, c, name)
    assert bool(torch.isfinite(yc).all()), name
    d = float((_nchw(yc, c).double() - want).abs().max())
    MAXREL['F-resize'] = max(MAXREL.get('F-resize', 0.0), d)
    print('F resize %s off by %.3g absolute (bar %.3g)' % (name, d, RESIZE_BAR))
    assert d < RESIZE_BAR, (name, d)


# ================================================================================================ refusals
# csrc/spade.hip exports 16 functions that launch and csrc/eval_ops.hip 3; with the two pure-host queries cat_bn_ws_bytes and
# cat_spectral_norm_ws_bytes (no CAT_REQUIRE; test_plan_mirrors_match_the_workspace_queries) that is 21 symbols, one more than a count of 20
LAUNCHING = ('cat_bn_stats_fwd', 'cat_bn_finalize', 'cat_bn_stats_bwd', 'cat_bn_apply_bwd', 'cat_spade_fwd', 'cat_spade_bwd_stats',
             'cat_spade_bwd_apply', 'cat_interp_nearest_fwd', 'cat_upsample_nearest_bwd', 'cat_avgpool3x3s2_fwd', 'cat_avgpool3x3s2_bwd',
             'cat_maxpool2x2_fwd', 'cat_maxpool2x2_bwd', 'cat_onehot_edges', 'cat_spectral_norm_fwd', 'cat_spectral_norm_bwd', 'cat_pool2d_fwd',
             'cat_global_avgpool_fwd', 'cat_resize_bilinear_fwd')


def _refusals(f, i32, st):
    """(entry point, arguments): every one fails a CAT_REQUIRE, which returns before anything is launched.  f / i32: a float / an int buffer."""
    r = []
    add = lambda name, *args: r.append((name, args + (st,)))
    for m, c, cs in ((2, 4, 6), (2, 5, 4), (0, 4, 4)):      # cs % 4, cs < C, M <= 0
        add('cat_bn_stats_fwd', f, m, c, cs, f, f)
        add('cat_bn_stats_bwd', f, f, f, f, f, f, m, c, cs, ACT_RELU, SLOPE, f, f)
        add('cat_bn_apply_bwd', f, f, f, f, f, f, f, 2.0, f, f, f, f, 0, m, c, cs, ACT_RELU, SLOPE)
        add('cat_spade_fwd', f, f, f, f, f, m, c, cs, 8, ACT_RELU, SLOPE)
        add('cat_spade_bwd_stats', f, f, f, f, f, f, f, f, f, m, c, cs, 8, ACT_RELU, SLOPE, f)
        add('cat_spade_bwd_apply', f, f, f, f, 2.0, f, m, c, cs)
    add('cat_bn_stats_fwd', f, 2, 4, 4, f, None)             # NULL workspace
    add('cat_bn_stats_fwd', f, 2, 4, 4, None, f)             # NULL sums
    add('cat_bn_stats_bwd', f, f, f, f, f, f, 2, 4, 4, ACT_RELU, SLOPE, f, None)
    add('cat_bn_stats_bwd', f, f, f, f, f, f, 2, 4, 4, ACT_RELU, SLOPE, None, f)
    for c, cs, count, mean in ((4, 6, 2.0, f), (5, 4, 2.0, f), (4, 4, 0.0, f), (4, 4, 2.0, None)):
        add('cat_bn_finalize', f, count, c, cs, EPS, 0, MOM, f, f, mean, f, f, f, f, f, f, f)
    add('cat_bn_apply_bwd', f, f, f, f, f, f, f, 0.0, f, f, f, f, 0, 2, 4, 4, ACT_RELU, SLOPE)      # count == 0
    add('cat_spade_bwd_apply', f, f, f, f, 0.0, f, 2, 4, 4)
    for gcs in (6, 4):                                        # gcs % 4, gcs < 2C
        add('cat_spade_fwd', f, f, f, f, f, 2, 4, 4, gcs, ACT_RELU, SLOPE)
        add('cat_spade_bwd_stats', f, f, f, f, f, f, f, f, f, 2, 4, 4, gcs, ACT_RELU, SLOPE, f)
    add('cat_spade_bwd_stats', f, f, f, f, f, f, f, f, f, 2, 4, 4, 8, ACT_RELU, SLOPE, None)
    for n, ho, c, xcs, ycs in ((1, 2, 4, 4, 8), (1, 2, 5, 8, 4), (0, 2, 4, 4, 4), (1, 0, 4, 4, 4), (1, 2, 4, 6, 4)):      # xcs < ycs, ycs < C, ...
        add('cat_interp_nearest_fwd', f, f, n, 2, 2, ho, 2, c, xcs, ycs)
    for n, ff, c, cs in ((1, 2, 4, 6), (1, 2, 5, 4), (1, 0, 4, 4), (0, 2, 4, 4)):
        add('cat_upsample_nearest_bwd', f, f, n, 2, 2, ff, c, cs)
    for n, h, c, cs in ((1, 4, 4, 6), (1, 4, 5, 4), (0, 4, 4, 4), (1, 0, 4, 4)):
        add('cat_avgpool3x3s2_fwd', f, f, n, h, 4, c, cs)
        add('cat_avgpool3x3s2_bwd', f, f, n, h, 4, c, cs)
    for n, h, w, c, cs in ((1, 1, 4, 4, 4), (1, 4, 1, 4, 4), (1, 4, 4, 4, 6), (1, 4, 4, 5, 4), (0, 4, 4, 4, 4)):      # H < 2, W < 2, ...
        add('cat_maxpool2x2_fwd', f, f, n, h, w, c, cs)
        add('cat_maxpool2x2_bwd', f, f, f, n, h, w, c, cs)
    add('cat_onehot_edges', i32, i32, f, 1, 2, 2, 4, 6)
    add('cat_onehot_edges', i32, i32, f, 1, 2, 2, 4, 4)       # no room for the edge channel
    add('cat_onehot_edges', None, i32, f, 1, 2, 2, 4, 8)
    add('cat_onehot_edges', i32, i32, f, 0, 2, 2, 4, 8)
    for o, i, taps, wcs, u, ws in ((2, 4, 1, 6, f, f), (2, 5, 1, 4, f, f), (0, 4, 1, 4, f, f), (2, 4, 0, 4, f, f), (2, 4, 1, 4, None, f),
                                   (2, 4, 1, 4, f, None)):
        add('cat_spectral_norm_fwd', f, o, i, taps, wcs, u, f, 1, SN_EPS, f, f, f, ws)
    for o, taps, wcs, dw, ws in ((2, 1, 6, f, f), (0, 1, 4, f, f), (2, 0, 4, f, f), (2, 1, 4, None, f), (2, 1, 4, f, None)):
        add('cat_spectral_norm_bwd', f, f, f, f, f, o, taps, wcs, dw, 0, ws)
    # pool2d on a 6 x 6 plane: k > 7, 2 * pad > k, a wrong Ho, a wrong Wo, the layout, the mode, the stride
    for xcs, c4, k, s, p, mode, ycs, ho, wo in ((4, 4, 8, 1, 3, 0, 4, 5, 5), (4, 4, 3, 1, 2, 0, 4, 8, 8), (4, 4, 3, 2, 0, 0, 4, 3, 2),
                                                (4, 4, 3, 2, 0, 0, 4, 2, 3), (4, 8, 3, 2, 0, 0, 8, 2, 2), (8, 6, 3, 2, 0, 0, 8, 2, 2),
                                                (4, 4, 3, 2, 0, 0, 6, 2, 2), (4, 4, 3, 2, 0, 2, 4, 2, 2),
                                                (4, 4, 3, 0, 0, 0, 4, 2, 2), (4, 4, 0, 1, 0, 0, 4, 6, 6)):
        add('cat_pool2d_fwd', f, xcs, 1, 6, 6, c4, k, s, p, mode, f, ycs, ho, wo)
    add('cat_pool2d_fwd', None, 4, 1, 6, 6, 4, 3, 2, 0, 0, f, 4, 2, 2)
    for xcs, n, hw, c4, ycs in ((4, 1, 0, 4, 4), (4, 1, 4, 8, 8), (4, 1, 4, 4, 6), (4, 0, 4, 4, 4), (4, 1, 4, 6, 8)):
        add('cat_global_avgpool_fwd', f, xcs, n, hw, c4, f, ycs)
    for x, xcs, c, ycs, ho in ((f, 4, 5, 4, 2), (f, 4, 3, 6, 2), (f, 4, 3, 4, 0), (None, 4, 3, 4, 2), (f, 4, 0, 4, 2)):
        add('cat_resize_bilinear_fwd', x, xcs, 1, 2, 2, c, f, ycs, ho, 2, 1.0, 0.0)
    return r


@pytest.mark.gpu
def test_every_require_refuses_and_writes_nothing(dev):
    """argument checks only: each call returns -22 before any launch, L.call raises, and the one buffer every pointer names stays the sentinel"""
    L = _lib()
    ff, f = _out((1 << 16,), dev, SENTINEL)
    ii = torch.full((4096,), int(SENTINEL), dtype=torch.int32, device=dev)
    cases = _refusals(_p(f), C.c_void_p(ii.data_ptr()), _stream())
    assert len(LAUNCHING) == 19 and set(LAUNCHING) <= set(L.SIGNATURES) and {name for name, args in cases} == set(LAUNCHING)
    for name, args in cases:
        with pytest.raises(RuntimeError, match=name):
            L.call(name, *args)
        assert L.query(name, *args) == -22, (name, args)
    torch.cuda.synchronize()
    assert bool((ff == SENTINEL).all()) and bool((ii == int(SENTINEL)).all()), 'a refused call wrote'
