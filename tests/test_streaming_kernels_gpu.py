"""The stand-alone streaming kernels (csrc/norm.hip, csrc/dwconv.hip, csrc/ka_loss.hip, csrc/loss_multi.hip and the reductions / optimiser step of
csrc/elementwise.hip) through the C ABI against float64 ATen / numpy on the host, at the shapes their own launch plans switch on: more than one
partial block, the second trip of every finalize loop, the block caps with their grid-stride loops, idle lanes, NULL arguments, accumulate.

A (host): Python mirrors of the launch plans (plan / walk_blocks of norm.hip, dw_wg_plan, gram_plan, cs_plan, loss_nb, ew_grid) held to the
          library's pure-host *_ws_bytes queries; a coverage test that names every regime of B-E and fails when a table edit loses one; for every
          case the float64 reference and the same computation in float32 ATen agree to a tenth of the bar used for it.
B (GPU):  cat_norm_fwd / cat_norm_bwd: y, save_mean, save_rstd, running statistics, num_batches_tracked, dx, dgamma, dbeta; rel() over the tensor and
          per (group, channel); NULL gamma / beta / dgamma / dbeta, accumulate, every activation, the origin case (first pixel 0, mean 8).
C (GPU):  cat_dwconv2d_fwd / _dgrad / _wgrad / _multi_fwd: channel slices, planes smaller than the window, every kw of the weight gradient with
          accumulate, the LDS limit on both sides, the grid-stride trip, the run table of the multi kernel, containment of a non-finite pixel.
D (GPU):  cat_ka_fwd / cat_ka_bwd on correlated rows: gram_kernel<3> and <4>, D == 4, the cap of 512 partial blocks, nbx != nby, the first
          unrolled trip of ka_gram_reduce_kernel; the workspace pins the gram_plan mirror to the kernel.
E (GPU):  cat_loss_fwd / cat_loss_bwd (kinds 0..7, the size ladder up to both block caps, cat_loss_multi_* bit for bit), cat_channel_sum,
          cat_adam_step against cat_adam_step_dev, cat_add_n.

Bars: TOL = 1e-4 with rel() of test_kernels_gpu.py (5 * TOL for the norm's and KA's gradients, as test_norm_fwd_bwd / test_ka have them), 1e-5
absolute for the KA value, 1e-6 for the scalar losses, Adam and add_n; exact equality for zero lanes, sentinels and repeated runs.  Workspaces and
fresh-write destinations start as NaN, everything a kernel must not touch as the sentinel 7.0.  The element-walk norm kernels (CAT_NORM_WALK=0)
are not covered here; csrc/spade.hip and csrc/eval_ops.hip are in test_spade_eval_kernels_gpu.py.  Largest distances observed on an MI355X:
B 2.2e-6 (origin case 1.1e-5), C 1.8e-7, D 3.2e-7 on the gradient and 9.0e-8 on the value, E 2.6e-9 / 5.6e-8 on a loss value / gradient,
1.7e-7 channel sum, 8.5e-8 add_n, Adam's second moment 1.3e-5."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_kernels_gpu import TOL, rel

SENTINEL = 7.0
NAN = float('nan')
EPS, MOM, SLOPE = 1e-5, 0.1, 0.2
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_RELU6 = 0, 1, 2, 3, 4
DWMULTI_MAXQ, DWMULTI_MAXRUN = 64, 8      # include/cat_hip.h
KA_MAXN, KA_MAXNB = 64, 512               # csrc/ka_loss.hip
DW_MAXW = 16384                           # csrc/dwconv.hip: taps * cs floats of LDS filter
MAXREL = {}      # section -> largest distance from the float64 reference seen in this process (printed by every case)


def cs4(c):
    return (c + 3) // 4 * 4


def cdiv(a, b):
    return -(-a // b)


def _act(v, act, slope=SLOPE):
    return {ACT_NONE: v, ACT_RELU: F.relu(v), ACT_LRELU: F.leaky_relu(v, slope), ACT_TANH: torch.tanh(v), ACT_RELU6: torch.clamp(v, 0.0, 6.0)}[act]


def chan_rel(got, want, inst):
    """the largest rel() over the (group, channel) slices of [N, C, H, W]: one channel with small values cannot hide behind a large one"""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    red = (2, 3) if inst else (0, 2, 3)
    return float(((g - w).abs().amax(red) / (w.abs().amax(red) + 1e-12)).max())


def _dist(key, got, want, inst):
    """every figure a key is held to: (label, distance); 4-d keys of the norm cases also per (group, channel)"""
    out = [(key, rel(got, want))]
    if inst is not None and want.dim() == 4:
        out.append((key + '/channel', chan_rel(got, want, inst)))
    return out


def _cmp(section, what, got, want, bars=None, inst=None):
    """every tensor of the reference dict `want` against the same key of `got`: rel() < bars[key] (TOL where not named)"""
    bad = []      # every figure is printed before the first one fails the case
    for key in sorted(want):
        assert tuple(got[key].shape) == tuple(want[key].shape), (what, key, tuple(got[key].shape), tuple(want[key].shape))
        assert bool(torch.isfinite(got[key].double()).all()), (what, key)
        bar = (bars or {}).get(key, TOL)
        for label, d in _dist(key, got[key], want[key], inst):
            MAXREL[section] = max(MAXREL.get(section, 0.0), d)
            print('%s %s %s rel %.3g (bar %.3g)' % (section, what, label, d, bar))
            if not d < bar:
                bad.append((label, d))
    print('%s largest rel so far %.3g' % (section, MAXREL.get(section, 0.0)))
    assert not bad, (section, what, bad)


def _host(section, what, ref, bars=None, inst=None):
    """reachability of the bar: the float32 ATen twin of the reference within a tenth of the bar of the float64 one"""
    r64, r32 = ref(torch.float64), ref(torch.float32)
    assert sorted(r64) == sorted(r32)
    for key in sorted(r64):
        bar = (bars or {}).get(key, TOL)
        for label, d in _dist(key, r32[key], r64[key], inst):
            print('host %s %s %s fp32-vs-fp64 rel %.3g' % (section, what, label, d))
            assert d <= bar / 10, (section, what, label, d)


# ================================================================================================ mirrors of the launch plans
def norm_plan(mode, c, n, h, w):
    """plan() and walk_blocks() of csrc/norm.hip"""
    cs = cs4(c)
    G, Pg = (n, h * w) if mode == 'instance' else (1, n * h * w)
    nq = cs // 4
    nz = cdiv(nq, 256)
    zq = cdiv(nq, nz)
    ppl = 256 // zq
    nb = max(1, min(cdiv(2048, G * nz), 1024, cdiv(Pg, ppl * 16)))
    nbw = max(1, min(cdiv(4096, G * nz), cdiv(Pg, ppl * 8)))
    return dict(G=G, Pg=Pg, cs=cs, nq=nq, nz=nz, zq=zq, ppl=ppl, nb=nb, nbw=nbw, floats=G * nb * 2 * cs + 4 * G * cs)


def dw_wg_plan(n, ho, wo, xcs, kh):
    """dw_wg_plan() of csrc/dwconv.hip"""
    ppl = 256 // (xcs // 4)
    nb = max(1, min(cdiv(1024, kh), cdiv(n * ho * wo, ppl * 16)))
    return dict(ppl=ppl, nb=nb, nq=xcs // 4)


def gram_plan(n, d):
    """gram_plan() of csrc/ka_loss.hip"""
    nt = cdiv(n, 16)
    nb = max(1, min(d // 2048, KA_MAXNB))
    chunk = cdiv(cdiv(d, nb * 4), 16) * 16
    return dict(NT=nt, NN=nt * 16, nb=nb, chunk=chunk)


def cs_plan(m, cs):
    """cs_plan() of csrc/elementwise.hip"""
    nq = cs // 4
    nz = cdiv(nq, 256)
    zq = cdiv(nq, nz)
    ppl = 256 // zq
    return dict(nq=nq, nz=nz, zq=zq, ppl=ppl, nb=max(1, min(cdiv(512, nz), cdiv(m, ppl * 16))))


def loss_nb(nquads):
    return max(1, min(cdiv(nquads, 1024), 1024))


def loss_bwd_nb(nquads):
    return max(1, min(cdiv(nquads, 256), 8192))


def ew_grid(n):
    return max(1, min(cdiv(n, 256), 8192))


# ================================================================================================ case tables
# B: (mode, C, N, H, W, act, flags); flags: noaffine (gamma / beta NULL), nodparam (dgamma / dbeta NULL), acc (accumulate = 1), fwd (no backward),
# origin (x = 8 + normal, the group's first pixel 0)
NORM_CASES = [
    ('instance', 16, 2, 33, 33, ACT_RELU, ''),
    ('instance', 6, 3, 47, 45, ACT_LRELU, ''),
    ('batch', 256, 2, 48, 48, ACT_RELU, ''),
    ('instance', 1100, 2, 5, 5, ACT_NONE, ''),
    ('batch', 8, 2, 1, 1, ACT_NONE, 'fwd'),
    ('batch', 8, 2, 1, 3, ACT_NONE, ''),
    ('batch', 7, 3, 6, 5, ACT_RELU, 'noaffine'),
    ('instance', 7, 3, 6, 5, ACT_RELU, 'noaffine'),
    ('batch', 7, 3, 6, 5, ACT_LRELU, 'nodparam'),
    ('instance', 7, 3, 6, 5, ACT_LRELU, 'nodparam'),
    ('batch', 7, 3, 6, 5, ACT_RELU, 'acc'),
    ('instance', 7, 3, 6, 5, ACT_RELU, 'acc'),
    ('batch', 8, 2, 128, 128, ACT_RELU, 'origin'),
    ('instance', 8, 2, 128, 128, ACT_RELU, 'origin'),
] + [(m, 10, 2, 9, 7, a, '') for m in ('batch', 'instance') for a in (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_RELU6)]
NORM_BARS = {'dx': 5 * TOL}      # as test_norm_fwd_bwd has them
ORIGIN_BARS = {}                 # the origin case: TOL for everything


def _norm_id(case):
    return '%s-c%d-n%d-%dx%d-act%d%s' % (case[:6] + (('-' + case[6]) if case[6] else '',))


# C: (name, C, k, reflect, N, H, W, parts): pad = k // 2; the weight gradient always runs with accumulate 0 and 1
DW_CASES = [
    ('k7-zero-3x3', 5, 7, 0, 2, 3, 3, ('fwd', 'dgrad', 'wgrad')),          # the window is larger than the plane
    ('k5-reflect-3x3', 5, 5, 1, 2, 3, 3, ('fwd', 'dgrad', 'wgrad')),       # pad == H - 1
    ('wgrad-kw1', 44, 1, 0, 2, 20, 20, ('wgrad',)),
    ('wgrad-kw3', 44, 3, 1, 2, 20, 20, ('wgrad',)),
    ('wgrad-kw5', 44, 5, 0, 2, 20, 20, ('wgrad',)),
    ('wgrad-kw7', 44, 7, 1, 2, 20, 20, ('wgrad',)),                        # nq 11, ppl 23: three idle lanes, nb 3
    ('wgrad-ppl1', 1024, 3, 0, 1, 5, 5, ('wgrad',)),                       # ppl 1, nb 2
    ('lds-652', 652, 5, 0, 1, 4, 3, ('fwd', 'dgrad')),                     # 25 * 652 = 16300 floats: the largest filter that fits
    ('grid-stride', 68, 3, 0, 2, 250, 250, ('fwd', 'dgrad')),              # 2 125 000 lanes > 8192 * 256
]
DW_SLICE_ACTS = (ACT_LRELU, ACT_RELU6)
DW_LDS_REFUSED_C = 656
KS_CYCLE = (3, 1, 5)
DWM_PLANES = [(2, 3, 3), (1, 7, 13), (2, 19, 37)]


def _dwm_ks(pattern):
    """kernel size per quad: 'cycle' 7 quads of (3, 1, 5) (unsorted, runs of length 1), 'one' a single run, 'maxrun' exactly CAT_DWMULTI_MAXRUN
    runs, 'maxq' CAT_DWMULTI_MAXQ quads in runs of 8"""
    if pattern == 'cycle':
        return [KS_CYCLE[q % 3] for q in range(7)]
    if pattern == 'one':
        return [5] * 5
    if pattern == 'maxrun':
        return [KS_CYCLE[q % 3] for q in range(DWMULTI_MAXRUN)]
    return [KS_CYCLE[(q // 8) % 3] for q in range(DWMULTI_MAXQ)]


def _runs(ks):
    return 1 + sum(1 for a, b in zip(ks, ks[1:]) if a != b)


# (pattern, plane, reflect, extra floats of xcs, of ycs, act, bias)
DWM_CASES = [(pat, pl, refl, (4, 8, 0)[(i + pl) % 3], (8, 4, 12)[(i + refl) % 3], (ACT_RELU, ACT_NONE, ACT_LRELU)[(i + pl + refl) % 3], (i + pl) % 2)
             for i, pat in enumerate(('cycle', 'one', 'maxrun', 'maxq')) for pl in range(3) for refl in (0, 1)]

# D: (N, Cx, Cy, H, W)
KA_CASES = [
    (33, 64, 32, 32, 34),        # gram_kernel<3>
    (48, 8, 12, 6, 5),           # <3> at its upper edge
    (49, 20, 8, 64, 68),         # <4>; nbx 42, nby 17
    (64, 8, 12, 6, 5),           # <4>, N == KA_MAXN (64 KB of static LDS)
    (17, 4, 4, 1, 1),            # D == 4: nb 1, three empty waves
    (3, 260, 256, 65, 63),       # nb capped at 512, chunk 528: the trailing waves are entirely empty
    (5, 6, 9, 112, 110),         # nbx 48: one below the first unrolled trip of ka_gram_reduce_kernel; padding lanes
    (3, 6, 9, 112, 112),         # nbx 49: the first unrolled trip
    (2, 6, 3, 130, 128),         # nbx 65, nby 32
]
KA_GOUT = -1.3
KA_BARS = {'dX': 5 * TOL}


def _ka_dims(case):
    n, cx, cy, h, w = case
    return cs4(cx) * h * w, cs4(cy) * h * w


# E: scalar losses: kind -> (needs b, target)
LOSS_KINDS = {0: (1, 0.0), 1: (0, 1.0), 2: (0, 0.0), 3: (0, 0.0), 4: (0, 0.0), 5: (1, 0.0), 6: (0, 1.0), 7: (0, 0.0)}
LOSS_SMALL = (360, 5)                                            # M, C: padding lanes (cs 8), nb 1
LOSS_LADDER = [(1025, 3), (2 * 256 * 257, 5), (2 * 512 * 513, 13)]      # 1025 quads; 263 168 quads (nb 257); 2 101 248 quads (both caps)
LOSS_BAR = 1e-6
LOSS_GOUT = -0.5


def _loss_scale(m, c):
    """the `scale` of cat_loss_bwd, in [1, 2): with it gout * scale / (M * C) is a power of two, so the gradient of the float32 twin carries the one
    rounding of a - b (6e-8) and can be held to a tenth of 1e-6; with an arbitrary factor its three roundings alone reach 1.8e-7"""
    return m * c / 2.0 ** int(np.floor(np.log2(m * c)))
CHANSUM_CASES = [(50, 5), (4608, 256), (40, 1100), (9000, 16)]
ADAM_NS = (1, 255, 1027)
ADAM_WDS = (0.0, 0.01)
ADAM_HYPER = dict(lr=2e-4, b1=0.5, b2=0.999, eps=1e-8, gscale=0.5, steps=3)
ADAM_BAR = ADDN_BAR = 1e-6
ADDN_SMALL = 2 * 5 * 7 * 8
ADDN_LARGE = 4 * (8192 * 256 + 1000)


# ================================================================================================ references (any dtype)
def _norm_inputs(case):
    mode, c, n, h, w, act, flags = case
    if 'origin' in flags:
        x = 8.0 + detfill.normal((n, c, h, w), 713)
        if mode == 'instance':
            x[:, :, 0, 0] = 0.0      # the statistics pass shifts by the group's first pixel: here the shift is useless
        else:
            x[0, :, 0, 0] = 0.0
    else:
        x = detfill.normal((n, c, h, w), 713) * 2.0 + 3.0
    ga = (3.0 if act == ACT_RELU6 else 1.0) * (1.0 + 0.2 * detfill.normal((c,), 714))      # ReLU6: scaled so that both bounds are hit
    be = 0.1 * detfill.normal((c,), 715)
    if 'noaffine' in flags:
        ga, be = torch.ones(c), torch.zeros(c)
    gy = detfill.normal((n, c, h, w), 716)
    pre = (0.5 * detfill.normal((c,), 717), 0.5 * detfill.normal((c,), 718))      # dgamma / dbeta before an accumulating call
    return x, ga, be, gy, pre


def _norm_ref(case, dtype):
    mode, c, n, h, w, act, flags = case
    inst = mode == 'instance'
    x, ga, be, gy, pre = _norm_inputs(case)
    x, ga, be = (t.to(dtype).requires_grad_(True) for t in (x, ga, be))
    red = (2, 3) if inst else (0, 2, 3)
    mean = x.mean(red, keepdim=True)
    var = ((x - mean) ** 2).mean(red, keepdim=True)
    rstd = (var + EPS) ** -0.5
    y = _act((x - mean) * rstd * ga[None, :, None, None] + be[None, :, None, None], act)
    flat = lambda t: t.detach().reshape(n if inst else 1, c)
    out = {'y': y.detach(), 'mean': flat(mean), 'rstd': flat(rstd)}
    if act == ACT_RELU6:
        assert bool((out['y'] == 0).any()) and bool((out['y'] == 6).any())
    if not inst:
        cnt = n * h * w
        out['rm'] = MOM * flat(mean)[0]                                      # from zeros
        out['rv'] = (1 - MOM) * torch.ones(c, dtype=dtype) + MOM * flat(var)[0] * cnt / (cnt - 1)
    if 'fwd' not in flags:
        y.backward(gy.to(dtype))
        out['dx'] = x.grad
        if 'nodparam' not in flags:
            acc = 1.0 if 'acc' in flags else 0.0
            out['dgamma'] = ga.grad + acc * pre[0].to(dtype)
            out['dbeta'] = be.grad + acc * pre[1].to(dtype)
    return out


def _dw_inputs(case):
    name, c, k, reflect, n, h, w, parts = case
    x = detfill.normal((n, c, h, w), 731)
    wt = detfill.normal((c, 1, k, k), 732, 1.0 / k)
    b = detfill.normal((c,), 733, 0.1)
    gy = detfill.normal((n, c, h, w), 734)      # pad = k // 2: the output plane is the input plane
    pre = 0.5 * detfill.normal((c, 1, k, k), 735)
    return x, wt, b, gy, pre


def _dw_ref(case, dtype):
    """y; dx (under reflect padding the gradient of the PADDED plane, which is what cat_dwconv2d_dgrad writes); dw and pre + dw"""
    name, c, k, reflect, n, h, w, parts = case
    p = k // 2
    x, wt, b, gy, pre = _dw_inputs(case)
    x, wt = x.to(dtype).requires_grad_(True), wt.to(dtype).requires_grad_(True)
    if reflect and p:
        xp = F.pad(x, (p,) * 4, mode='reflect')
        xp.retain_grad()
        y = F.conv2d(xp, wt, b.to(dtype), groups=c)
    else:
        xp = x
        y = F.conv2d(x, wt, b.to(dtype), padding=p, groups=c)
    y.backward(gy.to(dtype))
    out = {}
    if 'fwd' in parts:
        out['y'] = y.detach()
    if 'dgrad' in parts:
        out['dx'] = xp.grad
    if 'wgrad' in parts:
        out['dw'] = wt.grad
        out['dw_acc'] = wt.grad + pre.to(dtype)
    return out


def _slice_inputs(act):
    x = detfill.normal((2, 7, 9, 7), 741)
    wt = detfill.normal((7, 1, 3, 3), 742, (3.0 if act == ACT_RELU6 else 1.0))
    b = detfill.normal((7,), 743, 0.1)
    return x, wt, b


def _slice_ref(act, dtype):
    x, wt, b = (t.to(dtype) for t in _slice_inputs(act))
    y = _act(F.conv2d(x, wt, b, padding=1, groups=7), act)
    if act == ACT_RELU6:
        assert bool((y == 0).any()) and bool((y == 6).any())
    return {'y': y}


def _dwm_inputs(case):
    pat, pl, refl, xe, ye, act, bias = case
    ks = _dwm_ks(pat)
    n, h, w = DWM_PLANES[pl]
    c = 4 * len(ks)
    x = detfill.normal((n, c, h, w), 751)
    frame = torch.zeros(c, 1, 5, 5)
    for q, k in enumerate(ks):
        o = 2 - k // 2
        frame[4 * q:4 * q + 4, :, o:o + k, o:o + k] = detfill.normal((4, 1, k, k), 760 + q, 1.0 / k)
    b = detfill.normal((c,), 752, 0.1) if bias else None
    return x, frame, b, ks


def _dwm_ref(case, dtype):
    """k x k filters centred in a 5 x 5 frame of zeros: one 5 x 5 depthwise conv over the plane padded by 2 is the same sum"""
    pat, pl, refl, xe, ye, act, bias = case
    x, frame, b, ks = _dwm_inputs(case)
    xp = F.pad(x.to(dtype), (2,) * 4, mode='reflect' if refl else 'constant')
    return {'y': _act(F.conv2d(xp, frame.to(dtype), None if b is None else b.to(dtype), groups=x.shape[1]), act)}


def _ka_inputs(case):
    """correlated rows (random rows in high dimension make both Gram matrices diagonal, KA ~ 1 and its gradient pure round-off):
    X_i = s_i * B + E_i, Y_i = t_i * B' + E'_i; -> X [N, Dx], Y [N, Dy] as the kernels see them, padding lanes zero"""
    n, cx, cy, h, w = case
    s = torch.linspace(-1.5, 2.0, n)
    t = s.flip(0) * s.flip(0).abs()
    rows = []
    for c, coef, seed in ((cx, s, 771), (cy, t, 781)):
        base = detfill.normal((1, h * w, c), seed)
        noise = detfill.normal((n, h * w, c), seed + 1)
        rows.append(F.pad(coef[:, None, None] * base + noise, (0, cs4(c) - c)).reshape(n, -1).contiguous())
    return rows


def _gram(X, chunk=2048):
    """X X^T as the pairwise sum of the Gram matrices of 2048-column slices: in float32 one matmul over a million columns is as accurate as the
    BLAS of the machine happens to block it (2.8e-6 on the KA value with one, 4e-7 with another); this order is fixed"""
    parts = [X[:, i:i + chunk] @ X[:, i:i + chunk].t() for i in range(0, X.shape[1], chunk)]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def _ka_ref(case, dtype):
    X, Y = _ka_inputs(case)
    X, Y = X.to(dtype).requires_grad_(True), Y.to(dtype)
    gx, gy = _gram(X), _gram(Y)
    ka = (gx * gy).sum() / ((gx * gx).sum() * (gy * gy).sum()).sqrt()
    (KA_GOUT * ka).backward()
    return {'ka': ka.detach(), 'dX': X.grad}


def _loss_inputs(kind, m, c):
    """[M, C] values scaled so that every mean stays below 0.25: the bar is 1e-6 ABSOLUTE, and a float32 cannot hold a value above 2 to a tenth
    of it.  BCE-with-logits (kind 6) gets logits out to |a| = 30 on both sides."""
    a = detfill.normal((m, c), 800 + kind)
    b = None
    if kind in (0, 5):
        a, b = 0.1 * a, 0.1 * detfill.normal((m, c), 810 + kind)
    elif kind == 1:
        a = 1.0 + 0.2 * a
    elif kind == 2:
        a = 0.9 + 0.3 * a
    elif kind == 3:
        a = -0.9 + 0.3 * a
    elif kind in (4, 7):
        a = 0.05 + 0.1 * a
    else:
        a = 3.0 + a
        a[0, 0], a[1, 1], a[2, 2], a[m - 1, c - 1] = 30.0, -30.0, 17.5, -9.0
    return a, b


def _loss_ref(kind, m, c, dtype):
    a, b = _loss_inputs(kind, m, c)
    t = LOSS_KINDS[kind][1]
    a = a.to(dtype).requires_grad_(True)
    b = None if b is None else b.to(dtype)
    if kind == 0:
        v = (a - b).abs().mean()
    elif kind == 1:
        v = ((a - t) ** 2).mean()
    elif kind == 2:
        v = -torch.clamp(a - 1.0, max=0.0).mean()
    elif kind == 3:
        v = -torch.clamp(-a - 1.0, max=0.0).mean()
    elif kind == 4:
        v = -a.mean()
    elif kind == 5:
        v = ((a - b) ** 2).mean()
    elif kind == 6:
        v = ((1.0 - t) * a + torch.clamp(-a, min=0.0) + torch.log1p(torch.exp(-a.abs()))).mean()
    else:
        v = a.mean()
    (LOSS_GOUT * _loss_scale(m, c) * v).backward()
    return {'value': v.detach(), 'da': a.grad}


def _loss_cmp(what, got, want, host=False):
    """the value within 1e-6 absolute, the gradient within 1e-6 rel() (a tenth of each on the host)"""
    bar = LOSS_BAR / 10 if host else LOSS_BAR
    dv = abs(float(got['value'].double()) - float(want['value']))
    dg = rel(got['da'], want['da'])
    if not host:
        MAXREL['E'] = max(MAXREL.get('E', 0.0), dv, dg)
    print('%sE %s value %.9g off by %.3g, da rel %.3g (bar %.3g)' % ('host ' if host else '', what, float(want['value']), dv, dg, bar))
    assert abs(float(want['value'])) < 0.25, (what, float(want['value']))
    assert (dv <= bar and dg <= bar) if host else (dv < bar and dg < bar), (what, dv, dg)


def _chansum_inputs(m, c):
    return 0.5 + detfill.normal((m, c), 830), detfill.normal((c,), 831)


def _chansum_ref(m, c, dtype):
    x, pre = _chansum_inputs(m, c)
    s = x.to(dtype).sum(0)
    return {'sum': s, 'sum_acc': s + pre.to(dtype)}


def _adam_inputs(n):
    h = ADAM_HYPER
    return detfill.normal((n,), 840), [detfill.normal((n,), 841 + s) for s in range(h['steps'])]


def _adam_ref(n, wd, dtype):
    """torch.optim.Adam (no amsgrad) written out; the bias corrections in double as the kernels' host side has them"""
    h = ADAM_HYPER
    p0, grads = _adam_inputs(n)
    p, m, v = p0.to(dtype), torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
    for step, g in enumerate(grads, 1):
        g = g.to(dtype) * h['gscale']
        if wd:
            g = g + wd * p
        m = m + (g - m) * (1 - h['b1'])
        v = h['b2'] * v + (1 - h['b2']) * g * g
        bc1, bc2 = 1.0 - h['b1'] ** step, 1.0 - h['b2'] ** step
        p = p - (h['lr'] / bc1) * (m / (v.sqrt() / bc2 ** 0.5 + h['eps']))
    return {'p': p, 'm': m, 'v': v}


def _addn_inputs(nsrc, n):
    return [detfill.normal((n,), 860 + i) for i in range(nsrc)]


def _addn_ref(nsrc, n, dtype):
    s = 0
    for t in _addn_inputs(nsrc, n):
        s = s + t.to(dtype)
    return {'sum': s}


# ================================================================================================ A: host
def _lib():
    from cat_amd import _lib as L
    L.load()
    return L


def _conv_geom(L, n, h, w, c, xcs, ycs, k, reflect, act=ACT_NONE, ycw=0):
    p = k // 2
    return L.ConvGeom(n, h, w, c, xcs, h, w, c, ycs, k, k, 1, p, L.PAD_REFLECT if reflect else L.PAD_ZERO, act, SLOPE, ycw, 0)


def test_plan_mirrors_match_the_workspace_queries():
    """cat_norm_ws_bytes, cat_dwconv2d_wgrad_ws_bytes and cat_channel_sum_ws_bytes are pure host functions: nb follows from the byte count"""
    L = _lib()
    for case in NORM_CASES:
        mode, c, n, h, w, act, flags = case
        p = norm_plan(mode, c, n, h, w)
        g = L.NormGeom(n, h * w, c, p['cs'], L.NORM_INSTANCE if mode == 'instance' else L.NORM_BATCH, EPS, MOM, act, SLOPE)
        nbytes = L.query('cat_norm_ws_bytes', C.byref(g))
        assert nbytes == 4 * p['floats'], (case, nbytes, p)
        assert (nbytes // 4 // (p['G'] * p['cs']) - 4) // 2 == p['nb'], (case, nbytes, p)
    for case in DW_CASES:
        name, c, k, reflect, n, h, w, parts = case
        if 'wgrad' in parts:
            p = dw_wg_plan(n, h, w, cs4(c), k)
            g = _conv_geom(L, n, h, w, c, cs4(c), cs4(c), k, reflect)
            nbytes = L.query('cat_dwconv2d_wgrad_ws_bytes', C.byref(g))
            assert nbytes == 4 * p['nb'] * k * k * cs4(c), (case, nbytes, p)
    for m, c in CHANSUM_CASES:
        nbytes = L.query('cat_channel_sum_ws_bytes', m, cs4(c))
        assert nbytes == 4 * cs_plan(m, cs4(c))['nb'] * cs4(c), (m, c, nbytes)
    for n in (1, 16, 17, 49, 64):
        assert L.query('cat_ka_ws_bytes', n) == 4 * (4 + 2 * n * n + 2 * KA_MAXNB * (cdiv(n, 16) * 16) ** 2)
    assert L.query('cat_loss_ws_bytes', 1 << 40) == 4 * 1024


def test_case_tables_reach_every_regime():
    """a table edit that loses a regime fails here, not silently on the GPU"""
    plans = [(case, norm_plan(*case[:5])) for case in NORM_CASES]
    has = lambda pred: any(pred(case, p) for case, p in plans)
    inst, batch = (lambda case: case[0] == 'instance'), (lambda case: case[0] == 'batch')
    assert has(lambda case, p: p['nb'] == 1)
    assert has(lambda case, p: inst(case) and p['nb'] == 2 and p['Pg'] % p['nb'] and case[1] % 4 == 0)              # ragged last block
    assert has(lambda case, p: inst(case) and p['nb'] == 2 and p['cs'] > case[1] and p['nq'] == 2)                   # padding channels, two quads
    assert has(lambda case, p: 1 < p['nb'] <= 64) and has(lambda case, p: p['nb'] > 64)                              # second trip of the finalize loops
    assert has(lambda case, p: p['nz'] > 1 and p['nb'] > 1 and p['G'] > 1)
    assert has(lambda case, p: p['nbw'] > 1 and p['Pg'] % p['nbw'])
    assert has(lambda case, p: batch(case) and p['Pg'] == 2 and 'fwd' in case[6])
    assert has(lambda case, p: batch(case) and 2 < p['Pg'] <= 8 and 'fwd' not in case[6])
    for mode in (inst, batch):
        for flag in ('noaffine', 'nodparam', 'acc', 'origin'):
            assert has(lambda case, p: mode(case) and flag in case[6]), flag
        for act in (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_RELU6):
            assert has(lambda case, p: mode(case) and case[5] == act), act
    assert dict(norm_plan('batch', 256, 2, 48, 48), floats=0) == dict(G=1, Pg=4608, cs=256, nq=64, nz=1, zq=64, ppl=4, nb=72, nbw=144, floats=0)

    dw = {case[0]: case for case in DW_CASES}
    wg = [(case, dw_wg_plan(case[4], case[5], case[6], cs4(case[1]), case[2])) for case in DW_CASES if 'wgrad' in case[7]]
    assert {case[2] for case, p in wg} == {1, 3, 5, 7}
    assert any(case[2] == 7 and p['nb'] > 1 and 0 < 256 - p['ppl'] * p['nq'] for case, p in wg)                       # idle pixel lanes
    assert any(p['ppl'] == 1 and p['nb'] > 1 and cs4(case[1]) == 1024 for case, p in wg)
    assert dw_wg_plan(2, 20, 20, 44, 7) == dict(ppl=23, nb=3, nq=11)
    assert any(case[2] > max(case[5], case[6]) and not case[3] for case in DW_CASES)                                  # window larger than the plane
    assert any(case[3] and case[2] // 2 == case[5] - 1 for case in DW_CASES)                                          # reflect pad == H - 1
    assert 25 * cs4(dw['lds-652'][1]) <= DW_MAXW < 25 * (cs4(dw['lds-652'][1]) + 4) == 25 * DW_LDS_REFUSED_C
    gs = dw['grid-stride']
    assert gs[4] * gs[5] * gs[6] * (cs4(gs[1]) // 4) > 8192 * 256 == ew_grid(1 << 40) * 256 and {'fwd', 'dgrad'} <= set(gs[7])
    ksets = {pat: _dwm_ks(pat) for pat in ('cycle', 'one', 'maxrun', 'maxq')}
    assert _runs(ksets['cycle']) == len(ksets['cycle']) and ksets['cycle'][:3] == list(KS_CYCLE)
    assert _runs(ksets['one']) == 1 and _runs(ksets['maxrun']) == DWMULTI_MAXRUN
    assert len(ksets['maxq']) == DWMULTI_MAXQ and _runs(ksets['maxq']) <= DWMULTI_MAXRUN
    for pat in ksets:
        assert {(c[1], c[2]) for c in DWM_CASES if c[0] == pat} == {(pl, r) for pl in range(3) for r in (0, 1)}
    assert any(c[3] > 0 for c in DWM_CASES) and any(c[4] > 0 for c in DWM_CASES)

    kp = [(case, gram_plan(case[0], _ka_dims(case)[0]), gram_plan(case[0], _ka_dims(case)[1])) for case in KA_CASES]
    assert {px['NT'] for case, px, py in kp} >= {3, 4}
    assert any(case[0] == 48 for case, px, py in kp) and any(case[0] == KA_MAXN for case, px, py in kp)
    assert any(_ka_dims(case) == (4, 4) and px['nb'] == 1 for case, px, py in kp)
    assert any(px['nb'] == KA_MAXNB and (4 * px['nb'] - 1) * px['chunk'] >= _ka_dims(case)[0] for case, px, py in kp)   # the last wave is empty
    assert any(px['NT'] == 4 and px['nb'] != py['nb'] and px['nb'] % 16 and py['nb'] % 16 for case, px, py in kp)
    assert {48, 49, 65} <= {px['nb'] for case, px, py in kp}
    assert any(_ka_dims(case)[0] % 16 for case in KA_CASES) and any(cs4(case[1]) != case[1] for case in KA_CASES)
    assert gram_plan(3, 1064700) == dict(NT=1, NN=16, nb=512, chunk=528)
    assert (gram_plan(49, 87040)['nb'], gram_plan(49, 34816)['nb']) == (42, 17)

    nq = lambda m, c: m * (cs4(c) // 4)
    assert loss_nb(nq(*LOSS_SMALL)) == 1 and cs4(LOSS_SMALL[1]) > LOSS_SMALL[1]
    assert [loss_nb(nq(m, c)) for m, c in LOSS_LADDER] == [2, 257, 1024]
    assert nq(*LOSS_LADDER[0]) == 1025 and nq(*LOSS_LADDER[2]) == 2101248 > 1024 * 1024        # grid-stride trips behind the cap of 1024
    assert cdiv(nq(*LOSS_LADDER[2]), 256) > 8192 == loss_bwd_nb(nq(*LOSS_LADDER[2]))
    cp = [cs_plan(m, cs4(c)) for m, c in CHANSUM_CASES]
    assert any(p['nb'] == 1 for p in cp) and any(1 < p['nb'] <= 64 for p in cp) and any(p['nb'] > 64 for p in cp) and any(p['nz'] > 1 for p in cp)
    assert cs_plan(4608, 256)['nb'] == 72
    assert ADDN_LARGE // 4 > 8192 * 256 and ADDN_SMALL % 4 == 0


def test_fp32_twin_of_every_reference_is_within_a_tenth_of_the_bar():
    """B-E on the host: float32 ATen against float64 ATen, within a tenth of the bar each key is held to on the GPU"""
    for case in NORM_CASES:
        _host('B', _norm_id(case), functools.partial(_norm_ref, case), ORIGIN_BARS if 'origin' in case[6] else NORM_BARS, inst=case[0] == 'instance')
    for case in DW_CASES:
        _host('C', case[0], functools.partial(_dw_ref, case))
    for act in DW_SLICE_ACTS:
        _host('C-slice', act, functools.partial(_slice_ref, act))
    for case in DWM_CASES:
        _host('C-multi', case, functools.partial(_dwm_ref, case))
    for case in KA_CASES:
        r64, r32 = _ka_ref(case, torch.float64), _ka_ref(case, torch.float32)
        dv, dg = abs(float(r32['ka']) - float(r64['ka'])), rel(r32['dX'], r64['dX'])
        print('host D %s KA %.6f fp32-vs-fp64 value %.3g dX rel %.3g' % (case, float(r64['ka']), dv, dg))
        assert 0.3 <= float(r64['ka']) <= 0.97, (case, float(r64['ka']))
        assert dv <= 1e-6 and dg <= 5 * TOL / 10, (case, dv, dg)
    for kind in LOSS_KINDS:
        _loss_cmp(('kind', kind) + LOSS_SMALL, _loss_ref(kind, *LOSS_SMALL, torch.float32), _loss_ref(kind, *LOSS_SMALL, torch.float64), host=True)
    for m, c in LOSS_LADDER:
        for kind in (0, 5):
            _loss_cmp(('kind', kind, m, c), _loss_ref(kind, m, c, torch.float32), _loss_ref(kind, m, c, torch.float64), host=True)
    for m, c in CHANSUM_CASES:
        _host('E-chansum', (m, c), functools.partial(_chansum_ref, m, c))
    for n in ADAM_NS:
        for wd in ADAM_WDS:
            _host('E-adam', (n, wd), functools.partial(_adam_ref, n, wd), {'p': ADAM_BAR})
    for nsrc in range(1, 9):
        _host('E-addn', nsrc, functools.partial(_addn_ref, nsrc, ADDN_SMALL), {'sum': ADDN_BAR})
    _host('E-addn', 'large', functools.partial(_addn_ref, 2, ADDN_LARGE), {'sum': ADDN_BAR})


# ================================================================================================ GPU plumbing
@pytest.fixture(scope='module')
def dev():
    _lib()
    return torch.device('cuda:0')


def _p(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * off)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _out(shape, dev, fill=NAN):
    """a destination of `shape` (NaN: fresh-write; the sentinel: must stay) with 64 sentinels behind it: a write past the end is seen"""
    numel = int(np.prod(shape))
    flat = torch.full((numel + 64,), fill, device=dev)
    flat[numel:] = SENTINEL
    return flat, flat[:numel].view(*shape)


def _in(t, dev):
    """a host tensor on the device, 64 sentinels behind it: a read past the end stays inside the allocation and gives a wrong answer"""
    flat = torch.full((t.numel() + 64,), SENTINEL)
    flat[:t.numel()] = t.reshape(-1)
    return flat.to(dev)[:t.numel()].view(*t.shape)


def _tail(flat, what):
    assert bool((flat[-64:] == SENTINEL).all()), (what, 'tail')


def _nhwc(x, cs, pad=0.0, fill=None, c0=0):
    """x [N, C, H, W] -> host [N, H, W, cs]: the channels from c0, `pad` in the padding lanes of the quad range, `fill` everywhere else"""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, cs), pad if fill is None else fill)
    buf[..., c0:c0 + cs4(c)] = pad
    buf[..., c0:c0 + c] = x.permute(0, 2, 3, 1)
    return buf


def _nchw(buf, c, c0=0):
    return buf[..., c0:c0 + c].permute(0, 3, 1, 2)


def _same(a, b, what):
    """bit for bit (no NaN on either side)"""
    for key in a:
        assert torch.equal(a[key], b[key]), (what, key, 'differs between two runs')


# ================================================================================================ B: norm
def _norm_run(L, dev, case, xg, dyg, gag, beg, preg):
    mode, c, n, h, w, act, flags = case
    inst = mode == 'instance'
    p = norm_plan(mode, c, n, h, w)
    cs, G = p['cs'], p['G']
    g = L.NormGeom(n, h * w, c, cs, L.NORM_INSTANCE if inst else L.NORM_BATCH, EPS, MOM, act, SLOPE)
    nws = L.query('cat_norm_ws_bytes', C.byref(g)) // 4
    wsf, ws = _out((nws,), dev)
    yf, y = _out((n, h, w, cs), dev)
    mf, mean = _out((G, c), dev)
    rf, rstd = _out((G, c), dev)
    rm, rv, nbt = torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.int64, device=dev)
    L.call('cat_norm_fwd', C.byref(g), _p(xg), _p(gag), _p(beg), _p(y), _p(mean), _p(rstd), None if inst else _p(rm), None if inst else _p(rv),
           None if inst else _p(nbt), _p(ws), _stream())
    torch.cuda.synchronize()
    for flat, what in ((wsf, 'ws'), (yf, 'y'), (mf, 'mean'), (rf, 'rstd')):
        _tail(flat, (case, what))
    yc = y.cpu()
    assert bool((yc[..., c:] == 0.0).all()), (case, 'padding channels of y')
    got = {'y': _nchw(yc, c), 'mean': mean.cpu(), 'rstd': rstd.cpu()}
    if not inst:
        got['rm'], got['rv'] = rm.cpu(), rv.cpu()
        assert int(nbt) == 1, (case, int(nbt))
    if 'fwd' in flags:
        return got
    wsf, ws = _out((nws,), dev)
    dxf, dx = _out((n, h, w, cs), dev)
    dg = db = None
    if 'nodparam' not in flags:
        dgf, dg = _out((c,), dev)
        dbf, db = _out((c,), dev)
        if 'acc' in flags:
            dg.copy_(preg[0])
            db.copy_(preg[1])
    L.call('cat_norm_bwd', C.byref(g), _p(xg), _p(dyg), _p(gag), _p(beg), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), int('acc' in flags), _p(ws),
           _stream())
    torch.cuda.synchronize()
    _tail(wsf, (case, 'bwd ws'))
    _tail(dxf, (case, 'dx'))
    dxc = dx.cpu()
    assert bool((dxc[..., c:] == 0.0).all()), (case, 'padding channels of dx')
    got['dx'] = _nchw(dxc, c)
    if dg is not None:
        _tail(dgf, (case, 'dgamma'))
        _tail(dbf, (case, 'dbeta'))
        got['dgamma'], got['dbeta'] = dg.cpu(), db.cpu()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize('case', NORM_CASES, ids=_norm_id)
def test_norm_fwd_bwd_at_the_plan_edges(dev, case):
    """cat_norm_fwd / cat_norm_bwd against float64; observed on an MI355X up to 2.2e-6.  Origin case (x = 8 + normal, first pixel 0, so the shifted
    sums shift by nothing; the bar is TOL for every output): observed rstd 1.1e-5, y 1.0e-5 and dx 1.1e-5 per channel, mean 1.8e-7, running_var
    1.9e-6 -- where an estimate from the code put a correct kernel."""
    L = _lib()
    mode, c, n, h, w, act, flags = case
    x, ga, be, gy, pre = _norm_inputs(case)
    want = _norm_ref(case, torch.float64)
    cs = cs4(c)
    xg, dyg = _in(_nhwc(x, cs), dev), _in(_nhwc(gy, cs), dev)
    affine = 'noaffine' not in flags
    gag, beg = (_in(ga, dev), _in(be, dev)) if affine else (None, None)
    preg = [t.to(dev) for t in pre]
    got = _norm_run(L, dev, case, xg, dyg, gag, beg, preg)
    _cmp('B-origin' if 'origin' in flags else 'B', _norm_id(case), got, want, ORIGIN_BARS if 'origin' in flags else NORM_BARS, inst=mode == 'instance')
    _same(got, _norm_run(L, dev, case, xg, dyg, gag, beg, preg), case)      # order-fixed partial sums: graph replays rely on it


# ================================================================================================ C: depthwise
def _dw_weight(wt, dev):
    return _in(wt.contiguous(), dev)


@pytest.mark.gpu
@pytest.mark.parametrize('case', DW_CASES, ids=lambda c: c[0])
def test_dwconv_fwd_dgrad_wgrad(dev, case):
    L = _lib()
    name, c, k, reflect, n, h, w, parts = case
    p = k // 2
    x, wt, b, gy, pre = _dw_inputs(case)
    want = _dw_ref(case, torch.float64)
    cs = cs4(c)
    g = _conv_geom(L, n, h, w, c, cs, cs, k, reflect)
    xg, dyg, wg, bg = _in(_nhwc(x, cs), dev), _in(_nhwc(gy, cs), dev), _dw_weight(wt, dev), _in(b, dev)
    got = {}
    if 'fwd' in parts:
        yf, y = _out((n, h, w, cs), dev)
        L.call('cat_dwconv2d_fwd', C.byref(g), _p(xg), _p(wg), _p(bg), _p(y), _stream())
        torch.cuda.synchronize()
        _tail(yf, (name, 'y'))
        yc = y.cpu()
        assert bool((yc[..., c:] == 0.0).all()), (name, 'padding channels of y')
        got['y'] = _nchw(yc, c)
    if 'dgrad' in parts:
        hin, win = (h + 2 * p, w + 2 * p) if reflect else (h, w)
        dxf, dx = _out((n, hin, win, cs), dev)
        L.call('cat_dwconv2d_dgrad', C.byref(g), _p(dyg), _p(wg), _p(dx), cs, _stream())
        torch.cuda.synchronize()
        _tail(dxf, (name, 'dx'))
        dxc = dx.cpu()
        assert bool((dxc[..., c:] == 0.0).all()), (name, 'padding channels of dx')
        got['dx'] = _nchw(dxc, c)
    if 'wgrad' in parts:
        nws = L.query('cat_dwconv2d_wgrad_ws_bytes', C.byref(g)) // 4
        assert nws == dw_wg_plan(n, h, w, cs, k)['nb'] * k * k * cs
        for acc, key in ((0, 'dw'), (1, 'dw_acc')):
            wsf, ws = _out((nws,), dev)
            dwf, dwt = _out((c, 1, k, k), dev)
            if acc:
                dwt.copy_(pre.to(dev))
            L.call('cat_dwconv2d_wgrad', C.byref(g), _p(xg), _p(dyg), _p(dwt), acc, _p(ws), _stream())
            torch.cuda.synchronize()
            _tail(wsf, (name, 'ws'))
            _tail(dwf, (name, key))
            assert bool(torch.isfinite(ws).all()), (name, 'the final kernel reads every partial')
            got[key] = dwt.cpu()
    _cmp('C', name, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize('act', DW_SLICE_ACTS)
def test_dwconv_fwd_into_a_channel_slice(dev, act):
    """xcs == ycs == 24; the call owns 8 channels (C = 7) from channel 8 (ycw = 8) with a fused activation"""
    L = _lib()
    x, wt, b = _slice_inputs(act)
    n, c, h, w = x.shape
    g = _conv_geom(L, n, h, w, c, 24, 24, 3, 0, act=act, ycw=8)
    xg = _in(_nhwc(x, 24, fill=SENTINEL, c0=8), dev)
    yf, y = _out((n, h, w, 24), dev, SENTINEL)
    wg, bg = _dw_weight(wt, dev), _in(b, dev)
    L.call('cat_dwconv2d_fwd', C.byref(g), _p(xg, 8), _p(wg), _p(bg), _p(y, 8), _stream())
    torch.cuda.synchronize()
    _tail(yf, (act, 'y'))
    yc = y.cpu()
    assert bool((yc[..., :8] == SENTINEL).all()) and bool((yc[..., 16:] == SENTINEL).all()), 'outside the slice'
    assert bool((yc[..., 15] == 0.0).all()), 'the padding channel of the slice'
    _cmp('C', ('slice', act), {'y': _nchw(yc, c, 8)}, _slice_ref(act, torch.float64))


@pytest.mark.gpu
def test_dwconv_lds_limit_is_refused_on_both_sides(dev):
    """k = 5: 652 channels fit the LDS filter stage (DW_CASES 'lds-652' computes), 656 do not: a non-zero return code, the output untouched"""
    L = _lib()
    n, h, w, k = 1, 4, 3, 5
    for c, dxcs, fn in ((DW_LDS_REFUSED_C, None, 'fwd'), (DW_LDS_REFUSED_C, DW_LDS_REFUSED_C, 'dgrad'), (652, DW_LDS_REFUSED_C, 'dgrad')):
        cs = cs4(c)
        g = _conv_geom(L, n, h, w, c, cs, cs, k, 0)
        xg, wg = _in(torch.zeros(n, h, w, cs), dev), _in(torch.zeros(c, 1, k, k), dev)
        of, o = _out((n, h, w, dxcs or cs), dev, SENTINEL)
        if fn == 'fwd':
            rc = L.query('cat_dwconv2d_fwd', C.byref(g), _p(xg), _p(wg), None, _p(o), _stream())
        else:
            rc = L.query('cat_dwconv2d_dgrad', C.byref(g), _p(xg), _p(wg), _p(o), dxcs, _stream())
        torch.cuda.synchronize()
        assert rc != 0, (c, dxcs, fn)
        assert bool((of == SENTINEL).all()), (c, dxcs, fn, 'a refused call wrote')
    # dxcs == 652 next to it computes: zeros in, zeros out
    g = _conv_geom(L, n, h, w, 652, 652, 652, k, 0)
    xg, wg = _in(torch.zeros(n, h, w, 652), dev), _in(torch.ones(652, 1, k, k), dev)
    of, o = _out((n, h, w, 652), dev)
    L.call('cat_dwconv2d_dgrad', C.byref(g), _p(xg), _p(wg), _p(o), 652, _stream())
    torch.cuda.synchronize()
    _tail(of, 'dx')
    assert bool((o == 0.0).all())


def _dwm_geom(L, n, h, w, ks, xcs, ycs, reflect, act, nq=None):
    g = L.DwMulti()
    g.N, g.H, g.W, g.nq, g.xcs, g.ycs, g.reflect, g.act, g.slope = n, h, w, len(ks) if nq is None else nq, xcs, ycs, reflect, act, SLOPE
    for q, k in enumerate(ks[:DWMULTI_MAXQ]):
        g.ks[q] = k
    return g


def _w25(frame, dev):
    """[C][1][5][5] -> the kernel's [25][C]"""
    return _in(frame[:, 0].permute(1, 2, 0).reshape(25, -1).contiguous(), dev)


@pytest.mark.gpu
@pytest.mark.parametrize('case', DWM_CASES, ids=lambda c: '%s-plane%d-refl%d' % c[:3])
def test_dwconv_multi_fwd_run_table(dev, case):
    L = _lib()
    pat, pl, refl, xe, ye, act, bias = case
    x, frame, b, ks = _dwm_inputs(case)
    n, c, h, w = x.shape
    xcs, ycs = c + xe, c + ye
    g = _dwm_geom(L, n, h, w, ks, xcs, ycs, refl, act)
    xg = _in(_nhwc(x, xcs, fill=SENTINEL), dev)
    yf, y = _out((n, h, w, ycs), dev, SENTINEL)
    w25, bg = _w25(frame, dev), (None if b is None else _in(b, dev))
    L.call('cat_dwconv2d_multi_fwd', C.byref(g), _p(xg), _p(w25), _p(bg), _p(y), _stream())
    torch.cuda.synchronize()
    _tail(yf, (case, 'y'))
    yc = y.cpu()
    assert bool((yc[..., c:] == SENTINEL).all()), (case, 'beyond 4 * nq')
    _cmp('C', ('multi',) + case[:3], {'y': _nchw(yc, c)}, _dwm_ref(case, torch.float64))


@pytest.mark.gpu
def test_dwconv_multi_fwd_refuses_what_its_tables_cannot_hold(dev):
    L = _lib()
    n, h, w = 1, 3, 3
    for ks, nq in (([KS_CYCLE[q % 3] for q in range(DWMULTI_MAXRUN + 1)], None), ([1] * DWMULTI_MAXQ, DWMULTI_MAXQ + 1)):
        c = 4 * (nq or len(ks))
        g = _dwm_geom(L, n, h, w, ks, c, c, 0, ACT_NONE, nq)
        xg, w25 = _in(torch.zeros(n, h, w, c), dev), _in(torch.zeros(25, c), dev)
        yf, y = _out((n, h, w, c), dev, SENTINEL)
        rc = L.query('cat_dwconv2d_multi_fwd', C.byref(g), _p(xg), _p(w25), None, _p(y), _stream())
        torch.cuda.synchronize()
        assert rc != 0, (len(ks), nq)
        assert bool((yf == SENTINEL).all()), 'a refused call wrote'


@pytest.mark.gpu
@pytest.mark.parametrize('entry', ['cat_dwconv2d_fwd', 'cat_dwconv2d_multi_fwd'])
@pytest.mark.parametrize('k', [3, 5])
def test_dwconv_contains_a_non_finite_pixel(dev, entry, k):
    """+inf at pixel (0, 0) of one channel, zero padding: outputs of that channel whose window does not hold (0, 0), and every other channel, equal
    the run without it bit for bit (out-of-plane taps must be skipped or selected away, never multiplied by 0)"""
    L = _lib()
    n, h, w, c, ch = 2, 6, 7, 8, 5
    ks = [8 - k, k]      # the multi kernel: quad 0 has the other kernel size, quad 1 (channel 5) has k
    x = detfill.normal((n, c, h, w), 791)
    frame = torch.zeros(c, 1, 5, 5)
    for q, kq in enumerate(ks if entry.endswith('multi_fwd') else [k, k]):
        o = 2 - kq // 2
        frame[4 * q:4 * q + 4, :, o:o + kq, o:o + kq] = 0.5 + detfill.normal((4, 1, kq, kq), 792 + q).abs()      # no zero tap: inf * w stays inf
    b = detfill.normal((c,), 794, 0.1)
    outs = []
    for poisoned in (0, 1):
        xx = x.clone()
        if poisoned:
            xx[0, ch, 0, 0] = float('inf')
        xg, bg = _in(_nhwc(xx, c), dev), _in(b, dev)
        yf, y = _out((n, h, w, c), dev)
        if entry.endswith('multi_fwd'):
            g = _dwm_geom(L, n, h, w, ks, c, c, 0, ACT_NONE)
            L.call(entry, C.byref(g), _p(xg), _p(_w25(frame, dev)), _p(bg), _p(y), _stream())
        else:
            o = 2 - k // 2
            g = _conv_geom(L, n, h, w, c, c, c, k, 0)
            L.call(entry, C.byref(g), _p(xg), _p(_dw_weight(frame[:, :, o:o + k, o:o + k], dev)), _p(bg), _p(y), _stream())
        torch.cuda.synchronize()
        _tail(yf, (entry, k))
        outs.append(_nchw(y.cpu(), c))
    clean, dirty = outs
    assert bool(torch.isfinite(clean).all())
    r = k // 2
    holds = torch.zeros(n, c, h, w, dtype=torch.bool)
    holds[0, ch, :r + 1, :r + 1] = True      # windows that contain pixel (0, 0) of the poisoned plane
    assert bool((dirty[holds] == float('inf')).all()), 'the windows that hold the pixel'
    bad = (dirty != clean) & ~holds
    assert not bool(bad.any()), (entry, k, 'outputs changed by a pixel outside their window (n, c, y, x):', bad.nonzero()[:8].tolist())


# ================================================================================================ D: kernel alignment
def _ka_run(L, dev, case, Xg, Yg):
    n = case[0]
    dx_, dy_ = _ka_dims(case)
    px, py = gram_plan(n, dx_), gram_plan(n, dy_)
    nws = L.query('cat_ka_ws_bytes', n) // 4
    wsf, ws = _out((nws,), dev, SENTINEL)
    of, out = _out((1,), dev)
    L.call('cat_ka_fwd', _p(Xg), dx_, _p(Yg), dy_, n, _p(out), _p(ws), _stream())
    torch.cuda.synchronize()
    _tail(wsf, (case, 'ws'))
    _tail(of, (case, 'out'))
    wc = ws.cpu()
    head, used = 4 + 2 * n * n, (px['nb'] + py['nb']) * px['NN'] ** 2
    assert bool((wc[:head] != SENTINEL).all()), (case, 'sums and Gram matrices')
    assert bool((wc[head:head + used] != SENTINEL).all()), (case, 'a partial block that gram_plan promises was not written')
    assert bool((wc[head + used:] == SENTINEL).all()), (case, 'writes beyond (nbx + nby) * NN * NN partials')
    gout = torch.full((1,), KA_GOUT, device=dev)
    df, dX = _out((n, dx_), dev)
    L.call('cat_ka_bwd', _p(Xg), dx_, n, _p(gout), _p(ws), _p(dX), _stream())
    torch.cuda.synchronize()
    _tail(df, (case, 'dX'))
    return {'ka': out.cpu()[0], 'dX': dX.cpu()}


@pytest.mark.gpu
@pytest.mark.parametrize('case', KA_CASES, ids=lambda c: 'n%d-cx%d-cy%d-%dx%d' % c)
def test_ka_fwd_bwd_at_the_plan_edges(dev, case):
    L = _lib()
    n, cx, cy, h, w = case
    X, Y = _ka_inputs(case)
    want = _ka_ref(case, torch.float64)
    Xg, Yg = _in(X, dev), _in(Y, dev)
    got = _ka_run(L, dev, case, Xg, Yg)
    dv = abs(float(got['ka']) - float(want['ka']))
    MAXREL['D-value'] = max(MAXREL.get('D-value', 0.0), dv)
    print('D %s KA %.6f off by %.3g (largest so far %.3g)' % (case, float(want['ka']), dv, MAXREL['D-value']))
    if cs4(cx) != cx:
        lanes = got['dX'].view(n, h * w, cs4(cx))[..., cx:]
        assert bool((lanes == 0.0).all()), (case, 'padding lanes of dX')
    try:
        _cmp('D', case, {'dX': got['dX']}, {'dX': want['dX']}, KA_BARS)
    finally:
        assert dv < 1e-5, (case, dv)
    _same(got, _ka_run(L, dev, case, Xg, Yg), case)


@pytest.mark.gpu
def test_ka_refuses_more_rows_than_its_tiles_hold(dev):
    L = _lib()
    n = KA_MAXN + 1
    Xg = _in(torch.ones(n, 8), dev)
    wsf, ws = _out((L.query('cat_ka_ws_bytes', KA_MAXN) // 4,), dev, SENTINEL)
    of, out = _out((1,), dev, SENTINEL)
    assert L.query('cat_ka_fwd', _p(Xg), 8, _p(Xg), 8, n, _p(out), _p(ws), _stream()) != 0
    assert L.query('cat_ka_bwd', _p(Xg), 8, n, _p(out), _p(ws), _p(out), _stream()) != 0
    torch.cuda.synchronize()
    assert bool((wsf == SENTINEL).all()) and bool((of == SENTINEL).all())


# ================================================================================================ E: losses, channel sum, Adam, add_n
def _loss_run(L, dev, kind, m, c, ag, bg):
    """-> value, da [M, C] (padding lanes checked), the partial-sum workspace"""
    cs = cs4(c)
    t = LOSS_KINDS[kind][1]
    wsf, ws = _out((1024,), dev, SENTINEL)
    of, out = _out((1,), dev)
    L.call('cat_loss_fwd', kind, _p(ag), _p(bg), t, m, c, cs, _p(out), _p(ws), _stream())
    gout = torch.full((1,), LOSS_GOUT, device=dev)
    df, da = _out((m, cs), dev)
    L.call('cat_loss_bwd', kind, _p(ag), _p(bg), t, m, c, cs, _p(gout), _loss_scale(m, c), _p(da), _stream())
    torch.cuda.synchronize()
    for flat, what in ((wsf, 'ws'), (of, 'out'), (df, 'da')):
        _tail(flat, (kind, m, c, what))
    nb = loss_nb(m * cs // 4)
    wc = ws.cpu()
    assert bool((wc[:nb] != SENTINEL).all()) and bool((wc[nb:] == SENTINEL).all()), (kind, m, c, 'exactly nb partials', nb)
    dac = da.cpu()
    assert bool((dac[:, c:] == 0.0).all()), (kind, m, c, 'padding lanes of da')
    return {'value': out.cpu()[0], 'da': dac[:, :c]}


def _loss_dev_inputs(dev, kind, m, c):
    """the padding lanes of a and b hold the sentinel: they belong to no term"""
    a, b = _loss_inputs(kind, m, c)
    lanes = lambda t: None if t is None else _in(F.pad(t, (0, cs4(c) - c), value=SENTINEL), dev)
    return lanes(a), lanes(b)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', sorted(LOSS_KINDS))
def test_loss_kinds_against_closed_forms(dev, kind):
    L = _lib()
    m, c = LOSS_SMALL
    ag, bg = _loss_dev_inputs(dev, kind, m, c)
    got = _loss_run(L, dev, kind, m, c, ag, bg)
    _loss_cmp(('kind', kind, m, c), got, _loss_ref(kind, m, c, torch.float64))
    _same(got, _loss_run(L, dev, kind, m, c, ag, bg), kind)


@functools.lru_cache(maxsize=None)
def _ladder_ref(kind, m, c):
    return _loss_ref(kind, m, c, torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize('m,c', LOSS_LADDER)
def test_loss_size_ladder(dev, m, c):
    """kinds 0 and 5 over 2, 257 and 1024 partial blocks; the largest also through cat_loss_multi_fwd / _bwd, bit for bit"""
    L = _lib()
    cs = cs4(c)
    runs = {}
    for kind in (0, 5):
        ag, bg = _loss_dev_inputs(dev, kind, m, c)
        runs[kind] = (ag, bg, _loss_run(L, dev, kind, m, c, ag, bg))
        _loss_cmp(('kind', kind, m, c), runs[kind][2], _ladder_ref(kind, m, c))
    if (m, c) != LOSS_LADDER[-1]:
        return
    terms = (L.LossTerm * 2)()
    das = []
    for i, kind in enumerate((0, 5)):
        ag, bg, _ = runs[kind]
        das.append(_out((m, cs), dev))
        terms[i].a, terms[i].b, terms[i].da = ag.data_ptr(), bg.data_ptr(), das[i][1].data_ptr()
        terms[i].M, terms[i].kind, terms[i].C, terms[i].cs, terms[i].target, terms[i].scale = m, kind, c, cs, 0.0, _loss_scale(m, c)
    nws = L.query('cat_loss_multi_ws_bytes', terms, 2) // 4
    assert nws == 2 * 1024
    wsf, ws = _out((nws,), dev)
    of, out = _out((2,), dev)
    L.call('cat_loss_multi_fwd', terms, 2, _p(out), _p(ws), _stream())
    gouts = [torch.full((1,), LOSS_GOUT, device=dev) for _ in range(2)]
    L.call('cat_loss_multi_bwd', terms, 2, (C.c_void_p * 2)(*[t.data_ptr() for t in gouts]), _stream())
    torch.cuda.synchronize()
    _tail(wsf, 'multi ws')
    _tail(of, 'multi out')
    for i, kind in enumerate((0, 5)):
        _tail(das[i][0], 'multi da')
        assert float(out[i]) == float(runs[kind][2]['value']), (kind, 'cat_loss_multi_fwd differs from cat_loss_fwd')
        assert torch.equal(das[i][1].cpu()[:, :c], runs[kind][2]['da']), (kind, 'cat_loss_multi_bwd differs from cat_loss_bwd')
        assert bool((das[i][1][:, c:] == 0.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize('m,c', CHANSUM_CASES)
def test_channel_sum(dev, m, c):
    L = _lib()
    cs = cs4(c)
    x, pre = _chansum_inputs(m, c)
    xg = _in(F.pad(x, (0, cs - c), value=SENTINEL), dev)      # the padding lanes belong to no channel
    nws = L.query('cat_channel_sum_ws_bytes', m, cs) // 4
    got = {}
    for acc, key in ((0, 'sum'), (1, 'sum_acc')):
        wsf, ws = _out((nws,), dev)
        of, out = _out((c,), dev)
        if acc:
            out.copy_(pre.to(dev))
        L.call('cat_channel_sum', _p(xg), m, c, cs, _p(out), acc, _p(ws), _stream())
        torch.cuda.synchronize()
        _tail(wsf, (m, c, 'ws'))
        _tail(of, (m, c, key))
        got[key] = out.cpu()
    _cmp('E-chansum', (m, c), got, _chansum_ref(m, c, torch.float64))


@pytest.mark.gpu
@pytest.mark.parametrize('wd', ADAM_WDS)
@pytest.mark.parametrize('n', ADAM_NS)
def test_adam_host_and_device_entry_points(dev, n, wd):
    """three steps of cat_adam_step (hyper-parameters from the host) and cat_adam_step_dev (device block): bit for bit the same, the parameters 1e-6
    from float64; the moments are held to TOL only: the kernels form 1 - beta2 in float32, 1.3e-5 from the double's"""
    L = _lib()
    h = ADAM_HYPER
    p0, grads = _adam_inputs(n)
    res = []
    for entry in ('cat_adam_step', 'cat_adam_step_dev'):
        pf, p = _out((n,), dev)
        p.copy_(p0.to(dev))
        mf, m = _out((n,), dev, 0.0)
        vf, v = _out((n,), dev, 0.0)
        hf, hyper = _out((8,), dev)
        hyper.copy_(torch.tensor([h['lr'], h['b1'], h['b2'], h['eps'], wd, 0.0, NAN, NAN]))
        for step, g in enumerate(grads, 1):
            gg = _in(g, dev)
            if entry == 'cat_adam_step':
                L.call(entry, _p(p), _p(gg), _p(m), _p(v), n, h['lr'], h['b1'], h['b2'], h['eps'], wd, step, h['gscale'], _stream())
            else:
                L.call(entry, _p(p), _p(gg), _p(m), _p(v), n, _p(hyper), h['gscale'], _stream())
            torch.cuda.synchronize()
        for flat in (pf, mf, vf, hf):
            _tail(flat, (entry, n, wd))
        if entry == 'cat_adam_step_dev':
            assert float(hyper[5]) == float(h['steps'])
        res.append({'p': p.cpu(), 'm': m.cpu(), 'v': v.cpu()})
    _same(res[0], res[1], ('host against device entry point', n, wd))
    _cmp('E-adam', (n, wd), res[0], _adam_ref(n, wd, torch.float64), {'p': ADAM_BAR})


@pytest.mark.gpu
@pytest.mark.parametrize('nsrc,n', [(k, ADDN_SMALL) for k in range(1, 9)] + [(2, ADDN_LARGE)], ids=lambda v: str(v))
def test_add_n(dev, nsrc, n):
    L = _lib()
    srcs = [_in(t, dev) for t in _addn_inputs(nsrc, n)]
    of, out = _out((n,), dev)
    L.call('cat_add_n', (C.c_void_p * nsrc)(*[t.data_ptr() for t in srcs]), nsrc, _p(out), n, _stream())
    torch.cuda.synchronize()
    _tail(of, (nsrc, n))
    _cmp('E-addn', (nsrc, n), {'sum': out.cpu()}, _addn_ref(nsrc, n, torch.float64), {'sum': ADDN_BAR})
