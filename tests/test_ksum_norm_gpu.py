"""GPU parity of the normalising, statistics-writing wide-tile convolution sum (csrc/conv_ksum.hip, cat_conv2d_ksum_norm_fwd through ctypes):

    y[m][co] = bias[co] + sum_s sum_taps sum_c f_s(src_s[pixel(m, tap)][c]) * w_s[co][tap][c],   f_s(v) = act_s(v * scale_s[n][c] + shift_s[n][c])

+ the per-tile statistics of y for the norm behind it -- stage 2 of a wide eval-mode InstanceNorm block (reference
models/modules/inception_modules.py:230-236 with the InstanceNorm2d of models/networks.py:41-44 in front of every second conv) -- against a
float64 reference from F.conv2d, reflect F.pad and the affine + activation.  Output bar: tests/test_ksum_gpu.py's, 1e-4 of the output's range.
Statistics bar: the one tests/test_fused_kernels_gpu.py applies to cat_tconv_fwd's table and to cat_tnorm_finalize* (rel() < 1e-4 per tensor),
on the raw table and again after cat_tnorm_finalize2 on the kernel's lattice."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4
EPS = 1e-5
NONE, RELU, LRELU = 0, 1, 2
NAN = float('nan')


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


# name -> (N, H, W, [(channels, k, normalised, act, slope)], Cout, bias, statistics, one table row for the batch, extra output lanes)
CASES = {
    # each sample is exactly one 128-pixel row tile: a kernel that reads sample 0's table for sample 1 fails
    'teacher-tail': (2, 8, 16, [(44, 1, 1, RELU, 0.0), (132, 1, 1, RELU, 0.0), (44, 3, 1, RELU, 0.0), (44, 5, 1, RELU, 0.0)], 256, True, True, False, 0),
    # the first 1 x 1 group of the block: no staging function, statistics only, two 96-wide N tiles, th 4 x tw 32
    'stage1': (3, 16, 32, [(256, 1, 0, NONE, 0.0)], 176, False, True, False, 0),
    # ragged 128-wide N tile; the flat walk (11 quads per tap: a chunk straddles a tap boundary), one tap per chunk (3 quads), scale NULL
    'mixed': (2, 16, 16, [(44, 3, 1, LRELU, 0.2), (12, 3, 1, RELU, 0.0), (20, 1, 0, NONE, 0.0)], 72, True, True, False, 8),
    'w128': (2, 2, 128, [(44, 3, 1, RELU, 0.0), (20, 1, 1, LRELU, 0.1)], 64, True, True, False, 0),
    'one-row': (2, 8, 16, [(44, 1, 1, RELU, 0.0), (44, 3, 1, RELU, 0.0)], 128, True, True, True, 0),
}


def _inputs(name):
    n, h, w, segs, cout, has_bias, _, one_row, _ = CASES[name]
    g = torch.Generator().manual_seed(4321 + sorted(CASES).index(name))
    G = 1 if one_row else n
    xs = [torch.randn(n, c, h, w, generator=g) for c, *_ in segs]
    ws = [torch.randn(cout, c, k, k, generator=g) / (c * k * k) ** 0.5 for c, k, *_ in segs]
    tabs = [(0.5 + torch.rand(G, c, generator=g), torch.randn(G, c, generator=g)) if nrm else None for c, _, nrm, *_ in segs]
    bias = torch.randn(cout, generator=g) if has_bias else None
    return xs, ws, tabs, bias


def _f(x, tab, act, slope, dt):
    if tab is None:
        return x.to(dt)
    sc, sh = (t.to(dt).expand(x.shape[0], -1)[:, :, None, None] for t in tab)
    v = x.to(dt) * sc + sh
    return {NONE: v, RELU: F.relu(v), LRELU: F.leaky_relu(v, slope)}[act]


def _ref(xs, ws, tabs, bias, segs, reflect=True, dt=torch.float64):
    y = None
    for x, wt, tab, (c, k, nrm, act, slope) in zip(xs, ws, tabs, segs):
        a, p = _f(x, tab, act, slope, dt), k // 2
        if p and reflect:
            t = F.conv2d(F.pad(a, (p,) * 4, mode='reflect'), wt.to(dt))
        else:
            t = F.conv2d(a, wt.to(dt), None, 1, p)
        y = t if y is None else y + t
    return y if bias is None else y + bias.to(dt).view(1, -1, 1, 1)


def _tile_stats(y, th, tw):
    """sum and squared deviations from the tile mean over th x tw lattice tiles (ragged tiles: their true pixel count), row-major per image"""
    n, c, h, w = y.shape
    ty, tx = -(-h // th), -(-w // tw)
    yp = F.pad(y, (0, tx * tw - w, 0, ty * th - h)).view(n, c, ty, th, tx, tw)
    mk = F.pad(torch.ones(h, w, dtype=y.dtype), (0, tx * tw - w, 0, ty * th - h)).view(ty, th, tx, tw)
    s = yp.sum((3, 5))
    d = (yp - (s / mk.sum((1, 3)))[:, :, :, None, :, None]) * mk
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(n * ty * tx, c)
    return flat(s), flat((d * d).sum((3, 5)))


def _instance_ref(y, gamma, beta):
    mean = y.mean((2, 3))
    var = ((y - mean[:, :, None, None]) ** 2).mean((2, 3))
    rstd = (var + EPS) ** -0.5
    scale = gamma.double() * rstd
    return {'scale': scale, 'shift': beta.double() - mean * scale, 'mean': mean, 'rstd': rstd}


def _device_segments(dev, xs, ws, tabs, segs, reflect=True):
    """-> (ksum.NormSegment list, tensors to keep alive).  Tables: [G][cs_for(c)] rows with zeros in the padding channels."""
    from cat_amd import ksum, ops
    out, keep = [], []
    for x, wt, tab, (c, k, nrm, act, slope) in zip(xs, ws, tabs, segs):
        wd = ops.padded_weight_like(tuple(wt.shape), dev)
        wd.copy_(wt.to(dev))
        kw = {}
        if tab is not None:
            G, c4 = tab[0].shape[0], ops.cs_for(c)
            sc, sh = torch.zeros(G, c4), torch.zeros(G, c4)
            sc[:, :c], sh[:, :c] = tab[0], tab[1]
            sc, sh = sc.to(dev), sh.to(dev)
            keep += [sc, sh]
            kw = dict(scale=sc, shift=sh, sstride=c4 if G > 1 else 0, act=act, slope=slope)
        out.append(ksum.NormSegment(ops.to_nhwc(x.to(dev)), wd, reflect and k > 1, **kw))
        keep.append(wd)
    return out, keep


def _finalize(dev, part, n, h, w, th, tw, cout, scs, gamma, beta):
    from cat_amd import _lib as L, ops
    sl = (L.NSlice * 1)()
    sl[0].c0, sl[0].c = 0, cout
    rows = [torch.full((n, scs), NAN, device=dev) for _ in range(4)]
    gg, bg = gamma.to(dev), beta.to(dev)
    L.call('cat_tnorm_finalize2', ops._p(part), scs, n, n, h, w, th, tw, 1, ops._p(gg), ops._p(bg), 1, sl, EPS, 0.1, *[ops._p(r) for r in rows], scs,
           ops._stream())
    torch.cuda.synchronize()
    return {k: r.cpu()[:, :cout] for k, r in zip(('scale', 'shift', 'mean', 'rstd'), rows)}


def _check(what, got, want):
    bad = []
    for key in sorted(want):
        assert bool(torch.isfinite(got[key].double()).all()), (what, key)
        d = rel(got[key], want[key])
        print('%s %s rel %.3g' % (what, key, d))      # every figure is printed before the first one fails the case
        if not d < TOL:
            bad.append((key, d))
    assert not bad, (what, bad)


@pytest.mark.parametrize('name', sorted(CASES))
def test_ksum_norm_matches_float64(dev, name):
    from cat_amd import _lib as L, ksum, ops
    n, h, w, segs, cout, _, stats, _, extra = CASES[name]
    xs, ws, tabs, bias = _inputs(name)
    want = _ref(xs, ws, tabs, bias, segs)
    ks, keep = _device_segments(dev, xs, ws, tabs, segs)
    th, tw = ksum.lattice(h, w)
    cs = ops.cs_for(cout) + extra
    tiles = n * h * w // 128
    bd = None if bias is None else bias.to(dev)
    old = ksum.set_min_workgroups(1)
    try:
        assert ksum.norm_applicable(ks, n, h, w, cout)
    finally:
        ksum.set_min_workgroups(old)
    runs = []
    for _ in range(2):
        y = ops.empty_act(n, cout, h, w, dev, cs=cs)
        raw = torch.as_strided(y, (n, h, w, cs), (h * w * cs, w * cs, cs, 1))
        raw.fill_(NAN)      # every owned element must be written; padding lanes must come out as exact zeros
        part = torch.full((tiles, 2, cs), NAN, device=dev)
        g, keep_w = ksum._geom(ks, n, h, w, cout, cs, cs, 0, L.ACT_NONE, 0.0)
        nm = ksum._norm_geom(ks, part if stats else None, cs)
        assert L.query('cat_conv2d_ksum_norm_supported', C.byref(g), C.byref(nm)) == 1
        L.call('cat_conv2d_ksum_norm_fwd', C.byref(g), C.byref(nm), ops._p(bd), None, ops._p(y), ops._stream())
        torch.cuda.synchronize()
        runs.append((raw.cpu(), part.cpu()))
    (raw, part), (raw2, part2) = runs
    assert torch.equal(raw, raw2) and torch.equal(part, part2), 'two launches are bitwise equal'
    assert not torch.isnan(raw).any() and not torch.isnan(part).any()
    if cs > cout:
        assert float(raw[..., cout:].abs().max()) == 0.0 and float(part[..., cout:].abs().max()) == 0.0
    got = {'y': raw[..., :cout].permute(0, 3, 1, 2)}
    ref = {'y': want}
    ref['sum'], ref['m2'] = _tile_stats(want, th, tw)
    got['sum'], got['m2'] = part[:, 0, :cout], part[:, 1, :cout]
    _check(name, got, ref)
    g2 = torch.Generator().manual_seed(5)
    gamma, beta = 0.5 + torch.rand(cs, generator=g2), torch.randn(cs, generator=g2)
    fin = _finalize(dev, part.to(dev), n, h, w, th, tw, cout, cs, gamma, beta)
    _check(name + ' finalize2', fin, _instance_ref(want, gamma[:cout], beta[:cout]))


# name -> (N, H, W, segments, Cout, reflect, epilogue activation): outside the kernel's domain
DECLINES = {
    'plane-12x12': (2, 12, 12, [(44, 3, 1, RELU, 0.0), (20, 1, 1, RELU, 0.0)], 64, True, NONE),
    'plane-8x24': (2, 8, 24, [(44, 3, 1, RELU, 0.0), (20, 1, 1, RELU, 0.0)], 64, True, NONE),        # 128 % 24 != 0
    'zero-padding': (2, 8, 16, [(44, 3, 1, RELU, 0.0), (20, 1, 1, RELU, 0.0)], 64, False, NONE),     # f(0) != 0: the zero border is no source value
    'stats-with-act': (2, 8, 16, [(44, 3, 1, RELU, 0.0), (20, 1, 1, RELU, 0.0)], 64, True, RELU),
}


@pytest.mark.parametrize('name', sorted(DECLINES))
def test_outside_the_domain_the_wrapper_takes_the_lds_tile_kernel(dev, name):
    from cat_amd import _lib as L, ksum, ops
    n, h, w, segs, cout, reflect, act = DECLINES[name]
    g = torch.Generator().manual_seed(99 + sorted(DECLINES).index(name))
    xs = [torch.randn(n, c, h, w, generator=g) for c, *_ in segs]
    ws = [torch.randn(cout, c, k, k, generator=g) / (c * k * k) ** 0.5 for c, k, *_ in segs]
    tabs = [(0.5 + torch.rand(n, c, generator=g), torch.randn(n, c, generator=g)) for c, *_ in segs]
    bias = torch.randn(cout, generator=g)
    want = _ref(xs, ws, tabs, bias, segs, reflect)
    ks, keep = _device_segments(dev, xs, ws, tabs, segs, reflect)
    cs = ops.cs_for(cout)
    kg, keep_w = ksum._geom(ks, n, h, w, cout, cs, cs, 0, act, 0.0)
    nm = ksum._norm_geom(ks, 16, cs)
    assert L.query('cat_conv2d_ksum_supported', C.byref(kg)) == 1, 'the plain sum takes this geometry'
    assert L.query('cat_conv2d_ksum_norm_supported', C.byref(kg), C.byref(nm)) == 0
    old = ksum.set_min_workgroups(1)
    try:
        assert not ksum.norm_applicable(ks, n, h, w, cout, True, act)
        y = ops.empty_act(n, cout, h, w, dev)
        y.fill_(NAN)
        part, th, tw = ksum.run_norm(ks, bias.to(dev), y, act=act)
    finally:
        ksum.set_min_workgroups(old)
    torch.cuda.synchronize()
    assert (th, tw) == (8, 16)
    got = {'y': y.cpu()}
    ref = {'y': F.relu(want) if act == RELU else want}
    ref['sum'], ref['m2'] = _tile_stats(want, th, tw)      # (statistics of the sum in front of the epilogue activation)
    got['sum'], got['m2'] = part.cpu()[:, 0, :cout], part.cpu()[:, 1, :cout]
    _check(name, got, ref)
    gamma, beta = torch.ones(cs), torch.zeros(cs)
    fin = _finalize(dev, part, n, h, w, th, tw, cout, cs, gamma, beta)
    _check(name + ' finalize2', fin, _instance_ref(want, gamma[:cout], beta[:cout]))
