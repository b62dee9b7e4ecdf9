"""GPU: the kernels behind the cityscapes mIoU one by one against float64 ATen / numpy references.

A: cat_conv2d_fwd_ex -- dilation {1, 2, 4} x kernel {1, 3, 7} over every dispatch path of the entry point (direct-to-LDS 128 x 128 tile,
   BK = 32 register-staged tiles, the generic ragged-channel tiles, small-M and full-M tiles), with / without bias, activation, residual,
   residual and output as channel slices, against F.conv2d(dilation=) in float64 at 1e-3; dilation 1 without residual == cat_conv2d_fwd.
B: cat_seg_up_logsoftmax against F.conv_transpose2d(groups=C) + log_softmax in float64.
C: cat_seg_confusion against a numpy restatement on inputs whose float32 arithmetic is exact: exact equality, ties included."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_conv_variants_gpu import _padded_weight, _profiled
from test_kernels_gpu import rel

pytestmark = pytest.mark.gpu
SENTINEL = 7.0
CONV_TOL = 1e-3


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _act64(y, act):
    return {0: y, 1: F.relu(y), 2: F.leaky_relu(y, 0.2), 3: torch.tanh(y)}[act]


def _wide(n, c, h, w, dev, extra, fill):
    """An NHWC buffer with `extra` more channels in front of and behind a [c0, c0 + c) slice; returns (full logical view, c0)."""
    from cat_amd import ops
    c0 = extra
    buf = ops.empty_act(n, c0 + c + extra, h, w, dev)
    torch.as_strided(buf, (n, ops.act_cs(buf), h, w), buf.stride()).fill_(fill)
    return buf, c0


# (cin, cout, k, stride, dil, pad, act, bias, res, yslice, N, H, W, profile family the dispatch must take)
# res: 0 none, 1 a tensor of its own, 2 a channel slice of a wider buffer.  pad None = dil * (k - 1) / 2 ('same').
EX_CASES = [
    # direct-to-LDS 128 x 128 x 32 tile: Cin % 32 == 0, Cout > 96
    (64, 256, 3, 1, 2, None, 1, 1, 0, 0, 1, 23, 37, 'conv_fwd32d_4x4x2x2'),
    (512, 256, 3, 1, 4, None, 1, 1, 1, 0, 1, 23, 37, 'conv_fwd32d_4x4x2x2'),
    (256, 1024, 1, 1, 1, None, 1, 1, 2, 0, 2, 23, 37, 'conv_fwd32d_4x4x2x2'),      # the last 1 x 1 of a bottleneck: relu(conv + bias + res)
    (256, 1024, 1, 1, 2, None, 0, 0, 1, 1, 1, 9, 11, 'conv_fwd32d_4x4x2x2'),
    (64, 256, 7, 1, 4, None, 1, 1, 0, 0, 1, 23, 37, 'conv_fwd32d_4x4x2x2'),
    (64, 256, 3, 1, 4, None, 1, 1, 1, 0, 2, 3, 5, 'conv_fwd32d_4x4x2x2'),           # plane smaller than the dilation: only the centre tap is inside
    (64, 256, 3, 2, 1, 1, 1, 1, 1, 0, 1, 23, 37, 'conv_fwd32d_4x4x2x2'),            # stride 2 at dilation 1
    # BK = 32 register-staged tiles: per-tap extent a multiple of 16, Cout <= 96 (or Cin % 32 != 0)
    (64, 64, 3, 1, 2, None, 1, 1, 1, 0, 1, 23, 37, 'conv_fwd32_2x4x4x1'),
    (16, 16, 3, 1, 4, None, 1, 1, 2, 1, 1, 23, 37, 'conv_fwd32_2x1x4x1'),           # small-M tile of the 16-wide row
    (16, 16, 3, 1, 2, None, 1, 1, 1, 0, 1, 448, 448, 'conv_fwd32_4x1x4x1'),         # full-M tile (>= 768 tiles of 256 rows)
    (44, 19, 7, 1, 2, None, 0, 1, 1, 0, 1, 23, 37, 'conv_fwd32_2x2x4x1'),           # 44 -> tap extent 48 (zero-filled quads), ragged Cout
    (512, 19, 1, 1, 4, None, 0, 1, 0, 0, 2, 23, 37, 'conv_fwd32_2x2x4x1'),          # the classifier's shape at an idle dilation
    (16, 32, 3, 2, 1, 1, 1, 0, 2, 0, 1, 23, 37, 'conv_fwd32_2x2x4x1'),
    (48, 256, 3, 1, 2, None, 3, 1, 1, 1, 1, 23, 37, 'conv_fwd32_4x4x2x2'),
    # generic tiles (BK = 16, per-lane tap walk): ragged channel counts
    (3, 16, 7, 1, 1, None, 1, 1, 1, 0, 1, 23, 37, 'conv_fwd_2x1x4x1'),              # the stem's shape, with a residual
    (3, 16, 7, 1, 2, None, 1, 1, 0, 0, 1, 23, 37, 'conv_fwd_2x1x4x1'),
    (3, 64, 3, 1, 4, None, 2, 1, 2, 0, 2, 23, 37, 'conv_fwd_2x4x4x1'),
    (3, 1024, 1, 1, 2, None, 0, 1, 1, 0, 1, 9, 11, 'conv_fwd_4x4x2x2'),
    (3, 19, 3, 1, 4, None, 1, 0, 1, 0, 1, 3, 5, 'conv_fwd_2x2x4x1'),
    (6, 16, 3, 1, 2, None, 1, 1, 1, 0, 1, 448, 448, 'conv_fwd_4x1x4x1'),
]


def _run_ex(case, dev):
    from cat_amd import _lib as L, ops
    cin, cout, k, stride, dil, pad, act, bias, res, yslice, n, h, w, _ = case
    pad = dil * (k - 1) // 2 if pad is None else pad
    x = detfill.normal((n, cin, h, w), 1)
    wt = detfill.normal((cout, cin, k, k), 2, 1.0 / np.sqrt(cin * k * k))
    b = detfill.normal((cout,), 3, 0.1) if bias else None
    ho, wo = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    r = detfill.normal((n, cout, ho, wo), 5) if res else None
    want = F.conv2d(x.double(), wt.double(), b.double() if bias else None, stride, pad, dil)
    want = _act64(want + (r.double() if res else 0.0), act)
    xg, wg = ops.to_nhwc(x.to(dev)), _padded_weight(wt, dev)
    bg = b.to(dev) if bias else None
    rbuf, rc0 = None, 0
    if res == 1:
        rbuf = ops.to_nhwc(r.to(dev))
    elif res == 2:
        rbuf, rc0 = _wide(n, cout, ho, wo, dev, 8, float('nan'))
        rbuf[:, rc0:rc0 + cout].copy_(r.to(dev))
    if yslice:
        ybuf, c0 = _wide(n, cout, ho, wo, dev, 4, SENTINEL)
        ycw = cout
    else:
        ybuf, c0 = ops.empty_act(n, cout, ho, wo, dev), 0
        torch.as_strided(ybuf, (n, ops.act_cs(ybuf), ho, wo), ybuf.stride()).fill_(SENTINEL)
        ycw = ops.act_cs(ybuf)
    g = ops._conv_geom(n, h, w, cin, ops.act_cs(xg), ho, wo, cout, ops.act_cs(ybuf), k, k, stride, pad, L.PAD_ZERO, act, 0.2, ycw=ycw,
                       wcs=ops.weight_wcs(wg))
    rp = C.c_void_p(rbuf.data_ptr() + 4 * rc0) if rbuf is not None else None
    L.call('cat_conv2d_fwd_ex', C.byref(g), dil, ops._p(xg), ops._p(wg), ops._p(bg), rp, ops.act_cs(rbuf) if rbuf is not None else 0,
           C.c_void_p(ybuf.data_ptr() + 4 * c0), ops._stream())
    full = torch.as_strided(ybuf, (n, ops.act_cs(ybuf), ho, wo), ybuf.stride())
    return want, ybuf, full, c0


@pytest.mark.parametrize('case', EX_CASES, ids=lambda c: 'cin%d_cout%d_k%d_s%d_d%d_a%d_b%d_r%d_y%d_%dx%dx%d_%s' % (c[:5] + c[6:]))
def test_conv_ex_against_float64(dev, case):
    cin, cout = case[0], case[1]
    (want, ybuf, full, c0), fam = _profiled(lambda: _run_ex(case, dev))
    assert fam.get(case[-1], 0) == 1 and sum(v for k, v in fam.items() if k.startswith('conv_')) == 1, fam      # the dispatch path under test
    got = full[:, c0:c0 + cout]
    err = rel(got, want)
    print('conv_ex %s: rel err %.2e' % (case, err))
    assert err <= CONV_TOL
    if case[9]:      # output slice: the neighbouring channels are untouched
        assert bool((full[:, :c0] == SENTINEL).all()) and bool((full[:, c0 + cout:] == SENTINEL).all())
    else:            # padding channels of y stay 0
        assert bool((full[:, cout:] == 0).all())


def test_ex_case_table_spans_the_issue_grid():
    """dilation {1, 2, 4} x kernel {1, 3, 7}, the channel counts, a ragged plane, a plane smaller than the dilation, stride 2 at dilation 1."""
    assert {(c[4], c[2]) for c in EX_CASES} >= {(d, k) for d in (1, 2, 4) for k in (1, 3, 7)}
    assert {c[0] for c in EX_CASES} >= {3, 16, 44, 64, 256, 512} and {c[1] for c in EX_CASES} >= {16, 19, 64, 256, 1024}
    assert any(c[3] == 2 and c[4] == 1 for c in EX_CASES) and any((c[11], c[12]) == (3, 5) and c[4] == 4 for c in EX_CASES)
    assert {c[-1].split('_')[1] for c in EX_CASES} == {'fwd32d', 'fwd32', 'fwd'}


@pytest.mark.parametrize('shape', [(64, 256, 3, 1, 9, 11), (64, 64, 3, 1, 23, 37), (3, 64, 7, 1, 23, 37)], ids=['direct', 'bk32', 'generic'])
def test_conv_ex_plain_is_bit_identical_to_conv2d_fwd(dev, shape):
    """dilation 1, res NULL: the same bits as cat_conv2d_fwd; and with an all-zero residual through the EX kernels, the same bits again
    (acc + bias + 0 before the ReLU)."""
    from cat_amd import _lib as L, ops
    cin, cout, k, n, h, w = shape
    x, wt, b = detfill.normal((n, cin, h, w), 1), detfill.normal((cout, cin, k, k), 2, 1.0 / np.sqrt(cin * k * k)), detfill.normal((cout,), 3, 0.1)
    xg, wg, bg = ops.to_nhwc(x.to(dev)), _padded_weight(wt, dev), b.to(dev)
    outs = []
    for mode in ('fwd', 'ex', 'ex_zero_res'):
        y = ops.empty_act(n, cout, h, w, dev)
        y.fill_(SENTINEL)
        g = ops._conv_geom(n, h, w, cin, ops.act_cs(xg), h, w, cout, ops.act_cs(y), k, k, 1, k // 2, L.PAD_ZERO, L.ACT_RELU, 0.0, ycw=ops.act_cs(y),
                           wcs=ops.weight_wcs(wg))
        if mode == 'fwd':
            L.call('cat_conv2d_fwd', C.byref(g), ops._p(xg), ops._p(wg), ops._p(bg), ops._p(y), ops._stream())
        else:
            z = ops.to_nhwc(torch.zeros(n, cout, h, w, device=dev)) if mode == 'ex_zero_res' else None
            L.call('cat_conv2d_fwd_ex', C.byref(g), 1, ops._p(xg), ops._p(wg), ops._p(bg), ops._p(z), ops.act_cs(z) if z is not None else 0, ops._p(y),
                   ops._stream())
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])
    assert rel(outs[0], F.relu(F.conv2d(x.double(), wt.double(), b.double(), 1, k // 2))) <= CONV_TOL


def test_conv_ex_rejects_what_it_does_not_compute(dev):
    from cat_amd import _lib as L, ops
    x = ops.to_nhwc(torch.zeros(1, 16, 8, 8, device=dev))
    wg = _padded_weight(torch.zeros(16, 16, 3, 3), dev)
    y = ops.empty_act(1, 16, 4, 4, dev)
    g = ops._conv_geom(1, 8, 8, 16, 16, 4, 4, 16, 16, 3, 3, 2, 2, L.PAD_ZERO, 0, 0.0, ycw=16, wcs=16)
    with pytest.raises(RuntimeError, match='stride 1'):
        L.call('cat_conv2d_fwd_ex', C.byref(g), 2, ops._p(x), ops._p(wg), None, None, 0, ops._p(y), ops._stream())
    g = ops._conv_geom(1, 8, 8, 16, 16, 8, 8, 16, 16, 3, 3, 1, 1, L.PAD_ZERO, 0, 0.0, ycw=16, wcs=16)      # 'same' size of dilation 1, not of 2
    y = ops.empty_act(1, 16, 8, 8, dev)
    with pytest.raises(RuntimeError, match='output size'):
        L.call('cat_conv2d_fwd_ex', C.byref(g), 2, ops._p(x), ops._p(wg), None, None, 0, ops._p(y), ops._stream())


# ------------------------------------------------------------------------------------------------ B: up-sampling + log-softmax
# Bound: every up-sampled value is a sum of <= 4 float32 products (relative error <= 4 * 2^-24 of the largest term), the log-softmax adds
# <= C + 2 roundings and two library calls of <= 2 ulp: <= ~40 * 2^-24 = 2.4e-6 of the largest magnitude.  1e-5 leaves a factor of four.
UP_TOL = 1e-5


@pytest.mark.parametrize('c,n,h,w,bilinear', [(19, 2, 16, 32, False), (19, 1, 5, 7, True), (5, 2, 5, 7, False), (21, 1, 6, 3, True), (19, 1, 1, 2, False)],
                         ids=['c19_random', 'c19_bilinear_ragged', 'c5_random_ragged', 'c21_bilinear', 'c19_single_row'])
def test_seg_up_logsoftmax(dev, c, n, h, w, bilinear):
    from cat_amd import _lib as L, ops
    from cat_amd.metric.drn import bilinear_up_weights
    x = detfill.normal((n, c, h, w), 11, 5.0)
    wt = bilinear_up_weights(c, 16) if bilinear else detfill.normal((c, 1, 16, 16), 12, 0.3)
    want = F.log_softmax(F.conv_transpose2d(x.double(), wt.double(), None, stride=8, padding=4, groups=c), dim=1)
    xg = ops.to_nhwc(x.to(dev))
    cs = ops.act_cs(xg)
    xfull = torch.as_strided(xg, (n, cs, h, w), xg.stride())
    if cs > c:
        xfull[:, c:] = float('nan')      # the padding channel poisoned beforehand: it must not enter the softmax
    y = ops.empty_act(n, c, h * 8, w * 8, dev)
    yfull = torch.as_strided(y, (n, ops.act_cs(y), h * 8, w * 8), y.stride())
    yfull.fill_(float('nan'))
    L.call('cat_seg_up_logsoftmax', ops._p(xg), cs, n, h, w, c, ops._p(wt.to(dev).contiguous()), 8, ops._p(y), ops.act_cs(y), ops._stream())
    assert tuple(want.shape) == tuple(y.shape)
    err = rel(y, want)
    print('seg_up_logsoftmax c=%d %dx%dx%d: rel err %.2e' % (c, n, h, w, err))
    assert err <= UP_TOL
    assert bool((yfull[:, c:] == 0).all())
    assert float((y.double().exp().sum(1) - 1).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ C: resize + argmax + confusion matrix
def _np_resize(lp, hl, wl, scale32=False):
    """float64 numpy restatement of the half-pixel, clamped-edge bilinear resize (F.interpolate(align_corners=False)); scale32: the
    in / out ratio rounded to float32 first, as a float32 tensor's interpolation defines it."""
    n, c, h, w = lp.shape
    if (h, w) == (hl, wl):
        return lp.astype(np.float64)

    def axis(inn, out):
        s = float(np.float32(inn) / np.float32(out)) if scale32 else inn / out
        src = np.maximum(s * (np.arange(out) + 0.5) - 0.5, 0.0)
        i0 = np.minimum(np.floor(src).astype(np.int64), inn - 1)
        i1 = np.minimum(i0 + 1, inn - 1)
        l1 = src - i0
        return i0, i1, l1, 1.0 - l1
    y0, y1, ly1, ly0 = axis(h, hl)
    x0, x1, lx1, lx0 = axis(w, wl)
    v = lp.astype(np.float64)
    top = lx0 * v[:, :, y0][:, :, :, x0] + lx1 * v[:, :, y0][:, :, :, x1]
    bot = lx0 * v[:, :, y1][:, :, :, x0] + lx1 * v[:, :, y1][:, :, :, x1]
    return ly0[:, None] * top + ly1[:, None] * bot


def _np_hist(pred, label, ncls):
    k = (label >= 0) & (label < ncls)
    return np.bincount(ncls * label[k].astype(int) + pred[k], minlength=ncls ** 2).reshape(ncls, ncls)


def _gpu_confusion(lp, label, ncls, dev, hist=None, want_pred=True):
    from cat_amd import ops
    from cat_amd.metric import miou
    lg = ops.to_nhwc(torch.from_numpy(lp).float().to(dev))
    cs = ops.act_cs(lg)
    if cs > lp.shape[1]:
        torch.as_strided(lg, (lp.shape[0], cs) + lp.shape[2:], lg.stride())[:, lp.shape[1]:] = 1e30      # a padding channel must never win
    lab = torch.from_numpy(label).to(dev)
    hist = torch.zeros((ncls, ncls), dtype=torch.int64, device=dev) if hist is None else hist
    pred = torch.full_like(lab, 200) if want_pred else None
    miou.confusion(lg, lab, hist, ncls, pred)
    return hist, (pred.cpu().numpy() if want_pred else None)


def _labels(shape, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, ncls + 3, size=shape)      # ncls .. ncls + 2: values >= n, never counted
    lab[rng.random(shape) < 0.1] = 255
    return lab.astype(np.uint8)


@pytest.mark.parametrize('c,n,h,w,up', [(19, 2, 16, 32, 8), (19, 1, 5, 7, 8), (5, 2, 6, 3, 8), (19, 2, 24, 40, 1)],
                         ids=['c19_x8', 'c19_x8_ragged', 'c5_x8', 'c19_no_resize'])
def test_seg_confusion_exact(dev, c, n, h, w, up):
    """Small-integer log-probabilities and x8 enlargement: the bilinear weights are k / 16, every product and sum is exact in float32, so
    pred and hist must EQUAL the numpy restatement, ties (plenty, by construction) going to the lowest index."""
    rng = np.random.default_rng(100 + c + h)
    lp = rng.integers(-3, 1, size=(n, c, h, w)).astype(np.float32)
    hl, wl = h * up, w * up
    label = _labels((n, hl, wl), c, 7)
    big = _np_resize(lp, hl, wl)
    assert np.array_equal(big, big.astype(np.float32).astype(np.float64))      # exact in float32
    want_pred = big.argmax(axis=1)
    srt = np.sort(big, axis=1)
    assert (srt[:, -1] == srt[:, -2]).mean() > 0.05                            # ties are really there
    hist, pred = _gpu_confusion(lp, label, c, dev)
    assert np.array_equal(pred, want_pred.astype(np.uint8))
    assert np.array_equal(hist.cpu().numpy(), _np_hist(want_pred.flatten(), label.flatten(), c))
    assert int(hist.sum()) == int((label < c).sum()) and 0 < int((label >= c).sum())
    # a second call accumulates into the same matrix; pred is optional
    hist2, _ = _gpu_confusion(lp, label, c, dev, hist=hist, want_pred=False)
    assert np.array_equal(hist2.cpu().numpy(), 2 * _np_hist(want_pred.flatten(), label.flatten(), c))


def test_seg_confusion_more_classes_than_channels(dev):
    """n_classes > C (labels up to n - 1 counted, predictions below C): the matrix is n x n."""
    rng = np.random.default_rng(5)
    lp = rng.integers(-3, 1, size=(1, 5, 4, 4)).astype(np.float32)
    label = rng.integers(0, 9, size=(1, 32, 32)).astype(np.uint8)
    want = _np_resize(lp, 32, 32).argmax(axis=1)
    hist, pred = _gpu_confusion(lp, label, 7, dev)
    assert np.array_equal(pred, want.astype(np.uint8)) and np.array_equal(hist.cpu().numpy(), _np_hist(want.flatten(), label.flatten(), 7))


def test_seg_confusion_general_ratio(dev):
    """24 x 40 -> 100 x 90 (neither ratio a power of two: the source coordinates are not exact in float32) against float64.  Pixels
    whose float64 top-2 margin is below 1e-5 are exempt; the inputs (0.25 * N(0, 1), 19 classes) keep that share far below the 1 % cap."""
    c, n, h, w, hl, wl = 19, 2, 24, 40, 100, 90
    lp = (0.25 * np.random.default_rng(9).standard_normal((n, c, h, w))).astype(np.float32)
    label = _labels((n, hl, wl), c, 8)
    big = _np_resize(lp, hl, wl, scale32=True)
    srt = np.sort(big, axis=1)
    exempt = (srt[:, -1] - srt[:, -2]) < 1e-5
    assert exempt.mean() <= 0.01
    want = big.argmax(axis=1)
    hist, pred = _gpu_confusion(lp, label, c, dev)
    assert np.array_equal(pred[~exempt], want.astype(np.uint8)[~exempt])
    diff = np.abs(hist.cpu().numpy() - _np_hist(want.flatten(), label.flatten(), c)).sum()
    print('general ratio: exempt %d of %d pixels, |hist diff| %d' % (int(exempt.sum()), exempt.size, int(diff)))
    assert diff <= 2 * int((exempt & (label < c)).sum())
