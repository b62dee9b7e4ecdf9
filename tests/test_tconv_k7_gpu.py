"""cat_tconv_fwd with 7 x 7 segments (csrc/conv_pk7.hip: the (8 + 6) x (16 + 6) patch kernels) through the C ABI against float64 ATen on the
host, at TOL = 1e-4 with rel() (tests/test_kernels_gpu.py), with sentinels outside every written slice and behind every buffer as in part B of
tests/test_fused_kernels_gpu.py.  The reference's parser default is --kernel_sizes 3 5 7 (options/distill_options.py:100-104): these are the
first / second convs of its blocks (7 x 7 'same' convs under zero and reflect padding), their input gradients (padv = 6 into an (H + 6) x (W + 6)
plane under reflect padding, padv = 3 under zero padding) and the branch sum with mixed kernel sizes.  The profiler family of every launch is
conv_tconv7 / conv_tconv7_multi: the new kernels ran, not the (8 + 4)-patch ones.

TCONV7_NT_CASES holds one case per tconv7_kernel<NT, 16> instantiation and value of `stats`; a host test holds the table to the dispatch arms of
conv_pk7.hip and to the symbols of tests/golden/codegen_conv_pk7.json.  Two launches have the production shape of a wide 3 5 7 block: the
256-wide branch sum and the 256-channel input gradient, two N blocks of NT = 8 each.  Largest distance observed on an MI355X: 1.3e-6."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_fused_kernels_gpu import (ACT_LRELU, ACT_NONE, ACT_RELU, DGRAD, FWD, ROOT, SENTINEL, _act, _cmp, _columns, _host, _nchw, _nhwc_buffer,
                                    _pad, _padded_weight, _profiled, _sentinel, _tail, _tile_stats, cdiv, cs4, dev)      # noqa: F401  (dev: fixture)

PK7_SRC = os.path.join(ROOT, 'cat_amd', 'csrc', 'conv_pk7.hip')
PK7_GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'codegen_conv_pk7.json')

# (N, H, W, Cin, Cout, reflect): ragged tiles both ways + one full chunk and a one-quad remainder + a ragged N tile; the plane equals the kernel
# (every halo pixel mirrored, remainder-only chunk); 9 N tiles = two N blocks
SINGLE = [(2, 9, 17, 20, 23, 0), (1, 7, 7, 4, 5, 1), (2, 9, 17, 36, 136, 1)]


@functools.lru_cache(maxsize=None)
def _single_inputs(case):
    n, h, w, cin, cout, reflect = case
    return (detfill.normal((n, cin, h, w), 900), detfill.normal((cout, cin, 7, 7), 901, 1.0 / np.sqrt(cin * 49)), detfill.normal((cout,), 902, 0.2),
            detfill.normal((n, cout, h, w), 903))


def _run_single(dev, case, epilogue):
    """one 7 x 7 'same' conv; epilogue: LeakyReLU 0.2 + residual instead of the plain bias"""
    from cat_amd import ops, tconv
    n, h, w, cin, cout, reflect = case
    x, wt, b, res = _single_inputs(case)
    y64 = F.conv2d(_pad(x.double(), 3, reflect), wt.double(), b.double())
    want = {'y': F.leaky_relu(y64, 0.2) + res.double() if epilogue else y64}
    xg = ops.to_nhwc(x.to(dev))
    pack = tconv.pack(_padded_weight(wt, dev), FWD)
    assert pack.numel() == tconv.pack_floats(7, cs4(cin), cout)
    ycw, ycs = cs4(cout), cs4(cout) + 8
    yflat, y = _sentinel((n, h, w, ycs), dev)
    seg = tconv.Segment(xg, 7, 3, reflect, 0)
    rg = ops.to_nhwc(res.to(dev)) if epilogue else None
    _, fam = _profiled(lambda: tconv.run([seg], pack, b.to(dev), None, cout, n, h, w, h, w, act=ACT_LRELU if epilogue else ACT_NONE, slope=0.2, ycs=ycs,
                                         ycw=ycw, yptr=y.data_ptr(), res=rg))
    assert fam.get('conv_tconv7', 0) == 1 and 'conv_tconv' not in fam, fam
    yc = y.cpu()
    _columns(yc, range(ycw), range(cout), (case, 'y'))
    _tail(yflat, (case, 'y'))
    _cmp('K7', (case, epilogue), {'y': _nchw(yc, 0, cout)}, want)


@pytest.mark.gpu
@pytest.mark.parametrize('case', SINGLE, ids=lambda c: '%dx%dx%d-%dto%d-refl%d' % c)
def test_tconv_7x7_same_conv(dev, case):
    _run_single(dev, case, False)


@pytest.mark.gpu
def test_tconv_7x7_epilogue_activation_and_residual(dev):
    _run_single(dev, SINGLE[0], True)


def _run_input_gradient(dev, reflect, cin, cout):
    from cat_amd import ops, tconv
    n, h, w = 2, 9, 17
    wt, dy = detfill.normal((cout, cin, 7, 7), 911, 1.0 / np.sqrt(cout * 49)), detfill.normal((n, cout, h, w), 912)
    pad = 3
    ho, wo = (h + 2 * pad, w + 2 * pad) if reflect else (h, w)
    xin = torch.zeros((n, cin, ho, wo), dtype=torch.float64, requires_grad=True)      # the padded plane itself is the leaf under reflect padding
    yref = F.conv2d(xin, wt.double(), padding=0 if reflect else pad)
    want = {'dx': torch.autograd.grad(yref, xin, dy.double())[0]}
    pack = tconv.pack(_padded_weight(wt, dev), DGRAD)
    dyg = _nhwc_buffer(dy, cs4(cout), dev)
    seg = tconv.Segment(None, 7, 6 if reflect else 3, False, 0, c4=cs4(cout), cin=cout, xcs=cs4(cout), ptr=dyg.data_ptr())
    ycw, ycs = cs4(cin), cs4(cin) + 4
    yflat, y = _sentinel((n, ho, wo, ycs), dev)
    _, fam = _profiled(lambda: tconv.run([seg], pack, None, None, cin, n, h, w, ho, wo, ycs=ycs, ycw=ycw, yptr=y.data_ptr()))
    assert fam.get('conv_tconv7', 0) == 1 and 'conv_tconv' not in fam, fam
    yc = y.cpu()
    _columns(yc, range(ycw), range(cin), (reflect, 'dx'))
    _tail(yflat, (reflect, 'dx'))
    _cmp('K7', ('dgrad', reflect, cin, cout), {'dx': _nchw(yc, 0, cin)}, want)


@pytest.mark.gpu
@pytest.mark.parametrize('reflect', [1, 0], ids=['padv6-padded-plane', 'padv3-zero'])
def test_tconv_7x7_input_gradient(dev, reflect):
    """the input gradient of a 7 x 7 conv 23 -> 20 as the backward pass launches it: under reflect padding into the padded (H + 6) x (W + 6)
    plane (padv = k - 1 = 6; the reflect fold is another kernel), under zero padding with padv = k - 1 - pad = 3"""
    _run_input_gradient(dev, reflect, 23, 20)


@pytest.mark.gpu
def test_tconv_7x7_stage1_input_gradient_two_n_blocks(dev):
    """the stage-1 input gradient of a wide 3 5 7 block: 256 channels (two N blocks of tconv7_kernel<8, 16>) from a 44-channel dy, padv = 6"""
    assert tconv7_launch(256) == (8, 2)
    _run_input_gradient(dev, 1, 256, 44)


SUM_MS, SUM_KS = [7, 12, 18, 5, 9, 4], [7, 5, 3, 1, 1, 1]
SUM_SHAPE, SUM_NN = (2, 9, 17), 23
SUM_WIDE = (256, 4)      # the 256-wide branch sum of a 3 5 7 block: the first four slices, ks (7, 5, 3, 1)


@functools.lru_cache(maxsize=None)
def _sum_inputs(nn=SUM_NN):
    n, h, w = SUM_SHAPE
    hb = [detfill.normal((n, m, h, w), 920 + i) for i, m in enumerate(SUM_MS)]
    sc = [detfill.normal((n, m), 930 + i).abs() + 0.5 for i, m in enumerate(SUM_MS)]
    sh = [detfill.normal((n, m), 940 + i, 0.3) for i, m in enumerate(SUM_MS)]
    ws = [detfill.normal((nn, m, k, k), 950 + i, 1.0 / np.sqrt(m * k * k * 6)) for i, (m, k) in enumerate(zip(SUM_MS, SUM_KS))]
    return hb, sc, sh, ws, detfill.normal((nn,), 960, 0.1)


def _sum_ref(nn, nseg, act, reflect, dtype):
    n, h, w = SUM_SHAPE
    hb, sc, sh, ws, b = _sum_inputs(nn)
    y = torch.zeros((n, nn, h, w), dtype=dtype)
    for i, k in enumerate(SUM_KS[:nseg]):
        a = _act(hb[i].to(dtype) * sc[i].to(dtype)[:, :, None, None] + sh[i].to(dtype)[:, :, None, None], act)
        y = y + F.conv2d(_pad(a, k // 2, reflect), ws[i].to(dtype))
    y = y + b.to(dtype).view(1, -1, 1, 1)
    s, m2, _ = _tile_stats(y)
    return {'y': y, 'sum': s, 'm2': m2}


def _run_sum(dev, nn, nseg, act, reflect):
    """the first `nseg` of the six slices into `nn` output channels: three per hidden buffer, as the 23-wide launch lays them out"""
    from cat_amd import tconv
    n, h, w = SUM_SHAPE
    hb, sc, sh, ws, b = _sum_inputs(nn)
    want = _sum_ref(nn, nseg, act, reflect, torch.float64)
    # buffer 0 holds the first three slices, buffer 1 the last three; a sentinel slice behind each (a neighbour's channels)
    bufs = []
    for lo, hi in ((0, 3), (3, 6)):
        offs = np.cumsum([0] + [cs4(m) for m in SUM_MS[lo:hi]])
        hc = int(offs[-1]) + 4
        hbuf, scb, shb = torch.full((n, h, w, hc), SENTINEL), torch.full((n, hc), SENTINEL), torch.full((n, hc), SENTINEL)
        hbuf[..., :hc - 4], scb[:, :hc - 4], shb[:, :hc - 4] = 0.0, 0.0, 0.0
        for j, i in enumerate(range(lo, hi)):
            o, m = int(offs[j]), SUM_MS[i]
            hbuf[..., o:o + m], scb[:, o:o + m], shb[:, o:o + m] = hb[i].permute(0, 2, 3, 1), sc[i], sh[i]
        bufs.append((hbuf.to(dev), scb.to(dev), shb.to(dev), offs, hc))
    packs = [tconv.pack(_padded_weight(wt, dev), FWD) for wt in ws[:nseg]]
    segs, poff = [], 0
    for i, (m, k) in enumerate(list(zip(SUM_MS, SUM_KS))[:nseg]):
        hg, scg, shg, offs, hc = bufs[i // 3]
        o = int(offs[i % 3])
        segs.append(tconv.Segment(None, k, k // 2, reflect and k > 1, poff, c4=cs4(m), cin=m, xcs=hc, ptr=hg.data_ptr() + 4 * o,
                                  scale=scg.data_ptr() + 4 * o, shift=shg.data_ptr() + 4 * o, act=act, slope=0.2, sstride=hc))
        poff += packs[i].numel()
    # zero columns [Nn, ycw) inside the last 16-wide N tile, the only ones cat_tconv_t promises (256 channels fill their tiles: none)
    ycw = min(cs4(nn) + 4, cdiv(nn, 16) * 16)
    ycs, scs = ycw + 8, ycw + 4
    yflat, y = _sentinel((n, h, w, ycs), dev)
    tiles = n * cdiv(h, 8) * cdiv(w, 16)
    tflat, tab = _sentinel((tiles, 2, scs), dev)
    _, fam = _profiled(lambda: tconv.run(segs, torch.cat(packs), b.to(dev), None, nn, n, h, w, h, w, ycs=ycs, ycw=ycw, yptr=y.data_ptr(), stats=tab, scs=scs))
    assert fam.get('conv_tconv7_multi', 0) == 1 and 'conv_tconv_multi' not in fam, fam
    yc, tc = y.cpu(), tab.cpu()
    _columns(yc, range(ycw), range(nn), ('sum', 'y'))           # [Nn, ycw) exactly 0, [ycw, ycs) untouched
    _columns(tc, range(ycw), range(nn), ('sum', 'table'))
    _tail(yflat, 'y')
    _tail(tflat, 'table')
    _cmp('K7', ('sum', nn, act, reflect), {'y': _nchw(yc, 0, nn), 'sum': tc[:, 0, :nn], 'm2': tc[:, 1, :nn]}, want)


@pytest.mark.gpu
@pytest.mark.parametrize('act,reflect', [(ACT_RELU, 0), (ACT_LRELU, 1)], ids=['relu-zero', 'lrelu-reflect'])
def test_tconv_branch_sum_with_a_7x7_segment(dev, act, reflect):
    """six K-concatenated segments with ks (7, 5, 3, 1, 1, 1) over channel slices of TWO hidden buffers, per-sample staging affine + activation,
    bias, per-tile statistics, N = 2: the stage-2 launch of a 3 5 7 block"""
    assert (cs4(SUM_NN) + 4, cs4(SUM_NN) + 12, cs4(SUM_NN) + 8) == (28, 36, 32)      # ycw, ycs, scs of the launch
    _run_sum(dev, SUM_NN, 6, act, reflect)


@pytest.mark.gpu
def test_tconv_256_wide_branch_sum_two_n_blocks(dev):
    """Cout = 256: nt_total = 16, two N blocks of tconv7_kernel<8, 16>, ks (7, 5, 3, 1) with statistics"""
    nn, nseg = SUM_WIDE
    assert tconv7_launch(nn) == (8, 2) and SUM_KS[:nseg] == [7, 5, 3, 1]
    _run_sum(dev, nn, nseg, ACT_LRELU, 1)


# ================================================================================================ every tconv7_kernel<NT, 16> instantiation
def tconv7_launch(nn):
    """mirror of (nt, nblk) of tconv7_launch: at most 8 N tiles of 16 channels per workgroup, the N blocks evened out"""
    nt_total = cdiv(nn, 16)
    nblk = cdiv(nt_total, 8)
    nt = cdiv(nt_total, nblk)
    return nt, cdiv(nt_total, nt)


# (NT, stats) -> (cin, cout, reflect, bias, N, H, W): one 7 x 7 'same' conv; reflect / zero and bias / no bias alternate down the rows
TCONV7_NT_CASES = {}
for _nt, (_cin, _cout) in enumerate([(8, 13), (20, 30), (12, 44), (9, 54), (16, 77), (11, 90), (18, 100), (10, 120)], 1):
    TCONV7_NT_CASES[(_nt, 0)] = (_cin, _cout, _nt % 2, (_nt // 2) % 2, 2, 9, 17)
    TCONV7_NT_CASES[(_nt, 1)] = (_cin, _cout, (_nt + 1) % 2, (_nt // 2 + 1) % 2, 3, 7, 7)


def test_case_table_covers_the_tconv7_instantiations():
    arms = re.findall(r'(?:case (\d+)|default): CAT_PK7_LAUNCH\((\d+)\)', open(PK7_SRC).read())
    assert all(a == '' or a == b for a, b in arms), arms      # (the default arm serves the largest NT)
    launched = sorted(int(b) for _, b in arms)
    symbols = sorted(int(m.group(1)) for m in (re.search(r'tconv7_kernelILi(\d+)ELi16EE', name) for name in json.load(open(PK7_GOLDEN))) if m)
    assert launched == symbols == list(range(1, 9)), (launched, symbols)
    assert set(TCONV7_NT_CASES) == {(nt, st) for nt in launched for st in (0, 1)}
    for (nt, st), (cin, cout, reflect, bias, n, h, w) in TCONV7_NT_CASES.items():
        assert tconv7_launch(cout) == (nt, 1), ((nt, st), tconv7_launch(cout))
        assert 8 <= cin <= 20 and (h, w) in ((9, 17), (7, 7))
    assert [c[1] for k, c in sorted(TCONV7_NT_CASES.items()) if k[1] == 0] == [13, 30, 44, 54, 77, 90, 100, 120]
    for st in (0, 1):
        rows = [TCONV7_NT_CASES[(nt, st)] for nt in range(1, 9)]
        assert {(r[2], r[3]) for r in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert tconv7_launch(256) == (8, 2) and tconv7_launch(136) == (5, 2) and tconv7_launch(129) == (5, 2) and tconv7_launch(128) == (8, 1)


@functools.lru_cache(maxsize=2)
def _k7_inputs(key):
    cin, cout, reflect, bias, n, h, w = TCONV7_NT_CASES[key]
    return (detfill.normal((n, cin, h, w), 970), detfill.normal((cout, cin, 7, 7), 971, 1.0 / np.sqrt(cin * 49)),
            detfill.normal((cout,), 972, 0.2) if bias else None)


def _k7_ref(key, dtype):
    cin, cout, reflect, bias, n, h, w = TCONV7_NT_CASES[key]
    x, wt, b = _k7_inputs(key)
    y = F.conv2d(_pad(x.to(dtype), 3, reflect), wt.to(dtype), None if b is None else b.to(dtype))
    if key[1]:
        s, m2, _ = _tile_stats(y)
        return {'y': y, 'sum': s, 'm2': m2}
    return {'y': F.leaky_relu(y, 0.2)}


def test_fp32_twin_of_the_tconv7_references_is_within_a_tenth_of_the_bar():
    """the deepest and the shallowest case of the table (K = 49 * cin), and the two production-shaped launches"""
    by_depth = sorted(TCONV7_NT_CASES, key=lambda k: (TCONV7_NT_CASES[k][0], k))
    for key in (by_depth[0], by_depth[-1]):
        _host('K7', key, functools.partial(_k7_ref, key))
    _host('K7', ('sum',) + SUM_WIDE, functools.partial(_sum_ref, SUM_WIDE[0], SUM_WIDE[1], ACT_LRELU, 1))


@pytest.mark.gpu
@pytest.mark.parametrize('key', sorted(TCONV7_NT_CASES), ids=lambda k: 'nt%d-stats%d' % k)
def test_tconv7_instantiation(dev, key):
    """the checks of test_tconv_instantiation (tests/test_fused_kernels_gpu.py) on the 7 x 7 translation unit"""
    from cat_amd import ops, tconv
    cin, cout, reflect, bias, n, h, w = TCONV7_NT_CASES[key]
    nt, stats = key
    assert tconv7_launch(cout) == (nt, 1)
    x, wt, b = _k7_inputs(key)
    want = _k7_ref(key, torch.float64)
    xg = ops.to_nhwc(x.to(dev))
    pack = tconv.pack(_padded_weight(wt, dev), FWD)
    ycw, ycs = cs4(cout), cs4(cout) + 8
    scs = ycw + 4
    yflat, y = _sentinel((n, h, w, ycs), dev)
    tiles = n * cdiv(h, 8) * cdiv(w, 16)
    tflat, tab = _sentinel((tiles, 2, scs), dev)
    seg = tconv.Segment(xg, 7, 3, reflect, 0)
    bg = None if b is None else b.to(dev)

    def call():
        tconv.run([seg], pack, bg, None, cout, n, h, w, h, w, act=ACT_NONE if stats else ACT_LRELU, slope=0.2, ycs=ycs, ycw=ycw, yptr=y.data_ptr(),
                  stats=tab if stats else None, scs=scs if stats else 0)
    _, fam = _profiled(call)
    assert fam.get('conv_tconv7', 0) == 1 and 'conv_tconv' not in fam, fam
    yc, tc = y.cpu(), tab.cpu()
    _columns(yc, range(ycw), range(cout), (key, 'y'))
    _tail(yflat, (key, 'y'))
    _tail(tflat, (key, 'table'))
    got = {'y': _nchw(yc, 0, cout)}
    if stats:
        _columns(tc, range(ycw), range(cout), (key, 'table'))
        got['sum'], got['m2'] = tc[:, 0, :cout], tc[:, 1, :cout]
    else:
        assert bool((tc == SENTINEL).all())
    _cmp('K7', key, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize('ks,padv,reflect,h,match', [(9, 4, 0, 9, 'kernel size'), (7, 7, 0, 9, 'padv'), (7, 3, 1, 6, 'reflect')],
                         ids=['ks9', 'padv7', 'reflect-H6'])
def test_tconv_refuses_outside_its_domain(dev, ks, padv, reflect, h, match):
    from cat_amd import tconv
    n, w, cin, cout = 1, 16, 8, 8
    xg = torch.zeros((n, h, w, cin), device=dev)
    pack = torch.zeros(ks * ks * cin * 16 * 4, device=dev)
    yflat, y = _sentinel((n, h, w, cout), dev)
    seg = tconv.Segment(None, ks, padv, reflect, 0, c4=cin, cin=cin, xcs=cin, ptr=xg.data_ptr())
    with pytest.raises(RuntimeError, match=match):
        tconv.run([seg], pack, None, None, cout, n, h, w, h, w, ycs=cout, ycw=cout, yptr=y.data_ptr())
    torch.cuda.synchronize()
    assert bool((yflat == SENTINEL).all())
