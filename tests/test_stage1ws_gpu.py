"""cat_tstage1ws_fwd (csrc/conv_s1ws.hip) -- stage 1 of a wide InvertedResidualChannels block in one launch with statistics, the teacher's
widths 42 / 42 / 4 x 42 -- through the C ABI against float64 ATen on the host, with the harness, the quantities and the bars of part B of
tests/test_fused_kernels_gpu.py (the same checks for cat_tstage1_fwd): every slot's slice of the pre-norm buffer, zeros in the slices'
padding columns, sentinels in every column of y and of the statistics table outside the three slices and behind the buffers, the per-tile
sum and M2, then mean / variance out of cat_tnorm_finalize over that table (G = 1 with running statistics, G = N).

Cases: N = 2; planes 16 x 16 (whole tiles) and 9 x 17 (partial tiles in both directions: 128, 16, 16 and 1 valid pixels per tile); cin 256
and 36 (the last 16-channel chunk has one quad); zero and reflect padding; with and without bias."""
import ctypes as C

import pytest
import torch

from test_fused_kernels_gpu import (FWD, SENTINEL, _cmp, _columns, _concat_pack, _finalize_gpu, _host, _nchw, _nhwc_buffer, _padded_weight, _profiled,
                                    _s1_inputs, _s1_layout, _s1_ref, _s1_widths, _sentinel, _tail, cdiv, cs4)

W5, W3, W1C = 42, 42, (42, 42, 42, 42)      # the 5 x 5 and 3 x 3 residual branches; the k = 1 residual branch + three depthwise branches
# (cin, w5, w3, 1 x 1 composition, reflect, bias, N, H, W, extra pixel stride of x): the case tuples of test_fused_kernels_gpu's part B
CASES = [(cin, W5, W3, W1C, reflect, bias, 2, h, w, 0) for cin in (256, 36) for (h, w) in ((16, 16), (9, 17)) for reflect in (0, 1) for bias in (1, 0)]
_id = lambda c: 'cin%d-%dx%d-%s-bias%d' % (c[0], c[7], c[8], 'reflect' if c[4] else 'zero', c[5])


def ws_supported(w5, w3, w1):
    """mirror of cat_tstage1ws_supported: 3 + 3 + 11 N tiles"""
    return 32 < w5 <= 48 and 32 < w3 <= 48 and 160 < w1 <= 176


def test_cases_are_in_the_kernels_domain_and_the_bar_is_reachable():
    assert _s1_widths(W5, W3, W1C) == (44, 44, 176) and ws_supported(44, 44, 176)
    assert len(CASES) == 16 and len(set(CASES)) == 16
    for case in (CASES[0], CASES[-1]):      # fp32 ATen within TOL / 10 of float64: a correct fp32 kernel has ten-fold room (K = 256 * 25 and 36 * 25)
        _host('B', case, lambda dt, case=case: _s1_ref(case, dt))


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.mark.gpu
def test_support_predicate_matches_its_mirror(dev):
    from cat_amd import _lib as L
    for w5 in (0, 32, 33, 44, 48, 49):
        for w3 in (16, 32, 33, 48, 49):
            for w1 in (44, 160, 161, 176, 177):
                assert bool(L.query('cat_tstage1ws_supported', w5, w3, w1)) == ws_supported(w5, w3, w1), (w5, w3, w1)
    assert not L.query('cat_tstage1_supported', 44, 44, 176)      # the widths the narrow one-launch kernel refuses


def _launch(dev, case, entry='cat_tstage1ws_fwd'):
    from cat_amd import _lib as L, ops, tconv
    cin, w5, w3, w1c, reflect, bias, n, h, w, xpad = case
    width, col0, ycs, branches = _s1_layout(case)
    x, ws, bs, gamma, beta, run = _s1_inputs(case)
    scs, tiles = ycs, n * cdiv(h, 8) * cdiv(w, 16)
    xg = _nhwc_buffer(x, cs4(cin) + xpad, dev, pad_to=cs4(cin))
    wgs = [_padded_weight(wt, dev) for wt in ws]
    packs = {}
    for k in (1, 3, 5):
        items = [(wgs[i], o - col0[k]) for i, (bk, m, o) in enumerate(branches) if bk == k]
        packs[k] = tconv.pack(items[0][0], FWD) if k > 1 else _concat_pack(items, FWD, k, cin, width[k], dev)
    bvec = torch.zeros(ycs)
    for (k, m, o), b in zip(branches, bs):
        if b is not None:
            bvec[o:o + m] = b
    bg = bvec.to(dev) if bias else None
    gs = L.Stage1Geom()
    gs.N, gs.H, gs.W, gs.xcs, gs.cin, gs.reflect, gs.ycs, gs.scs = n, h, w, cs4(cin) + xpad, cin, reflect, ycs, scs
    pk = (C.c_void_p * 3)()
    for slot, k in enumerate((5, 3, 1)):
        gs.col0[slot], gs.width[slot], gs.nvalid[slot] = col0[k], width[k], sum(m for bk, m, o in branches if bk == k)
        pk[slot] = packs[k].data_ptr()
    zflat, z = _sentinel((n, h, w, ycs), dev)
    tflat, tab = _sentinel((tiles, 2, scs), dev)
    call = lambda: L.call(entry, C.byref(gs), ops._p(xg), pk, ops._p(bg), ops._p(z), ops._p(tab), ops._stream())
    return call, (zflat, z, tflat, tab), (gs, xg, pk, packs, wgs, bg)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=_id)
def test_stage1ws_fwd(dev, case):
    cin, w5, w3, w1c, reflect, bias, n, h, w, xpad = case
    width, col0, ycs, branches = _s1_layout(case)
    x, ws, bs, gamma, beta, run = _s1_inputs(case)
    want = _s1_ref(case, torch.float64)
    call, (zflat, z, tflat, tab), keep = _launch(dev, case)
    _, fam = _profiled(call)
    assert fam.get('conv_tstage1ws', 0) == 1, fam
    zc, tc = z.cpu(), tab.cpu()
    owned = [c for k in (1, 3, 5) for c in range(col0[k], col0[k] + width[k])]
    valid = [c for k, m, o in branches for c in range(o, o + m)]
    _columns(zc, owned, valid, (case, 'Z1'))
    _columns(tc, owned, valid, (case, 'table'))
    _tail(zflat, (case, 'Z1'))
    _tail(tflat, (case, 'table'))
    got = {}
    for i, (k, m, o) in enumerate(branches):
        got.update({'z%d' % i: _nchw(zc, o, m), 'sum%d' % i: tc[:, 0, o:o + m], 'm2%d' % i: tc[:, 1, o:o + m]})
    pairs = [(o, m) for k, m, o in branches]
    for tag, inst in (('b', 0), ('i', 1)):
        r = _finalize_gpu(dev, tab, ycs, inst, n, h, w, gamma, beta, pairs, run, ycs)
        got.update({tag + key: v for key, v in r.items()})
    _cmp('B', case, got, want)


@pytest.mark.gpu
def test_stage1ws_fwd_refuses_what_it_has_no_kernel_for(dev):
    """widths outside 3 + 3 + 11 N tiles, and a reflect-padded plane smaller than the 5 x 5 window: an error, nothing written"""
    call, (zflat, z, tflat, tab), keep = _launch(dev, CASES[0])
    gs = keep[0]
    gs.width[2] = 180
    with pytest.raises(RuntimeError, match='tstage1ws'):
        call()
    gs.width[2] = 176
    gs.reflect, gs.H, gs.W = 1, 4, 64
    with pytest.raises(RuntimeError, match='tstage1ws'):
        call()
    torch.cuda.synchronize()
    assert bool((zflat == SENTINEL).all()) and bool((tflat == SENTINEL).all())
