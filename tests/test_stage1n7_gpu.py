"""cat_tstage1n7_fwd / cat_tstage1n7_dgrad (csrc/conv_s1n7.hip) -- the narrow one-launch stage 1 for the kernel sizes 3 5 7 and the second convs'
input gradients of such a unit in one launch: the 7 x 7, 5 x 5 and 3 x 3 convs and the N-concatenated 1 x 1 group from ONE staging of the
source -- through the C ABI against float64 ATen on the host (F.conv2d with explicit reflect / zero padding via F.pad), with the checks and
the bar of parts B and C of tests/test_fused_kernels_gpu.py (cat_tstage1_fwd / cat_tstage1_dgrad: TOL with rel() for every tensor, exact
zeros in a slice's padding columns, sentinels everywhere else and behind the buffers): every slot's slice of the pre-norm buffer, the
per-tile sum and M2, then scale / shift / mean / rstd / running statistics out of cat_tnorm_finalize over that table (G = 1 and G = N).

Cases: N = 2 throughout (the image stride matters).  Every instantiation -- the 32 N-tile combinations the predicate admits, with and
without statistics -- runs at (cin, H, W) = (6, 9, 17): a ragged channel quad, partial tiles both ways; padding alternates between
reflect and zero over them.  Beyond those: a 5 x 7 plane with zero padding (smaller than one tile), 7 x 7 with reflect (the smallest
mirrored window), cin 20 (a second, partial chunk) and 36 (the gamma|beta input: three chunks through both tile buffers), an x pixel stride
wider than cs4(cin), with and without bias.  Everywhere: nvalid < width in every slot, col0 = 4 for the first slice, a statistics row
wider than the pre-norm row's slices (scs = ycs + 4).  The dgrad cases alternate between four buffers with four strides and the layout of
fused_unit's backward step 4 (the three wide slots as slices of one buffer, the 1 x 1 slot in its own)."""
import ctypes as C
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_fused_kernels_gpu import (DGRAD, FWD, SENTINEL, _cmp, _columns, _concat_pack, _finalize_gpu, _host, _nchw, _nhwc_buffer, _norm_ref, _pad,
                                    _padded_weight, _profiled, _sentinel, _tail, _tile_stats, cdiv, cs4)

N = 2
KS = (7, 5, 3, 1)
WIDE = {1: 13, 2: 18}                                                     # channels of a wide slot with 1 / 2 N tiles: widths 16 / 20
ONE = {1: (6,), 2: (9, 10), 3: (15, 14, 5), 4: (15, 15, 15, 13)}          # 1 x 1 compositions: widths 8 / 24 / 40 / 64
COMBOS = list(itertools.product((1, 2), (1, 2), (1, 2), (1, 2, 3, 4)))    # N tiles of the 7 / 5 / 3 / 1 slot


def _chans(combo):
    return WIDE[combo[0]], WIDE[combo[1]], WIDE[combo[2]], ONE[combo[3]]


# name -> (cin, extra pixel stride of the source, branch channels (m7, m5, m3, 1 x 1 composition), H, W, reflect, bias)
FWD_CASES = {'t%d%d%d%d' % c: (6, 0, _chans(c), 9, 17, i & 1, 1) for i, c in enumerate(COMBOS)}
FWD_CASES.update({
    'cin20-5x7-zero-xpad': (20, 4, _chans((1, 2, 1, 2)), 5, 7, 0, 1),
    'cin36-7x7-reflect': (36, 0, _chans((2, 1, 2, 3)), 7, 7, 1, 1),
    'cin36-9x17-reflect-xpad-nobias': (36, 8, _chans((1, 1, 1, 4)), 9, 17, 1, 0),
    'cin20-9x17-zero-nobias': (20, 0, _chans((2, 2, 2, 1)), 9, 17, 0, 0),
})
DEEPEST = 'cin36-7x7-reflect'      # K = 36 * 49 on 49 pixels
# name -> (dy channels, extra pixel stride of dy, branch channels, H, W, layout)
DG_CASES = {'t%d%d%d%d' % c: (6, 0, _chans(c), 9, 17, ('sep', 'unit')[i & 1]) for i, c in enumerate(COMBOS)}
DG_CASES.update({
    'cout20-5x7-xpad-unit': (20, 4, _chans((1, 2, 1, 2)), 5, 7, 'unit'),
    'cout36-9x17-sep': (36, 0, _chans((2, 1, 2, 3)), 9, 17, 'sep'),
    'cout36-7x7-xpad-unit': (36, 8, _chans((2, 2, 1, 4)), 7, 7, 'unit'),
})


def supported(w7, w5, w3, w1):
    """mirror of cat_tstage1n7_supported: every slot present, <= 2 / 2 / 2 / 4 N tiles"""
    return min(w7, w5, w3, w1) > 0 and max(w7, w5, w3) <= 32 and w1 <= 64


def _widths(chans):
    m7, m5, m3, m1c = chans
    return {7: cs4(m7), 5: cs4(m5), 3: cs4(m3), 1: sum(cs4(m) for m in m1c)}


def _layout(name):
    """Z1 = [4 sentinel lanes | k = 1 slice | k = 3 slice | k = 5 slice | k = 7 slice | 4 sentinel lanes], the order of a plan -> slot widths,
    first columns (both by kernel size), pixel stride, branches (k, channels, first column)"""
    m7, m5, m3, m1c = FWD_CASES[name][2]
    width = _widths(FWD_CASES[name][2])
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
    cin, xpad, chans, h, w, reflect, bias = FWD_CASES[name]
    ycs, branches = _layout(name)[2:]
    x = detfill.normal((N, cin, h, w), 2100)
    ws = [detfill.normal((m, cin, k, k), 2110 + i, 1.0 / (cin * k * k) ** 0.5) for i, (k, m, o) in enumerate(branches)]
    bs = [detfill.normal((m,), 2130 + i, 0.3) if bias else None for i, (k, m, o) in enumerate(branches)]
    gamma, beta = detfill.normal((ycs + 4,), 2150).abs() + 0.5, detfill.normal((ycs + 4,), 2151, 0.3)
    run = [(detfill.normal((m,), 2160 + i, 0.1), detfill.normal((m,), 2180 + i).abs() + 0.5) for i, (k, m, o) in enumerate(branches)]
    return x, ws, bs, gamma, beta, run


def _ref(name, dtype):
    cin, xpad, chans, h, w, reflect, bias = FWD_CASES[name]
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


def _dg_layout(name):
    """-> slot widths (7, 5, 3, 1), per slot (buffer index, first column), pixel stride per buffer, branches (slot, k, channels, column in slot)"""
    cout, xpad, chans, h, w, layout = DG_CASES[name]
    wd = _widths(chans)
    width = [wd[k] for k in KS]
    if layout == 'sep':
        place = [(0, 4), (1, 0), (2, 8), (3, 4)]
        strides = [width[0] + 8, width[1] + 4, width[2] + 12, width[3] + 8]
    else:      # hidden-activation gradients of a unit: [. | k = 3 | k = 5 | k = 7 | .] in one buffer, the depthwise ones in their own
        place = [(0, 4 + width[2] + width[1]), (0, 4 + width[2]), (0, 4), (1, 0)]
        strides = [4 + width[2] + width[1] + width[0] + 4, width[3] + 4]
    m7, m5, m3, m1c = chans
    branches, o = [(0, 7, m7, 0), (1, 5, m5, 0), (2, 3, m3, 0)], 0
    for m in m1c:
        branches.append((3, 1, m, o))
        o += cs4(m)
    return width, place, strides, branches


@functools.lru_cache(maxsize=None)
def _dg_inputs(name):
    cout, xpad, chans, h, w, layout = DG_CASES[name]
    branches = _dg_layout(name)[3]
    dy = detfill.normal((N, cout, h, w), 2200)
    ws = [detfill.normal((cout, m, k, k), 2210 + i, 1.0 / (cout * k * k) ** 0.5) for i, (slot, k, m, o) in enumerate(branches)]
    return dy, ws


def _dg_ref(name, dtype):
    cout, xpad, chans, h, w, layout = DG_CASES[name]
    branches = _dg_layout(name)[3]
    dy, ws = _dg_inputs(name)
    out = {}
    for i, (slot, k, m, o) in enumerate(branches):
        a = torch.zeros((N, m, h, w), dtype=dtype, requires_grad=True)
        out['dx%d' % i], = torch.autograd.grad(F.conv2d(a, ws[i].to(dtype), padding=k // 2), a, dy.to(dtype))
    return out


def test_cases_reach_every_instantiation_and_edge_and_the_bar_is_reachable():
    for table in (FWD_CASES, DG_CASES):
        rows = {tuple(cdiv(_widths(c[2])[k], 16) for k in KS) for c in table.values()}
        assert rows == set(COMBOS) and len(COMBOS) == 32
        assert all(supported(*[_widths(c[2])[k] for k in KS]) for c in table.values())
        assert all(m % 4 for c in table.values() for m in c[2][:3]) and all(any(m % 4 for m in c[2][3]) for c in table.values())      # nvalid < width
        assert {c[0] for c in table.values()} == {6, 20, 36} and any(c[1] for c in table.values())
        assert {(9, 17), (5, 7), (7, 7)} <= {c[3:5] for c in table.values()}
    assert {c[5] for c in FWD_CASES.values() if c[3:5] == (9, 17)} == {0, 1} and {c[6] for c in FWD_CASES.values()} == {0, 1}
    assert FWD_CASES['cin20-5x7-zero-xpad'][5] == 0 and FWD_CASES[DEEPEST][5] == 1
    assert all(c[3] >= 7 and c[4] >= 7 for c in FWD_CASES.values() if c[5])
    assert {c[5] for c in DG_CASES.values()} == {'sep', 'unit'}
    assert any(len(set(_dg_layout(n)[2])) == 4 for n in DG_CASES) and any(len(_dg_layout(n)[2]) == 2 for n in DG_CASES)
    # fp32 ATen within TOL / 10 of float64 at the deepest K: a correct fp32 kernel has ten-fold room under the bar
    _host('B', DEEPEST, lambda dt: _ref(DEEPEST, dt))
    _host('C', 'cout36-9x17-sep', lambda dt: _dg_ref('cout36-9x17-sep', dt))


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.mark.gpu
def test_support_predicate_matches_its_mirror(dev):
    from cat_amd import _lib as L
    for w7 in (0, 4, 16, 17, 32, 33):
        for w5 in (0, 16, 32, 36):
            for w3 in (-4, 0, 8, 20, 32, 36, 48):
                for w1 in (0, 4, 16, 17, 48, 49, 64, 65, 68, 132):
                    assert bool(L.query('cat_tstage1n7_supported', w7, w5, w3, w1)) == supported(w7, w5, w3, w1), (w7, w5, w3, w1)


def _launch(dev, name):
    from cat_amd import _lib as L, ops
    cin, xpad, chans, h, w, reflect, bias = FWD_CASES[name]
    width, col0, ycs, branches = _layout(name)
    x, ws, bs, gamma, beta, run = _inputs(name)
    scs, tiles = ycs + 4, N * cdiv(h, 8) * cdiv(w, 16)
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
    call = lambda: L.call('cat_tstage1n7_fwd', C.byref(gs), ops._p(xg), pk, ops._p(bg), ops._p(z), ops._p(tab), ops._stream())
    return call, (zflat, z, tflat, tab), (gs, xg, pk, packs, wgs, bg)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(FWD_CASES))
def test_stage1n7_fwd(dev, name):
    cin, xpad, chans, h, w, reflect, bias = FWD_CASES[name]
    width, col0, ycs, branches = _layout(name)
    x, ws, bs, gamma, beta, run = _inputs(name)
    call, (zflat, z, tflat, tab), keep = _launch(dev, name)
    _, fam = _profiled(call)
    assert fam.get('conv_tstage1n7', 0) == 1, fam
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
    # (the table's sentinel columns lie in no slice: the finalize reads none of them)
    for tag, inst in (('b', 0), ('i', 1)):
        r = _finalize_gpu(dev, tab, ycs + 4, inst, N, h, w, gamma, beta, pairs, run, ycs + 4)
        got.update({tag + key: v for key, v in r.items()})
    _cmp('B', name, got, _ref(name, torch.float64))


def _dg_launch(dev, name):
    from cat_amd import _lib as L, ops
    cout, xpad, chans, h, w, layout = DG_CASES[name]
    width, place, strides, branches = _dg_layout(name)
    dy, ws = _dg_inputs(name)
    dyg = _nhwc_buffer(dy, cs4(cout) + xpad, dev, pad_to=cs4(cout))
    wgs = [_padded_weight(wt, dev) for wt in ws]
    packs = [_concat_pack([(wgs[i], o) for i, (s, k, m, o) in enumerate(branches) if s == slot], DGRAD, KS[slot], cout, width[slot], dev)
             for slot in range(4)]
    bufs = [_sentinel((N, h, w, cs), dev) for cs in strides]
    gs = L.Stage1S7Geom()
    gs.N, gs.H, gs.W, gs.xcs, gs.cin, gs.reflect, gs.ycs, gs.scs = N, h, w, cs4(cout) + xpad, cout, 0, 0, 0
    pk, dxs, dxcs = (C.c_void_p * 4)(), (C.c_void_p * 4)(), (C.c_int * 4)()
    for slot in range(4):
        bi, c0 = place[slot]
        gs.col0[slot], gs.width[slot], gs.nvalid[slot] = c0, width[slot], sum(m for s, k, m, o in branches if s == slot)
        pk[slot], dxs[slot], dxcs[slot] = packs[slot].data_ptr(), bufs[bi][1].data_ptr(), strides[bi]
    call = lambda: L.call('cat_tstage1n7_dgrad', C.byref(gs), ops._p(dyg), pk, dxs, dxcs, ops._stream())
    return call, bufs, (gs, dyg, pk, dxs, dxcs, packs, wgs)


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(DG_CASES))
def test_stage1n7_dgrad(dev, name):
    width, place, strides, branches = _dg_layout(name)
    call, bufs, keep = _dg_launch(dev, name)
    _, fam = _profiled(call)
    assert fam.get('conv_tstage1n7_dgrad', 0) == 1, fam
    host = [b[1].cpu() for b in bufs]
    for bi, (flat, _) in enumerate(bufs):
        owned = [c for slot in range(4) if place[slot][0] == bi for c in range(place[slot][1], place[slot][1] + width[slot])]
        valid = [c for slot, k, m, o in branches if place[slot][0] == bi for c in range(place[slot][1] + o, place[slot][1] + o + m)]
        _columns(host[bi], owned, valid, (name, 'buffer', bi))
        _tail(flat, (name, 'buffer', bi))
    got = {'dx%d' % i: _nchw(host[place[slot][0]], place[slot][1] + o, m) for i, (slot, k, m, o) in enumerate(branches)}
    _cmp('C', name, got, _dg_ref(name, torch.float64))


@pytest.mark.gpu
def test_stage1n7_refuses_what_it_has_no_kernel_for(dev):
    """widths outside the domain, a reflect-padded plane smaller than the 7 x 7 window, reflect padding in the input-gradient form: an error
    that names the entry, nothing written"""
    call, (zflat, z, tflat, tab), keep = _launch(dev, 'cin36-7x7-reflect')
    gs = keep[0]
    for slot, bad in ((0, 36), (1, 0), (2, 48), (3, 68)):
        good, gs.width[slot] = gs.width[slot], bad
        with pytest.raises(RuntimeError, match='cat_tstage1n7_fwd.*tstage1n7'):
            call()
        gs.width[slot] = good
    for hh, ww in ((6, 7), (7, 6)):
        gs.H, gs.W = hh, ww
        with pytest.raises(RuntimeError, match='cat_tstage1n7_fwd.*reflect'):
            call()
    dcall, bufs, dkeep = _dg_launch(dev, 'cout20-5x7-xpad-unit')
    dgs = dkeep[0]
    dgs.reflect = 1
    with pytest.raises(RuntimeError, match='cat_tstage1n7_dgrad.*tstage1n7 dgrad'):
        dcall()
    dgs.reflect, dgs.width[3] = 0, 80
    with pytest.raises(RuntimeError, match='cat_tstage1n7_dgrad.*tstage1n7 dgrad'):
        dcall()
    torch.cuda.synchronize()
    assert bool((zflat == SENTINEL).all()) and bool((tflat == SENTINEL).all())
    assert all(bool((flat == SENTINEL).all()) for flat, _ in bufs)
