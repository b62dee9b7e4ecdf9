"""The depthwise stage with 7 x 7 quads (cat_dwm7_fwd / cat_dwm7_bwd: the halo-3 instantiations of the stage kernels of csrc/block_norm.hip,
filters in a 7 x 7 frame) and the preparation job that writes the frame (cat_prep_run kind 5), through the C ABI against float64 ATen on the
host at TOL = 1e-4 with rel(), sentinels outside every written slice and behind every buffer (as part E of tests/test_fused_kernels_gpu.py
does for the 5 x 5 frame)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_fused_kernels_gpu import (ACT_RELU, NAN, SENTINEL, _act, _cmp, _columns, _dwm_geom, _nchw, _nhwc_buffer, _pad, _prep_run, _profiled,
                                    _sentinel, _tail, _tile_stats, cdiv, cs4, dev)      # noqa: F401  (dev: fixture)

PLANES = [(2, 9, 17), (1, 8, 16), (1, 4, 4)]      # ragged multi-tile; exactly one tile; the smallest plane reflect padding by 3 allows
KS9 = (7, 3, 1, 5, 7, 7, 7, 7, 7)                 # the run of five sevens is cut into two quad groups (kDwGroup = 4)


def frame49(w_list, ks_list):
    """depthwise filters [c][k][k] -> [C][7][7]: a k x k filter centred, tap (ky, kx) at row (ky + 3 - k // 2) * 7 + kx + 3 - k // 2"""
    rows = []
    for wt, k in zip(w_list, ks_list):
        o = 3 - k // 2
        f = torch.zeros((wt.shape[0], 7, 7), dtype=wt.dtype)
        f[:, o:o + k, o:o + k] = wt
        rows.append(f)
    return torch.cat(rows)


def _w49(frame, dev):
    return frame.permute(1, 2, 0).reshape(49, -1).contiguous().to(dev)


# (ks per quad, plane, reflect, per-sample rows, statistics)
FWD_CASES = [(KS9, pl, refl, int(pl == 0 and refl == 1), 1) for pl in range(3) for refl in (0, 1)] + [(KS9, 0, 0, 1, 0), ((7,) * 24, 1, 1, 0, 1)]


@functools.lru_cache(maxsize=None)
def _fwd_inputs(case):
    ks, plane, reflect, per_image, stats = case
    n, h, w = PLANES[plane]
    c = 4 * len(ks)
    G = n if per_image else 1
    return (detfill.normal((n, c, h, w), 1000), detfill.normal((G, c), 1001).abs() + 0.5, detfill.normal((G, c), 1002, 0.3),
            [detfill.normal((4, k, k), 1010 + q, 1.0 / k) for q, k in enumerate(ks)], detfill.normal((c,), 1003, 0.2))


@pytest.mark.gpu
@pytest.mark.parametrize('case', FWD_CASES, ids=lambda c: 'nq%d-plane%d-refl%d-inst%d-stats%d' % ((len(c[0]),) + c[1:]))
def test_dwm7_fwd(dev, case):
    from cat_amd import _lib as L, ops
    ks, plane, reflect, per_image, stats = case
    x, scale, shift, ws, b = _fwd_inputs(case)
    n, c, h, w = x.shape
    nq = len(ks)
    a = _act(x.double() * scale.double().view(-1, c, 1, 1) + shift.double().view(-1, c, 1, 1), ACT_RELU)
    y64 = torch.cat([F.conv2d(_pad(a[:, 4 * q:4 * q + 4], k // 2, reflect), ws[q].double().unsqueeze(1), b[4 * q:4 * q + 4].double(), groups=4)
                     for q, k in enumerate(ks)], 1)
    want = {'y': y64}
    if stats:
        want['sum'], want['m2'], _ = _tile_stats(y64)
    xcs, ycs, scs, sstride = c + 4, c + 8, c + 4, (c + 4 if per_image else 0)
    xg = _nhwc_buffer(x, xcs, dev)
    rows = lambda v: F.pad(v, (0, 4), value=SENTINEL).to(dev) if per_image else v.reshape(-1).to(dev)
    g = _dwm_geom(n, h, w, nq, xcs, ycs, scs, sstride, reflect, ACT_RELU, ks)
    tiles = n * cdiv(h, 8) * cdiv(w, 16)
    yflat, y = _sentinel((n, h, w, ycs), dev)
    tflat, tab = _sentinel((tiles, 2, scs), dev)
    w49 = _w49(frame49(ws, ks), dev)
    scg, shg, bg = rows(scale), rows(shift), b.to(dev)
    _, fam = _profiled(lambda: L.call('cat_dwm7_fwd', C.byref(g), ops._p(xg), ops._p(scg), ops._p(shg), ops._p(w49), ops._p(bg), ops._p(y),
                                      ops._p(tab) if stats else None, ops._stream()))
    assert fam.get('dwconv_fwd', 0) == 1, fam
    yc, tc = y.cpu(), tab.cpu()
    _columns(yc, range(c), range(c), (case, 'y'))
    _tail(yflat, (case, 'y'))
    _tail(tflat, (case, 'table'))
    got = {'y': _nchw(yc, 0, c)}
    if stats:
        _columns(tc, range(c), range(c), (case, 'table'))
        got['sum'], got['m2'] = tc[:, 0, :c], tc[:, 1, :c]
    else:
        assert bool((tc == SENTINEL).all())
    _cmp('D7', case[1:], got, want)


BRANCHES = [(5, 7), (12, 3), (7, 7)]      # (channels, k): channel offsets 0, 8, 20 of a 28-channel concatenation
# (branches, plane, reflect)
BWD_CASES = [(tuple(BRANCHES), 0, 1), (tuple(BRANCHES), 0, 0), (tuple(BRANCHES), 2, 1), (((72, 7),), 1, 1)]


@functools.lru_cache(maxsize=None)
def _bwd_inputs(case):
    br, plane, reflect = case
    n, h, w = PLANES[plane]
    c4 = sum(cs4(c) for c, k in br)
    a, dz = torch.zeros((n, c4, h, w)), torch.zeros((n, c4, h, w))      # padding channels of a branch: zeros, as the product leaves them
    ws, prev, o = [], [], 0
    for i, (c, k) in enumerate(br):
        a[:, o:o + c] = F.relu(detfill.normal((n, c, h, w), 1100 + i) + 0.3)
        dz[:, o:o + c] = detfill.normal((n, c, h, w), 1120 + i)
        ws.append(detfill.normal((c, k, k), 1140 + i, 1.0 / k))
        prev.append(detfill.normal((c, k, k), 1160 + i, float((n * h * w) ** 0.5)))
        o += cs4(c)
    return a, dz, ws, prev


@pytest.mark.gpu
@pytest.mark.parametrize('case', BWD_CASES, ids=lambda c: 'nq%d-plane%d-refl%d' % (sum(cs4(m) for m, k in c[0]) // 4, c[1], c[2]))
def test_dwm7_bwd(dev, case):
    from cat_amd import _lib as L, ops
    br, plane, reflect = case
    a32, dz, ws, prev = _bwd_inputs(case)
    n, c4, h, w = a32.shape
    nq = c4 // 4
    a = a32.double().requires_grad_(True)
    wl = [wt.double().unsqueeze(1).requires_grad_(True) for wt in ws]
    zs, gz, c0s, o = [], [], [], 0
    for (c, k), wt in zip(br, wl):
        zs.append(F.conv2d(_pad(a[:, o:o + c], k // 2, reflect), wt, groups=c))
        gz.append(dz[:, o:o + c].double())
        c0s.append(o)
        o += cs4(c)
    grads = torch.autograd.grad(zs, [a] + wl, gz)
    want = {'da': grads[0]}
    for i, gw in enumerate(grads[1:]):
        want['dw%d' % i] = gw.squeeze(1)
        want['dwacc%d' % i] = prev[i].double() + gw.squeeze(1)
    acs, zcs, dacs = c4 + 4, c4 + 8, c4 + 12
    ks = [k for c, k in br for _ in range(cs4(c) // 4)]
    wpad = [F.pad(wt, (0, 0, 0, 0, 0, cs4(wt.shape[0]) - wt.shape[0])) for wt in ws]      # zero filters in a branch's padding channels
    w49 = _w49(frame49(wpad, [k for c, k in br]), dev)
    ag, zg = _nhwc_buffer(a32, acs, dev), _nhwc_buffer(dz, zcs, dev)
    g = _dwm_geom(n, h, w, nq, acs, zcs, 0, 0, reflect, 0, ks)
    nb = len(br)
    IA = C.c_int * nb
    nbytes = int(L.query('cat_dwm7_bwd_ws_bytes', C.byref(g)))
    assert nbytes == n * cdiv(h, 8) * cdiv(w, 16) * 49 * c4 * 4
    got = {}
    for accumulate in (0, 1):
        dflat, da = _sentinel((n, h, w, dacs), dev)
        wsflat, wsbuf = _sentinel((nbytes // 4,), dev, NAN)
        dsts = [_sentinel((c * k * k,), dev, NAN) for c, k in br]
        if accumulate:
            for (flat, d), p in zip(dsts, prev):
                d.copy_(p.reshape(-1))
        _, fam = _profiled(lambda: L.call('cat_dwm7_bwd', C.byref(g), ops._p(ag), ops._p(zg), ops._p(w49), ops._p(da), dacs, nb, IA(*c0s),
                                          IA(*[c for c, k in br]), IA(*[k for c, k in br]), (C.c_void_p * nb)(*[d.data_ptr() for flat, d in dsts]),
                                          accumulate, ops._p(wsbuf), ops._stream()))
        assert fam.get('dwconv_bwd', 0) == 1, fam
        dc = da.cpu()
        _columns(dc, range(c4), range(c4), (case, 'da'))
        _tail(dflat, (case, 'da'))
        _tail(wsflat, (case, 'workspace'))
        assert bool(torch.isfinite(wsbuf).all()), 'every partial of the workspace is written'
        if not accumulate:
            got['da'] = _nchw(dc, 0, c4)
        else:
            assert torch.equal(_nchw(dc, 0, c4), got['da']), 'accumulate only concerns the filter gradient'
        for i, ((c, k), (flat, d)) in enumerate(zip(br, dsts)):
            _tail(flat, (case, 'dw', i))
            got[('dwacc%d' if accumulate else 'dw%d') % i] = d.cpu().view(c, k, k)
    _cmp('D7', case[1:], got, want)


@pytest.mark.gpu
def test_dwm7_bwd_refuses_19_quads(dev):
    from cat_amd import _lib as L, ops
    n, h, w, nq = 1, 8, 16, 19
    c = 4 * nq
    g = _dwm_geom(n, h, w, nq, c, c, c, 0, 0, 0, [7] * nq)
    xg, zg, w49 = torch.zeros((n, h, w, c), device=dev), torch.zeros((n, h, w, c), device=dev), torch.zeros((49, c), device=dev)
    yflat, y = _sentinel((n, h, w, c), dev)
    tflat, tab = _sentinel((c * 49,), dev)
    wsb = torch.zeros(49 * c, device=dev)
    with pytest.raises(RuntimeError, match='dwm'):
        L.call('cat_dwm7_bwd', C.byref(g), ops._p(xg), ops._p(zg), ops._p(w49), ops._p(y), c, 1, (C.c_int * 1)(0), (C.c_int * 1)(c), (C.c_int * 1)(7),
               (C.c_void_p * 1)(tab.data_ptr()), 0, ops._p(wsb), ops._stream())
    torch.cuda.synchronize()
    assert bool((yflat == SENTINEL).all()) and bool((tflat == SENTINEL).all())


@pytest.mark.gpu
def test_prep_kind5_writes_the_7x7_frame(dev):
    """depthwise filters [C][k][k] of three branches (k = 7, 3, 5) -> one [49][cs] frame, bit for bit the frame built on the host"""
    br = [(5, 7), (12, 3), (6, 5)]
    ws = [detfill.normal((c, k, k), 1200 + i) for i, (c, k) in enumerate(br)]
    cs = sum(cs4(c) for c, k in br)
    flat, dst = _sentinel((49, cs), dev, 0.0)
    wg = [wt.to(dev).contiguous() for wt in ws]
    jobs, o = [], 0
    for (c, k), t in zip(br, wg):
        jobs.append(dict(kind=5, srcs=[t.data_ptr()], dst=dst.data_ptr(), Nn=c, ks=k, col0=o, cs=cs, threads=c * k * k))
        o += cs4(c)
    _prep_run(jobs, dev)
    wpad = [F.pad(wt, (0, 0, 0, 0, 0, cs4(wt.shape[0]) - wt.shape[0])) for wt in ws]
    want = frame49(wpad, [k for c, k in br]).permute(1, 2, 0).reshape(49, cs)
    assert torch.equal(dst.cpu(), want)
    _tail(flat, 'frame')
