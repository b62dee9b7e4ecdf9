"""The one-launch norm kernels of small statistic groups (csrc/norm_resident.hip) through cat_norm_fwd / cat_norm_bwd against float64, with the
runner, references and bars of the three-launch path (tests/test_streaming_kernels_gpu.py: _norm_run, _norm_ref, _norm_inputs, _cmp, NORM_BARS,
ORIGIN_BARS -- imported, not copied; no new tolerance).

1  forward and backward against float64 with the switch on, cat_norm_launches asserting that the case is in the domain: one pixel per group, a
   group of exactly the forward / backward limit, pixel counts that are no multiple of the pixel lanes, C = 3 in cs 4, C = 18 in cs 20 (ragged last
   slab), two full slabs, BatchNorm with N = 3 (running statistics, num_batches_tracked == 1), BatchNorm with shards = 2 on N = 3 (short last
   group), InstanceNorm with running statistics, activations none / ReLU / LeakyReLU, with and without affine, accumulate, no parameter gradients,
   the origin case and one with mean 1e3 and standard deviation 1 (both at ORIGIN_BARS).  Padding channels of y and dx are 0, the guard tails are
   intact, a second run is bit-identical (_norm_run and _ext_run check the first two, every test the third).
2  the dispatch is observable: a sentinel-filled workspace survives an in-domain forward and loses its partial sums with the switch off;
   cat_norm_launches 1 / 3 / 3 beyond either limit / 2 with parameter gradients over two groups.
3  on against off within twice the bars, each within the bars of float64.
4  a torch.cuda.graph of one forward and one backward, replayed twice, bit-identical to the eager run.
5  cat_amd.nn.InstanceNorm2d / BatchNorm2d with LeakyReLU through autograd against torch on the host in float64, switch on and off.

Slab geometry (csrc/norm_plan.h): 256 lanes = zq quads x 256 / zq pixel lanes, zq = 4 (2, 1 for cs 8, 4) while the pixels of a group fit 16
per lane, else 2, else 1."""
import ctypes as C

import pytest
import torch

from oracle import detfill
from test_kernels_gpu import TOL, rel
import test_streaming_kernels_gpu as sk
from test_streaming_kernels_gpu import (ACT_LRELU, ACT_NONE, ACT_RELU, EPS, MOM, NORM_BARS, ORIGIN_BARS, SENTINEL, SLOPE, _cmp, _in, _nchw, _nhwc,
                                        _norm_id, _norm_inputs, _norm_ref, _norm_run, _out, _p, _same, _stream, _tail, cs4, norm_plan)


@pytest.fixture(scope='module')
def dev():
    sk._lib()
    return torch.device('cuda:0')


@pytest.fixture
def L():
    """the library with the one-launch kernels switched on; the previous value comes back afterwards"""
    lib = sk._lib()
    prev = lib.query('cat_norm_set_resident', 1)
    yield lib
    lib.query('cat_norm_set_resident', prev)


def _caps(lib):
    return lib.query('cat_norm_resident_max_pixels', 0), lib.query('cat_norm_resident_max_pixels', 1)


def _geom(lib, case, shards=0):
    mode, c, n, h, w, act, flags = case
    return lib.NormGeom(n, h * w, c, cs4(c), lib.NORM_INSTANCE if mode == 'instance' else lib.NORM_BATCH, EPS, MOM, act, SLOPE, shards)


def _launches(lib, case, backward, params, shards=0):
    g = _geom(lib, case, shards)
    return lib.query('cat_norm_launches', C.byref(g), int(backward), int(params))


def _in_domain(lib, case, shards=0):
    """the forward is one launch; the backward, where the case has one, is one launch plus the parameter-gradient launch over several groups"""
    mode, c, n, h, w, act, flags = case
    assert _launches(lib, case, 0, 0, shards) == 1, case
    if 'fwd' not in flags:
        params = 'nodparam' not in flags
        groups = n if mode == 'instance' else max(1, min(shards, n))
        assert _launches(lib, case, 1, params, shards) == (2 if params and groups > 1 else 1), case


def _device_inputs(dev, case, inputs=None):
    mode, c, n, h, w, act, flags = case
    x, ga, be, gy, pre = inputs or _norm_inputs(case)
    cs = cs4(c)
    xg, dyg = _in(_nhwc(x, cs), dev), _in(_nhwc(gy, cs), dev)
    gag, beg = (_in(ga, dev), _in(be, dev)) if 'noaffine' not in flags else (None, None)
    return xg, dyg, gag, beg, [t.to(dev) for t in pre]


def _check(L, dev, case, section='R'):
    """_norm_run twice against the float64 reference at the three-launch path's bars"""
    _in_domain(L, case)
    args = _device_inputs(dev, case)
    got = _norm_run(L, dev, case, *args)
    origin = 'origin' in case[6]
    _cmp(section + ('-origin' if origin else ''), _norm_id(case), got, _norm_ref(case, torch.float64), ORIGIN_BARS if origin else NORM_BARS,
         inst=case[0] == 'instance')
    _same(got, _norm_run(L, dev, case, *args), case)
    return got


# the limits are fixed by the issue's bounds; the tables below need them at import time, test_limits_are_what_the_tables_assume holds them to the library
FWDCAP, BWDCAP = 4096, 4096

SIZE_CASES = [
    ('instance', 3, 2, 1, 1, ACT_NONE, ''),                    # one pixel per group: variance 0, rstd = 1 / sqrt(eps); C = 3 in cs 4
    ('instance', 18, 1, 64, FWDCAP // 64, ACT_LRELU, 'fwd'),   # exactly the forward limit; C = 18 in cs 20: five one-quad slabs
    ('instance', 18, 1, 64, BWDCAP // 64, ACT_RELU, ''),       # exactly the backward limit, forward and backward
    ('instance', 18, 1, 32, 64, ACT_RELU, ''),                 # 2048 pixels: two-quad slabs, the last one ragged
    ('instance', 16, 2, 31, 65, ACT_NONE, ''),                 # 2015 pixels: no multiple of 64 / 128 lanes; two full two-quad slabs
    ('instance', 16, 2, 33, 65, ACT_NONE, ''),                 # 2145 pixels: no multiple of 256 lanes; four one-quad slabs
    ('batch', 24, 3, 7, 9, ACT_RELU, ''),                      # 189 pixels on 64 lanes: idle lanes in the last trip; one full and one half slab
    ('instance', 18, 2, 17, 33, ACT_LRELU, ''),                # four-quad slabs, the second one ragged (one quad of four)
    ('batch', 18, 3, 17, 33, ACT_LRELU, ''),                   # BatchNorm, N = 3: running statistics, num_batches_tracked == 1 (_norm_run)
]
FLAG_CASES = [
    ('batch', 7, 3, 6, 5, ACT_RELU, 'noaffine'),
    ('instance', 7, 3, 6, 5, ACT_NONE, 'noaffine'),
    ('batch', 7, 3, 6, 5, ACT_LRELU, 'nodparam'),
    ('instance', 7, 3, 6, 5, ACT_LRELU, 'nodparam'),
    ('batch', 7, 3, 6, 5, ACT_RELU, 'acc'),
    ('instance', 7, 3, 6, 5, ACT_RELU, 'acc'),
    ('batch', 8, 2, 64, 32, ACT_RELU, 'origin'),               # x = 8 + normal, the group's first pixel 0
    ('instance', 8, 2, 64, 64, ACT_RELU, 'origin'),
]


@pytest.mark.gpu
def test_limits_are_what_the_tables_assume(dev, L):
    assert _caps(L) == (FWDCAP, BWDCAP)


@pytest.mark.gpu
@pytest.mark.parametrize('case', SIZE_CASES + FLAG_CASES, ids=_norm_id)
def test_resident_against_float64(dev, L, case):
    got = _check(L, dev, case)
    if case[3] * case[4] == 1:
        assert rel(got['rstd'], torch.full_like(got['rstd'], EPS ** -0.5)) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['instance', 'batch'])
def test_mean_1e3_std_1_holds_the_origin_bars(dev, L, mode, monkeypatch):
    """|mean| = 1e3 std: sums of squares about 0 would lose every digit of the variance; deviations about the mean of the resident data do not.
    Observed on an MI355X: y 2.4e-5 per channel and dgamma 3.7e-5 (the float32 mean of 2048 values near 1e3 is off by ~2e-5 standard deviations),
    rstd and dx below 2e-6; every other case of this file stays below 1e-6."""
    case = (mode, 8, 2, 32, 64, ACT_RELU, 'origin')

    def inputs(cs):
        x, ga, be, gy, pre = _norm_inputs(cs[:6] + ('',))
        return 1e3 + detfill.normal(tuple(x.shape), 719), ga, be, gy, pre
    monkeypatch.setattr(sk, '_norm_inputs', inputs)      # _norm_ref reads its inputs there
    _in_domain(L, case)
    args = _device_inputs(dev, case, inputs(case))
    got = _norm_run(L, dev, case, *args)
    want = _norm_ref(case, torch.float64)
    assert abs(float(want['mean'].mean()) - 1e3) < 0.1 and abs(float(want['rstd'].mean()) - 1.0) < 0.1
    _cmp('R-1e3', _norm_id(case), got, want, ORIGIN_BARS, inst=mode == 'instance')
    _same(got, _norm_run(L, dev, case, *args), case)


def _ext_ref(x, ga, be, gy, groups, act, dtype):
    """float64 reference of a norm over `groups` = [(first sample, samples)]: a sharded BatchNorm, or an InstanceNorm (one sample per group)"""
    x, ga, be = (t.to(dtype).requires_grad_(True) for t in (x, ga, be))
    ys, means, rstds, uvars = [], [], [], []
    for n0, cnt in groups:
        xs = x[n0:n0 + cnt]
        mean = xs.mean((0, 2, 3), keepdim=True)
        var = ((xs - mean) ** 2).mean((0, 2, 3), keepdim=True)
        rstd = (var + EPS) ** -0.5
        ys.append(sk._act((xs - mean) * rstd * ga[None, :, None, None] + be[None, :, None, None], act))
        npix = xs.numel() // xs.shape[1]
        means.append(mean.detach().reshape(-1))
        rstds.append(rstd.detach().reshape(-1))
        uvars.append(var.detach().reshape(-1) * npix / max(npix - 1, 1))
    y = torch.cat(ys)
    y.backward(gy.to(dtype))
    return {'y': y.detach(), 'mean': torch.stack(means), 'rstd': torch.stack(rstds), 'dx': x.grad, 'dgamma': ga.grad, 'dbeta': be.grad}, means, uvars


def _ext_run(L, dev, case, shards, track, xg, dyg, gag, beg, groups):
    """cat_norm_fwd / cat_norm_bwd with cat_norm_t.shards or an InstanceNorm's running statistics -- what _norm_run has no argument for"""
    mode, c, n, h, w, act, flags = case
    cs, G = cs4(c), len(groups)
    g = _geom(L, case, shards)
    nws = L.query('cat_norm_ws_bytes', C.byref(g)) // 4
    wsf, ws = _out((nws,), dev)
    yf, y = _out((n, h, w, cs), dev)
    mf, mean = _out((G, c), dev)
    rf, rstd = _out((G, c), dev)
    rmf, rm = _out((c,), dev, 0.0)
    rvf, rv = _out((c,), dev, 1.0)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    L.call('cat_norm_fwd', C.byref(g), _p(xg), _p(gag), _p(beg), _p(y), _p(mean), _p(rstd), _p(rm) if track else None, _p(rv) if track else None,
           _p(nbt) if track and mode == 'batch' else None, _p(ws), _stream())
    dxf, dx = _out((n, h, w, cs), dev)
    dgf, dg = _out((c,), dev)
    dbf, db = _out((c,), dev)
    L.call('cat_norm_bwd', C.byref(g), _p(xg), _p(dyg), _p(gag), _p(beg), _p(mean), _p(rstd), _p(dx), _p(dg), _p(db), 0, _p(ws), _stream())
    torch.cuda.synchronize()
    for flat, what in ((wsf, 'ws'), (yf, 'y'), (mf, 'mean'), (rf, 'rstd'), (rmf, 'rm'), (rvf, 'rv'), (dxf, 'dx'), (dgf, 'dgamma'), (dbf, 'dbeta')):
        _tail(flat, (case, what))
    yc, dxc = y.cpu(), dx.cpu()
    assert bool((yc[..., c:] == 0.0).all()) and bool((dxc[..., c:] == 0.0).all()), (case, 'padding channels')
    return {'y': _nchw(yc, c), 'mean': mean.cpu(), 'rstd': rstd.cpu(), 'dx': _nchw(dxc, c), 'dgamma': dg.cpu(), 'dbeta': db.cpu(), 'rm': rm.cpu(),
            'rv': rv.cpu(), 'nbt': nbt.cpu()}


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['shards', 'instance-running'])
def test_sharded_batchnorm_and_instance_running_statistics(dev, L, kind):
    """BatchNorm with shards = 2 on N = 3: groups of 2 and 1 samples, running statistics from group 0, counted once.  InstanceNorm with
    running statistics: the batch mean of the per-instance means / unbiased variances (in_running_kernel stays the second launch)."""
    sharded = kind == 'shards'
    case = ('batch' if sharded else 'instance', 18, 3, 17, 33, ACT_LRELU, '')
    mode, c, n, h, w, act, flags = case
    shards = 2 if sharded else 0
    groups = [(0, 2), (2, 1)] if sharded else [(i, 1) for i in range(n)]
    _in_domain(L, case, shards)
    inputs = _norm_inputs(case)
    x, ga, be, gy, pre = inputs
    xg, dyg, gag, beg, _ = _device_inputs(dev, case, inputs)
    want, means, uvars = _ext_ref(x, ga, be, gy, groups, act, torch.float64)
    if sharded:
        want['rm'], want['rv'] = MOM * means[0], (1 - MOM) + MOM * uvars[0]
    else:
        want['rm'], want['rv'] = MOM * torch.stack(means).mean(0), (1 - MOM) + MOM * torch.stack(uvars).mean(0)
    got = _ext_run(L, dev, case, shards, True, xg, dyg, gag, beg, groups)
    assert int(got.pop('nbt')) == (1 if sharded else 0)
    _cmp('R-' + kind, _norm_id(case), got, want, NORM_BARS, inst=None)
    again = _ext_run(L, dev, case, shards, True, xg, dyg, gag, beg, groups)
    again.pop('nbt')
    _same(got, again, case)


# ================================================================================================ 2: the dispatch is observable
@pytest.mark.gpu
def test_dispatch_is_observable(dev, L):
    case = ('instance', 18, 2, 17, 33, ACT_LRELU, '')
    mode, c, n, h, w, act, flags = case
    p = norm_plan(mode, c, n, h, w)
    g = _geom(L, case)
    xg, dyg, gag, beg, preg = _device_inputs(dev, case)

    def forward():
        ws = torch.full((L.query('cat_norm_ws_bytes', C.byref(g)) // 4,), SENTINEL, device=dev)
        y, mean, rstd = torch.empty(n, h, w, p['cs'], device=dev), torch.empty(n, c, device=dev), torch.empty(n, c, device=dev)
        L.call('cat_norm_fwd', C.byref(g), _p(xg), _p(gag), _p(beg), _p(y), _p(mean), _p(rstd), None, None, None, _p(ws), _stream())
        torch.cuda.synchronize()
        return ws.cpu()
    assert _launches(L, case, 0, 0) == 1
    assert bool((forward() == SENTINEL).all()), 'an in-domain forward wrote to the workspace'
    assert L.query('cat_norm_set_resident', 0) == 1
    try:
        assert _launches(L, case, 0, 0) == 3 and _launches(L, case, 1, 0) == 3 and _launches(L, case, 1, 1) == 4
        ws = forward()
        assert not bool((ws[:p['G'] * p['nb'] * 2 * p['cs']] == SENTINEL).any()), 'the three launches left partial sums unwritten'
    finally:
        assert L.query('cat_norm_set_resident', 1) == 0
    fwdcap, bwdcap = _caps(L)
    assert _launches(L, ('instance', 8, 1, 1, fwdcap, 0, ''), 0, 0) == 1 and _launches(L, ('instance', 8, 1, 1, fwdcap + 1, 0, ''), 0, 0) == 3
    assert _launches(L, ('instance', 8, 1, 1, bwdcap, 0, ''), 1, 0) == 1 and _launches(L, ('instance', 8, 1, 1, bwdcap + 1, 0, ''), 1, 0) == 3
    assert _launches(L, ('batch', 8, 2, 1, fwdcap // 2 + 1, 0, ''), 0, 0) == 3      # BatchNorm: the batch is the group
    assert _launches(L, ('instance', 8, 2, 17, 33, 0, ''), 1, 1) == 2 and _launches(L, ('instance', 8, 2, 17, 33, 0, ''), 1, 0) == 1
    assert _launches(L, ('batch', 8, 2, 17, 33, 0, ''), 1, 1) == 1


# ================================================================================================ 3: on against off
@pytest.mark.gpu
@pytest.mark.parametrize('case', [SIZE_CASES[2], SIZE_CASES[-1], FLAG_CASES[5]], ids=_norm_id)
def test_on_against_off(dev, L, case):
    want = _norm_ref(case, torch.float64)
    args = _device_inputs(dev, case)
    _in_domain(L, case)
    on = _norm_run(L, dev, case, *args)
    L.query('cat_norm_set_resident', 0)
    try:
        assert _launches(L, case, 0, 0) == 3
        off = _norm_run(L, dev, case, *args)
    finally:
        L.query('cat_norm_set_resident', 1)
    inst = case[0] == 'instance'
    _cmp('R-on', _norm_id(case), on, want, NORM_BARS, inst=inst)
    _cmp('R-off', _norm_id(case), off, want, NORM_BARS, inst=inst)
    _cmp('R-on-off', _norm_id(case), on, off, {key: 2 * NORM_BARS.get(key, TOL) for key in want}, inst=inst)


# ================================================================================================ 4: graph replay
@pytest.mark.gpu
def test_graph_replay_is_bit_identical_to_the_eager_run(dev, L):
    case = ('instance', 18, 2, 17, 33, ACT_LRELU, '')
    mode, c, n, h, w, act, flags = case
    _in_domain(L, case)
    cs = cs4(c)
    g = _geom(L, case)
    xg, dyg, gag, beg, preg = _device_inputs(dev, case)
    ws = torch.zeros(L.query('cat_norm_ws_bytes', C.byref(g)) // 4, device=dev)
    bufs = {'y': (n, h, w, cs), 'mean': (n, c), 'rstd': (n, c), 'dx': (n, h, w, cs), 'dgamma': (c,), 'dbeta': (c,)}

    def run(o):
        L.call('cat_norm_fwd', C.byref(g), _p(xg), _p(gag), _p(beg), _p(o['y']), _p(o['mean']), _p(o['rstd']), None, None, None, _p(ws), _stream())
        L.call('cat_norm_bwd', C.byref(g), _p(xg), _p(dyg), _p(gag), _p(beg), _p(o['mean']), _p(o['rstd']), _p(o['dx']), _p(o['dgamma']),
               _p(o['dbeta']), 0, _p(ws), _stream())
    eager = {k: torch.full(s, float('nan'), device=dev) for k, s in bufs.items()}
    run(eager)
    torch.cuda.synchronize()
    out = {k: torch.full(s, float('nan'), device=dev) for k, s in bufs.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(out)
    for replay in range(2):
        for t in out.values():
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        _same({k: v.cpu() for k, v in eager.items()}, {k: v.cpu() for k, v in out.items()}, ('replay', replay))


# ================================================================================================ 5: through the modules
@pytest.mark.gpu
@pytest.mark.parametrize('resident', [True, False], ids=['on', 'off'])
@pytest.mark.parametrize('kind', ['instance', 'batch'])
def test_through_the_modules(dev, L, kind, resident):
    from cat_amd import nn as cnn, ops
    n, c, h, w = 2, 8, 8, 16
    ref = (torch.nn.InstanceNorm2d(c, affine=True) if kind == 'instance' else torch.nn.BatchNorm2d(c)).double()
    mod = cnn.InstanceNorm2d(c, affine=True) if kind == 'instance' else cnn.BatchNorm2d(c)
    with torch.no_grad():
        ref.weight.copy_(1.0 + 0.2 * detfill.normal((c,), 31))
        ref.bias.copy_(0.1 * detfill.normal((c,), 32))
    mod.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in ref.state_dict().items()})
    mod = mod.to(dev)
    ref.train(), mod.train()
    x, gy = detfill.normal((n, c, h, w), 40) * 1.5 + 0.7, detfill.normal((n, c, h, w), 50)
    xr = x.double().requires_grad_(True)
    yr = torch.nn.functional.leaky_relu(ref(xr), SLOPE)
    yr.backward(gy.double())
    prev = ops.set_norm_resident(resident)
    try:
        assert prev is True
        geom = L.NormGeom(n, h * w, c, cs4(c), L.NORM_INSTANCE if kind == 'instance' else L.NORM_BATCH, EPS, MOM, ACT_LRELU, SLOPE, 0)
        assert L.query('cat_norm_launches', C.byref(geom), 0, 0) == (1 if resident else 3)
        xg = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
        y = mod(xg, fuse_act=cnn.LeakyReLU(SLOPE))
        y.backward(ops.to_nhwc(gy.to(dev)))
        torch.cuda.synchronize()
    finally:
        assert ops.set_norm_resident(prev) is bool(resident)
    for what, got, want in (('y', y, yr), ('dx', xg.grad, xr.grad), ('dgamma', mod.weight.grad, ref.weight.grad), ('dbeta', mod.bias.grad, ref.bias.grad)):
        d = rel(got, want)
        print('modules %s %s %s rel %.3g' % (kind, 'on' if resident else 'off', what, d))
        assert d < TOL, (what, d)
    if kind == 'batch':
        assert rel(mod.running_mean, ref.running_mean) < TOL and rel(mod.running_var, ref.running_var) < TOL
        assert int(mod.num_batches_tracked) == 1
