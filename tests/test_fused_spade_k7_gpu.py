"""GPU: the fused GauGAN units (cat_amd/fused_spade.py) at the reference's default kernel sizes 3 5 7, under CAT_FUSED_SPADE_K7 / set_k7 -- the
main six-branch unit of SPADEInvertedResidualChannels and the gamma|beta net of its InceptionSPADE on the shared pipeline with the 7 x 7
depthwise frame, the wide-patch LDS-tile convs and, where the widths allow, ONE cat_tstage1n7_fwd for stage 1 and ONE cat_tstage1n7_dgrad
for the second convs' input gradients (csrc/conv_s1n7.hip).

Follows tests/test_spade_gpu.py::test_fused_spade_units_match_general_path with its cases, shapes and bars (output 2e-5, input gradient
1e-4, parameter gradients 1e-3 of the largest, running statistics): fused against the per-layer path of a deep copy; then the same
modules against the reference's own float64 run (tests/golden/spade_k7_unit.npz, tools/make_golden_spade_k7.py), the frozen form, a whole
student generator, and the launch logs with the switch on and off.

ReLU kinks.  Two evaluations of a unit land a pre-activation that lies within round-off of zero on different sides, which moves one
element of dx by 1e-2 (tools/debug/fused_spade_dbg.py).  The input seed below was chosen on the CPU, with the float64 oracle
(oracle/ref_spade_cpu.py) against its float32 twin: over every element of every ReLU input of the unit (the modulation and the nine
hidden norms of each of its two nets), |pre-activation (float64)| / |float32 - float64| -- how many of its own round-offs the element is
away from its kink.  SEED_X = 600 gives at least 12.2 for the five (fin, fout, channels) of CASES (80.5, 36.5, 17.8, 90.8, 12.2; seed 601
has 7.2 and seed 603 1.5 in one case); the fixture's input seed 2300 gives 319.9 and 71.0 for its two modules.  `_kink_margin` is that
check; the first test below repeats it without a GPU for the seeds in use and asserts at least MIN_MARGIN = 8 round-offs."""
import copy
import functools
import json
from argparse import Namespace
from unittest import mock

import pytest
import torch

import helpers as H
from oracle import detfill
from oracle import ref_spade_cpu as R

CASES = [(48, 24, None, False), (24, 24, None, False), (40, 16, [30, 6, 12], False), (40, 16, [30, 6, 12], True), (24, 24, [6, 6, 6], True),
         (40, 16, [96, 36, 60], True)]
N, HH, WW = 2, 24, 40
SEED_X = 600
KS = [3, 5, 7]
MIN_MARGIN = 8.0      # round-offs between the nearest pre-activation and its kink


def dev():
    return torch.device('cuda', 0)


@functools.lru_cache(maxsize=None)
def _opt():
    from test_spade_gpu import fixture
    return fixture()[1]


def _o(channels, ks=KS):
    o = Namespace(**vars(_opt()))
    o.norm_G, o.channels, o.kernel_sizes = 'spadesyncbatch3x3', channels, list(ks)
    return o


def _block(fin, fout, channels, seed=411, ks=KS):
    from cat_amd.inception_modules import SPADEInvertedResidualChannels
    o = _o(channels, ks)
    blk = SPADEInvertedResidualChannels(fin, fout, o)
    sd = detfill.fill_state_dict(blk.state_dict(), seed, gamma_abs_normal=True)
    blk.load_state_dict(sd)
    return blk, sd, o


def _seg(o, n, h, w, seed=413):
    return (detfill.normal((n, o.semantic_nc, h // 4, w // 4), seed) > 0.8).float().repeat_interleave(4, 2).repeat_interleave(4, 3)


def _kink_margin(sd, x, seg):
    """over every element of every ReLU input of the unit: min |pre-activation (float64)| / |float32 - float64| of that element"""
    runs = {}
    relu = torch.nn.functional.relu
    for dt in (torch.float64, torch.float32):
        pres = []

        def rec(t, *a, pres=pres, **k):
            pres.append(t.detach().double())
            return relu(t, *a, **k)
        with mock.patch.object(R.F, 'relu', rec), torch.no_grad():
            R.spade_inverted_residual_channels({'b.' + k: (v.clone().to(dt) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}, 'b',
                                               x.to(dt), seg.to(dt), True, False)
        runs[dt] = pres
    assert len(runs[torch.float64]) == len(runs[torch.float32]) > 0
    return min(float((a.abs() / (a - b).abs().clamp_min(1e-30)).min()) for a, b in zip(runs[torch.float64], runs[torch.float32]))


@functools.lru_cache(maxsize=None)
def _golden():
    return H.load('spade_k7_unit.npz')


def test_no_pre_activation_sits_on_a_relu_kink():
    for fin, fout, channels, owned in CASES:
        if owned and (fin, fout, channels, False) in CASES:
            continue
        blk, sd, o = _block(fin, fout, channels)
        m = _kink_margin(sd, detfill.normal((N, fin, HH, WW), SEED_X), _seg(o, N, HH, WW))
        print('kink margin', fin, fout, channels, '%.1f' % m)
        assert m >= MIN_MARGIN, (fin, fout, channels, m)
    g = _golden()
    for tag in ('u', 'p'):
        blk, sd, o = _block(int(g['fin']), int(g['fout']), json.loads(str(g[tag + '_channels'])), int(g[tag + '_seed']))
        m = _kink_margin(sd, detfill.normal((int(g['n']), int(g['fin']), int(g['h']), int(g['w'])), int(g['seed_x'])), torch.from_numpy(g['seg']).float())
        print('kink margin fixture', tag, '%.1f' % m)
        assert m >= MIN_MARGIN, (tag, m)


# ------------------------------------------------------------------------------------------------------------------ GPU
def rel(a, b, floor=0.0):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-30))


def nhwc(t):
    from cat_amd import ops
    return ops.to_nhwc(t.to(dev()))


class _K7:
    """set_k7(on) + the LDS-tile threshold of the test shapes, restored on exit"""

    def __init__(self, on=True, min_tiles=1):
        self.on, self.min_tiles = on, min_tiles

    def __enter__(self):
        from cat_amd import fused_spade, ops
        self.old = fused_spade.set_k7(self.on), ops.set_tconv_min_tiles(self.min_tiles)

    def __exit__(self, *exc):
        from cat_amd import fused_spade, ops
        fused_spade.set_k7(self.old[0])
        ops.set_tconv_min_tiles(self.old[1])
        fused_spade.set_enabled(True)


def _want_n7(p):
    """(stage 1 in one launch?, second-conv input gradients in one launch?) for a plan, by the predicate's mirror"""
    from test_stage1n7_gpu import supported
    by_k = {g['k']: g['width'] for g in p.groups}
    fwd = set(by_k) == {1, 3, 5, 7} and supported(*[by_k[k] for k in (7, 5, 3, 1)])
    r = {k: [b for b in p.res if b['k'] == k] for k in (7, 5, 3)}
    dg = all(len(v) == 1 for v in r.values()) and bool(p.dws) and supported(r[7][0]['w1'], r[5][0]['w1'], r[3][0]['w1'], p.hcd)
    return fwd, dg


def _grads_match(blk, ref, bar=1e-3):
    from cat_amd.inception_modules import ConvSyncBNReLU
    gtop = max(float(q.grad.abs().max()) for q in ref.parameters() if q.grad is not None)
    # a conv bias directly in front of a batch norm has exact gradient 0 (round-off in both paths)
    zero_grad = {id(m.conv.bias) for m in ref.modules() if isinstance(m, ConvSyncBNReLU) and m.conv.bias is not None}
    bad = {}
    for (k, pa), (_, pb) in zip(blk.named_parameters(), ref.named_parameters()):
        assert (pa.grad is None) == (pb.grad is None), k
        if pb.grad is None or id(pb) in zero_grad:
            continue
        err = float((pa.grad - pb.grad).abs().max()) / max(float(pb.grad.abs().max()), 1e-3 * gtop)
        if err > bar:
            bad[k] = err
    assert not bad, bad


def _buffers_match(blk, ref):
    for (k, ba), (_, bb) in zip(blk.named_buffers(), ref.named_buffers()):
        if ba.dtype.is_floating_point:
            assert rel(ba, bb, 1e-6) < 1e-5, k
        else:
            assert torch.equal(ba, bb), k


@pytest.mark.gpu
@pytest.mark.parametrize('fin,fout,channels,owned', CASES)
def test_fused_spade_k7_units_match_general_path(fin, fout, channels, owned):
    from test_fused_launch_order_gpu import _Recorder, _names
    from cat_amd import fused_spade
    blk, sd, o = _block(fin, fout, channels)
    blk = blk.to(dev()).train()
    ref = copy.deepcopy(blk)
    if owned:      # parameters and gradients are slices of FusedAdam's flat buffers (a one-channel conv weight is stored unpadded there)
        from cat_amd.optim import FusedAdam
        for net in (blk, ref):
            FusedAdam(list(net.parameters()), lr=0.0).zero_grad()
    x, seg, gy = detfill.normal((N, fin, HH, WW), SEED_X), _seg(o, N, HH, WW), detfill.normal((N, fout, HH, WW), 414)
    before = dict(fused_spade.STATS)
    with _K7():
        xa, sa = nhwc(x).detach().requires_grad_(True), nhwc(seg)
        assert fused_spade.applicable(blk.res_ops, blk.dw_ops, xa, True) and fused_spade.applicable(blk.spade.res_ops, blk.spade.dw_ops, sa, True)
        ya = blk(xa, sa)
        ya.backward(nhwc(gy))
        plans = fused_spade.units_of(blk)
        assert getattr(blk, '_cat_fused_main', None) in plans and getattr(blk.spade, '_cat_fused_gb', None) in plans and len(plans) == 2
        assert fused_spade.STATS['train_fwd'] - before['train_fwd'] == 2 and fused_spade.STATS['bwd'] - before['bwd'] == 2
        assert all(p.stage1_n7 and p.fs == 7 for p in plans)
        fused_spade.set_enabled(False)
        xb, sb = nhwc(x).detach().requires_grad_(True), nhwc(seg)
        yb = ref(xb, sb)
        yb.backward(nhwc(gy))
        fused_spade.set_enabled(True)
        torch.cuda.synchronize()
        assert rel(ya, yb) < 2e-5, rel(ya, yb)
        assert rel(xa.grad, xb.grad) < 1e-4, rel(xa.grad, xb.grad)
        _grads_match(blk, ref)
        _buffers_match(blk, ref)
        # the steady-state launch log (second step): one cat_tstage1n7_fwd / one cat_tstage1n7_dgrad per plan whose widths the predicate admits
        for q in blk.parameters():
            q.grad = None
        rec = _Recorder()
        with rec:
            blk(nhwc(x).detach().requires_grad_(True), sa).backward(nhwc(gy))
            torch.cuda.synchronize()
        names = _names(rec.calls)
        want = [_want_n7(p) for p in plans]
        assert names.count('cat_tstage1n7_fwd') == sum(f for f, d in want) and names.count('cat_tstage1n7_dgrad') == sum(d for f, d in want), (want, names)
        for p, (f, d) in zip(plans, want):
            assert (p.s1d7 is not None) == d and (p.s1d is None or not d)
        if channels is not None:      # the pruned widths are inside the kernel's domain: both plans take both launches
            assert want == [(True, True), (True, True)], want
        assert 'cat_dwm7_fwd' in names and 'cat_dwm7_bwd' in names and 'cat_dwm_fwd' not in names
        # under no_grad (the D step's fake image) the fused forward equals the general one as well
        with torch.no_grad():
            y1 = blk(nhwc(x), nhwc(seg))
            fused_spade.set_enabled(False)
            y2 = ref(nhwc(x), nhwc(seg))
            fused_spade.set_enabled(True)
        assert rel(y1, y2) < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['u', 'p'])
def test_fused_spade_k7_units_match_the_reference(tag):
    """against the reference's float64 run of the same module (tests/golden/spade_k7_unit.npz)"""
    import numpy as np
    from cat_amd import fused_spade
    g = _golden()
    assert list(g['kernel_sizes']) == KS and int(g['semantic_nc']) == _opt().semantic_nc
    fin, fout, n, h, w = (int(g[k]) for k in ('fin', 'fout', 'n', 'h', 'w'))
    blk, sd, o = _block(fin, fout, json.loads(str(g[tag + '_channels'])), int(g[tag + '_seed']))
    assert [[k, list(v.shape)] for k, v in sd.items()] == json.loads(str(g[tag + '_shapes']))      # the reference's keys, order and shapes
    chk = lambda t: np.array([t.double().sum().item(), t.double().abs().sum().item(), (t.double() ** 2).sum().item()])
    np.testing.assert_allclose(np.stack([chk(v) for v in sd.values()]), g[tag + '_sd_checks'], rtol=1e-12, atol=0)      # ... and values
    x, gy = detfill.normal((n, fin, h, w), int(g['seed_x'])), detfill.normal((n, fout, h, w), int(g['seed_gy']))
    np.testing.assert_allclose(chk(x), g['x_checks'], rtol=1e-12, atol=0)
    np.testing.assert_allclose(chk(gy), g['gy_checks'], rtol=1e-12, atol=0)
    seg = torch.from_numpy(g['seg']).float()
    blk = blk.to(dev()).train()
    before = dict(fused_spade.STATS)
    with _K7():
        xa = nhwc(x).detach().requires_grad_(True)
        ya = blk(xa, nhwc(seg))
        ya.backward(nhwc(gy))
        torch.cuda.synchronize()
    assert fused_spade.STATS['train_fwd'] - before['train_fwd'] == 2 and fused_spade.STATS['bwd'] - before['bwd'] == 2
    assert rel(ya, torch.from_numpy(g[tag + '_y'])) < 2e-5
    assert rel(xa.grad, torch.from_numpy(g[tag + '_dx'])) < 1e-4
    names, goff, grads, gnorm = json.loads(str(g[tag + '_params'])), g[tag + '_goff'], g[tag + '_grads'], g[tag + '_gnorm']
    params = dict(blk.named_parameters())
    assert list(params) == names
    gtop = float(np.abs(grads).max())
    stride = lambda numel: 1 if numel <= int(g['sample']) else -(-numel // int(g['sample']))
    bad = {}
    for i, k in enumerate(names):
        if '.0.conv.bias' in k or '.1.conv.bias' in k and 'dw_ops' in k:
            continue      # a conv bias directly in front of a batch norm has exact gradient 0 (round-off on both sides)
        got = params[k].grad.detach().cpu().double().reshape(-1)
        want = torch.from_numpy(grads[goff[i]:goff[i + 1]]).double()
        err = float((got[::stride(got.numel())] - want).abs().max()) / max(float(want.abs().max()), 1e-3 * gtop)
        nerr = abs(float(got.norm()) - float(gnorm[i])) / max(float(gnorm[i]), 1e-3 * gtop)
        if err > 1e-3 or nerr > 1e-3:
            bad[k] = (err, nerr)
    assert not bad, bad
    flat, o_ = torch.from_numpy(g[tag + '_bufs']).double(), 0
    bufs = dict(blk.named_buffers())
    assert [[k, list(b.shape)] for k, b in bufs.items()] == json.loads(str(g[tag + '_buffers']))
    for k, b in bufs.items():
        want = flat[o_:o_ + b.numel()].reshape(b.shape)
        o_ += b.numel()
        if b.dtype.is_floating_point:
            assert rel(b, want, 1e-6) < 1e-5, k
        else:
            assert torch.equal(b.cpu().double(), want), k


@pytest.mark.gpu
@pytest.mark.parametrize('fin,fout,channels', [(48, 24, None), (40, 16, [30, 6, 12])])
def test_fused_spade_k7_units_frozen_match_general_path(fin, fout, channels):
    from cat_amd import fused_spade
    blk, sd, o = _block(fin, fout, channels, seed=421)
    blk = blk.to(dev()).eval()
    ref = copy.deepcopy(blk)
    x, seg = detfill.normal((N, fin, HH, WW), SEED_X), _seg(o, N, HH, WW)
    before = dict(fused_spade.STATS)
    with _K7(), torch.no_grad():
        assert fused_spade.applicable(blk.res_ops, blk.dw_ops, nhwc(x), False)
        y1 = blk(nhwc(x), nhwc(seg))
        assert fused_spade.STATS['frozen_fwd'] - before['frozen_fwd'] == 2 and fused_spade.STATS['train_fwd'] == before['train_fwd']
        fused_spade.set_enabled(False)
        y2 = ref(nhwc(x), nhwc(seg))
        fused_spade.set_enabled(True)
        torch.cuda.synchronize()
    assert rel(y1, y2) < 2e-5
    _buffers_match(blk, ref)      # a frozen unit writes no statistics


@pytest.mark.gpu
def test_student_generator_at_357_matches_the_per_layer_path():
    """One InceptionSPADEGenerator student with kernel sizes 3 5 7, ngf 8, train forward + backward, fused against per-layer with the bars of
    tests/test_spade_gpu.py::test_generator_forward_backward (1e-3 for the image, the tapped activations and the running statistics,
    check_grads for the parameters).  Output 32 x 64: the smallest plane the generator admits at aspect ratio 2 (its latent map is
    crop_size / 32 wide and half as high: 2 x 1).  The LDS-tile threshold is three 8 x 16 tiles over the batch: the blocks on planes of several
    tiles (up_2, up_3 at 16 x 32 and 32 x 64) take the fused units, the five on planes of at most one tile run layer by layer."""
    from test_spade_gpu import check_grads
    from cat_amd import fused_spade, networks
    o = _o(None)
    o.ngf, o.crop_size, o.aspect_ratio, o.num_upsampling_layers = 8, 64, 2.0, 'normal'
    G = networks.define_G(o.input_nc, 3, 8, 'inception_spade', 'instance', 0, 'xavier', 0.02, [0], opt=o)
    G.load_state_dict(detfill.fill_state_dict(G.state_dict(), 431, gamma_abs_normal=True))
    G = G.train()
    ref = copy.deepcopy(G)
    h, w = 32, 64
    seg = _seg(o, 2, h, w, 433)
    r = detfill.normal((2, 3, h, w), 434)
    taps = None
    out = {}
    before = dict(fused_spade.STATS)
    with _K7(min_tiles=3):
        for tag, net in (('fused', G), ('layers', ref)):
            fused_spade.set_enabled(tag == 'fused')
            y, acts = net(nhwc(seg), mapping_layers=R.MAPPING_LAYERS)
            if taps is None:
                taps = [detfill.normal(tuple(acts[k].shape), 440 + i) for i, k in enumerate(R.MAPPING_LAYERS)]
            torch.autograd.backward([y] + [acts[k] for k in R.MAPPING_LAYERS], [nhwc(r)] + [nhwc(t) for t in taps])
            out[tag] = (y, acts)
            if tag == 'fused':
                ran = fused_spade.STATS['train_fwd'] - before['train_fwd']
        fused_spade.set_enabled(True)
        torch.cuda.synchronize()
    assert tuple(out['fused'][0].shape[2:]) == (h, w) and ran == 4 and fused_spade.STATS['bwd'] - before['bwd'] == 4      # 2 blocks x 2 units
    assert len(fused_spade.units_of(G)) == 4 and not fused_spade.units_of(ref)
    assert rel(out['fused'][0], out['layers'][0]) < 1e-3
    for k in R.MAPPING_LAYERS:
        assert rel(out['fused'][1][k], out['layers'][1][k]) < 1e-3, k
    check_grads(G.named_parameters(), {k: q.grad.detach().cpu() for k, q in ref.named_parameters() if q.grad is not None})
    for k in ('head_0.spade.param_free_norm.running_mean', 'up_3.res_ops.1.0.norm.running_var', 'fc_norm.running_var'):
        assert rel(G.state_dict()[k], ref.state_dict()[k]) < 1e-3, k


def _log(blk, x, seg, gy, k7, enabled=True):
    """the launch log of the second forward + backward of a fresh copy of blk"""
    from test_fused_launch_order_gpu import _Recorder
    from cat_amd import fused_spade
    net = copy.deepcopy(blk)
    with _K7(k7):
        fused_spade.set_enabled(enabled)
        rec = _Recorder()
        for step in range(2):
            for q in net.parameters():
                q.grad = None
            if step == 1:
                rec.__enter__()
            try:
                net(nhwc(x).detach().requires_grad_(True), nhwc(seg)).backward(nhwc(gy))
                torch.cuda.synchronize()
            finally:
                if step == 1:
                    rec.__exit__()
    return rec.calls, net


@pytest.mark.gpu
def test_the_switch_changes_357_units_only():
    from cat_amd import fused_spade
    fin, fout, channels = 40, 16, [30, 6, 12]
    x, gy = detfill.normal((N, fin, HH, WW), SEED_X), detfill.normal((N, fout, HH, WW), 414)
    b7, _, o = _block(fin, fout, channels)
    b7 = b7.to(dev()).train()
    seg = _seg(o, N, HH, WW)
    off, net_off = _log(b7, x, seg, gy, k7=False)
    layers, _ = _log(b7, x, seg, gy, k7=True, enabled=False)
    on, net_on = _log(b7, x, seg, gy, k7=True)
    assert off == layers and not fused_spade.units_of(net_off)      # switch off: the calls of the commit before, which fused nothing at 3 5 7
    assert on != off and len(on) < len(off) and len(fused_spade.units_of(net_on)) == 2
    assert not any(c[0].startswith('cat_tstage1n7') for c in off)
    b5, _, o5 = _block(fin, fout, channels, ks=[1, 3, 5])
    b5 = b5.to(dev()).train()
    on5, n1 = _log(b5, x, seg, gy, k7=True)
    off5, n2 = _log(b5, x, seg, gy, k7=False)
    assert on5 == off5 and len(fused_spade.units_of(n1)) == len(fused_spade.units_of(n2)) == 2
    assert not any(c[0].startswith('cat_tstage1n7') or c[0].startswith('cat_dwm7') for c in on5)
