"""GPU: InvertedResidualChannels with the reference's default kernel sizes [3, 5, 7] (options/distill_options.py:100-104) on the fused pipeline
(cat_amd/fused_block.py with set_k7(True); cat_amd/fused_unit.py): against the layer-by-layer path of the same module and against a float64
twin out of stock torch.nn layers on the host, at the four bars of tests/test_fused_block_gpu.py -- forward against the general path 2e-5,
forward against the twin 1e-4, input gradient 2e-4, parameter gradients 5e-4 in that file's normalisation.  The same general-path block is
measured against the twin beside it (printed with every case): that is the baseline a bar would have to be derived from, never the fused path's
own error.  Planes are tiny, so every test lowers the LDS-tile threshold to 1 and restores it."""
import contextlib
import copy
import functools

import pytest
import torch

from oracle import detfill
from test_fused_block_gpu import _torch_twin, rel

pytestmark = pytest.mark.gpu
KS = [3, 5, 7]
FULL, PRUNED, RES_ONLY = ((11, 12, 18), (15, 15, 12)), ((7, 0, 9), (16, 5, 0)), ((7, 5, 9), (0, 0, 0))
# (norm, padding, (N, C, H, W), (res widths, dw widths))
CASES = [('batch', 'zero', (2, 24, 9, 17), FULL), ('batch', 'zero', (2, 24, 9, 17), PRUNED), ('batch', 'reflect', (1, 77, 7, 7), FULL),
         ('instance', 'reflect', (2, 40, 16, 32), FULL), ('instance', 'reflect', (2, 40, 16, 32), PRUNED), ('batch', 'zero', (2, 24, 9, 17), RES_ONLY),
         ('instance', 'reflect', (2, 40, 16, 32), RES_ONLY)]
IDS = ['%s-%s-%dx%dx%dx%d-%s' % ((c[0], c[1]) + c[2] + ({FULL: 'full', PRUNED: 'pruned', RES_ONLY: 'resonly'}[c[3]],)) for c in CASES]


def _block(norm, dev, inp, res, dw, padding, ks=KS):
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    nl = cnn.BatchNorm2d if norm == 'batch' else functools.partial(cnn.InstanceNorm2d, affine=False, track_running_stats=False)
    blk = InvertedResidualChannels(inp, list(res), list(dw), 1, list(ks), list(ks), padding_type=padding, use_bias=norm != 'batch', norm_layer=nl,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    blk.load_state_dict(detfill.fill_state_dict(blk.state_dict(), 77, gamma_abs_normal=True))
    return blk.to(dev).train()


@contextlib.contextmanager
def k7_small_planes():
    from cat_amd import _lib, fused_block, ops
    _lib.load()
    old_tiles, old_k7 = ops.set_tconv_min_tiles(1), fused_block.set_k7(True)
    try:
        yield
    finally:
        ops.set_tconv_min_tiles(old_tiles)
        fused_block.set_k7(old_k7)
        fused_block.set_enabled(True)


def _grad_errs(named, tgrads, skip):
    top = max(float(q.grad.abs().max()) for q in tgrads.values())
    out = {}
    for k, q in named:
        assert q.grad is not None, k
        if skip(k):
            continue
        ref = tgrads[k].grad
        out[k] = float((q.grad.detach().cpu().double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * top)
    return out


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_k7_block_forward_and_backward(case):
    from cat_amd import fused_block, ops
    norm, padding, shape, (res, dw) = case
    dev = torch.device('cuda:0')
    n, c, h, w = shape
    x, gy = detfill.normal(shape, 5), detfill.normal(shape, 6)
    with k7_small_planes():
        blk = _block(norm, dev, c, res, dw, padding)
        gen = copy.deepcopy(blk)
        twin, twin_fwd = _torch_twin(blk)
        twin.double()
        xr = x.double().requires_grad_(True)
        y_t = twin_fwd(xr)
        y_t.backward(gy.double())
        xf = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
        assert fused_block.applicable(blk, xf)
        y_f = blk(xf)
        y_f.backward(ops.to_nhwc(gy.to(dev)))
        fused_block.set_enabled(False)
        xg = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
        assert not fused_block.applicable(gen, xg)
        y_g = gen(xg)
        y_g.backward(ops.to_nhwc(gy.to(dev)))
        fused_block.set_enabled(True)
        torch.cuda.synchronize()
    # per-channel shift directly in front of an InstanceNorm: zero gradient in exact arithmetic, round-off on every path
    skip = lambda k: norm == 'instance' and k.endswith('.bias')
    tg = dict(twin.named_parameters())
    ef, eg = _grad_errs(blk.named_parameters(), tg, skip), _grad_errs(gen.named_parameters(), tg, skip)
    fig = dict(fwd_fused_general=rel(y_f, y_g), fwd_fused_twin=rel(y_f, y_t), fwd_general_twin=rel(y_g, y_t), dx_fused_twin=rel(xf.grad, xr.grad),
               dx_general_twin=rel(xg.grad, xr.grad), dparam_fused_twin=max(ef.values()), dparam_general_twin=max(eg.values()))
    print('[k7 block %s] %s' % (case, ', '.join('%s %.3g' % kv for kv in fig.items())))
    assert fig['fwd_fused_general'] < 2e-5, fig
    assert fig['fwd_fused_twin'] < 1e-4, fig
    assert fig['fwd_general_twin'] < 1e-4, fig              # the baseline: the layer-by-layer path, which had no test at kernel size 7 either
    assert fig['dx_fused_twin'] < 2e-4, fig
    bad = {k: e for k, e in ef.items() if e > 5e-4}
    assert not bad, (bad, fig)
    cs = ops.act_cs(y_f)
    full = torch.as_strided(y_f.detach(), (n, cs, h, w), y_f.stride())
    assert cs == c or float(full[:, c:].abs().max()) == 0.0
    if norm == 'batch':      # running statistics and the batch counter of every norm module advanced exactly like torch's
        tsd = twin.state_dict()
        for k, v in blk.state_dict().items():
            if 'running_' in k:
                assert rel(v, tsd[k]) < 1e-5, k
            if 'num_batches_tracked' in k:
                assert int(v) == int(tsd[k]) == 1, k


class _Log:
    """cat_amd._lib.call wrapped while active: the entry-point names, in order"""

    def __enter__(self):
        from cat_amd import _lib
        self.lib, self.real, self.names = _lib, _lib.call, []

        def call(name, *args):
            self.names.append(name)
            return self.real(name, *args)
        _lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.real


@pytest.mark.parametrize('widths,nk', [(FULL, 4), (PRUNED, 3), (RES_ONLY, 3)], ids=['full', 'pruned', 'resonly'])
def test_k7_block_launch_log(widths, nk):
    """A steady-state training-mode forward is one cat_tconv_fwd per first-conv kernel size (the depthwise branches' 1 x 1s are one size),
    then finalize, the depthwise stage on the 7 x 7 frame, finalize, the branch sum, finalize, the closing affine + residual -- and no
    layer-by-layer launch.  A [1, 3, 5] block beside it never reaches a cat_dwm7_* entry point."""
    from cat_amd import fused_block, ops
    dev = torch.device('cuda:0')
    shape = (2, 40, 16, 32)
    x = ops.to_nhwc(detfill.normal(shape, 5).to(dev))
    with k7_small_planes():
        logs = {}
        for ks in (KS, [1, 3, 5]):
            blk = _block('batch', dev, 40, widths[0], widths[1], 'reflect', ks)
            with torch.no_grad():
                assert fused_block.applicable(blk, x)
                blk(x)      # the first forward also prepares the operands (cat_prep_run)
                with _Log() as log:
                    blk(x)
            torch.cuda.synchronize()
            logs[tuple(ks)] = log.names
    dws = any(widths[1])
    dwm = 'cat_dwm7_fwd' if widths[1][2] else 'cat_dwm_fwd'      # one frame side per plan: 7 only with a 7 x 7 depthwise branch (pruned: 3 and 5 are left)
    want = ['cat_tconv_fwd'] * nk + ['cat_tnorm_finalize'] + ([dwm, 'cat_tnorm_finalize'] if dws else []) + \
           ['cat_tconv_fwd', 'cat_tnorm_finalize', 'cat_affine_res_fwd']
    assert logs[(3, 5, 7)] == want, logs[(3, 5, 7)]
    for names in logs.values():
        assert not any(nm in ('cat_conv2d_fwd', 'cat_norm_fwd') or nm.startswith('cat_dwconv2d_') for nm in names), names
    assert not any(nm.startswith('cat_dwm7_') for nm in logs[(1, 3, 5)]), logs[(1, 3, 5)]
    assert ('cat_dwm_fwd' in logs[(1, 3, 5)]) == dws


def test_k7_switch_off_keeps_the_layer_by_layer_path():
    from cat_amd import fused_block, ops
    dev = torch.device('cuda:0')
    x = ops.to_nhwc(detfill.normal((2, 40, 16, 32), 5).to(dev))
    with k7_small_planes():
        blk = _block('batch', dev, 40, *PRUNED, 'reflect')
        assert fused_block.applicable(blk, x)
        assert fused_block.set_k7(False) is True
        assert not fused_block.applicable(blk, x)
        assert fused_block.applicable(_block('batch', dev, 40, *PRUNED, 'reflect', [1, 3, 5]), x)


def test_k7_block_with_dropout():
    """Dropout 0.5 on every branch: fused and general path draw the same masks from the same generator state (one draw per block forward);
    both against the float64 twin carrying those masks"""
    from test_dropout_gpu import SEED, _set_rate, _with_masks
    from cat_amd import fused_block, ops, rng
    dev = torch.device('cuda:0')
    shape = (2, 40, 16, 32)
    x, gy = detfill.normal(shape, 5), detfill.normal(shape, 6)
    with k7_small_planes():
        blk = _block('batch', dev, 40, *FULL, 'reflect')
        _set_rate(blk, 0.5)
        gen = copy.deepcopy(blk)
        twin, twin_fwd = _torch_twin(blk)
        _with_masks([twin], 0.5, 50)
        twin.double()
        xr = x.double().requires_grad_(True)
        y_t = twin_fwd(xr)
        y_t.backward(gy.double())
        out = {}
        for name, b, fused in (('fused', blk, True), ('general', gen, False)):
            xg = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
            rng.set_state(SEED, 50, dev)
            fused_block.set_enabled(fused)
            assert fused_block.applicable(b, xg) == fused
            y = b(xg)
            y.backward(ops.to_nhwc(gy.to(dev)))
            torch.cuda.synchronize()
            assert rng.get_state(dev) == (SEED, 51), name
            out[name] = (y.detach(), xg.grad)
        fused_block.set_enabled(True)
    tg = dict(twin.named_parameters())
    ef = _grad_errs(blk.named_parameters(), tg, lambda k: False)
    fig = dict(fwd_fused_general=rel(out['fused'][0], out['general'][0]), fwd_fused_twin=rel(out['fused'][0], y_t),
               fwd_general_twin=rel(out['general'][0], y_t), dx_fused_twin=rel(out['fused'][1], xr.grad), dparam_fused_twin=max(ef.values()))
    print('[k7 block dropout] %s' % ', '.join('%s %.3g' % kv for kv in fig.items()))
    assert fig['fwd_fused_general'] < 2e-5 and fig['fwd_fused_twin'] < 1e-4 and fig['dx_fused_twin'] < 2e-4, fig
    assert not {k: e for k, e in ef.items() if e > 5e-4}, ef


def test_k7_block_with_two_virtual_replicas():
    """BatchNorm at S = 2: statistics per torch.chunk(batch, 2) shard.  Against the float64 twin run on each chunk by itself (the chunks'
    parameter gradients add, as DataParallel's replicas' do)."""
    from cat_amd import fused_block, networks, ops
    dev = torch.device('cuda:0')
    shape = (4, 24, 9, 17)
    x = detfill.normal(shape, 5) + 0.5 * torch.arange(4, dtype=torch.float32).reshape(4, 1, 1, 1)
    gy = detfill.normal(shape, 6)
    with k7_small_planes():
        blk = _block('batch', dev, 24, *FULL, 'zero')
        networks.set_virtual_replicas(blk, 2)
        twin, twin_fwd = _torch_twin(blk)
        twin.double()
        ys, gxs = [], []
        for xc, gc in zip(x.double().chunk(2), gy.double().chunk(2)):
            xr = xc.clone().requires_grad_(True)
            y = twin_fwd(xr)
            y.backward(gc)
            ys.append(y.detach())
            gxs.append(xr.grad)
        y_t, gx_t = torch.cat(ys), torch.cat(gxs)
        xf = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
        assert fused_block.applicable(blk, xf)
        y_f = blk(xf)
        assert fused_block.plan_for(blk, xf).shards == 2 and fused_block.plan_for(blk, xf).fs == 7
        y_f.backward(ops.to_nhwc(gy.to(dev)))
        torch.cuda.synchronize()
    ef = _grad_errs(blk.named_parameters(), dict(twin.named_parameters()), lambda k: False)
    fig = dict(fwd_fused_twin=rel(y_f, y_t), dx_fused_twin=rel(xf.grad, gx_t), dparam_fused_twin=max(ef.values()))
    print('[k7 block S=2] %s' % ', '.join('%s %.3g' % kv for kv in fig.items()))
    assert fig['fwd_fused_twin'] < 1e-4 and fig['dx_fused_twin'] < 2e-4, fig
    assert not {k: e for k, e in ef.items() if e > 5e-4}, ef
