"""GPU: the consumers of cat_tstage1ws7_fwd (csrc/conv_s1ws7.hip; fused_unit.stage1 under CAT_STAGE1WS7) -- full-width
InvertedResidualChannels blocks with kernel sizes [3, 5, 7], res (42, 42, 42) and dw (42, 42, 42), whose stage 1 is then ONE launch instead
of one cat_tconv_fwd per first-conv kernel size:

  * the frozen InstanceNorm teacher's block (cat_amd/frozen_in.py, owned, eval mode, no_grad): the launch log with the switch on and off,
    the two outputs against each other (2e-5) and each against a float64 twin out of stock torch.nn layers (1e-4);
  * the wide training block (cat_amd/fused_block.py, CAT_FUSED_WIDE): forward and backward against the twin and the layer-by-layer path at
    the four bars of tests/test_fused_block_k7_gpu.py (forward against the general path 2e-5, against the twin 1e-4, input gradient 2e-4,
    parameter gradients 5e-4), running statistics and num_batches_tracked as there, and one BatchNorm case with two virtual replicas;
  * the plans it must not touch: a [1, 3, 5] wide block and a narrow [3, 5, 7] block issue the same launches with the switch on and off
    and never reach the new entry point.

Planes are tiny, so every test lowers the LDS-tile threshold to 1 and restores it."""
import copy

import pytest
import torch

from oracle import detfill
from test_fused_block_gpu import _torch_twin, rel
from test_fused_block_k7_gpu import _Log, _block, _grad_errs

pytestmark = pytest.mark.gpu
M = (42, 42, 42)
ENTRY = 'cat_tstage1ws7_fwd'


def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def small_planes():
    from cat_amd import _lib, fused_block, fused_unit, ops
    _lib.load()
    old_tiles = ops.set_tconv_min_tiles(1)
    old = fused_block.set_k7(True), fused_block.set_wide(True), fused_unit.set_stage1ws7(True), fused_unit.set_stage1_wide(True)
    yield
    ops.set_tconv_min_tiles(old_tiles)
    fused_block.set_k7(old[0])
    fused_block.set_wide(old[1])
    fused_unit.set_stage1ws7(old[2])
    fused_unit.set_stage1_wide(old[3])
    fused_block.set_enabled(True)


def _forms(run):
    """run() under CAT_STAGE1WS7 on and off -> [(output, steady-state launch log)]"""
    from cat_amd import fused_unit
    out = []
    for on in (True, False):
        old = fused_unit.set_stage1ws7(on)
        try:
            run()      # (the first forward of a form also prepares operands)
            with _Log() as log:
                y = run()
        finally:
            fused_unit.set_stage1ws7(old)
        out.append((y, log.names))
    return out


# ------------------------------------------------------------------------------------------------ the InstanceNorm teacher's block
@pytest.mark.parametrize('padding,shape', [('reflect', (2, 40, 16, 32)), ('zero', (2, 24, 9, 17))], ids=['reflect-16x32', 'zero-9x17'])
def test_owned_instance_block_runs_stage1_in_one_launch(padding, shape):
    from cat_amd import frozen_in, ops
    blk = _block('instance', dev(), shape[1], M, M, padding).eval()
    x = ops.to_nhwc(detfill.normal(shape, 5).to(dev()))
    twin, twin_fwd = _torch_twin(blk)
    twin.eval().double()
    with torch.no_grad():
        y_t = twin_fwd(detfill.normal(shape, 5).double())
    frozen_in.own(blk, 1)
    try:
        def run():
            with torch.no_grad():
                assert frozen_in.applicable(blk, x)
                y = blk(x)
            torch.cuda.synchronize()
            return y
        (y_on, on_log), (y_off, off_log) = _forms(run)
    finally:
        frozen_in.disown(blk)
    # the tail is the one cat_tconv_fwd of both forms; off: one more per first-conv kernel size
    assert on_log.count(ENTRY) == 1 and on_log.count('cat_tconv_fwd') == 1, on_log
    assert off_log.count(ENTRY) == 0 and off_log.count('cat_tconv_fwd') == 5, off_log
    i = on_log.index(ENTRY)
    assert off_log == on_log[:i] + ['cat_tconv_fwd'] * 4 + on_log[i + 1:], (on_log, off_log)      # nothing else moves
    fig = dict(on_off=rel(y_on, y_off), on_twin=rel(y_on, y_t), off_twin=rel(y_off, y_t))
    print('[stage1ws7 frozen_in %s] %s' % (padding, ', '.join('%s %.3g' % kv for kv in fig.items())))
    assert fig['on_off'] < 2e-5, fig
    assert fig['on_twin'] < 1e-4 and fig['off_twin'] < 1e-4, fig


# ------------------------------------------------------------------------------------------------ the wide training block
def _train_step(blk, x, gy):
    from cat_amd import ops
    xg = ops.to_nhwc(x.to(dev())).detach().requires_grad_(True)
    with _Log() as log:
        y = blk(xg)
        y.backward(ops.to_nhwc(gy.to(dev())))
    torch.cuda.synchronize()
    return y.detach(), xg.grad, log.names


@pytest.mark.parametrize('norm,padding,shape', [('batch', 'zero', (2, 24, 9, 17)), ('instance', 'reflect', (2, 40, 16, 32))],
                         ids=['batch-zero-9x17', 'instance-reflect-16x32'])
def test_wide_training_block_forward_and_backward(norm, padding, shape):
    from cat_amd import fused_block, ops
    n, c, h, w = shape
    x, gy = detfill.normal(shape, 5), detfill.normal(shape, 6)
    blk = _block(norm, dev(), c, M, M, padding)
    gen = copy.deepcopy(blk)
    twin, twin_fwd = _torch_twin(blk)
    twin.double()
    xr = x.double().requires_grad_(True)
    y_t = twin_fwd(xr)
    y_t.backward(gy.double())
    assert fused_block.applicable(blk, ops.to_nhwc(x.to(dev())))
    y_f, dx_f, names = _train_step(blk, x, gy)
    assert names.count(ENTRY) == 1, names
    fused_block.set_enabled(False)
    assert not fused_block.applicable(gen, ops.to_nhwc(x.to(dev())))
    y_g, dx_g, general = _train_step(gen, x, gy)
    fused_block.set_enabled(True)
    assert ENTRY not in general
    # per-channel shift directly in front of an InstanceNorm: zero gradient in exact arithmetic, round-off on every path
    skip = lambda k: norm == 'instance' and k.endswith('.bias')
    tg = dict(twin.named_parameters())
    ef, eg = _grad_errs(blk.named_parameters(), tg, skip), _grad_errs(gen.named_parameters(), tg, skip)
    fig = dict(fwd_fused_general=rel(y_f, y_g), fwd_fused_twin=rel(y_f, y_t), fwd_general_twin=rel(y_g, y_t), dx_fused_twin=rel(dx_f, xr.grad),
               dx_general_twin=rel(dx_g, xr.grad), dparam_fused_twin=max(ef.values()), dparam_general_twin=max(eg.values()))
    print('[stage1ws7 wide block %s %s] %s' % (norm, padding, ', '.join('%s %.3g' % kv for kv in fig.items())))
    assert fig['fwd_fused_general'] < 2e-5, fig
    assert fig['fwd_fused_twin'] < 1e-4, fig
    assert fig['dx_fused_twin'] < 2e-4, fig
    bad = {k: e for k, e in ef.items() if e > 5e-4}
    assert not bad, (bad, fig)
    if norm == 'batch':      # running statistics and the batch counter of every norm module advanced exactly like torch's
        tsd = twin.state_dict()
        for k, v in blk.state_dict().items():
            if 'running_' in k:
                assert rel(v, tsd[k]) < 1e-5, k
            if 'num_batches_tracked' in k:
                assert int(v) == int(tsd[k]) == 1, k


def test_wide_training_block_with_two_virtual_replicas():
    """BatchNorm at S = 2: statistics per torch.chunk(batch, 2) shard, out of the one launch's tile table.  Against the float64 twin run on
    each chunk by itself (the chunks' parameter gradients add, as DataParallel's replicas' do)."""
    from cat_amd import fused_block, networks, ops
    shape = (4, 24, 9, 17)
    x = detfill.normal(shape, 5) + 0.5 * torch.arange(4, dtype=torch.float32).reshape(4, 1, 1, 1)
    gy = detfill.normal(shape, 6)
    blk = _block('batch', dev(), 24, M, M, 'zero')
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
    xf = ops.to_nhwc(x.to(dev()))
    assert fused_block.applicable(blk, xf)
    y_f, dx_f, names = _train_step(blk, x, gy)
    assert names.count(ENTRY) == 1 and fused_block.plan_for(blk, xf).shards == 2, names
    ef = _grad_errs(blk.named_parameters(), dict(twin.named_parameters()), lambda k: False)
    fig = dict(fwd_fused_twin=rel(y_f, y_t), dx_fused_twin=rel(dx_f, gx_t), dparam_fused_twin=max(ef.values()))
    print('[stage1ws7 wide block S=2] %s' % ', '.join('%s %.3g' % kv for kv in fig.items()))
    assert fig['fwd_fused_twin'] < 1e-4 and fig['dx_fused_twin'] < 2e-4, fig
    assert not {k: e for k, e in ef.items() if e > 5e-4}, ef


# ------------------------------------------------------------------------------------------------ plans the switch does not concern
@pytest.mark.parametrize('ks,res,dw', [([1, 3, 5], M, M), ([3, 5, 7], (11, 12, 18), (15, 15, 12)), ([3, 5, 7], (42, 0, 42), M)],
                         ids=['135-wide', '357-narrow', '357-wide-pruned'])
def test_other_plans_issue_what_they_issued(ks, res, dw):
    from cat_amd import fused_block, ops
    x = ops.to_nhwc(detfill.normal((2, 40, 16, 32), 5).to(dev()))
    blk = _block('batch', dev(), 40, res, dw, 'reflect', ks)

    def run():
        with torch.no_grad():      # train mode, no graph: the forward's launches alone
            assert fused_block.applicable(blk, x)
            y = blk(x)
        torch.cuda.synchronize()
        return y
    (y_on, on_log), (y_off, off_log) = _forms(run)
    assert on_log == off_log and ENTRY not in on_log, (on_log, off_log)
    assert torch.equal(y_on, y_off)
    if ks == [1, 3, 5]:      # stage 1 in its own one launch + the branch sum
        assert on_log.count('cat_tstage1ws_fwd') == 1 and on_log.count('cat_tconv_fwd') == 1, on_log
    else:                    # one launch per first-conv kernel size (the depthwise branches' 1 x 1s are one size) + the branch sum
        assert on_log.count('cat_tconv_fwd') == len({1} | {k for k, m in zip(ks, res) if m}) + 1, on_log
