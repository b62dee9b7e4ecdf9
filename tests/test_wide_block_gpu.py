"""GPU: InvertedResidualChannels blocks whose depthwise branches sum to more than CAT_DWM_MAXQ_BWD channel quads on the fused training
pipeline (cat_amd/fused_block.py, CAT_FUSED_WIDE): the depthwise stage as branch-aligned launches on channel slices with per-launch filter
frames (cat_amd/fused_unit.py dwm_fwd / dw_bwd), stage 1 of the teacher's widths in one statistics-writing launch (cat_tstage1ws_fwd,
CAT_STAGE1WS), and the CycleGAN / pix2pix teacher steps built on such blocks.

Blocks: the full-width teacher block (256 channels, 3 x 11 quads, launches 11 | 11 | 11) and inp 40 / res (7, 0, 9) / dw (28, 28, 26)
(21 quads, launches 14 + 7: an empty branch, and a branch of 26 channels in a 28-channel slot at the end).  The twin is
export.to_reference_module(blk).double() on the host.  Bars: the project's 1e-3 relative contract against float64 (BAR, as
tests/test_frozen_in_gpu.py), parameter gradients judged per tensor against max(own scale, 1e-3 of the largest gradient) without those that
are zero in exact arithmetic (tests/test_fused_block_gpu.py); the fused path's distance from the general path and the general path's own
distance from float64 are printed and held to the same bar.  Small planes go through the tile kernels with ops.set_tconv_min_tiles(1)."""
import copy
import functools
import json
import random

import pytest
import torch

import helpers as H
from oracle import detfill
from test_frozen_in_gpu import BAR, _Launches

pytestmark = pytest.mark.gpu
SEED = 0x1234ABCD5678EF01
BLOCKS = {      # name -> (constructor arguments inp, res, dw, reduction factor; input shape; depthwise launches in quads)
    'teacher': ((256, None, None, 6), (2, 256, 16, 16), [11, 11, 11]),
    'q21': ((40, [7, 0, 9], [28, 28, 26], 1), (3, 40, 13, 21), [14, 7]),
}
NORMS = ['batch', 'instance', 'instance-affine']


def dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def small_planes():
    """the planes of this file (4 .. 12 tiles of 8 x 16) through the tile kernels; both switches on; everything restored afterwards"""
    from cat_amd import _lib, fused_block, fused_unit, ops
    _lib.load()
    old = ops.set_tconv_min_tiles(1)
    wide, s1 = fused_block.set_wide(True), fused_unit.set_stage1_wide(True)
    yield
    ops.set_tconv_min_tiles(old)
    fused_block.set_wide(wide)
    fused_unit.set_stage1_wide(s1)


def _block(name, norm='batch', padding='reflect', seed=77, args=None):
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    inp, res, dw, factor = args or BLOCKS[name][0]
    nl = cnn.BatchNorm2d if norm == 'batch' else functools.partial(cnn.InstanceNorm2d, affine=norm == 'instance-affine', track_running_stats=False)
    blk = InvertedResidualChannels(inp, res, dw, factor, [1, 3, 5], [1, 3, 5], padding_type=padding, use_bias=norm != 'batch', norm_layer=nl,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    blk.load_state_dict(detfill.fill_state_dict(blk.state_dict(), seed, gamma_abs_normal=True))
    return blk.to(dev()).train()


def _io(name, seeds=(5, 6)):
    from cat_amd import ops
    shape = BLOCKS[name][1]
    x, gy = detfill.normal(shape, seeds[0]), detfill.normal(shape, seeds[1])
    return x, gy, ops.to_nhwc(x.to(dev())), ops.to_nhwc(gy.to(dev()))


def _step(blk, xg, gyg):
    """forward + backward of a train-mode block -> y, dx, {name: gradient}, {name: buffer}, all on the host"""
    xg = xg.detach().requires_grad_(True)
    y = blk(xg)
    y.backward(gyg)
    torch.cuda.synchronize()
    return (y.detach().cpu(), xg.grad.cpu(), {k: q.grad.detach().cpu().clone() for k, q in blk.named_parameters()},
            {k: v.detach().cpu().clone() for k, v in blk.named_buffers()})


def _general(fn):
    from cat_amd import fused_block
    old = fused_block.set_wide(False)
    try:
        return fn()
    finally:
        fused_block.set_wide(old)


def _exact_zero(blk, norm):
    """names of the parameters whose gradient is zero in exact arithmetic: a conv bias or a 1 x 1 depthwise scale directly in front of an
    InstanceNorm (pure round-off in every implementation)"""
    from cat_amd import nn as cnn
    if norm == 'batch':
        return set()
    out = set()
    for name, m in blk.named_modules():
        if isinstance(m, cnn.Conv2d):
            if m.bias is not None:
                out.add(name + '.bias')
            if m.groups > 1 and m.kernel_size[0] == 1:
                out.add(name + '.weight')
    return out


def _grad_errs(got, want, skip):
    top = max(float(v.abs().max()) for v in want.values())
    return {k: float((got[k].double() - want[k].double()).abs().max()) / max(float(want[k].abs().max()), 1e-3 * top) for k in want if k not in skip}


# ------------------------------------------------------------------------------------------------ admission
def test_the_teacher_block_is_admitted_and_the_switch_restores_the_general_path():
    from cat_amd import fused_block
    blk = _block('teacher', 'instance')
    x, gy, xg, gyg = _io('teacher')
    assert fused_block.applicable(blk, xg)      # 33 quads: refused before CAT_FUSED_WIDE
    _step(blk, xg, gyg)      # (the first step of a path also packs filters: the logs below are steady-state ones)
    with _Launches() as log:
        _step(blk, xg, gyg)
    wide = log.names
    assert wide.count('cat_dwm_fwd') == 3 and wide.count('cat_dwm_bwd') == 3 and wide.count('cat_tstage1ws_fwd') == 1
    fused_block.set_enabled(False)
    try:
        _step(blk, xg, gyg)
        with _Launches() as log:
            _step(blk, xg, gyg)
    finally:
        fused_block.set_enabled(True)
    general = log.names
    assert 'cat_dwm_fwd' not in general and 'cat_tnorm_finalize' not in general and len(general) > len(wide)
    print('launches of one forward + backward: fused %d, layer by layer %d' % (len(wide), len(general)))

    def off():
        assert not fused_block.applicable(blk, xg)
        with _Launches() as log:
            _step(blk, xg, gyg)
        return log.names
    assert _general(off) == general


def test_a_branch_wider_than_a_launch_is_refused_either_way():
    from cat_amd import fused_block, ops
    blk = _block(None, 'batch', args=(40, [7, 0, 9], [76, 0, 0], 1))      # one depthwise branch of 19 quads
    xg = ops.to_nhwc(detfill.normal((3, 40, 13, 21), 5).to(dev()))
    assert not fused_block.applicable(blk, xg)
    assert not _general(lambda: fused_block.applicable(blk, xg))
    narrow = _block(None, 'batch', args=(40, [7, 0, 9], [72, 0, 0], 1))   # 18 quads: one launch, admitted with the switch off as well
    assert fused_block.applicable(narrow, xg) and _general(lambda: fused_block.applicable(narrow, xg))


def test_plan_groups_and_filter_frames():
    """the plans' launches, and every launch's 5 x 5 filter frame [25][launch width] as the preparation jobs write it: the k x k window of
    each channel's filter centred in the frame, zeros elsewhere"""
    from cat_amd import fused_block
    for name in BLOCKS:
        blk = _block(name, 'batch')
        xg = _io(name)[2]
        p = fused_block.plan_for(blk, xg)
        p.prepare()
        torch.cuda.synchronize()
        assert [(end - o) // 4 for bs, o, end in p.dw_groups] == BLOCKS[name][2]
        w25 = p.w25.cpu()
        for bs, o, end in p.dw_groups:
            width = end - o
            frame = w25[25 * o:25 * end].view(5, 5, width)
            want = torch.zeros(5, 5, width)
            for b in bs:
                k, m, c0 = b['kd'], b['m'], b['od'] - o
                want[2 - k // 2:3 + k // 2, 2 - k // 2:3 + k // 2, c0:c0 + m] = b['dconv'].weight.detach().cpu()[:, 0].permute(1, 2, 0)
            assert torch.equal(frame, want), (name, o)


# ------------------------------------------------------------------------------------------------ forward and backward against float64
@pytest.mark.parametrize('padding', ['reflect', 'zero'])
@pytest.mark.parametrize('norm', NORMS)
@pytest.mark.parametrize('name', list(BLOCKS))
def test_wide_block_matches_float64_and_the_general_path(name, norm, padding):
    from cat_amd import export, fused_block
    blk = _block(name, norm, padding)
    ref_blk = copy.deepcopy(blk)
    x, gy, xg, gyg = _io(name)
    twin = export.to_reference_module(blk).double()
    assert twin.training
    xr = x.double().requires_grad_(True)
    y64 = twin(xr)
    y64.backward(gy.double())
    g64 = {k: q.grad for k, q in twin.named_parameters()}
    b64 = dict(twin.named_buffers())
    assert fused_block.applicable(blk, xg)
    with _Launches() as log:
        y_f, dx_f, g_f, b_f = _step(blk, xg, gyg)
    assert log.names.count('cat_dwm_fwd') == log.names.count('cat_dwm_bwd') == len(BLOCKS[name][2])
    y_g, dx_g, g_g, b_g = _general(lambda: _step(ref_blk, xg, gyg))
    skip = _exact_zero(blk, norm)
    assert sorted(g_f) == sorted(g64) and skip < set(g64)
    figures = {}
    for what, a, b in (('fused vs float64', (y_f, dx_f, g_f), (y64.detach(), xr.grad, g64)), ('general vs float64', (y_g, dx_g, g_g), (y64.detach(), xr.grad, g64)),
                       ('fused vs general', (y_f, dx_f, g_f), (y_g, dx_g, g_g))):
        errs = _grad_errs(a[2], b[2], skip)
        worst = max(errs, key=errs.get)
        figures[what] = (H.rel_err(a[0], b[0]), H.rel_err(a[1], b[1]), errs[worst])
        print('%s %s %s %s: y %.3g dx %.3g parameter gradients %.3g (%s)' % ((name, norm, padding, what) + figures[what] + (worst,)))
    for what, v in figures.items():
        assert max(v) < BAR, (what, v)
    if norm == 'batch':
        assert sorted(b_f) == sorted(b64)
        for k, v in b_f.items():
            if k.endswith('num_batches_tracked'):
                assert int(v) == int(b64[k]) == int(b_g[k]) == 1, k
            else:
                e = H.rel_err(v, b64[k])
                assert e < BAR and H.rel_err(b_g[k], b64[k]) < BAR, (k, e)
    else:
        assert not b_f


# ------------------------------------------------------------------------------------------------ accumulation (one launch carries two branches, the next one)
@pytest.mark.parametrize('streams', [False, True])
def test_second_backward_adds_exactly_once_into_optimizer_buffers(streams):
    from cat_amd import ops
    from cat_amd.optim import FusedAdam
    blk = _block('q21', 'batch')
    x, gy, xg, gyg = _io('q21')
    opt = FusedAdam(list(blk.parameters()), lr=0.0)
    was = ops.branch_streams_enabled()
    ops.set_branch_streams(streams)
    try:
        opt.zero_grad()
        _step(blk, xg, gyg)
        once = {k: q.grad.clone() for k, q in blk.named_parameters()}
        _step(blk, xg, gyg)
    finally:
        ops.set_branch_streams(was)
    for k, q in blk.named_parameters():
        assert float(once[k].abs().max()) > 0.0, k
        assert q.grad.data_ptr() == q._cat_grad_view.data_ptr(), k
        assert torch.equal(q.grad, once[k] + once[k]), k


def test_backward_with_mixed_parameter_ownership():
    from cat_amd.optim import FusedAdam
    blk = _block('q21', 'batch')
    x, gy, xg, gyg = _io('q21')
    plain = copy.deepcopy(blk)
    _step(plain, xg, gyg)
    params = list(blk.parameters())
    mine = {id(q) for q in params[::2]}
    FusedAdam(params[::2], lr=0.0).zero_grad()
    _step(blk, xg, gyg)
    ref = dict(plain.named_parameters())
    dwn = [n + '.weight' for n, m in blk.named_modules() if isinstance(m, torch.nn.Conv2d) and m.groups > 1]
    assert len(dwn) == 3 and 0 < sum(id(dict(blk.named_parameters())[n]) in mine for n in dwn) < 3      # the depthwise sink itself is mixed
    for k, q in blk.named_parameters():
        view = getattr(q, '_cat_grad_view', None)
        assert (view is not None) == (id(q) in mine), k
        assert q.grad is not None, k
        if view is not None:
            assert q.grad.data_ptr() == view.data_ptr(), k
        assert float(q.grad.abs().max()) > 0.0, k
        assert torch.equal(q.grad, ref[k].grad), k


# ------------------------------------------------------------------------------------------------ other forms: fused against general on equal weights
def _fused_vs_general(blk, xg, gyg, before=lambda: None):
    from cat_amd import fused_block
    ref_blk = copy.deepcopy(blk)
    before()
    assert fused_block.applicable(blk, xg)
    y_f, dx_f, g_f, b_f = _step(blk, xg, gyg)
    before()
    y_g, dx_g, g_g, b_g = _general(lambda: _step(ref_blk, xg, gyg))
    errs = _grad_errs(g_f, g_g, set())
    worst = max(errs, key=errs.get)
    v = (H.rel_err(y_f, y_g), H.rel_err(dx_f, dx_g), errs[worst])
    print('fused vs general: y %.3g dx %.3g parameter gradients %.3g (%s)' % (v + (worst,)))
    assert max(v) < BAR, v
    for k in b_f:
        assert H.rel_err(b_f[k], b_g[k]) < BAR, k
    return y_f


def test_virtual_replicas():
    from cat_amd import fused_block, networks
    blk = _block('q21', 'batch')
    assert networks.set_virtual_replicas(blk, 2) >= 7
    x, gy, xg, gyg = _io('q21')
    y2 = _fused_vs_general(blk, xg, gyg)
    assert fused_block.plan_for(blk, xg).shards == 2
    one = _block('q21', 'batch')
    y1 = _step(one, xg, gyg)[0]
    assert H.rel_err(y2, y1) > 1e-2      # per-shard statistics: another function than one group over the batch


def test_dropout_with_a_fixed_ticket():
    from cat_amd import rng
    from test_dropout_gpu import _set_rate
    blk = _block('q21', 'batch')
    _set_rate(blk, 0.25)
    x, gy, xg, gyg = _io('q21')
    y = _fused_vs_general(blk, xg, gyg, before=lambda: rng.set_state(SEED, 50, dev()))
    assert rng.get_state(dev()) == (SEED, 51)      # one draw per block forward
    plain = _block('q21', 'batch')
    assert H.rel_err(y, _step(plain, xg, gyg)[0]) > 1e-2      # the masks were applied


# ------------------------------------------------------------------------------------------------ the stage-1 switch
def _stage1_forms(run):
    """run() under CAT_STAGE1WS on and off -> the two (output, launch log)"""
    from cat_amd import fused_unit
    out = []
    for on in (True, False):
        old = fused_unit.set_stage1_wide(on)
        try:
            run()      # (the first forward of a form also prepares operands: the logs are steady-state ones)
            with _Launches() as log:
                y = run()
        finally:
            fused_unit.set_stage1_wide(old)
        out.append((y, log.names))
    (y_on, on_log), (y_off, off_log) = out
    # stage 2 is the one cat_tconv_fwd of both forms; off: one more per first-conv kernel size
    assert on_log.count('cat_tstage1ws_fwd') == 1 and on_log.count('cat_tconv_fwd') == 1, on_log
    assert off_log.count('cat_tstage1ws_fwd') == 0 and off_log.count('cat_tconv_fwd') == 4, off_log
    assert len(off_log) == len(on_log) + 2
    e = H.rel_err(y_on, y_off)
    print('stage 1 in one launch vs three: %.3g' % e)
    assert e < BAR
    return y_on


@pytest.mark.parametrize('padding', ['reflect', 'zero'])
def test_stage1_switch_training_forward(padding):
    blk = _block('teacher', 'batch', padding)
    xg = _io('teacher')[2]

    def run():
        with torch.no_grad():      # train mode, no graph: the forward's launches alone
            y = blk(xg)
        torch.cuda.synchronize()
        return y.cpu()
    _stage1_forms(run)


def test_stage1_switch_frozen_teacher_block():
    from cat_amd import export, frozen_in
    blk = _block('teacher', 'instance-affine').eval()
    xg = _io('teacher')[2]
    want = export.to_reference_module(blk).double()(xg.detach().cpu().double().contiguous()).detach()
    frozen_in.own(blk, 1)
    try:
        def run():
            with torch.no_grad():
                assert frozen_in.applicable(blk, xg)
                y = blk(xg)
            torch.cuda.synchronize()
            return y.cpu()
        y = _stage1_forms(run)
        assert H.rel_err(y, want) < BAR
        with _Launches() as log:
            run()
        assert log.names.count('cat_dwm_fwd') == 2      # the forward-only path keeps its 22 + 11 grouping
    finally:
        frozen_in.disown(blk)


# ------------------------------------------------------------------------------------------------ model level: ngf 40 teachers (160-channel blocks, 21 quads)
def _fill(net, seed):
    net.load_state_dict(detfill.fill_state_dict(net.state_dict(), seed))


def _cyclegan():
    from cat_amd.models import create_model
    from test_train_models import _opt_for
    meta = json.loads(str(H.load('train_steps.npz')['cyc_meta']))
    meta = dict(meta, ngf=40)
    opt = _opt_for(meta, model='cycle_gan', dataset_mode='unaligned', lambda_A=meta['lambda_A'], lambda_B=meta['lambda_B'],
                   lambda_identity=meta['lambda_identity'], pool_size=50)
    m = create_model(opt, verbose=False)
    for i, name in enumerate(('netG_A', 'netG_B', 'netD_A', 'netD_B')):
        _fill(getattr(m, name), 401 + i)
    m.setup(opt, verbose=False)
    m.fake_A_pool.rng = m.fake_B_pool.rng = random.Random(1)
    return m


def _pix2pix():
    from cat_amd.models import create_model
    from test_train_models import _opt_for
    meta = json.loads(str(H.load('train_steps.npz')['p2p_meta']))
    meta = dict(meta, ngf=40)
    opt = _opt_for(meta, model='pix2pix', lambda_recon=meta['lambda_recon'], lambda_gan=1.0, recon_loss_type='l1')
    m = create_model(opt, verbose=False)
    _fill(m.netG, 301)
    _fill(m.netD, 302)
    m.setup(opt, verbose=False)
    return m


def _batches(k, n=2):
    return [{'A': detfill.images((n, 3, 64, 64), 870 + i).cuda(), 'B': detfill.images((n, 3, 64, 64), 880 + i).cuda(), 'A_paths': [], 'B_paths': []}
            for i in range(k)]


def _blocks_of(net):
    from cat_amd.inception_modules import InvertedResidualChannels
    return [b for b in net.modules() if isinstance(b, InvertedResidualChannels)]


def _probe(net):
    """the first 64 values of every parameter of the trunk's first and last block and of the head"""
    sd = net.state_dict()
    keys = [k for k in sd if k.startswith(('features.0.', 'features.8.', 'up_sampling.')) and sd[k].dtype == torch.float32]
    assert len(keys) > 20
    return torch.cat([sd[k].detach().reshape(-1)[:64].cpu() for k in keys])


def _train(make, gens, steps, wide):
    from cat_amd import fused_block
    old = fused_block.set_wide(wide)
    try:
        m = make()
        log = None
        losses = []
        for i, b in enumerate(_batches(steps)):
            m.set_input(b)
            with _Launches() as log:
                m.optimize_parameters(i)
            losses.append(dict(m.get_current_losses()))
        torch.cuda.synchronize()
        return losses, [_probe(getattr(m, g)) for g in gens], log.names, m
    finally:
        fused_block.set_wide(old)


def _same_training(make, gens, steps, passes):
    """`passes`: generator forward + backward passes of one step, each over nine blocks of 21 quads (launches 14 + 7)"""
    la, pa, log_a, m = _train(make, gens, steps, True)
    lb, pb, log_b, _ = _train(make, gens, steps, False)
    quads = [sum(b.dw_channels[i] // 4 + (b.dw_channels[i] % 4 > 0) for i in range(3)) for g in gens for b in _blocks_of(getattr(m, g))]
    assert quads == [21] * 9 * len(gens)
    fwd, bwd = passes
    assert log_a.count('cat_dwm_fwd') == 2 * 9 * fwd and log_a.count('cat_dwm_bwd') == 2 * 9 * bwd, (log_a.count('cat_dwm_fwd'), log_a.count('cat_dwm_bwd'))
    assert 'cat_dwm_fwd' not in log_b and len(log_a) < len(log_b)
    print('launches of one step: wide path %d, layer by layer %d' % (len(log_a), len(log_b)))
    for i, (a, b) in enumerate(zip(la, lb)):
        assert sorted(a) == sorted(b)
        for k in a:
            print('step %d %s: wide %.9g general %.9g' % (i, k, a[k], b[k]))
        for k in a:
            assert abs(a[k] - b[k]) <= BAR * max(1.0, abs(b[k])), (i, k, a[k], b[k])
    for g, a, b in zip(gens, pa, pb):
        e = H.rel_err(a, b)
        print('%s: probe of updated weights %.3g' % (g, e))
        assert e < BAR, g


def test_cyclegan_teacher_steps_wide_against_general():
    # a CycleGAN step runs each generator three times forward (fake, cycle, identity), all with a graph: six passes over nine blocks
    _same_training(_cyclegan, ('netG_A', 'netG_B'), 2, (6, 6))


def test_pix2pix_teacher_step_wide_against_general():
    _same_training(_pix2pix, ('netG',), 1, (1, 1))


def test_cyclegan_graph_replay_equals_eager_on_the_wide_path():
    from cat_amd.graph import GraphedStep
    batches = _batches(5)
    eager, graphed = _cyclegan(), _cyclegan()
    with _Launches() as log:
        eager.set_input(batches[0])
        eager.optimize_parameters(0)
    assert log.names.count('cat_dwm_bwd') == 2 * 9 * 6      # the step runs the path under test
    for i in (1, 2):
        eager.set_input(batches[0])
        eager.optimize_parameters(i)
    step = GraphedStep(graphed, batches[0], warmup=3)
    for i in (3, 4):
        eager.set_input(batches[i])
        eager.optimize_parameters(i)
        step(batches[i])
        le, lg = eager.get_current_losses(), graphed.get_current_losses()
        assert len(le) == 8
        for k in le:
            assert le[k] == lg[k], (i, k, le[k], lg[k])
    assert step.replays == 2
    torch.cuda.synchronize()
    for name in ('netG_A', 'netG_B', 'netD_A', 'netD_B'):
        for (ka, va), (_, vb) in zip(getattr(graphed, name).state_dict().items(), getattr(eager, name).state_dict().items()):
            assert torch.equal(va, vb), (name, ka)
