"""GPU: `--norm syncbatch` on the inception family.  The reference wraps these networks in plain nn.DataParallel (models/networks.py:157-161),
so its SynchronizedBatchNorm2d stays on the F.batch_norm arm (sync_batchnorm/batchnorm.py:68-72) on any number of GPUs: per-replica batch
statistics, num_batches_tracked never advanced, no collective.  A `syncbatch` network must therefore issue exactly the launches of the
`batch` network (no fall-back to the general path where `batch` is fused), compute bit-identical results from equal weights, leave every
num_batches_tracked at 0, and never touch a reducer installed with ops.set_bn_sync.  No tolerance anywhere in the comparisons against
`batch`: the arithmetic is the same launches in the same order.  The two-step fixture (tests/golden/step_syncbn.npz) is the reference's own
run (tools/make_golden_norm_recon.py) and takes the bars of test_model_gpu.test_two_distill_steps_match_reference."""
import functools
import json
import random

import numpy as np
import pytest
import torch

import helpers as H
from oracle import detfill

pytestmark = pytest.mark.gpu
N, C, HB, WB = 2, 40, 16, 32      # the fused-block shape of test_fused_launch_order_gpu.py: 2 x 2 tiles of 8 x 16 per image
RES, DW = (7, 6, 9), (16, 5, 0)


class _Recorder:
    """Wraps cat_amd._lib.call while active: [entry point, 'm' (main stream) or 's' (side stream)] per call."""

    def __init__(self):
        from cat_amd import _lib
        _lib.load()
        self.lib, self.calls = _lib, []

    def __enter__(self):
        main = torch.cuda.current_stream().cuda_stream
        real = self.real = self.lib.call

        def call(name, *args):
            stream = getattr(args[-1], 'value', args[-1])      # the stream is every entry point's last argument
            self.calls.append([name, 'm' if (stream or 0) == main else 's'])
            return real(name, *args)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.real


class _TwoIdenticalRanks:
    """What ops.set_bn_sync expects of a reducer; the other rank holds the same shard: sums double."""
    world_size = 2

    def __init__(self):
        self.calls = 0

    def all_reduce_sum_(self, t):
        self.calls += 1
        return t.mul_(2.0)


def _dev():
    return torch.device('cuda:0')


def _build(what, kind):
    """-> (module in training mode on the device with seeded weights, input shape); equal weights for `batch` and `syncbatch`."""
    from cat_amd import networks
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    opt = H.make_opt(norm=kind, track=True)
    if what == 'block':
        nl = networks.get_norm_layer(kind, affine=True, track_running_stats=True)
        net = InvertedResidualChannels(C, list(RES), list(DW), 1, [1, 3, 5], [1, 3, 5], padding_type='reflect', use_bias=False, norm_layer=nl,
                                       norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
        shape = (N, C, HB, WB)
    elif what == 'G':
        net = networks.define_G(3, 3, 16, 'inception_9blocks', kind, 0, 'normal', 0.02, [], opt=opt)
        shape = (2, 3, 64, 64)
    else:
        net = networks.define_D(6, 16, 'n_layers', 3, kind, 'normal', 0.02, [], opt=opt)
        shape = (2, 6, 64, 64)
    net.load_state_dict(detfill.fill_state_dict(net.state_dict(), 77, gamma_abs_normal=True))
    return net.to(_dev()).train(), shape


def _run(what, kind, synced=False):
    """One forward + backward in training mode -> dict(calls, y, dx, grads, buffers, exchanges, net)."""
    from cat_amd import fused_block, nn as cnn, ops
    net, shape = _build(what, kind)
    x = ops.to_nhwc((detfill.images(shape, 5) if what != 'block' else detfill.normal(shape, 5)).to(_dev())).detach().requires_grad_(True)
    rec, ranks = _Recorder(), _TwoIdenticalRanks()
    was, old = ops.branch_streams_enabled(), ops.set_tconv_min_tiles(1)
    ops.set_branch_streams(False)
    ops.set_bn_sync(ranks if synced else None)
    try:
        if what == 'block':
            assert fused_block.applicable(net, x)
        with rec:
            y = net(x)
            y.backward(ops.to_nhwc(detfill.normal(tuple(y.shape), 6).to(_dev())))
            torch.cuda.synchronize()
    finally:
        ops.set_bn_sync(None)
        ops.set_branch_streams(was)
        ops.set_tconv_min_tiles(old)
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    return dict(calls=rec.calls, y=y.detach(), dx=x.grad.detach(), grads=grads, buffers={k: v.detach().clone() for k, v in net.named_buffers()},
                exchanges=ranks.calls, net=net)


@functools.lru_cache(maxsize=None)
def _result(what, kind):
    return _run(what, kind)


def _assert_same_results(b, s, what):
    assert torch.equal(b['y'], s['y']) and torch.equal(b['dx'], s['dx']), what
    assert list(b['grads']) == list(s['grads']) and len(b['grads']) > 0
    for k in b['grads']:
        assert torch.equal(b['grads'][k], s['grads'][k]), (what, k)
    assert list(b['buffers']) == list(s['buffers'])
    moved = 0
    for k, v in b['buffers'].items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == 1 and int(s['buffers'][k]) == 0, (what, k)
        else:
            assert torch.equal(v, s['buffers'][k]), (what, k)
            moved += int(k.endswith('running_mean') and bool(v.abs().max() > 0))
    assert moved > 0      # the running statistics did move


def _names(r):
    return [c[0] for c in r['calls']]


@pytest.mark.parametrize('what', ['block', 'G', 'D'])
def test_same_launches_and_bit_identical_to_batch(what):
    from cat_amd import nn as cnn
    b, s = _result(what, 'batch'), _result(what, 'syncbatch')
    norms = [m for m in s['net'].modules() if isinstance(m, cnn.BatchNorm2d)]
    assert norms and all(type(m) is cnn.SynchronizedBatchNorm2d and m.replica_local for m in norms)
    got, want = s['calls'], b['calls']
    first = next((i for i, (p, q) in enumerate(zip(got, want)) if p != q), min(len(got), len(want)))
    assert got == want, (len(got), len(want), first, got[first:first + 3], want[first:first + 3])
    assert len(want) > 0
    if what == 'block':      # the fused path ran, for both
        assert hasattr(b['net'], '_cat_fused_plan') and hasattr(s['net'], '_cat_fused_plan') and 'cat_conv2d_wgrad_batch' in _names(s)
    if what == 'G':          # the edge convs on the quad-granule kernel and the blocks on the fused path, for both
        assert 'cat_qconv_fwd' in _names(s) and 'cat_qconv_fwd' in _names(b)
        assert all(hasattr(blk, '_cat_fused_plan') for r in (b, s) for blk in r['net'].features)
    _assert_same_results(b, s, what)


def test_a_layer_that_exchanges_keeps_the_general_path():
    """The SPADE path's SynchronizedBatchNorm2d (no replica_local) is still declined by the fused block and by the edge-conv path."""
    from cat_amd import fused_block, nn as cnn, ops
    net, shape = _build('block', 'syncbatch')
    x = ops.to_nhwc(detfill.normal(shape, 5).to(_dev()))
    old = ops.set_tconv_min_tiles(1)
    try:
        assert fused_block.applicable(net, x)
        net.pw_bn.replica_local = False
        assert not fused_block.applicable(net, x)
        conv = cnn.Conv2d(3, 16, 7, bias=False).to(_dev())
        img = cnn.ReflectionPad2d(3)(ops.to_nhwc(detfill.images((2, 3, 64, 64), 5).to(_dev())))
        assert cnn._edge_conv(conv, cnn.SynchronizedBatchNorm2d(16, replica_local=True).to(_dev()), img)
        assert cnn._edge_conv(conv, cnn.BatchNorm2d(16).to(_dev()), img)
        assert not cnn._edge_conv(conv, cnn.SynchronizedBatchNorm2d(16).to(_dev()), img)
    finally:
        ops.set_tconv_min_tiles(old)


@pytest.mark.parametrize('what', ['G', 'D'])
def test_never_exchanges_under_an_installed_reducer(what):
    from cat_amd import ops
    s = _result(what, 'syncbatch')
    r = _run(what, 'syncbatch', synced=True)
    assert ops.bn_sync() is None      # restored
    assert r['exchanges'] == 0
    assert r['calls'] == s['calls']
    assert torch.equal(r['y'], s['y']) and torch.equal(r['dx'], s['dx'])
    assert all(torch.equal(r['grads'][k], s['grads'][k]) for k in s['grads'])
    assert all(torch.equal(r['buffers'][k], s['buffers'][k]) for k in s['buffers'])


def test_two_distill_steps_match_reference():
    from cat_amd import nn as cnn, ops
    TOL = 1e-3
    g = H.load('step_syncbn.npz')
    meta = json.loads(str(g['meta']))
    assert meta['norm'] == 'syncbatch' and meta['track']
    opt = H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                     lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16,
                     distill_G_loss_type=meta.get('distill', 'ka'))
    model = H.build_distiller(opt, g['student_shapes'])
    for net in (model.netG_teacher, model.netG_student, model.netD):
        norms = [m for m in net.modules() if isinstance(m, cnn.BatchNorm2d)]
        assert norms and all(type(m) is cnn.SynchronizedBatchNorm2d and m.replica_local for m in norms)
    ops.STATS['conform_copies'] = 0
    for step in range(2):
        A = detfill.images((meta['nbatch'], 3, meta['size'], meta['size']), H.SEED_X + 10 + step)
        B = detfill.images((meta['nbatch'], 3, meta['size'], meta['size']), H.SEED_X + 20 + step)
        model.set_input({'A': A, 'B': B, 'A_paths': [], 'B_paths': []})
        model.optimize_parameters(step)
        losses = model.get_current_losses()
        for k, v in losses.items():
            ref = float(g[f'loss{step}:{k}'])
            print('step %d %s: %.7g (reference %.7g)' % (step, k, v, ref))
            assert abs(v - ref) <= TOL * max(1.0, abs(ref)), (step, k, v, ref)
        assert H.rel_err(H.sub(model.Sfake_B, 3, 4), g[f'Sfake{step}']) < (TOL if step == 0 else 1e-2)
        ssd, dsd = model.netG_student.state_dict(), model.netD.state_dict()
        asd = {f'{i}.{k}': v for i, a in enumerate(model.netAs) for k, v in a.state_dict().items()}
        for key in g.files:
            if key.startswith((f'S{step}:', f'D{step}:', f'A{step}:')):
                sd = {'S': ssd, 'D': dsd, 'A': asd}[key[0]]
                got = sd[key.split(':', 1)[1]].detach().cpu().reshape(-1)[:len(g[key])].numpy()
                diff, scale = np.abs(got - g[key]), np.abs(g[key]).max()
                assert np.quantile(diff, 0.75) <= 2e-5 + 2e-4 * scale, (key, diff)
                assert diff.max() <= 2 * meta['lr'] * (step + 1) + 1e-3 * scale, (key, diff)
        for name, sd in (('S', ssd), ('D', dsd)):
            nbt = np.array([int(v) for k, v in sd.items() if k.endswith('num_batches_tracked')], dtype=np.int64)
            assert len(nbt) > 0 and np.array_equal(nbt, g[f'nbt{step}:{name}']) and not nbt.any(), (step, name)
    assert ops.STATS['conform_copies'] == 0, 'the hot path produced tensors outside the native NHWC layout'


def _cycle_gan_step(norm):
    from cat_amd.models import create_model
    opt = H.make_opt(norm=norm, track=True, ndf=16, gan_mode='lsgan', ngf=8, netG='inception_9blocks', dropout_rate=0, direction='AtoB',
                     model='cycle_gan', dataset_mode='unaligned', lambda_A=10.0, lambda_B=10.0, lambda_identity=0.5, pool_size=2)
    m = create_model(opt, verbose=False)
    for i, name in enumerate(('netG_A', 'netG_B', 'netD_A', 'netD_B')):
        net = getattr(m, name)
        net.load_state_dict(detfill.fill_state_dict(net.state_dict(), 401 + i))
    m.setup(opt, verbose=False)
    random.seed(1234)
    m.set_input({'A': detfill.images((1, 3, 64, 64), 420), 'B': detfill.images((1, 3, 64, 64), 430)})
    m.optimize_parameters(0)
    torch.cuda.synchronize()
    return m, m.get_current_losses()


def test_cycle_gan_step_equals_the_batch_step():
    mb, lb = _cycle_gan_step('batch')
    ms, ls = _cycle_gan_step('syncbatch')
    assert lb == ls and len(lb) >= 8 and all(np.isfinite(v) for v in lb.values())
    assert torch.equal(mb.fake_B.detach(), ms.fake_B.detach()) and torch.equal(mb.rec_A.detach(), ms.rec_A.detach())
    for name in ('netG_A', 'netG_B', 'netD_A', 'netD_B'):
        sb, ss = getattr(mb, name).state_dict(), getattr(ms, name).state_dict()
        assert list(sb) == list(ss)
        counted = [int(v) for k, v in sb.items() if k.endswith('num_batches_tracked')]
        assert counted and all(c >= 1 for c in counted)
        for k in sb:
            if k.endswith('num_batches_tracked'):
                assert int(ss[k]) == 0, (name, k)
            else:
                assert torch.equal(sb[k], ss[k]), (name, k)


def test_eval_teacher_takes_the_frozen_fold():
    from cat_amd import frozen, networks, ops
    outs = {}
    x = ops.to_nhwc(detfill.images((2, 3, 64, 64), 991).to(_dev()))
    for norm in ('batch', 'syncbatch'):
        opt = H.make_opt(norm=norm, track=True)
        T = networks.define_G(3, 3, 64, 'inception_9blocks', norm, 0, 'normal', 0.02, [0], opt=opt)
        T.load_state_dict(H.teacher_sd(opt))
        T.eval()
        with torch.no_grad():
            assert frozen.applicable(T.features[0], T.down_sampling(x)), norm
            outs[norm] = T(x)
        assert all(int(v) == 0 for k, v in T.state_dict().items() if k.endswith('num_batches_tracked'))
    assert torch.equal(outs['batch'], outs['syncbatch'])
