"""GPU: the forward-only fused pipeline of owned, wide, eval-mode InstanceNorm blocks (cat_amd/frozen_in.py) -- the CycleGAN-style
distillation's frozen teacher (reference distillers/base_inception_distiller.py:168, inception_distiller.py:100-104; the block:
models/modules/inception_modules.py:124-180, 230-236; InstanceNorm2d without running statistics: models/networks.py:41-44).

Block level: the owned path against the general path and against the float64 stock-torch twin (export.to_reference_module(...).double()),
under tests/test_pretrained_gpu.py's bars (BAR against float64, and the mutual distance); who is admitted; the launch logs.  Distiller
level: ownership after construction, the switch, teacher outputs and taps, one step's losses, and hipGraph replay bit for bit.
Small planes are forced through the kernels with the existing setters: ksum.set_min_workgroups(1) and the owner's tile threshold at 1."""
import copy
import functools
import json

import pytest
import torch

import helpers as H
from oracle import detfill

pytestmark = pytest.mark.gpu
BAR = 1e-3


def dev():
    return torch.device('cuda:0')


class _Launches:
    """Profiler-free launch log (as tests/test_pretrained_gpu.py's): wraps cat_amd._lib.call while active and records the entry-point names."""

    def __init__(self):
        from cat_amd import _lib
        _lib.load()
        self.lib, self.names = _lib, []

    def __enter__(self):
        real = self.real = self.lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.real


def _eval(net, x):
    net.eval()
    with torch.no_grad():
        y = net(x)
    torch.cuda.synchronize()
    return y


def _launches(net, x):
    with _Launches() as log:
        _eval(net, x)
    return log.names


@pytest.fixture
def small_planes():
    """one 128 x 128 tile is enough for the wide-tile sum, the path on, stage 2 on the wide tile where its domain holds; the process-wide
    settings are restored afterwards"""
    from cat_amd import frozen_in, ksum
    old = ksum.set_min_workgroups(1)
    was = frozen_in.set_enabled(True)
    tail = frozen_in.set_tail('ksum')
    yield
    ksum.set_min_workgroups(old)
    frozen_in.set_enabled(was)
    frozen_in.set_tail(tail)


def _block(affine=True, padding='reflect', track=False, seed=77):
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    nl = functools.partial(cnn.InstanceNorm2d, affine=affine, track_running_stats=track)
    blk = InvertedResidualChannels(256, None, None, 6, [1, 3, 5], [1, 3, 5], padding_type=padding, norm_layer=nl,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    blk.load_state_dict(detfill.fill_state_dict(blk.state_dict(), seed))
    return blk.to(dev()).eval()


def _x():
    from cat_amd import ops
    return ops.to_nhwc(detfill.normal((2, 256, 16, 16), 5).to(dev()))


def _finalizes(names):
    return sum(1 for n in names if n.startswith('cat_tnorm_finalize'))


# ------------------------------------------------------------------------------------------------ block level
@pytest.mark.parametrize('affine', [True, False])
def test_owned_block_matches_the_general_path_and_float64(small_planes, affine):
    from cat_amd import export, frozen_in
    blk, other = _block(affine), _block(affine, seed=78)
    x = _x()
    want = export.to_reference_module(blk).double()(x.detach().cpu().double().contiguous()).detach().numpy()
    y_general = _eval(blk, x).cpu().numpy()
    _eval(other, x)      # (the first forward also packs filters: the logs below are steady-state ones)
    general, other_before = _launches(blk, x), _launches(other, x)
    assert 'cat_conv2d_ksum_norm_fwd' not in general and _finalizes(general) == 0
    frozen_in.own(blk, 1)
    try:
        with torch.no_grad():
            assert frozen_in.applicable(blk, x)
        y_owned = _eval(blk, x).cpu().numpy()
        own = _launches(blk, x)
        print(f'launches of one block forward: general {len(general)}, owned {len(own)}: {own}')
        assert own.count('cat_conv2d_ksum_norm_fwd') == 1 and _finalizes(own) == 3 and len(own) < len(general)
        assert _launches(other, x) == other_before      # a block nobody owns issues the launches it issued before
        e_o, e_g, mutual = H.rel_err(y_owned, want), H.rel_err(y_general, want), H.rel_err(y_owned, y_general)
        print(f'affine {affine}: owned vs float64 {e_o:.3e}, general vs float64 {e_g:.3e}, owned vs general {mutual:.3e}')
        assert e_o < BAR and e_g < BAR and mutual < BAR
        # stage 2 on the LDS-tile kernel behind the same switch
        frozen_in.set_tail('tconv')
        y_t = _eval(blk, x).cpu().numpy()
        log_t = _launches(blk, x)
        assert 'cat_conv2d_ksum_norm_fwd' not in log_t and _finalizes(log_t) == 3
        assert H.rel_err(y_t, want) < BAR
        frozen_in.set_tail('ksum')
        # the switch off: the launches of the general path
        frozen_in.set_enabled(False)
        assert _launches(blk, x) == general
        frozen_in.set_enabled(True)
    finally:
        frozen_in.disown(blk)
    assert _launches(blk, x) == general


def test_who_is_admitted(small_planes):
    from cat_amd import frozen_in
    x = _x()
    blk, tracked, hooked = _block(), _block(track=True), _block(seed=79)
    for b in (blk, tracked, hooked):
        frozen_in.own(b, 1)
    handle = hooked.res_ops[0][4].register_forward_hook(lambda m, i, o: None)
    tap = blk.register_forward_hook(lambda m, i, o: None)      # a hook on the block itself (the distiller's taps) does not refuse it
    try:
        with torch.no_grad():
            assert frozen_in.applicable(blk, x)
            assert not frozen_in.applicable(copy.deepcopy(blk), x), 'ownership does not travel with a copy'
            assert not frozen_in.applicable(tracked, x) and not frozen_in.applicable(hooked, x)
            blk.train()
            assert not frozen_in.applicable(blk, x)
            blk.eval()
            frozen_in.own(blk)                                 # the package's own tile threshold: 4 tiles do not fill the chip
            assert not frozen_in.applicable(blk, x)
            frozen_in.own(blk, 1)
        with torch.enable_grad():
            assert not frozen_in.applicable(blk, x)
        frozen_in.disown(blk)
        with torch.no_grad():
            assert not frozen_in.applicable(blk, x)
    finally:
        handle.remove()
        tap.remove()
        for b in (blk, tracked, hooked):
            frozen_in.disown(b)


def test_zero_padding_block_runs_stage2_on_the_lds_tile_kernel(small_planes):
    from cat_amd import export, frozen_in
    blk = _block(padding='zero', seed=80)
    x = _x()
    want = export.to_reference_module(blk).double()(x.detach().cpu().double().contiguous()).detach().numpy()
    y_general = _eval(blk, x).cpu().numpy()
    frozen_in.own(blk, 1)
    try:
        with torch.no_grad():
            assert frozen_in.applicable(blk, x)
        y = _eval(blk, x).cpu().numpy()
        log = _launches(blk, x)
        assert 'cat_conv2d_ksum_norm_fwd' not in log and 'cat_tconv_fwd' in log and _finalizes(log) == 3
        assert H.rel_err(y, want) < BAR and H.rel_err(y, y_general) < BAR
    finally:
        frozen_in.disown(blk)


# ------------------------------------------------------------------------------------------------ distiller level
def _c3_distiller():
    g = H.load('step_in.npz')
    meta = json.loads(str(g['meta']))
    opt = H.make_opt(norm='instance', track=False, ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                     lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16)
    return H.build_distiller(opt, g['student_shapes'])


def _batch(i):
    return {'A': detfill.images((2, 3, 64, 64), 500 + i).cuda(), 'B': detfill.images((2, 3, 64, 64), 600 + i).cuda(), 'A_paths': [], 'B_paths': []}


def _own_teacher(model, min_tiles=1):
    from cat_amd import frozen_in
    for b in model.netG_teacher.features:
        frozen_in.own(b, min_tiles)


def test_distiller_owns_its_instance_norm_teacher(small_planes):
    from cat_amd import frozen_in
    model, twin = _c3_distiller(), _c3_distiller()
    T = model.netG_teacher
    assert len(T.features) == 9 and all(frozen_in.owned(b) for b in T.features)
    assert not any(frozen_in.owned(m) for m in model.netG_student.modules())
    assert not any(frozen_in.owned(m) for m in copy.deepcopy(T).modules())
    batch = _batch(0)
    model.set_input(batch)
    x = model.real_A
    # nothing owned: the launches the teacher always issued
    for b in T.features:
        frozen_in.disown(b)
    _eval(T, x)
    general = _launches(T, x)
    _own_teacher(model)
    frozen_in.set_enabled(False)
    assert _launches(T, x) == general
    model.forward()
    off = [model.Tfake_B.detach().cpu().numpy()] + [model.Tacts[k].detach().cpu().numpy() for k in sorted(model.Tacts)]
    frozen_in.set_enabled(True)
    _eval(T, x)
    own = _launches(T, x)
    print(f'teacher forward: {len(general)} launches on the general path, {len(own)} owned')
    assert own.count('cat_conv2d_ksum_norm_fwd') == 9 and len(own) < len(general)
    model.forward()
    on = [model.Tfake_B.detach().cpu().numpy()] + [model.Tacts[k].detach().cpu().numpy() for k in sorted(model.Tacts)]
    assert len(on) == 5
    for a, b in zip(on, off):
        assert H.rel_err(a, b) < BAR, H.rel_err(a, b)
    # one step, switch on against switch off, from the same state
    _own_teacher(twin)
    model.set_input(batch)
    model.optimize_parameters(0)
    frozen_in.set_enabled(False)
    twin.set_input(batch)
    twin.optimize_parameters(0)
    frozen_in.set_enabled(True)
    la, lb = model.get_current_losses(), twin.get_current_losses()
    for k in lb:
        print(k, la[k], lb[k])
        assert abs(la[k] - lb[k]) <= BAR * max(1.0, abs(lb[k])), (k, la[k], lb[k])


def test_graph_replay_equals_eager_with_the_owned_teacher(small_planes):
    from cat_amd.graph import GraphedStep
    batches = [_batch(i) for i in range(3)]
    eager, graphed = _c3_distiller(), _c3_distiller()
    _own_teacher(eager)
    _own_teacher(graphed)
    with _Launches() as log:
        eager.set_input(batches[0])
        eager.optimize_parameters(0)
    assert log.names.count('cat_conv2d_ksum_norm_fwd') == 9      # the step runs the path under test
    for i in (1, 2):
        eager.set_input(batches[0])
        eager.optimize_parameters(i)
    step = GraphedStep(graphed, batches[0], warmup=3)
    for i in (1, 2):
        eager.set_input(batches[i])
        eager.optimize_parameters(3 + i)
        step(batches[i])
        le, lg = eager.get_current_losses(), graphed.get_current_losses()
        for k in le:
            assert le[k] == lg[k], (k, le[k], lg[k])
    torch.cuda.synchronize()
    assert torch.equal(graphed.Tfake_B, eager.Tfake_B)
    for a, b in ((graphed.netG_student, eager.netG_student), (graphed.netD, eager.netD)):
        for (ka, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(va, vb), ka
