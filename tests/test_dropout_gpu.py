"""GPU: dropout on the Philox kernels (csrc/dropout.hip): masks bit-exact against the numpy restatement (test_dropout_host.py), their
statistics, DropoutFn's backward, InvertedResidualChannels with dropout on the fused and the general path against each other and against
stock torch with the same masks, a whole student generator, the eval / frozen paths, graph replays and a cycle_gan step."""
import copy
import json

import numpy as np
import pytest
import torch

import helpers as H
from oracle import detfill
from test_dropout_host import keep_mask, scale_of

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SEED = 0x1234ABCD5678EF01


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _ticket(d, seed=SEED):
    from cat_amd import rng
    rng.set_state(seed, d, DEV)
    t = rng.draw(DEV)
    assert rng.get_state(DEV) == (seed, d + 1)
    assert t.cpu().tolist() == [d if d < 2 ** 31 else d - 2 ** 32, np.int32(np.uint32(seed & 0xFFFFFFFF)), np.int32(np.uint32(seed >> 32)), 0]
    return t


def _apply(x, xcs, c0, C, p, j, d, seed=SEED):
    """plain mode on channels [c0, c0 + C) of an [npix, xcs] buffer, written to a fresh [npix, xcs] buffer (rest = 1)"""
    from cat_amd import ops
    npix = x.shape[0]
    y = torch.full_like(x, 7.0)
    g = ops.dropout_geom(npix, xcs, xcs, xcs, p, [(c0, C, j)])
    ops.dropout_apply(g, x, y, _ticket(d, seed))
    return y


# ---------------------------------------------------------------------------------------------------------------- 1. bit-exact masks
@pytest.mark.parametrize('C', [1, 3, 4, 17, 44])
@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
def test_masks_match_the_numpy_restatement(C, p):
    from cat_amd import _lib
    _lib.load()
    npix = 2 * 5 * 7                                  # N*H*W = 70, not a multiple of 4
    c0 = 8
    xcs = c0 + (C + 3) // 4 * 4 + 4                   # a slice at channel 8 of a wider (padded) buffer
    x = torch.from_numpy(np.random.default_rng(C).standard_normal((npix, xcs)).astype(np.float32)).to(DEV)
    y = _apply(x, xcs, c0, C, p, 3, 1000 + C).cpu()
    keep = keep_mask(npix, C, 3, 1000 + C, SEED, p)
    xs = x.cpu()[:, c0:c0 + C].numpy()
    want = np.where(keep, xs * scale_of(p), np.float32(0))
    np.testing.assert_array_equal(y[:, c0:c0 + C].numpy(), want)
    np.testing.assert_array_equal(y[:, :c0].numpy(), x.cpu()[:, :c0].numpy())        # outside the segment: copied
    np.testing.assert_array_equal(y[:, c0 + C:].numpy(), x.cpu()[:, c0 + C:].numpy())
    ones = torch.ones_like(x)
    y1 = _apply(ones, xcs, c0, C, p, 3, 1000 + C).cpu()[:, c0:c0 + C].numpy()
    np.testing.assert_array_equal(y1, keep * scale_of(p))


def test_module_p1_p0_and_eval():
    from cat_amd import nn as cnn, ops, rng
    x = ops.to_nhwc(detfill.normal((2, 5, 9, 11), 3).to(DEV))
    rng.set_state(SEED, 40, DEV)
    y = cnn.Dropout(1.0).train()(x)
    assert float(y.abs().max()) == 0.0 and rng.get_state(DEV) == (SEED, 41)
    for m in (cnn.Dropout(0.0).train(), cnn.Dropout(0.5).eval()):
        assert m(x) is x
    assert rng.get_state(DEV) == (SEED, 41)            # no draw, no launch
    # a stand-alone module: its own draw, j = 0, on the logical NHWC tensor of C = 5 channels (stride 8)
    rng.set_state(SEED, 77, DEV)
    y = cnn.Dropout(0.3).train()(x)
    keep = keep_mask(2 * 9 * 11, 5, 0, 77, SEED, 0.3).reshape(2, 9, 11, 5).transpose(0, 3, 1, 2)
    want = np.where(keep, x.cpu().numpy() * scale_of(0.3), np.float32(0))
    np.testing.assert_array_equal(y.cpu().numpy(), want)
    cs = ops.act_cs(y)
    assert float(torch.as_strided(y, (2, cs, 9, 11), y.stride())[:, 5:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 2. statistics
def test_mask_statistics():
    from cat_amd import ops
    npix, C, p = 64 * 128 * 32, 64, 0.3                   # 16.8 M elements
    x = torch.ones((npix, C), device=DEV)
    keep = (_apply(x, C, 0, C, p, 0, 5) != 0).double()
    n = keep.numel()
    rate = float(keep.mean())
    assert abs(rate - (1 - p)) < 6 * (p * (1 - p) / n) ** 0.5, rate
    k = keep - keep.mean()
    var = float((k * k).mean())
    for a, b in ((k[:, :-1], k[:, 1:]), (k[:-1], k[1:]), (k[:-64], k[64:])):      # neighbouring channels, pixels, rows of 64 pixels
        corr = float((a * b).mean()) / var
        assert abs(corr) < 6 / a.numel() ** 0.5, corr
    base = _apply(x, C, 0, C, p, 0, 5)
    for other in (_apply(x, C, 0, C, p, 0, 6), _apply(x, C, 0, C, p, 1, 5), _apply(x, C, 0, C, p, 0, 5, seed=SEED + 1)):
        diff = float((base != other).double().mean())
        assert abs(diff - 2 * p * (1 - p)) < 0.01, diff
    assert torch.equal(base, _apply(x, C, 0, C, p, 0, 5))


# ---------------------------------------------------------------------------------------------------------------- 3. DropoutFn backward
def test_dropout_fn_backward_is_the_masked_gradient():
    from cat_amd import ops, rng
    x = ops.to_nhwc(detfill.normal((3, 17, 10, 13), 4).to(DEV)).detach().requires_grad_(True)
    gy = ops.to_nhwc(detfill.normal((3, 17, 10, 13), 5).to(DEV))
    t = _ticket(9)
    y = ops.DropoutFn.apply(x, 0.4, t, 2)
    y.backward(gy)
    keep = keep_mask(3 * 10 * 13, 17, 2, 9, SEED, 0.4).reshape(3, 10, 13, 17).transpose(0, 3, 1, 2)
    np.testing.assert_array_equal(x.grad.cpu().numpy(), np.where(keep, gy.cpu().numpy() * scale_of(0.4), np.float32(0)))
    np.testing.assert_array_equal(y.detach().cpu().numpy(), np.where(keep, x.detach().cpu().numpy() * scale_of(0.4), np.float32(0)))
    assert rng.get_state(DEV)[1] == 10


# ---------------------------------------------------------------------------------------------------------------- 4. one block
class _FixedMask(torch.nn.Module):
    """nn.Dropout of the reference with the mask the kernels draw (numpy restatement) for block ticket d and module index j."""

    def __init__(self, p, j, d, seed=SEED):
        super().__init__()
        self.p, self.j, self.d, self.seed = p, j, d, seed

    def forward(self, x):
        n, c, h, w = x.shape
        keep = keep_mask(n * h * w, c, self.j, self.d, self.seed, self.p).reshape(n, h, w, c).transpose(0, 3, 1, 2)
        return x * torch.from_numpy(np.ascontiguousarray(keep)).float() * float(scale_of(self.p))


def _with_masks(twin_blocks, p, d0):
    """block k of twin_blocks gets the masks of ticket d0 + k: every nn.Dropout j (res branches first) -> _FixedMask"""
    for k, blk in enumerate(twin_blocks):
        ops_ = list(blk.res_ops) + list(blk.dw_ops)
        for j, op in enumerate(ops_):
            for name, m in list(op.named_children()):
                if isinstance(m, torch.nn.Dropout):
                    op._modules[name] = _FixedMask(p, j, d0 + k)


def _set_rate(net, p):
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels
    for m in net.modules():
        if isinstance(m, cnn.Dropout):
            m.p = p
        if isinstance(m, InvertedResidualChannels):
            m.dropout_rate = p


@pytest.mark.parametrize('norm,padding,shape', [('batch', 'reflect', (4, 77, 48, 64)), ('instance', 'reflect', (4, 77, 48, 64)),
                                                ('batch', 'zero', (3, 77, 50, 70)), ('batch', 'reflect', (8, 40, 32, 48))])
def test_block_with_dropout_fused_general_and_torch(norm, padding, shape):
    from test_fused_block_gpu import _block, _torch_twin
    from cat_amd import fused_block, ops, rng
    n, c, h, w = shape
    res, dw = ((11, 12, 18), (15, 15, 12)) if c == 77 else ((7, 0, 9), (16, 5, 0))
    blk = _block(norm, DEV, c, res, dw, padding)
    _set_rate(blk, 0.25)
    gen_blk = copy.deepcopy(blk)
    twin, twin_fwd = _torch_twin(blk)
    _with_masks([twin], 0.25, 50)
    x, gy = detfill.normal((n, c, h, w), 5), detfill.normal((n, c, h, w), 6)
    xr = x.clone().requires_grad_(True)
    y_t = twin_fwd(xr)
    y_t.backward(gy)
    out = {}
    for name, b, fused in (('fused', blk, True), ('general', gen_blk, False)):
        xg = ops.to_nhwc(x.to(DEV)).detach().requires_grad_(True)
        rng.set_state(SEED, 50, DEV)
        fused_block.set_enabled(fused)
        try:
            assert fused_block.applicable(b, xg) == fused
            y = b(xg)
            y.backward(ops.to_nhwc(gy.to(DEV)))
        finally:
            fused_block.set_enabled(True)
        torch.cuda.synchronize()
        assert rng.get_state(DEV) == (SEED, 51), name          # one draw per block forward
        out[name] = (y.detach(), xg.grad, {k: q.grad for k, q in b.named_parameters()})
    (yf, gf, pf), (yg, gg, pg) = out['fused'], out['general']
    assert rel(yf, yg) < 2e-5 and rel(gf, gg) < 2e-5, (rel(yf, yg), rel(gf, gg))
    top = max(float(q.abs().max()) for q in pg.values())
    # parameter gradients are reductions over all pixels in another order on each path (a wrong mask would be an O(1) difference); those
    # that are zero in exact arithmetic in front of an InstanceNorm are round-off only
    zero = (lambda k: norm == 'instance' and (k.endswith('.bias') or k == 'dw_ops.0.2.0.weight'))
    for k in pf:
        if not zero(k):
            assert float((pf[k] - pg[k]).abs().max()) <= 2e-4 * max(float(pg[k].abs().max()), 1e-3 * top), k
    tgrads = dict(twin.named_parameters())
    ttop = max(float(q.grad.abs().max()) for q in tgrads.values())
    for y, gx, pgr in out.values():
        assert rel(y, y_t) < 1e-4, rel(y, y_t)
        assert rel(gx, xr.grad) < 5e-4, rel(gx, xr.grad)
        for k, q in pgr.items():
            if zero(k):
                continue
            ref = tgrads[k].grad
            err = float((q.detach().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * ttop)
            assert err < 5e-4, (k, err)


# ---------------------------------------------------------------------------------------------------------------- 5. whole student
def test_student_generator_with_dropout_against_the_reference_twin():
    from cat_amd import export, ops, rng
    from cat_amd.inception_modules import InvertedResidualChannels
    g = H.load('forward_bn.npz')
    opt = H.make_opt(norm='batch', track=True)
    shapes = H.sd_from_shapes(g['student_shapes'])
    net = H.student_from_shapes(opt, shapes)
    net.load_state_dict(detfill.fill_state_dict(shapes, H.SEED_S))
    net = net.to(DEV).train()
    _set_rate(net, 0.1)
    twin = export.to_reference_module(net).train()
    blocks = [m for m in twin.modules() if isinstance(m, export.TwinInvertedResidualChannels)]
    assert len(blocks) == sum(isinstance(m, InvertedResidualChannels) for m in net.modules()) > 0
    _with_masks(blocks, 0.1, 300)
    x = detfill.images((2, 3, 128, 128), H.SEED_X)
    gy = detfill.normal((2, 3, 128, 128), 8)
    xr = x.clone().requires_grad_(True)
    y_t = twin(xr)
    y_t.backward(gy)
    rng.set_state(SEED, 300, DEV)
    xg = ops.to_nhwc(x.to(DEV)).detach().requires_grad_(True)
    y = net(xg)
    y.backward(ops.to_nhwc(gy.to(DEV)))
    torch.cuda.synchronize()
    assert rng.get_state(DEV) == (SEED, 300 + len(blocks))
    assert rel(y, y_t) < 1e-4, rel(y, y_t)
    tgrads = dict(twin.named_parameters())
    top = max(float(q.grad.abs().max()) for q in tgrads.values())
    for k, q in net.named_parameters():
        ref = tgrads[k].grad
        err = float((q.grad.detach().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-3 * top)
        assert err < 5e-4, (k, err)
    assert rel(xg.grad, xr.grad) < 5e-4


# ---------------------------------------------------------------------------------------------------------------- 6. eval / frozen
def test_eval_mode_ignores_the_rate_and_takes_the_frozen_path(monkeypatch):
    """a teacher and an eval-mode student (BatchNorm with running statistics) built with dropout_rate 0.5 give bitwise the output of
    dropout_rate 0, on the frozen teacher's fused blocks, and draw nothing"""
    from cat_amd import frozen, networks, ops, rng
    opt = H.make_opt(norm='batch', track=True)
    g = H.load('forward_bn.npz')
    shapes = H.sd_from_shapes(g['student_shapes'])

    def teacher(rate):
        T = networks.define_G(3, 3, 64, 'inception_9blocks', 'batch', rate, 'normal', 0.02, [], opt=opt)
        T.load_state_dict(H.teacher_sd(opt))
        return T

    def student(rate):
        S = H.student_from_shapes(opt, shapes)
        S.load_state_dict(detfill.fill_state_dict(shapes, H.SEED_S))
        _set_rate(S, rate)
        return S
    x = ops.to_nhwc(detfill.images((1, 3, 64, 64), 3).to(DEV))
    for make in (teacher, student):
        outs, ncalls = [], []
        for rate in (0.0, 0.5):
            net = make(rate).to(DEV).eval()
            calls = []
            real = frozen.block_forward
            monkeypatch.setattr(frozen, 'block_forward', lambda b, x_, real=real, calls=calls: calls.append(1) or real(b, x_))
            before = rng.get_state(DEV)
            with torch.no_grad():
                outs.append(net(x).cpu())
            assert rng.get_state(DEV) == before
            monkeypatch.undo()
            ncalls.append(len(calls))
        assert ncalls[0] == ncalls[1] > 0, (make.__name__, ncalls)
        if make is teacher:
            assert ncalls[0] == 9
        assert torch.equal(outs[0], outs[1]), make.__name__


# ---------------------------------------------------------------------------------------------------------------- 7. graph replays
def test_graph_replays_equal_eager_steps_with_dropout():
    from cat_amd import nn as cnn, rng
    from cat_amd.graph import GraphedStep
    from cat_amd.inception_modules import InvertedResidualChannels
    from test_graph_gpu import _max_param_diff
    g = H.load('step_bn.npz')
    meta = json.loads(str(g['meta']))

    def build():
        opt = H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                         lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16)
        m = H.build_distiller(opt, g['student_shapes'])
        _set_rate(m.netG_student, 0.1)
        return m
    n, s = meta['nbatch'], meta['size']
    batches = [{'A': detfill.images((n, 3, s, s), 700 + i).cuda(), 'B': detfill.images((n, 3, s, s), 800 + i).cuda(), 'A_paths': [], 'B_paths': []}
               for i in range(3)]
    eager, graphed = build(), build()
    nblk = sum(isinstance(m, InvertedResidualChannels) for m in eager.netG_student.modules())
    assert any(isinstance(m, cnn.Dropout) and m.p == 0.1 for m in eager.netG_student.modules())
    rng.set_state(SEED, 0, DEV)
    for i in range(3):
        eager.set_input(batches[0])
        eager.optimize_parameters(i)
    c_eager = rng.get_state(DEV)[1]
    assert c_eager == 3 * nblk, (c_eager, nblk)         # the student's blocks draw once per forward; eval / frozen teacher never
    rng.set_state(SEED, 0, DEV)
    step = GraphedStep(graphed, batches[0], warmup=3)
    assert rng.get_state(DEV)[1] == c_eager
    for i in (1, 2, 1):
        rng.set_state(SEED, c_eager, DEV)
        eager.set_input(batches[i])
        eager.optimize_parameters(3 + i)
        c_eager = rng.get_state(DEV)[1]
        rng.set_state(SEED, c_eager - nblk, DEV)
        step(batches[i])
        assert rng.get_state(DEV)[1] == c_eager          # a replay advances the device counter like the eager step
        le, lg = eager.get_current_losses(), graphed.get_current_losses()
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-5 * max(1.0, abs(le[k])), (k, le[k], lg[k])
    assert _max_param_diff(graphed.netG_student, eager.netG_student) < 1e-5
    assert _max_param_diff(graphed.netD, eager.netD) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- 8. cycle_gan
def test_cyclegan_step_with_dropout_draws_per_forward():
    import random
    from cat_amd import rng
    from cat_amd.inception_modules import InvertedResidualChannels
    from cat_amd.models import create_model
    from test_train_models import _opt_for
    g = H.load('train_steps.npz')
    meta = json.loads(str(g['cyc_meta']))
    opt = _opt_for(meta, model='cycle_gan', dataset_mode='unaligned', lambda_A=meta['lambda_A'], lambda_B=meta['lambda_B'],
                   lambda_identity=meta['lambda_identity'], pool_size=meta['pool_size'])
    opt.dropout_rate = 0.5
    m = create_model(opt, verbose=False)
    gsh, dsh = H.sd_from_shapes(g['cyc_G_shapes']), H.sd_from_shapes(g['cyc_D_shapes'])
    m.netG_A.load_state_dict(detfill.fill_state_dict(gsh, 401))
    m.netG_B.load_state_dict(detfill.fill_state_dict(gsh, 402))
    m.netD_A.load_state_dict(detfill.fill_state_dict(dsh, 411))
    m.netD_B.load_state_dict(detfill.fill_state_dict(dsh, 412))
    m.setup(opt, verbose=False)
    for net in (m.netG_A, m.netG_B):
        blocks = [b for b in net.modules() if isinstance(b, InvertedResidualChannels)]
        assert blocks and all(b.dropout_rate == 0.5 for b in blocks)
    tickets = {}

    def spy(name):
        def hook(mod, inp):
            tickets.setdefault(name, []).append(int(rng.get_state(DEV)[1]))
        return hook
    first = {name: next(b for b in net.modules() if isinstance(b, InvertedResidualChannels)) for name, net in (('A', m.netG_A), ('B', m.netG_B))}
    handles = [b.register_forward_pre_hook(spy(name)) for name, b in first.items()]
    random.seed(meta['seed'])
    A, B = detfill.images((1, 3, 64, 64), 420), detfill.images((1, 3, 64, 64), 430)
    m.set_input({'A': A, 'B': B})
    m.optimize_parameters(0)
    torch.cuda.synchronize()
    for h in handles:
        h.remove()
    losses = m.get_current_losses()
    assert all(np.isfinite(v) for v in losses.values()), losses
    for name in ('A', 'B'):
        ds = tickets[name]
        assert len(ds) >= 2 and len(set(ds)) == len(ds), (name, ds)     # G(real) and G(fake) (+ identity) draw different d
