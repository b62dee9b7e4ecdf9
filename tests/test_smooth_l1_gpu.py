"""GPU: the smooth-L1 reconstruction loss (torch.nn.SmoothL1Loss() with its defaults, beta 1, mean reduction: the L1 kind of cat_loss_fwd /
cat_loss_bwd and of cat_loss_multi_* with beta as its `target`; the loss-kind table is pinned at eight kinds by test_abi.py, and beta 0 is
plain L1 bit for bit) against float64 F.smooth_l1_loss on the host, alone through ops.LossFn and as one term of ops.MultiLossFn next to a
plain L1 term, and through the two models that take `--recon_loss_type smooth_l1`.

Inputs as in test_loss_multi_gpu.py: NHWC buffers whose pad lanes hold 1e30, a = normal * 1.5, b = normal, so a - b ~ N(0, 3.25) and about
42 % of the elements fall in the quadratic branch.  Bars (the project's LOSS_BAR): 1e-6 relative to max(1, |f64|) for the mean -- a float32
wave-tree sum of <= 3075 terms is good to a few 1e-7 -- and 1e-6 relative for the gradient (the rounding of a - b and two multiplies)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as H
from oracle import detfill
from test_loss_multi_gpu import dev, grad_buffer, padded, relerr

pytestmark = pytest.mark.gpu

L1 = 0
SMOOTH_L1 = (L1, 1.0)      # (kind, target): beta 1
BAR = 1e-6
SHAPES = [(360, 5), (1025, 3)]      # (M, C): cs 8 with pad lanes, 720 quads, one workgroup; cs 4, 1025 quads, two workgroups
GOUT = (0.75, -0.5)                 # backward seeds of the (L1, smooth-L1) terms


def f64_smooth_l1(a, b, beta=1.0):
    a = a.double().clone().requires_grad_(True)
    v = F.smooth_l1_loss(a, b.double(), beta=beta)
    v.backward()
    return float(v), a.grad


def _single(a, b, gout, beta=1.0):
    """smooth-L1 alone through ops.LossFn -> (0-d value, the kernel's gradient buffer with its pad lanes, the gradient in float64)."""
    from cat_amd import ops
    leaf, cap = padded(a).requires_grad_(True), []
    leaf.register_hook(cap.append)
    out = ops.LossFn.apply(leaf, padded(b), L1, beta)
    out.backward(torch.full((), gout, device=dev()))
    return out.detach(), grad_buffer(cap[0]).cpu(), leaf.grad.detach().double().cpu()


def _multi(a, b, a1, b1):
    """(L1 of (a1, b1), smooth-L1 of (a, b)) in one MultiLossFn call -> the second term's value and gradient buffer."""
    from cat_amd import ops
    leaves, raw = [padded(a1).requires_grad_(True), padded(a).requires_grad_(True)], {}
    for t, x in enumerate(leaves):
        x.register_hook(lambda grad, t=t: raw.__setitem__(t, grad))
    outs = ops.MultiLossFn.apply(((L1, 0.0), SMOOTH_L1), leaves[0], padded(b1), leaves[1], padded(b))
    torch.autograd.backward(list(outs), [torch.full((), g, device=dev()) for g in GOUT])
    return outs[0].detach(), outs[1].detach(), grad_buffer(raw[1]).cpu(), leaves[1].grad.detach().double().cpu()


@pytest.mark.parametrize('m,c', SHAPES)
def test_smooth_l1_matches_float64_alone_and_in_a_table(m, c):
    shape = (1, c, m, 1)
    a, b = detfill.normal(shape, 1200 + m) * 1.5, detfill.normal(shape, 1201 + m)
    a1, b1 = detfill.normal(shape, 1202 + m) * 1.5, detfill.normal(shape, 1203 + m)
    quad = float(((a - b).abs() < 1).double().mean())
    print('(M, C) = (%d, %d): %.1f %% of the elements in the quadratic branch' % (m, c, 100 * quad))
    assert 0.2 <= quad <= 0.8
    ref, gref = f64_smooth_l1(a, b)
    one, one_buf, one_grad = _single(a, b, GOUT[1])
    l1, many, many_buf, many_grad = _multi(a, b, a1, b1)
    errs = relerr(one_grad, gref * GOUT[1]), relerr(many_grad, gref * GOUT[1])
    print('mean: LossFn %.9g  MultiLossFn %.9g  f64 %.9g;  gradient relative error %.3g / %.3g' % (float(one), float(many), ref, *errs))
    assert abs(float(one) - ref) <= BAR * max(1.0, abs(ref)) and abs(float(many) - ref) <= BAR * max(1.0, abs(ref))
    assert errs[0] < BAR and errs[1] < BAR
    l1_ref = float((a1.double() - b1.double()).abs().mean())
    assert abs(float(l1) - l1_ref) <= BAR * max(1.0, l1_ref)      # the neighbouring term is still its own
    cs = (c + 3) // 4 * 4
    assert one_buf.shape[-1] == cs and torch.count_nonzero(one_buf[..., c:]) == 0 and torch.count_nonzero(many_buf[..., c:]) == 0
    assert torch.count_nonzero(one_buf[..., :c]) == m * c      # d = 0 has measure zero here
    assert torch.equal(one.cpu(), many.cpu()) and torch.equal(one_buf, many_buf)      # one definition of the arm, one summation order


def test_other_betas_and_plain_l1():
    """beta 0.5 against float64, and beta 0 -- what every L1 caller passes -- against float64 |a - b|, at the pad-lane shape."""
    m, c = SHAPES[0]
    a, b = detfill.normal((1, c, m, 1), 1250) * 1.5, detfill.normal((1, c, m, 1), 1251)
    for beta in (0.5, 0.0):
        ref, gref = f64_smooth_l1(a, b, beta)
        out, buf, grad = _single(a, b, GOUT[1], beta)
        print('beta %g: mean %.9g (f64 %.9g), gradient relative error %.3g' % (beta, float(out), ref, relerr(grad, gref * GOUT[1])))
        assert abs(float(out) - ref) <= BAR * max(1.0, abs(ref)) and relerr(grad, gref * GOUT[1]) < BAR
        assert torch.count_nonzero(buf[..., c:]) == 0
    assert abs(ref - float((a.double() - b.double()).abs().mean())) < 1e-15      # F.smooth_l1_loss(beta=0) is F.l1_loss
    assert set(grad.reshape(-1).float().abs().mul(m * c / abs(GOUT[1])).round().tolist()) == {1.0}      # +-gout / (M C), nothing in between


def test_kinks():
    """|d| = 1 and its float32 neighbours, and d = 0: value and derivative are continuous at the kink, so the float64 bar holds whichever
    branch the kernel's float32 comparison takes."""
    e = 2.0 ** -20
    d = torch.tensor([0.0, 1.0, -1.0, 1 - e, -(1 - e), 1 + e, -(1 + e)], dtype=torch.float32)
    assert d[3] < 1 < d[5]      # representable: 2^-20 is 8 ulps of 1
    b = detfill.normal((7,), 1300)
    for base in (torch.zeros(7), b):
        a = (base + d).reshape(1, 7, 1, 1)
        bb = base.reshape(1, 7, 1, 1).clone()
        ref, gref = f64_smooth_l1(a, bb)
        out, buf, grad = _single(a, bb, 1.0)
        print('kinks: mean %.9g (f64 %.9g), gradient relative error %.3g' % (float(out), ref, relerr(grad, gref)))
        assert abs(float(out) - ref) <= BAR * max(1.0, abs(ref))
        assert relerr(grad, gref) < BAR
        assert torch.count_nonzero(buf[..., 7:]) == 0
    # with b = 0 the differences are exact in float32: d = 0 gives exactly 0 both ways, |d| >= 1 exactly +-1 / 7
    a = d.reshape(1, 7, 1, 1)
    _, _, grad = _single(a, torch.zeros(1, 7, 1, 1), 1.0)
    g = grad.reshape(-1).float()
    seventh = torch.tensor(1.0) / torch.tensor(7.0)
    assert g[0] == 0 and g[1] == seventh and g[2] == -seventh and g[5] == seventh and g[6] == -seventh
    assert 0 < g[3] <= seventh and -seventh <= g[4] < 0


def test_two_distill_steps_match_reference():
    """The `in` configuration with recon_loss_type='smooth_l1', two optimize_parameters steps against the reference's own run
    (tests/golden/step_smooth_l1.npz, tools/make_golden_norm_recon.py); the bars of test_model_gpu.test_two_distill_steps_match_reference."""
    from cat_amd import loss as closs, ops
    TOL = 1e-3
    g = H.load('step_smooth_l1.npz')
    meta = json.loads(str(g['meta']))
    assert meta['recon_loss_type'] == 'smooth_l1'
    opt = H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                     lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16,
                     distill_G_loss_type=meta.get('distill', 'ka'), recon_loss_type='smooth_l1')
    model = H.build_distiller(opt, g['student_shapes'])
    assert type(model.criterionRecon) is closs.SmoothL1Loss
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
    assert ops.STATS['conform_copies'] == 0


def test_pix2pix_step_reports_lambda_times_smooth_l1():
    from cat_amd import loss as closs
    from cat_amd.models import create_model
    g = H.load('train_steps.npz')
    meta = json.loads(str(g['p2p_meta']))
    opt = H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], gan_mode=meta['gan_mode'], ngf=meta['ngf'], netG='inception_9blocks',
                     dropout_rate=0, direction='AtoB', lr=meta['lr'], beta1=meta['beta1'], model='pix2pix', lambda_recon=meta['lambda_recon'],
                     lambda_gan=1.0, recon_loss_type='smooth_l1')
    m = create_model(opt, verbose=False)
    assert type(m.criterionRecon) is closs.SmoothL1Loss
    m.netG.load_state_dict(detfill.fill_state_dict(H.sd_from_shapes(g['p2p_G_shapes']), 301))
    m.netD.load_state_dict(detfill.fill_state_dict(H.sd_from_shapes(g['p2p_D_shapes']), 302))
    m.setup(opt, verbose=False)
    before = m.netG.state_dict()['up_sampling.7.weight'].detach().clone()
    # targets scaled so that both branches of the loss are populated (tanh outputs against images in [-1, 1] alone stay mostly below 1)
    A, B = detfill.images((2, 3, 64, 64), 310), detfill.images((2, 3, 64, 64), 320) * 2.0
    m.set_input({'A': A, 'B': B, 'A_paths': [], 'B_paths': []})
    m.optimize_parameters(0)
    got = m.get_current_losses()['G_loss/G_recon']
    fake, real = m.fake_B.detach().cpu().double(), m.real_B.detach().cpu().double()
    quad = float(((fake - real).abs() < 1).double().mean())
    ref = meta['lambda_recon'] * float(F.smooth_l1_loss(fake, real))
    print('G_recon %.9g, lambda_recon * f64 smooth-L1 %.9g, %.1f %% quadratic' % (got, ref, 100 * quad))
    assert 0.05 < quad < 0.95
    assert abs(got - ref) <= 1e-6 * abs(ref)
    assert not torch.equal(m.netG.state_dict()['up_sampling.7.weight'].detach(), before)      # the step reached the generator
