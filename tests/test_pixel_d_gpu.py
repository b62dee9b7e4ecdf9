"""GPU: the 1x1 PixelGAN discriminator (`--netD pixel`) on the fused kernels of csrc/pixel_d.hip and on the general kernels, against a stock-torch
float64 nn.Sequential twin built from the same state_dict (tests/golden/pixel_d.npz pins that twin to the reference's own numbers).

Bars: helpers.rel_err (max-abs error over max-abs reference) <= 1e-4 for the output, dx and every parameter gradient -- the bar of
test_kernels_gpu.py.  conv2's bias gradient under InstanceNorm is a sum that cancels to zero: it is compared absolutely against 1e-4 x the twin's
sum |dz|.  LeakyReLU's derivative jumps at 0, so every case picks the first detfill seed for which none of the twin's two pre-activations lies
within 1e-5 of zero and asserts that on the twin: a property of the inputs, no element is excluded.

Shapes (N, C0, H, W, ndf) -- the smallest at which the plan can go wrong:
  (3, 6, 5, 7, 16)    pixel stride 8 with pad lanes (poisoned with 1e30), 35 pixels per image: no multiple of any tile, three instance groups
  (2, 3, 8, 8, 48)    pixel stride 4; 48 / 96 channels: 3 channel tiles, 24 quads per pixel (no power of two), hidden width padded to 64
  (1, 6, 8, 8, 128)   the default width's LDS / register plan
  (1, 3, 40, 52, 16)  2080 pixels: 9 statistics entries over 3 workgroups, 33 backward tiles over 9 workgroups -> every workgroup walks several
                      tiles (a ragged last one) and the ordered reduce adds 9 partials
  (2, 1, 6, 6, 16)    one input channel (grayscale cycle_gan): the first conv's weight is never re-housed, its rows stay dense (row stride 1)
  (2, 5, 6, 6, 16)    five input channels: pixel stride 8 with three pad lanes, weight rows of 8"""
import itertools
import json

import numpy as np
import pytest
import torch
from torch import nn

import helpers as H
from oracle import detfill
from test_loss_multi_gpu import dev, grad_buffer, padded

pytestmark = pytest.mark.gpu

BAR = 1e-4
KINK = 1e-5
SHAPES = {'pad': (3, 6, 5, 7, 16), 'ndf48': (2, 3, 8, 8, 48), 'ndf128': (1, 6, 8, 8, 128), 'walk': (1, 3, 40, 52, 16),
          'c1': (2, 1, 6, 6, 16), 'c5': (2, 5, 6, 6, 16)}
CASES = [(s, n, False) for s in SHAPES for n in ('instance', 'batch')] + [('pad', 'instance', True)]
SEED_W = 61


def build(norm, c0, ndf, affine=False, seed=SEED_W):
    from cat_amd import networks
    opt = H.make_opt(norm=norm, track=norm not in ('instance', 'none'), ndf=ndf)
    opt.norm_affine_D = affine
    D = networks.define_D(c0, ndf, 'pixel', 3, norm, 'normal', 0.02, [0], opt=opt)
    D.load_state_dict(detfill.fill_state_dict(D.state_dict(), seed))
    return D.train()


def twin_of(D):
    """The stock-torch float64 twin of a PixelDiscriminator, on the host, from its state_dict."""
    sd = {k[len('net.'):]: v.detach().cpu().double() for k, v in D.state_dict().items()}
    c0, ndf = sd['0.weight'].shape[1], sd['0.weight'].shape[0]
    src = D.net[3]
    if isinstance(src, nn.InstanceNorm2d):
        norm = nn.InstanceNorm2d(2 * ndf, eps=src.eps, affine=src.affine, track_running_stats=False)
    elif isinstance(src, nn.BatchNorm2d):
        norm = nn.BatchNorm2d(2 * ndf, eps=src.eps, momentum=src.momentum, affine=src.affine, track_running_stats=src.track_running_stats)
    else:
        norm = nn.Identity()
    t = nn.Sequential(nn.Conv2d(c0, ndf, 1), nn.LeakyReLU(0.2), nn.Conv2d(ndf, 2 * ndf, 1, bias='2.bias' in sd), norm, nn.LeakyReLU(0.2),
                      nn.Conv2d(2 * ndf, 1, 1, bias='5.bias' in sd)).double()
    t.load_state_dict(sd, strict=True)
    return t.train(D.training)


def kink_margin(twin, x):
    """Smallest |pre-activation| in front of the twin's two LeakyReLUs."""
    with torch.no_grad():
        sd = {k: v.clone() for k, v in twin.state_dict().items()}
        p1 = twin[0](x.double())
        p2 = twin[3](twin[2](twin[1](p1)))
        twin.load_state_dict(sd)      # a train-mode BatchNorm moved its running statistics
    return min(float(p1.abs().min()), float(p2.abs().min()))


def pick_input(twin, shape, seed0):
    for seed in range(seed0, seed0 + 64):
        x = detfill.normal(shape, seed)
        if kink_margin(twin, x) > KINK:
            return x, seed
    raise AssertionError('no seed without a pre-activation near a LeakyReLU kink')


def twin_run(twin, x, gout, n_calls=1):
    """Forward (+ backward seeded with gout) of a fresh copy of the twin -> out, dx, parameter gradients by state_dict key, sum |dz|, the copy."""
    import copy
    t = copy.deepcopy(twin)
    xs = x if isinstance(x, (list, tuple)) else [x]
    gs = gout if isinstance(gout, (list, tuple)) else [gout]
    outs, leaves, dz_abs = [], [], []

    def tap(module, inputs, output):      # returns None: the output passes through
        output.register_hook(lambda g: dz_abs.append(float(g.abs().sum())))
    hook = t[2].register_forward_hook(tap)
    for xi in xs:
        leaf = xi.double().clone().requires_grad_(True)
        leaves.append(leaf)
        outs.append(t(leaf))
    torch.autograd.backward(outs, [g.double() for g in gs])
    hook.remove()
    grads = {'net.' + k: p.grad for k, p in t.named_parameters()}
    return [o.detach() for o in outs], [l.grad for l in leaves], grads, sum(dz_abs), t


def gpu_run(D, x, gout, params, poison=True):
    """One forward + backward on the device.  params=True: parameter gradients, x needs none; False: parameters frozen, dx wanted.
    -> (output buffer with its pad lanes, dx buffer or None, {key: gradient})"""
    for p in D.parameters():
        p.requires_grad_(params)
        p.grad = None
    leaf, cap = padded(x, 1e30 if poison else 0.0), []
    if not params:
        leaf.requires_grad_(True)
        leaf.register_hook(cap.append)
    out = D(leaf)
    out.backward(padded(gout, 1e30 if poison else 0.0))
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().double() for k, p in D.named_parameters()} if params else {}
    for p in D.parameters():
        p.requires_grad_(True)
    return grad_buffer(out.detach()).cpu(), (grad_buffer(cap[0]).cpu() if cap else None), grads


def check(tag, got, ref, scale_abs=None):
    if scale_abs is not None:
        err = float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max())
        print('%-24s abs err %.3g (bar %.3g)' % (tag, err, BAR * scale_abs))
        assert err <= BAR * scale_abs, (tag, err)
        return
    err = H.rel_err(got, ref)
    print('%-24s rel err %.3g' % (tag, err))
    assert err <= BAR, (tag, err)


def compare_with_twin(D, twin, x, gout, inst, label):
    """Both backward forms against the twin, pad lanes, and a second run bit for bit."""
    (ref_out,), (ref_dx,), ref_grads, dz_abs, _ = twin_run(twin, x, gout)
    n, c0 = x.shape[:2]
    sd0 = {k: v.clone() for k, v in D.state_dict().items()}
    runs = []
    for rep in range(2):
        D.load_state_dict(sd0)      # BatchNorm's running statistics moved
        a = gpu_run(D, x, gout, params=True)
        D.load_state_dict(sd0)
        b = gpu_run(D, x, gout, params=False)
        runs.append((a, b))
    (out, _, grads), (out2, dx, _) = runs[0]
    check(label + ' out', out[..., 0], ref_out[:, 0])
    assert torch.equal(out, out2)
    assert torch.count_nonzero(out[..., 1:]) == 0 and out.shape[-1] == 4
    check(label + ' dx', dx[..., :c0].permute(0, 3, 1, 2), ref_dx)
    assert torch.count_nonzero(dx[..., c0:]) == 0 and dx.shape[-1] == (c0 + 3) // 4 * 4
    assert sorted(grads) == sorted(ref_grads)
    for k, ref in ref_grads.items():
        if inst and k == 'net.2.bias':
            check(label + ' ' + k, grads[k], ref, scale_abs=dz_abs)
        else:
            check(label + ' ' + k, grads[k], ref)
    (o1, _, g1), (o2, d2, _) = runs[1]
    assert torch.equal(o1, out) and torch.equal(o2, out2) and torch.equal(d2, dx)
    assert all(torch.equal(g1[k], grads[k]) for k in grads)


@pytest.mark.parametrize('shape,norm,affine', CASES, ids=['%s-%s%s' % (s, n, '-affine' if a else '') for s, n, a in CASES])
def test_fused_path_matches_the_float64_twin(shape, norm, affine):
    from cat_amd import pixel_d
    n, c0, h, w, ndf = SHAPES[shape]
    D = build(norm, c0, ndf, affine)
    twin = twin_of(D)
    x, seed = pick_input(twin, (n, c0, h, w), 700 + 10 * list(SHAPES).index(shape))
    margin = kink_margin(twin, x)
    print('seed %d: smallest |pre-activation| %.3g' % (seed, margin))
    assert margin > KINK
    assert pixel_d.applicable(D, padded(x))
    if shape == 'walk':
        pl = pixel_d.plan(pixel_d.geometry(n, h * w, c0, 4, ndf, n if norm == 'instance' else 1))
        print('plan: %d entries over %d workgroups, %d backward tiles over %d workgroups' % (n * pl.tiles, pl.fwd_grid, pl.b2_tiles, pl.b2_grid))
        assert 2 * pl.fwd_grid <= n * pl.tiles and 2 * pl.b2_grid <= pl.b2_tiles and pl.b2_grid > 1 and pl.fwd_grid > 1
        assert (h * w) % pl.tile_px and (h * w) % 64
    gout = 2 * twin_run(twin, x, torch.zeros(n, 1, h, w))[0][0].float()      # the gradient of sum(out ** 2)
    compare_with_twin(D, twin, x, gout, norm == 'instance', '%s %s' % (shape, norm))


@pytest.mark.parametrize('norm', ['instance', 'batch'])
def test_twin_is_pinned_to_the_reference(norm):
    """tests/golden/pixel_d.npz: the reference PixelDiscriminator's own float64 output and gradients of sum(out ** 2); the twin reproduces them
    to float64 rounding, the fused path to the bar."""
    g = H.load('pixel_d.npz')
    meta = json.loads(str(g['meta']))
    D = build(norm, meta['input_nc'], meta['ndf'], seed=meta['seed_w'])
    twin = twin_of(D)
    x = detfill.normal(tuple(meta['shape']), meta['seed_x'])
    (y,), _, _, _, _ = twin_run(twin, x, torch.zeros(2, 1, 8, 8))
    (out,), (dx,), grads, dz_abs, _ = twin_run(twin, x, 2 * y)
    assert H.rel_err(out, g[f'out:{norm}']) < 1e-12 and H.rel_err(dx, g[f'dx:{norm}']) < 1e-10
    for k, v in grads.items():
        ref = g[f'grad:{norm}:{k}']
        assert np.abs(v.numpy() - ref).max() <= 1e-10 * max(np.abs(ref).max(), dz_abs), k
    assert kink_margin(twin, x) > KINK
    got, _, ggrads = gpu_run(D, x, (2 * y).float(), params=True, poison=False)
    check('reference out', got[..., 0], g[f'out:{norm}'][:, 0])
    for k in ggrads:
        check('reference ' + k, ggrads[k], g[f'grad:{norm}:{k}'], scale_abs=dz_abs if (norm == 'instance' and k == 'net.2.bias') else None)


def test_batch_norm_statistics_and_syncbatch():
    """running_mean / running_var after one forward against the twin; num_batches_tracked advances for `batch`, never for the replica-local
    `syncbatch`, which is otherwise bit-identical to `batch` from equal weights."""
    from cat_amd import pixel_d
    n, c0, h, w, ndf = SHAPES['pad']
    Db, Ds = build('batch', c0, ndf), build('syncbatch', c0, ndf)
    assert list(Db.state_dict()) == list(Ds.state_dict())
    twin = twin_of(Db)
    x, _ = pick_input(twin, (n, c0, h, w), 700)
    gout = detfill.normal((n, 1, h, w), 790)
    _, _, _, _, t_after = twin_run(twin, x, gout)
    assert pixel_d.applicable(Db, padded(x)) and pixel_d.applicable(Ds, padded(x))
    ob, _, gb = gpu_run(Db, x, gout, params=True)
    os_, _, gs = gpu_run(Ds, x, gout, params=True)
    for key in ('running_mean', 'running_var'):
        ref = getattr(t_after[3], key)
        err = H.rel_err(getattr(Db.net[3], key).cpu(), ref)
        print('%s rel err %.3g' % (key, err))
        assert err <= 1e-5
        assert torch.equal(getattr(Db.net[3], key), getattr(Ds.net[3], key))
    assert int(Db.net[3].num_batches_tracked) == 1 and int(t_after[3].num_batches_tracked) == 1
    assert int(Ds.net[3].num_batches_tracked) == 0
    assert torch.equal(ob, os_) and all(torch.equal(gb[k], gs[k]) for k in gb)
    _, dxb, _ = gpu_run(Db, x, gout, params=False)
    _, dxs, _ = gpu_run(Ds, x, gout, params=False)
    assert torch.equal(dxb, dxs)


@pytest.mark.parametrize('shape', ['pad', 'ndf48', 'c1'])
@pytest.mark.parametrize('norm', ['instance', 'batch'])
def test_fused_agrees_with_the_general_path(shape, norm, monkeypatch):
    from cat_amd import pixel_d
    n, c0, h, w, ndf = SHAPES[shape]
    D = build(norm, c0, ndf)
    twin = twin_of(D)
    x, _ = pick_input(twin, (n, c0, h, w), 700 + 10 * list(SHAPES).index(shape))
    gout = detfill.normal((n, 1, h, w), 791)
    dz_abs = twin_run(twin, x, gout)[3]
    sd0 = {k: v.clone() for k, v in D.state_dict().items()}
    res = {}
    for on in (True, False):
        monkeypatch.setattr(pixel_d, 'ENABLED', on)
        assert pixel_d.applicable(D, padded(x)) is on
        D.load_state_dict(sd0)
        o, _, g = gpu_run(D, x, gout, params=True, poison=False)      # the general kernels rely on zero pad lanes
        D.load_state_dict(sd0)
        _, dx, _ = gpu_run(D, x, gout, params=False, poison=False)
        res[on] = (o[..., 0], dx[..., :c0], g)
    for name, a, b in [('out', res[True][0], res[False][0]), ('dx', res[True][1], res[False][1])] + \
                      [(k, res[True][2][k], res[False][2][k]) for k in res[True][2]]:
        scale = max(float(b.abs().max()), 1e-30)
        err = float((a - b).abs().max()) / scale
        print('%s %s %-14s fused vs general %.3g' % (shape, norm, name, err))
        if norm == 'instance' and name == 'net.2.bias':      # both are rounding noise around an exact zero: absolute, against sum |dz|
            assert float((a - b).abs().max()) <= 2e-4 * dz_abs, (name, float((a - b).abs().max()))
            continue
        assert err <= 2e-4, (name, err)


@pytest.mark.parametrize('what', ['ndf24', 'none', 'eval'])
def test_declined_configurations_take_the_general_path(what):
    from cat_amd import pixel_d
    n, c0, h, w = 2, 6, 8, 8
    D = build('none' if what == 'none' else 'batch', c0, 24 if what == 'ndf24' else 16)
    if what == 'eval':
        D.eval()
    twin = twin_of(D)
    x, _ = pick_input(twin, (n, c0, h, w), 760)
    gout = detfill.normal((n, 1, h, w), 792)
    if what == 'eval':
        with torch.no_grad():
            assert not pixel_d.applicable(D, padded(x))
            out = D(padded(x, 0.0))
            ref = twin(x.double())
        check('eval out', out.cpu()[:, 0], ref[:, 0])
        return
    assert not pixel_d.applicable(D, padded(x))
    (ref_out,), (ref_dx,), ref_grads, _, _ = twin_run(twin, x, gout)
    out, _, grads = gpu_run(D, x, gout, params=True, poison=False)      # the general kernels rely on zero pad lanes
    check(what + ' out', out[..., 0], ref_out[:, 0])
    for k, ref in ref_grads.items():
        check(what + ' ' + k, grads[k], ref)
    _, dx, _ = gpu_run(D, x, gout, params=False, poison=False)
    check(what + ' dx', dx[..., :c0].permute(0, 3, 1, 2), ref_dx)


@pytest.mark.parametrize('shape', ['pad', 'c1'])
@pytest.mark.parametrize('norm', ['instance', 'batch'])
def test_two_calls_accumulate_into_the_optimizer_bucket(norm, shape):
    """backward_D's pattern: two discriminator calls, one backward, gradients in a FusedAdam-owned flat bucket = the twin's sum."""
    from cat_amd import optim, pixel_d
    n, c0, h, w, ndf = SHAPES[shape]
    D = build(norm, c0, ndf, affine=True)
    twin = twin_of(D)
    xa, sa = pick_input(twin, (n, c0, h, w), 700)
    xb, _ = pick_input(twin, (n, c0, h, w), sa + 1)
    ga, gb = detfill.normal((n, 1, h, w), 793), detfill.normal((n, 1, h, w), 794)
    _, _, ref_grads, dz_abs, _ = twin_run(twin, [xa, xb], [ga, gb])
    opt = optim.FusedAdam(D.parameters(), lr=1e-3)
    opt.zero_grad()
    assert all(optim.owned(p) for p in D.parameters()) and pixel_d.applicable(D, padded(xa))
    outs = [D(padded(xa)), D(padded(xb))]
    torch.autograd.backward(outs, [padded(ga), padded(gb)])
    torch.cuda.synchronize()
    flat = opt.flat_grads()[0]
    for k, p in D.named_parameters():
        assert p.grad.data_ptr() == p._cat_grad_view.data_ptr() and flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + 4 * flat.numel()
        check('two calls ' + k, p.grad.detach().cpu(), ref_grads[k], scale_abs=dz_abs if (norm == 'instance' and k == 'net.2.bias') else None)
    opt.zero_grad()
    D(padded(xa)).backward(padded(ga))      # the first writer after zero_grad overwrites
    _, _, one, dz1, _ = twin_run(twin_of(D), xa, ga)
    for k, p in D.named_parameters():
        check('after zero_grad ' + k, p.grad.detach().cpu(), one[k], scale_abs=dz1 if (norm == 'instance' and k == 'net.2.bias') else None)


# ------------------------------------------------------------------------------------------------------------------ through the models
def build_pixel_distiller(g):
    """helpers.build_distiller with a detfill-filled pixel discriminator (that helper loads an n_layers state_dict)."""
    from cat_amd import nn as cnn
    from cat_amd.distillers import create_distiller
    from cat_amd.optim import FusedAdam
    meta = json.loads(str(g['meta']))
    opt = H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                     lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16,
                     distill_G_loss_type=meta.get('distill', 'ka'), netD=meta['netD'])
    model = create_distiller(opt, verbose=False)
    model.netG_teacher.load_state_dict(H.teacher_sd(opt))
    shapes = H.sd_from_shapes(g['student_shapes'])
    student = H.student_from_shapes(opt, shapes).to(model.device)
    student.load_state_dict(detfill.fill_state_dict(shapes, H.SEED_S))
    model.netG_student = student.train()
    model.netD.load_state_dict(detfill.fill_state_dict(model.netD.state_dict(), H.SEED_D))
    model.netD.train()
    trunk = student.state_dict()['down_sampling.7.weight'].shape[0]
    model.netAs = [cnn.Conv2d(trunk, a.out_channels, 1).to(model.device) for a in model.netAs]
    for a, sd in zip(model.netAs, H.netA_sds(student.state_dict())):
        a.load_state_dict(sd)
    gp = [a.parameters() for a in model.netAs]
    model.optimizer_G = FusedAdam([{'params': model.netG_student.parameters()}, {'params': itertools.chain(*gp)}], lr=opt.lr, betas=(opt.beta1, 0.999))
    model.optimizers = [model.optimizer_G, model.optimizer_D]
    model.setup(opt, verbose=False)
    return model, meta


def test_two_distill_steps_with_pixel_d_match_reference():
    """tests/golden/step_pixel.npz (tools/make_golden_pixel_d.py): the reference's own two optimize_parameters steps with netD='pixel'; loop and
    bars of test_smooth_l1_gpu.test_two_distill_steps_match_reference."""
    from cat_amd import discriminators, ops, pixel_d
    TOL = 1e-3
    g = H.load('step_pixel.npz')
    model, meta = build_pixel_distiller(g)
    assert type(model.netD) is discriminators.PixelDiscriminator and meta['netD'] == 'pixel'
    assert model.d_stage_plan() is None      # the data-parallel schedule takes plain backward_D
    b2_start = model.netD.state_dict()['net.2.bias'].detach().cpu().clone()
    calls = []
    real_forward = pixel_d.forward
    pixel_d.forward = lambda m, x: (calls.append(1), real_forward(m, x))[1]
    ops.STATS['conform_copies'] = 0
    try:
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
            seen_d = 0
            for key in g.files:
                if key.startswith((f'S{step}:', f'D{step}:', f'A{step}:')):
                    sd = {'S': ssd, 'D': dsd, 'A': asd}[key[0]]
                    seen_d += key[0] == 'D'
                    got = sd[key.split(':', 1)[1]].detach().cpu().reshape(-1)[:len(g[key])].numpy()
                    diff, scale = np.abs(got - g[key]), np.abs(g[key]).max()
                    assert np.quantile(diff, 0.75) <= 2e-5 + 2e-4 * scale, (key, diff)
                    assert diff.max() <= 2 * meta['lr'] * (step + 1) + 1e-3 * scale, (key, diff)
            assert seen_d == len(dsd) - 1
            # net.2.bias sits in front of InstanceNorm: its gradient is exactly zero, Adam turns the rounding noise into steps of about lr (the max bar above)
            b2 = dsd['net.2.bias'].detach().cpu()
            assert float((b2 - b2_start).abs().max()) <= 2 * meta['lr'] * (step + 1)
    finally:
        pixel_d.forward = real_forward
    assert ops.STATS['conform_copies'] == 0
    assert len(calls) == 6      # three discriminator calls per step, all on the fused path


def test_graph_replay_equals_eager_with_pixel_d():
    """The same two steps replayed through cat_amd.graph.GraphedStep give the eager run's losses and weights (test_graph_gpu.py's criterion)."""
    from cat_amd.graph import GraphedStep
    from test_graph_gpu import _max_param_diff
    g = H.load('step_pixel.npz')
    (eager, meta), (graphed, _) = build_pixel_distiller(g), build_pixel_distiller(g)
    n, s = meta['nbatch'], meta['size']
    batches = [{'A': detfill.images((n, 3, s, s), 500 + i).cuda(), 'B': detfill.images((n, 3, s, s), 600 + i).cuda(), 'A_paths': [], 'B_paths': []}
               for i in range(3)]
    for i in range(3):
        eager.set_input(batches[0])
        eager.optimize_parameters(i)
    step = GraphedStep(graphed, batches[0], warmup=3)
    for i in (1, 2):
        eager.set_input(batches[i])
        eager.optimize_parameters(3 + i)
        step(batches[i])
        le, lg = eager.get_current_losses(), graphed.get_current_losses()
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-5 * max(1.0, abs(le[k])), (k, le[k], lg[k])
    assert _max_param_diff(graphed.netG_student, eager.netG_student) < 1e-5
    assert _max_param_diff(graphed.netD, eager.netD) < 1e-5


def _teacher_step(model_name, **kw):
    from cat_amd import discriminators
    from cat_amd.models import create_model
    opt = H.make_opt(ndf=16, ngf=8, netG='inception_9blocks', dropout_rate=0, direction='AtoB', model=model_name, netD='pixel', **kw)
    m = create_model(opt, verbose=False)
    nets = [k for k in vars(m) if k.startswith('net') and isinstance(getattr(m, k), nn.Module)]
    for i, name in enumerate(sorted(nets)):
        net = getattr(m, name)
        net.load_state_dict(detfill.fill_state_dict(net.state_dict(), 401 + i))
    m.setup(opt, verbose=False)
    ds = [getattr(m, k) for k in sorted(nets) if k.startswith('netD')]
    assert ds and all(type(d) is discriminators.PixelDiscriminator for d in ds)
    return m, ds


def test_pix2pix_step_with_pixel_d():
    m, (d,) = _teacher_step('pix2pix', norm='batch', track=True, gan_mode='hinge', lambda_recon=10.0, lambda_gan=1.0)
    assert d.net[0].in_channels == 6
    before = m.netG.state_dict()['up_sampling.7.weight'].detach().clone()
    d_before = d.net[2].weight.detach().clone()
    m.set_input({'A': detfill.images((2, 3, 64, 64), 310), 'B': detfill.images((2, 3, 64, 64), 320), 'A_paths': [], 'B_paths': []})
    m.optimize_parameters(0)
    losses = m.get_current_losses()
    print(losses)
    assert len(losses) >= 4 and all(np.isfinite(v) for v in losses.values())
    assert not torch.equal(m.netG.state_dict()['up_sampling.7.weight'].detach(), before)
    assert not torch.equal(d.net[2].weight.detach(), d_before) and int(d.net[3].num_batches_tracked) == 3


def test_cycle_gan_step_with_pixel_d():
    """C0 = 3 and two discriminators in one FusedAdam bucket."""
    import random
    m, ds = _teacher_step('cycle_gan', norm='instance', track=False, gan_mode='lsgan', dataset_mode='unaligned', lambda_A=10.0, lambda_B=10.0,
                          lambda_identity=0.5, pool_size=2)
    assert len(ds) == 2 and all(d.net[0].in_channels == 3 for d in ds)
    random.seed(1234)
    before = [m.netG_A.state_dict()['up_sampling.7.weight'].detach().clone(), m.netG_B.state_dict()['up_sampling.7.weight'].detach().clone()]
    d_before = [d.net[2].weight.detach().clone() for d in ds]
    m.set_input({'A': detfill.images((2, 3, 64, 64), 420), 'B': detfill.images((2, 3, 64, 64), 430)})
    m.optimize_parameters(0)
    torch.cuda.synchronize()
    losses = m.get_current_losses()
    print(losses)
    assert len(losses) >= 8 and all(np.isfinite(v) for v in losses.values())
    assert not torch.equal(m.netG_A.state_dict()['up_sampling.7.weight'].detach(), before[0])
    assert not torch.equal(m.netG_B.state_dict()['up_sampling.7.weight'].detach(), before[1])
    assert all(not torch.equal(d.net[2].weight.detach(), b) for d, b in zip(ds, d_before))
    flat = m.optimizer_D.flat_grads()
    assert len(flat) == 1 and all(p._cat_grad_view.untyped_storage().data_ptr() == flat[0].untyped_storage().data_ptr()
                                  for d in ds for p in d.parameters())
