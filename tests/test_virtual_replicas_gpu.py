"""GPU: virtual replicas -- one process on one GPU computes what S reference GPUs under nn.DataParallel compute on the same batch.
Kernel level against float64 on the host (BatchNorm over torch.chunk groups, sharded KA, the fused block against the layer-by-layer
path); step level against the oracle's DataParallel restatement (ref_cpu.distill_step / ref_spade_cpu.spade_step with n_shards), the
teacher step against its own halves, hipGraph replay against eager steps, and the launch count against S."""
import copy
import json

import pytest
import torch
import torch.nn.functional as F

import helpers as H
from oracle import detfill, ref_cpu

pytestmark = pytest.mark.gpu
TOL = 1e-4            # tests/test_kernels_gpu.py: the bar of cat_norm_fwd / cat_norm_bwd and (5 x) of the KA gradient


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _nhwc(x, dev, requires_grad=False):
    from cat_amd import ops
    y = ops.to_nhwc(x.to(dev))
    return y.detach().requires_grad_(True) if requires_grad else y


# ---------------------------------------------------------------------------------------------------------------- norm kernels
NORM_SHAPES = [(6, 3), (4, 2), (5, 2), (5, 4), (4, 4)]      # 3 groups of 2 | 2 of 2 | 3 + 2 | 2 + 2 + 1 (fewer groups than S) | 4 groups of 1


@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('c', [5, 20])
@pytest.mark.parametrize('n,s', NORM_SHAPES)
def test_sharded_batchnorm_fwd_bwd(dev, n, s, c, act):
    """Training BatchNorm over the torch.chunk(batch, S) groups against F.batch_norm in float64 on each chunk (gradients by autograd);
    running statistics and num_batches_tracked equal ATen's on chunk 0 ALONE (replica 0 shares its buffers with the module)."""
    from cat_amd import ops, _lib as L
    h, w = 7, 9
    x = detfill.normal((n, c, h, w), 13) * 2.0 + 3.0
    x = x + torch.arange(n, dtype=torch.float32).reshape(n, 1, 1, 1)      # every sample its own mean: a wrong grouping cannot pass
    ga, be = 1.0 + 0.2 * detfill.normal((c,), 14), 0.1 * detfill.normal((c,), 15)
    gy = detfill.normal((n, c, h, w), 16)
    xr, gr, br = x.double().requires_grad_(True), ga.double().requires_grad_(True), be.double().requires_grad_(True)
    rm, rv = torch.zeros(c, dtype=torch.float64), torch.ones(c, dtype=torch.float64)
    outs = []
    for i, xc in enumerate(xr.chunk(s, 0)):
        yc = F.batch_norm(xc, rm if i == 0 else None, rv if i == 0 else None, gr, br, True, 0.1, 1e-5)
        outs.append(F.relu(yc) if act == 1 else yc)
    yr = torch.cat(outs, 0)
    yr.backward(gy.double())
    xg = _nhwc(x, dev, True)
    gg, bg = ga.to(dev).requires_grad_(True), be.to(dev).requires_grad_(True)
    rmg, rvg, nbt = torch.zeros(c, device=dev), torch.ones(c, device=dev), torch.zeros((), dtype=torch.long, device=dev)
    y = ops.NormActFn.apply(xg, gg, bg, rmg, rvg, L.NORM_BATCH, 1e-5, 0.1, act, 0.2, nbt, None, s)
    e = dict(y=rel(y, yr), rm=rel(rmg, rm), rv=rel(rvg, rv))
    y.backward(_nhwc(gy, dev))
    e.update(dx=rel(xg.grad, xr.grad), dgamma=rel(gg.grad, gr.grad), dbeta=rel(bg.grad, br.grad))
    print('\n[sharded bn N=%d S=%d C=%d act=%d] %s' % (n, s, c, act, ' '.join('%s %.2e' % kv for kv in e.items())))
    assert e['y'] < TOL and e['rm'] < TOL and e['rv'] < TOL
    assert int(nbt) == 1
    assert e['dx'] < 5 * TOL and e['dgamma'] < TOL and e['dbeta'] < TOL


def test_one_virtual_replica_is_the_plain_batchnorm_bit_for_bit(dev):
    from cat_amd import ops, _lib as L
    n, c, h, w = 4, 20, 7, 9
    x, gy = detfill.normal((n, c, h, w), 13) * 2.0 + 3.0, detfill.normal((n, c, h, w), 16)
    ga, be = 1.0 + 0.2 * detfill.normal((c,), 14), 0.1 * detfill.normal((c,), 15)
    got = []
    for extra in ((), (None, None, 1)):
        xg = _nhwc(x, dev, True)
        gg, bg = ga.to(dev).requires_grad_(True), be.to(dev).requires_grad_(True)
        rmg, rvg = torch.zeros(c, device=dev), torch.ones(c, device=dev)
        y = ops.NormActFn.apply(xg, gg, bg, rmg, rvg, L.NORM_BATCH, 1e-5, 0.1, 1, 0.0, *extra)
        y.backward(_nhwc(gy, dev))
        got.append([t.detach().clone() for t in (y, rmg, rvg, xg.grad, gg.grad, bg.grad)])
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_module_reads_the_stamp_in_training_mode_only(dev):
    """nn.BatchNorm2d stamped with S = 2: per-shard statistics in train(), the running statistics in eval(); InstanceNorm2d ignores it."""
    from cat_amd import networks, nn as cnn
    n, c, h, w = 4, 5, 7, 9
    x = detfill.normal((n, c, h, w), 21) + torch.arange(n, dtype=torch.float32).reshape(n, 1, 1, 1)
    bn, inorm = cnn.BatchNorm2d(c).to(dev), cnn.InstanceNorm2d(c).to(dev)
    net = torch.nn.Sequential(bn, inorm)
    assert networks.set_virtual_replicas(net, 2) == 1
    ref = torch.nn.BatchNorm2d(c).double()
    with torch.no_grad():
        want = torch.cat([torch.nn.BatchNorm2d(c).double().train()(xc) for xc in x.double().chunk(2, 0)], 0)
        ref.train()(x.double()[:2])
        assert rel(bn.train()(_nhwc(x, dev)), want) < TOL
        assert rel(bn.running_mean, ref.running_mean) < TOL and rel(bn.running_var, ref.running_var) < TOL and int(bn.num_batches_tracked) == 1
        assert rel(bn.eval()(_nhwc(x, dev)), ref.eval()(x.double())) < TOL
        assert rel(inorm(_nhwc(x, dev)), F.instance_norm(x.double())) < TOL


# ---------------------------------------------------------------------------------------------------------------- sharded KA
@pytest.mark.parametrize('mean', [False, True])
@pytest.mark.parametrize('n,s', [(6, 3), (5, 2), (72, 2)])
def test_sharded_ka(dev, n, s, mean):
    """The sum / mean over the shards of KA(X_g, Y_g) and its gradient against per-chunk ka in float64; N = 72 > 64 rows in all."""
    from cat_amd import ops
    cx, cy, h, w = 8, 12, 4, 4      # Dx = 128, Dy = 192
    X, Y = detfill.normal((n, cx, h, w), 100 + n), detfill.normal((n, cy, h, w), 200 + n)
    Xr = X.double().requires_grad_(True)
    parts = [ref_cpu.ka(a, b) for a, b in zip(Xr.chunk(s, 0), Y.double().chunk(s, 0))]
    vr = sum(parts) / (len(parts) if mean else 1)
    (-1.3 * vr).backward()
    Xg = _nhwc(X, dev, True)
    v = ops.ka_sharded(Xg, _nhwc(Y, dev), s, mean)
    torch.autograd.backward([v], [torch.full((), -1.3, device=dev)])
    print('\n[sharded ka N=%d S=%d mean=%d] value %.7f ref %.7f  dX %.2e' % (n, s, mean, v.item(), vr.item(), rel(Xg.grad, Xr.grad)))
    assert abs(v.item() - vr.item()) < 1e-5
    assert rel(Xg.grad, Xr.grad) < 5 * TOL
    if n > 64:      # what the sharded form lifts: the plain kernel's limit is 64 rows in all
        with pytest.raises(RuntimeError):
            ops.ka(_nhwc(X, dev), _nhwc(Y, dev))


def test_one_shard_is_the_plain_ka_bit_for_bit(dev):
    from cat_amd import ops
    X, Y = detfill.normal((17, 8, 4, 4), 117), detfill.normal((17, 12, 4, 4), 217)
    got = []
    for fn in (ops.ka, lambda a, b: ops.ka_sharded(a, b, 1)):
        Xg = _nhwc(X, dev, True)
        v = fn(Xg, _nhwc(Y, dev))
        torch.autograd.backward([v], [torch.full((), -1.3, device=dev)])
        got.append((v.detach().clone(), Xg.grad.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


# ---------------------------------------------------------------------------------------------------------------- fused block
@pytest.mark.parametrize('n,s', [(4, 2), (5, 2)])
def test_fused_block_keeps_the_fused_path(dev, n, s, monkeypatch):
    """One InvertedResidualChannels with training BatchNorm at S = 2 on a 10 x 18 plane (2 x 2 ragged LDS tiles, threshold lowered as the
    fused-path tests do): fused against the layer-by-layer path -- outputs, running statistics, input gradient, every parameter gradient
    at tests/test_fused_block_gpu.py's bars -- and the fused pipeline really ran.  The stamp is changed to 1 between the fused forward and
    its backward: the backward pass works with the shard count its forward ran with (the saved tables have that shape)."""
    import test_fused_block_gpu as TF
    from cat_amd import fused_block, networks, ops
    c, h, w = 40, 10, 18
    blk = TF._block('batch', dev, c, (7, 0, 9), (16, 5, 0), 'reflect')
    assert networks.set_virtual_replicas(blk, s) == sum(isinstance(m, torch.nn.BatchNorm2d) for m in blk.modules()) >= 7
    ref_blk = copy.deepcopy(blk)
    x = detfill.normal((n, c, h, w), 5) + 0.5 * torch.arange(n, dtype=torch.float32).reshape(n, 1, 1, 1)
    gy = ops.to_nhwc(detfill.normal((n, c, h, w), 6).to(dev))
    calls = []
    real = fused_block.forward

    def counted(b, xx, save=None):
        y = real(b, xx, save)
        calls.append(fused_block.plan_for(b, xx).shards)
        return y
    monkeypatch.setattr(fused_block, 'forward', counted)
    old = ops.set_tconv_min_tiles(1)
    try:
        xf = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
        assert fused_block.applicable(blk, xf)
        yf = blk(xf)
        networks.set_virtual_replicas(blk, 1)
        yf.backward(gy)
        networks.set_virtual_replicas(blk, s)
        assert calls == [s], calls
        fused_block.set_enabled(False)
        try:
            xl = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
            assert not fused_block.applicable(ref_blk, xl)
            yl = ref_blk(xl)
            yl.backward(gy)
        finally:
            fused_block.set_enabled(True)
        torch.cuda.synchronize()
    finally:
        ops.set_tconv_min_tiles(old)
    assert calls == [s], calls
    assert rel(yf, yl) < 2e-5, rel(yf, yl)
    lsd = ref_blk.state_dict()
    for k, v in blk.state_dict().items():
        if 'running_' in k:
            assert rel(v, lsd[k]) < 1e-5, k
        if 'num_batches_tracked' in k:
            assert int(v) == int(lsd[k]) == 1, k
    assert rel(xf.grad, xl.grad) < 2e-4, rel(xf.grad, xl.grad)
    lg = dict(ref_blk.named_parameters())
    top = max(float(q.grad.abs().max()) for q in lg.values())
    bad = {}
    for k, q in blk.named_parameters():
        assert q.grad is not None, k
        err = float((q.grad - lg[k].grad).abs().max()) / max(float(lg[k].grad.abs().max()), 1e-3 * top)
        if err > 5e-4:
            bad[k] = err
    assert not bad, bad
    # ... and the layer-by-layer path it is compared with is not the whole-batch one: S = 1 gives another output
    networks.set_virtual_replicas(ref_blk, 1)
    fused_block.set_enabled(False)
    try:
        with torch.no_grad():
            y1 = ref_blk(ops.to_nhwc(x.to(dev)))
    finally:
        fused_block.set_enabled(True)
    assert rel(y1, yl) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- distillation step
def _distill_opt(meta):
    return H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                      lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16)


def _gpu_half_step(model, A, B):
    """forward -> D backward (gradients kept) -> Adam D -> G backward: the student's gradients are read before Adam consumes them."""
    model.set_input({'A': A, 'B': B, 'A_paths': [], 'B_paths': []})
    model.forward()
    model.set_requires_grad(model.netD, True)
    model.optimizer_D.zero_grad()
    model.backward_D()
    gD = {k: p.grad.detach().cpu().clone() for k, p in model.netD.named_parameters()}
    model.optimizer_D.step()
    model.set_requires_grad(model.netD, False)
    model.optimizer_G.zero_grad()
    model.backward_G(0)
    torch.cuda.synchronize()
    return gD


_STEP = {}


def _distill_case(tag):
    """The configuration of step_<tag>.npz at batch 4: the GPU step at S = 2 (fused kernels on: LDS-tile threshold 1), its distillation
    loss at S = 1, and the oracle's DataParallel restatement over 2 shards -- computed once, shared by the tests below, never changed."""
    if tag in _STEP:
        return _STEP[tag]
    from cat_amd import ops
    g = H.load(f'step_{tag}.npz')
    meta = json.loads(str(g['meta']))
    opt = _distill_opt(meta)
    n, size = 4, meta['size']
    A, B = detfill.images((n, 3, size, size), H.SEED_X + 10), detfill.images((n, 3, size, size), H.SEED_X + 20)
    old = ops.set_tconv_min_tiles(1)
    try:
        out = {}
        for s in (2, 1):
            model = H.build_distiller(opt, g['student_shapes'])
            model.set_virtual_replicas(s)
            gD = _gpu_half_step(model, A, B)
            out[s] = dict(model=model, gD=gD, losses={k.split('/')[-1]: float(v) for k, v in model.get_current_losses().items()})
    finally:
        ops.set_tconv_min_tiles(old)
    ncfg = H.cfg_for(meta['norm'])
    cfg = dict(T=ncfg, S=ncfg, D=ncfg, dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'], lambda_recon=meta['lambda_recon'],
               lambda_distill=meta['lambda_distill'], lambda_gan=1.0, lr=meta['lr'], beta1=meta['beta1'])
    S = detfill.fill_state_dict(H.sd_from_shapes(g['student_shapes']), H.SEED_S)
    st = ref_cpu.DistillState(H.teacher_sd(opt), S, H.disc_sd(opt, 6 if meta['dataset_mode'] == 'aligned' else 3), cfg)
    ref_cpu.distill_step(st, A, B, n_shards=2)
    st64 = None
    if tag == 'in':      # the same oracle step in float64: what the fp32 oracle's own gradients are worth (see the gradient test)
        import test_spade_gpu as TS
        st64 = ref_cpu.DistillState(TS.to64(H.teacher_sd(opt)), TS.to64(S), TS.to64(H.disc_sd(opt, 3)), cfg)
        ref_cpu.distill_step(st64, A.double(), B.double(), n_shards=2)
    _STEP[tag] = (out, st, st64)
    return _STEP[tag]


@pytest.mark.parametrize('tag', ['bn', 'in'])
def test_distill_step_losses_and_image_match_two_shard_oracle(dev, tag):
    out, st, _ = _distill_case(tag)
    got = out[2]['losses']
    for k, ref in st.losses.items():
        print('[virtual replicas %s] %-12s gpu %.6f oracle %.6f (S = 1: %.6f)' % (tag, k, got[k], ref, out[1]['losses'][k]))
    for k, ref in st.losses.items():      # G_distill (and every G_distill<i>) is the SUM over the shards, as the reference logs it
        assert abs(got[k] - ref) <= 1e-3 * max(1.0, abs(ref)), (k, got[k], ref)
    assert rel(out[2]['model'].Sfake_B, st.Sfake_B) < 1e-3
    # the setting is not ignored: the whole-batch term lies further from the two-shard one than the bar
    ref = st.losses['G_distill']
    assert abs(out[1]['losses']['G_distill'] - ref) > 1e-3 * max(1.0, abs(ref)), (out[1]['losses']['G_distill'], ref)


@pytest.mark.parametrize('tag', ['bn', 'in'])
def test_distill_step_gradients_match_two_shard_oracle(dev, tag):
    """Student gradients (read before Adam) and discriminator gradients through test_spade_gpu.check_grads.

    BatchNorm configuration: the plain form, as tests/test_model_gpu.py::test_student_gradients_match_oracle uses it (measured: worst
    err / gmax 9.1e-05, median 1.1e-04).  InstanceNorm configuration at batch 4: the fp32 oracle's OWN student gradients lie further from
    the same step in float64 (median 4.3e-03 of a tensor's scale, worst tensor 4.6e-02) than the plain form's bars (1e-03 / 5e-03), with
    one replica and with two alike -- many of these tensors are zero in exact arithmetic (a shift or scale directly in front of an
    InstanceNorm) and pure round-off on both sides; the GPU's lie at 2.7e-03 / 1.4e-02 of the float64 gradients.  No implementation can meet
    the plain bars against that reference, so this configuration takes check_grads' measured form: every figure against the float64 step,
    with the fp32 oracle's own distance to it as the yardstick.
    What this configuration can and cannot show: KA is about 0.9999 per shard on this fixture, so the distillation term's gradient is about
    zero and the oracle's student gradients for one and for two shards agree to the printed digits -- a wrong sharded-KA backward would not
    move these figures.  That backward is held by test_sharded_ka (float64, kernel level) and, at step level, by the BatchNorm
    configuration, whose KA terms lie at 0.80 - 0.96 per shard and whose two-shard loss differs from the whole-batch one by a factor 2.4."""
    import test_spade_gpu as TS
    out, st, st64 = _distill_case(tag)
    TS.check_grads(out[2]['model'].netG_student.named_parameters(), st.grads_S, None if st64 is None else st64.grads_S,
                   label=f'student gradients, S = 2 ({tag})')

    class _G:      # check_grads reads .grad
        def __init__(self, g):
            self.grad = g
    TS.check_grads([(k, _G(v)) for k, v in out[2]['gD'].items()], st.grads_D, label=f'discriminator gradients, S = 2 ({tag})')


# ---------------------------------------------------------------------------------------------------------------- teacher model
def test_pix2pix_step_equals_the_mean_of_its_halves(dev):
    """pix2pix, --norm batch, batch 4, S = 2: every term is a global mean and every BatchNorm is per shard, so the G and D gradients are
    the mean of the gradients of two S = 1 passes over each half from the same weights."""
    import test_spade_gpu as TS
    from cat_amd.models import create_model
    opt = H.make_opt(norm='batch', track=True, ndf=32, gan_mode='hinge', ngf=16, netG='inception_9blocks', dropout_rate=0, direction='AtoB',
                     model='pix2pix', lambda_recon=100.0, lambda_gan=1.0, recon_loss_type='l1', virtual_replicas=2)
    torch.manual_seed(7)
    m = create_model(opt, verbose=False)
    m.setup(opt, verbose=False)
    assert m.virtual_replicas == 2 and all(b.virtual_replicas == 2 for net in (m.netG, m.netD) for b in net.modules()
                                           if isinstance(b, torch.nn.BatchNorm2d))
    A, B = detfill.images((4, 3, 64, 64), 901), detfill.images((4, 3, 64, 64), 902)

    def grads(s, a, b):
        m.set_virtual_replicas(s)
        m.set_input({'A': a, 'B': b, 'A_paths': [], 'B_paths': []})
        m.forward()
        m.set_requires_grad(m.netD, True)
        m.optimizer_D.zero_grad()
        m.backward_D()
        gD = {k: p.grad.detach().cpu().clone() for k, p in m.netD.named_parameters()}
        m.set_requires_grad(m.netD, False)
        m.optimizer_G.zero_grad()
        m.backward_G()
        torch.cuda.synchronize()
        return {k: p.grad.detach().cpu().clone() for k, p in m.netG.named_parameters()}, gD

    class _G:
        def __init__(self, g):
            self.grad = g
    gG2, gD2 = grads(2, A, B)
    halves = [grads(1, A[:2], B[:2]), grads(1, A[2:], B[2:])]
    whole = grads(1, A, B)
    for i, (got, name) in enumerate(((gG2, 'G'), (gD2, 'D'))):
        want = {k: 0.5 * (halves[0][i][k] + halves[1][i][k]) for k in got}
        TS.check_grads([(k, _G(v)) for k, v in got.items()], want, label=f'pix2pix {name} gradients, S = 2 vs the mean of the halves')
        worst = max(float((whole[i][k] - want[k]).abs().max()) / (float(want[k].abs().max()) + 1e-12) for k in got)
        assert worst > 1e-2, worst      # (whole-batch statistics give other gradients: the comparison can tell)


def test_mse_distillation_is_the_per_shard_mean_summed(dev):
    """--distill_G_loss_type mse at S = 2 (step_mse.npz's configuration, batch 4): the per-device MSE summed over the devices = the
    whole-batch mean times the number of equal shards (a seed factor), against the oracle's n_shards = 2."""
    g = H.load('step_mse.npz')
    meta = json.loads(str(g['meta']))
    opt = H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                     lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16, distill_G_loss_type='mse')
    n, size = 4, meta['size']
    A, B = detfill.images((n, 3, size, size), H.SEED_X + 10), detfill.images((n, 3, size, size), H.SEED_X + 20)
    model = H.build_distiller(opt, g['student_shapes'])
    model.set_virtual_replicas(2)
    _gpu_half_step(model, A, B)
    got = {k.split('/')[-1]: float(v) for k, v in model.get_current_losses().items()}
    ncfg = H.cfg_for(meta['norm'])
    cfg = dict(T=ncfg, S=ncfg, D=ncfg, dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'], lambda_recon=meta['lambda_recon'],
               lambda_distill=meta['lambda_distill'], lambda_gan=1.0, lr=meta['lr'], beta1=meta['beta1'], distill_G_loss_type='mse')
    S = detfill.fill_state_dict(H.sd_from_shapes(g['student_shapes']), H.SEED_S)
    st = ref_cpu.DistillState(H.teacher_sd(opt), S, H.disc_sd(opt, 6 if meta['dataset_mode'] == 'aligned' else 3), cfg, H.netA_sds(S))
    ref = ref_cpu.distill_step(st, A, B, n_shards=2)
    for k, v in ref.items():
        print('[virtual replicas mse] %-12s gpu %.6f oracle %.6f' % (k, got[k], v))
        assert abs(got[k] - v) <= 1e-3 * max(1.0, abs(v)), (k, got[k], v)
    import test_spade_gpu as TS
    gA = {'%d.%s' % (i, k): p for i, a in enumerate(model.netAs) for k, p in a.named_parameters()}
    refA = {k: v.grad for k, v in st.A.items() if v.grad is not None}
    TS.check_grads(list(gA.items()), refA, label='adaptor gradients, mse, S = 2')


# ---------------------------------------------------------------------------------------------------------------- SPADE distiller
def test_spade_distiller_matches_two_shard_oracle(dev):
    """SPADEDistiller at the shapes of tests/test_dp_gpu.py::_worker_spade, S = 2, in one process: SynchronizedBatchNorm statistics over
    the whole batch with the reference's multi-replica formula (ops.ReplicaSync), the distillation terms the MEAN over the shards' KA --
    losses at that test's bars and student gradients against spade_step(n_shards=2)."""
    import test_dp_gpu as TD
    import test_spade_gpu as TS
    from cat_amd import ops
    from oracle import ref_spade_cpu as R
    g, opt, lab, ins, img, sds, cfg = TS.fixture()
    opt.isTrain, opt.distiller, opt.log_dir = True, 'spade', '/tmp/cat_amd_logs'
    model = TS.build_spade_distiller(opt, sds)
    batch = TD.spade_batch(opt, int(g['h']), int(g['w']))
    try:
        model.set_virtual_replicas(2)
        assert isinstance(ops.bn_sync(), ops.ReplicaSync)
        model.set_input(batch)
        model.optimize_parameters(0)
        torch.cuda.synchronize()
    finally:
        model.set_virtual_replicas(1)
    assert ops.bn_sync() is None
    got = {k.split('/')[-1]: float(v) for k, v in model.get_current_losses().items()}
    sem = R.preprocess_input(batch['label'], batch['instance'], opt.input_nc)
    st = R.SpadeState(sds['T'], sds['S'], sds['D'], sds['V'], cfg)
    ref = R.spade_step(st, sem, batch['image'], n_shards=2)
    for k in ('G_gan', 'G_feat', 'G_vgg', 'G_distill', 'D_real', 'D_fake'):
        print('[virtual replicas spade] %-10s gpu %.6f oracle %.6f' % (k, got[k], ref[k]))
    for k in ('G_gan', 'G_feat', 'G_vgg', 'G_distill', 'D_real', 'D_fake'):
        assert abs(got[k] - ref[k]) <= 5e-3 * max(abs(ref[k]), 1e-2), (k, got[k], ref[k])
    TS.check_grads(model.modules_on_one_gpu.netG_student.named_parameters(), st.grads_S, label='SPADE student gradients, S = 2')


# ---------------------------------------------------------------------------------------------------------------- graph + launches
def test_graph_replay_equals_eager_with_virtual_replicas(dev):
    """GraphedStep at S = 2 captures and replays: two replays against two eager steps from equal weights, weights bit-identical."""
    from cat_amd import ops
    from cat_amd.graph import GraphedStep
    g = H.load('step_bn.npz')
    meta = json.loads(str(g['meta']))
    n, s = 4, meta['size']
    batches = [{'A': detfill.images((n, 3, s, s), 500 + i).cuda(), 'B': detfill.images((n, 3, s, s), 600 + i).cuda(), 'A_paths': [], 'B_paths': []}
               for i in range(3)]
    old = ops.set_tconv_min_tiles(1)
    try:
        eager, graphed = (H.build_distiller(_distill_opt(meta), g['student_shapes']) for _ in range(2))
        for m in (eager, graphed):
            m.set_virtual_replicas(2)
        for i in range(3):
            eager.set_input(batches[0])
            eager.optimize_parameters(i)
        step = GraphedStep(graphed, batches[0], warmup=3)
        for i in (1, 2):
            eager.set_input(batches[i])
            eager.optimize_parameters(3 + i)
            step(batches[i])
        torch.cuda.synchronize()
    finally:
        ops.set_tconv_min_tiles(old)
    le, lg = eager.get_current_losses(), graphed.get_current_losses()
    for k in le:
        assert le[k] == lg[k], (k, le[k], lg[k])
    for a, b in ((eager.netG_student, graphed.netG_student), (eager.netD, graphed.netD)):
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka


def _calls_per_step(model, batch, nprof=2):
    """library calls of one optimize_parameters, counted as tools/spade_teacher_bench.py counts them (the library's profiling hook)"""
    import ctypes as C
    from cat_amd import _lib
    lib = _lib.load()
    lib.cat_prof_enable(1)
    for i in range(nprof):
        model.set_input(batch)
        model.optimize_parameters(i)
    torch.cuda.synchronize()
    nfam = lib.cat_prof_collect()
    lib.cat_prof_enable(0)
    fams, name = {}, C.create_string_buffer(64)
    cnt, tms, fl = C.c_int64(), C.c_double(), C.c_double()
    for i in range(nfam):
        lib.cat_prof_family(i, name, 64, C.byref(cnt), C.byref(tms), C.byref(fl))
        fams[name.value.decode()] = cnt.value / nprof
    return fams


def test_launch_count_does_not_grow_with_replicas(dev, monkeypatch):
    """Library calls per step on the fused path at S = 1, 2, 4 (batch 4): S > 1 costs a constant (the paths that decline run layer by layer),
    and nothing depends on S itself -- S = 2 and S = 4 make the same calls.  The counted steps take the fused block at every S: the same
    number of fused-block forwards as at S = 1, each with the step's shard count."""
    from cat_amd import fused_block, ops
    g = H.load('step_bn.npz')
    meta = json.loads(str(g['meta']))
    n, size = 4, meta['size']
    batch = {'A': detfill.images((n, 3, size, size), 1).cuda(), 'B': detfill.images((n, 3, size, size), 2).cuda(), 'A_paths': [], 'B_paths': []}
    old = ops.set_tconv_min_tiles(1)
    try:
        model = H.build_distiller(_distill_opt(meta), g['student_shapes'])
        model.set_input(batch)
        model.optimize_parameters(0)      # (first-use preparation is not part of a step)
        fams, fused = {}, {}
        real = fused_block.forward

        def counted(b, xx, save=None):
            y = real(b, xx, save)
            fused[s].append(fused_block.plan_for(b, xx).shards)
            return y
        monkeypatch.setattr(fused_block, 'forward', counted)
        for s in (1, 2, 4):
            fused[s] = []
            model.set_virtual_replicas(s)
            fams[s] = _calls_per_step(model, batch)
    finally:
        ops.set_tconv_min_tiles(old)
    nblocks = len(model.netG_student.features)
    for s in (1, 2, 4):      # 2 counted steps x (student forward with grad + the blocks are not re-run in the D step)
        assert len(fused[s]) == len(fused[1]) >= 2 * nblocks and set(fused[s]) == {s}, (s, len(fused[s]), set(fused[s]))
    total = {s: sum(f.values()) for s, f in fams.items()}
    print('\n[virtual replicas] library calls per step: S=1 %.1f, S=2 %.1f, S=4 %.1f' % (total[1], total[2], total[4]))
    print('  families that differ between S=1 and S=4:', {k: (fams[1].get(k, 0), fams[4].get(k, 0)) for k in set(fams[1]) | set(fams[4])
                                                             if fams[1].get(k, 0) != fams[4].get(k, 0)})
    assert fams[2] == fams[4], {k: (fams[2].get(k, 0), fams[4].get(k, 0)) for k in set(fams[2]) | set(fams[4]) if fams[2].get(k, 0) != fams[4].get(k, 0)}
    assert total[1] > 50
