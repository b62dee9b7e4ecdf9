"""GPU: whole steps with the reference's default kernel sizes [3, 5, 7] on the fused block path (fused_block.set_k7(True)): one
InceptionDistiller step against the CPU oracle (oracle/ref_cpu.distill_step) with the helpers and the check_grads bars of
tests/test_virtual_replicas_gpu.py, hipGraph replays against eager steps bit for bit, and the inference runner on an InstanceNorm 3 5 7
student at the bar tests/test_pretrained_gpu.py holds the runner to.  The student is the unpruned ngf-16 InceptionGenerator (trunk 64,
branches 10 wide), the teacher the canonical ngf-64 one with the same kernel sizes; its frozen blocks keep the layer-by-layer path."""
import contextlib
import json

import pytest
import torch

import helpers as H
from oracle import detfill, ref_cpu

pytestmark = pytest.mark.gpu
KS = [3, 5, 7]
N, SIZE = 2, 32
BAR = 1e-3      # tests/test_pretrained_gpu.py


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


def _meta(tag):
    return json.loads(str(H.load(f'step_{tag}.npz')['meta']))


def _opt(meta):
    return H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                      lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16, kernel_sizes=list(KS))


def _student_shapes(opt):
    """the recorded-shapes form H.build_distiller takes, for the unpruned ngf-16 student of `opt`"""
    from cat_amd import networks
    net = networks.define_G(3, 3, 16, 'inception_9blocks', opt.norm, 0, 'normal', 0.02, [], opt=opt)
    assert [b.res_kernel_sizes for b in net.features] == [KS] * 9
    return json.dumps([[k, list(v.shape)] for k, v in net.state_dict().items()])


_STEP = {}


def _distill_case(tag):
    """one GPU step (student and discriminator gradients read before Adam) and the oracle's step on the same weights and images, once"""
    if tag in _STEP:
        return _STEP[tag]
    import test_spade_gpu as TS
    from test_virtual_replicas_gpu import _gpu_half_step
    from cat_amd import fused_block
    meta = _meta(tag)
    opt = _opt(meta)
    shapes = _student_shapes(opt)
    A, B = detfill.images((N, 3, SIZE, SIZE), H.SEED_X + 10), detfill.images((N, 3, SIZE, SIZE), H.SEED_X + 20)
    fused, real = [], fused_block.forward

    def counted(b, xx, save=None):
        fused.append(fused_block.plan_for(b, xx).fs)
        return real(b, xx, save)
    with k7_small_planes():
        fused_block.forward = counted
        try:
            model = H.build_distiller(opt, shapes)
            gD = _gpu_half_step(model, A, B)
        finally:
            fused_block.forward = real
    losses = {k.split('/')[-1]: float(v) for k, v in model.get_current_losses().items()}
    ncfg = H.cfg_for(meta['norm'])
    d_in = 6 if meta['dataset_mode'] == 'aligned' else 3
    cfg = dict(T=ncfg, S=ncfg, D=ncfg, dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'], lambda_recon=meta['lambda_recon'],
               lambda_distill=meta['lambda_distill'], lambda_gan=1.0, lr=meta['lr'], beta1=meta['beta1'])
    S = detfill.fill_state_dict(H.sd_from_shapes(shapes), H.SEED_S)
    st = ref_cpu.DistillState(H.teacher_sd(opt), S, H.disc_sd(opt, d_in), cfg)
    ref_cpu.distill_step(st, A, B)
    st64 = None
    if tag == 'in':      # the same oracle step in float64: what the fp32 oracle's own gradients are worth (check_grads' measured form)
        st64 = ref_cpu.DistillState(TS.to64(H.teacher_sd(opt)), TS.to64(S), TS.to64(H.disc_sd(opt, d_in)), cfg)
        ref_cpu.distill_step(st64, A.double(), B.double())
    _STEP[tag] = (model, gD, losses, st, st64, fused)
    return _STEP[tag]


@pytest.mark.parametrize('tag', ['bn', 'in'])
def test_k7_distill_step_matches_the_oracle(tag):
    import test_spade_gpu as TS
    model, gD, losses, st, st64, fused = _distill_case(tag)
    assert fused == [7] * 9, fused      # the nine student blocks took the fused path once each, on the 7 x 7 frame
    for k, ref in st.losses.items():
        print('[k7 step %s] %-12s gpu %.6f oracle %.6f' % (tag, k, losses[k], ref))
    for k, ref in st.losses.items():
        assert abs(losses[k] - ref) <= 1e-3 * max(1.0, abs(ref)), (k, losses[k], ref)
    d = float((model.Sfake_B.detach().cpu().double() - st.Sfake_B.double()).abs().max() / st.Sfake_B.double().abs().max())
    print('[k7 step %s] Sfake_B rel %.3g' % (tag, d))
    assert d < 1e-3
    TS.check_grads(model.netG_student.named_parameters(), st.grads_S, None if st64 is None else st64.grads_S, label=f'k7 student gradients ({tag})')

    class _G:      # check_grads reads .grad
        def __init__(self, g):
            self.grad = g
    TS.check_grads([(k, _G(v)) for k, v in gD.items()], st.grads_D, label=f'k7 discriminator gradients ({tag})')


def test_k7_graph_replays_equal_eager_steps():
    """two GraphedStep replays against two eager steps from equal weights: losses and weights bit-identical"""
    from cat_amd.graph import GraphedStep
    meta = _meta('bn')
    opt = _opt(meta)
    shapes = _student_shapes(opt)
    batches = [{'A': detfill.images((N, 3, SIZE, SIZE), 500 + i).cuda(), 'B': detfill.images((N, 3, SIZE, SIZE), 600 + i).cuda(), 'A_paths': [],
                'B_paths': []} for i in range(3)]
    with k7_small_planes():
        eager, graphed = (H.build_distiller(_opt(meta), shapes) for _ in range(2))
        for i in range(3):
            eager.set_input(batches[0])
            eager.optimize_parameters(i)
        step = GraphedStep(graphed, batches[0], warmup=3)
        for i in (1, 2):
            eager.set_input(batches[i])
            eager.optimize_parameters(3 + i)
            step(batches[i])
        torch.cuda.synchronize()
    le, lg = eager.get_current_losses(), graphed.get_current_losses()
    for k in le:
        assert le[k] == lg[k], (k, le[k], lg[k])
    for a, b in ((eager.netG_student, graphed.netG_student), (eager.netD, graphed.netD)):
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka


def test_k7_student_runner_matches_the_general_eval_forward():
    from test_fused_block_k7_gpu import _Log
    from cat_amd import networks, ops
    from cat_amd.infer import StudentRunner
    dev = torch.device('cuda:0')
    opt = _opt(_meta('in'))
    S = networks.define_G(3, 3, 16, 'inception_9blocks', opt.norm, 0, 'normal', 0.02, [], opt=opt)
    S.load_state_dict(detfill.fill_state_dict(S.state_dict(), H.SEED_S))
    S = S.to(dev).eval()
    x = detfill.images((2, 3, 64, 64), H.SEED_X)
    with torch.no_grad():
        y_general = S(ops.to_nhwc(x.to(dev)))
    with k7_small_planes():
        runner = StudentRunner(S, x)
        try:
            runner(x)
            with _Log() as log:
                y_runner = runner(x)
            torch.cuda.synchronize()
        finally:
            runner.release()
    assert log.names.count('cat_dwm7_fwd') == 9, log.names
    assert not any(nm.startswith('cat_dwconv2d_') for nm in log.names)
    d = H.rel_err(y_runner.cpu().numpy(), y_general.cpu().numpy())
    print('[k7 runner] runner vs general eval forward %.3e' % d)
    assert d < BAR
