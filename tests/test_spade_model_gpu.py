"""GPU: the GauGAN teacher step (`create_model` with --model spade: cat_amd/models/spade_model.py + cat_amd/spade_model_modules.py) against
tests/golden/spade_model_step.npz, recorded from the reference's own SPADEModelModules by tools/make_golden_spade_model.py: two full
optimize_parameters steps at the SPADE fixture's geometry (n 2, 128 x 256, ngf 8, ndf 8, num_D 2, n_layers_D 4, hinge, TTUR, VGG / 8).

Bars: step-1 losses 2e-3 * max(|ref|, 1e-2); fake_B 1e-3 relative; check_step_grads at 1e-2 (G) and 3e-2 (D), the calibrated bars
of test_spade_distill_step (whole-step gradients pass through the piecewise-linear discriminator, see test_oracle_spade_golden.test_spade_step);
spectral-norm u and running statistics 1e-3 after step 1 -- the TWICE-advanced value: compute_D_loss regenerates fake_B in train mode -- and
2e-3 after step 2; step-2 losses 5e-3 * max(|ref|, 1e-2), except where float32 itself does not carry that: see test_second_step_carries_the_state.

Run as a script (`python tests/test_spade_model_gpu.py OUT.npz`) it performs step 1 and dumps the losses and the generator gradient probes:
the CAT_LOSS_MULTI=0 case starts it in a fresh child process, because the switch is read once at import."""
import json
import os
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import helpers as H  # noqa: E402
from oracle import detfill  # noqa: E402

pytestmark = pytest.mark.gpu
LOSSES = ('G_gan', 'G_feat', 'G_vgg', 'D_fake', 'D_real')
RM_KEY, RV_KEY, U_KEY = 'head_0.spade.param_free_norm.running_mean', 'G_middle_0.spade.param_free_norm.running_var', 'discriminator_1.model2.0.0.weight_u'


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def fixture(log_dir='/tmp/cat_amd_logs', **kw):
    import test_oracle_spade_golden as TG
    g = H.load('spade_model_step.npz')
    o = json.loads(str(g['opt']))
    o.update(gpu_ids=[0], vgg_width_div=8, model='spade', isTrain=True, no_fid=True, no_mIoU=True, log_dir=log_dir, restore_G_path=None,
             restore_D_path=None, restore_O_path=None)
    o.update(kw)
    sds = dict(G=detfill.fill_state_dict(H.sd_from_shapes(g['G_shapes']), int(g['seed_G'])),
               D=detfill.fill_state_dict(H.sd_from_shapes(g['D_shapes']), int(g['seed_D'])),
               V=detfill.fill_state_dict(TG.spade_vgg_feature_shapes(g), int(g['seed_V'])))
    data = {'label': torch.from_numpy(g['label'].astype(np.int64)).float(), 'instance': torch.from_numpy(g['instance']),
            'image': detfill.images((int(g['n']), 3, int(g['h']), int(g['w'])), int(g['image_seed'])), 'path': []}
    return g, Namespace(**o), sds, data


def build(opt, sds):
    from cat_amd.models import create_model
    model = create_model(opt, verbose=False)
    m = model.modules_on_one_gpu
    m.netG.load_state_dict(sds['G'])
    if opt.isTrain:
        m.netD.load_state_dict(sds['D'])
        m.criterionVGG.vgg.load_torchvision_state_dict(sds['V'])
        m.train()
    return model


def current_losses(model):
    return {k.split('/')[-1]: v for k, v in model.get_current_losses().items()}


_RUN = {}


def two_steps():
    """Both optimize_parameters steps, once for the whole module; everything the tests read is copied out as it stood after each step."""
    if _RUN:
        return _RUN
    from cat_amd import ops
    g, opt, sds, data = fixture()
    model = build(opt, sds)
    m = model.modules_on_one_gpu
    ops.STATS['conform_copies'] = 0
    model.set_input(data)
    model.optimize_parameters(0)
    r = _RUN
    r['losses1'] = current_losses(model)
    r['fake_B'] = model.fake_B.detach().cpu()
    r['gG'] = {k: p.grad.detach().clone() for k, p in m.netG.named_parameters()}
    r['gD'] = {k: p.grad.detach().clone() for k, p in m.netD.named_parameters()}
    r['sdG1'] = {k: v.detach().cpu().clone() for k, v in m.netG.state_dict().items()}
    r['sdD1'] = {k: v.detach().cpu().clone() for k, v in m.netD.state_dict().items()}
    r['conform_copies'] = ops.STATS['conform_copies']
    model.optimize_parameters(1)
    r['losses2'] = current_losses(model)
    r['sdG2'] = {k: v.detach().cpu().clone() for k, v in m.netG.state_dict().items()}
    r['sdD2'] = {k: v.detach().cpu().clone() for k, v in m.netD.state_dict().items()}
    r['g'], r['sds'] = g, sds
    return r


def test_first_step_matches_the_reference():
    import test_oracle_spade_golden as TG
    r = two_steps()
    g = r['g']
    ref = json.loads(str(g['losses1']))
    for k in LOSSES:
        print('step 1 %s: %.7g (reference %.7g)' % (k, r['losses1'][k], ref[k]))
    for k in LOSSES:
        assert abs(r['losses1'][k] - ref[k]) <= 2e-3 * max(abs(ref[k]), 1e-2), (k, r['losses1'][k], ref[k])
    err = rel(r['fake_B'][:, :6, ::4, ::4], g['fake_B_sub'])
    print('fake_B relative error %.3g' % err)
    assert err < 1e-3
    TG.check_step_grads(g, 'G', r['gG'], r['sdG1'], int(g['seed_G']), 1e-2)
    TG.check_step_grads(g, 'D', r['gD'], r['sdD1'], int(g['seed_D']), 3e-2)
    errs = dict(u=rel(r['sdD1'][U_KEY], g['D_u_step1']), rm=rel(r['sdG1'][RM_KEY], g['G_rm_step1']), rv=rel(r['sdG1'][RV_KEY], g['G_rv_step1']))
    print('after step 1: weight_u %.3g, running_mean %.3g, running_var %.3g (a single advance would be %.3g / %.3g away)' % (
        errs['u'], errs['rm'], errs['rv'], rel(g['G_rm_single'], g['G_rm_step1']), rel(g['G_rv_single'], g['G_rv_step1'])))
    assert max(errs.values()) < 1e-3, errs
    nbt = [k for k in r['sdG1'] if k.endswith('num_batches_tracked')]
    assert nbt and all(torch.equal(r['sdG1'][k], r['sds']['G'][k]) for k in nbt)
    assert r['conform_copies'] == 0


def test_second_step_carries_the_state():
    """Adam moments, spectral-norm u vectors and running statistics carried into step 2.

    The general margin 5e-3 * max(|ref|, 1e-2) is 5e-5 for G_gan (reference -0.0051656), and the REFERENCE does not hold it against itself: in
    the golden tool its float32 step on 8 threads and on 1 thread give G_gan -0.0051656 and -0.0052339 (6.8e-5 apart), and both are up to 7.0e-5
    from its float64 step (after Adam's first +-lr step, whose sign on noise-level gradients is arbitrary, the hinge-G term is a small difference
    of O(1) discriminator outputs).  Where a margin is tighter than the reference's own float32 carries, the bar of a loss is twice the reference's
    float32-vs-float64 distance recorded in the fixture (`losses2_f32_vs_f64`): 1.4e-4 for G_gan.  For the other four losses and for the running
    statistics twice that distance (G_feat 4.2e-3, G_vgg 2.7e-6, D_fake 6.2e-4, D_real 1.3e-4; statistics 1.8e-4 / 1.7e-3) is below the general
    margin, which stays.  Nothing here was calibrated on the code under test."""
    r = two_steps()
    g = r['g']
    ref = json.loads(str(g['losses2']))
    for k in LOSSES:
        print('step 2 %s: %.7g (reference %.7g)' % (k, r['losses2'][k], ref[k]))
    errs = dict(rm=rel(r['sdG2'][RM_KEY], g['G_rm_step2']), rv=rel(r['sdG2'][RV_KEY], g['G_rv_step2']))
    print('after step 2: running_mean %.3g, running_var %.3g' % (errs['rm'], errs['rv']))
    dist = json.loads(str(g['losses2_f32_vs_f64']))
    for k in LOSSES:
        bar = max(5e-3 * max(abs(ref[k]), 1e-2), 2 * dist[k])
        assert abs(r['losses2'][k] - ref[k]) <= bar, (k, r['losses2'][k], ref[k], bar)
    assert 2 * float(g['stats2_f32_vs_f64'].max()) < 2e-3
    assert max(errs.values()) < 2e-3, errs
    assert all(torch.equal(r['sdG2'][k], r['sds']['G'][k]) for k in r['sdG2'] if k.endswith('num_batches_tracked'))


def first_step_probes():
    """step 1 on a fresh model: the five losses and the generator gradient probes (what the child process dumps)."""
    g, opt, sds, data = fixture()
    model = build(opt, sds)
    model.set_input(data)
    model.optimize_parameters(0)
    out = {'loss/' + k: np.float64(v) for k, v in current_losses(model).items()}
    grads = dict(model.modules_on_one_gpu.netG.named_parameters())
    for k in json.loads(str(g['probe_G'])):
        out['grad/' + k] = grads[k].grad.detach().cpu().numpy().reshape(-1)[:256]
    return out


def test_per_term_loss_path_gives_the_same_step(tmp_path):
    """CAT_LOSS_MULTI=0 (one LossFn per term) in a fresh child process against the default MultiLossFn path in this one."""
    from cat_amd import spade_model_modules
    assert spade_model_modules.loss_multi_enabled()
    r = two_steps()
    g = r['g']
    out = str(tmp_path / 'per_term.npz')
    env = dict(os.environ, CAT_LOSS_MULTI='0')
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert 'loss_multi False' in p.stdout
    c = np.load(out)
    gmax = float(g['G_gmax'])
    for k in LOSSES:
        a, b = float(c['loss/' + k]), r['losses1'][k]
        print('%s: per-term %.9g, multi %.9g' % (k, a, b))
        assert abs(a - b) <= 1e-6 * abs(b), (k, a, b)
    for k in json.loads(str(g['probe_G'])):
        d = float(np.abs(c['grad/' + k] - r['gG'][k].cpu().numpy().reshape(-1)[:256]).max())
        assert d <= 1e-6 * gmax, (k, d, gmax)


def test_test_mode_builds_the_generator_only():
    from cat_amd import prune
    g, opt, sds, data = fixture()
    trained = build(opt, sds)
    trained.set_input(data)
    trained.modules_on_one_gpu.netG.eval()
    with torch.no_grad():
        want = trained.modules_on_one_gpu(trained.input_semantics, mode='generate_fake')
    g, topt, sds, data = fixture(isTrain=False)
    model = build(topt, sds)
    m = model.modules_on_one_gpu
    assert not hasattr(m, 'netD') and not hasattr(m, 'criterionVGG') and not m.netG.training and model.model_names == ['G']
    model.set_input(data)
    model.test()
    assert torch.equal(model.fake_B.cpu(), want.cpu())
    n, c, h, w = model.input_semantics.shape
    assert model.profile(verbose=False) == prune.model_profiling(trained.modules_on_one_gpu.netG, h, w, 1, c)
    assert model.profile(verbose=False)[0] > 0


def test_checkpoints_round_trip(tmp_path):
    g, opt, sds, data = fixture(log_dir=str(tmp_path))
    model = build(opt, sds)
    model.set_input(data)
    model.optimize_parameters(0)             # weights, u vectors and running statistics that differ from the initial fill
    model.save_networks('latest')
    ckpt = tmp_path / 'checkpoints'
    assert sorted(os.listdir(ckpt)) == ['latest_net_D.pth', 'latest_net_G.pth', 'latest_optim-0.pth', 'latest_optim-1.pth']
    g, opt2, sds, data = fixture(log_dir=str(tmp_path), restore_G_path=str(ckpt / 'latest_net_G.pth'), restore_D_path=str(ckpt / 'latest_net_D.pth'))
    fresh = build(opt2, sds)
    fresh.load_networks(verbose=False)
    for name, tag in (('netG', 'G'), ('netD', 'D')):
        a, b = getattr(model.modules_on_one_gpu, name).state_dict(), getattr(fresh.modules_on_one_gpu, name).state_dict()
        saved = torch.load(str(ckpt / ('latest_net_%s.pth' % tag)), map_location='cpu')
        assert sorted(saved) == sorted(k for k, _ in json.loads(str(g[tag + '_shapes'])))      # the reference's state_dict keys
        assert sorted(a) == sorted(b) == sorted(saved)
        for k in a:
            assert torch.equal(a[k].cpu(), b[k].cpu()), k
        assert any(not torch.equal(a[k].cpu(), sds[tag][k]) for k in a)


def test_evaluate_model_without_metrics(tmp_path):
    g, opt, sds, data = fixture(log_dir=str(tmp_path))
    model = build(opt, sds)
    batches = []
    for i in range(2):
        batches.append(dict(data, path=['/data/val/b%d_%d.png' % (i, j) for j in range(int(g['n']))]))
    model.eval_dataloader = batches
    ret = model.evaluate_model(7)
    assert ret == {}
    assert model.modules_on_one_gpu.netG.training and not model.is_best
    root = tmp_path / 'eval' / '7'
    assert sorted(os.listdir(root)) == ['fake', 'input', 'real']
    for kind in ('fake', 'input', 'real'):
        names = sorted(os.listdir(root / kind))
        assert names == sorted('b%d_%d.png' % (i, j) for i in range(2) for j in range(int(g['n']))) and len(names) <= 10


if __name__ == '__main__':
    from cat_amd import spade_model_modules
    print('loss_multi', spade_model_modules.loss_multi_enabled())
    np.savez(sys.argv[1], **first_step_probes())
