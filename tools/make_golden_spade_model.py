"""Generate tests/golden/spade_model_step.npz by RUNNING THE REFERENCE's GauGAN teacher step (`--model spade`: SPADEModelModules of
snap-research/CAT imported on the CPU, gpu_ids=[]).  Build container only:  python tools/make_golden_spade_model.py [--check]

Sibling of tools/make_golden_spade.py, whose options, synthetic inputs, sub-sampling, checksums and narrow-VGG stub it imports: same geometry
(n = 2, 128 x 256, input_nc 5 + edges, ngf 8, ndf 8, num_D 2, n_layers_D 4, spadesyncbatch3x3 / spectralinstance, hinge, lambda 1 / 10 / 10,
TTUR, VGG width / 8), weights from oracle/detfill with fixed seeds.  Adam is constructed with betas (0.0, 0.9) by hand because torch 2.10
rejects the int 0 the reference passes (spade_model_modules.py:57-64).  Two full optimize_parameters steps in the reference's order
(models/spade_model.py:189-215) are recorded: the five losses of each, fake_B of step 1, gradient / norm / updated-value probes of netG and
netD for step 1, one spectral-norm u vector and two SynchronizedBatchNorm running statistics after each step.

compute_D_loss regenerates fake_B with the generator in train mode, so the running statistics advance TWICE per step; the value a single
advance gives (taken right after the G-step forward) is recorded too and asserted here to differ from the recorded one by far more than the
test's 1e-3 bar.  Step 2 is also run a second time in float32 (one thread) and once in float64: the distances between those runs of the
reference are recorded, and tests/test_spade_model_gpu.py holds its step-2 bars against them.  No reference source is stored, only seeds, shapes and outputs.  --check regenerates and compares with the committed file."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_spade as MG  # noqa: E402  (installs the reference import path and the narrow-VGG stub)
from make_golden_spade import checks, shapes_json, spade_opt, sub, synth_inputs  # noqa: E402

import torch  # noqa: E402

from oracle import detfill  # noqa: E402
from models.modules.spade_modules.spade_model_modules import SPADEModelModules  # noqa: E402  (reference)
from models.spade_model import SPADEModel  # noqa: E402

SEED_G, SEED_D, SEED_X = 211, 241, 231
RM_KEY, RV_KEY, U_KEY = 'head_0.spade.param_free_norm.running_mean', 'G_middle_0.spade.param_free_norm.running_var', 'discriminator_1.model2.0.0.weight_u'
PROBE_G = ['fc.weight', 'fc_norm.weight', 'head_0.spade.res_ops.1.0.conv.weight', 'head_0.spade.dw_ops.2.2.bias',
           'G_middle_1.res_ops.2.1.conv.weight', 'up_1.dw_ops.1.1.conv.weight', 'up_1.shortcut.0.weight', 'up_1.shortcut.1.conv.weight',
           'up_3.spade.dw_ops.0.1.norm.bias', 'conv_img.weight', 'conv_img.bias']
PROBE_D = ['discriminator_0.model0.0.weight', 'discriminator_0.model2.0.0.weight_orig', 'discriminator_0.model4.0.bias',
           'discriminator_1.model1.0.0.weight_orig', 'discriminator_1.model3.0.0.weight_orig', 'discriminator_1.model4.0.weight']
LOSSES = ('G_gan', 'G_feat', 'G_vgg', 'D_fake', 'D_real')


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def generate(dtype=torch.float32, threads=8):
    torch.set_num_threads(threads)
    opt = spade_opt(ngf=8, netG='inception_spade', dropout_rate=0, restore_G_path=None)
    h, w, n = int(opt.crop_size / opt.aspect_ratio), opt.crop_size, 2
    lab, ins, img = synth_inputs(n, h, w, opt.input_nc, SEED_X)
    out = dict(label=lab.astype(np.int16), instance=ins, image_seed=SEED_X + 1, h=h, w=w, n=n, seed_G=SEED_G, seed_D=SEED_D, seed_V=MG.SEED_V,
               opt=json.dumps({k: v for k, v in vars(opt).items() if isinstance(v, (int, float, str, bool, list, type(None)))}))
    sm = SPADEModel.__new__(SPADEModel)
    sm.opt, sm.device = opt, torch.device('cpu')
    sem, real_B = sm.preprocess_input({'label': torch.from_numpy(lab).float(), 'instance': torch.from_numpy(ins), 'image': img})
    sem, real_B = sem.to(dtype), real_B.to(dtype)

    m = SPADEModelModules(opt).to(dtype)
    m.netG.load_state_dict(detfill.fill_state_dict(m.netG.state_dict(), SEED_G))
    m.netD.load_state_dict(detfill.fill_state_dict(m.netD.state_dict(), SEED_D))
    out['G_shapes'], out['D_shapes'] = shapes_json(m.netG.state_dict()), shapes_json(m.netD.state_dict())
    out['V_shapes'] = shapes_json(m.criterionVGG.vgg.state_dict())
    out['V_keymap'] = json.dumps({k: k.split('.', 1)[1] for k in m.criterionVGG.vgg.state_dict()})
    nbt0 = {k: int(v) for k, v in m.netG.state_dict().items() if k.endswith('num_batches_tracked')}

    seen = []      # every generator forward: (output, the two running statistics right after it)
    m.netG.register_forward_hook(lambda mod, i, o: seen.append((o.detach().clone(), mod.state_dict()[RM_KEY].clone(), mod.state_dict()[RV_KEY].clone())))
    opt_G = torch.optim.Adam(list(m.netG.parameters()), lr=opt.lr / 2, betas=(0.0, 0.9))
    opt_D = torch.optim.Adam(list(m.netD.parameters()), lr=opt.lr * 2, betas=(0.0, 0.9))
    m.train()
    for step in (1, 2):
        # models/spade_model.py:207-215
        for p in m.netD.parameters():
            p.requires_grad_(False)
        opt_G.zero_grad()
        losses = m(sem, real_B, mode='G_loss')
        losses['loss_G'].mean().backward()
        got = {k: float(v.detach().mean()) for k, v in losses.items()}
        gG = {k: v.grad.clone() for k, v in m.netG.named_parameters() if v.grad is not None}
        opt_G.step()
        for p in m.netD.parameters():
            p.requires_grad_(True)
        opt_D.zero_grad()
        losses = m(sem, real_B, mode='D_loss')
        losses['loss_D'].mean().backward()
        got.update({k: float(v.detach().mean()) for k, v in losses.items()})
        gD = {k: v.grad.clone() for k, v in m.netD.named_parameters() if v.grad is not None}
        opt_D.step()
        sdG, sdD = m.netG.state_dict(), m.netD.state_dict()
        out['losses%d' % step] = json.dumps({k: got[k] for k in LOSSES})
        out['G_rm_step%d' % step], out['G_rv_step%d' % step] = sdG[RM_KEY].float().numpy().copy(), sdG[RV_KEY].float().numpy().copy()
        out['D_u_step%d' % step] = sdD[U_KEY].float().numpy().copy()
        if step == 1 and dtype == torch.float32:
            assert len(seen) == 2      # the G-step forward and compute_D_loss's regeneration
            out['fake_B_sub'], out['fake_B_checks'] = sub(seen[0][0]), checks(seen[0][0])
            out['G_rm_single'], out['G_rv_single'] = seen[0][1].numpy().copy(), seen[0][2].numpy().copy()
            out['G_gmax'] = np.float64(max(float(v.abs().max()) for v in gG.values()))
            out['D_gmax'] = np.float64(max(float(v.abs().max()) for v in gD.values()))
            out['probe_G'], out['probe_D'] = json.dumps(PROBE_G), json.dumps(PROBE_D)
            for tag, probe, sd, grads in (('G', PROBE_G, sdG, gG), ('D', PROBE_D, sdD, gD)):
                for k in probe:
                    out['%s_after/%s' % (tag, k)] = sd[k].numpy().reshape(-1)[:256].copy()
                    out['%s_grad/%s' % (tag, k)] = grads[k].numpy().reshape(-1)[:256].copy()
                    out['%s_gnorm/%s' % (tag, k)] = np.float64(grads[k].double().norm().item())
    assert len(seen) == 4
    if dtype != torch.float32:
        return out
    assert {k: int(v) for k, v in m.netG.state_dict().items() if k.endswith('num_batches_tracked')} == nbt0      # one rank: F.batch_norm, not advanced
    # the second-forward quirk is pinned: a single advance is far from the recorded statistics (the test's bar is 1e-3)
    d_rm, d_rv = rel(out['G_rm_single'], out['G_rm_step1']), rel(out['G_rv_single'], out['G_rv_step1'])
    assert d_rm > 1e-2 and d_rv > 1e-2, (d_rm, d_rv)
    out['single_vs_double'] = np.array([d_rm, d_rv])
    print('losses', out['losses1'], out['losses2'])
    print('running statistics: single vs double advance differ by %.3g (mean) %.3g (var)' % (d_rm, d_rv))
    return out


def step2_distance(out):
    """How far the reference is from ITSELF in step 2: the float32 run that fills the fixture against a second float32 run on one thread
    (another summation order) and a float64 run of the same step.  Where one of the test's step-2 margins is tighter than float32 carries,
    the test's bar is twice the float32-vs-float64 distance recorded here -- never anything measured on the code under test."""
    f32b, f64 = generate(torch.float32, threads=1), generate(torch.float64)
    a, b, d = (json.loads(str(o['losses2'])) for o in (out, f32b, f64))
    out['losses2_f64'] = json.dumps(d)
    out['losses2_f32_vs_f64'] = json.dumps({k: max(abs(a[k] - d[k]), abs(b[k] - d[k])) for k in LOSSES})
    out['losses2_f32_vs_f32'] = json.dumps({k: abs(a[k] - b[k]) for k in LOSSES})
    out['stats2_f32_vs_f64'] = np.array([max(rel(o[k], f64[k]) for o in (out, f32b)) for k in ('G_rm_step2', 'G_rv_step2')])
    print('step 2, float32 vs float64:', out['losses2_f32_vs_f64'], 'statistics', out['stats2_f32_vs_f64'])
    print('step 2, float32 (8 threads) vs float32 (1 thread):', out['losses2_f32_vs_f32'])


def main():
    out = generate()
    step2_distance(out)
    path = os.path.join(MG.OUT, 'spade_model_step.npz')
    if '--check' in sys.argv:
        old = np.load(path, allow_pickle=False)
        assert sorted(old.files) == sorted(out), 'key sets differ'
        for k in old.files:
            np.testing.assert_array_equal(old[k], np.asarray(out[k]), err_msg=k)
        print('spade_model_step.npz regenerates bit-identically (%d arrays)' % len(old.files))
        return
    np.savez_compressed(path, **out)
    print('spade_model_step.npz', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
