"""Generate tests/golden/pixel_d.npz and step_pixel.npz by RUNNING THE REFERENCE on the CPU (tools/make_golden.py's run_config, with the
reference's networks.define_D wrapped so that it builds netD='pixel'):

  pixel_d.npz     the reference PixelDiscriminator (models/modules/discriminators.py:82-126) at (input_nc 6, ndf 16):
                  `shapes:{norm}`  its state_dict key list and shapes for norm in {instance, batch, syncbatch} (norm_affine_D off, the parser default);
                  for instance and batch, detfill weights (seed 61) and a detfill input 2 x 6 x 8 x 8 (seed 62), in float64, train mode:
                  `out:{norm}`, `dx:{norm}` and `grad:{norm}:{key}` of loss = sum(out ** 2)
  step_pixel.npz  the `in` configuration of make_golden.main_configs() made aligned / hinge (64 x 64, batch 2) with netD='pixel', ndf 16: two
                  optimize_parameters steps in step_smooth_l1.npz's layout, plus the discriminator's weights after each step (`D{step}:net.*`).
                  net.2.bias is left out: a bias in front of InstanceNorm has an exactly zero gradient, what arrives is rounding noise, and Adam
                  turns noise of either sign into a full +-lr step -- no two float32 implementations agree on it (make_golden.probe_D leaves
                  the PatchGAN's such biases out likewise)

Run in the build container only:  python tools/make_golden_pixel_d.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the reference import)
import ref_import  # noqa: E402
import torch  # noqa: E402
from models import networks  # noqa: E402  (reference)
from oracle import detfill  # noqa: E402

SEED_W, SEED_X = 61, 62
_define_D = networks.define_D
_ref_distiller = mg.ref_distiller


def define_pixel(input_nc, ndf, netD, *args, **kw):
    return _define_D(input_nc, ndf, 'pixel', *args, **kw)


def module_fixture():
    out = {}
    for norm in ('instance', 'batch', 'syncbatch'):
        opt = ref_import.make_opt(norm=norm, track=norm != 'instance')
        opt.norm_affine_D = False
        D = _define_D(6, 16, 'pixel', 3, norm, 'normal', 0.02, [], opt=opt)
        out[f'shapes:{norm}'] = mg.shapes_json(D.state_dict())
        if norm == 'syncbatch':
            continue
        D.load_state_dict(detfill.fill_state_dict(D.state_dict(), SEED_W))
        D = D.double().train()
        x = detfill.normal((2, 6, 8, 8), SEED_X).double().requires_grad_(True)
        y = D(x)
        (y * y).sum().backward()
        out[f'out:{norm}'], out[f'dx:{norm}'] = y.detach().numpy(), x.grad.numpy()
        for k, p in D.named_parameters():
            out[f'grad:{norm}:{k}'] = p.grad.numpy()
    out['meta'] = json.dumps(dict(input_nc=6, ndf=16, seed_w=SEED_W, seed_x=SEED_X, shape=[2, 6, 8, 8]))
    np.savez_compressed(os.path.join(mg.ROOT, 'tests', 'golden', 'pixel_d.npz'), **out)
    print('pixel_d.npz', {k: json.loads(str(v)) for k, v in out.items() if k.startswith('shapes')})


def step_fixture():
    extra = {}

    def distiller(opt, T, D):
        m = _ref_distiller(opt, T, D)
        step_fn = m.optimize_parameters

        def optimize_parameters(step):
            step_fn(step)
            for k, v in m.netD.state_dict().items():
                if k != 'net.2.bias':
                    extra[f'D{step}:{k}'] = v.reshape(-1)[:64].numpy().copy()
        m.optimize_parameters = optimize_parameters
        return m

    with tempfile.TemporaryDirectory() as tmp:
        mg.OUT, mg.ref_distiller, networks.define_D = tmp, distiller, define_pixel
        try:
            mg.run_config('pixel', 'instance', False, 2.6e9, 'aligned', 'hinge', 16, 5.0, 1.0, 64, 2, keep=('step',))
        finally:
            networks.define_D, mg.ref_distiller = _define_D, _ref_distiller
        step = dict(np.load(os.path.join(tmp, 'step_pixel.npz'), allow_pickle=False))
    meta = json.loads(str(step['meta']))
    meta.update(netD='pixel')
    step['meta'] = json.dumps(meta)
    step.update(extra)
    np.savez_compressed(os.path.join(mg.ROOT, 'tests', 'golden', 'step_pixel.npz'), **step)
    print('step_pixel.npz', sorted(k for k in step if k.startswith('D1:')))


if __name__ == '__main__':
    module_fixture()
    step_fixture()
