"""Generate tests/golden/step_syncbn.npz and step_smooth_l1.npz by RUNNING THE REFERENCE on the CPU, like tools/make_golden.py (whose
run_config this drives, so the layout is step_bn.npz's):

  step_syncbn.npz     the `bn` configuration of make_golden.main_configs() with norm='syncbatch', plus the student's and the
                      discriminator's num_batches_tracked after each step (`nbt{step}:S` / `nbt{step}:D`, one entry per norm layer)
  step_smooth_l1.npz  the `in` configuration with recon_loss_type='smooth_l1' (torch.nn.SmoothL1Loss(), base_inception_distiller.py:176-177)

The reference's shrink of the syncbatch teacher is compared against the committed shrink_bn.npz (threshold, MACs, configuration, copied
weights); shrink_syncbn.npz is written only if they differ.  Run in the build container only:  python tools/make_golden_norm_recon.py"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the reference import)
import torch  # noqa: E402

_ref_distiller = mg.ref_distiller


def _run(tag, args, recon=None, record_nbt=False, **kw):
    """make_golden.run_config into a scratch directory -> (step dict, shrink dict).  `recon`: the criterion the reference's constructor
    would have built; `record_nbt`: every num_batches_tracked of student and discriminator after each optimize_parameters."""
    extra = {}

    def distiller(opt, T, D):
        m = _ref_distiller(opt, T, D)
        if recon is not None:
            m.criterionRecon = recon
        if record_nbt:
            step_fn = m.optimize_parameters

            def optimize_parameters(step):
                step_fn(step)
                for name, net in (('S', m.netG_student), ('D', m.netD)):
                    nbt = [v for k, v in net.state_dict().items() if k.endswith('num_batches_tracked')]
                    extra[f'nbt{step}:{name}'] = torch.stack(nbt).numpy().astype(np.int64)
            m.optimize_parameters = optimize_parameters
        return m

    with tempfile.TemporaryDirectory() as tmp:
        mg.OUT, mg.ref_distiller = tmp, distiller
        mg.run_config(tag, *args, keep=('shrink', 'step'))
        step = dict(np.load(os.path.join(tmp, f'step_{tag}.npz'), allow_pickle=False))
        shrink = dict(np.load(os.path.join(tmp, f'shrink_{tag}.npz'), allow_pickle=False))
    meta = json.loads(str(step['meta']))
    meta.update(kw)
    step['meta'] = json.dumps(meta)
    step.update(extra)
    return step, shrink


def main():
    out = os.path.join(mg.ROOT, 'tests', 'golden')
    # ---- --norm syncbatch: the `bn` configuration ------------------------------------------------------------------------------
    step, shrink = _run('syncbn', ('syncbatch', True, 4.6e9, 'aligned', 'hinge', 128, 100.0, 1.3, 64, 2), record_nbt=True)
    assert all(not step[k].any() for k in step if k.startswith('nbt')), 'the reference advanced num_batches_tracked'
    np.savez_compressed(os.path.join(out, 'step_syncbn.npz'), **step)
    bn = np.load(os.path.join(out, 'shrink_bn.npz'), allow_pickle=False)
    differ = [k for k in bn.files if k != 'norm' and not np.array_equal(bn[k], shrink[k])] + [k for k in shrink if k not in bn.files]
    if differ:
        np.savez_compressed(os.path.join(out, 'shrink_syncbn.npz'), **shrink)
        print('shrink of the syncbatch teacher DIFFERS from shrink_bn.npz in', differ, '-> wrote shrink_syncbn.npz')
    else:
        print('shrink of the syncbatch teacher equals shrink_bn.npz (%d entries): no new fixture' % len(bn.files))
    # ---- --recon_loss_type smooth_l1: the `in` configuration -------------------------------------------------------------------
    step, _ = _run('smooth_l1', ('instance', False, 2.6e9, 'unaligned', 'lsgan', 64, 5.0, 1.0, 64, 2), recon=torch.nn.SmoothL1Loss(),
                   recon_loss_type='smooth_l1')
    np.savez_compressed(os.path.join(out, 'step_smooth_l1.npz'), **step)


if __name__ == '__main__':
    main()
