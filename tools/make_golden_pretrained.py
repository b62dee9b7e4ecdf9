"""Generate tests/golden/pretrained_student.npz by RUNNING THE REFERENCE's load_pretrained_student / load_pretrained_spade_student
(utils/common.py:49-312, imported on the CPU like tools/make_golden.py does).  Build container only:

    python tools/make_golden_pretrained.py

Per case the checkpoint is NOT stored: it is `detfill.fill_state_dict(<recorded shapes>, <recorded seed>)`, which the tests rebuild.  The
shapes are the shrunk students of the existing shrink fixtures (shrink_bn.npz, shrink_in.npz, spade_shrink.npz tag a) and one hand-pruned
variant of each: a block without res_ops, a block without any branch, a branch one channel wide -- shapes only checkpoints produce.
Recorded: every block's channel / kernel lists, n_macs, keys and shapes of the loaded student, the netA shapes, optimizer_G's groups and
hyper-parameters, and a sub-sample of the loaded student's eval-mode forward in float32 and float64 (head conv scaled by a recorded power
of two: record_forward).  No reference source is stored."""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.environ['GOLDEN_STEP'] = '0'          # make_golden_spade: import its builders, do not regenerate spade_step.npz
import make_golden as MG  # noqa: E402  (installs the reference import recipe)
import make_golden_spade as MGS  # noqa: E402
import torch  # noqa: E402
from models import networks  # noqa: E402  (reference)
from utils import common as uc  # noqa: E402

from oracle import detfill  # noqa: E402
import helpers as H  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
SEED_CKPT, SEED_IN = 701, 711
INCEPTION_X = (2, 3, 196, 516)      # trunk planes 49 x 129: odd, two samples fill the LDS-tile kernels' minimum, one sample does not
SPADE_X = (2, 6, 128, 256)
SUB = 6
HEAD = {'inception': ('up_sampling.7.weight', 'up_sampling.7.bias'), 'spade': ('conv_img.weight', 'conv_img.bias')}


def prune_shapes(shapes, family):
    """The hand-pruned variant: [key, shape] list -> list."""
    if family == 'spade':
        no_res, no_branch, thin = 'G_middle_0.', 'G_middle_1.', 'up_0.dw_ops.0.'
        last_w, last_b = '.2.conv.weight', '.2.conv.bias'
    else:
        no_res, no_branch, thin = 'features.1.', 'features.2.', 'features.3.dw_ops.0.'
        last_w, last_b = '.4.weight', '.4.bias'
    out = []
    for k, s in shapes:
        if k.startswith(no_res + 'res_ops.') or k.startswith(no_branch + 'res_ops.') or k.startswith(no_branch + 'dw_ops.'):
            continue
        s = list(s)
        if k.startswith(thin) and not k.endswith('num_batches_tracked') and not k.endswith(last_b):
            s[1 if k.endswith(last_w) else 0] = 1
        out.append([k, s])
    return out


def checkpoint(shapes, seed):
    return detfill.fill_state_dict(H.sd_from_shapes(json.dumps(shapes)), seed)


def sub(y):
    return y.detach()[:, :, ::SUB, ::SUB].contiguous().numpy()


def record_forward(out, tag, S, head, x, family):
    """detfill's unit-variance layers drive the closing tanh into saturation, where every error vanishes: the head conv (weight and bias) is
    scaled by the power of two that brings its output to unit scale -- in the loaded student here, in the checkpoint by the tests (the
    recorded `head_scale`; a power of two commutes with every rounding) -- and the eval-mode forward is recorded in float64 and in float32."""
    seen = {}
    handle = head.register_forward_hook(lambda mod, inp, res: seen.update(std=float(res.double().std())))
    S.eval()
    with torch.no_grad():
        S(x)
        handle.remove()
        scale = 2.0 ** round(float(np.log2(1.0 / seen['std'])))
        head.weight.mul_(scale)
        head.bias.mul_(scale)
        out[f'{tag}:out32'] = sub(S(x)).astype(np.float32)
        S.double()
        out[f'{tag}:out'] = sub(S(x.double())).astype(np.float64)
    out[f'{tag}:head_scale'] = np.float64(scale)
    out[f'{tag}:head_keys'] = json.dumps(list(HEAD[family]))
    print(tag, 'head scale', scale, 'saturated share', float((np.abs(out[f'{tag}:out']) > 0.999).mean()))


def record_common(out, tag, S, net_as, optim, shapes, x_shape):
    out[f'{tag}:shapes'] = json.dumps(shapes)
    out[f'{tag}:seed'] = np.int64(SEED_CKPT)
    out[f'{tag}:loaded_shapes'] = MG.shapes_json(S.state_dict())
    out[f'{tag}:n_macs'] = np.int64(S.n_macs)
    out[f'{tag}:netA'] = json.dumps([list(a.weight.shape) for a in net_as])
    out[f'{tag}:optim'] = json.dumps([dict(n=len(g['params']), lr=g['lr'], betas=[float(b) for b in g['betas']]) for g in optim.param_groups])
    out[f'{tag}:x'] = json.dumps(dict(shape=list(x_shape), seed=SEED_IN, sub=SUB))


def inception_case(out, tag, norm, track, target, dataset_mode, gan_mode, ndf, pruned):
    g = H.load(f'shrink_{"bn" if norm == "batch" else "in"}.npz')
    shapes = json.loads(str(g['student_shapes']))
    if pruned:
        shapes = prune_shapes(shapes, 'inception')
    opt = MG.ref_import.make_opt(norm=norm, track=track, target_flops=target, dataset_mode=dataset_mode, gan_mode=gan_mode, ndf=ndf)
    with tempfile.TemporaryDirectory() as d:
        opt.pretrained_student_G_path = os.path.join(d, 'student.pth')
        torch.save(checkpoint(shapes, SEED_CKPT), opt.pretrained_student_G_path)
        T = MG.teacher(opt)
        D = networks.define_D(6 if dataset_mode == 'aligned' else 3, ndf, 'n_layers', 3, norm, 'normal', 0.02, [], opt=opt)
        m = MG.ref_distiller(opt, T, D)
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            uc.load_pretrained_student(m, opt)
    S = m.netG_student
    out[f'{tag}:prints'] = json.dumps([ln for ln in buf.getvalue().splitlines() if ln.startswith('features.')])
    out[f'{tag}:blocks'] = json.dumps([[b.res_channels, b.res_kernel_sizes, b.dw_channels, b.dw_kernel_sizes] for b in S.features])
    out[f'{tag}:opt'] = json.dumps(dict(norm=norm, track=track, target_flops=target, dataset_mode=dataset_mode, gan_mode=gan_mode, ndf=ndf))
    record_common(out, tag, S, m.netAs, m.optimizer_G, shapes, INCEPTION_X)
    assert m.optimizers[0] is m.optimizer_G and len(m.schedulers) == 2
    record_forward(out, tag, S, S.up_sampling[-2], detfill.images(INCEPTION_X, SEED_IN), 'inception')
    print(tag, 'n_macs', int(S.n_macs), 'blocks[1..3]', json.loads(out[f'{tag}:blocks'])[1:4])


def spade_input(shape, seed):
    """A detfill field thresholded into sparse 0 / 1 maps (what the one-hot label + edge planes look like to the network)."""
    return (detfill.normal(shape, seed) > 0.8).float()


def spade_case(out, tag, pruned):
    from argparse import Namespace
    uc.Adam = lambda params, lr, betas: torch.optim.Adam(params, lr=lr, betas=(float(betas[0]), float(betas[1])))   # torch 2.10 rejects int 0
    g = H.load('spade_shrink.npz')
    shapes = json.loads(str(g['a_S_shapes']))
    if pruned:
        shapes = prune_shapes(shapes, 'spade')
    opt = MGS.spade_opt(target_flops=float(g['a_target']), prune_cin_lb=int(g['a_lb']), data_height=128, data_width=256, data_channel=6,
                        lr_policy='linear')
    with tempfile.TemporaryDirectory() as d:
        opt.pretrained_student_G_path = os.path.join(d, 'student.pth')
        torch.save(checkpoint(shapes, SEED_CKPT), opt.pretrained_student_G_path)
        m = MGS.build(opt)
        m.netG_teacher.load_state_dict(detfill.fill_state_dict(m.netG_teacher.state_dict(), MGS.SEED_T + 1, gamma_abs_normal=True))
        model = Namespace(modules_on_one_gpu=m, device=torch.device('cpu'), isTrain=True,
                          optimizer_D=torch.optim.Adam(m.netD.parameters(), lr=1e-4, betas=(0.0, 0.9)))
        with contextlib.redirect_stdout(io.StringIO()):
            uc.load_pretrained_spade_student(model, opt)
    S = m.netG_student
    blocks = {}
    for name, blk in S.get_named_block_list().items():
        blocks[name] = dict(input_dim=blk.input_dim, output_dim=blk.output_dim, res=[blk.res_channels, blk.res_kernel_sizes],
                            dw=[blk.dw_channels, blk.dw_kernel_sizes], spade_res=[blk.spade.res_channels, blk.spade.res_kernel_sizes],
                            spade_dw=[blk.spade.dw_channels, blk.spade.dw_kernel_sizes], shortcut=blk.shortcut is not None)
    out[f'{tag}:blocks'] = json.dumps(blocks)
    out[f'{tag}:opt'] = json.dumps({k: v for k, v in vars(opt).items() if isinstance(v, (int, float, str, bool, list, type(None)))
                                    and k != 'pretrained_student_G_path'})
    record_common(out, tag, S, m.netAs, model.optimizer_G, shapes, SPADE_X)
    assert model.optimizers[0] is model.optimizer_G and len(model.schedulers) == 2
    record_forward(out, tag, S, S.conv_img, spade_input(SPADE_X, SEED_IN), 'spade')
    print(tag, 'n_macs', int(S.n_macs), 'G_middle_0', blocks['G_middle_0'])


def main():
    torch.set_num_threads(8)
    out = {}
    for pruned in (False, True):
        sfx = '_pruned' if pruned else ''
        inception_case(out, 'bn' + sfx, 'batch', True, 4.6e9, 'aligned', 'hinge', 128, pruned)
        inception_case(out, 'in' + sfx, 'instance', False, 2.6e9, 'unaligned', 'lsgan', 64, pruned)
        spade_case(out, 'spade' + sfx, pruned)
    path = os.path.join(OUT, 'pretrained_student.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
