"""Generate tests/golden/spade_k7_unit.npz by RUNNING THE REFERENCE's SPADEInvertedResidualChannels (snap-research/CAT imported through
tools/ref_import.py, CPU) with the parser default kernel sizes 3 5 7.  Build container only:  python tools/make_golden_spade_k7.py

Two modules, fin 24 -> fout 12, norm_G = 'spadesyncbatch3x3': 'u' unpruned (channels None) and 'p' with a pruned `channels` list.  Both are
filled deterministically as tools/make_golden_spade.py fills its networks (oracle.detfill.fill_state_dict, gamma_abs_normal) and run ONCE in
train mode on one CPU device in float64 at (2, 24, 16, 24): output, input gradient, every parameter gradient, the running statistics the
forward updated.

What is stored, to stay in the size class of the other SPADE fixtures (< 300 KB; the unpruned gamma|beta net alone has 94 000 weights):
inputs that detfill regenerates bit for bit are stored as their SEED plus three float64 checksums (x, the output gradient, the state dicts:
keys + shapes + seed, as spade_step.npz stores its networks); the segmentation map in full (uint8); outputs and input gradients in full,
rounded to float32 (6e-8 relative, far below every bar they are compared at); a parameter gradient in full (float32) up to 256 elements
and as a strided sample of at most 256 elements plus its float64 norm above; the buffers after the step (running statistics, batch counters)
in full.  No reference source is stored."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_import  # noqa: E402

ref_import.install()
import torch  # noqa: E402

from oracle import detfill  # noqa: E402
from models.modules.inception_modules import SPADEInvertedResidualChannels  # noqa: E402  (reference)

OUT = os.path.join(ROOT, 'tests', 'golden', 'spade_k7_unit.npz')
FIN, FOUT, N, H, W = 24, 12, 2, 16, 24
SEED_X, SEED_SEG, SEED_GY = 2300, 2301, 2302
MODULES = {'u': (None, 2310), 'p': ([30, 12, 18], 2311)}      # tag -> (opt.channels, state-dict seed): hidden widths 2 2 2 | 21 21 21 and 5 2 3
SAMPLE = 256


def checks(t):
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


def sample_stride(numel):
    return 1 if numel <= SAMPLE else -(-numel // SAMPLE)


def main():
    opt = ref_import.make_opt(norm_G='spadesyncbatch3x3', semantic_nc=6, kernel_sizes=[3, 5, 7], channels_reduction_factor=6, active_fn='nn.ReLU')
    x32 = detfill.normal((N, FIN, H, W), SEED_X)
    gy32 = detfill.normal((N, FOUT, H, W), SEED_GY)
    seg = (detfill.normal((N, opt.semantic_nc, H // 4, W // 4), SEED_SEG) > 0.8).float().repeat_interleave(4, 2).repeat_interleave(4, 3)
    out = dict(fin=FIN, fout=FOUT, n=N, h=H, w=W, semantic_nc=opt.semantic_nc, kernel_sizes=np.array(opt.kernel_sizes), seed_x=SEED_X, seed_gy=SEED_GY,
               x_checks=checks(x32), gy_checks=checks(gy32), seg=seg.numpy().astype(np.uint8), sample=SAMPLE)
    for tag, (channels, seed) in MODULES.items():
        opt.channels = channels
        blk = SPADEInvertedResidualChannels(FIN, FOUT, opt)
        sd0 = detfill.fill_state_dict(blk.state_dict(), seed, gamma_abs_normal=True)
        blk.load_state_dict(sd0)
        out[tag + '_channels'] = json.dumps(channels)
        out[tag + '_seed'] = seed
        out[tag + '_shapes'] = json.dumps([[k, list(v.shape)] for k, v in sd0.items()])
        out[tag + '_sd_checks'] = np.stack([checks(v) for v in sd0.values()])
        blk = blk.double().train()
        x = x32.double().requires_grad_(True)
        y = blk(x, seg.double())
        y.backward(gy32.double())
        out[tag + '_y'] = y.detach().float().numpy()
        out[tag + '_dx'] = x.grad.float().numpy()
        out[tag + '_y_checks'], out[tag + '_dx_checks'] = checks(y), checks(x.grad)
        # one array per kind (a zip member costs ~350 bytes of headers): parameter k's gradient sample is grads[goff[k]:goff[k + 1]]
        names, grads, gnorm = [], [], []
        for k, q in blk.named_parameters():
            names.append(k)
            g = q.grad.reshape(-1)
            grads.append(g[::sample_stride(g.numel())].float().numpy())
            gnorm.append(g.norm().item())
        out[tag + '_params'] = json.dumps(names)
        out[tag + '_grads'], out[tag + '_gnorm'] = np.concatenate(grads), np.array(gnorm, dtype=np.float64)
        out[tag + '_goff'] = np.cumsum([0] + [len(g) for g in grads])
        bufs = [(k, b) for k, b in blk.named_buffers()]
        out[tag + '_buffers'] = json.dumps([[k, list(b.shape)] for k, b in bufs])
        out[tag + '_bufs'] = np.concatenate([b.double().reshape(-1).numpy() for k, b in bufs]).astype(np.float32)      # (counters are small integers: exact)
        print(tag, channels, 'res', blk.res_channels, 'dw', blk.dw_channels, 'spade', blk.spade.res_channels, blk.spade.dw_channels, len(names), 'parameters')
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
