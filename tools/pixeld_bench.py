"""Time the 1x1 PixelGAN discriminator (`--netD pixel`) on the fused kernels (csrc/pixel_d.hip) against the general path (the same module layer by
layer on the general kernels, CAT_PIXELD=0), at the headline shape: 256 x 256, batch 16 (M = 1 048 576 pixels), ndf 128.

Per channel count C0 in {6 (aligned, BatchNorm: the pix2pix distillation), 3 (unaligned, InstanceNorm: the CycleGAN-style one)}:
  (a) forward + backward with parameter gradients and no dx   -- what backward_D runs, twice per step
  (b) forward + backward with dx and the parameters frozen    -- what backward_G runs
then one whole InceptionDistiller.optimize_parameters (bench.py's pix2pix workload with netD='pixel').  Each figure: warm-up, then HIP events
around --iters calls on the stream (100 by default: a window of about half a second per figure), one synchronisation at the end.  The switch is read at import, so every run is a child process; the two
modes alternate over --repeats runs each and the table gives the median and the spread.  Rates are algorithmic: the two 2 M C1 C2 products
(68.7 GFLOP each) the call has to do -- one in forward, one (dx only) or two (parameter gradients) in backward -- over the call's time, and
the bytes of the pre-norm tensor z the FUSED decomposition moves (forward: 1 write + 1 read; backward: 2 reads) over the same time.

    python tools/pixeld_bench.py [--repeats 3] [--iters 100] [--warmup 5] [--no-step]         # prints a table and one JSON line"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, SIZE, NDF = 16, 256, 128
CONFIGS = {6: 'batch', 3: 'instance'}


def _time(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def child(a):
    import torch
    from cat_amd import networks, ops, pixel_d, synthetic
    out = {'fused': pixel_d.ENABLED}
    for c0, norm in CONFIGS.items():
        opt = synthetic.default_options(norm=norm, track=norm == 'batch', ndf=NDF, gpu_ids=[0])
        torch.manual_seed(233)
        D = networks.define_D(c0, NDF, 'pixel', 3, norm, 'normal', 0.02, [0], opt=opt).train()
        x = ops.to_nhwc(synthetic.images((N, c0, SIZE, SIZE), 900 + c0).cuda())
        gout = ops.to_nhwc((synthetic.images((N, 1, SIZE, SIZE), 910 + c0) * 1e-3).cuda())
        assert pixel_d.applicable(D, x) == pixel_d.ENABLED

        def call(params):
            for p in D.parameters():
                p.requires_grad_(params)
                p.grad = None
            leaf = x if params else x.detach().requires_grad_(True)
            D(leaf).backward(gout)

        out[f'a{c0}'] = _time(lambda: call(True), a.warmup, a.iters)
        out[f'b{c0}'] = _time(lambda: call(False), a.warmup, a.iters)
        with torch.no_grad():
            out[f'f{c0}'] = _time(lambda: D(x), a.warmup, a.iters)
        del D, x, gout
        torch.cuda.empty_cache()
    if not a.no_step:
        import bench
        bench.C2 = dict(bench.C2, netD='pixel')
        model, opt = bench.build_model(Namespace(workload='c2', target_flops=4.6e9, size=SIZE), 0)
        batches = [{'A': synthetic.images((N, 3, SIZE, SIZE), 920 + i).cuda(), 'B': synthetic.images((N, 3, SIZE, SIZE), 930 + i).cuda(),
                    'A_paths': [], 'B_paths': []} for i in range(2)]
        k = [0]

        def step():
            model.set_input(batches[k[0] % 2])
            model.optimize_parameters(k[0])
            k[0] += 1
        out['step'] = _time(step, a.warmup, a.iters)
        out['finite'] = all(v == v and abs(v) < 1e30 for v in model.get_current_losses().values())
    print('RESULT ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = {'1': [], '0': []}
    for rep in range(a.repeats):
        for mode in ('1', '0'):
            cmd = [sys.executable, os.path.abspath(__file__), '--child', '--iters', str(a.iters), '--warmup', str(a.warmup)] + \
                  (['--no-step'] if a.no_step else [])
            r = subprocess.run(cmd, env=dict(os.environ, CAT_PIXELD=mode), capture_output=True, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit('child failed (CAT_PIXELD=%s)' % mode)
            res = json.loads(line[0][len('RESULT '):])
            assert res['fused'] == (mode == '1')
            runs[mode].append(res)
    m = N * SIZE * SIZE
    gemm = 2.0 * m * NDF * 2 * NDF                  # FLOP of one C1 x C2 product over all pixels
    zbytes = 4.0 * m * 2 * NDF
    work = {'a': (3 * gemm, 4 * zbytes), 'b': (2 * gemm, 4 * zbytes), 'f': (gemm, 2 * zbytes)}
    keys = [k + str(c) for c in CONFIGS for k in ('a', 'b', 'f')] + ([] if a.no_step else ['step'])
    names = {'a': 'fwd + bwd, parameter gradients, no dx', 'b': 'fwd + bwd, dx, parameters frozen', 'f': 'forward, no grad'}
    summary = {}
    print('%-52s %12s %12s %7s   %s' % ('ms per call: median [min, max] of %d runs' % a.repeats, 'fused', 'general', 'ratio', 'fused: TFLOP/s on the GEMMs, GB/s on z'))
    for k in keys:
        fu, ge = [r[k] for r in runs['1']], [r[k] for r in runs['0']]
        mf, mg = statistics.median(fu), statistics.median(ge)
        label = 'optimize_parameters, netD pixel (C0 6)' if k == 'step' else 'C0 %s %s: %s' % (k[1:], CONFIGS[int(k[1:])], names[k[0]])
        rate = ''
        if k != 'step':
            fl, by = work[k[0]]
            rate = '%.1f TFLOP/s, %.0f GB/s' % (fl / mf * 1e-9, by / mf * 1e-6)
        print('%-52s %12.3f %12.3f %7.2f   %s' % (label, mf, mg, mg / mf, rate))
        print('%-52s %12s %12s' % ('', '[%.3f, %.3f]' % (min(fu), max(fu)), '[%.3f, %.3f]' % (min(ge), max(ge))))
        summary[k] = dict(fused_ms=mf, general_ms=mg, fused_range=[min(fu), max(fu)], general_range=[min(ge), max(ge)])
    if not a.no_step:
        assert all(r['finite'] for rs in runs.values() for r in rs)
    faster = all(summary[k + str(c)]['fused_ms'] < summary[k + str(c)]['general_ms'] for c in CONFIGS for k in ('a', 'b'))
    print('fused faster than general in (a) and (b) for both channel counts: %s' % faster)
    print(json.dumps(dict(shape=[N, SIZE, SIZE], ndf=NDF, repeats=a.repeats, iters=a.iters, fused_faster=faster, results=summary)))


if __name__ == '__main__':
    main()
