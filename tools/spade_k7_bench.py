"""The fused GauGAN units at the reference's default kernel sizes [3, 5, 7] (fused_spade.set_k7 / CAT_FUSED_SPADE_K7) against the layer-by-layer
path, and the narrow one-launch stage 1 (cat_tstage1n7_fwd / cat_tstage1n7_dgrad, csrc/conv_s1n7.hip) against the launches it replaces.

One measuring process per (tree, round), started by this driver as a bounded child (its own time limit; a child that fails or runs out of
time ends the whole run: nothing more is started on the GPU).  Trees alternate within a round, so a drift of the machine hits both alike:

    python tools/spade_k7_bench.py [--trees this=. parent=/path/to/parent/checkout] [--rounds 3] [--what unit,kernel,step,bench] [--out FILE]

profiles/spade_k7_bench.txt is the output of --what unit,kernel,step followed by that of --what bench (two runs, so that each stays short)
and the result of comparing the files of bench.py --dump-outputs between the two trees.

A tree is name=path: a checkout with its library built.  The child runs THIS file with the tree's package first on sys.path.  A tree without
fused_spade.set_k7 (the parent commit) runs every [3, 5, 7] unit layer by layer, which is also what `this` does with the switch off.
Per child, by HIP events:
    step        the graphed GauGAN distillation step of bench.py --workload spade with kernel_sizes [3, 5, 7]: 512 x 256, batch 4, student
                ngf 48 pruned to 5.6e9 MACs: ms per replay
    main / gb   one main unit (40 -> 16, hidden widths 5 1 2 of channels [30, 6, 12]) and the gamma|beta net of its SPADE layer (36 -> 80) at
                (4, 128, 256), student widths: forward + backward, us, and library calls per forward + backward
    s1 / dgrad  (the tree with the kernel only) cat_tstage1n7_fwd on the gamma|beta net's stage 1 (36 channels -> 8 | 4 | 8 | 20 columns) and
                cat_tstage1n7_dgrad on its backward step 4 (80 channels) per launch, against the four cat_tconv_fwd of stage 1 and the four
                (three wide + the concatenated 1 x 1) of step 4 they replace, us
    bench135    (--what with `bench`) the default bench.py line and --workload spade at kernel sizes 1 3 5, images/s
Medians over the rounds with their spread (max - min)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.abspath(__file__)
KS = [3, 5, 7]


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


def _unit(dev):
    """one SPADEInvertedResidualChannels at student widths, and its two units as callables: the main unit needs the whole block (its SPADE layer
    in front), so `main` = block forward + backward minus nothing -- the gamma|beta net is timed on its own as well"""
    from argparse import Namespace
    import torch
    from cat_amd import ops, synthetic
    from cat_amd.inception_modules import SPADEInvertedResidualChannels, _run_branches
    o = Namespace(kernel_sizes=list(KS), channels=[30, 6, 12], channels_reduction_factor=6, active_fn='nn.ReLU', norm_G='spadesyncbatch3x3', semantic_nc=36)
    blk = SPADEInvertedResidualChannels(40, 16, o)
    blk.load_state_dict(synthetic.fill_state_dict(blk.state_dict(), 411, gamma_abs_normal=True))
    blk = blk.to(dev).train()
    n, h, w = 4, 128, 256
    x = ops.to_nhwc(synthetic.normal((n, 40, h, w), 600).to(dev)).detach().requires_grad_(True)
    seg = ops.to_nhwc((synthetic.normal((n, 36, h // 4, w // 4), 413) > 0.8).float().repeat_interleave(4, 2).repeat_interleave(4, 3).to(dev))
    gy = ops.to_nhwc(synthetic.normal((n, 16, h, w), 414).to(dev))
    ggb = ops.to_nhwc(synthetic.normal((n, 80, h, w), 415).to(dev))

    def block():
        x.grad = None
        blk.zero_grad(set_to_none=True)
        blk(x, seg).backward(gy)

    def gb():
        from cat_amd import fused_spade
        sp = blk.spade
        sp.zero_grad(set_to_none=True)
        if fused_spade.applicable(sp.res_ops, sp.dw_ops, seg, True):
            y = fused_spade.apply(sp, fused_spade.GB, sp.res_ops, sp.dw_ops, sp.input_dim, 2 * sp.output_dim, seg)
        else:
            y = _run_branches(list(sp.res_ops) + list(sp.dw_ops), seg)
        y.backward(ggb)
    return blk, block, gb


def _kernel_times(dev, iters):
    """cat_tstage1n7_fwd / _dgrad per launch against the cat_tconv_fwd launches they replace, on the gamma|beta net's shapes"""
    import ctypes as C
    import torch
    from cat_amd import _lib as L, ops, tconv
    n, h, w = 4, 128, 256
    out = {}
    for key, cin, widths in (('s1', 36, {7: 8, 5: 4, 3: 8, 1: 20}), ('dgrad', 80, {7: 8, 5: 4, 3: 8, 1: 20})):
        csi = (cin + 3) // 4 * 4
        x = torch.randn((n, h, w, csi), device=dev)
        hc = sum(widths.values())
        y = torch.empty((n, h, w, hc), device=dev)
        tiles = n * ((h + 7) // 8) * ((w + 15) // 16)
        part = torch.empty((tiles, 2, hc), device=dev)
        packs = {k: torch.randn(tconv.pack_floats(k, csi, wd), device=dev) * 0.05 for k, wd in widths.items()}
        col0, o = {}, 0
        for k in (1, 3, 5, 7):
            col0[k] = o
            o += widths[k]
        gs = L.Stage1S7Geom()
        gs.N, gs.H, gs.W, gs.xcs, gs.cin, gs.reflect, gs.ycs, gs.scs = n, h, w, csi, cin, 0, hc, hc
        pk, dxs, dxcs = (C.c_void_p * 4)(), (C.c_void_p * 4)(), (C.c_int * 4)(hc, hc, hc, hc)
        for slot, k in enumerate((7, 5, 3, 1)):
            gs.col0[slot], gs.width[slot], gs.nvalid[slot] = col0[k], widths[k], widths[k]
            pk[slot], dxs[slot] = packs[k].data_ptr(), y.data_ptr()
        stats = key == 's1'
        if stats:
            one = lambda: L.call('cat_tstage1n7_fwd', C.byref(gs), ops._p(x), pk, None, ops._p(y), ops._p(part), ops._stream())
        else:
            one = lambda: L.call('cat_tstage1n7_dgrad', C.byref(gs), ops._p(x), pk, dxs, dxcs, ops._stream())

        def per_size():
            for k in (1, 3, 5, 7):
                seg = tconv.Segment(None, k, (k - 1) // 2, False, 0, c4=csi, cin=cin, xcs=csi, ptr=x.data_ptr())
                kw = dict(stats=part.data_ptr() + 4 * col0[k], scs=hc) if stats else {}
                tconv.run([seg], packs[k], None, None, widths[k], n, h, w, h, w, ycs=hc, ycw=widths[k], yptr=y.data_ptr() + 4 * col0[k], **kw)
        out[key + '_one_us'] = 1e3 * _time(one, 5, iters)
        out[key + '_four_us'] = 1e3 * _time(per_size, 5, iters)
    return out


def _step(dev, step_iters):
    import types
    root = os.getcwd()
    sys.path.insert(0, root)
    import bench
    from cat_amd import synthetic
    from cat_amd.graph import GraphedStep
    real = synthetic.default_options
    synthetic.default_options = lambda **kw: real(**dict(kw, kernel_sizes=list(KS)))      # bench.build_spade_model with the parser default sizes
    try:
        args = types.SimpleNamespace(size=256, batch=4, target_flops=5.6e9)
        model, opt = bench.build_spade_model(args, 0)
    finally:
        synthetic.default_options = real
    batches = bench.spade_batches(args, 0, 2)
    step = GraphedStep(model, batches[0])
    i = [0]

    def replay():
        i[0] += 1
        step(batches[i[0] & 1])
    return _time(replay, 3, step_iters)


def child(a):
    import torch
    from cat_amd import _lib, fused_spade, ops
    _lib.load()
    dev = torch.device('cuda:0')
    has_k7 = hasattr(fused_spade, 'set_k7')
    if has_k7:
        fused_spade.set_k7(bool(a.k7))
    out = {'has_k7': has_k7, 'k7': bool(a.k7) and has_k7}
    if 'unit' in a.what:
        names = []
        real = _lib.call

        def logged(name, *args):
            names.append(name)
            return real(name, *args)
        blk, block, gb = _unit(dev)
        for key, fn in (('main', block), ('gb', gb)):
            fn()
            _lib.call = logged
            try:
                del names[:]
                fn()
            finally:
                _lib.call = real
            out[key + '_calls'] = len(names)
            out[key + '_n7'] = sum(nm.startswith('cat_tstage1n7') for nm in names)
            out[key + '_us'] = 1e3 * _time(fn, 3, a.iters)
        del blk, block, gb
        torch.cuda.empty_cache()
    if 'kernel' in a.what and 'cat_tstage1n7_fwd' in _lib.SIGNATURES:
        out.update(_kernel_times(dev, 5 * a.iters))
    if 'step' in a.what:
        out['step_ms'] = _step(dev, a.step_iters)
        torch.cuda.empty_cache()
    print('SPADEK7 ' + json.dumps(out), flush=True)


def bench135(path, timeout):
    """the default bench.py line and --workload spade (kernel sizes 1 3 5) of one tree -> images/s"""
    out = {}
    for key, extra in (('bench_c2', []), ('bench_spade', ['--workload', 'spade'])):
        cmd = ['timeout', '-k', '10', str(timeout), sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5', '--no-cpu-baseline', '--no-kernel-profile'] + extra
        p = subprocess.run(cmd, cwd=path, capture_output=True, text=True)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit('spade_k7_bench: bench.py (%s) ended with %d: stopping' % (key, p.returncode))
        out[key] = json.loads(line[-1])['value']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trees', nargs='+', default=['this=' + os.path.dirname(os.path.dirname(HERE))])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--what', default='unit,kernel,step,bench')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--step-iters', type=int, default=10, dest='step_iters')
    ap.add_argument('--timeout', type=int, default=300, help='seconds per child')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--k7', type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    trees = [t.split('=')[:2] for t in a.trees]
    runs = [(trees[0][0] + ', CAT_FUSED_SPADE_K7=0', trees[0][1], 0), (trees[0][0] + ', CAT_FUSED_SPADE_K7=1', trees[0][1], 1)]
    runs += [(name, path, 0) for name, path in trees[1:]]
    res = {name: [] for name, _, _ in runs}
    b135 = {name: [] for name, _ in trees}
    if not set(a.what.split(',')) & {'unit', 'kernel', 'step'}:
        runs = []
    for rnd in range(a.rounds):
        for name, path, k7 in runs:
            path = os.path.abspath(path)
            env = dict(os.environ, PYTHONPATH=path + os.pathsep + os.environ.get('PYTHONPATH', ''))
            cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, HERE, '--child', '--k7', str(k7), '--what', a.what, '--iters', str(a.iters),
                   '--step-iters', str(a.step_iters)]
            p = subprocess.run(cmd, cwd=path, env=env, capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('SPADEK7 ')]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit('spade_k7_bench: child (%s, round %d) ended with %d: stopping' % (name, rnd, p.returncode))
            res[name].append(json.loads(line[0][8:]))
            print('round %d  %-32s %s' % (rnd, name, line[0][8:]), flush=True)
        if 'bench' in a.what:
            for name, path in trees:
                b135[name].append(bench135(os.path.abspath(path), a.timeout))
                print('round %d  %-32s %s' % (rnd, name, json.dumps(b135[name][-1])), flush=True)
    lines = ['GauGAN units at kernel sizes [3, 5, 7]: fused path (CAT_FUSED_SPADE_K7) against layer by layer; one process per (tree, round), trees',
             'alternating, median of %d rounds, spread = max - min' % a.rounds, '']
    keys = [('step_ms', 'graphed GauGAN distillation step, 512 x 256, batch 4, kernel sizes 3 5 7, ms'),
            ('main_us', 'one block 40 -> 16 (SPADE layer + main unit) at (4, 128, 256), widths of channels [30, 6, 12]: fwd + bwd, us'),
            ('gb_us', 'its gamma|beta net 36 -> 80 alone: fwd + bwd, us'),
            ('s1_one_us', 'stage 1 of the gamma|beta net (36 -> 8 | 4 | 8 | 20): ONE cat_tstage1n7_fwd, us'),
            ('s1_four_us', '    the four cat_tconv_fwd launches it replaces, us'),
            ('dgrad_one_us', 'backward step 4 of the gamma|beta net (80 -> 8 | 4 | 8 | 20): ONE cat_tstage1n7_dgrad, us'),
            ('dgrad_four_us', '    the four cat_tconv_fwd launches it replaces, us')]
    for key, title in keys:
        if not any(key in r for rs in res.values() for r in rs):
            continue      # not asked for (--what)
        lines.append(title)
        for name, rs in res.items():
            if not all(key in r for r in rs):
                lines.append('    %-32s not measured' % name)
                continue
            v = [r[key] for r in rs]
            extra = ''
            if key in ('main_us', 'gb_us'):
                extra = '   %d library calls per fwd + bwd, %d of them cat_tstage1n7_*' % (rs[0][key[:-3] + '_calls'], rs[0][key[:-3] + '_n7'])
            lines.append('    %-32s %s   median %.3f, spread %.3f%s' % (name, '  '.join('%.3f' % t for t in v), statistics.median(v), max(v) - min(v), extra))
    for key, title in (('bench_c2', 'bench.py --gpus 1 --steps 20 --warmup 5 (kernel sizes 1 3 5), images/s'),
                       ('bench_spade', 'bench.py --workload spade (kernel sizes 1 3 5), images/s')):
        if 'bench' not in a.what:
            continue
        lines.append(title)
        for name, rs in b135.items():
            if not rs:
                lines.append('    %-32s not measured' % name)
                continue
            v = [r[key] for r in rs]
            lines.append('    %-32s %s   median %.3f, spread %.3f' % (name, '  '.join('%.3f' % t for t in v), statistics.median(v), max(v) - min(v)))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
