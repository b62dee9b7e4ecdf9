"""The fused block path at the reference's default kernel sizes [3, 5, 7] (fused_block.set_k7 / CAT_FUSED_K7) against the layer-by-layer path.

One measuring process per (tree, round), started by this driver as a bounded child (its own time limit; a child that fails or runs out of
time ends the whole run: nothing more is started on the GPU).  Trees alternate within a round, so a drift of the machine hits both alike:

    python tools/k7_block_bench.py [--trees this=. parent=/path/to/parent/checkout=block,runner] [--rounds 3] [--out profiles/k7_block_bench.txt]

A tree is name=path[=what]: a checkout with its library built and, optionally, the measurements to take there (default: --what).  The child
runs THIS file with the tree's package first on sys.path.  A tree without fused_block.set_k7 (the parent commit) runs every [3, 5, 7] block
layer by layer, which is also what `this` does with the switch off; the parent commit cannot run the [3, 5, 7] pix2pix step at all (its
BatchNorm-folded teacher, cat_amd/frozen.py, packs the 7 x 7 residual convs with cat_tconv_pack, which refused kernel size 7), so there the
step is left out and `this` with the switch off is the step's baseline.
Per child, by HIP events:
    block77     one block at (8, 77, 64, 64), student widths (11, 12, 18) / (15, 15, 12), BatchNorm, reflect: forward + backward, us
    block256    one block at (8, 256, 64, 64), 42-wide branches, InstanceNorm with affine, reflect: forward + backward, us (its 33 depthwise
                quads need CAT_FUSED_WIDE as well: the child switches both on)
    step        the graphed pix2pix distillation step of cat_amd/synthetic.py's option set with kernel_sizes [3, 5, 7], 256 x 256, batch 16,
                student pruned to 4.6e9 MACs: ms per replay
    runner1/16  StudentRunner(graph=True) on a seeded InstanceNorm student (the canonical [3, 5, 7] teacher pruned to 2.6e9 MACs), 256 x 256,
                batch 1 and batch 16: ms per batch
Medians over the rounds with their spread (max - min)."""
import argparse
import copy
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


def _one_block(c, m, norm, dev):
    import functools
    import torch
    from cat_amd import nn as cnn, ops, synthetic
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    nl = cnn.BatchNorm2d if norm == 'batch' else functools.partial(cnn.InstanceNorm2d, affine=True, track_running_stats=False)
    res, dw = m
    blk = InvertedResidualChannels(c, list(res), list(dw), 1, list(KS), list(KS), padding_type='reflect', use_bias=norm != 'batch', norm_layer=nl,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    blk.load_state_dict(synthetic.fill_state_dict(blk.state_dict(), 77, gamma_abs_normal=True))
    blk = blk.to(dev).train()
    x = ops.to_nhwc(synthetic.normal((8, c, 64, 64), 5).to(dev)).detach().requires_grad_(True)
    gy = ops.to_nhwc(synthetic.normal((8, c, 64, 64), 6).to(dev))

    def fb():
        x.grad = None
        blk.zero_grad(set_to_none=True)
        blk(x).backward(gy)
    return blk, x, fb


def _distiller(dev):
    import itertools
    import torch
    from cat_amd import networks, prune, synthetic
    from cat_amd.distillers import create_distiller
    from cat_amd.optim import FusedAdam
    opt = synthetic.default_options(norm='batch', track=True, ndf=128, dataset_mode='aligned', gan_mode='hinge', lambda_recon=100.0, lambda_distill=1.3,
                                    kernel_sizes=list(KS), target_flops=4.6e9, prune_cin_lb=16, student_ngf=32, gpu_ids=[0], data_height=256,
                                    data_width=256)
    torch.manual_seed(233)
    model = create_distiller(opt, verbose=False)
    model.netG_teacher.load_state_dict(synthetic.fill_state_dict(model.netG_teacher.state_dict(), synthetic.SEED_TEACHER, gamma_abs_normal=True))
    model.setup(opt, verbose=False)
    prune.shrink(model, opt)
    model.netG_student = networks.init_net(model.netG_student, opt.init_type, opt.init_gain, []).to(model.device)
    model.remove_mapping_hook()
    gp = [a.parameters() for a in model.netAs]
    model.optimizer_G = FusedAdam([{'params': model.netG_student.parameters()}, {'params': itertools.chain(*gp)}], lr=opt.lr, betas=(opt.beta1, 0.999))
    model.optimizers = [model.optimizer_G, model.optimizer_D]
    model.add_mapping_hook()
    model.netG_student.train()
    model.netD.train()
    return model


def _instance_student(dev):
    from cat_amd import networks, prune, synthetic
    opt = synthetic.default_options(norm='instance', track=False, target_flops=2.6e9, gpu_ids=[], kernel_sizes=list(KS))
    T = networks.define_G(3, 3, 64, 'inception_9blocks', 'instance', 0, 'normal', 0.02, [], opt=opt)
    T.load_state_dict(synthetic.fill_state_dict(T.state_dict(), synthetic.SEED_TEACHER, gamma_abs_normal=True))
    T.eval()
    thr, _ = prune.search_threshold(T, opt.target_flops, opt)
    S = copy.deepcopy(T)
    prune._apply_structure(S, T, thr, opt, copy_weights=True)
    sd = synthetic.fill_state_dict(S.state_dict(), 21)
    sd['up_sampling.7.weight'] = sd['up_sampling.7.weight'] / 64      # keeps the closing tanh out of saturation (timing does not care)
    S.load_state_dict(sd)
    return S.to(dev).eval()


def child(a):
    import torch
    from cat_amd import _lib, fused_block, ops, synthetic
    from cat_amd.inception_modules import InvertedResidualChannels
    _lib.load()
    dev = torch.device('cuda:0')
    has_k7 = hasattr(fused_block, 'set_k7')
    if has_k7:
        fused_block.set_k7(bool(a.k7))
    out = {'has_k7': has_k7, 'k7': bool(a.k7) and has_k7}
    names = []
    real = _lib.call

    def logged(name, *args):
        names.append(name)
        return real(name, *args)
    if 'block' in a.what:
        for key, c, m, norm in (('block77', 77, ((11, 12, 18), (15, 15, 12)), 'batch'), ('block256', 256, ((42, 42, 42), (42, 42, 42)), 'instance')):
            old = fused_block.set_wide(True) if c == 256 and out['k7'] else None
            blk, x, fb = _one_block(c, m, norm, dev)
            out[key + '_fused'] = bool(fused_block.applicable(blk, x))
            fb()
            _lib.call = logged
            try:
                del names[:]
                fb()
            finally:
                _lib.call = real
            out[key + '_calls'] = len(names)
            out[key + '_us'] = 1e3 * _time(fb, 3, a.iters)
            if old is not None:
                fused_block.set_wide(old)
            del blk, x, fb
            torch.cuda.empty_cache()
    if 'runner' in a.what:      # before the step: a training step leaves process-wide state behind that slows a later eval capture
        from cat_amd.infer import StudentRunner
        S = _instance_student(dev)
        for n in (1, 16):
            x = ops.to_nhwc(synthetic.images((n, 3, 256, 256), 970 + n).cuda())
            r = StudentRunner(S, x, graph=True)
            out['runner%d_ms' % n] = _time(lambda: r(x), 5, a.iters)
            r.release()
            del r
            torch.cuda.empty_cache()
    if 'step' in a.what:
        from cat_amd.graph import GraphedStep
        model = _distiller(dev)
        blocks = [b for b in model.netG_student.modules() if isinstance(b, InvertedResidualChannels)]
        out['student_blocks'] = [[list(b.res_channels), list(b.dw_channels)] for b in blocks]
        batches = [{'A': synthetic.images((16, 3, 256, 256), 1000 + 10 * i).cuda(), 'B': synthetic.images((16, 3, 256, 256), 2000 + 10 * i).cuda(),
                    'A_paths': [], 'B_paths': []} for i in range(2)]
        step = GraphedStep(model, batches[0])
        i = [0]

        def replay():
            i[0] += 1
            step(batches[i[0] & 1])
        out['step_ms'] = _time(replay, 3, a.step_iters)
        del step, model
        torch.cuda.empty_cache()
    print('K7BENCH ' + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trees', nargs='+', default=['this=' + os.path.dirname(os.path.dirname(HERE))])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--what', default='block,step,runner')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--step-iters', type=int, default=10, dest='step_iters')
    ap.add_argument('--timeout', type=int, default=240, help='seconds per child')
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--k7', type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    trees = [(t.split('=') + [a.what])[:3] for t in a.trees]
    runs = [(name, path, 1, what) for name, path, what in trees]
    runs.insert(1, (trees[0][0] + ', CAT_FUSED_K7=0', trees[0][1], 0, trees[0][2]))      # the first tree also with the switch off
    res = {name: [] for name, _, _, _ in runs}
    for rnd in range(a.rounds):
        for name, path, k7, what in runs:
            path = os.path.abspath(path)
            env = dict(os.environ, PYTHONPATH=path + os.pathsep + os.environ.get('PYTHONPATH', ''))
            cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, HERE, '--child', '--k7', str(k7), '--what', what, '--iters', str(a.iters),
                   '--step-iters', str(a.step_iters)]
            p = subprocess.run(cmd, cwd=path, env=env, capture_output=True, text=True)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('K7BENCH ')]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit('k7_block_bench: child (%s, round %d) ended with %d: stopping' % (name, rnd, p.returncode))
            res[name].append(json.loads(line[0][8:]))
            print('round %d  %-24s %s' % (rnd, name, line[0][8:]), flush=True)
    lines = ['kernel sizes [3, 5, 7]: fused block path (CAT_FUSED_K7) against layer by layer; one process per (tree, round), trees alternating,',
             'median of %d rounds, spread = max - min' % a.rounds, '']
    keys = [('block77_us', 'block (8, 77, 64, 64) fwd + bwd, us'), ('block256_us', 'block (8, 256, 64, 64) fwd + bwd, us'),
            ('step_ms', 'graphed pix2pix distillation step, batch 16, ms'), ('runner1_ms', 'StudentRunner(graph=True) batch 1, ms'),
            ('runner16_ms', 'StudentRunner(graph=True) batch 16, ms')]
    for key, title in keys:
        lines.append(title)
        for name, rs in res.items():
            if not all(key in r for r in rs):
                lines.append('    %-24s not measured' % name)
                continue
            v = [r[key] for r in rs]
            extra = ''
            if key.startswith('block'):
                extra = '   fused path %s, %d library calls per fwd + bwd' % (rs[0][key[:-3] + '_fused'], rs[0][key[:-3] + '_calls'])
            lines.append('    %-24s %s   median %.3f, spread %.3f%s' % (name, '  '.join('%.3f' % t for t in v), statistics.median(v), max(v) - min(v), extra))
    first = next(iter(res.values()))[0]
    if 'student_blocks' in first:
        lines += ['', 'student of the step (res widths, dw widths per block): %s' % first['student_blocks']]
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
