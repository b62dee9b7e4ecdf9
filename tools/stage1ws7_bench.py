"""Stage 1 of a wide [3, 5, 7] block in ONE statistics-writing launch (cat_tstage1ws7_fwd, csrc/conv_s1ws7.hip; fused_unit.set_stage1ws7 /
CAT_STAGE1WS7) against the four cat_tconv_fwd launches it replaces, in the two consumers: the frozen InstanceNorm teacher
(cat_amd/frozen_in.py) and the wide training block (cat_amd/fused_block.py, CAT_FUSED_WIDE).

The protocol of tools/k7_teacher_bench.py: one measuring process per (tree, round), started by this driver as a bounded child (its own time
limit; a child that fails or runs out of time ends the whole run: nothing more is started on the GPU).  Trees alternate within a round, so a
drift of the machine hits both alike:

    python tools/stage1ws7_bench.py [--trees this=. parent=/path/to/parent/checkout] [--what stage1,in,step,wide,bench] [--rounds 3]
                                    [--out profiles/stage1ws7_bench.txt]

A tree is name=path[=what]: a checkout with its library built.  The child runs THIS file with the tree's package first on sys.path.  A tree
without fused_unit.set_stage1ws7 (the parent commit) issues the four launches whatever the environment says; the first tree is also measured
with CAT_STAGE1WS7=0 (--off-what).  Per child, by HIP events unless said otherwise:
    stage1  one eval-mode InstanceNorm block, 256 inputs, 42-wide branches, kernel sizes [3, 5, 7], reflect, owned, at (8, 256, 64, 64) under
            no_grad: us per forward; by the library's profiler (one profiled forward) the launches, us and algorithmic FLOPs of stage 1 -- every
            conv family of the forward but the tail's -- and with them its share of the fp32 MFMA peak
    in      the [3, 5, 7] InstanceNorm teacher (inception_9blocks, ngf 64) forward alone, its blocks owned, batch 8, 256 x 256: ms
    step    the graphed CycleGAN-style distillation step (InstanceNorm, lsgan, unaligned, ndf 64, student S_2.6; kernel sizes [3, 5, 7]),
            batch 8, 256 x 256: ms per replay
    wide    one train-mode InstanceNorm block (8, 256, 64, 64), 42-wide branches, forward + backward under CAT_FUSED_WIDE=1: us
    bench   `python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` in the tree (kernel sizes 1 3 5: nothing there may change):
            ms per step out of its JSON line; the dumps of the first round of every tree are compared byte for byte
Medians over the rounds with their spread (max - min)."""
import argparse
import ctypes as C
import filecmp
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.abspath(__file__)
sys.path.insert(0, os.path.dirname(HERE))
KS = [3, 5, 7]
M = (42, 42, 42)
TAIL = ('conv_tconv7_multi', 'conv_tconv_multi')      # the block's last launch: the K-concatenated LDS-tile sum
MFMA_F32_PEAK_TFLOPS = 157.3      # v_mfma_f32_16x16x4_f32, 256 CUs at 2.4 GHz (bench.py's figure)
C3 = dict(norm='instance', track=False, ndf=64, dataset_mode='unaligned', gan_mode='lsgan', lambda_recon=5.0, lambda_distill=1.0)


def _families(fn):
    """{family: [launches, ms, FLOPs]} of one call of fn, by the library's profiler"""
    import torch
    from cat_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.cat_prof_enable(1)
    fn()
    torch.cuda.synchronize()
    n = lib.cat_prof_collect()
    lib.cat_prof_enable(0)
    name, cnt, ms, fl = C.create_string_buffer(64), C.c_int64(), C.c_double(), C.c_double()
    out = {}
    for i in range(n):
        lib.cat_prof_family(i, name, 64, C.byref(cnt), C.byref(ms), C.byref(fl))
        out[name.value.decode()] = [cnt.value, ms.value, fl.value]
    return out


def _block(dev, train):
    import functools
    from cat_amd import nn as cnn, synthetic
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    nl = functools.partial(cnn.InstanceNorm2d, affine=False, track_running_stats=False)
    blk = InvertedResidualChannels(256, list(M), list(M), 1, list(KS), list(KS), padding_type='reflect', use_bias=True, norm_layer=nl,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    blk.load_state_dict(synthetic.fill_state_dict(blk.state_dict(), 77, gamma_abs_normal=True))
    blk = blk.to(dev)
    return blk.train() if train else blk.eval()


def _distiller(dev, batch):
    """bench.py's build_model with the c3 option set and kernel sizes [3, 5, 7]"""
    import itertools
    import torch
    from cat_amd import networks, prune, synthetic
    from cat_amd.distillers import create_distiller
    from cat_amd.optim import FusedAdam
    opt = synthetic.default_options(**C3, kernel_sizes=list(KS), target_flops=2.6e9, prune_cin_lb=16, student_ngf=32, gpu_ids=[0], data_height=256,
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


def child(a):
    import torch
    from k7_block_bench import _time
    from k7_teacher_bench import _teacher
    from cat_amd import _lib, frozen_in, fused_block, fused_unit, ops, synthetic
    _lib.load()
    dev = torch.device('cuda:0')
    has = hasattr(fused_unit, 'set_stage1ws7')
    if has:
        fused_unit.set_stage1ws7(bool(a.on))
    out = {'has_ws7': has, 'ws7': bool(a.on) and has}
    with torch.no_grad():
        if 'stage1' in a.what:
            blk = _block(dev, False)
            frozen_in.own(blk)
            x = ops.to_nhwc(synthetic.normal((8, 256, 64, 64), 5).to(dev))
            out['stage1_fused'] = bool(frozen_in.applicable(blk, x))
            out['block_us'] = 1e3 * _time(lambda: blk(x), 3, a.iters)
            out['block_families'] = _families(lambda: blk(x))
            del blk, x
            torch.cuda.empty_cache()
        if 'in' in a.what:
            net = _teacher('instance', dev)
            out['in_owned'] = len(frozen_in.own_network(net))
            x = ops.to_nhwc(synthetic.images((8, 3, 256, 256), 1000).to(dev))
            out['in_fused'] = bool(frozen_in.applicable(net.features[0], net.down_sampling(x)))
            out['in_ms'] = _time(lambda: net(x), 3, a.iters)
            del net, x
            torch.cuda.empty_cache()
    if 'wide' in a.what:
        old = fused_block.set_wide(True)
        blk = _block(dev, True)
        x = ops.to_nhwc(synthetic.normal((8, 256, 64, 64), 5).to(dev)).detach().requires_grad_(True)
        gy = ops.to_nhwc(synthetic.normal((8, 256, 64, 64), 6).to(dev))
        out['wide_fused'] = bool(fused_block.applicable(blk, x))

        def fb():
            x.grad = None
            blk.zero_grad(set_to_none=True)
            blk(x).backward(gy)
        out['wide_us'] = 1e3 * _time(fb, 3, a.iters)
        fused_block.set_wide(old)
        del blk, x, gy
        torch.cuda.empty_cache()
    if 'step' in a.what:
        from cat_amd.graph import GraphedStep
        model = _distiller(dev, 8)
        batches = [{'A': synthetic.images((8, 3, 256, 256), 1000 + 10 * i).cuda(), 'B': synthetic.images((8, 3, 256, 256), 2000 + 10 * i).cuda(),
                    'A_paths': [], 'B_paths': []} for i in range(2)]
        step = GraphedStep(model, batches[0])
        i = [0]

        def replay():
            i[0] += 1
            step(batches[i[0] & 1])
        out['step_ms'] = _time(replay, 3, a.step_iters)
    print('STAGE1WS7 ' + json.dumps(out), flush=True)


def _stage1(fam):
    """stage 1 of one block forward as (launches, us, FLOPs): every conv family but the tail's"""
    keys = [k for k in fam if k.startswith('conv_') and k not in TAIL]
    return sum(fam[k][0] for k in keys), 1e3 * sum(fam[k][1] for k in keys), sum(fam[k][2] for k in keys)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trees', nargs='+', default=['this=' + os.path.dirname(os.path.dirname(HERE))])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--what', default='stage1,in,step,wide')
    ap.add_argument('--off-what', default='stage1,in,wide', dest='off_what', help='what the first tree also measures with CAT_STAGE1WS7=0')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--step-iters', type=int, default=10, dest='step_iters')
    ap.add_argument('--bench-steps', type=int, default=10, dest='bench_steps')
    ap.add_argument('--bench-warmup', type=int, default=3, dest='bench_warmup')
    ap.add_argument('--timeout', type=int, default=300, help='seconds per child')
    ap.add_argument('--out', default=None, help='the table is appended to this file')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--on', type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    trees = [(t.split('=') + [a.what])[:3] for t in a.trees]
    runs = [(name, path, 1, what) for name, path, what in trees]
    off = ','.join(w for w in a.off_what.split(',') if w in trees[0][2].split(','))
    if off:
        runs.insert(1, (trees[0][0] + ', CAT_STAGE1WS7=0', trees[0][1], 0, off))
    res = {name: [] for name, _, _, _ in runs}
    dumps = {}
    tmp = tempfile.mkdtemp(prefix='stage1ws7_bench_')
    for rnd in range(a.rounds):
        for name, path, on, what in runs:
            path = os.path.abspath(path)
            env = dict(os.environ, PYTHONPATH=path + os.pathsep + os.environ.get('PYTHONPATH', ''), CAT_STAGE1WS7=str(on))
            row = {}
            inner = ','.join(w for w in what.split(',') if w != 'bench')
            if inner:
                cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, HERE, '--child', '--on', str(on), '--what', inner, '--iters', str(a.iters),
                       '--step-iters', str(a.step_iters)]
                p = subprocess.run(cmd, cwd=path, env=env, capture_output=True, text=True)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith('STAGE1WS7 ')]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit('stage1ws7_bench: child (%s, round %d) ended with %d: stopping' % (name, rnd, p.returncode))
                row.update(json.loads(line[0][10:]))
            if 'bench' in what.split(','):
                ddir = os.path.join(tmp, '%s_%d' % (name.replace(' ', '_').replace(',', '').replace('=', ''), rnd))
                cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup',
                       str(a.bench_warmup), '--dump-outputs', ddir]
                p = subprocess.run(cmd, cwd=path, env=env, capture_output=True, text=True)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit('stage1ws7_bench: bench.py (%s, round %d) ended with %d: stopping' % (name, rnd, p.returncode))
                row['bench_ms'] = json.loads(line[-1])['ms_per_step']
                dumps.setdefault(name, ddir)
            res[name].append(row)
            print('round %d  %-26s %s' % (rnd, name, json.dumps(row)), flush=True)
    lines = table(res, a.rounds, a.what)
    if len(dumps) > 1:
        names = list(dumps)
        for other in names[1:]:
            files = sorted(os.listdir(dumps[names[0]]))
            same = files == sorted(os.listdir(dumps[other])) and all(filecmp.cmp(os.path.join(dumps[names[0]], f), os.path.join(dumps[other], f), shallow=False)
                                                                     for f in files)
            lines.append('bench.py --dump-outputs, %s against %s: %d arrays, %s' % (names[0], other, len(files), 'bit-identical' if same else 'DIFFERENT'))
    print('\n'.join(lines))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


def table(res, rounds, what):
    """{run name: [one result row per round]} -> the lines of the table"""
    lines = ['kernel sizes [3, 5, 7], full-width blocks: stage 1 in one statistics-writing launch (CAT_STAGE1WS7) against one launch per kernel size;',
             'one process per (tree, round), trees alternating, median of %d rounds, spread = max - min; --what %s' % (rounds, what), '']
    keys = [('block_us', 'owned InstanceNorm block (8, 256, 64, 64) forward, us'),
            ('in_ms', 'InstanceNorm teacher forward (blocks owned), batch 8, 256 x 256, ms'),
            ('step_ms', 'graphed CycleGAN-style distillation step, kernel sizes 3 5 7, batch 8, ms'),
            ('wide_us', 'wide training block (8, 256, 64, 64) forward + backward, CAT_FUSED_WIDE=1, us'),
            ('bench_ms', 'bench.py default (kernel sizes 1 3 5), ms per step')]
    for key, title in keys:
        if not any(key in r for rs in res.values() for r in rs):
            continue
        lines.append(title)
        for name, rs in res.items():
            if not all(key in r for r in rs):
                lines.append('    %-26s not measured' % name)
                continue
            v = [r[key] for r in rs]
            extra = ''
            for flag, text in (('block_us', 'stage1_fused'), ('in_ms', 'in_fused'), ('wide_us', 'wide_fused')):
                if key == flag:
                    extra = '   on the fused pipeline: %s' % bool(rs[0][text])
            lines.append('    %-26s %s   median %.3f, spread %.3f%s' % (name, '  '.join('%.3f' % t for t in v), statistics.median(v), max(v) - min(v), extra))
    if any('block_families' in r for rs in res.values() for r in rs):
        lines += ['', 'stage 1 of that block, one profiled forward per round: launches, us (median, spread), share of the %.1f TFLOP/s fp32 MFMA peak'
                  % MFMA_F32_PEAK_TFLOPS]
        for name, rs in res.items():
            if not all('block_families' in r for r in rs):
                continue
            st = [_stage1(r['block_families']) for r in rs]
            us = [s[1] for s in st]
            med = statistics.median(us)
            lines.append('    %-26s %d launch%s  %s   median %.1f us, spread %.1f;  %.2f GFLOP, %.1f %% of peak'
                         % (name, st[0][0], '' if st[0][0] == 1 else 'es', '  '.join('%.1f' % t for t in us), med, max(us) - min(us), st[0][2] / 1e9,
                            100.0 * st[0][2] / (med * 1e-6) / (MFMA_F32_PEAK_TFLOPS * 1e12)))
            lines.append('    %-26s families: %s' % ('', ', '.join('%s x%d' % (k, v[0]) for k, v in sorted(rs[0]['block_families'].items()))))
    return lines


if __name__ == '__main__':
    main()
