"""The frozen teachers of a distillation with the reference's default kernel sizes [3, 5, 7] on their fused paths (frozen.set_k7 /
CAT_FROZEN_K7 for the BatchNorm-folded teacher, cat_amd/frozen.py; the InstanceNorm teacher of cat_amd/frozen_in.py) against the launches
they issued before.

One measuring process per (tree, round), started by this driver as a bounded child (its own time limit; a child that fails or runs out of
time ends the whole run: nothing more is started on the GPU).  Trees alternate within a round, so a drift of the machine hits both alike:

    python tools/k7_teacher_bench.py [--trees this=. parent=/path/to/parent/checkout] [--what block,bn,in,step,bench] [--rounds 3]
                                     [--out profiles/k7_teacher_bench.txt]

A tree is name=path[=what]: a checkout with its library built.  The child runs THIS file with the tree's package first on sys.path.  A tree
without frozen.set_k7 (the parent commit) runs every [3, 5, 7] teacher block the way `this` does with the switch off; the first tree is also
measured with CAT_FROZEN_K7=0 (--off-what).  Per child, by HIP events unless said otherwise:
    block   one eval-mode BatchNorm block, 256 inputs, 42-wide branches, kernel sizes [3, 5, 7], reflect, at (16, 256, 64, 64) under no_grad:
            us per forward, and per launch family of the library's profiler (one profiled forward): stage 1, the depthwise stage, the tail
    bn      the [3, 5, 7] BatchNorm teacher (inception_9blocks, ngf 64) forward alone, batch 16, 256 x 256: ms
    in      the [3, 5, 7] InstanceNorm teacher forward, its blocks owned (frozen_in.own_network), batch 8, 256 x 256: ms
    step    the graphed pix2pix distillation step of tools/k7_block_bench.py (kernel sizes [3, 5, 7], batch 16, 256 x 256): ms per replay
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
TAIL = ('conv_tconv7_multi', 'conv_tconv_multi')      # the block's last launch: the K-concatenated LDS-tile sum (else the wide tile, conv_ksum)


def _families(fn):
    """{family: [launches, ms]} of one call of fn, by the library's profiler"""
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
        out[name.value.decode()] = [cnt.value, ms.value]
    return out


def _teacher(norm, dev):
    from cat_amd import networks, synthetic
    opt = synthetic.default_options(norm=norm, track=norm == 'batch', kernel_sizes=list(KS))
    net = networks.define_G(3, 3, 64, 'inception_9blocks', opt.norm, 0, 'normal', 0.02, [], opt=opt)
    net.load_state_dict(synthetic.fill_state_dict(net.state_dict(), synthetic.SEED_TEACHER, gamma_abs_normal=True))
    return net.to(dev).eval()


def child(a):
    import torch
    from k7_block_bench import _distiller, _time
    from cat_amd import _lib, frozen, frozen_in, nn as cnn, ops, synthetic
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    _lib.load()
    dev = torch.device('cuda:0')
    has_k7 = hasattr(frozen, 'set_k7')
    if has_k7:
        frozen.set_k7(bool(a.k7))
    out = {'has_k7': has_k7, 'k7': bool(a.k7) and has_k7}
    with torch.no_grad():
        if 'block' in a.what:
            blk = InvertedResidualChannels(256, [42] * 3, [42] * 3, 1, list(KS), list(KS), padding_type='reflect', use_bias=False,
                                           norm_layer=cnn.BatchNorm2d, norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
            blk.load_state_dict(synthetic.fill_state_dict(blk.state_dict(), 77, gamma_abs_normal=True))
            blk = blk.to(dev).eval()
            x = ops.to_nhwc(synthetic.normal((16, 256, 64, 64), 5).to(dev))
            out['block_us'] = 1e3 * _time(lambda: blk(x), 3, a.iters)
            out['block_families'] = _families(lambda: blk(x))
            del blk, x
            torch.cuda.empty_cache()
        if 'bn' in a.what:
            net = _teacher('batch', dev)
            x = ops.to_nhwc(synthetic.images((16, 3, 256, 256), 1000).to(dev))
            out['bn_ms'] = _time(lambda: net(x), 3, a.iters)
            del net, x
            torch.cuda.empty_cache()
        if 'in' in a.what:
            net = _teacher('instance', dev)
            out['in_owned'] = len(frozen_in.own_network(net))
            x = ops.to_nhwc(synthetic.images((8, 3, 256, 256), 1000).to(dev))
            out['in_fused'] = bool(frozen_in.applicable(net.features[0], net.down_sampling(x)))
            out['in_ms'] = _time(lambda: net(x), 3, a.iters)
            del net, x
            torch.cuda.empty_cache()
    if 'step' in a.what:
        from cat_amd.graph import GraphedStep
        model = _distiller(dev)
        batches = [{'A': synthetic.images((16, 3, 256, 256), 1000 + 10 * i).cuda(), 'B': synthetic.images((16, 3, 256, 256), 2000 + 10 * i).cuda(),
                    'A_paths': [], 'B_paths': []} for i in range(2)]
        step = GraphedStep(model, batches[0])
        i = [0]

        def replay():
            i[0] += 1
            step(batches[i[0] & 1])
        out['step_ms'] = _time(replay, 3, a.step_iters)
    print('K7TEACHER ' + json.dumps(out), flush=True)


def _stages(fam):
    """(stage 1, depthwise stage, tail) of one block forward as (launches, us): the tail is the K-concatenated launch, the depthwise stage the
    dwconv family, stage 1 everything else the block launched (with the switch off: the 1 x 1 GEMM, family conv_ksum, and the three first convs)"""
    pick = lambda keys: (sum(fam[k][0] for k in keys), 1e3 * sum(fam[k][1] for k in keys))
    tail = [k for k in fam if k in TAIL] or [k for k in fam if k == 'conv_ksum']
    dw = [k for k in fam if k.startswith('dwconv')]
    return pick([k for k in fam if k not in tail and k not in dw]), pick(dw), pick(tail)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trees', nargs='+', default=['this=' + os.path.dirname(os.path.dirname(HERE))])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--what', default='block,bn,in,step')
    ap.add_argument('--off-what', default='block,bn', dest='off_what', help='what the first tree also measures with CAT_FROZEN_K7=0')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--step-iters', type=int, default=10, dest='step_iters')
    ap.add_argument('--bench-steps', type=int, default=10, dest='bench_steps')
    ap.add_argument('--bench-warmup', type=int, default=3, dest='bench_warmup')
    ap.add_argument('--timeout', type=int, default=300, help='seconds per child')
    ap.add_argument('--out', default=None, help='the table is appended to this file')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--k7', type=int, default=1)
    a = ap.parse_args()
    if a.child:
        return child(a)
    trees = [(t.split('=') + [a.what])[:3] for t in a.trees]
    runs = [(name, path, 1, what) for name, path, what in trees]
    off = ','.join(w for w in a.off_what.split(',') if w in trees[0][2].split(','))
    if off:
        runs.insert(1, (trees[0][0] + ', CAT_FROZEN_K7=0', trees[0][1], 0, off))
    res = {name: [] for name, _, _, _ in runs}
    dumps = {}
    tmp = tempfile.mkdtemp(prefix='k7_teacher_bench_')
    for rnd in range(a.rounds):
        for name, path, k7, what in runs:
            path = os.path.abspath(path)
            env = dict(os.environ, PYTHONPATH=path + os.pathsep + os.environ.get('PYTHONPATH', ''), CAT_FROZEN_K7=str(k7))
            row = {}
            inner = ','.join(w for w in what.split(',') if w != 'bench')
            if inner:
                cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, HERE, '--child', '--k7', str(k7), '--what', inner, '--iters', str(a.iters),
                       '--step-iters', str(a.step_iters)]
                p = subprocess.run(cmd, cwd=path, env=env, capture_output=True, text=True)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith('K7TEACHER ')]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit('k7_teacher_bench: child (%s, round %d) ended with %d: stopping' % (name, rnd, p.returncode))
                row.update(json.loads(line[0][10:]))
            if 'bench' in what.split(','):
                ddir = os.path.join(tmp, '%s_%d' % (name.replace(' ', '_').replace(',', '').replace('=', ''), rnd))
                cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup',
                       str(a.bench_warmup), '--dump-outputs', ddir]
                p = subprocess.run(cmd, cwd=path, env=env, capture_output=True, text=True)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    raise SystemExit('k7_teacher_bench: bench.py (%s, round %d) ended with %d: stopping' % (name, rnd, p.returncode))
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
    lines = ['kernel sizes [3, 5, 7]: the frozen teachers on their fused paths (CAT_FROZEN_K7) against the launches they issued before;',
             'one process per (tree, round), trees alternating, median of %d rounds, spread = max - min; --what %s' % (rounds, what), '']
    keys = [('block_us', 'BatchNorm block (16, 256, 64, 64) forward, us'), ('bn_ms', 'BatchNorm teacher forward, batch 16, 256 x 256, ms'),
            ('in_ms', 'InstanceNorm teacher forward (blocks owned), batch 8, 256 x 256, ms'),
            ('step_ms', 'graphed pix2pix distillation step, kernel sizes 3 5 7, batch 16, ms'),
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
            if key == 'in_ms':
                extra = '   first block on the fused pipeline: %s' % bool(rs[0]['in_fused'])
            lines.append('    %-26s %s   median %.3f, spread %.3f%s' % (name, '  '.join('%.3f' % t for t in v), statistics.median(v), max(v) - min(v), extra))
    if any('block_families' in r for rs in res.values() for r in rs):
        lines += ['', 'the block per stage, one profiled forward per round: launches, us (median over the rounds)']
        for name, rs in res.items():
            if not all('block_families' in r for r in rs):
                continue
            st = [_stages(r['block_families']) for r in rs]
            cell = lambda i: '%d launch%s %.1f us' % (st[0][i][0], '' if st[0][i][0] == 1 else 'es', statistics.median(s[i][1] for s in st))
            lines.append('    %-26s stage 1: %s;  depthwise stage: %s;  tail: %s' % (name, cell(0), cell(1), cell(2)))
            lines.append('    %-26s families: %s' % ('', ', '.join('%s x%d' % (k, v[0]) for k, v in sorted(rs[0]['block_families'].items()))))
    return lines


if __name__ == '__main__':
    main()
