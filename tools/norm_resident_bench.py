"""The one-launch norm kernels of small statistic groups (csrc/norm_resident.hip; CAT_NORM_RESIDENT / ops.set_norm_resident) against the three
launches of csrc/norm.hip: where a training step's norm calls fall, what one call costs either way, and what the steps gain.

    python tools/norm_resident_bench.py [--what hist,geom,default,steps] [--trees parent=/path/to/parent/checkout this=.] [--rounds 3]
                                        [--out profiles/norm_resident_bench.txt]

One measuring process per figure, started by this driver as a bounded child (its own time limit; a child that fails or runs out of time ends
the whole run: nothing more is started on the GPU).  A tree is name=path: a checkout with its library built; children of a tree run in it with
its package first on sys.path.  Trees alternate within a round, so a drift of the machine hits both alike; medians over the rounds with their
spread (max - min).

    hist     (last tree) one eager step each of the GauGAN distillation (bench.py --workload spade), the CycleGAN-style distillation (--workload c3)
             and the CycleGAN teacher (tools/cyclegan_teacher_bench.py, batch 4) with cat_amd._lib.call wrapped on the host: every cat_norm_fwd /
             cat_norm_bwd geometry (mode, N, HW, C, shards, affine) with its call count and cat_norm_launches off / on; the share of the calls
             inside the domain; the kernel launches of the step's norm calls either way
    geom     (last tree) every in-domain geometry of those histograms, forward and backward, switch off against on: us per call by HIP events
             around a replayed graph of --calls (100) calls on one set of buffers (the tensors stay cache-resident, as behind their producer)
    default  bench.py's default workload with --dump-outputs in every tree: the arrays compared byte for byte
    steps    per tree and round: bench.py --workload spade, bench.py --workload c3 (ms per step out of their JSON lines) and the graphed
             CycleGAN teacher step at batch 4 (tools/cyclegan_teacher_bench.py --only graph)
The last tree runs with CAT_NORM_RESIDENT=1 whatever its default; a tree without the switch ignores it."""
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
ROOT = os.path.dirname(os.path.dirname(HERE))
MODES = {0: 'instance', 1: 'batch'}


# ------------------------------------------------------------------------------------------------ children
def _trace(run):
    """{(entry, mode, N, HW, C, cs, shards, affine, params, act): calls} of one run(), by wrapping cat_amd._lib.call on the host"""
    from cat_amd import _lib
    seen, real = {}, _lib.call

    def call(name, *args):
        if name in ('cat_norm_fwd', 'cat_norm_bwd'):
            g = args[0]._obj
            params = name == 'cat_norm_bwd' and (args[8] is not None or args[9] is not None)
            key = (name, g.mode, g.N, g.HW, g.C, g.cs, g.shards, args[2 if name == 'cat_norm_fwd' else 3] is not None, params, g.act)
            seen[key] = seen.get(key, 0) + 1
        return real(name, *args)
    _lib.call = call
    try:
        run()
    finally:
        _lib.call = real
    return seen


def _steps(which):
    """an eager step function of the workload, warmed up"""
    import random
    import torch
    sys.path.insert(0, os.getcwd())
    if which == 'cycle':
        sys.path.insert(0, os.path.join(os.getcwd(), 'tools'))
        import cyclegan_teacher_bench as cb
        from cat_amd import synthetic
        random.seed(233)
        m = cb.build(500)
        batch = {'A': synthetic.images((4, 3, 256, 256), 3000).cuda(), 'B': synthetic.images((4, 3, 256, 256), 4000).cuda()}
    else:
        import bench
        spade = which == 'spade'
        args = argparse.Namespace(workload=which, size=256, batch=4 if spade else 8, target_flops=5.6e9 if spade else 2.6e9)
        m, _ = (bench.build_spade_model if spade else bench.build_model)(args, 0)
        if spade:
            batch = bench.spade_batches(args, 0, 1)[0]
        else:
            from cat_amd import synthetic
            batch = {'A': synthetic.images((8, 3, 256, 256), 1000).cuda(), 'B': synthetic.images((8, 3, 256, 256), 2000).cuda(), 'A_paths': [], 'B_paths': []}

    def step(i):
        m.set_input(batch)
        m.optimize_parameters(i)
    for i in range(2):
        step(i)
    torch.cuda.synchronize()
    return step


def child_hist(a):
    import torch
    from cat_amd import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    step = _steps(a.workload)
    seen = _trace(lambda: step(2))
    torch.cuda.synchronize()
    rows = []
    for key, calls in sorted(seen.items()):
        name, mode, n, hw, c, cs, shards, affine, params, act = key
        g = _lib.NormGeom(n, hw, c, cs, mode, 1e-5, 0.1, act, 0.2, shards)
        bwd = int(name == 'cat_norm_bwd')
        launches = []
        for on in (0, 1):
            prev = lib.cat_norm_set_resident(on)
            launches.append(lib.cat_norm_launches(C.byref(g), bwd, int(params)))
            lib.cat_norm_set_resident(prev)
        rows.append(dict(entry=name, mode=MODES[mode], N=n, HW=hw, C=c, cs=cs, shards=shards, affine=affine, params=params, act=act, calls=calls,
                         off=launches[0], on=launches[1]))
    print('NORMRES ' + json.dumps(dict(workload=a.workload, rows=rows)), flush=True)


def child_geom(a):
    """us per call, off and on, of the geometries in the JSON file a.geoms"""
    import torch
    from cat_amd import _lib
    lib = _lib.load()
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    out = []
    for row in json.load(open(a.geoms)):
        n, hw, c, cs, mode = row['N'], row['HW'], row['C'], row['cs'], {v: k for k, v in MODES.items()}[row['mode']]
        g = _lib.NormGeom(n, hw, c, cs, mode, 1e-5, 0.1, row['act'], 0.2, row['shards'])
        gen = torch.Generator(device=dev).manual_seed(7)
        x, dy = (torch.randn(n, hw, cs, device=dev, generator=gen) for _ in range(2))
        y, dx = torch.empty_like(x), torch.empty_like(x)
        groups = n if mode == 0 else max(1, min(row['shards'], n))
        mean, rstd = torch.empty(groups, c, device=dev), torch.empty(groups, c, device=dev)
        ga, be = (torch.ones(c, device=dev), torch.zeros(c, device=dev)) if row['affine'] else (None, None)
        dga, dbe = (torch.empty(c, device=dev), torch.empty(c, device=dev)) if row['params'] else (None, None)
        ws = torch.empty(lib.cat_norm_ws_bytes(C.byref(g)) // 4, device=dev)

        def fwd():
            _lib.call('cat_norm_fwd', C.byref(g), p(x), p(ga), p(be), p(y), p(mean), p(rstd), None, None, None, p(ws),
                      C.c_void_p(torch.cuda.current_stream().cuda_stream))

        def bwd():
            _lib.call('cat_norm_bwd', C.byref(g), p(x), p(dy), p(ga), p(be), p(mean), p(rstd), p(dx), p(dga), p(dbe), 0, p(ws),
                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
        res = dict(row)
        for on in (0, 1):
            prev = lib.cat_norm_set_resident(on)
            fwd()
            torch.cuda.synchronize()
            for tag, fn in (('fwd', fwd), ('bwd', bwd)):
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    for _ in range(a.calls):
                        fn()
                graph.replay()
                torch.cuda.synchronize()
                ts = []
                for _ in range(5):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    graph.replay()
                    t1.record()
                    t1.synchronize()
                    ts.append(1e3 * t0.elapsed_time(t1) / a.calls)
                res['%s_%s_us' % (tag, 'on' if on else 'off')] = round(statistics.median(ts), 2)
                res['%s_%s_launches' % (tag, 'on' if on else 'off')] = lib.cat_norm_launches(C.byref(g), int(tag == 'bwd'), int(row['params']))
                del graph
            lib.cat_norm_set_resident(prev)
        out.append(res)
    print('NORMRES ' + json.dumps(out), flush=True)


# ------------------------------------------------------------------------------------------------ driver
def _child(cmd, path, env, limit, prefix, what):
    p = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, cwd=path, env=env, capture_output=True, text=True)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith(prefix)]
    if p.returncode != 0 or not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit('norm_resident_bench: %s ended with %d: stopping' % (what, p.returncode))
    return json.loads(line[-1][len(prefix):].strip() if prefix != '{' else line[-1])


def _geom_name(r):
    return '%-8s N %-2d HW %-6d C %-4d%s%s' % (r['mode'], r['N'], r['HW'], r['C'], ' shards %d' % r['shards'] if r['shards'] > 1 else '',
                                             '' if r['affine'] else ' no affine')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trees', nargs='+', default=['this=' + ROOT])
    ap.add_argument('--what', default='hist,geom,default,steps')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--calls', type=int, default=100, help='geom: calls per replayed graph')
    ap.add_argument('--bench-steps', type=int, default=10, dest='bench_steps')
    ap.add_argument('--bench-warmup', type=int, default=3, dest='bench_warmup')
    ap.add_argument('--timeout', type=int, default=300, help='seconds per child')
    ap.add_argument('--out', default=None, help='the tables are appended to this file')
    ap.add_argument('--child', default=None, choices=['hist', 'geom'])
    ap.add_argument('--workload', default='spade')
    ap.add_argument('--geoms', default=None)
    a = ap.parse_args()
    if a.child:
        return {'hist': child_hist, 'geom': child_geom}[a.child](a)
    what = a.what.split(',')
    trees = [(t.split('=')[0], os.path.abspath(t.split('=')[1])) for t in a.trees]
    last = trees[-1][1]
    tmp = tempfile.mkdtemp(prefix='norm_resident_bench_')
    lines = []

    def say(*ls):
        for ln in ls:
            print(ln, flush=True)
            lines.append(ln)

    def env_of(path, name):
        env = dict(os.environ, PYTHONPATH=path + os.pathsep + os.environ.get('PYTHONPATH', ''))
        if (name, path) == trees[-1]:
            env['CAT_NORM_RESIDENT'] = '1'
        return env
    hist = {}
    if 'hist' in what or 'geom' in what:
        for wl, title in (('spade', 'GauGAN distillation step (bench.py --workload spade, batch 4, 256 x 512)'),
                          ('c3', 'CycleGAN-style distillation step (bench.py --workload c3, batch 8, 256 x 256)'),
                          ('cycle', 'CycleGAN teacher step (train.py --model cycle_gan, batch 4, 256 x 256)')):
            rows = _child([sys.executable, HERE, '--child', 'hist', '--workload', wl], last, env_of(last, trees[-1][0]), a.timeout, 'NORMRES ',
                          'hist ' + wl)['rows']
            hist[wl] = rows
            calls = sum(r['calls'] for r in rows)
            inside = sum(r['calls'] for r in rows if r['on'] < r['off'])
            off, on = sum(r['calls'] * r['off'] for r in rows), sum(r['calls'] * r['on'] for r in rows)
            say('', title + ': cat_norm_fwd / cat_norm_bwd calls of one eager step, by geometry (host-side trace of the library calls)',
                '    %-52s %-13s %5s  launches off -> on' % ('geometry', 'entry', 'calls'))
            for r in rows:
                say('    %-52s %-13s %5d  %d -> %d%s' % (_geom_name(r), r['entry'], r['calls'], r['off'], r['on'], '' if r['on'] < r['off'] else '   outside'))
            say('    %d calls, %d inside the domain (%.1f %%); kernel launches of the norm calls per step: %d -> %d (%d fewer)'
                % (calls, inside, 100.0 * inside / max(calls, 1), off, on, off - on))
    if 'geom' in what:
        uniq = {}
        for rows in hist.values():
            for r in rows:
                if r['on'] < r['off']:
                    key = (r['mode'], r['N'], r['HW'], r['C'], r['cs'], r['shards'], r['affine'], r['act'])
                    u = uniq.setdefault(key, dict(r, params=False, calls=0))
                    u['params'] = u['params'] or r['params']
                    u['calls'] += r['calls']
        gfile = os.path.join(tmp, 'geoms.json')
        json.dump(list(uniq.values()), open(gfile, 'w'))
        res = _child([sys.executable, HERE, '--child', 'geom', '--geoms', gfile, '--calls', str(a.calls)], last, env_of(last, trees[-1][0]), a.timeout,
                     'NORMRES ', 'geom')
        say('', 'in-domain geometries, us per call (median of 5 replays of a graph of %d calls), three launches -> one launch (launch counts in brackets)' % a.calls,
            '    %-52s %-26s %-26s' % ('geometry', 'forward', 'backward'))
        for r in sorted(res, key=lambda r: (r['mode'], r['HW'], r['C'], r['N'])):
            say('    %-52s %6.2f -> %6.2f [%d -> %d]   %6.2f -> %6.2f [%d -> %d]%s'
                % (_geom_name(r), r['fwd_off_us'], r['fwd_on_us'], r['fwd_off_launches'], r['fwd_on_launches'], r['bwd_off_us'], r['bwd_on_us'],
                   r['bwd_off_launches'], r['bwd_on_launches'],
                   '   SLOWER' if r['fwd_on_us'] > r['fwd_off_us'] and r['fwd_on_launches'] < r['fwd_off_launches']
                   or r['bwd_on_us'] > r['bwd_off_us'] and r['bwd_on_launches'] < r['bwd_off_launches'] else ''))
    bench = [sys.executable, 'bench.py', '--gpus', '1', '--steps', str(a.bench_steps), '--warmup', str(a.bench_warmup)]
    if 'default' in what:
        dumps = {}
        for name, path in trees:
            dumps[name] = os.path.join(tmp, 'dump_' + name)
            row = _child(bench + ['--dump-outputs', dumps[name]], path, env_of(path, name), a.timeout, '{', 'bench.py default, ' + name)
            say('bench.py default workload, %s: %.3f ms per step' % (name, row['ms_per_step']))
        names = list(dumps)
        for other in names[1:]:
            files = sorted(os.listdir(dumps[names[0]]))
            same = files == sorted(os.listdir(dumps[other])) and all(filecmp.cmp(os.path.join(dumps[names[0]], f), os.path.join(dumps[other], f), shallow=False)
                                                                     for f in files)
            say('bench.py --dump-outputs, %s against %s: %d arrays, %s' % (names[0], other, len(files), 'bit-identical' if same else 'DIFFERENT'))
    if 'steps' in what:
        res = {name: {'spade': [], 'c3': [], 'cycle': []} for name, _ in trees}
        for rnd in range(a.rounds):
            for name, path in trees:
                env = env_of(path, name)
                for wl in ('spade', 'c3'):
                    res[name][wl].append(_child(bench + ['--workload', wl], path, env, a.timeout, '{', 'bench.py %s, %s' % (wl, name))['ms_per_step'])
                row = _child([sys.executable, os.path.join('tools', 'cyclegan_teacher_bench.py'), '--batches', '4', '--only', 'graph', '--rounds', '1',
                              '--steps', str(a.bench_steps), '--out', os.path.join(tmp, 'cycle.txt')], path, env, a.timeout, '{', 'cycle, ' + name)
                res[name]['cycle'].append(row['graph']['median_ms'])
                print('round %d  %-8s %s' % (rnd, name, json.dumps({k: v[-1] for k, v in res[name].items()})), flush=True)
        say('', 'whole steps, ms per step (graph replay), one process per (tree, round), trees alternating, median of %d rounds, spread = max - min' % a.rounds)
        for wl, title in (('spade', 'bench.py --workload spade (GauGAN distillation, batch 4)'), ('c3', 'bench.py --workload c3 (batch 8)'),
                          ('cycle', 'CycleGAN teacher step, batch 4, graphed')):
            say(title)
            for name, _ in trees:
                v = res[name][wl]
                say('    %-8s %s   median %.3f, spread %.3f' % (name, '  '.join('%.3f' % t for t in v), statistics.median(v), max(v) - min(v)))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()
