"""Inference time of a compressed student through cat_amd.infer.StudentRunner, at 256 x 256 and batch 1, 2 and 16.

The student is a checkpoint (`--checkpoint student.pth --norm instance|batch`, loaded by cat_amd.pretrained through a holder object) or, by
default, a seeded one: the canonical teacher of cat_amd.synthetic pruned to the launch scripts' budget (InstanceNorm: 2.6e9, the CycleGAN
students; BatchNorm: 4.6e9, the pix2pix students) with seeded weights.  Per batch size, ms per batch by HIP events (warm-up, then --iters calls,
one synchronise), the modes alternating over --repeats rounds, median [min, max]:

    general       eval() + no_grad with no runner and the block fast paths off: the per-layer launches (for the InstanceNorm student this is
                  exactly what evaluate_model issues, today and at the parent commit)
    fast          StudentRunner(min_tiles=None): InstanceNorm blocks on the fused pipeline, BatchNorm blocks on the frozen fold, where the
                  package's LDS-tile threshold admits the plane (96 output tiles; a 64 x 64 plane has 32 per sample)
    fast, tiles 1 the same with min_tiles=1, the runner's default: the threshold lifted for the runner's own fused InstanceNorm blocks (the
                  stem / head layers and the BatchNorm fold keep the package's: for the BatchNorm student these rows repeat the plain ones)
    graph         StudentRunner(graph=True, min_tiles=None)  graph, tiles 1: StudentRunner(graph=True, min_tiles=1)

    python tools/student_infer_bench.py [--norm instance batch] [--checkpoint PATH] [--out profiles/student_infer_bench.txt]"""
import argparse
import copy
import os
import statistics
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, BATCHES = 256, (1, 2, 16)


def seeded_student(norm, dev):
    import torch
    from cat_amd import networks, prune, synthetic
    track = norm == 'batch'
    opt = synthetic.default_options(norm=norm, track=track, target_flops=4.6e9 if track else 2.6e9, gpu_ids=[])
    T = networks.define_G(3, 3, 64, 'inception_9blocks', norm, 0, 'normal', 0.02, [], opt=opt)
    T.load_state_dict(synthetic.fill_state_dict(T.state_dict(), synthetic.SEED_TEACHER, gamma_abs_normal=True))
    T.eval()
    thr, _ = prune.search_threshold(T, opt.target_flops, opt)
    S = copy.deepcopy(T)
    prune._apply_structure(S, T, thr, opt, copy_weights=True)
    sd = synthetic.fill_state_dict(S.state_dict(), 21)
    sd['up_sampling.7.weight'] = sd['up_sampling.7.weight'] / 64      # keeps the closing tanh out of saturation (timing does not care)
    S.load_state_dict(sd)
    prune.model_profiling(S, SIZE, SIZE)
    return S.to(dev).eval()


def checkpoint_student(path, norm, dev):
    import torch
    from cat_amd import networks, pretrained, synthetic
    opt = synthetic.default_options(norm=norm, track=norm == 'batch', gpu_ids=[], data_height=SIZE, data_width=SIZE)
    opt.pretrained_student_G_path = path
    T = networks.define_G(3, 3, 64, 'inception_9blocks', norm, 0, 'normal', 0.02, [], opt=opt).eval()
    holder = Namespace(netG_teacher=T, netAs=[], device=dev, isTrain=False, optimizer_D=None, remove_mapping_hook=lambda: None,
                       add_mapping_hook=lambda: None)
    pretrained.load_pretrained_student(holder, opt)
    return holder.netG_student.eval()


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


def bench_student(S, norm, a, say):
    import torch
    from cat_amd import ops, synthetic
    from cat_amd.infer import StudentRunner
    from cat_amd.inception_modules import InvertedResidualChannels
    blocks = [m for m in S.modules() if isinstance(m, InvertedResidualChannels)]
    ops.set_branch_streams(False)
    for n in BATCHES:
        x = ops.to_nhwc(synthetic.images((n, 3, SIZE, SIZE), 970 + n).cuda())

        def general():
            for b in blocks:
                b._cat_frozen_off = True
            try:
                with torch.no_grad():
                    return S(x)
            finally:
                for b in blocks:
                    del b._cat_frozen_off

        runners = {'fast': StudentRunner(S, x, min_tiles=None), 'fast, tiles 1': StudentRunner(S, x, min_tiles=1),
                   'graph': StudentRunner(S, x, graph=True, min_tiles=None), 'graph, tiles 1': StudentRunner(S, x, graph=True, min_tiles=1)}
        if norm == 'batch':        # nothing of a BatchNorm student reads the runner's threshold
            for k in ('fast, tiles 1', 'graph, tiles 1'):
                runners.pop(k).release()
        for r in runners.values():
            r.release()            # each mode owns the blocks only while it is timed
        y_ref = general().clone()
        times = {k: [] for k in ['general'] + list(runners)}
        err = {}
        for rep in range(a.repeats):
            times['general'].append(_time(general, a.warmup, a.iters))
            for k, r in runners.items():
                r.own()
                times[k].append(_time(lambda: r(x), a.warmup, a.iters))
                err[k] = float((r(x) - y_ref).abs().max() / y_ref.abs().max())
                r.release()
        base = statistics.median(times['general'])
        for k, v in times.items():
            med = statistics.median(v)
            say('%-9s batch %2d  %-15s %8.3f ms/batch [%7.3f, %7.3f]  %7.3f ms/img  x%5.2f vs general%s' % (
                norm, n, k, med, min(v), max(v), med / n, base / med, '' if k == 'general' else '  max rel diff vs general %.1e' % err[k]))
        del runners
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--norm', nargs='+', default=['instance', 'batch'], choices=['instance', 'batch'])
    ap.add_argument('--checkpoint', default=None)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'student_infer_bench.txt'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('student_infer_bench: needs an MI355X (a time measured without the GPU says nothing)')
    dev = torch.device('cuda:0')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    say('student inference, %d x %d, ms per batch by HIP events: median [min, max] of %d rounds x %d calls, modes alternating' % (
        SIZE, SIZE, a.repeats, a.iters))
    for norm in a.norm:
        S = checkpoint_student(a.checkpoint, norm, dev) if a.checkpoint else seeded_student(norm, dev)
        say('%s student: n_macs %d, %d parameters%s' % (norm, S.n_macs, sum(p.numel() for p in S.parameters()),
                                                     ' (%s)' % a.checkpoint if a.checkpoint else ' (seeded: canonical teacher pruned)'))
        bench_student(S, norm, a, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
