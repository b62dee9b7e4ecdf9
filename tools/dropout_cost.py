"""Cost of dropout on the C2 distillation step (bench.py's workload: canonical teacher, student pruned to 4.6e9 MACs, batch 16, 256 x 256).

Two models are built with bench.py's own builder: one as bench.py builds it, one whose TEACHER is built with --teacher_dropout_rate 0.1 --
shrink deep-copies the teacher, so that rate reaches every block of the pruned student (the reference's behaviour).  Both steps are replayed
as captured graphs, alternating in rounds, and the per-step times are printed as one JSON line.

    python tools/dropout_cost.py [--steps 20] [--rounds 3] [--only base|dropout]"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(rate):
    import bench
    from cat_amd import synthetic
    orig = synthetic.default_options
    synthetic.default_options = lambda **kw: orig(teacher_dropout_rate=rate, **kw)
    try:
        args = types.SimpleNamespace(workload='c2', target_flops=4.6e9, size=256, batch=16)
        model, opt = bench.build_model(args, 0)
    finally:
        synthetic.default_options = orig
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--rate', type=float, default=0.1)
    ap.add_argument('--only', default=None, choices=['base', 'dropout'])
    args = ap.parse_args()
    from cat_amd import _lib, rng, synthetic
    from cat_amd import nn as cnn
    from cat_amd.graph import GraphedStep
    from cat_amd.inception_modules import InvertedResidualChannels
    _lib.load()
    torch.cuda.set_device(0)
    batches = [{'A': synthetic.images((16, 3, 256, 256), 1000 + 10 * i).cuda(), 'B': synthetic.images((16, 3, 256, 256), 2000 + 10 * i).cuda(),
                'A_paths': [], 'B_paths': []} for i in range(4)]
    names = [args.only] if args.only else ['base', 'dropout']
    models, steps, info = {}, {}, {}
    for name in names:
        m = build(args.rate if name == 'dropout' else 0.0)
        blocks = [b for b in m.netG_student.modules() if isinstance(b, InvertedResidualChannels)]
        drops = [d for b in blocks for d in b.modules() if isinstance(d, cnn.Dropout)]
        info[name] = dict(student_blocks=len(blocks), student_dropout_rates=sorted({float(d.p) for d in drops}),
                          teacher_dropout_rates=sorted({float(b.dropout_rate) for b in m.netG_teacher.modules() if isinstance(b, InvertedResidualChannels)}))
        models[name], steps[name] = m, GraphedStep(m, batches[0])
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for r in range(args.rounds):
        for name in names:
            for i in range(3):
                steps[name](batches[i % 4])
            torch.cuda.synchronize()
            c0 = rng.get_state()[1] if name == 'dropout' else None
            t0 = time.perf_counter()
            for i in range(args.steps):
                steps[name](batches[i % 4])
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
            if c0 is not None:
                info[name]['draws_per_step'] = (rng.get_state()[1] - c0) / args.steps
    for name in names:
        losses = models[name].get_current_losses()
        assert all(v == v for v in losses.values()), (name, losses)
    out = {n: dict(info[n], ms_per_step=[round(t, 3) for t in times[n]], best_ms=round(min(times[n]), 3),
                   images_per_s=round(16e3 / min(times[n]), 2)) for n in names}
    if len(names) == 2:
        out['overhead_pct'] = round(100.0 * (out['dropout']['best_ms'] / out['base']['best_ms'] - 1.0), 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
