"""ms per step of the CycleGAN teacher step (`train.py --model cycle_gan`), launched eagerly against replayed as one captured graph
(cat_amd.graph.GraphedStep; the image pools are fed through ImagePool.stage).

The networks carry the flags of the reference's scripts/cycle_gan/*/train_inception_teacher.sh (inception_9blocks, --norm_affine,
--norm_affine_D, --channels_reduction_factor 6, --kernel_sizes 1 3 5; ngf 64, ndf 64, InstanceNorm, lsgan, lambda_identity 0.5) with seeded
weights and `random.seed`; 256 x 256 images, --pool_size 50, per-GPU batch 1 and 4 (the script's 32 images over 8 GPUs).  Both models first run
until both pools are full and swapping; then `--rounds` alternating rounds of `--steps` steps each, timed by HIP events; the median round is
the figure.  One JSON line per batch size, printed and written to --out (appended with --append).

    python tools/cyclegan_teacher_bench.py [--batches 1 4] [--steps 10] [--rounds 3] [--only eager|graph] [--label TEXT] [--out FILE] [--append]

`--only eager` touches nothing but create_model / set_input / optimize_parameters: it measures any revision of the package.
The generators' 256-channel blocks take the fused block path with CAT_FUSED_WIDE=1 in the environment (off by default; the comparison:
profiles/wide_block_bench.txt)."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

POOL_SIZE, SIZE = 50, 256


def build(seed):
    from cat_amd import synthetic
    from cat_amd.models import create_model
    opt = synthetic.default_options(norm='instance', model='cycle_gan', dataset_mode='unaligned', netG='inception_9blocks', ngf=64, ndf=64,
                                    gan_mode='lsgan', dropout_rate=0, direction='AtoB', lambda_A=10.0, lambda_B=10.0, lambda_identity=0.5,
                                    pool_size=POOL_SIZE)
    torch.manual_seed(233)
    m = create_model(opt, verbose=False)
    for k, name in enumerate(m.model_names):
        net = getattr(m, 'net' + name)
        net.load_state_dict(synthetic.fill_state_dict(net.state_dict(), seed + k))
    m.setup(opt, verbose=False)
    return m


def timed(run, steps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(steps):
        run(i)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / steps


def measure(batch, modes, steps, rounds):
    from cat_amd import synthetic
    batches = [{'A': synthetic.images((batch, 3, SIZE, SIZE), 3000 + 10 * i).cuda(), 'B': synthetic.images((batch, 3, SIZE, SIZE), 4000 + 10 * i).cuda()}
               for i in range(4)]
    runs, models = {}, {}
    for mode in modes:
        m = models[mode] = build(500)
        if mode == 'graph':
            from cat_amd.graph import GraphedStep
            step = GraphedStep(m, batches[0])
            runs[mode] = lambda i, step=step: step(batches[i % 4])
        else:
            def eager(i, m=m):
                m.set_input(batches[i % 4])
                m.optimize_parameters(i)
            runs[mode] = eager
    fill = -(-POOL_SIZE // batch) + 5      # both pools full, the last steps already draw
    for mode in modes:
        for i in range(fill):
            runs[mode](i)
    torch.cuda.synchronize()
    times = {mode: [] for mode in modes}
    for _ in range(rounds):
        for mode in modes:
            times[mode].append(timed(runs[mode], steps))
    row = {'batch': batch, 'size': SIZE, 'pool_size': POOL_SIZE, 'steps': steps}
    for mode in modes:
        m = models[mode]
        losses = m.get_current_losses()
        assert len(losses) == 8 and all(v == v for v in losses.values()), (mode, losses)
        row[mode] = {'ms_per_step': [round(t, 3) for t in times[mode]], 'median_ms': round(statistics.median(times[mode]), 3)}
        pools = [m.fake_A_pool, m.fake_B_pool]
        if all(hasattr(p, 'decide') for p in pools):      # (an older revision keeps a list and has no codes to count)
            assert all(p.num_imgs == POOL_SIZE and p.images is None for p in pools), mode
    if len(modes) == 2:
        row['graph_over_eager'] = round(row['graph']['median_ms'] / row['eager']['median_ms'], 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--only', default=None, choices=['eager', 'graph'])
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cyclegan_graph_bench.txt'))
    ap.add_argument('--append', action='store_true')
    args = ap.parse_args()
    from cat_amd import _lib
    _lib.load()
    torch.cuda.set_device(0)
    modes = [args.only] if args.only else ['eager', 'graph']
    lines = []
    for batch in args.batches:
        random.seed(233)
        row = measure(batch, modes, args.steps, args.rounds)
        if args.label:
            row = dict(label=args.label, **row)
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    with open(args.out, 'a' if args.append else 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
