"""Step time and library-call count of the headline distillation step (bench.py's C2: pix2pix InceptionDistiller, 256 x 256, batch 16,
BatchNorm, student pruned to 4.6 GMACs) with one replica and with --virtual_replicas 4 (host.StepHost.set_virtual_replicas: BatchNorm
statistics per shard of 4 samples, four 4 x 4 KA terms summed).

ONE bounded child process builds the model once and alternates the two settings over --repeats rounds: per round and setting 3 warm-up
steps, then HIP events around --steps eager steps on the stream (one synchronisation at the end).  Afterwards 2 steps per setting run under
the library's profiling hook, which counts the entry-point calls of libcat_hip per kernel family (as tools/spade_teacher_bench.py does).
Nothing is promised about the ratio: the tool reports it.

    python tools/virtual_replicas_bench.py [--repeats 3] [--steps 10] [--out profiles/virtual_replicas_bench.txt]"""
import argparse
import json
import os
import subprocess
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, BATCH, REPLICAS = 256, 16, (1, 4)


def child(a):
    import ctypes as C

    import torch
    import bench
    from cat_amd import _lib, synthetic
    model, _ = bench.build_model(Namespace(workload='c2', target_flops=4.6e9, size=SIZE), 0)
    batches = [{'A': synthetic.images((BATCH, 3, SIZE, SIZE), 1000 + 10 * i).cuda(), 'B': synthetic.images((BATCH, 3, SIZE, SIZE), 2000 + 10 * i).cuda(),
                'A_paths': [], 'B_paths': []} for i in range(4)]

    def step(i):
        model.set_input(batches[i % 4])
        model.optimize_parameters(i)

    ms = {s: [] for s in REPLICAS}
    for _ in range(a.repeats):
        for s in REPLICAS:
            model.set_virtual_replicas(s)
            for i in range(3):
                step(i)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(a.steps):
                step(3 + i)
            t1.record()
            torch.cuda.synchronize()
            ms[s].append(t0.elapsed_time(t1) / a.steps)
    lib = _lib.load()
    calls, nprof = {}, 2
    for s in REPLICAS:
        model.set_virtual_replicas(s)
        step(0)
        torch.cuda.synchronize()
        lib.cat_prof_enable(1)
        for i in range(nprof):
            step(i)
        torch.cuda.synchronize()
        n = lib.cat_prof_collect()
        lib.cat_prof_enable(0)
        fams, name = {}, C.create_string_buffer(64)
        cnt, tms, fl = C.c_int64(), C.c_double(), C.c_double()
        for i in range(n):
            lib.cat_prof_family(i, name, 64, C.byref(cnt), C.byref(tms), C.byref(fl))
            fams[name.value.decode()] = cnt.value / nprof
        calls[s] = fams
    losses = {k: float(v) for k, v in model.get_current_losses().items()}
    print('RESULT ' + json.dumps(dict(ms={str(s): v for s, v in ms.items()}, calls={str(s): v for s, v in calls.items()},
                                      finite=all(v == v and abs(v) < 1e30 for v in losses.values()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=None, help='append the report to this file as well')
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--repeats', str(a.repeats), '--steps', str(a.steps)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=480)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith('RESULT ')]
    if p.returncode != 0 or not line:
        sys.exit('child run failed (exit %d):\n%s' % (p.returncode, (p.stdout + p.stderr)[-3000:]))
    r = json.loads(line[0][7:])
    med = {}
    out = ['C2 distillation step, %d x %d, batch %d: %d rounds alternating S = 1 and S = 4 in one process, 3 warm-up + %d timed eager steps each' %
           (SIZE, SIZE, BATCH, a.repeats, a.steps), 'virtual replicas   ms/step (rounds)                 images/s   library calls/step']
    for s in REPLICAS:
        v = sorted(r['ms'][str(s)])
        med[s] = v[len(v) // 2]
        out.append('S = %-14d %8.2f (%s)   %8.1f   %18.1f' % (s, med[s], ' '.join('%.2f' % x for x in v), BATCH / med[s] * 1e3,
                                                              sum(r['calls'][str(s)].values())))
    c1, c4 = r['calls']['1'], r['calls']['4']
    out.append('S = 4 / S = 1 step time: %.3f' % (med[4] / med[1]))
    out.append('call families that differ (S = 1 -> S = 4): ' + ', '.join('%s %g -> %g' % (k, c1.get(k, 0), c4.get(k, 0))
                                                                            for k in sorted(set(c1) | set(c4)) if c1.get(k, 0) != c4.get(k, 0)))
    out.append(json.dumps(dict(tool='virtual_replicas_bench', image=[SIZE, SIZE], batch=BATCH, steps=a.steps, ms=r['ms'],
                               calls_per_step={s: sum(v.values()) for s, v in r['calls'].items()}, ratio=med[4] / med[1], finite=r['finite'])))
    print('\n'.join(out))
    if a.out:
        with open(a.out, 'a') as f:
            f.write('\n'.join(out) + '\n')


if __name__ == '__main__':
    main()
