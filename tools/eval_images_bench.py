"""One `evaluate_model` pass with the generated image set on the host (the reference's list of CPU float tensors: `eval_images = 'host'`)
and on the device (uint8, cat_amd.metric.DeviceImages: `eval_images = 'device'`).

A BatchNorm inception distiller (student ngf 16) at 256 x 256, batch 2, over a synthetic loader of `--images` images; InceptionV3 with seeded
weights (timing does not depend on the values) and a synthetic real set; the Frechet tail on the device for both (attach_fid(frechet='device')),
so that scipy's 2048 x 2048 square root, which is the same work either way, does not drown the part that differs.  This is host-bound code:
per mode the wall time of the pass, the time between two HIP events around it, and the same two for the metric call alone; the peak device
memory of the pass above what was allocated before it, and the process's peak resident set after it ('device' runs first: the resident-set
peak never falls).  The set's own sizes are printed from the shapes.

    python tools/eval_images_bench.py [--images 300] [--out profiles/eval_images_bench.txt]"""
import argparse
import json
import os
import resource
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H = W = 256
BATCH = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=300)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_images_bench.txt'))
    a = ap.parse_args()
    from cat_amd import _lib, metric, synthetic
    from cat_amd.distillers import create_distiller, evaluation as E
    _lib.load()
    torch.manual_seed(0)
    opt = synthetic.default_options(norm='batch', track=True, ndf=64, teacher_ngf=64, student_ngf=16)
    opt.log_dir, opt.eval_batch_size = tempfile.mkdtemp(prefix='eval_images_bench_'), 50
    model = create_distiller(opt, verbose=False)
    rs = np.random.RandomState(1)
    feats = rs.standard_normal((256, 2048))
    E.attach_fid(model, metric.InceptionV3([3]), npz={'mu': feats.mean(0), 'sigma': np.cov(feats, rowvar=False)}, frechet='device')
    distinct = [synthetic.images((BATCH, 3, H, W), 900 + i) for i in range(8)]
    n_batches = a.images // BATCH
    model.eval_dataloader = [{'A': distinct[i % 8], 'B': distinct[(i + 1) % 8], 'A_paths': ['/d/%d_%d.png' % (i, j) for j in range(BATCH)],
                             'B_paths': ['/d/%d_%d.png' % (i, j) for j in range(BATCH)]} for i in range(n_batches)]
    n = n_batches * BATCH
    timing = {}
    real_get_fid = metric.get_fid

    def timed_get_fid(*args, **kw):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        v = real_get_fid(*args, **kw)
        e1.record()
        torch.cuda.synchronize()
        timing['metric_wall_ms'], timing['metric_event_ms'] = (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)
        return v
    metric.get_fid = timed_get_fid

    def one_pass(mode, step):
        model.eval_images = mode
        model.best_fid, model.fids = 1e9, []
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fid = model.evaluate_model(step)['metric/fid']
        e1.record()
        torch.cuda.synchronize()
        return dict(mode=mode, fid=fid, wall_ms=(time.perf_counter() - t0) * 1e3, event_ms=e0.elapsed_time(e1), metric_wall_ms=timing['metric_wall_ms'],
                    metric_event_ms=timing['metric_event_ms'], peak_device_mib=(torch.cuda.max_memory_allocated() - base) / 2 ** 20,
                    peak_rss_mib=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024)
    one_pass('device', 0)                                  # warm-up: plans, the frozen student's fold, the real set's root
    rows = [one_pass('device', 1), one_pass('host', 2), one_pass('device', 3), one_pass('host', 4)]
    px = n * H * W
    sizes = dict(device_uint8_set_mib=px * 4 / 2 ** 20, host_float32_list_mib=px * 12 / 2 ** 20, host_float32_concat_mib=px * 12 / 2 ** 20,
                 host_uint8_mib=px * 3 / 2 ** 20, host_float64_mib=px * 24 / 2 ** 20)
    lines = ['eval_images_bench: %d images %d x %d, batch %d, BatchNorm student ngf 16, FID batch %d, Frechet tail on the device' % (n, H, W, BATCH, opt.eval_batch_size),
             'mode    pass wall ms  pass event ms  metric wall ms  metric event ms  peak device MiB  peak RSS MiB  fid']
    for r in rows:
        lines.append('%-6s  %12.1f  %13.1f  %14.1f  %15.1f  %15.1f  %12.1f  %.6f' % (r['mode'], r['wall_ms'], r['event_ms'], r['metric_wall_ms'],
                                                                                      r['metric_event_ms'], r['peak_device_mib'], r['peak_rss_mib'], r['fid']))
    lines.append('image set, from the shapes: device uint8 [n, H, W, 4] %.1f MiB; host path: list of float32 batches %.1f MiB + their concatenation %.1f MiB '
                 '+ uint8 %.1f MiB + float64 %.1f MiB' % (sizes['device_uint8_set_mib'], sizes['host_float32_list_mib'], sizes['host_float32_concat_mib'],
                                                          sizes['host_uint8_mib'], sizes['host_float64_mib']))
    lines.append(json.dumps(dict(tool='eval_images_bench', images=n, rows=rows, sizes=sizes)))
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
