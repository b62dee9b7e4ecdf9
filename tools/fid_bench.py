"""Cost of one FID evaluation tail -- everything after the InceptionV3 features -- on the host and on the device, on one GPU machine.

Seeded features (tests/fid_numpy.features; 2000 real ones give the real set's mu and sigma, computed once outside the clocks):
  * `host`    np.mean + np.cov of the fake features + calculate_frechet_distance (numpy + scipy.linalg.sqrtm), as get_fid runs it, on the CPUs
              this process may use: seconds, one run per shape;
  * `device`  frechet_distance_from_features on features resident on the device, HIP events around the whole tail: with a cold cache (sigma1
              uploaded, its trace and -- full form -- its root computed) and with the cache a second evaluation finds; steps of the iteration;
  * `gemm`    cat_gemm_f64 alone at 2048^3: ms and TFLOP/s, against the MI355X's float64 matrix peak of 78.6 TFLOP/s (AMD's data sheet).
Shapes: n = 200 and n = 1000 fakes at d = 2048 (Gram form), and the full form at d = 2048 (n = 2100 > d).

    python tools/fid_bench.py [--no-host] [--shapes 200,1000,2100]        # prints a table and one JSON line"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

D = 2048
F64_MATRIX_PEAK_TFLOPS = 78.6


def event_ms(fn):
    """milliseconds of fn() between two HIP events on the current stream, and its result"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='200,1000,2100')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--n-real', type=int, default=2000)
    a = ap.parse_args()
    import fid_numpy as FN
    from cat_amd import _lib
    from cat_amd.metric import fid_score as F
    _lib.load()
    assert torch.cuda.is_available(), 'fid_bench measures on the GPU only'
    dev = torch.device('cuda:0')
    real = FN.features(1, a.n_real, D, 0.0)
    mu1, s1 = FN.stats(real)
    rows = []
    for n in [int(v) for v in a.shapes.split(',')]:
        f2 = FN.features(2 + n, n, D, 0.2)
        feats = torch.from_numpy(f2.astype(np.float32)).to(dev)
        F.frechet_distance_from_features(mu1, s1, feats, cache={})            # warm-up: code objects, allocator
        cache, info = {}, {}
        cold, fd = event_ms(lambda: F.frechet_distance_from_features(mu1, s1, feats, cache=cache, info=info))
        warm = min(event_ms(lambda: F.frechet_distance_from_features(mu1, s1, feats, cache=cache))[0] for _ in range(3))
        row = dict(n=n, d=D, form=info['form'], steps=info['steps'], converged=info['converged'], device_ms_cold=cold, device_ms_cached=warm,
                   fd_device=fd, cpus=len(os.sched_getaffinity(0)))
        if not a.no_host:
            t0 = time.perf_counter()
            mu2, s2 = np.mean(f2, axis=0), np.cov(f2, rowvar=False)
            t1 = time.perf_counter()
            fd_host = float(F.calculate_frechet_distance(mu1, s1, mu2, s2))
            t2 = time.perf_counter()
            row.update(host_s_stats=t1 - t0, host_s_frechet=t2 - t1, fd_host=fd_host)
        rows.append(row)
        print(row, flush=True)
    x = torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, (D, D))).to(dev)
    y = torch.empty_like(x)
    F._gemm(x, x, out=y)
    ms = min(event_ms(lambda: F._gemm(x, x, out=y))[0] for _ in range(5))
    tf = 2.0 * D ** 3 / (ms * 1e-3) / 1e12
    gemm = dict(m=D, n=D, k=D, ms=ms, tflops=tf, share_of_f64_matrix_peak=tf / F64_MATRIX_PEAK_TFLOPS)
    print('gemm_f64 %d^3: %.3f ms, %.2f TFLOP/s = %.1f %% of %.1f' % (D, ms, tf, 100 * tf / F64_MATRIX_PEAK_TFLOPS, F64_MATRIX_PEAK_TFLOPS))
    print(json.dumps(dict(tool='fid_bench', tails=rows, gemm=gemm)))


if __name__ == '__main__':
    main()
