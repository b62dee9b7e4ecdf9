"""Cost of the kernel inception distance on one GPU: feature extraction per image, and the MMD tail on the device next to numpy on the host.

Seeded weights and features (timing does not depend on the values).  Device-synchronised host clocks around enough repeats to fill a
fraction of a second or more, after a warm-up of every shape:
  * `features`  cat_amd.metric.InceptionV3([3]) on 256 x 256 images resident on the device, per batch size: ms per image;
  * `mmd`       one cat_kid_poly_sums call (two launches) for all subsets at (subset_size, n_subsets) = (100, 100) -- what the evaluation
                scripts run -- and (1000, 50) -- polynomial_mmd_averages' defaults -- on 2048-wide features: ms per call, and the f64 MFMA
                rate over the MACs the launch multiplies (4 products of padded 64-row panels: an end-to-end rate of the call, not a share of peak);
  * `host`      the same sums in float64 numpy on the CPUs this process may use (the reference's sklearn route does the same three matrix
                products per subset): ms per subset, over a few subsets.

    python tools/kid_bench.py [--images 200] [--batch 2,50] [--host-subsets 3]        # prints a table and one JSON line"""
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


def timed(fn, iters):
    """(mean, min) milliseconds of fn() over `iters` calls, each one device-synchronised"""
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.mean(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=200)
    ap.add_argument('--batch', default='2,50')
    ap.add_argument('--host-subsets', type=int, default=3)
    ap.add_argument('--n-features', type=int, default=2000)
    a = ap.parse_args()
    import kid_numpy as KN
    from cat_amd import _lib
    from cat_amd.metric import InceptionV3, kid_score as K
    from oracle import detfill
    _lib.load()
    assert torch.cuda.is_available(), 'kid_bench measures on the GPU only'
    dev = torch.device('cuda:0')
    net = InceptionV3([3])
    net.load_state_dict(detfill.fill_state_dict({k: torch.zeros_like(v) for k, v in net.state_dict().items()}, 41))
    net = net.to(dev).eval()
    feats = []
    with torch.no_grad():
        for b in [int(v) for v in a.batch.split(',')]:
            x = ((detfill.images((b, 3, 256, 256), 7) + 1) / 2).to(dev)
            timed(lambda: net(x), 3)
            iters = max(3, (a.images + b - 1) // b)
            mean, best = timed(lambda: net(x), iters)
            feats.append(dict(batch=b, images=iters * b, ms_per_image=mean / b, ms_per_image_min=best / b))
    x, y = KN.features(5, a.n_features, a.n_features, D)
    xd, yd = torch.from_numpy(x.astype(np.float32)).to(dev), torch.from_numpy(y.astype(np.float32)).to(dev)
    mmd = []
    for m, S in ((100, 100), (1000, 50)):
        np.random.seed(3)
        gi, ri = K.draw_subsets(len(x), len(y), S, m)
        gd, rd = torch.from_numpy(gi).to(dev), torch.from_numpy(ri).to(dev)
        out = torch.empty((S, 6 * m + 4), dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, _lib.query('cat_kid_poly_sums_ws_bytes', S, m) // 8), dtype=torch.float64, device=dev)

        def launch():
            K.poly_sums_device(xd, yd, gd, rd, 3, None, 1, out=out, ws=ws)
        timed(launch, 2)
        mean, best = timed(launch, 20 if m <= 100 else 5)
        pm = (m + 63) // 64 * 64
        flops = 2.0 * 4 * S * pm * pm * D
        hs = []
        for s in range(min(a.host_subsets, S)):
            t0 = time.perf_counter()
            KN.poly_sums(x, y, gi[s:s + 1], ri[s:s + 1])
            hs.append((time.perf_counter() - t0) * 1e3)
        mmd.append(dict(subset_size=m, n_subsets=S, ms_per_call=mean, ms_per_call_min=best, f64_tflops=flops / (mean * 1e-3) / 1e12,
                        host_ms_per_subset=float(np.mean(hs)), host_ms_all_subsets=float(np.mean(hs)) * S, cpus=len(os.sched_getaffinity(0))))
    print('features: batch  images  ms/img (min)')
    for r in feats:
        print('          %5d  %6d  %7.3f (%7.3f)' % (r['batch'], r['images'], r['ms_per_image'], r['ms_per_image_min']))
    print('mmd: subset  subsets  GPU ms/call (min)  f64 TF/s   host numpy ms/subset  x subsets')
    for r in mmd:
        print('     %6d  %7d  %9.3f (%7.3f)  %7.2f   %12.1f  %10.0f   (%d CPUs)' % (
            r['subset_size'], r['n_subsets'], r['ms_per_call'], r['ms_per_call_min'], r['f64_tflops'], r['host_ms_per_subset'],
            r['host_ms_all_subsets'], r['cpus']))
    print(json.dumps(dict(tool='kid_bench', d=D, features=feats, mmd=mmd)))


if __name__ == '__main__':
    main()
