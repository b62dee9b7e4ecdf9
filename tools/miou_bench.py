"""Per-image cost of the cityscapes mIoU path on the GPU (cat_amd.metric.DRNSeg + the fused tail) next to what an integrator runs today.

Synthetic 256 x 512 images and 1024 x 2048 labels, resident on the device; seeded weights (timing does not depend on the values).  Per batch
size, device-synchronised times per image of
  * `fwd`   DRNSeg.features: DRN-D-105 `base` + `seg` up to the class logits, on cat_conv2d_fwd_ex (FLOPs counted from the shapes: true conv
            MACs x 2; the TF/s is a whole-network rate, launch gaps and the narrow full-resolution layers included, not a kernel's share of peak);
  * `tail`  cat_seg_up_logsoftmax + cat_seg_confusion (up-sampling, log-softmax, resize to the label size, argmax, confusion matrix);
and the yardsticks in the same process, like for like:
  * `torch_fwd`   the stock-torch twin of the same network up to the class logits (tests/drn_torch.py moved to the device: ATen = MIOpen);
  * `torch_head`  the twin's grouped conv_transpose2d + log_softmax (the first half of `tail`; the second half has no device twin);
  * `host_tail`   the reference-style tail after the head: device-to-host copy of the [1, 19, 256, 512] map, PIL bilinear enlargement to
                  2048 x 1024 in one thread per channel (19 threads, as the reference starts them, on the CPUs this process may use: the
                  count is printed), numpy argmax + bincount.  A few images only: it takes about a second each.

    python tools/miou_bench.py [--images 50] [--warmup 5] [--batch 1,4] [--host-images 3]        # prints a table and one JSON line"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

H, W, LH, LW, NCLS = 256, 512, 1024, 2048, 19


def count_flops(net, x):
    """2 x MACs of every convolution of one `features` call, from the shapes the launches see."""
    from cat_amd.metric import drn
    total = [0.0]
    inner = drn.conv_bn_act

    def counting(xx, conv, bn, act, res=None):
        y = inner(xx, conv, bn, act, res)
        total[0] += 2.0 * y.shape[0] * y.shape[2] * y.shape[3] * conv.out_channels * conv.kernel_size[0] * conv.kernel_size[1] * conv.in_channels
        return y
    drn.conv_bn_act = counting
    try:
        net.features(x)
    finally:
        drn.conv_bn_act = inner
    return total[0]


def timed(fn, iters):
    """mean milliseconds of fn() over `iters` calls, each one device-synchronised"""
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.mean(ms)), float(np.min(ms))


def host_tail(final, label):
    """metric/mIoU_score.py:180-206, 238-241 restated: D2H copy, PIL resize per channel in threads, argmax, bincount."""
    from PIL import Image
    t = final.cpu().numpy()
    out = np.empty((t.shape[0], t.shape[1], LH, LW), dtype=np.float32)

    def resize_channel(j):
        for i in range(t.shape[0]):
            out[i, j] = np.array(Image.fromarray(t[i, j]).resize((LW, LH), Image.BILINEAR))
    workers = [threading.Thread(target=resize_channel, args=(j,)) for j in range(t.shape[1])]
    for w in workers:
        w.start()
    for w in workers:
        w.join()
    pred = out.argmax(axis=1).flatten()
    lab = label.flatten()
    k = (lab >= 0) & (lab < NCLS)
    return np.bincount(NCLS * lab[k].astype(int) + pred[k], minlength=NCLS ** 2).reshape(NCLS, NCLS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', default='1,4')
    ap.add_argument('--host-images', type=int, default=3)
    a = ap.parse_args()
    import drn_torch as DT
    from cat_amd import _lib
    from cat_amd.metric import DRNSeg, miou
    from oracle import detfill
    _lib.load()
    dev = torch.device('cuda:0')
    net = DRNSeg('drn_d_105', NCLS, pretrained=False)
    sd = detfill.fill_state_dict({k: torch.zeros_like(v) for k, v in net.state_dict().items()}, 31)
    sd['up.weight'] = net.up.weight.detach().clone()
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    rows = []
    with torch.no_grad():
        for b in [int(v) for v in a.batch.split(',')]:
            x = DT.normalized_input(DT.fakes_to_u8(detfill.images((b, 3, H, W), 7))).to(dev)
            label = torch.from_numpy(DT.make_labels(9, b, list(range(NCLS)) + [255], (LH, LW))).to(dev)
            hist = torch.zeros((NCLS, NCLS), dtype=torch.int64, device=dev)
            flops = count_flops(net, x) / b
            logits = net.features(x)
            iters = max(1, (a.images + b - 1) // b)

            def tail():
                miou.confusion(net.head(logits), label, hist, NCLS)

            def torch_fwd():
                return DT.drnseg_forward(sd_dev, x, dtype=torch.float32, head=False)

            def torch_head():
                return F.log_softmax(F.conv_transpose2d(logits_nchw, sd_dev['up.weight'], None, stride=8, padding=4, groups=NCLS), dim=1)
            logits_nchw = torch_fwd()[1]
            for fn in (lambda: net.features(x), tail, torch_fwd, torch_head):
                timed(fn, max(1, a.warmup // b + 1))
            fwd, fwd_min = timed(lambda: net.features(x), iters)
            tl, tl_min = timed(tail, iters)
            tw, tw_min = timed(torch_fwd, iters)
            th, th_min = timed(torch_head, iters)
            rows.append(dict(batch=b, images=iters * b, gflop_per_image=flops / 1e9, fwd_ms_per_image=fwd / b, fwd_ms_min=fwd_min / b,
                             fwd_tflops=flops / (fwd / b * 1e-3) / 1e12, tail_ms_per_image=tl / b, tail_ms_min=tl_min / b,
                             torch_fwd_ms_per_image=tw / b, torch_fwd_ms_min=tw_min / b, torch_head_ms_per_image=th / b, torch_head_ms_min=th_min / b))
        host = None
        if a.host_images > 0:
            x = DT.normalized_input(DT.fakes_to_u8(detfill.images((1, 3, H, W), 7))).to(dev)
            label = DT.make_labels(9, 1, list(range(NCLS)) + [255], (LH, LW))
            final = net(x)[0]
            hist = torch.zeros((NCLS, NCLS), dtype=torch.int64, device=dev)
            miou.confusion(final, torch.from_numpy(label).to(dev), hist, NCLS)
            ts = []
            for _ in range(a.host_images):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                href = host_tail(final, label)
                ts.append((time.perf_counter() - t0) * 1e3)
            host = dict(images=a.host_images, host_tail_ms_per_image=float(np.mean(ts)), host_tail_ms_min=float(np.min(ts)),
                        hist_abs_diff_vs_gpu=int(np.abs(href - hist.cpu().numpy()).sum()), cpus=len(os.sched_getaffinity(0)))
    print('batch  GFLOP/img  fwd ms/img (min)   TF/s   tail ms/img (min)   torch fwd ms/img (min)   torch head ms/img (min)')
    for r in rows:
        print('%5d  %9.2f  %8.3f (%7.3f)  %5.1f  %8.3f (%7.3f)    %8.3f (%7.3f)    %8.3f (%7.3f)' % (
            r['batch'], r['gflop_per_image'], r['fwd_ms_per_image'], r['fwd_ms_min'], r['fwd_tflops'], r['tail_ms_per_image'], r['tail_ms_min'],
            r['torch_fwd_ms_per_image'], r['torch_fwd_ms_min'], r['torch_head_ms_per_image'], r['torch_head_ms_min']))
    if host:
        print('host tail (D2H + PIL x 19 threads on %d CPUs + numpy): %.1f ms/img (min %.1f) over %d images; |hist - hist_gpu| = %d' % (
            host['cpus'], host['host_tail_ms_per_image'], host['host_tail_ms_min'], host['images'], host['hist_abs_diff_vs_gpu']))
    print(json.dumps(dict(tool='miou_bench', image=[H, W], label=[LH, LW], rows=rows, host=host)))


if __name__ == '__main__':
    main()
