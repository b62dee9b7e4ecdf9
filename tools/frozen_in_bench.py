"""ms per forward of the frozen InstanceNorm teacher of the CycleGAN-style distillation (BASELINE configs[2]: inception_9blocks, ngf 64,
InstanceNorm without running statistics, eval mode under no_grad) at batch 8, 256 x 256, on three paths:

    general      nobody owns the blocks: layer by layer, the launches of the parent revision
    fused-tconv  cat_amd/frozen_in.py with stage 2 on the LDS-tile kernel (cat_tconv_fwd with f_s and stats)
    fused-s1x3   ... and stage 1 as one cat_tconv_fwd per kernel size instead of ONE cat_tstage1ws_fwd (CAT_STAGE1WS=0)
    fused-ksum   ... with stage 2 on the normalising wide DMA tile (cat_conv2d_ksum_norm_fwd)

timed by HIP events around `--iters` eager forwards, `--rounds` alternating rounds after a warm-up of every path; the median round is the
figure and the spread of the rounds stands next to it.  Then one profiled forward per fused path (cat_prof_enable: an event pair per entry
point): the time per launch of the block tail on either kernel (families `conv_ksum_norm` and `conv_tconv_multi`: the multi-segment launches of
cat_tconv_fwd are the tails and nothing else), both as a share of the fp32 MFMA peak from the algorithmic FLOPs the entry points report; and
stage 1 per block on either form (family `conv_tstage1ws` against the single-segment `conv_tconv` launches it replaces: 64 x 64 planes at
the default size).  One JSON line, printed and written to --out.

    python tools/frozen_in_bench.py [--batch 8] [--size 256] [--iters 10] [--rounds 3] [--out profiles/frozen_in_teacher.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MFMA_F32_PEAK_TFLOPS = 157.3      # v_mfma_f32_16x16x4_f32, 256 CUs at 2.4 GHz (bench.py's constant)
PATHS = ('general', 'fused-tconv', 'fused-s1x3', 'fused-ksum')


def teacher():
    from cat_amd import networks, synthetic
    opt = synthetic.default_options(norm='instance', track=False)
    net = networks.define_G(3, 3, 64, 'inception_9blocks', opt.norm, 0, 'normal', 0.02, [], opt=opt)
    net.load_state_dict(synthetic.fill_state_dict(net.state_dict(), 11))
    return net.cuda().eval()


def select(net, path):
    from cat_amd import frozen_in, fused_unit
    for b in net.features:
        frozen_in.disown(b)
    fused_unit.set_stage1_wide(path != 'fused-s1x3')
    if path != 'general':
        frozen_in.own_network(net)
        frozen_in.set_tail('ksum' if path == 'fused-ksum' else 'tconv')


def forward(net, x):
    with torch.no_grad():
        return net(x)


def timed(net, x, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        forward(net, x)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def families(net, x):
    """{family: (launches, ms, flops)} of one forward"""
    from cat_amd import _lib
    lib = _lib.load()
    torch.cuda.synchronize()
    lib.cat_prof_enable(1)
    forward(net, x)
    torch.cuda.synchronize()
    n = lib.cat_prof_collect()
    lib.cat_prof_enable(0)
    name, cnt, ms, fl = C.create_string_buffer(64), C.c_int64(), C.c_double(), C.c_double()
    out = {}
    for i in range(n):
        lib.cat_prof_family(i, name, 64, C.byref(cnt), C.byref(ms), C.byref(fl))
        out[name.value.decode()] = (cnt.value, ms.value, fl.value)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'frozen_in_teacher.json'))
    args = ap.parse_args()
    from cat_amd import _lib, frozen_in, ops, synthetic
    _lib.load()
    torch.cuda.set_device(0)
    net = teacher()
    default_tail = frozen_in.set_tail('tconv')      # (the package's default stage-2 choice, reported with the figures)
    x = ops.to_nhwc(synthetic.images((args.batch, 3, args.size, args.size), 1000).cuda())
    outs = {}
    for path in PATHS:      # warm-up of every path at this shape (filter packs, plans), and the outputs for the parity figure
        select(net, path)
        for _ in range(3):
            y = forward(net, x)
        outs[path] = y.clone()
    torch.cuda.synchronize()
    times = {p: [] for p in PATHS}
    for _ in range(args.rounds):
        for path in PATHS:
            select(net, path)
            times[path].append(timed(net, x, args.iters))
    row = {'batch': args.batch, 'size': args.size, 'iters': args.iters, 'blocks_owned': sum(frozen_in.owned(b) for b in net.features),
           'default_tail': default_tail}
    for path in PATHS:
        row[path] = {'ms': [round(t, 3) for t in times[path]], 'median_ms': round(statistics.median(times[path]), 3),
                     'spread_ms': round(max(times[path]) - min(times[path]), 3)}
        if path != 'general':
            d = (outs[path] - outs['general']).abs().max() / outs['general'].abs().max()
            row[path]['max_rel_diff_vs_general'] = float(d)
    fam = {}
    for path in PATHS[1:]:
        select(net, path)
        forward(net, x)
        fam[path] = families(net, x)
    nb = len(net.features)
    kc, kms, kfl = fam['fused-ksum'].get('conv_ksum_norm', (0, 0.0, 0.0))
    tc, tms, tfl = fam['fused-tconv'].get('conv_tconv_multi', (0, 0.0, 0.0))      # the multi-segment launches: the tails and nothing else
    share = lambda fl, ms: round(fl / 1e9 / ms / MFMA_F32_PEAK_TFLOPS, 4) if ms > 0 else None
    row['tail'] = {'launches': int(kc), 'ksum_norm_us_per_launch': round(1e3 * kms / max(kc, 1), 1), 'ksum_norm_share_of_fp32_mfma_peak': share(kfl, kms),
                   'tconv_launches': int(tc), 'tconv_us_per_launch': round(1e3 * tms / max(tc, 1), 1), 'tconv_share_of_fp32_mfma_peak': share(tfl, tms)}
    assert kc == nb and tc == nb, (kc, tc, nb)
    # stage 1: ONE cat_tstage1ws_fwd per block against the three single-segment cat_tconv_fwd launches it replaces
    wc, wms, wfl = fam['fused-tconv'].get('conv_tstage1ws', (0, 0.0, 0.0))
    c1, ms1, fl1 = fam['fused-tconv'].get('conv_tconv', (0, 0.0, 0.0))      # (single-segment launches that are not stage 1, if any)
    c3, ms3, fl3 = fam['fused-s1x3'].get('conv_tconv', (0, 0.0, 0.0))
    assert wc == nb and c3 - c1 == 3 * nb and 'conv_tstage1ws' not in fam['fused-s1x3'], (wc, c1, c3, nb)
    row['stage1'] = {'one_launch_us_per_block': round(1e3 * wms / nb, 1), 'one_launch_share_of_fp32_mfma_peak': share(wfl, wms),
                     'three_launches_us_per_block': round(1e3 * (ms3 - ms1) / nb, 1), 'three_launches_share_of_fp32_mfma_peak': share(fl3 - fl1, ms3 - ms1)}
    for path in PATHS[1:]:
        row['families_' + path.replace('-', '_')] = {k: [v[0], round(v[1], 3)] for k, v in sorted(fam[path].items())}
    line = json.dumps(row)
    print(line, flush=True)
    with open(args.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
