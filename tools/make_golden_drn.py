"""tests/golden/drn_miou.npz: the REFERENCE's own cityscapes mIoU path (DRNSeg('drn_d_105', 19) + metric/mIoU_score.py's `test`) on seeded
weights, images and labels.

Runs only in the build container (imports /root/reference).  What executes is the reference's metric/drn.py and metric/mIoU_score.py
(DRNSeg, SegList with its transforms, resize_4d_tensor's PIL enlargement, fast_hist, per_class_iu); `metric/__init__.py` pulls in modules
that are absent offline, so `metric` is a stub package whose path is the reference's directory.  Weights are not stored: the fixture holds
the key / shape list and a seed, tests rebuild them with oracle/detfill (plus the recorded bilinear `up.weight` plane, which the filler
overwrites).  Recorded besides the results: e32 = max |log p (float32) - log p (float64)| of the reference module itself -- the float bar of
the tests is delta = 100 * e32 -- and the UNDECIDED mask: label-map pixels whose float64 top-2 margin (float64 map, float64 resize) is
<= 2 * delta, where an argmax cannot be held to bit-exactness.

    python tools/make_golden_drn.py        # rewrites tests/golden/drn_miou.npz"""
import importlib
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref_import  # noqa: E402
import drn_torch as DT  # noqa: E402
from oracle import detfill  # noqa: E402

SEED_W, SEED_X, SEED_L = 31, 932, 933
N, H, W = 2, 128, 256
LH, LW = 1024, 2048
UNDECIDED_CAP = 0.005


def import_reference_miou():
    ref_import.install()
    for name in [m for m in sys.modules if m == 'metric' or m.startswith('metric.')]:
        del sys.modules[name]
    pkg = types.ModuleType('metric')
    pkg.__path__ = [os.path.join(ref_import.REF, 'metric')]
    sys.modules['metric'] = pkg
    mod = importlib.import_module('metric.mIoU_score')
    assert mod.__file__.startswith(ref_import.REF + '/'), mod.__file__
    return mod


def main():
    if not hasattr(np, 'int'):
        np.int = int      # the reference's ToTensor spells the label dtype `np.int`
    M = import_reference_miou()
    torch.manual_seed(0)
    model = M.DRNSeg('drn_d_105', 19, pretrained=False)
    ref_sd = model.state_dict()
    shapes = [[k, list(v.shape)] for k, v in ref_sd.items()]
    up_plane = ref_sd['up.weight'][0, 0].clone()
    assert all(torch.equal(ref_sd['up.weight'][c, 0], up_plane) for c in range(19))
    sd = detfill.fill_state_dict({k: torch.zeros(v.shape, dtype=v.dtype) for k, v in ref_sd.items()}, SEED_W)
    sd['up.weight'] = up_plane.expand(19, 1, 16, 16).clone()
    model.load_state_dict(sd)
    model.eval()

    fakes = detfill.images((N, 3, H, W), SEED_X)
    ims = DT.fakes_to_u8(fakes)
    names = ['frankfurt_%06d' % i for i in range(N)]

    # the reference's own float32 forward and the same module in float64, on the input exactly as SegList hands it over
    x32 = DT.normalized_input(ims)
    with torch.no_grad():
        logp32, seg32 = model(x32)
        m64 = M.DRNSeg('drn_d_105', 19, pretrained=False)
        m64.load_state_dict(sd)
        m64 = m64.double().eval()
        logp64, seg64 = m64(x32.double())
    e32 = float((logp32.double() - logp64).abs().max())
    delta = 100.0 * e32
    rng_lp = float(logp64.abs().max())
    print('e32 = %.3e (%.2e of max |log p64| = %.2f), delta = %.3e' % (e32, e32 / rng_lp, rng_lp, delta))
    print('seg logits: std %.2f, all finite %s' % (float(seg32.std()), bool(torch.isfinite(logp32).all())))

    # the torch restatement against the reference's run, right here
    mine_lp, mine_seg = DT.drnseg_forward(sd, x32, dtype=torch.float32)
    print('restatement vs reference: logits %.2e, log p %.2e (relative to max)' % (
        float((mine_seg - seg32).abs().max() / seg32.abs().max()), float((mine_lp - logp32).abs().max() / logp32.abs().max())))
    mine64 = DT.drnseg_forward(sd, x32, dtype=torch.float64)[0]
    assert float((mine64 - logp64).abs().max()) <= e32, 'the float64 restatement must sit inside the reference\'s own float32 error'

    # float64 ground truth of the resized map: decided / undecided pixels, float64 argmax
    arg64 = np.empty((N, LH, LW), dtype=np.uint8)
    undecided = np.empty((N, LH, LW), dtype=bool)
    for i in range(N):
        big = DT.bilinear_resize64(logp64[i:i + 1], (LH, LW))[0]
        top2 = big.topk(2, dim=0)
        arg64[i] = top2.indices[0].numpy().astype(np.uint8)
        undecided[i] = ((top2.values[0] - top2.values[1]) <= 2 * delta).numpy()
        del big, top2
    predicted = sorted(set(np.unique(arg64).tolist()))
    never = [c for c in range(19) if c not in predicted]
    assert never, 'every class is predicted: pick another seed (the nanmean path needs an absent class)'
    label_classes = [c for c in range(19) if c != never[-1]] + [255]
    labels = DT.make_labels(SEED_L, N, label_classes, (LH, LW))
    print('predicted classes', predicted, '-> absent class', never[-1])

    # the reference's `test`, with fast_hist wrapped to keep its per-image prediction and matrix
    seen = {'pred': [], 'hist': np.zeros((19, 19), dtype=np.int64)}
    fast_hist = M.fast_hist

    def recording_fast_hist(pred, label, n):
        h = fast_hist(pred, label, n)
        seen['pred'].append(np.asarray(pred, dtype=np.uint8).reshape(LH, LW).copy())
        seen['hist'] += h
        return h
    M.fast_hist = recording_fast_hist
    with tempfile.TemporaryDirectory() as tmp:
        table = DT.write_label_set(tmp, labels, names)
        ds = M.SegList(ims, names, table, tmp)
        assert all(torch.equal(ds[i][0], x32[i]) and np.array_equal(ds[i][1].numpy(), labels[i]) for i in range(N)), 'input restatement'
        miou = M.test(ims, names, model, torch.device('cpu'), table_path=table, data_dir=tmp, batch_size=1, num_workers=0, num_classes=19,
                      use_tqdm=False)
    M.fast_hist = fast_hist
    pred_ref = np.stack(seen['pred'])
    hist = seen['hist']
    share = float(undecided.mean())
    wrong_decided = int(((pred_ref != arg64) & ~undecided).sum())
    print('reference mIoU %.2f; undecided %.4f %% of the label map; reference vs float64 argmax: %d differ in all, %d on decided pixels' % (
        miou, 100 * share, int((pred_ref != arg64).sum()), wrong_decided))
    assert wrong_decided == 0, 'the reference\'s own prediction must equal the float64 argmax on every decided pixel'
    assert share <= UNDECIDED_CAP, 'undecided share above the cap: change the seed, not the cap'
    ious = M.per_class_iu(hist.astype(np.float64))
    assert np.isnan(ious[never[-1]]) and hist.sum() == int((labels < 19).sum())
    valid_undecided = int((undecided & (labels < 19)).sum())

    def checks(t):
        t = t.double()
        return [float(t.sum()), float(t.abs().sum()), float((t ** 2).sum())]
    out = dict(shapes=json.dumps(shapes), seed_w=SEED_W, seed_x=SEED_X, seed_l=SEED_L, size=np.array([N, H, W, LH, LW]), names=json.dumps(names),
               label_classes=np.array(label_classes), up_plane=up_plane.numpy(), seg=seg32.numpy(), logp_sample=logp32[:, :, 5::16, 3::16].contiguous().numpy(),
               seg_checks=np.array(checks(seg32)), logp_checks=np.array(checks(logp32)),
               logp64_checks=np.array(checks(logp64)), e32=e32, hist=hist, miou=float(miou), pred=pred_ref, undecided=np.packbits(undecided),
               undecided_share=share, valid_undecided=valid_undecided)
    path = os.path.join(ROOT, 'tests', 'golden', 'drn_miou.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
