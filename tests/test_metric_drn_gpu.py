"""GPU: the cityscapes mIoU end to end on the HIP kernels -- cat_amd.metric.DRNSeg('drn_d_105', 19) + get_mIoU against the reference's own
run (tests/golden/drn_miou.npz, tools/make_golden_drn.py) and against the float64 torch restatement (tests/drn_torch.py).

Float bar: delta = 100 * e32, where e32 = max |log p (float32) - log p (float64)| of the REFERENCE module on its own CPU run (recorded in
the fixture; for the second shape, the restatement's own deviation on that input, computed here).  The GPU sums in another order (MFMA
tiles, BatchNorm folded into the filters), the project's observed forward errors are 1e-7 .. 2e-5 of the range: two orders of magnitude over
the reference's own float32 error cover that and stay ten times below the general 1e-3 bar, which must hold as well.
Class maps are integers: they must equal the reference's on every DECIDED label pixel (float64 top-2 margin > 2 * delta, mask recorded in
the fixture, <= 0.5 % undecided), and the confusion matrix may differ by at most two counts per undecided pixel with a valid label."""

import numpy as np
import pytest
import torch

import drn_torch as DT
import helpers as H
from test_metric_drn import fixture_inputs, fixture_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def net(dev):
    from cat_amd.metric import DRNSeg
    g = H.load('drn_miou.npz')
    sd = fixture_state_dict(g)
    m = DRNSeg('drn_d_105', 19, pretrained=False)
    m.load_state_dict(sd)
    return g, sd, m.to(dev).eval()


def test_drnseg_forward_within_delta_of_float64(dev, net):
    """Measured on the MI355X (recorded in DESIGN): see the printed figures."""
    from cat_amd import ops
    g, sd, m = net
    fakes, _, _ = fixture_inputs(g)
    x = DT.normalized_input(DT.fakes_to_u8(fakes))
    with torch.no_grad():
        logp, seg = m(x.to(dev))
    torch.cuda.synchronize()
    assert tuple(logp.shape) == (2, 19, 128, 256) and tuple(seg.shape) == (2, 19, 16, 32)
    logp64, seg64 = DT.drnseg_forward(sd, x, dtype=torch.float64)
    e32 = float(g['e32'])
    delta = 100 * e32
    err = float((logp.cpu().double() - logp64).abs().max())
    rng = float(logp64.abs().max())
    seg_err = float((seg.cpu().double() - seg64).abs().max())
    print('DRNSeg fixture: max |log p - log p64| = %.3e (e32 = %.3e, delta = %.3e, range %.2f -> %.2e of the range); logits err %.3e of %.2f' % (
        err, e32, delta, rng, err / rng, seg_err, float(seg64.abs().max())))
    assert err <= delta
    assert err <= 1e-3 * rng and seg_err <= 1e-3 * float(seg64.abs().max())
    # the reference's recorded float32 run: logits, strided sample, checksums
    assert float((seg.cpu() - torch.from_numpy(g['seg'])).abs().max()) <= delta
    assert float((logp.cpu()[:, :, 5::16, 3::16] - torch.from_numpy(g['logp_sample'])).abs().max()) <= delta + e32
    d = logp.cpu().double()
    got = np.array([float(d.sum()), float(d.abs().sum()), float((d ** 2).sum())])
    nel = d.numel()      # every element within delta: sum and abs-sum move by <= nel * delta, the square sum by <= nel * (2 * range + delta) * delta
    assert np.all(np.abs(got - g['logp64_checks']) <= np.array([nel * delta, nel * delta, nel * (2 * rng + delta) * delta]))
    # padding channel of both outputs stays 0
    for t in (logp, seg):
        full = torch.as_strided(t, (t.shape[0], ops.act_cs(t)) + tuple(t.shape[2:]), t.stride())
        assert bool((full[:, 19:] == 0).all())
    assert ops.act_cs(logp) == 20


def test_get_miou_end_to_end_against_the_reference(dev, net, tmp_path):
    from cat_amd import metric
    from cat_amd.metric import miou
    g, sd, m = net
    fakes, labels, names = fixture_inputs(g)
    n, h, w, lh, lw = (int(v) for v in g['size'])
    table = DT.write_label_set(str(tmp_path), labels, names)
    undecided = np.unpackbits(g['undecided'])[:n * lh * lw].reshape(n, lh, lw).astype(bool)
    assert undecided.mean() <= 0.005
    # class maps and the matrix, through the package's own loop (batch size 1 as the reference's default, then the whole set in one batch)
    for bs in (1, 2):
        preds = []
        hist = miou.confusion_matrix(metric.tensor2im_batch(fakes), names, m, dev, table, str(tmp_path), bs, 19, preds=preds)
        pred = np.concatenate(preds)
        wrong = pred != g['pred']
        diff = int(np.abs(hist - g['hist']).sum())
        print('batch %d: %d of %d label pixels differ from the reference, %d of them decided; sum |hist - hist_ref| = %d (cap %d); mIoU %.2f vs %.2f' % (
            bs, int(wrong.sum()), wrong.size, int((wrong & ~undecided).sum()), diff, 2 * int(g['valid_undecided']), miou.miou_from_hist(hist), float(g['miou'])))
        assert int((wrong & ~undecided).sum()) == 0
        assert diff <= 2 * int(g['valid_undecided'])
        assert hist.dtype == np.int64 and int(hist.sum()) == int((labels < 19).sum())
    assert miou.miou_from_hist(g['hist']) == float(g['miou'])
    # the public entry points: the reference's list of [-1, 1] batches and names
    chunks = [fakes[:1], fakes[1:]]
    v = metric.get_mIoU(chunks, names, m, dev, table_path=table, data_dir=str(tmp_path), batch_size=1, num_workers=0, use_tqdm=False)
    assert isinstance(v, float) and v == miou.miou_from_hist(hist)
    assert metric.get_cityscapes_mIoU(chunks, names, m, dev, table_path=table, data_dir=str(tmp_path), batch_size=2) == v


def test_drnseg_second_shape_against_float64_restatement(dev, net):
    """1 x 3 x 96 x 160 (not a multiple of 64); bar = 100 x the restatement's own float32-vs-float64 deviation on this input."""
    from oracle import detfill
    g, sd, m = net
    x = DT.normalized_input(DT.fakes_to_u8(detfill.images((1, 3, 96, 160), 977)))
    lp64 = DT.drnseg_forward(sd, x, dtype=torch.float64)[0]
    lp32 = DT.drnseg_forward(sd, x, dtype=torch.float32)[0]
    e32 = float((lp32.double() - lp64).abs().max())
    with torch.no_grad():
        logp, seg = m(x.to(dev))
    err = float((logp.cpu().double() - lp64).abs().max())
    print('DRNSeg 1x3x96x160: max |log p - log p64| = %.3e, restatement e32 = %.3e, bar %.3e, range %.2f' % (err, e32, 100 * e32, float(lp64.abs().max())))
    assert tuple(logp.shape) == (1, 19, 96, 160) and tuple(seg.shape) == (1, 19, 12, 20)
    assert err <= 100 * e32 and err <= 1e-3 * float(lp64.abs().max())


def test_drn_d_22_basic_blocks_against_float64_restatement(dev):
    """The BasicBlock network (two 3x3 convs per block, shortcut in the second one's epilogue) on seeded weights, 1 x 3 x 64 x 96; bar = 100 x
    the restatement's own float32-vs-float64 deviation on this input, and the general 1e-3."""
    from cat_amd.metric import DRNSeg
    from oracle import detfill
    m = DRNSeg('drn_d_22', 19)
    sd = detfill.fill_state_dict({k: torch.zeros_like(v) for k, v in m.state_dict().items()}, 33)
    sd['up.weight'] = m.up.weight.detach().clone()
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    x = DT.normalized_input(DT.fakes_to_u8(detfill.images((1, 3, 64, 96), 978)))
    lp64 = DT.drnseg_forward(sd, x, name='drn_d_22', dtype=torch.float64)[0]
    lp32 = DT.drnseg_forward(sd, x, name='drn_d_22', dtype=torch.float32)[0]
    e32 = float((lp32.double() - lp64).abs().max())
    with torch.no_grad():
        logp, seg = m(x.to(dev))
    err = float((logp.cpu().double() - lp64).abs().max())
    print('drn_d_22 1x3x64x96: max |log p - log p64| = %.3e, restatement e32 = %.3e, bar %.3e, range %.2f' % (err, e32, 100 * e32, float(lp64.abs().max())))
    assert tuple(logp.shape) == (1, 19, 64, 96) and bool(torch.isfinite(lp64).all())
    assert err <= 100 * e32 and err <= 1e-3 * float(lp64.abs().max())


def test_drnseg_refolds_when_a_tensor_changes(dev, net):
    g, sd, m = net
    x = torch.zeros(1, 3, 32, 32, device=dev)
    with torch.no_grad():
        a = m(x)[1].clone()
        m.seg.bias.add_(1.0)
        b = m(x)[1].clone()
        m.seg.bias.sub_(1.0)
        c = m(x)[1]
    assert torch.allclose(b, a + 1.0, atol=1e-4) and torch.allclose(a, c, atol=1e-5) and not torch.allclose(a, b, atol=0.5)


def test_evaluate_model_with_attach_miou(dev, net, tmp_path):
    """evaluate_model on the GPU with attach_miou on a generator stub: `metric/mIoU*` with the reference's bookkeeping."""
    from cat_amd.distillers import evaluation as E
    from test_evaluation import _inception_stub
    g, sd, _ = net
    fakes, labels, names = fixture_inputs(g)
    table = DT.write_label_set(str(tmp_path / 'data'), labels, names)
    model, _ = _inception_stub(tmp_path / 'log', mode='unaligned', dataroot='database/cityscapes', direction='BtoA')
    model.device = dev
    model.fid_fn = lambda fakes: 10.0
    model.opt.table_path, model.opt.cityscapes_path, model.opt.eval_batch_size, model.opt.num_threads = table, str(tmp_path / 'data'), 1, 0
    model.eval_dataloader = [{'A': fakes[i:i + 1] * 2.0, 'A_paths': ['/x/%s.png' % names[i]]} for i in range(2)]      # the stub's student halves A
    E.attach_miou(model, sd)
    assert next(model.drn_model.parameters()).is_cuda and not model.drn_model.training
    r = model.evaluate_model(1)
    from cat_amd import metric
    want = metric.get_mIoU([fakes], names, model.drn_model, dev, table_path=table, data_dir=str(tmp_path / 'data'), batch_size=1, use_tqdm=False)
    print('evaluate_model: mIoU %.2f (direct call %.2f, reference %.2f)' % (r['metric/mIoU'], want, float(g['miou'])))
    assert r['metric/mIoU'] == want      # integer sums: the same matrix, the same value
    assert r['metric/mIoU-best'] == r['metric/mIoU'] == r['metric/mIoU-mean'] and model.is_best
    r2 = model.evaluate_model(2)
    assert r2['metric/mIoU'] == r['metric/mIoU'] and not model.is_best and len(model.mIoUs) == 2
