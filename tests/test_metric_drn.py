"""CPU: the host side of the cityscapes mIoU (cat_amd/metric/drn.py, cat_amd/metric/miou.py, evaluation.attach_miou) and the torch
restatement of the network (tests/drn_torch.py), pinned to the reference's own run recorded in tests/golden/drn_miou.npz
(tools/make_golden_drn.py: DRNSeg('drn_d_105', 19) + metric/mIoU_score.py's `test` on seeded weights, images and labels).
The kernels themselves are GPU tests: tests/test_seg_kernels_gpu.py, tests/test_metric_drn_gpu.py."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import drn_torch as DT
import helpers as H
from oracle import detfill


def fixture_state_dict(g):
    """The seeded weights of the fixture: detfill over the recorded key / shape list, then the recorded bilinear plane back into `up.weight`
    (the filler overwrites it)."""
    sd = detfill.fill_state_dict(H.sd_from_shapes(g['shapes']), int(g['seed_w']))
    sd['up.weight'] = torch.from_numpy(g['up_plane']).expand(19, 1, 16, 16).clone()
    return sd


def fixture_inputs(g):
    n, h, w, lh, lw = (int(v) for v in g['size'])
    fakes = detfill.images((n, 3, h, w), int(g['seed_x']))
    labels = DT.make_labels(int(g['seed_l']), n, [int(c) for c in g['label_classes']], (lh, lw))
    return fakes, labels, json.loads(str(g['names']))


def test_drnseg_state_dict_surface_is_the_references():
    """Keys, order and shapes of DRNSeg('drn_d_105', 19).state_dict() against the reference's recorded list (651 entries); a reference-keyed
    dict (num_batches_tracked and up.weight included) loads strictly."""
    from cat_amd.metric import DRNSeg
    g = H.load('drn_miou.npz')
    want = [(k, tuple(s)) for k, s in json.loads(str(g['shapes']))]
    net = DRNSeg('drn_d_105', 19, pretrained=False)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert len(want) == 651 and got == want
    sd = fixture_state_dict(g)
    assert 'base.0.1.num_batches_tracked' in sd and 'up.weight' in sd
    missing, unexpected = net.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    assert torch.equal(net.state_dict()['base.5.22.bn3.running_var'], sd['base.5.22.bn3.running_var'])
    assert torch.equal(net.up.weight, sd['up.weight']) and not any(p.requires_grad for p in net.parameters())
    # the constructor's own `up` fill is the reference's bilinear plane
    assert torch.equal(DRNSeg('drn_d_22', 19).up.weight[7, 0], torch.from_numpy(g['up_plane']))


def test_drnseg_refuses_training_and_grad_mode():
    from cat_amd.metric import DRNSeg
    net = DRNSeg('drn_d_22', 19)
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match='eval mode under no_grad'):
        net(x)
    net.eval()
    with pytest.raises(NotImplementedError, match='eval mode under no_grad'):
        net(x)
    with pytest.raises(NotImplementedError):
        DRNSeg('drn_c_26', 19)


def test_torch_restatement_reproduces_the_reference_run():
    """tests/drn_torch.py against the recorded logits, log-probability sample and checksums at the oracle bar (2e-5 of the range), and the
    reference's class map on every decided pixel."""
    g = H.load('drn_miou.npz')
    sd = fixture_state_dict(g)
    fakes, labels, names = fixture_inputs(g)
    x = DT.normalized_input(DT.fakes_to_u8(fakes))
    logp, seg = DT.drnseg_forward(sd, x, dtype=torch.float32)
    assert float((seg - torch.from_numpy(g['seg'])).abs().max()) <= 2e-5 * float(np.abs(g['seg']).max())
    sample = logp[:, :, 5::16, 3::16]
    assert float((sample - torch.from_numpy(g['logp_sample'])).abs().max()) <= 2e-5 * float(np.abs(g['logp_sample']).max())
    for t, name in ((seg, 'seg_checks'), (logp, 'logp_checks')):
        d = t.double()
        got = np.array([float(d.sum()), float(d.abs().sum()), float((d ** 2).sum())])
        assert np.all(np.abs(got - g[name]) <= 2e-5 * np.abs(g[name][1:]).max()), name
    logp64 = DT.drnseg_forward(sd, x, dtype=torch.float64)[0]
    d64 = logp64.double()
    got = np.array([float(d64.sum()), float(d64.abs().sum()), float((d64 ** 2).sum())])
    assert np.all(np.abs(got - g['logp64_checks']) <= 1e-9 * np.abs(g['logp64_checks']))
    # class map on decided pixels, image by image (float64 resize of the float64 map)
    n, h, w, lh, lw = (int(v) for v in g['size'])
    undecided = np.unpackbits(g['undecided'])[:n * lh * lw].reshape(n, lh, lw).astype(bool)
    assert abs(undecided.mean() - float(g['undecided_share'])) < 1e-12 and undecided.mean() <= 0.005
    for i in range(n):
        arg = DT.bilinear_resize64(logp64[i:i + 1], (lh, lw))[0].argmax(0).numpy()
        assert np.array_equal(arg[~undecided[i]], g['pred'][i][~undecided[i]])


def test_label_name_matching(tmp_path):
    from cat_amd.metric import miou
    table = tmp_path / 'table.txt'
    table.write_text('1 gt/a_label.png left/aachen_000000_000019_leftImg8bit.png\n'
                     '2 gt/b_label.png left/bochum_000001_000019_leftImg8bit.png\n'
                     '3 gt/c_label.png left/xbochum_000001_000019_leftImg8bit.png\n')
    # by id, by the `endswith` rule on the image path without '.png' (first matching line wins), in the order of `names`
    got = miou.read_label_list(['2', 'aachen_000000_000019_leftImg8bit', 'bochum_000001_000019_leftImg8bit', '000019_leftImg8bit'], str(table))
    assert got == ['gt/b_label.png', 'gt/a_label.png', 'gt/b_label.png', 'gt/a_label.png']
    with pytest.raises(AssertionError):
        miou.read_label_list(['1', 'cologne_000000'], str(table))


def test_per_class_iu_nanmean_and_rounding():
    from cat_amd import metric
    hist = np.array([[6, 2, 0], [1, 3, 0], [0, 0, 0]], dtype=np.int64)      # class 2: never labelled, never predicted
    iu = metric.per_class_iu(hist)
    assert np.isnan(iu[2]) and np.allclose(iu[:2], [6 / 9, 3 / 6])
    assert metric.miou_from_hist(hist) == round((6 / 9 + 3 / 6) / 2 * 100, 2) == 58.33
    g = H.load('drn_miou.npz')
    assert metric.miou_from_hist(g['hist']) == float(g['miou'])      # the reference's value from the reference's matrix, exactly
    assert np.isnan(metric.per_class_iu(g['hist'])).sum() >= 1


def test_image_normalisation_and_label_loading(tmp_path):
    from cat_amd import metric
    from cat_amd.metric import miou
    fakes = detfill.images((2, 3, 8, 12), 5)
    ims = metric.tensor2im_batch(fakes)
    assert ims.dtype == np.uint8 and np.array_equal(ims, DT.fakes_to_u8(fakes))
    assert torch.equal(miou.normalize_images(ims), DT.normalized_input(ims))
    labels = DT.make_labels(3, 2, [0, 7, 18, 255], (16, 32), (4, 8))
    DT.write_label_set(str(tmp_path), labels, ['a', 'b'])
    got = miou.load_labels(['gtFine/a_labelTrainIds.png', 'gtFine/b_labelTrainIds.png'], str(tmp_path))
    assert got.dtype == np.uint8 and np.array_equal(got, labels)


def _stub(tmp_path):
    from test_evaluation import _inception_stub
    m, _ = _inception_stub(tmp_path, mode='unaligned', dataroot='database/cityscapes', direction='BtoA')
    m.fid_fn = lambda fakes: 10.0
    m.opt.table_path, m.opt.cityscapes_path, m.opt.eval_batch_size, m.opt.num_threads = 'opt_table.txt', 'opt_dir', 3, 5
    m.device = torch.device('cpu')
    return m


def test_evaluate_uses_drn_model_without_a_miou_fn(tmp_path, monkeypatch):
    from cat_amd import metric
    m = _stub(tmp_path)
    with pytest.raises(RuntimeError, match='miou_fn') as e:
        m.evaluate_model(1)
    assert 'attach_miou' in str(e.value)
    seen = {}

    def fake_get_mIoU(fakes, names, model, device, **kw):
        seen.update(kw, fakes=fakes, names=names, model=model, device=device)
        return 12.34
    monkeypatch.setattr(metric, 'get_mIoU', fake_get_mIoU)
    m.drn_model = object()
    r = m.evaluate_model(2)
    assert r['metric/mIoU'] == 12.34 and r['metric/mIoU-best'] == 12.34 and r['metric/mIoU-mean'] == 12.34 and m.is_best
    assert seen['model'] is m.drn_model and seen['names'][:2] == ['im0a', 'im0b'] and len(seen['fakes']) == 7
    assert (seen['table_path'], seen['data_dir'], seen['batch_size'], seen['num_workers']) == ('opt_table.txt', 'opt_dir', 3, 5)
    # an attached miou_fn still wins
    m2 = _stub(tmp_path)
    m2.drn_model = object()
    m2.miou_fn = lambda fakes, names: 0.5
    assert m2.evaluate_model(3)['metric/mIoU'] == 0.5 and 'table_path' in seen


def test_attach_miou_builds_the_network_from_a_reference_checkpoint(tmp_path):
    from cat_amd.distillers import evaluation as E
    from cat_amd.metric import DRNSeg
    g = H.load('drn_miou.npz')
    sd = fixture_state_dict(g)
    path = os.path.join(str(tmp_path), 'drn-d-105_ms_cityscapes.pth')
    torch.save(sd, path)
    m = Namespace(device=torch.device('cpu'))
    net = E.attach_miou(m, path, table_path='t.txt', data_dir='d')
    assert isinstance(m.drn_model, DRNSeg) and m.drn_model is net and not net.training
    assert (m.miou_table_path, m.miou_data_dir) == ('t.txt', 'd')
    assert torch.equal(net.seg.bias, sd['seg.bias']) and torch.equal(net.base[6][2].conv2.weight, sd['base.6.2.conv2.weight'])


def test_new_entry_points_are_exported():
    from cat_amd import _build, _lib
    _build.build(verbose=False)
    lib = _lib.load()
    for name in ('cat_conv2d_fwd_ex', 'cat_seg_up_logsoftmax', 'cat_seg_confusion'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
