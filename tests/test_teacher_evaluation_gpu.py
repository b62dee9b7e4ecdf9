"""GPU: the device-resident image set through the metrics, and `evaluate_model` of the real teacher models.

A: for one set of generated batches (3 + 3 + 2 images: FID's short last batch, KID's dropped tail) the network input the metric loops produce
   from a DeviceImages equals, torch.equal, the one they produce from the reference's list of CPU tensors -- FID and mIoU, recorded at the
   network's own forward -- and get_fid / get_kid / get_mIoU return the same numbers exactly: the same bytes, kernels and batching.
B: a real Pix2PixModel and a real CycleGANModel in the smallest configuration of tests/test_train_models.py: one training step,
   evaluate_model twice on a 3-batch loader with the inception network attached, finite FIDs, the bookkeeping, weights unchanged, the PNG
   dumps equal to the set's bytes, and a further training step afterwards.
C: a BatchNorm inception distiller returns the same metric/fid with eval_images 'device' as with 'host'.
Measured on the MI355X: every comparison holds exactly (the printed pairs agree to the last digit, repeated evaluations included); no kernel
on the path is run-to-run non-deterministic.  The model tests take the Frechet tail on the device: scipy's 2048 x 2048 root is seconds per call."""
import json
import os
import random

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
def inception(dev):
    """(state_dict, InceptionV3([3]) on the GPU) with the seeded weights of tests/golden/inception_fid.npz"""
    from cat_amd.metric import InceptionV3
    from oracle import ref_inception_cpu as RI
    g = H.load('inception_fid.npz')
    sd = RI.seeded_state_dict(H.sd_from_shapes(g['shapes']), int(g['seed_w']))
    net = InceptionV3([3])
    net.load_fid_state_dict(sd)
    return sd, net.to(dev).eval()


@pytest.fixture(scope='module')
def real_npz():
    feats = np.random.default_rng(11).standard_normal((64, 2048))
    return {'mu': feats.mean(0), 'sigma': np.cov(feats, rowvar=False)}


@pytest.fixture(scope='module')
def generated(dev):
    """(the reference's list of CPU batches, the DeviceImages of the same batches)"""
    from cat_amd.metric import DeviceImages
    from oracle import detfill
    fakes = [detfill.images((b, 3, 40, 56), 720 + i) * 1.1 for i, b in enumerate((3, 3, 2))]      # some values beyond [-1, 1]: the clip works
    s = DeviceImages(capacity=4)
    for f in fakes:
        s.append(f.to(dev))
    return fakes, s


class _Recorder(torch.nn.Module):
    """the network behind it, with every input kept as an NCHW host tensor"""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []

    def forward(self, x):
        self.seen.append(x.detach().cpu().contiguous())
        return self.net(x)


# ---------------------------------------------------------------------------------------------------------------- A: the metrics
def test_fid_network_input_and_value_equal_the_list_path(dev, inception, real_npz, generated):
    from cat_amd import metric
    from cat_amd.metric import fid_score
    _, net = inception
    fakes, s = generated
    assert np.array_equal(s.numpy(), metric.tensor2im_batch(torch.cat(fakes, 0)))
    values, inputs = [], []
    for arg in (fakes, s):
        rec = _Recorder(net)
        values.append(metric.get_fid(arg, rec, real_npz, device=dev, batch_size=3, use_tqdm=False, frechet='device'))
        inputs.append(rec.seen)
    assert [tuple(x.shape) for x in inputs[0]] == [(3, 3, 40, 56), (3, 3, 40, 56), (2, 3, 40, 56)]          # the short last batch
    assert len(inputs[1]) == 3 and all(torch.equal(a, b) for a, b in zip(*inputs))
    print('get_fid: list %.12g, DeviceImages %.12g' % tuple(values))
    assert np.isfinite(values[0]) and values[0] == values[1]
    # the default tail (numpy + scipy on the host, seconds per call at 2048 x 2048) is a function of the float64 features alone: the host
    # loop hands it the same ones
    host = [fid_score.get_activations_from_ims(arg, net, 3, 2048, dev, use_tqdm=False)
            for arg in (metric.tensor2im_batch(torch.cat(fakes, 0)).astype(float), s)]
    assert host[0].dtype == np.float64 and host[0].shape == (8, 2048) and np.array_equal(host[0], host[1])


def test_kid_equals_the_list_path(dev, inception, generated):
    from cat_amd import metric
    _, net = inception
    fakes, s = generated
    real_codes = np.random.default_rng(5).standard_normal((12, 2048))
    values, inputs = [], []
    for arg in (fakes, s):
        rec = _Recorder(net)
        np.random.seed(3)
        values.append(metric.get_kid(arg, real_codes, rec, device=dev, batch_size=3, n_subsets=4, subset_size=5))
        inputs.append(rec.seen)
    assert len(inputs[0]) == 2 and len(inputs[1]) == 2 and all(torch.equal(a, b) for a, b in zip(*inputs))          # the tail of 2 is dropped
    print('get_kid: list %r, DeviceImages %r' % tuple(values))
    assert np.isfinite(values[0]).all() and values[0] == values[1]


def test_miou_network_input_and_value_equal_the_list_path(dev, tmp_path):
    from cat_amd import metric
    from cat_amd.metric import DRNSeg, DeviceImages, miou
    g = H.load('drn_miou.npz')
    net = DRNSeg('drn_d_105', 19, pretrained=False)
    net.load_state_dict(fixture_state_dict(g))
    net = net.to(dev).eval()
    fakes, labels, names = fixture_inputs(g)
    table = DT.write_label_set(str(tmp_path), labels, names)
    chunks = [fakes[:1], fakes[1:]]
    s = DeviceImages()
    for c in chunks:
        s.append(c.to(dev))
    values, inputs = [], []
    for arg in (chunks, s):
        rec = _Recorder(net)
        values.append(metric.get_mIoU(arg, names, rec, dev, table_path=table, data_dir=str(tmp_path), batch_size=1, num_workers=0, use_tqdm=False))
        inputs.append(rec.seen)
    assert len(inputs[0]) == len(names) and all(torch.equal(a, b) for a, b in zip(*inputs))
    assert torch.equal(torch.cat(inputs[1], 0), miou.normalize_images(metric.tensor2im_batch(fakes)))
    print('get_mIoU: list %.4f, DeviceImages %.4f' % tuple(values))
    assert values[0] == values[1] and values[0] > 0
    assert metric.get_cityscapes_mIoU(s, names, net, dev, table_path=table, data_dir=str(tmp_path), batch_size=2) == values[0]


# ---------------------------------------------------------------------------------------------------------------- B: the teacher models
def _opt_for(meta, tmp_path, **kw):
    opt = H.make_opt(norm=meta['norm'], track=meta.get('track', False), ndf=meta['ndf'], gan_mode=meta['gan_mode'], ngf=meta['ngf'],
                     netG='inception_9blocks', dropout_rate=0, direction='AtoB', lr=meta['lr'], beta1=meta['beta1'], **kw)
    opt.log_dir, opt.eval_batch_size = str(tmp_path), 2
    return opt


def _snapshot(nets):
    return [{k: v.detach().clone() for k, v in n.state_dict().items()} for n in nets]


def _same(nets, snap):
    return all(torch.equal(v, s[k]) for n, s in zip(nets, snap) for k, v in n.state_dict().items())


def _capture_sets(monkeypatch):
    """metric.get_fid, recording the image set it is handed"""
    from cat_amd import metric
    seen, real = [], metric.get_fid

    def get_fid(fakes, *a, **k):
        seen.append(fakes)
        return real(fakes, *a, **k)
    monkeypatch.setattr(metric, 'get_fid', get_fid)
    return seen


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_pix2pix_model_evaluates_on_the_device(dev, inception, real_npz, tmp_path, monkeypatch):
    from cat_amd.distillers import evaluation as E
    from cat_amd.metric import DeviceImages
    from cat_amd.models import create_model
    from oracle import detfill
    g = H.load('train_steps.npz')
    meta = json.loads(str(g['p2p_meta']))
    opt = _opt_for(meta, tmp_path, model='pix2pix', lambda_recon=meta['lambda_recon'], lambda_gan=1.0, recon_loss_type='l1')
    m = create_model(opt, verbose=False)
    m.netG.load_state_dict(detfill.fill_state_dict(H.sd_from_shapes(g['p2p_G_shapes']), 301))
    m.netD.load_state_dict(detfill.fill_state_dict(H.sd_from_shapes(g['p2p_D_shapes']), 302))
    m.setup(opt, verbose=False)

    def train(step):
        m.set_input({'A': detfill.images((2, 3, 64, 64), 310 + step), 'B': detfill.images((2, 3, 64, 64), 320 + step), 'A_paths': [], 'B_paths': []})
        m.optimize_parameters(step)
        losses = m.get_current_losses()
        assert all(np.isfinite(v) for v in losses.values()), losses
        return losses
    train(0)
    with pytest.raises(RuntimeError, match='fid_fn'):          # nothing attached and no checkpoint option
        m.evaluate_model(0)
    E.attach_fid(m, inception[1], npz=real_npz, frechet='device')          # the Frechet tail on the device: scipy's 2048 x 2048 root takes seconds
    with pytest.raises(RuntimeError, match='eval_dataloader'):
        m.evaluate_model(0)
    m.eval_dataloader = [{'A': detfill.images((2, 3, 64, 64), 800 + i), 'B': detfill.images((2, 3, 64, 64), 810 + i),
                         'A_paths': ['/d/p%d_%d.jpg' % (i, j) for j in range(2)]} for i in range(3)]
    assert m.eval_images == 'device'
    sets = _capture_sets(monkeypatch)
    snap = _snapshot([m.netG, m.netD])
    r0 = m.evaluate_model(0)
    assert sorted(r0) == ['metric/fid', 'metric/fid-best', 'metric/fid-mean']
    assert np.isfinite(r0['metric/fid']) and r0['metric/fid'] > 0 and m.is_best and m.best_fid == r0['metric/fid'] and m.netG.training
    r1 = m.evaluate_model(1)
    print('pix2pix evaluate_model: fid %.10g, again %.10g' % (r0['metric/fid'], r1['metric/fid']))
    assert np.isfinite(r1['metric/fid']) and not m.is_best and len(m.fids) == 2 and r1['metric/fid-best'] == r0['metric/fid']
    assert r1['metric/fid'] == r0['metric/fid']          # the same weights, inputs and kernels, none of which sums in a run-dependent order
    assert _same([m.netG, m.netD], snap)                    # evaluation changes no weight
    assert len(sets) == 2 and isinstance(sets[0], DeviceImages) and len(sets[0]) == 6          # the set never left the device
    # the image dumps come from the same kernel: the PNG of a sample holds the set's bytes, and the host conversion agrees
    d = os.path.join(str(tmp_path), 'eval', '0')
    assert sorted(os.listdir(d)) == ['fake', 'input', 'real'] and len(os.listdir(os.path.join(d, 'fake'))) == 6
    assert np.array_equal(_png(os.path.join(d, 'fake', 'p1_0.png')), sets[0].numpy(2, 3)[0])
    assert np.array_equal(_png(os.path.join(d, 'input', 'p2_1.png')), E.tensor2im(m.eval_dataloader[2]['A'][1]))
    # 'host' gives the same number from the reference's list
    m.eval_images = 'host'
    r2 = m.evaluate_model(2)
    assert isinstance(sets[2], list) and r2['metric/fid'] == r0['metric/fid']
    m.eval_images = 'device'
    before = _snapshot([m.netG])
    train(1)                                               # no stale eval-mode plan: the next step trains
    assert not _same([m.netG], before)


def test_cycle_gan_model_evaluates_on_the_device(dev, inception, real_npz, tmp_path, monkeypatch):
    from cat_amd.metric import DeviceImages
    from cat_amd.models import create_model
    from oracle import detfill
    g = H.load('train_steps.npz')
    meta = json.loads(str(g['cyc_meta']))
    opt = _opt_for(meta, tmp_path, model='cycle_gan', dataset_mode='unaligned', lambda_A=meta['lambda_A'], lambda_B=meta['lambda_B'],
                   lambda_identity=meta['lambda_identity'], pool_size=meta['pool_size'])
    m = create_model(opt, verbose=False)
    gsh, dsh = H.sd_from_shapes(g['cyc_G_shapes']), H.sd_from_shapes(g['cyc_D_shapes'])
    m.netG_A.load_state_dict(detfill.fill_state_dict(gsh, 401))
    m.netG_B.load_state_dict(detfill.fill_state_dict(gsh, 402))
    m.netD_A.load_state_dict(detfill.fill_state_dict(dsh, 411))
    m.netD_B.load_state_dict(detfill.fill_state_dict(dsh, 412))
    m.setup(opt, verbose=False)
    random.seed(meta['seed'])
    nets = [m.netG_A, m.netG_B, m.netD_A, m.netD_B]

    def train(step):
        m.set_input({'A': detfill.images((1, 3, 64, 64), 420 + step), 'B': detfill.images((1, 3, 64, 64), 430 + step)})
        m.optimize_parameters(step)
        losses = m.get_current_losses()
        assert all(np.isfinite(v) for v in losses.values()), losses
    train(0)
    m.inception_model = inception[1]
    other = np.random.default_rng(12).standard_normal((64, 2048))
    m.npz_A, m.npz_B = real_npz, {'mu': other.mean(0), 'sigma': np.cov(other, rowvar=False)}
    # the Frechet tail on the device (scipy's 2048 x 2048 root takes seconds), as attach_fid(frechet='device') sets it up, per real set
    m.fid_frechet, m.fid_cache = 'device', {}
    m.npz_A_device, m.npz_B_device = ({k: torch.from_numpy(z[k]).to(dev) for k in ('mu', 'sigma')} for z in (m.npz_A, m.npz_B))
    m.eval_dataloader_AtoB = [{'A': detfill.images((1, 3, 64, 64), 820 + i), 'A_paths': ['/d/a%d.jpg' % i]} for i in range(3)]
    m.eval_dataloader_BtoA = [{'A': detfill.images((1, 3, 64, 64), 830 + i), 'A_paths': ['/d/b%d.jpg' % i]} for i in range(3)]
    sets = _capture_sets(monkeypatch)
    snap = _snapshot(nets)
    r0 = m.evaluate_model(0)
    assert list(r0) == ['metric/fid_B', 'metric/fid_B-mean', 'metric/fid_B-best', 'metric/fid_A', 'metric/fid_A-mean', 'metric/fid_A-best']
    assert all(np.isfinite(v) and v > 0 for v in r0.values()) and r0['metric/fid_A'] != r0['metric/fid_B']
    assert m.is_best_A and m.is_best_B and m.best_fid_B == r0['metric/fid_B'] and m.best_fid_A == r0['metric/fid_A']
    assert all(n.training for n in nets)
    r1 = m.evaluate_model(1)
    print('cycle_gan evaluate_model: fid_B %.10g / %.10g, fid_A %.10g / %.10g' % (r0['metric/fid_B'], r1['metric/fid_B'], r0['metric/fid_A'], r1['metric/fid_A']))
    assert not m.is_best_A and not m.is_best_B and len(m.fids_A) == 2 and len(m.fids_B) == 2
    for k in ('metric/fid_A', 'metric/fid_B'):
        assert r1[k] == r0[k] and r1[k + '-best'] == r0[k]
    assert _same(nets, snap)
    assert len(sets) == 4 and all(isinstance(s, DeviceImages) and len(s) == 3 for s in sets)
    d = os.path.join(str(tmp_path), 'eval', '0')
    assert sorted(os.listdir(d)) == ['AtoB', 'BtoA'] and sorted(os.listdir(os.path.join(d, 'BtoA'))) == ['fake', 'input']
    assert np.array_equal(_png(os.path.join(d, 'AtoB', 'fake', 'a1.png')), sets[0].numpy(1, 2)[0])
    assert np.array_equal(_png(os.path.join(d, 'BtoA', 'fake', 'b2.png')), sets[1].numpy(2, 3)[0])
    before = _snapshot([m.netG_A, m.netG_B])
    train(1)
    assert not _same([m.netG_A, m.netG_B], before)


# ---------------------------------------------------------------------------------------------------------------- C: the distiller opts in
def test_batchnorm_distiller_gives_the_same_fid_on_either_path(dev, inception, real_npz, tmp_path, monkeypatch):
    from cat_amd.distillers import create_distiller, evaluation as E
    from cat_amd.metric import DeviceImages
    from oracle import detfill
    opt = H.make_opt(norm='batch', track=True, ndf=8, teacher_ngf=16, student_ngf=8)
    opt.log_dir, opt.eval_batch_size = str(tmp_path), 2
    model = create_distiller(opt, verbose=False)
    E.attach_fid(model, inception[1], npz=real_npz)
    model.eval_dataloader = [{'A': detfill.images((2, 3, 64, 64), 840 + i), 'B': detfill.images((2, 3, 64, 64), 850 + i),
                             'A_paths': ['/d/s%d_%d.png' % (i, j) for j in range(2)], 'B_paths': ['/d/s%d_%d.png' % (i, j) for j in range(2)]}
                            for i in range(3)]
    sets = _capture_sets(monkeypatch)
    assert getattr(model, 'eval_images', 'host') == 'host'          # the distillers keep the reference's path unless asked
    host = model.evaluate_model(0)
    model.eval_images = 'device'
    device = model.evaluate_model(1)
    print('distiller evaluate_model: host %.12g, device %.12g' % (host['metric/fid'], device['metric/fid']))
    assert isinstance(sets[0], list) and isinstance(sets[1], DeviceImages) and len(sets[1]) == 6
    assert np.isfinite(host['metric/fid']) and device['metric/fid'] == host['metric/fid']
    for kind in ('Sfake', 'Tfake', 'input', 'real'):          # the dumps: the kernel's bytes equal the host conversion's
        for name in os.listdir(os.path.join(str(tmp_path), 'eval', '0', kind)):
            assert np.array_equal(_png(os.path.join(str(tmp_path), 'eval', '0', kind, name)), _png(os.path.join(str(tmp_path), 'eval', '1', kind, name)))
    # an attached callable has the reference's contract: the host path, whatever eval_images says
    got = {}
    model.fid_fn = lambda fakes: got.setdefault('fakes', fakes) and 7.0
    assert model.evaluate_model(2)['metric/fid'] == 7.0 and isinstance(got['fakes'], list) and not got['fakes'][0].is_cuda
