"""CPU: `--norm syncbatch` and `--recon_loss_type smooth_l1` through the host layers of the inception family.

The reference wraps the inception family in plain nn.DataParallel (models/networks.py:157-161), so its SynchronizedBatchNorm2d never leaves
the F.batch_norm arm (sync_batchnorm/batchnorm.py:68-72): on this path `syncbatch` is BatchNorm2d with per-replica statistics whose
num_batches_tracked never advances.  Here: the factory, the state_dict layout, shrink (bit-exact against the reference's run -- its shrink of
the syncbatch teacher equals shrink_bn.npz entry for entry, which tools/make_golden_norm_recon.py asserts), weight transfer, export and the
option values."""
import argparse
import copy
import json
import warnings

import numpy as np
import pytest
import torch

import helpers as H
from oracle import detfill


def _nets(norm, track=True):
    from cat_amd import networks
    opt = H.make_opt(norm=norm, track=track, gpu_ids=[])
    G = networks.define_G(3, 3, 16, 'inception_9blocks', norm, 0, 'normal', 0.02, [], opt=opt)
    D = networks.define_D(6, 16, 'n_layers', 3, norm, 'normal', 0.02, [], opt=opt)
    return opt, G, D


def _norms(net):
    from cat_amd import nn as cnn
    return [m for m in net.modules() if isinstance(m, cnn.BatchNorm2d)]


def test_factory_builds_the_class_and_warns_without_running_stats():
    from cat_amd import networks, nn as cnn
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        layer = networks.get_norm_layer('syncbatch', affine=True, track_running_stats=True)(12)
    assert type(layer) is cnn.SynchronizedBatchNorm2d and isinstance(layer, cnn.BatchNorm2d)
    assert layer.replica_local and layer.affine and layer.track_running_stats and layer.num_features == 12
    with pytest.warns(UserWarning, match='track_running_stats=False is not supported by the SynchronizedBatchNorm'):
        layer = networks.get_norm_layer('syncbatch', affine=False, track_running_stats=False)(5)
    assert layer.replica_local and not layer.affine and layer.running_mean is None
    # the SPADE path's constructor call keeps the exchange: the keyword's default is the behaviour before it existed
    assert not cnn.SynchronizedBatchNorm2d(4, affine=True).replica_local
    assert not copy.deepcopy(cnn.SynchronizedBatchNorm2d(4)).replica_local and copy.deepcopy(layer).replica_local


def test_networks_have_the_batch_state_dict_layout():
    from cat_amd import nn as cnn
    _, Gb, Db = _nets('batch')
    _, Gs, Ds = _nets('syncbatch')
    for b, s in ((Gb, Gs), (Db, Ds)):
        assert [(k, tuple(v.shape), v.dtype) for k, v in b.state_dict().items()] == [(k, tuple(v.shape), v.dtype) for k, v in s.state_dict().items()]
        assert len(_norms(s)) == len(_norms(b)) > 0
        assert all(type(m) is cnn.SynchronizedBatchNorm2d and m.replica_local for m in _norms(s))
        assert not any(isinstance(m, cnn.SynchronizedBatchNorm2d) for m in _norms(b))
        s.load_state_dict(b.state_dict())
    # init_weights matches by class name: the gammas were drawn from N(1, 0.02), not left at 1
    assert all(float((m.weight.detach() - 1).abs().max()) > 0 for m in _norms(Gs))


def test_shrink_of_a_syncbatch_teacher_is_bit_exact_and_stays_replica_local():
    from cat_amd import networks, nn as cnn, prune
    g = H.load('shrink_bn.npz')
    target = 4.6e9
    opt = H.make_opt(norm='syncbatch', track=True, target_flops=target, gpu_ids=[])
    T = networks.define_G(3, 3, 64, 'inception_9blocks', 'syncbatch', 0, 'normal', 0.02, [], opt=opt)
    T.load_state_dict(H.teacher_sd(opt))
    T.eval()
    macs, _ = prune.model_profiling(T, 256, 256)
    assert [macs, T.down_sampling.n_macs, T.features.n_macs, T.up_sampling.n_macs] == list(g['t_macs'])
    assert np.array_equal(T.down_sampling[2].weight.detach().numpy(), g['g_down0'])
    thr, searched = prune.search_threshold(T, target, opt)
    assert np.float32(thr.item()) == g['thr'] and searched == int(g['s_macs'][0])
    S = copy.deepcopy(T)
    trunk, _ = prune._apply_structure(S, T, thr, opt, copy_weights=True)
    cfg = json.loads(str(g['cfg']))
    assert [S.down_sampling[i].num_features for i in (2, 5, 8)] == cfg['down'] and trunk == cfg['down'][2]
    assert [S.up_sampling[i].num_features for i in (1, 4)] == cfg['up']
    assert [[b.res_channels, b.dw_channels] for b in S.features] == cfg['blocks']
    macs, _ = prune.model_profiling(S, 256, 256)
    assert [macs, S.down_sampling.n_macs, S.features.n_macs, S.up_sampling.n_macs] == list(g['s_macs'])
    ssd = S.state_dict()
    assert [[k, list(v.shape)] for k, v in ssd.items()] == json.loads(str(g['student_shapes']))
    copied = [k for k in g.files if k.startswith('copied:')]
    assert len(copied) >= 8
    for key in copied:
        assert np.array_equal(ssd[key[7:]].numpy(), g[key]), key
    norms = _norms(S)
    assert len(norms) == len(_norms(T)) - sum(c == 0 for b in cfg['blocks'] for c in b[0]) - 2 * sum(c == 0 for b in cfg['blocks'] for c in b[1])
    assert all(type(m) is cnn.SynchronizedBatchNorm2d and m.replica_local for m in norms)


def test_weight_transfer_and_export_accept_the_network():
    from cat_amd import export, networks
    from cat_amd.weight_transfer import load_pretrained_weight
    nets = {}
    for norm in ('batch', 'syncbatch'):
        opt = H.make_opt(norm=norm, track=True, gpu_ids=[])
        A = networks.define_G(3, 3, 32, 'inception_9blocks', norm, 0, 'normal', 0.02, [], opt=opt)
        B = networks.define_G(3, 3, 20, 'inception_9blocks', norm, 0, 'normal', 0.02, [], opt=opt)
        A.load_state_dict(detfill.fill_state_dict(A.state_dict(), 501))
        B.load_state_dict(detfill.fill_state_dict(B.state_dict(), 502))
        load_pretrained_weight('inception_9blocks', 'inception_9blocks', A, B, 32, 20)
        nets[norm] = B
    sb, ss = nets['batch'].state_dict(), nets['syncbatch'].state_dict()
    assert list(sb) == list(ss) and all(torch.equal(sb[k], ss[k]) for k in sb)      # the same index selection, tensor for tensor
    assert not torch.equal(ss['down_sampling.1.weight'], detfill.fill_state_dict(ss, 502)['down_sampling.1.weight'])      # and it copied
    # the stock-torch twin: nn.BatchNorm2d in the class's place (F.batch_norm is what the reference's class runs here), same output
    x = detfill.images((2, 3, 32, 32), 77)
    outs = {}
    for norm, net in nets.items():
        twin = export.to_reference_module(net.train())
        assert list(twin.state_dict()) == list(ss)
        assert all(type(m).__module__.startswith(('torch.nn', 'cat_amd.export')) for m in twin.modules())
        with torch.no_grad():
            outs[norm] = twin(x)
    assert torch.equal(outs['batch'], outs['syncbatch'])


def _parser(setter):
    p = argparse.ArgumentParser()
    setter(p, True)
    return p


def test_option_values_are_accepted():
    from cat_amd import loss as closs
    from cat_amd.distillers.base_inception_distiller import BaseInceptionDistiller
    from cat_amd.models.pix2pix_model import Pix2PixModel
    for setter in (BaseInceptionDistiller.modify_commandline_options, Pix2PixModel.modify_commandline_options):
        assert _parser(setter).parse_args(['--recon_loss_type', 'smooth_l1']).recon_loss_type == 'smooth_l1'
    assert _parser(BaseInceptionDistiller.modify_commandline_options).parse_args(['--recon_loss_type', 'vgg']).recon_loss_type == 'vgg'
    # what both constructors build from the value
    assert type(closs.recon_criterion('smooth_l1')) is closs.SmoothL1Loss
    assert type(closs.recon_criterion('l1')) is closs.L1Loss and type(closs.recon_criterion('l2')) is closs.MSELoss
    with pytest.raises(NotImplementedError, match='VGGLoss'):      # the reference raises TypeError at VGGLoss(self.device): nothing to match
        closs.recon_criterion('vgg')
    with pytest.raises(NotImplementedError, match='Unknown reconstruction loss type'):
        closs.recon_criterion('huber')
    crit = closs.recon_criterion('smooth_l1')
    assert crit.beta == 1.0 and closs.SmoothL1Loss(0.25).beta == 0.25
    with pytest.raises(ValueError):
        closs.SmoothL1Loss(-1.0)
