"""CPU: the public surface of virtual replicas (`--virtual_replicas`, networks.set_virtual_replicas, host.StepHost.set_virtual_replicas) and
the one sharding rule every kernel of the feature follows (ops.shard_bounds = torch.chunk).  The arithmetic itself needs the GPU:
tests/test_virtual_replicas_gpu.py."""
import argparse

import pytest
import torch


def _parser(defaults=()):
    p = argparse.ArgumentParser()
    for flag, d in defaults:
        p.add_argument(flag, default=d)
    return p


def test_flag_parses_everywhere_and_defaults_to_one():
    from cat_amd import distillers, models
    setters = [
        (distillers.get_option_setter('inception'), [('--norm', None), ('--dataset_mode', None), ('--log_dir', None)]),
        (distillers.get_option_setter('spade'), [('--netD', 'n_layers'), ('--ndf', 128), ('--dataset_mode', None), ('--batch_size', 1),
                                                  ('--print_freq', 100), ('--save_latest_freq', 1), ('--save_epoch_freq', 1), ('--nepochs', 1),
                                                  ('--nepochs_decay', 1), ('--init_type', 'normal'), ('--n_layers_D', 3)]),
        (models.get_option_setter('pix2pix'), []),
        (models.get_option_setter('cycle_gan'), []),
    ]
    for setter, defaults in setters:
        p = setter(_parser(defaults), True)
        assert p.parse_args([]).virtual_replicas == 1
        assert p.parse_args(['--virtual_replicas', '4']).virtual_replicas == 4


def test_spade_model_flag():
    from cat_amd import models
    p = _parser([('--netG', None), ('--netD', 'n_layers'), ('--ndf', 128), ('--dataset_mode', None), ('--batch_size', 1), ('--print_freq', 100),
                 ('--save_latest_freq', 1), ('--save_epoch_freq', 1), ('--nepochs', 1), ('--nepochs_decay', 1), ('--init_type', 'normal'),
                 ('--n_layers_D', 3), ('--active_fn', None)])
    p = models.get_option_setter('spade')(p, True)
    assert p.parse_args(['--real_stat_path', 'x']).virtual_replicas == 1
    assert p.parse_args(['--real_stat_path', 'x', '--virtual_replicas', '2']).virtual_replicas == 2


def test_shard_bounds_equal_torch_chunk():
    """groups of ceil(N / S) consecutive samples, the last may be short, there may be fewer than S: torch.chunk's sizes for every case"""
    from cat_amd import ops
    for n in range(1, 13):
        for s in range(1, 7):
            want = [len(c) for c in torch.arange(n).chunk(s, 0)]
            got = ops.shard_bounds(n, s)
            assert [e - b for b, e in got] == want, (n, s, got, want)
            assert got[0][0] == 0 and got[-1][1] == n and all(a[1] == b[0] for a, b in zip(got, got[1:]))
            assert ops.norm_groups(n, s) == (len(want) if s > 1 else 1)
    with pytest.raises(ValueError):
        ops.shard_bounds(4, 0)


def test_stamp_reaches_training_batchnorms_only():
    """networks.set_virtual_replicas: BatchNorm2d and the replica-local SynchronizedBatchNorm2d carry the count; InstanceNorm2d and a
    SynchronizedBatchNorm2d that exchanges statistics (the SPADE family's: truly synchronised) keep 1."""
    from cat_amd import networks, nn as cnn
    net = torch.nn.Sequential(cnn.BatchNorm2d(4), cnn.InstanceNorm2d(4), cnn.SynchronizedBatchNorm2d(4, replica_local=True),
                              cnn.SynchronizedBatchNorm2d(4), torch.nn.Sequential(cnn.BatchNorm2d(3)))
    assert [m.virtual_replicas for m in net.modules() if hasattr(m, 'virtual_replicas')] == [1, 1, 1, 1, 1]
    assert networks.set_virtual_replicas(net, 4) == 3
    assert [net[0].virtual_replicas, net[1].virtual_replicas, net[2].virtual_replicas, net[3].virtual_replicas, net[4][0].virtual_replicas] == \
        [4, 1, 4, 1, 4]
    assert networks.set_virtual_replicas(net, 1) == 3 and net[0].virtual_replicas == 1
    with pytest.raises(ValueError):
        networks.set_virtual_replicas(net, 0)


def test_host_stamps_every_network_it_owns():
    """StepHost.set_virtual_replicas walks the host's attributes (networks and lists of networks) without needing a device."""
    from cat_amd import host, nn as cnn
    h = host.StepHost.__new__(host.StepHost)
    h.netG = torch.nn.Sequential(cnn.BatchNorm2d(4))
    h.netAs = [torch.nn.Sequential(cnn.BatchNorm2d(2))]
    h.set_virtual_replicas(3)
    assert h.virtual_replicas == 3 and h.netG[0].virtual_replicas == 3 and h.netAs[0][0].virtual_replicas == 3
    with pytest.raises(ValueError):
        h.set_virtual_replicas(0)


def test_host_with_exchanging_syncbatchnorm_installs_the_replica_exchange():
    """The SPADE family's SynchronizedBatchNorm2d is synchronised over the replicas: it is never stamped (whole-batch statistics), but at
    S > 1 it must take the reference's multi-replica arm -- the host installs ops.ReplicaSync (an identity exchange) and removes it at 1."""
    from cat_amd import host, nn as cnn, ops

    class Loss(torch.nn.Sequential):
        def calc_distill_loss(self):
            return None

    h = host.StepHost.__new__(host.StepHost)
    h.modules_on_one_gpu = Loss(cnn.SynchronizedBatchNorm2d(4), cnn.BatchNorm2d(4))
    assert ops.bn_sync() is None
    try:
        h.set_virtual_replicas(2)
        sync = ops.bn_sync()
        assert isinstance(sync, ops.ReplicaSync) and sync.world_size == 1
        t = torch.arange(4.0)
        assert sync.all_reduce_sum_(t) is t and sync.all_reduce_sum_many_([t])[0] is t
        assert h.modules_on_one_gpu.virtual_replicas == 2
        assert h.modules_on_one_gpu[0].virtual_replicas == 1 and h.modules_on_one_gpu[1].virtual_replicas == 2
    finally:
        h.set_virtual_replicas(1)
    assert ops.bn_sync() is None and h.modules_on_one_gpu.virtual_replicas == 1
