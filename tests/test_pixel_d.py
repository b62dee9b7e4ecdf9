"""CPU: the 1x1 PixelGAN discriminator (`--netD pixel`, reference models/modules/discriminators.py:82-126) as a module: construction through
networks.define_D, the reference's state_dict keys and shapes (tests/golden/pixel_d.npz, tools/make_golden_pixel_d.py), initialisation, the
stock-torch twin, and that the fused path's applicable() declines on the host without raising."""
import json

import pytest
import torch
from torch import nn

import helpers as H

NORMS = ('instance', 'batch', 'syncbatch')


def _define(norm, ndf=16, input_nc=6, **kw):
    from cat_amd import networks
    opt = H.make_opt(norm=norm, track=norm != 'instance', ndf=ndf, **kw)
    opt.norm_affine_D = kw.get('norm_affine_D', False)
    return networks.define_D(input_nc, ndf, 'pixel', 3, norm, 'normal', 0.02, [], opt=opt)


@pytest.mark.parametrize('norm', NORMS)
def test_define_d_builds_the_reference_state_dict(norm):
    from cat_amd import discriminators, nn as cnn
    g = H.load('pixel_d.npz')
    D = _define(norm)
    assert type(D) is discriminators.PixelDiscriminator and type(D.net) is cnn.FusedSequential and len(D.net) == 6
    got = [[k, list(v.shape)] for k, v in D.state_dict().items()]
    assert got == json.loads(str(g[f'shapes:{norm}']))
    keys = [k for k, _ in got]
    assert 'net.0.bias' in keys
    assert ('net.2.bias' in keys) == ('net.5.bias' in keys) == (norm == 'instance')      # the 1-channel head has a bias only with InstanceNorm
    assert all(isinstance(D.net[i], nn.LeakyReLU) and D.net[i].negative_slope == 0.2 for i in (1, 4))
    if norm == 'syncbatch':
        assert type(D.net[3]) is cnn.SynchronizedBatchNorm2d and D.net[3].replica_local


def test_norm_none_has_no_bias_and_an_identity():
    from cat_amd import nn as cnn
    D = _define('none')
    assert type(D.net[3]) is cnn.Identity
    assert list(D.state_dict()) == ['net.0.weight', 'net.0.bias', 'net.2.weight', 'net.5.weight']


def test_init_weights_touches_convs_and_batchnorm():
    """as for NLayerDiscriminator: conv weights N(0, 0.02) with biases 0, BatchNorm weights N(1, 0.02) (affine here), InstanceNorm untouched."""
    from cat_amd import networks
    torch.manual_seed(5)
    D = _define('batch', ndf=64, norm_affine_D=True)
    for i in (0, 2, 5):
        w = D.net[i].weight.detach()
        assert abs(float(w.mean())) < 0.01 and 0.01 < float(w.std()) < 0.03
    assert float(D.net[0].bias.detach().abs().max()) == 0
    gamma, beta = D.net[3].weight.detach(), D.net[3].bias.detach()
    assert abs(float(gamma.mean()) - 1) < 0.01 and 0.005 < float(gamma.std()) < 0.04 and float(beta.abs().max()) == 0
    Di = _define('instance', ndf=64, norm_affine_D=True)
    assert torch.equal(Di.net[3].weight.detach(), torch.ones(128)) and float(Di.net[2].bias.detach().abs().max()) == 0
    assert float(Di.net[5].bias.detach().abs().max()) == 0
    with pytest.raises(NotImplementedError):
        networks.init_weights(D, 'nonsense')


@pytest.mark.parametrize('norm', NORMS)
def test_twin_loads_the_state_dict_strictly(norm):
    from cat_amd import export
    from oracle import detfill
    D = _define(norm)
    D.load_state_dict(detfill.fill_state_dict(D.state_dict(), 61))
    twin = export.to_reference_module(D)
    assert not any(type(m).__module__.startswith('cat_amd') for m in twin.net.modules())
    twin.load_state_dict(D.state_dict(), strict=True)
    ref = nn.Sequential(nn.Conv2d(6, 16, 1), nn.LeakyReLU(0.2), nn.Conv2d(16, 32, 1, bias=norm == 'instance'),
                        nn.InstanceNorm2d(32) if norm == 'instance' else nn.BatchNorm2d(32, affine=False), nn.LeakyReLU(0.2),
                        nn.Conv2d(32, 1, 1, bias=norm == 'instance'))
    ref.load_state_dict({k[len('net.'):]: v for k, v in D.state_dict().items()}, strict=True)
    x = detfill.normal((2, 6, 8, 8), 62)
    assert torch.equal(twin(x), ref(x))


def test_applicable_declines_on_the_host_without_raising():
    from cat_amd import pixel_d
    D = _define('batch')
    assert pixel_d.applicable(D, torch.zeros(2, 6, 8, 8)) is False
    assert pixel_d.applicable(D, None) is False and pixel_d.applicable(object(), torch.zeros(1)) is False
    with pytest.raises(RuntimeError):      # and the module itself has no CPU path, like every other layer here
        D(torch.zeros(2, 6, 8, 8))


def test_plan_is_a_pure_host_function():
    from cat_amd import pixel_d
    pl = pixel_d.plan(pixel_d.geometry(16, 256 * 256, 6, 8, 128, 1))
    assert pl.tile_px == 256 and pl.tiles == 256 and pl.fwd_lds <= 160 * 1024 and pl.b2_lds <= 160 * 1024
    assert pl.table_floats == 16 * 256 * 2 * 256 and pl.b2_tiles == 16 * 1024 and 0 < pl.b2_grid <= pl.b2_tiles
    assert pl.ws2_floats == pl.b2_grid * (256 * 128 + 256 + 128 + 1024)
    assert pixel_d.geometry(1, 64, 6, 8, 16, 1).w1cs == 8 and pixel_d.geometry(1, 64, 1, 4, 16, 1, w1cs=1).w1cs == 1
    assert pixel_d.plan(pixel_d.geometry(1, 64, 1, 4, 16, 1, w1cs=1)).tiles == 1      # a dense 1-channel weight row is a geometry of its own
    with pytest.raises(RuntimeError):
        pixel_d.plan(pixel_d.geometry(1, 64, 6, 8, 24, 1))      # ndf % 16
