"""GPU: frozen teacher blocks with the reference's default kernel sizes 3 5 7 on their fused paths.

The BatchNorm-folded teacher (cat_amd/frozen.py, CAT_FROZEN_K7 / frozen.set_k7): an eval-mode InvertedResidualChannels block with 256 inputs
and 42-wide branches at (2, 256, 16, 16) under no_grad -- stage 1 as ONE cat_tstage1w7_fwd, the depthwise stage as ONE
cat_dwconv2d_multi7_fwd, the tail as one cat_tconv_fwd -- against the same block on the general path (_cat_frozen_off) and against a float64
twin out of stock torch.nn layers, the project's 1e-3 relative bar; the launch lists of the 3 5 7 block with the switch on and off and of a
1 3 5 block, the latter two as the parent commit issued them (recorded from a run of it); plan freshness after in-place changes.

The InstanceNorm teacher (cat_amd/frozen_in.py): an owned 3 5 7 block on the forward-only fused pipeline (cat_dwm7_fwd, no cat_norm_fwd) against
the general path and float64; the same block, not owned, keeps the general path.  Planes are tiny, so every test lowers the LDS-tile
threshold to 1 and restores it."""
import contextlib
import copy
import functools

import pytest
import torch

from oracle import detfill
from test_fused_block_gpu import _torch_twin, rel
from test_fused_block_k7_gpu import _Log

pytestmark = pytest.mark.gpu
BAR = 1e-3
SHAPE = (2, 256, 16, 16)
M = (42, 42, 42)
K7_ON = ['cat_tstage1w7_fwd', 'cat_dwconv2d_multi7_fwd', 'cat_tconv_fwd']
# what the parent commit issued for these blocks (steady state, ops.set_tconv_min_tiles(1), reflect and zero padding alike)
PARENT_135 = ['cat_tstage1w_fwd', 'cat_dwconv2d_multi_fwd', 'cat_tconv_fwd']
PARENT_357 = ['cat_conv2d_fwd', 'cat_dwconv2d_fwd', 'cat_dwconv2d_fwd', 'cat_dwconv2d_fwd', 'cat_tconv_fwd', 'cat_tconv_fwd', 'cat_conv2d_fwd_ws',
              'cat_tconv_fwd']


def dev():
    return torch.device('cuda:0')


def _block(norm, padding, ks, seed=77):
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    nl = cnn.BatchNorm2d if norm == 'batch' else functools.partial(cnn.InstanceNorm2d, affine=False, track_running_stats=False)
    blk = InvertedResidualChannels(SHAPE[1], list(M), list(M), 1, list(ks), list(ks), padding_type=padding, use_bias=norm != 'batch', norm_layer=nl,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    # detfill: running_mean ~ 0.1 N(0, 1), running_var ~ U(0.5, 1.5), |N(0, 1)| gammas: nothing folds to the identity
    blk.load_state_dict(detfill.fill_state_dict(blk.state_dict(), seed, gamma_abs_normal=True))
    return blk.to(dev()).eval()


def _x():
    from cat_amd import ops
    return ops.to_nhwc(detfill.normal(SHAPE, 5).to(dev()))


def _eval(blk, x):
    with torch.no_grad():
        y = blk(x)
    torch.cuda.synchronize()
    return y


def _names(blk, x):
    with _Log() as log:
        _eval(blk, x)
    return log.names


def _twin64(blk, x):
    twin, fwd = _torch_twin(blk)
    twin.eval().double()
    with torch.no_grad():
        return fwd(x.detach().cpu().double().contiguous())


@contextlib.contextmanager
def small_planes():
    from cat_amd import _lib, frozen, fused_block, ops
    _lib.load()
    old_tiles, old_k7, old_fk7 = ops.set_tconv_min_tiles(1), frozen.set_k7(True), fused_block.set_k7(True)
    try:
        yield
    finally:
        ops.set_tconv_min_tiles(old_tiles)
        frozen.set_k7(old_k7)
        fused_block.set_k7(old_fk7)


# ------------------------------------------------------------------------------------------------ the BatchNorm-folded teacher
@pytest.mark.parametrize('padding', ['reflect', 'zero'])
def test_folded_357_block_one_launch_per_stage(padding):
    from cat_amd import frozen
    x = _x()
    with small_planes():
        blk = _block('batch', padding, [3, 5, 7])
        general = copy.deepcopy(blk)
        general._cat_frozen_off = True
        with torch.no_grad():
            assert frozen.applicable(blk, x) and not frozen.applicable(general, x)
        y = _eval(blk, x)      # (the first forward also packs the filter streams: the logs below are steady-state ones)
        names = _names(blk, x)
        assert names == K7_ON, names
        assert not any(nm in ('cat_dwconv2d_fwd', 'cat_conv2d_fwd') for nm in names)
        p = frozen._plan(blk)
        assert p['dwm']['fs'] == 7 and p['s1w7'] is not None and p['s1w'] is None and p['s1w7']['m'] == [42, 42, 42, 132]
        y_g, y_t = _eval(general, x), _twin64(blk, x)
        fig = dict(fused_general=rel(y, y_g), fused_twin=rel(y, y_t), general_twin=rel(y_g, y_t))
        print('[frozen k7 %s] %s' % (padding, ', '.join('%s %.3g' % kv for kv in fig.items())))
        assert fig['fused_general'] < BAR and fig['fused_twin'] < BAR and fig['general_twin'] < BAR, fig
        # the switch off: the launches of the parent commit, the same values within the bar; on again: the fused launches, bit for bit
        assert frozen.set_k7(False) is True
        y_off = _eval(blk, x)      # (the first forward on these launches packs their filters)
        off = _names(blk, x)
        assert off == PARENT_357, off
        d = rel(y_off, y_t)
        print('[frozen k7 %s] switch off against the twin %.3g' % (padding, d))
        assert d < BAR
        assert frozen.set_k7(True) is False
        assert _names(blk, x) == K7_ON and torch.equal(_eval(blk, x), y)


@pytest.mark.parametrize('padding', ['reflect', 'zero'])
def test_folded_135_block_issues_what_it_issued(padding):
    """the kernel sizes 1 3 5 never reach a 7 x 7 entry point, whatever the switch says"""
    from cat_amd import frozen
    x = _x()
    with small_planes():
        blk = _block('batch', padding, [1, 3, 5])
        y = _eval(blk, x)
        assert _names(blk, x) == PARENT_135
        assert frozen._plan(blk)['dwm']['fs'] == 5 and frozen._plan(blk)['s1w7'] is None
        frozen.set_k7(False)
        assert _names(blk, x) == PARENT_135 and torch.equal(_eval(blk, x), y)
        d = rel(y, _twin64(blk, x))
        print('[frozen 135 %s] against the twin %.3g' % (padding, d))
        assert d < BAR


def test_folded_357_plan_follows_in_place_changes():
    """one depthwise weight and one BatchNorm running mean changed in place: the next forward folds and packs again"""
    from cat_amd import frozen
    x = _x()
    with small_planes():
        blk = _block('batch', 'reflect', [3, 5, 7])
        y0 = _eval(blk, x)
        with torch.no_grad():
            blk.dw_ops[2][2][0].weight.mul_(3.0)                # the 7 x 7 depthwise filters
            blk.res_ops[2][1][1].running_mean.add_(2.0)         # the norm behind the 7 x 7 first conv
        y1 = _eval(blk, x)
        names = _names(blk, x)
        y_t = _twin64(blk, x)
        d, moved = rel(y1, y_t), rel(y1, y0)
        print('[frozen k7 freshness] after the change against the twin %.3g, against the forward before %.3g' % (d, moved))
        assert names == K7_ON and d < BAR and moved > 10 * BAR
        assert rel(y0, y_t) > 10 * BAR      # the change is visible at the bar: a stale plan would fail


# ------------------------------------------------------------------------------------------------ the InstanceNorm teacher
def test_owned_instance_357_block_takes_the_fused_pipeline():
    from cat_amd import frozen_in, fused_block
    x = _x()
    with small_planes():
        blk, other = _block('instance', 'reflect', [3, 5, 7]), _block('instance', 'reflect', [3, 5, 7], seed=78)
        y_t = _twin64(blk, x)
        y_g = _eval(blk, x)
        _eval(other, x)
        general, other_before = _names(blk, x), _names(other, x)
        assert 'cat_norm_fwd' in general and 'cat_dwm7_fwd' not in general
        frozen_in.own(blk, 1)
        try:
            with torch.no_grad():
                assert frozen_in.applicable(blk, x) and not frozen_in.applicable(other, x)
            y_o = _eval(blk, x)
            own = _names(blk, x)
            print('launches of one block forward: general %d, owned %d: %s' % (len(general), len(own), own))
            assert 'cat_dwm7_fwd' in own and 'cat_norm_fwd' not in own and len(own) < len(general)
            assert _names(other, x) == other_before == general      # the same block, not owned, keeps the general path
            fig = dict(owned_twin=rel(y_o, y_t), general_twin=rel(y_g, y_t), owned_general=rel(y_o, y_g))
            print('[frozen_in k7] %s' % ', '.join('%s %.3g' % kv for kv in fig.items()))
            assert fig['owned_twin'] < BAR and fig['general_twin'] < BAR and fig['owned_general'] < BAR, fig
            old = frozen_in.set_tail('ksum')      # the wide tile's domain is 1 3 5: a 7 x 7 branch keeps the LDS-tile tail
            try:
                assert _names(blk, x) == own
            finally:
                frozen_in.set_tail(old)
            fused_block.set_k7(False)             # under the fused block's own switch
            with torch.no_grad():
                assert not frozen_in.applicable(blk, x)
            assert _names(blk, x) == general
            fused_block.set_k7(True)
        finally:
            frozen_in.disown(blk)
        assert _names(blk, x) == general
