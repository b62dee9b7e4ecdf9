"""Host: cat_amd/derived.py -- the one keyed cache of derived operands -- and the one conv + eval-BatchNorm fold behind every cached fold
(nn.bn_affine / nn.fold_conv_bn), against the formulas the four call sites used to write out themselves."""
import importlib
import pkgutil

import pytest
import torch
from torch import nn

import cat_amd
from cat_amd import derived, ops, optim
from cat_amd import nn as cnn
from oracle import detfill

from test_optim_host import _eval_block


class Holder:
    pass


# ------------------------------------------------------------------------------------------------------------------------ lookup / peek / drop
def test_lookup_returns_the_cached_value_while_the_key_holds():
    h, slot, made = Holder(), derived.slot('_cat_test_slot'), []

    def make(prev):
        made.append(prev)
        return [len(made)]
    assert derived.peek(h, slot) is None
    v1 = derived.lookup(h, slot, ('k', 1), make)
    assert made == [None] and derived.peek(h, slot) == derived.Entry(('k', 1), v1) and derived.peek(h, slot).value is v1
    assert derived.lookup(h, slot, ('k', 1), make) is v1 and len(made) == 1          # same key: same object, make not called
    v2 = derived.lookup(h, slot, ('k', 2), make)
    assert len(made) == 2 and made[1].key == ('k', 1) and made[1].value is v1        # changed key: make sees the previous Entry
    assert v2 is not v1 and derived.peek(h, slot).key == ('k', 2) and derived.lookup(h, slot, ('k', 2), make) is v2


def test_a_make_that_refreshes_in_place_keeps_the_object():
    h, slot = Holder(), derived.slot('_cat_test_slot')

    def make(prev):
        buf = prev.value if prev is not None else torch.zeros(3)
        buf += 1
        return buf
    b1 = derived.lookup(h, slot, 1, make)
    b2 = derived.lookup(h, slot, 2, make)
    assert b2 is b1 and torch.equal(b1, torch.full((3,), 2.0)) and derived.peek(h, slot) == (2, b1)


def test_sub_keys_share_one_slot_and_keep_their_own_entries():
    h, slot = Holder(), derived.slot('_cat_test_slot')
    a = derived.lookup(h, slot, 1, lambda prev: ['a'], sub=0)
    b = derived.lookup(h, slot, 1, lambda prev: ['b'], sub=1)
    assert derived.peek(h, slot, 0).value is a and derived.peek(h, slot, 1).value is b and set(derived.peek(h, slot)) == {0, 1}
    a2 = derived.lookup(h, slot, 2, lambda prev: prev.value, sub=0)
    assert a2 is a and derived.peek(h, slot, 0).key == 2 and derived.peek(h, slot, 1) == (1, b)
    assert derived.peek(Holder(), slot, 0) is None


def test_drop_pops_every_registered_slot_and_nothing_else():
    h, s1, s2 = Holder(), derived.slot('_cat_test_slot'), derived.slot('_cat_test_slot2')
    assert derived.slot('_cat_test_slot') == s1 and derived.SLOTS.count(s1) == 1   # declaring twice registers once
    derived.lookup(h, s1, 1, lambda prev: 'x')
    derived.lookup(h, s2, 1, lambda prev: 'y', sub='m')
    h.other = 3
    derived.drop(h)
    assert derived.peek(h, s1) is None and derived.peek(h, s2) is None and derived.peek(h, s2, 'm') is None and h.__dict__ == {'other': 3}
    derived.drop(h)                                                                  # nothing cached: nothing to do
    assert derived.lookup(h, s1, 1, lambda prev: prev) is None                       # after a drop, make starts from nothing


# ------------------------------------------------------------------------------------------------------------------------ registry completeness
BROADCAST_POPPED = ('_cat_pk', '_cat_wt', '_cat_wtp', '_cat_frozen', '_cat_fold', '_cat_fused_plan', '_cat_fused_gb', '_cat_fused_main', '_cat_q')
NOT_CACHES = ()      # module-level `_cat_` attribute-name constants that are no derived operand: none today


def _package_constants():
    """{value: [module.NAME, ...]} of every module-level string constant of the package (every module imported)."""
    found = {}
    for info in pkgutil.walk_packages(cat_amd.__path__, 'cat_amd.'):
        mod = importlib.import_module(info.name)
        for name, value in vars(mod).items():
            if isinstance(value, str) and not name.startswith('__'):
                found.setdefault(value, []).append('%s.%s' % (info.name, name))
    return found


def test_every_cache_attribute_is_a_declared_slot():
    consts = _package_constants()
    slots = set(derived.SLOTS)
    assert slots >= set(BROADCAST_POPPED), sorted(set(BROADCAST_POPPED) - slots)       # what broadcast_parameters used to pop by name
    # every `_cat_` attribute name a module keeps as a constant went through slot() ...
    undeclared = {v: where for v, where in consts.items() if v.startswith('_cat_') and v not in slots and v not in NOT_CACHES}
    assert not undeclared, undeclared
    # ... and every slot is such a constant, next to its user (not a string literal at the point of use)
    package_slots = {s for s in slots if not s.startswith('_cat_test_')}
    assert all(s in consts for s in package_slots), sorted(s for s in package_slots if s not in consts)
    from cat_amd import frozen, fused_spade, fused_unit, qconv
    assert (ops.PK, ops.WT, ops.WTP, cnn.FOLD, cnn.Q, frozen.FROZEN, fused_unit.PLAN, fused_spade.MAIN, fused_spade.GB) == \
        ('_cat_pk', '_cat_wt', '_cat_wtp', '_cat_fold', '_cat_q', '_cat_frozen', '_cat_fused_plan', '_cat_fused_main', '_cat_fused_gb')
    assert fused_spade.EVAL_SS in slots and qconv.PK in slots


# ------------------------------------------------------------------------------------------------------------------------ the one fold
def _fill(t, seed, positive=False):
    v = detfill.normal(tuple(t.shape), seed)
    with torch.no_grad():
        t.copy_(v.abs() + 0.5 if positive else v)


def _pair(conv, channels, seed, affine=True):
    return _fill_pair(conv, nn.BatchNorm2d(channels, affine=affine).eval(), seed)


def _fill_pair(conv, bn, seed):
    _fill(conv.weight, seed)
    if conv.bias is not None:
        _fill(conv.bias, seed + 1)
    if bn.affine:
        _fill(bn.weight, seed + 2)
        _fill(bn.bias, seed + 3)
    _fill(bn.running_mean, seed + 4)
    _fill(bn.running_var, seed + 5, positive=True)
    return conv, bn


def _padded(values):
    out = ops.padded_weight_like(values.shape, values.device)
    out.copy_(values)
    return out


def _nn_form(conv, bn, out_dim):
    """nn._folded_eval_bn as it stood"""
    with torch.no_grad():
        scale = torch.rsqrt(bn.running_var + bn.eps)
        if bn.weight is not None:
            scale = scale * bn.weight
        shift = -bn.running_mean * scale
        if bn.bias is not None:
            shift = shift + bn.bias
        shape = [1, 1, 1, 1]
        shape[out_dim] = -1
        w = conv.weight.detach()
        if w.dim() == 4 and w.shape[1] > 1:
            wf = _padded(w * scale.view(shape))
        else:
            wf = (w * scale.view(shape)).contiguous()
        bf = shift if conv.bias is None else conv.bias.detach() * scale + shift
        return wf, bf.contiguous()


def _inception_form(conv, bn):
    """metric.inception.BasicConv2d._folded as it stood"""
    with torch.no_grad():
        scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        return _padded(conv.weight * scale.view(-1, 1, 1, 1)), (bn.bias - bn.running_mean * scale).contiguous()


def _drn_form(conv, bn):
    """metric.drn._folded as it stood"""
    with torch.no_grad():
        if bn is None:
            return _padded(conv.weight), conv.bias.detach().contiguous() if conv.bias is not None else None
        scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        bias = bn.bias - bn.running_mean * scale
        if conv.bias is not None:
            bias = bias + conv.bias * scale
        return _padded(conv.weight * scale.view(-1, 1, 1, 1)), bias.contiguous()


def _same(got, want):
    for g, w in zip(got, want):
        if w is None:
            assert g is None
            continue
        assert torch.equal(g, w) and g.shape == w.shape and g.stride() == w.stride() and g.dtype == w.dtype, (g.shape, g.stride(), w.stride())
        assert not g.requires_grad


# (name, conv factory, BatchNorm channels, out_dim): O = 5, I = 3, k = 3 (padded channels) | O = 8, I = 8, k = 1 | depthwise [6, 1, 3, 3] |
# transposed-conv weight [4, 6, 3, 3], folded along dim 1
CONVS = [('o5_i3_k3', lambda bias: nn.Conv2d(3, 5, 3, bias=bias), 5, 0),
         ('o8_i8_k1', lambda bias: nn.Conv2d(8, 8, 1, bias=bias), 8, 0),
         ('depthwise6_k3', lambda bias: nn.Conv2d(6, 6, 3, groups=6, bias=bias), 6, 0),
         ('convt_4_6_k3', lambda bias: nn.ConvTranspose2d(4, 6, 3, bias=bias), 6, 1)]


@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('affine', [True, False], ids=['affine', 'plain'])
@pytest.mark.parametrize('case', CONVS, ids=[c[0] for c in CONVS])
def test_nn_fold_is_bit_identical(case, affine, bias):
    name, make, channels, out_dim = case
    conv, bn = _pair(make(bias), channels, 300 + 10 * CONVS.index(case), affine=affine)
    assert tuple(conv.weight.shape) in ((5, 3, 3, 3), (8, 8, 1, 1), (6, 1, 3, 3), (4, 6, 3, 3))
    want = _nn_form(conv, bn, out_dim)
    _same(cnn.fold_conv_bn(conv, bn, out_dim), want)
    with torch.no_grad():
        got = cnn._folded_eval_bn(conv, bn, out_dim)
        assert cnn._folded_eval_bn(conv, bn, out_dim)[0] is got[0]
    _same(got, want)
    scale, shift = cnn.bn_affine(bn)
    assert torch.equal(want[1], shift if conv.bias is None else (conv.bias * scale + shift).detach())


@pytest.mark.parametrize('case', CONVS[:2], ids=[c[0] for c in CONVS[:2]])
def test_inception_fold_is_bit_identical(case):
    from cat_amd.metric import inception
    name, make, channels, _ = case
    ref = make(False)
    m = inception.BasicConv2d(ref.in_channels, ref.out_channels, ref.kernel_size[0]).eval()
    assert m.bn.eps == 0.001
    _fill_pair(m.conv, m.bn, 400 + 10 * CONVS.index(case))
    want = _inception_form(m.conv, m.bn)
    w, wcs, b = m._folded()
    _same((w, b), want)
    assert wcs == ops.weight_wcs(want[0]) and m._folded()[0] is w


@pytest.mark.parametrize('bias', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('with_bn', [True, False], ids=['bn', 'bare'])
@pytest.mark.parametrize('case', CONVS[:3], ids=[c[0] for c in CONVS[:3]])
def test_drn_fold_is_bit_identical(case, with_bn, bias):
    from cat_amd.metric import drn
    name, make, channels, _ = case
    conv, bn = _pair(make(bias), channels, 500 + 10 * CONVS.index(case))
    bn = bn if with_bn else None
    want = _drn_form(conv, bn)
    w, wcs, b = drn._folded(conv, bn)
    _same((w, b), want)
    assert wcs == ops.weight_wcs(want[0]) and drn._folded(conv, bn)[0] is w
    assert w.data_ptr() != conv.weight.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------ drop_derived
def test_drop_derived_re_derives_after_a_write_through_data():
    from cat_amd import frozen
    net = _eval_block()
    conv, bn, blk = net.down_sampling[4], net.down_sampling[5], net.features[0]
    with torch.no_grad():
        w1, b1 = cnn._folded_eval_bn(conv, bn, 0)
        p1 = frozen._plan(blk)
        w1v, wf1 = w1.clone(), p1['w_f'].clone()
        versions = [t._version for t in list(net.parameters()) + list(net.buffers())]
        conv.weight.data.mul_(2.0)                 # as a broadcast writes: through .data, no version bump
        blk.pw_bn.weight.data.mul_(2.0)
        assert [t._version for t in list(net.parameters()) + list(net.buffers())] == versions
        assert cnn._folded_eval_bn(conv, bn, 0)[0] is w1 and frozen._plan(blk) is p1        # nothing a key could see
        epoch = optim.weights_epoch()
        derived.drop_derived([net])
        assert optim.weights_epoch() == epoch + 1
        assert derived.peek(conv, cnn.FOLD) is None and derived.peek(blk, frozen.FROZEN) is None
        w2, b2 = cnn._folded_eval_bn(conv, bn, 0)
        p2 = frozen._plan(blk)
        assert w2 is not w1 and p2 is not p1
        assert torch.equal(w2, 2.0 * w1v) and torch.equal(b2, b1)                          # x 2 is exact in binary floating point
        assert torch.equal(p2['w_f'], 2.0 * wf1) and torch.equal(p2['w_a'], p1['w_a'])
        _same((w2, b2), _nn_form(conv, bn, 0))
