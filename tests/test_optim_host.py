"""Host: the two rules cat_amd/optim.py keeps for FusedAdam-owned parameters -- where a gradient goes (claim / deliver) and what a cache of
a derived operand keys on (epoch_of / weights_key) -- on CPU tensors adopted the way FusedAdam._flatten adopts its parameters."""
import pytest
import torch

from cat_amd import optim


def _param(n=3, owned=True):
    p = torch.nn.Parameter(torch.arange(1.0, n + 1))
    if owned:
        optim._adopt(p, torch.zeros(n))
    return p


def _reset(*params):
    """What FusedAdam.zero_grad does to its parameters' sink state."""
    for p in params:
        p._cat_grad_state['fresh'] = True


def test_adopt_installs_the_sink():
    p, q = _param(), _param(owned=False)
    assert optim.owned(p) and not optim.owned(q) and not optim.owned(None)
    assert p.grad is p._cat_grad_view and p._cat_grad_state == {'fresh': True}


def test_claim_one_parameter_writes_then_accumulates():
    p = _param()
    views, acc = optim.claim([p], 'one')
    assert acc == 0 and len(views) == 1 and views[0] is p._cat_grad_view
    assert optim.claim([p], 'one')[1] == 1
    assert optim.claim([p], 'one')[1] == 1
    _reset(p)
    assert optim.claim([p], 'one')[1] == 0


def test_claim_group_must_agree():
    a, b, c = _param(), _param(), _param()
    views, acc = optim.claim([a, b, c], 'group')
    assert acc == 0 and [v.data_ptr() for v in views] == [q._cat_grad_view.data_ptr() for q in (a, b, c)]
    assert optim.claim([a, b, c], 'group')[1] == 1
    _reset(b)
    with pytest.raises(RuntimeError, match='some unit backward: gradient buffers out of sync'):
        optim.claim([a, b, c], 'some unit backward')
    assert [q._cat_grad_state['fresh'] for q in (a, b, c)] == [False, True, False]      # a refused claim clears nothing


def test_claim_with_an_unowned_member_touches_nothing():
    a, b, u = _param(), _param(), _param(owned=False)
    optim.claim([b], 'one')
    assert optim.claim([a, u, b], 'mixed') is None
    assert optim.claim([u], 'mixed') is None and optim.claim([], 'nothing') is None
    assert a._cat_grad_state['fresh'] is True and b._cat_grad_state['fresh'] is False
    assert not hasattr(u, '_cat_grad_state') and u.grad is None


def test_deliver_copies_when_fresh_and_adds_afterwards():
    p, u = _param(), _param(owned=False)
    g = torch.tensor([1.0, 2.0, 4.0])
    p._cat_grad_view.fill_(7.0)                      # stale content: the first delivery overwrites it
    assert optim.deliver(p, g) is None
    assert torch.equal(p._cat_grad_view, g) and p._cat_grad_state['fresh'] is False
    assert optim.deliver(p, g) is None
    assert torch.equal(p._cat_grad_view, 2 * g)
    assert optim.claim([p], 'one')[1] == 1          # a delivery counts as the first writer
    _reset(p)
    assert optim.deliver(p, g) is None and torch.equal(p._cat_grad_view, g)
    assert optim.deliver(u, g) is g and optim.deliver(u, None) is None and optim.deliver(p, None) is None


def test_weights_key_and_epoch_follow_ownership():
    own, free = _param(), _param(owned=False)
    assert optim.epoch_of([free, None]) == -1 and optim.epoch_of([]) == -1 and optim.epoch_of([None]) == -1
    assert optim.epoch_of([free, None, own]) == optim.weights_epoch()
    k_free, k_mixed = optim.weights_key([free, None]), optim.weights_key([free, None, own])
    assert k_free == (((free.data_ptr(), free._version), None), -1)
    assert k_mixed == (((free.data_ptr(), free._version), None, (own.data_ptr(), own._version)), optim.weights_epoch())
    free.data.mul_(2.0)                              # a raw update (what the Adam kernel does): no version bump, same key
    assert optim.weights_key([free, None]) == k_free
    optim._bump_weights_epoch()                      # FusedAdam.step / note_graph_replay
    assert optim.weights_key([free, None]) == k_free
    assert optim.weights_key([free, None, own]) != k_mixed
    assert optim.weights_key([free, None, own])[0] == k_mixed[0] and optim.epoch_of([own]) == k_mixed[1] + 1
    with torch.no_grad():
        free.mul_(2.0)                               # an ordinary in-place update bumps the version: new key
    assert optim.weights_key([free, None]) != k_free


def _move_stats(bn):
    """What a train-mode norm forward does to a BatchNorm's running statistics: the wrapper announces the buffers it hands to the kernel
    (optim.note_stats_written, as ops.NormActFn / ops._bn_forward_stats / ops.norm_from_tiles / fused_unit.slices do) and the kernel
    updates them through raw pointers -- no version bump, no optimizer step."""
    optim.note_stats_written(bn.running_mean, bn.running_var)
    bn.running_var.data.mul_(4.0)
    bn.running_mean.data.add_(0.5)


def _eval_block():
    import helpers as H
    from cat_amd import networks
    net = networks.define_G(3, 3, 16, 'inception_9blocks', 'batch', 0, 'normal', 0.02, [], opt=H.make_opt(norm='batch', track=True))
    net.eval()
    return net


@pytest.mark.parametrize('owned', [False, True], ids=['no_optimizer', 'optimizer_owned_between_steps'])
def test_folds_follow_running_statistics_without_an_optimizer_step(owned):
    """eval forward (fold cached) -> train-mode forward (statistics move) -> eval forward, no FusedAdam.step in between: both folds that
    read running statistics on the host (nn._folded_eval_bn, frozen._plan) must be re-derived, for a net without an optimizer and for an
    optimizer-owned net between two steps alike -- and must stay cached while nothing moves."""
    from cat_amd import frozen
    from cat_amd import nn as cnn
    net = _eval_block()
    conv, bn, blk = net.down_sampling[4], net.down_sampling[5], net.features[0]
    if owned:
        for p in list(conv.parameters()) + list(bn.parameters()) + list(blk.parameters()):
            optim._adopt(p, torch.zeros_like(p))
    epoch = optim.weights_epoch()
    with torch.no_grad():
        w1, b1 = cnn._folded_eval_bn(conv, bn, 0)
        assert cnn._folded_eval_bn(conv, bn, 0)[0] is w1
        scale1 = (bn.weight * torch.rsqrt(bn.running_var + bn.eps)).clone()
        _move_stats(bn)
        w2, b2 = cnn._folded_eval_bn(conv, bn, 0)
        assert w2 is not w1 and b2 is not b1
        assert cnn._folded_eval_bn(conv, bn, 0)[0] is w2                      # still a cache
        scale2 = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        assert torch.allclose(w2, conv.weight * scale2.view(-1, 1, 1, 1)) and torch.allclose(w1, conv.weight * scale1.view(-1, 1, 1, 1))
        assert torch.allclose(w2, 0.5 * w1, rtol=1e-3)                       # var x 4 (eps aside): the fold halves
        assert not torch.allclose(b2, b1)
    p1 = frozen._plan(blk)
    assert frozen._plan(blk) is p1
    first_bn, pw = blk.res_ops[0][1][1], blk.pw_bn
    _move_stats(first_bn)
    p2 = frozen._plan(blk)
    assert p2 is not p1 and frozen._plan(blk) is p2
    assert not torch.equal(p2['w_a'], p1['w_a']) and torch.equal(p2['w_f'], p1['w_f'])
    _move_stats(pw)
    p3 = frozen._plan(blk)
    assert p3 is not p2 and frozen._plan(blk) is p3
    assert torch.equal(p3['w_a'], p2['w_a']) and torch.allclose(p3['w_f'], 0.5 * p2['w_f'], rtol=1e-3)
    assert optim.weights_epoch() == epoch                                     # nothing here stepped an optimizer


def test_statistics_counter_is_not_part_of_the_weight_pack_key():
    """The counter lives on the statistics buffers and only weights_key reads it: epoch_of -- the whole optimizer part of the filter-pack /
    transposed-filter / qconv-stream keys -- does not move when a norm layer of the same net runs in train mode."""
    w, rv = _param(), torch.ones(3)
    pack_key = optim.pack_key(w, w)
    fold_key = optim.weights_key([w, rv])
    assert optim.stat_writes(rv) == 0 and fold_key[0][1] == (rv.data_ptr(), rv._version)
    optim.note_stats_written(rv, None)
    assert optim.stat_writes(rv) == 1 and optim.stat_writes(w) == 0
    assert optim.pack_key(w, w) == pack_key == (((w.data_ptr(), w._version),), optim.epoch_of([w]))
    assert optim.weights_key([w, rv]) != fold_key and optim.weights_key([w]) == (fold_key[0][:1], fold_key[1])
