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
