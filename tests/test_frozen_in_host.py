"""CPU: the host rules of the frozen InstanceNorm teacher path (cat_amd/frozen_in.py, cat_amd/ksum.py): the (H, W) -> (th, tw) lattice of
the wide tile's statistics, the ownership registry, the K-concatenated depthwise filter segment, the branch-aligned depthwise launches and the
ctypes mirror of cat_ksum_norm_t."""
import copy
import ctypes as C
import gc
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('h,w,want', [
    (8, 16, (8, 16)), (16, 16, (8, 16)), (16, 32, (4, 32)), (64, 64, (2, 64)), (1, 128, (1, 128)), (2, 128, (1, 128)), (128, 128, (1, 128)),
    (256, 256, (1, 128)), (3, 256, (1, 128)), (128, 1, (128, 1)), (64, 2, (64, 2)), (32, 4, (32, 4)),
    (12, 12, None),      # 128 % 12 != 0
    (8, 24, None),       # 128 % 24 != 0
    (3, 64, None),       # 64 divides 128, but a 2-row tile straddles two samples on 3 rows
    (4, 8, None),        # a sample is smaller than a tile
    (7, 192, None),      # neither divides the other
    (0, 16, None), (16, 0, None),
])
def test_lattice_rule(h, w, want):
    from cat_amd import ksum
    assert ksum.lattice(h, w) == want
    if want is not None:
        th, tw = want
        assert th * tw == 128 and h % th == 0 and w % tw == 0      # whole tiles of 128 pixels, none across samples


def _block():
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    return InvertedResidualChannels(16, None, None, 2, [1, 3], [1, 3, 5], active_fn=get_active_fn('nn.ReLU'))


def test_ownership_is_weak_and_writes_nothing_on_the_module():
    from cat_amd import frozen_in
    blk, other = _block(), _block()
    before = {k: set(vars(m)) for k, m in blk.named_modules()}
    gc.collect()      # (owned blocks of earlier tests that are garbage already must not be counted: the collection below would take them too)
    count = len(frozen_in._OWNED)
    frozen_in.own(blk, 3)
    assert frozen_in.owned(blk) and not frozen_in.owned(other) and frozen_in._OWNED[blk] == (3,)
    assert {k: set(vars(m)) for k, m in blk.named_modules()} == before, 'nothing is written on the modules'
    dup = copy.deepcopy(blk)
    assert not frozen_in.owned(dup) and not any(frozen_in.owned(m) for m in dup.modules())
    assert len(frozen_in._OWNED) == count + 1
    del blk
    gc.collect()
    assert len(frozen_in._OWNED) == count, 'the registry does not keep a block alive'
    frozen_in.own(other)
    assert frozen_in._OWNED[other] == (None,)
    frozen_in.disown(other)
    frozen_in.disown(other)      # (twice is fine)
    assert not frozen_in.owned(other)


def test_own_network_takes_only_instance_norm_blocks_without_running_statistics():
    import functools
    from torch import nn
    from cat_amd import frozen_in, nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    mk = lambda nl: InvertedResidualChannels(16, None, None, 2, [1, 3], [1, 3, 5], norm_layer=nl, active_fn=get_active_fn('nn.ReLU'))
    plain = mk(functools.partial(cnn.InstanceNorm2d, affine=True, track_running_stats=False))
    tracked = mk(functools.partial(cnn.InstanceNorm2d, affine=True, track_running_stats=True))
    batch = mk(cnn.BatchNorm2d)
    net = nn.Sequential(plain, tracked, batch)
    got = frozen_in.own_network(net)
    try:
        assert got == [plain] and frozen_in.owned(plain) and not frozen_in.owned(tracked) and not frozen_in.owned(batch)
    finally:
        frozen_in.disown(plain)


def test_switch_setters_return_the_previous_value():
    from cat_amd import frozen_in
    was = frozen_in.set_enabled(False)
    assert frozen_in.set_enabled(was) is False
    old = frozen_in.set_tail('tconv')
    assert frozen_in.set_tail(old) == 'tconv'
    with pytest.raises(ValueError):
        frozen_in.set_tail('eager')


def test_depthwise_launches_are_branch_aligned():
    from cat_amd import _lib as L, frozen_in
    assert L.DWM_MAXQ == 24
    assert frozen_in.dw_launches([11, 11, 11]) == [(0, 2), (2, 3)]      # the teacher: 3 x 42 channels in 44-channel slots
    assert frozen_in.dw_launches([8, 8, 8]) == [(0, 3)]
    assert frozen_in.dw_launches([24, 1, 23]) == [(0, 1), (1, 3)]
    assert frozen_in.dw_launches([12, 13, 12]) == [(0, 1), (1, 2), (2, 3)]
    assert frozen_in.dw_launches([25]) is None and frozen_in.dw_launches([]) == []


def test_concatenated_depthwise_filters_keep_their_slot_offsets():
    from cat_amd import frozen_in, ops
    cout, widths = 10, [5, 3, 6]      # slots of 8, 4 and 8 channels
    g = torch.Generator().manual_seed(3)
    dws, off = [], 0
    for m in widths:
        conv = torch.nn.Conv2d(m, cout, 1)
        with torch.no_grad():
            conv.weight.copy_(torch.randn(cout, m, 1, 1, generator=g))
        dws.append(dict(od=off, m=m, conv2=conv))
        off += (m + 3) // 4 * 4
    w = frozen_in.dw_filter_segment(dws, cout, torch.device('cpu'))
    assert tuple(w.shape) == (cout, 20, 1, 1) and ops.weight_wcs(w) == 20
    want = torch.zeros(cout, 20)
    want[:, 0:5], want[:, 8:11], want[:, 12:18] = (d['conv2'].weight.detach()[:, :, 0, 0] for d in dws)
    assert torch.equal(w[:, :, 0, 0], want)
    flat = torch.as_strided(w, (cout, 20), (20, 1))      # the kernel's view: [Cout][wcs]
    assert torch.equal(flat, want)


def test_ksum_norm_struct_matches_its_ctypes_mirror(tmp_path):
    """sizeof / offsetof of cat_ksum_nseg_t / cat_ksum_norm_t as gcc lays them out against cat_amd/_lib.py (as tests/test_abi.py does for the
    structs it lists)."""
    from cat_amd import _lib
    structs = {'cat_ksum_nseg_t': _lib.KNormSeg, 'cat_ksum_norm_t': _lib.KSumNorm}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cat_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        c, f, v = ln.split()
        got[(c, f)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, 'size')] == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)
    assert _lib.KSumNorm.seg.size == C.sizeof(_lib.KNormSeg) * _lib.KSUM_MAXSEG
