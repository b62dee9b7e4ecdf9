"""CPU: the host side of kernel size 7 -- the 7 x 7 depthwise frame's index map, the packed-filter stream length for ks = 7, the fused
unit's plan (stage-1 order, kernel-size groups, one frame side per plan) for [3, 5, 7], [1, 3, 5] and residual-only blocks, and the register
pin of csrc/conv_pk7.hip (tests/golden/codegen_conv_pk7.json, written by tools/codegen_table.py; hipcc cross-compiles gfx950 here).
The plans are built on the CPU device with the preparation job table left out: the tables hold addresses of weights in the kernels' layout,
which only exists on the GPU; the layout under test is complete before they are built."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_frame_index_map():
    """tap (ky, kx) of a k x k filter sits at row (ky + 3 - k // 2) * 7 + kx + 3 - k // 2 of the [49][C] frame: centred, distinct rows, and
    the 5 x 5 frame's map is the same formula with 2 and 5"""
    from test_dwm_k7_gpu import frame49
    for k in (1, 3, 5, 7):
        wt = torch.arange(1, 2 * k * k + 1, dtype=torch.float32).reshape(2, k, k)
        fr = frame49([wt], [k]).reshape(2, 49)
        rows = [(ky + 3 - k // 2) * 7 + kx + 3 - k // 2 for ky in range(k) for kx in range(k)]
        assert len(set(rows)) == k * k and min(rows) >= 0 and max(rows) < 49
        assert rows[(k * k) // 2] == 24      # the centre tap at the centre of the frame
        assert torch.equal(fr[:, rows], wt.reshape(2, -1))
        rest = sorted(set(range(49)) - set(rows))
        assert float(fr[:, rest].abs().sum()) == 0.0


@pytest.mark.parametrize('c4,nn', [(20, 23), (4, 5), (36, 136), (64, 10), (12, 77)])
def test_pack_floats_for_ks7_is_the_group_formula(c4, nn):
    """per 16-channel chunk 49 groups of four (tap, quad) pairs; the remainder chunk ceil(49 * quads / 4); 256 floats per group and N tile"""
    from cat_amd import _lib, tconv
    _lib.load()
    nfull, rem = c4 // 16, (c4 % 16) // 4
    groups = nfull * 49 + ((49 * rem + 3) // 4 if rem else 0)
    assert tconv.pack_floats(7, c4, nn) == groups * ((nn + 15) // 16) * 256


def _plan(monkeypatch, res, dw, ks):
    from cat_amd import fused_block, fused_unit, nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    monkeypatch.setattr(fused_unit.Plan, '_build_jobs', lambda self: None)
    blk = InvertedResidualChannels(40, list(res), list(dw), 1, list(ks), list(ks), padding_type='reflect', use_bias=False, norm_layer=cnn.BatchNorm2d,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    return fused_block._Plan(blk, torch.device('cpu'))


def test_plan_of_a_357_block(monkeypatch):
    p = _plan(monkeypatch, (7, 6, 9), (16, 5, 3), [3, 5, 7])
    # [res k=1 | dw ... | res k=3 | res k=5 | res k=7]: the depthwise branches' 1 x 1 first convs, then the residual branches by kernel size
    assert [(b['kind'], b['k'], b.get('kd')) for b in p.branches] == [('dw', 1, 3), ('dw', 1, 5), ('dw', 1, 7), ('res', 3, None), ('res', 5, None),
                                                                      ('res', 7, None)]
    assert [(g['k'], g['off'], g['width']) for g in p.groups] == [(1, 0, 28), (3, 28, 8), (5, 36, 8), (7, 44, 12)]
    assert [b['k2'] for b in p.branches] == [1, 1, 1, 3, 5, 7]
    assert (p.fs, p.ft, p.hcd, p.w25.numel()) == (7, 49, 28, 49 * 28)
    assert (p.dw_fwd_entry, p.dw_bwd_entry, p.dw_ws_entry, p.dw_prep_kind) == ('cat_dwm7_fwd', 'cat_dwm7_bwd', 'cat_dwm7_bwd_ws_bytes', 5)
    assert p.s1d is None
    # a 7 x 7 residual branch alone does not widen the depthwise frame
    q = _plan(monkeypatch, (7, 6, 9), (16, 5, 0), [3, 5, 7])
    assert (q.fs, q.w25.numel()) == (5, 25 * 24) and q.dw_fwd_entry == 'cat_dwm_fwd'
    assert [g['k'] for g in q.groups] == [1, 3, 5, 7]


def test_plan_of_a_135_block_is_what_it_was(monkeypatch):
    p = _plan(monkeypatch, (7, 6, 9), (16, 5, 3), [1, 3, 5])
    assert [(b['kind'], b['k'], b.get('kd')) for b in p.branches] == [('res', 1, None), ('dw', 1, 1), ('dw', 1, 3), ('dw', 1, 5), ('res', 3, None),
                                                                      ('res', 5, None)]
    assert [(g['k'], g['off'], g['width']) for g in p.groups] == [(1, 0, 36), (3, 36, 8), (5, 44, 12)]
    assert (p.fs, p.ft, p.w25.numel()) == (5, 25, 25 * 28)
    assert (p.dw_fwd_entry, p.dw_bwd_entry, p.dw_ws_entry, p.dw_prep_kind) == ('cat_dwm_fwd', 'cat_dwm_bwd', 'cat_dwm_bwd_ws_bytes', 2)


def test_plan_of_a_residual_only_357_block(monkeypatch):
    """three kernel-size groups that are NOT (5, 3, 1): stage 1 chooses its one-launch kernels by the key set, not the group count (the
    launches themselves: tests/test_fused_block_k7_gpu.py, the residual-only cases)"""
    p = _plan(monkeypatch, (7, 6, 9), (0, 0, 0), [3, 5, 7])
    assert [g['k'] for g in p.groups] == [3, 5, 7] and not p.dws and p.fs == 5
    assert [(b['k'], b['k2'], b['o1'], b['w1']) for b in p.branches] == [(3, 3, 0, 8), (5, 5, 8, 8), (7, 7, 16, 12)]


def test_conv_pk7_kernels_keep_their_register_budget():
    import codegen_table
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'codegen_conv_pk7.json')))
    got = codegen_table.table('cat_amd/csrc/conv_pk7.hip')
    assert sorted(got) == sorted(want), 'kernel set of conv_pk7.hip changed: re-record with tools/codegen_table.py --write (after an A/B on hardware)'
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, 'register / scratch counts changed (committed, now): %s' % diff
    assert len(got) == 8 and all('tconv7_kernelILi%dELi16E' % nt in ''.join(got) for nt in range(1, 9))
    for k, v in got.items():      # every instantiation: no scratch, no spills, two workgroups per CU
        assert v['scratch'] == 0 and v['vspill'] == 0 and v['vgpr'] <= 256, (k, v)
