"""CPU: the host side of the fused GauGAN units at kernel sizes 3 5 7 -- the switch CAT_FUSED_SPADE_K7 / fused_spade.set_k7, the kernel-size
rule of fused_spade.applicable under it (on stub modules), what fused_unit.stage1 chooses for a plan that carries `stage1_n7` (plans stubbed
down to their groups, launches recorded instead of issued, as tests/test_stage1ws7_host.py does), the ctypes argument lists of the three
cat_tstage1n7_* entries against the header, and the register pin of csrc/conv_s1n7.hip (tests/golden/codegen_conv_s1n7.json, written by
tools/codegen_table.py; hipcc cross-compiles gfx950 here)."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_the_switch_and_its_environment_variable():
    from cat_amd import fused_block, fused_spade
    block_k7 = fused_block._K7
    old = fused_spade.set_k7(False)
    try:
        assert fused_spade.set_k7(True) is False and fused_spade.set_k7(True) is True and fused_spade._K7 is True
        assert fused_block._K7 is block_k7      # CAT_FUSED_K7 is another switch
    finally:
        fused_spade.set_k7(old)
    code = 'from cat_amd import fused_spade; print(int(fused_spade._K7))'
    got = {}
    for val in (None, '0', '1'):
        env = {k: v for k, v in os.environ.items() if k != 'CAT_FUSED_SPADE_K7'}
        if val is not None:
            env['CAT_FUSED_SPADE_K7'] = val
        got[val] = int(subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, check=True).stdout)
    assert got['0'] == 0 and got['1'] == 1
    assert got[None] == 1      # on by default: the README's CAT_FUSED_SPADE_K7 paragraph has the rule and the measurement behind it


def _unit(ks_res, ks_dw, m=5, cin=8, cout=8, conv2_k=None):
    """stub branch modules with the attributes fused_spade.applicable reads: [ConvSyncBNReLU, Conv] / [ConvSyncBNReLU, ConvSyncBNReLU, Conv]"""
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import Conv, ConvSyncBNReLU
    import functools
    norm = functools.partial(cnn.SynchronizedBatchNorm2d, affine=True)
    act = functools.partial(cnn.ReLU, inplace=True)
    res = [torch.nn.Sequential(ConvSyncBNReLU(cin, m, kernel_size=k, norm_layer=norm, active_fn=act),
                               Conv(m, cout, kernel_size=k if conv2_k is None else conv2_k)) for k in ks_res]
    dws = [torch.nn.Sequential(ConvSyncBNReLU(cin, m, kernel_size=1, norm_layer=norm, active_fn=act),
                               ConvSyncBNReLU(m, m, kernel_size=k, groups=m, norm_layer=norm, active_fn=act), Conv(m, cout, kernel_size=1)) for k in ks_dw]
    return torch.nn.ModuleList(res).train(), torch.nn.ModuleList(dws).train()


def test_applicable_admits_7x7_branches_only_under_the_switch(monkeypatch):
    from cat_amd import fused_spade, ops
    monkeypatch.setattr(ops, 'is_act', lambda x: True)
    monkeypatch.setattr(ops, 'tconv_applicable', lambda *a, **kw: True)
    monkeypatch.setattr(ops, 'bn_sync', lambda: None)
    x = types.SimpleNamespace(is_cuda=True, shape=(2, 8, 24, 40))
    u135, u357, u7dw, u9 = _unit((1, 3, 5), (1, 3, 5)), _unit((3, 5, 7), (3, 5, 7)), _unit((3,), (7,)), _unit((3, 5, 9), (3,))
    mixed = _unit((7,), (), conv2_k=5)      # conv2's kernel must equal the first conv's for a residual branch, at 7 as at 3 and 5
    old = fused_spade.set_k7(True)
    try:
        for training in (True, False):
            with torch.set_grad_enabled(training):
                for u in (u135, u357, u7dw, u9, mixed):
                    for blk in u:
                        blk.train(training)
                fused_spade.set_k7(True)
                assert fused_spade.applicable(*u135, x, training) and fused_spade.applicable(*u357, x, training) and fused_spade.applicable(*u7dw, x, training)
                assert not fused_spade.applicable(*u9, x, training) and not fused_spade.applicable(*mixed, x, training)
                fused_spade.set_k7(False)      # off: the function it was
                assert fused_spade.applicable(*u135, x, training)
                assert not any(fused_spade.applicable(*u, x, training) for u in (u357, u7dw, u9, mixed))
        # every other condition stays under the switch: a padding that is not (k - 1) // 2, the DWM_MAXQ limit
        fused_spade.set_k7(True)
        for blk in u357[0]:
            blk.train(True)
        for blk in u357[1]:
            blk.train(True)
        with torch.enable_grad():
            assert fused_spade.applicable(*u357, x, True)
            u357[0][2][0].conv.padding = (2, 2)
            assert not fused_spade.applicable(*u357, x, True)
            u357[0][2][0].conv.padding = (3, 3)
            wide = _unit((3, 5, 7), (3, 5, 7), m=28)      # 3 x 28 depthwise channels = 21 quads > CAT_DWM_MAXQ_BWD
            assert not fused_spade.applicable(*wide, x, True)
    finally:
        fused_spade.set_k7(old)


def _supported(name, *w):
    """mirrors of the support predicates stage1 asks"""
    if name == 'cat_tstage1_supported':
        a, b, c = (-(-v // 16) for v in w)
        return int(min(w) > 0 and a <= 2 and b <= 2 and 2 <= c <= 4)
    if name == 'cat_tstage1ws_supported':
        return int(32 < w[0] <= 48 and 32 < w[1] <= 48 and 160 < w[2] <= 176)
    if name == 'cat_tstage1ws7_supported':
        return int(all(32 < v <= 48 for v in w[:3]) and 128 < w[3] <= 144)
    if name == 'cat_tstage1n7_supported':
        return int(min(w) > 0 and max(w[:3]) <= 32 and w[3] <= 64)
    raise AssertionError(name)


def _stage1_entries(monkeypatch, widths, n7=True, part1=True, reflect=False, hw=(16, 32)):
    """the entry points fused_unit.stage1 issues for a plan whose first-conv groups are {kernel size: slot width}, in order, and the geometry
    of a one-launch call"""
    from cat_amd import _lib, fused_unit, ops, tconv
    names, geoms = [], []

    def call(name, *a):
        names.append(name)
        geoms.append(a[0]._obj)
    monkeypatch.setattr(_lib, 'query', _supported)
    monkeypatch.setattr(_lib, 'call', call)
    monkeypatch.setattr(tconv, 'run', lambda segs, *a, **kw: names.append('cat_tconv_fwd:%d' % segs[0].k))
    monkeypatch.setattr(tconv, 'Segment', lambda x, k, *a, **kw: types.SimpleNamespace(k=k))
    monkeypatch.setattr(ops, 'act_cs', lambda x: x.shape[1])
    monkeypatch.setattr(ops, '_p', lambda t: None)
    monkeypatch.setattr(ops, '_stream', lambda: None)
    off, groups = 0, []
    for k in (1, 3, 5, 7):
        if k in widths:
            groups.append(dict(k=k, off=off, width=widths[k], branches=[dict(m=widths[k] - 2)], pack=torch.zeros(4)))
            off += widths[k]
    p = types.SimpleNamespace(groups=groups, hc1=off, has_bias1=False, bias1=torch.zeros(4))
    if n7 is not None:
        p.stage1_n7 = n7
    x, z1 = torch.zeros(2, 16, *hw), torch.zeros(4)
    fused_unit.stage1(p, x, z1, torch.zeros(4) if part1 else None, reflect)
    return names, geoms


NARROW7 = {1: 24, 3: 8, 5: 4, 7: 8}
PER_SIZE = lambda ws: ['cat_tconv_fwd:%d' % k for k in sorted(ws)]


def test_stage1_chooses_the_narrow_one_launch_only_for_plans_that_carry_the_attribute(monkeypatch):
    names, geoms = _stage1_entries(monkeypatch, NARROW7)
    assert names == ['cat_tstage1n7_fwd']
    g = geoms[0]      # slot order 7, 5, 3, 1; columns in the plan's order [1 | 3 | 5 | 7]
    assert list(g.width) == [8, 4, 8, 24] and list(g.col0) == [36, 32, 24, 0] and list(g.nvalid) == [6, 2, 6, 22]
    assert (g.N, g.H, g.W, g.cin, g.xcs, g.reflect, g.ycs, g.scs) == (2, 16, 32, 16, 16, 0, 44, 44)
    assert _stage1_entries(monkeypatch, NARROW7, reflect=True, hw=(7, 7))[0] == ['cat_tstage1n7_fwd']
    assert _stage1_entries(monkeypatch, {1: 64, 3: 32, 5: 32, 7: 32})[0] == ['cat_tstage1n7_fwd']
    # every exception: one launch per size
    assert _stage1_entries(monkeypatch, NARROW7, n7=False)[0] == PER_SIZE(NARROW7)
    assert _stage1_entries(monkeypatch, NARROW7, n7=None)[0] == PER_SIZE(NARROW7)      # the plans of fused_block.py / frozen_in.py: no attribute
    assert _stage1_entries(monkeypatch, NARROW7, part1=False)[0] == PER_SIZE(NARROW7)      # the eval form: no statistics
    for ws in ({1: 24, 3: 8, 7: 8}, {3: 8, 5: 4, 7: 8}, {1: 24, 5: 4, 7: 8}, {1: 68, 3: 8, 5: 4, 7: 8}, {1: 24, 3: 8, 5: 4, 7: 36}, {1: 24, 3: 36, 5: 4, 7: 8}):
        assert _stage1_entries(monkeypatch, ws)[0] == PER_SIZE(ws), ws
    for hw in ((6, 32), (16, 6)):      # a mirrored window wider than the plane
        assert _stage1_entries(monkeypatch, NARROW7, reflect=True, hw=hw)[0] == PER_SIZE(NARROW7)
    assert _stage1_entries(monkeypatch, NARROW7, reflect=False, hw=(5, 7))[0] == ['cat_tstage1n7_fwd']      # zero padding has no such limit
    # a 1 3 5 plan issues what it always has, with or without the attribute; the wide 3 5 7 widths keep their kernel
    for n7 in (True, None):
        assert _stage1_entries(monkeypatch, {1: 44, 3: 12, 5: 20}, n7=n7)[0] == ['cat_tstage1_fwd']
        assert _stage1_entries(monkeypatch, {1: 132, 3: 44, 5: 44, 7: 44}, n7=n7)[0] == ['cat_tstage1ws7_fwd']


def _header_args(name):
    src = open(os.path.join(ROOT, 'include', 'cat_hip.h')).read()
    m = re.search(r'\bint %s\(([^;]*?)\);' % name, src, re.S)
    assert m, name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def test_ctypes_signatures_match_the_header():
    from cat_amd import _lib
    c_i, c_p = C.c_int, C.c_void_p
    kinds = {'int': c_i, 'const cat_tstage1s7_t*': C.POINTER(_lib.Stage1S7Geom), 'const float*': c_p, 'const float* const*': c_p, 'float*': c_p,
             'float* const*': c_p, 'const int*': c_p, 'cat_stream_t': c_p}
    for name, nargs in (('cat_tstage1n7_supported', 4), ('cat_tstage1n7_fwd', 7), ('cat_tstage1n7_dgrad', 6)):
        args = _header_args(name)
        types_ = [kinds[a.rsplit(' ', 1)[0]] for a in args]
        res, sig = _lib.SIGNATURES[name]
        assert res is c_i and len(args) == nargs and sig == types_, (name, args, sig)
    # the same argument lists as the entries they extend
    assert _lib.SIGNATURES['cat_tstage1n7_fwd'] == _lib.SIGNATURES['cat_tstage1ws7_fwd']
    assert [a.rsplit(' ', 1)[0] for a in _header_args('cat_tstage1n7_dgrad')][1:] == [a.rsplit(' ', 1)[0] for a in _header_args('cat_tstage1_dgrad')][1:]
    assert 'conv_s1n7.hip' in open(os.path.join(ROOT, 'cat_amd', '_build.py')).read()


def test_conv_s1n7_kernels_keep_their_register_budget():
    import codegen_table
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'codegen_conv_s1n7.json')))
    got = codegen_table.table('cat_amd/csrc/conv_s1n7.hip')
    assert sorted(got) == sorted(want), 'kernel set of conv_s1n7.hip changed: re-record with tools/codegen_table.py --write (after an A/B on hardware)'
    # every N-tile combination of the predicate's domain, with and without statistics
    inst = set()
    for k in got:
        m = re.search(r'tstage1n7_kernelILi(\d)ELi(\d)ELi(\d)ELi(\d)ELb([01])E', k)
        assert m, k
        inst.add(tuple(int(v) for v in m.groups()))
    assert inst == set(itertools.product((1, 2), (1, 2), (1, 2), (1, 2, 3, 4), (0, 1))) and len(got) == 64
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, 'register / scratch counts changed (committed, now): %s' % diff
    for k, v in got.items():      # no scratch, no spills, two workgroups per CU (59 520 B of LDS each: 256 registers are free at that occupancy)
        assert v['scratch'] == 0 and v['vspill'] == 0 and v['vgpr'] <= 256, (k, v)
