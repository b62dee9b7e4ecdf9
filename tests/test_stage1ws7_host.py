"""CPU: the host side of the one-launch stage 1 with statistics at kernel sizes 3 5 7 (cat_tstage1ws7_fwd) -- the ctypes mirror of
cat_tstage1s7_t against the header, the switch CAT_STAGE1WS7 and what fused_unit.stage1 chooses under it (on plans stubbed down to their
groups, with the launches recorded instead of issued), and the register pin of csrc/conv_s1ws7.hip (tests/golden/codegen_conv_s1ws7.json,
written by tools/codegen_table.py; hipcc cross-compiles gfx950 here)."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def test_stage1s7_geom_matches_the_header(tmp_path):
    from cat_amd import _lib
    cls = _lib.Stage1S7Geom
    assert [f for f, _ in cls._fields_] == [f for f, _ in _lib.Stage1Geom._fields_]      # the fields of cat_tstage1_t, four slots
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cat_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(cat_tstage1s7_t));']
    lines += ['  printf("%s %%zu\\n", offsetof(cat_tstage1s7_t, %s));' % (f, f) for f, _ in cls._fields_] + ['  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'probe')], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / 'probe')], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert C.sizeof(cls) == 4 * (8 + 3 * 4)


def test_the_switch():
    from cat_amd import fused_unit
    other = fused_unit._STAGE1WS
    old = fused_unit.set_stage1ws7(False)
    try:
        assert fused_unit.set_stage1ws7(True) is False and fused_unit.set_stage1ws7(True) is True
        assert fused_unit._STAGE1WS is other      # CAT_STAGE1WS is another switch
    finally:
        fused_unit.set_stage1ws7(old)
    src = open(os.path.join(ROOT, 'cat_amd', 'fused_unit.py')).read()
    assert "os.environ.get('CAT_STAGE1WS7'" in src


def _supported(name, *w):
    """mirrors of the support predicates stage1 asks"""
    if name == 'cat_tstage1_supported':
        a, b, c = (-(-v // 16) for v in w)
        return int(min(w) > 0 and a <= 2 and b <= 2 and 2 <= c <= 4)
    if name == 'cat_tstage1ws_supported':
        return int(32 < w[0] <= 48 and 32 < w[1] <= 48 and 160 < w[2] <= 176)
    if name == 'cat_tstage1ws7_supported':
        return int(all(32 < v <= 48 for v in w[:3]) and 128 < w[3] <= 144)
    raise AssertionError(name)


def _stage1_entries(monkeypatch, widths, part1=True, reflect=False, hw=(16, 32)):
    """the entry points fused_unit.stage1 issues for a plan whose first-conv groups are {kernel size: slot width}, in order"""
    from cat_amd import _lib, fused_unit, ops, tconv
    names = []
    monkeypatch.setattr(_lib, 'query', _supported)
    monkeypatch.setattr(_lib, 'call', lambda name, *a: names.append(name))
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
    x, z1 = torch.zeros(2, 16, *hw), torch.zeros(4)
    fused_unit.stage1(p, x, z1, torch.zeros(4) if part1 else None, reflect)
    return names


WIDE7 = {1: 132, 3: 44, 5: 44, 7: 44}
PER_SIZE = lambda ws: ['cat_tconv_fwd:%d' % k for k in sorted(ws)]


def test_stage1_chooses_the_one_launch_only_for_wide_357_plans_with_statistics(monkeypatch):
    from cat_amd import fused_unit
    old = fused_unit.set_stage1ws7(True), fused_unit.set_stage1_wide(True)
    try:
        assert _stage1_entries(monkeypatch, WIDE7) == ['cat_tstage1ws7_fwd']
        assert _stage1_entries(monkeypatch, WIDE7, reflect=True, hw=(7, 7)) == ['cat_tstage1ws7_fwd']
        fused_unit.set_stage1_wide(False)      # independent of CAT_STAGE1WS
        assert _stage1_entries(monkeypatch, WIDE7) == ['cat_tstage1ws7_fwd']
        assert _stage1_entries(monkeypatch, {1: 176, 3: 44, 5: 44}) == PER_SIZE((1, 3, 5))
        fused_unit.set_stage1_wide(True)
        # what stays as it is: the eval form, 1 3 5 plans, narrow widths, missing sizes, a mirrored window wider than the plane
        assert _stage1_entries(monkeypatch, WIDE7, part1=False) == PER_SIZE(WIDE7)
        assert _stage1_entries(monkeypatch, {1: 176, 3: 44, 5: 44}) == ['cat_tstage1ws_fwd']
        assert _stage1_entries(monkeypatch, {1: 44, 3: 12, 5: 20}) == ['cat_tstage1_fwd']
        for ws in ({1: 44, 3: 12, 5: 20, 7: 12}, {1: 132, 3: 44, 7: 44}, {3: 44, 5: 44, 7: 44}, {1: 132, 3: 44, 5: 44, 7: 52}, {1: 176, 3: 44, 5: 44, 7: 44}):
            assert _stage1_entries(monkeypatch, ws) == PER_SIZE(ws), ws
        assert _stage1_entries(monkeypatch, WIDE7, reflect=True, hw=(6, 32)) == PER_SIZE(WIDE7)
        fused_unit.set_stage1ws7(False)        # off: the parent's launches in the parent's order
        assert _stage1_entries(monkeypatch, WIDE7) == PER_SIZE(WIDE7)
        assert _stage1_entries(monkeypatch, {1: 176, 3: 44, 5: 44}) == ['cat_tstage1ws_fwd']
    finally:
        fused_unit.set_stage1ws7(old[0])
        fused_unit.set_stage1_wide(old[1])


def test_conv_s1ws7_kernel_keeps_its_register_budget():
    import codegen_table
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'codegen_conv_s1ws7.json')))
    got = codegen_table.table('cat_amd/csrc/conv_s1ws7.hip')
    assert sorted(got) == sorted(want), 'kernel set of conv_s1ws7.hip changed: re-record with tools/codegen_table.py --write (after an A/B on hardware)'
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, 'register / scratch counts changed (committed, now): %s' % diff
    assert len(got) == 1 and 'tstage1ws7_kernelILi3ELi3E' in ''.join(got)
    for k, v in got.items():      # no scratch, no spills, two workgroups per CU
        assert v['scratch'] == 0 and v['vspill'] == 0 and v['vgpr'] <= 256, (k, v)
