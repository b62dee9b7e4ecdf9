"""CPU: the host side of the frozen teachers at kernel sizes 3 5 7 -- the plan frozen._build_plan makes of CPU-built BatchNorm blocks (the
depthwise frame's side and index map, the one-launch stage-1 entry it chooses), the switch, the ctypes mirror of cat_tstage1w7_t, and the
register pin of csrc/conv_s1w7.hip (tests/golden/codegen_conv_s1w7.json, written by tools/codegen_table.py; hipcc cross-compiles gfx950 here).
The plans are built on the CPU device: folding is torch arithmetic, the packed filter streams are built at the first launch."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _supported(name, *w):
    """mirrors of the support predicates the plan asks"""
    if name == 'cat_tstage1w_supported':
        return int(32 < w[0] <= 48 and 32 < w[1] <= 48 and 160 < w[2] <= 176)
    if name == 'cat_tstage1w7_supported':
        return int(all(32 < v <= 48 for v in w[:3]) and 128 < w[3] <= 144)
    raise AssertionError(name)


def _plan(monkeypatch, ks, res=(42, 42, 42), dw=(42, 42, 42), cin=16):
    from oracle import detfill
    from cat_amd import _lib, frozen, nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    monkeypatch.setattr(_lib, 'query', _supported)
    blk = InvertedResidualChannels(cin, list(res), list(dw), 1, list(ks), list(ks), padding_type='reflect', use_bias=False, norm_layer=cnn.BatchNorm2d,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    blk.load_state_dict(detfill.fill_state_dict(blk.state_dict(), 77, gamma_abs_normal=True))
    blk.eval()
    with torch.no_grad():
        return blk, frozen._build_plan(blk)


def test_frame_row_is_the_centred_map():
    from cat_amd import frozen
    for fs in (5, 7):
        for k in (1, 3, 5, 7):
            if k > fs:
                continue
            rows = [frozen.frame_row(fs, k, ky, kx) for ky in range(k) for kx in range(k)]
            assert rows == [(ky + fs // 2 - k // 2) * fs + kx + fs // 2 - k // 2 for ky in range(k) for kx in range(k)]
            assert len(set(rows)) == k * k and min(rows) >= 0 and max(rows) < fs * fs and rows[k * k // 2] == fs * fs // 2


def test_plan_of_a_357_block(monkeypatch):
    from cat_amd import frozen
    blk, p = _plan(monkeypatch, [3, 5, 7])
    dwm = p['dwm']
    assert p['hc'] == 132 and dwm['fs'] == 7 and tuple(dwm['frame'].shape) == (49, 132) and dwm['ks'] == [3] * 11 + [5] * 11 + [7] * 11
    assert p['s1w'] is None and p['s1w7'] is not None and p['s1w7']['m'] == [42, 42, 42, 132] and p['s1w7']['packs'] is None
    assert [tuple(w.shape[2:]) for w in p['s1w7']['ws']] == [(7, 7), (5, 5), (3, 3), (1, 1)]
    # the frame against the folded filters: tap (ky, kx) of each k at its row, zeros everywhere else, zero filters and bias in the slots' padding
    want = torch.zeros(49, 132)
    for d in p['dws']:
        k = d['k']
        assert d['off'] == 44 * ((k - 3) // 2) and d['m'] == 42
        for ky in range(k):
            for kx in range(k):
                want[(ky + 3 - k // 2) * 7 + kx + 3 - k // 2, d['off']:d['off'] + 42] = d['w'][:, 0, ky, kx]
    assert torch.equal(dwm['frame'], want)
    assert float(dwm['frame'][:, 42:44].abs().sum()) == 0.0 and float(dwm['bias'][42:44].abs().sum()) == 0.0
    s2 = torch.rsqrt(blk.dw_ops[2][2][1].running_var + 1e-5) * blk.dw_ops[2][2][1].weight
    assert torch.allclose(dwm['frame'][0, 88:130], (blk.dw_ops[2][2][0].weight[:, 0, 0, 0] * s2).detach())      # the 7 x 7 corner tap: row 0


def test_plan_of_a_135_block_is_what_it_was(monkeypatch):
    blk, p = _plan(monkeypatch, [1, 3, 5])
    dwm = p['dwm']
    assert p['hc'] == 176 and dwm['fs'] == 5 and tuple(dwm['frame'].shape) == (25, 176) and dwm['ks'] == [1] * 22 + [3] * 11 + [5] * 11
    assert p['s1w7'] is None and p['s1w'] is not None and p['s1w']['m'] == [42, 42, 176]
    assert torch.equal(dwm['frame'][12, :42], torch.ones(42)) and float(dwm['frame'][:12, :88].abs().sum()) == 0.0      # the copy: centre weight 1
    for d in p['dws']:
        k, o = d['k'], 2 - d['k'] // 2
        for ky in range(k):
            for kx in range(k):
                assert torch.equal(dwm['frame'][(o + ky) * 5 + o + kx, d['off']:d['off'] + 42], d['w'][:, 0, ky, kx])


def test_a_7x7_residual_branch_alone_does_not_widen_the_frame(monkeypatch):
    blk, p = _plan(monkeypatch, [3, 5, 7], dw=(42, 42, 0))
    assert p['dwm']['fs'] == 5 and p['s1w7'] is None and p['s1w'] is None      # hc = 88: outside the one-launch kernel's widths
    blk, p = _plan(monkeypatch, [3, 5, 7], res=(42, 42, 0))
    assert p['dwm']['fs'] == 7 and p['s1w7'] is None and p['s1w'] is None      # wide branches {3, 5}, but a 132-wide 1 x 1 group


def test_the_switch():
    from cat_amd import frozen
    old = frozen.set_k7(False)
    try:
        assert frozen.set_k7(True) is False and frozen.set_k7(True) is True
    finally:
        frozen.set_k7(old)
    src = open(os.path.join(ROOT, 'cat_amd', 'frozen.py')).read()
    assert "os.environ.get('CAT_FROZEN_K7'" in src


def test_stage1w7_geom_matches_the_header(tmp_path):
    from cat_amd import _lib
    cls = _lib.Stage1W7Geom
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cat_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(cat_tstage1w7_t));']
    lines += ['  printf("%s %%zu\\n", offsetof(cat_tstage1w7_t, %s));' % (f, f) for f, _ in cls._fields_] + ['  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(tmp_path / 'probe')], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / 'probe')], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_conv_s1w7_kernel_keeps_its_register_budget():
    import codegen_table
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'codegen_conv_s1w7.json')))
    got = codegen_table.table('cat_amd/csrc/conv_s1w7.hip')
    assert sorted(got) == sorted(want), 'kernel set of conv_s1w7.hip changed: re-record with tools/codegen_table.py --write (after an A/B on hardware)'
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, 'register / scratch counts changed (committed, now): %s' % diff
    assert len(got) == 1 and 'tstage1w7_kernelILi3ELi3E' in ''.join(got)
    for k, v in got.items():      # no scratch, no spills, two workgroups per CU
        assert v['scratch'] == 0 and v['vspill'] == 0 and v['vgpr'] <= 256, (k, v)
