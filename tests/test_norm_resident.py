"""CPU: the host side of the one-launch norm kernels (csrc/norm_resident.hip).  cat_norm_launches, cat_norm_resident_max_pixels and
cat_norm_set_resident are pure host functions of the built library; the limits keep the bounds the domain was chosen by; cat_norm_ws_bytes is
what it was (callers size one workspace for either path); and the code generation of every instantiation is pinned the way
tests/test_codegen.py pins the LDS-tile kernels (tests/golden/codegen_norm_resident.json, written by
`tools/codegen_table.py cat_amd/csrc/norm_resident.hip --lds --write ...`): the kernels hold a group's pixels in registers, so a spill or a
VGPR count that costs a wave of occupancy has to be a decision, not a side effect."""
import ctypes as C
import json
import os
import sys

from test_streaming_kernels_gpu import EPS, MOM, SLOPE, NORM_CASES, cs4, norm_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _lib():
    from cat_amd import _lib as L
    L.load()
    return L


def _geom(L, mode, c, n, hw, shards=0):
    return L.NormGeom(n, hw, c, cs4(c), L.NORM_INSTANCE if mode == 'instance' else L.NORM_BATCH, EPS, MOM, 0, SLOPE, shards)


def test_limits_and_launch_counts_are_pure_host_functions():
    """no device is touched: 2176 <= forward <= 8192 (33 x 65 planes inside, the default workload's BatchNorm layers of 15 376 pixels outside),
    backward no larger than forward; the launch counts at the limits, per mode, per switch"""
    L = _lib()
    fwd, bwd = L.query('cat_norm_resident_max_pixels', 0), L.query('cat_norm_resident_max_pixels', 1)
    assert 2176 <= fwd <= 8192 and 2176 <= bwd <= fwd, (fwd, bwd)
    launches = lambda g, backward, params: L.query('cat_norm_launches', C.byref(g), backward, params)
    prev = L.query('cat_norm_set_resident', 1)
    try:
        for mode, n in (('instance', 1), ('instance', 3), ('batch', 1)):
            for c in (3, 18, 64):
                assert launches(_geom(L, mode, c, n, fwd), 0, 0) == 1 and launches(_geom(L, mode, c, n, fwd + 1), 0, 0) == 3
                groups = n if mode == 'instance' else 1
                for params in (0, 1):
                    extra = 1 if params and groups > 1 else 0
                    assert launches(_geom(L, mode, c, n, bwd), 1, params) == 1 + extra
                    assert launches(_geom(L, mode, c, n, bwd + 1), 1, params) == 3 + extra
        assert launches(_geom(L, 'batch', 16, 4, 33 * 65), 0, 0) == 3              # the batch is the group: 4 x 2145 pixels
        assert launches(_geom(L, 'instance', 256, 8, 4096), 0, 0) == 3 and launches(_geom(L, 'instance', 256, 8, 4096), 1, 0) == 1   # 32 MiB in one-quad slabs: forward stays
        assert launches(_geom(L, 'instance', 128, 4, 4096), 0, 0) == 1 and launches(_geom(L, 'instance', 4, 64, 4096), 0, 0) == 1
        assert launches(_geom(L, 'batch', 16, 4, 33 * 65, shards=4), 0, 0) == 1    # one sample per shard
        assert launches(_geom(L, 'batch', 16, 3, 33 * 65, shards=2), 1, 1) == 4    # groups of 2 and 1 samples: 4290 pixels, beyond the backward limit
        assert launches(_geom(L, 'batch', 16, 3, 17 * 33, shards=2), 1, 1) == 2
        assert launches(_geom(L, 'batch', 64, 4, 62 * 62), 0, 0) == 3              # 15 376 pixels: the default workload stays where it was
        assert L.query('cat_norm_set_resident', 0) == 1
        assert launches(_geom(L, 'instance', 16, 2, 64), 0, 0) == 3 and launches(_geom(L, 'instance', 16, 2, 64), 1, 1) == 4
        assert L.query('cat_norm_set_resident', 1) == 0
    finally:
        L.query('cat_norm_set_resident', prev)


def test_workspace_bytes_are_unchanged():
    """cat_norm_ws_bytes against plan() of csrc/norm.hip as tests/test_streaming_kernels_gpu.py mirrors it, with the switch on and off"""
    L = _lib()
    geoms = [case[:5] for case in NORM_CASES] + [('instance', 18, 1, 64, 128), ('instance', 18, 1, 64, 64), ('instance', 16, 2, 33, 65),
                                                   ('batch', 24, 3, 7, 9), ('instance', 3, 2, 1, 1), ('instance', 128, 2, 64, 128),
                                                   ('batch', 64, 4, 62, 62), ('instance', 1024, 1, 4, 8)]
    prev = L.query('cat_norm_set_resident', 1)
    try:
        for on in (1, 0):
            L.query('cat_norm_set_resident', on)
            for mode, c, n, h, w in geoms:
                p = norm_plan(mode, c, n, h, w)
                nbytes = L.query('cat_norm_ws_bytes', C.byref(_geom(L, mode, c, n, h * w)))
                assert nbytes == 4 * p['floats'], (mode, c, n, h, w, on, nbytes, p)
                assert (nbytes // 4 // (p['G'] * p['cs']) - 4) // 2 == p['nb']
    finally:
        L.query('cat_norm_set_resident', prev)


def test_resident_kernels_keep_their_register_budget():
    import codegen_table
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'codegen_norm_resident.json')))
    got = codegen_table.table('cat_amd/csrc/norm_resident.hip', lds=True)
    assert sorted(got) == sorted(want), 'kernel set of norm_resident.hip changed: re-record with tools/codegen_table.py --lds --write'
    diff = {k: (want[k], got[k]) for k in want if want[k] != got[k]}
    assert not diff, 'register / scratch / LDS counts changed (committed, now): %s' % diff
    fwd = [k for k in got if 'norm_fwd_resident_kernel' in k]
    bwd = [k for k in got if 'norm_bwd_resident_kernel' in k]
    assert len(fwd) == 3 and len(bwd) == 3, sorted(got)      # K = 4, 8, 16 pixels per lane
    for k, v in got.items():      # resident means registers: nothing in scratch, two 4 x 4 float4 tables in LDS, at least two waves per SIMD
        assert v['scratch'] == 0 and v['vspill'] == 0 and v['lds'] == 512 and v['vgpr'] <= 256, (k, v)
