"""The argument contract of the eight one-launch stage-1 entries (docs/CONV_VARIANTS.md, "Stage 1 in one launch"; the shared host checks:
csrc/conv_s1_host.h): each entry, called through the C ABI with malformed arguments, returns an error that carries its own name and
message prefix, and writes nothing.

Per entry the valid arguments are the smallest it takes: batch 1, a plane of 8 x 16 (one tile), cin = 16 (one chunk), zero padding, and
the narrowest channel counts of its width domain, each slice laid out in whole channel quads as every caller does.  One fault at a time:

    * a slot width one column below / above the domain of the entry's `*_supported` query, for every slot (cat_tstage1_fwd takes a 1 x 1
      slot of one N tile -- the instantiation the input-gradient form needs -- although cat_tstage1_supported does not offer it: no case);
    * reflect = 1 on a plane one pixel lower / narrower than the largest kernel (the input-gradient forms refuse reflect altogether);
    * a pixel stride of x that is no multiple of 4;  cin > xcs;  a null filter stream for a used slot, for every slot.

Every refusal comes from the host checks, before a launch.  The valid call runs last and is seen to launch once."""
import ctypes as C
import re

import pytest
import torch

from test_fused_kernels_gpu import SENTINEL, _profiled

H, W, CIN = 8, 16, 16
ARENA = 1 << 18      # floats; a slot's output (or the statistics table) owns a quarter

# entry -> (message prefix, geometry struct, contract, kernel size per slot, (lowest, highest) width per slot, family the profiler books)
N5, N7 = ((1, 32), (1, 32), (1, 64)), ((1, 32), (1, 32), (1, 32), (1, 64))
W5, W7 = ((33, 48), (33, 48), (161, 176)), ((33, 48), (33, 48), (33, 48), (129, 144))
ENTRIES = {
    'cat_tstage1_fwd': ('tstage1', 'Stage1Geom', 'slices', (5, 3, 1), ((1, 32), (1, 32), (17, 64)), 'conv_tstage1'),
    'cat_tstage1_dgrad': ('tstage1( dgrad)?', 'Stage1Geom', 'dgrad', (5, 3, 1), N5, 'conv_tstage1_dgrad'),
    'cat_tstage1w_fwd': ('tstage1w', 'Stage1WGeom', 'buffers', (5, 3, 1), W5, 'conv_tstage1w'),
    'cat_tstage1ws_fwd': ('tstage1ws', 'Stage1Geom', 'slices', (5, 3, 1), W5, 'conv_tstage1ws'),
    'cat_tstage1w7_fwd': ('tstage1w7', 'Stage1W7Geom', 'buffers', (7, 5, 3, 1), W7, 'conv_tstage1w7'),
    'cat_tstage1ws7_fwd': ('tstage1ws7', 'Stage1S7Geom', 'slices', (7, 5, 3, 1), W7, 'conv_tstage1ws7'),
    'cat_tstage1n7_fwd': ('tstage1n7', 'Stage1S7Geom', 'slices', (7, 5, 3, 1), N7, 'conv_tstage1n7'),
    'cat_tstage1n7_dgrad': ('tstage1n7 dgrad', 'Stage1S7Geom', 'dgrad', (7, 5, 3, 1), N7, 'conv_tstage1n7_dgrad'),
}
TAKEN_BELOW = {('cat_tstage1_fwd', 2)}      # (entry, slot) whose width one below the query's domain still has a kernel


def cs4(c):
    return (c + 3) // 4 * 4


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _args(dev, entry):
    """-> (call, geometry, filter-stream pointers, set_width(slot, channels, whole quads), output arena): valid arguments, to be spoilt in place"""
    from cat_amd import _lib as L, ops
    prefix, geom, contract, sizes, domain, family = ENTRIES[entry]
    ns = len(sizes)
    src = torch.zeros(ARENA, device=dev)      # x and every filter stream: zeros, larger than anything a launch of these shapes reads
    out = torch.full((ARENA,), SENTINEL, device=dev)
    at = lambda t, q: t.data_ptr() + 4 * q * (ARENA // 4)
    g = getattr(L, geom)()
    g.N, g.H, g.W, g.xcs, g.cin, g.reflect = 1, H, W, CIN, CIN, 0
    packs = (C.c_void_p * ns)(*[src.data_ptr()] * ns)
    if contract == 'buffers':
        g.act, g.slope = 1, 0.0
        ys = (C.c_void_p * ns)(*[at(out, k) for k in range(ns)])
        tail = (None, ys)      # no biases

        def set_width(k, m, quads=True):
            g.nvalid[k], g.ycs[k] = m, cs4(m)
    else:
        def set_width(k, m, quads=True):      # slices back to back from column 0
            g.width[k], g.nvalid[k] = cs4(m) if quads else m, m
            for j in range(1, ns):
                g.col0[j] = g.col0[j - 1] + g.width[j - 1]
            g.ycs = g.scs = max(4, cs4(g.col0[ns - 1] + g.width[ns - 1]))
            if contract == 'dgrad':
                for j in range(ns):
                    dxcs[j] = g.ycs
        if contract == 'dgrad':
            dxs, dxcs = (C.c_void_p * ns)(*[at(out, k) for k in range(ns)]), (C.c_int * ns)()
            tail = (dxs, dxcs)
        else:
            tail = (None, C.c_void_p(at(out, 0)), C.c_void_p(at(out, 2)))      # no bias; y; the statistics table
    for k, (lo, hi) in enumerate(domain):
        set_width(k, lo)
    call = lambda: L.call(entry, C.byref(g), ops._p(src), packs, *tail, ops._stream())
    return call, g, packs, set_width, out


@pytest.mark.gpu
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_stage1_entry_refuses_malformed_arguments_under_its_own_name(dev, entry):
    prefix, geom, contract, sizes, domain, family = ENTRIES[entry]
    call, g, packs, set_width, out = _args(dev, entry)
    match = re.escape(entry) + r' failed \(-22\): ' + prefix + ': '

    def refused(what):
        with pytest.raises(RuntimeError, match=match):
            call()
            pytest.fail('%s: %s was accepted' % (entry, what))

    for k, (lo, hi) in enumerate(domain):
        for m in (lo - 1, hi + 1):
            if m < lo and (entry, k) in TAKEN_BELOW:
                continue
            set_width(k, m, quads=False)
            refused('width %d in slot %d' % (m, k))
        set_width(k, lo)
    kmax = sizes[0]
    for hh, ww in ((kmax - 1, W), (H, kmax - 1)):
        g.reflect, g.H, g.W = 1, hh, ww
        refused('reflect on %d x %d' % (hh, ww))
    g.reflect, g.H, g.W = 0, H, W
    g.xcs = CIN + 2
    refused('xcs %d' % g.xcs)
    g.xcs, g.cin = CIN, CIN + 4
    refused('cin %d > xcs %d' % (g.cin, g.xcs))
    g.cin = CIN
    for k in range(len(sizes)):
        good, packs[k] = packs[k], None
        refused('a null filter stream in slot %d' % k)
        packs[k] = good
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    _, fam = _profiled(call)      # ... and the arguments they were spoilt from are valid
    assert fam.get(family, 0) == 1, fam
