"""CPU: the dropout generator's numpy restatement (Philox4x32-10 and the mask formula of include/cat_hip.h, cat_dropout_apply) against the
Random123 known-answer vectors, the cat_drop_t ctypes mirror against the C layout, and the reference quirk that a pruned student
inherits the teacher's dropout_rate (shrink deep-copies the teacher)."""
import os

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint32 arrays (broadcast) -> 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
    return [v.astype(np.uint32) for v in c]


def keep_mask(npix, C, j, d, seed, p):
    """bool [npix, C]: element e = pixel * C + c is kept iff philox((lo32(e>>2), hi32(e>>2), j, d), (lo32(seed), hi32(seed)))[e & 3] >= floor(p 2^32)."""
    E = npix * C
    b = np.arange((E + 3) // 4, dtype=np.uint64)
    r = philox4x32_10(b & _M32, b >> np.uint64(32), np.uint64(j), np.uint64(d), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    bits = np.stack(r, axis=1).reshape(-1)[:E]
    if p >= 1.0:
        return np.zeros((npix, C), dtype=bool)
    return (bits >= np.uint32(min(int(p * 4294967296.0), 4294967295))).reshape(npix, C)


def scale_of(p):
    return np.float32(1.0 / (1.0 - p))


def _hex(v):
    return ' '.join('%08x' % int(x) for x in v)


def test_philox_known_answers():
    assert _hex(philox4x32_10(0, 0, 0, 0, 0, 0)) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    f = 0xFFFFFFFF
    assert _hex(philox4x32_10(f, f, f, f, f, f)) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    got = philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)
    assert _hex(got) == 'd16cfe09 94fdcceb 5001e420 24126ea1'


def test_mask_formula_counts_elements_in_quads():
    """e >> 2 selects the Philox block, e & 3 the word; a block never mixes two modules' (j) streams, and the 64-bit block index is split
    into counter words 0 / 1."""
    m = keep_mask(5, 3, 2, 7, (11 << 32) | 5, 0.5)
    r = philox4x32_10(np.arange(4), 0, 2, 7, 5, 11)
    bits = np.stack(r, axis=1).reshape(-1)[:15]
    np.testing.assert_array_equal(m.reshape(-1), bits >= np.uint32(1 << 31))
    hi = philox4x32_10(np.uint64(1), np.uint64(1), 0, 0, 0, 0)      # block 2^32 + 1
    assert _hex(hi) != _hex(philox4x32_10(1, 0, 0, 0, 0, 0))


def test_dropout_struct_matches_its_ctypes_mirror(tmp_path):
    import ctypes as C
    import subprocess
    from cat_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    structs = {'cat_dropseg_t': _lib.DropSeg, 'cat_drop_t': _lib.DropGeom}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cat_hip.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  printf("const maxseg %d\\n", CAT_DROP_MAXSEG);', '  printf("const plain %d\\n", CAT_DROP_PLAIN);', '  printf("const norm %d\\n", CAT_DROP_NORM);',
              '  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(root, 'include'), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {}
    for ln in out.splitlines():
        c, f, v = ln.split()
        got[(c, f)] = int(v)
    assert (got[('const', 'maxseg')], got[('const', 'plain')], got[('const', 'norm')]) == (_lib.DROP_MAXSEG, _lib.DROP_PLAIN, _lib.DROP_NORM)
    for cname, cls in structs.items():
        assert int(got[(cname, 'size')]) == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert int(got[(cname, fname)]) == getattr(cls, fname).offset, (cname, fname)


def test_threshold_and_scale():
    from cat_amd import rng
    assert rng.threshold(0.0) == 0 and rng.threshold(0.5) == 1 << 31 and rng.threshold(0.25) == 1 << 30
    assert rng.threshold(1.0 - 2.0 ** -40) == 0xFFFFFFFF
    from cat_amd import ops
    g = ops.dropout_geom(10, 4, 4, 4, 0.1, [(0, 3, 1)])
    assert np.float32(g.s) == scale_of(0.1) and g.thresh == int(0.1 * 2 ** 32) and not g.drop_all
    assert ops.dropout_geom(10, 4, 4, 4, 1.0, [(0, 3, 1)]).drop_all == 1


def test_shrunk_student_carries_the_teacher_dropout_rate():
    """reference utils/common.py:319-389: shrink deep-copies the teacher, so the pruned student's blocks are rebuilt with the TEACHER's
    dropout_rate (every distill recipe prunes with --target_flops: --teacher_dropout_rate is the flag that reaches the trained student)."""
    import copy
    import torch
    import helpers as H
    from cat_amd import networks, prune
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels
    opt = H.make_opt(norm='instance', track=False, target_flops=2.6e9, prune_cin_lb=16)
    torch.manual_seed(233)
    T = networks.define_G(3, 3, 64, 'inception_9blocks', 'instance', 0.3, 'normal', 0.02, [], opt=opt)
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for m in T.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.InstanceNorm2d)) and getattr(m, 'weight', None) is not None:
                m.weight.copy_(torch.randn(m.weight.shape, generator=gen).abs())
    T.eval()
    thr, _ = prune.search_threshold(T, 2.6e9, opt)
    S = copy.deepcopy(T)
    prune._apply_structure(S, T, thr, opt, copy_weights=True)
    blocks = [m for m in S.modules() if isinstance(m, InvertedResidualChannels)]
    assert len(blocks) == 9
    for b in blocks:
        assert b.dropout_rate == 0.3
        drops = [m for m in b.modules() if isinstance(m, cnn.Dropout)]
        assert len(drops) == len(b.res_ops) + len(b.dw_ops) and all(m.p == 0.3 for m in drops)
    assert sum(b.res_channels[0] for b in blocks) < sum(b.res_channels[0] for b in T.modules() if isinstance(b, InvertedResidualChannels))
