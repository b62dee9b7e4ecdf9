"""Frozen-teacher fast path for WIDE InstanceNorm blocks (reference inception_modules.py:124-180, 230-236; networks.py:41-44).

The CycleGAN-style distillation runs an InstanceNorm teacher in eval mode under no_grad (base_inception_distiller.py:168,
inception_distiller.py:100-104).  An InstanceNorm2d without running statistics computes the same function in eval() as in train(), so
nothing folds (cat_amd/frozen.py folds BatchNorm only) -- but the block is exactly the forward of the fused training pipeline
(cat_amd/fused_unit.py, per-sample statistics), which in eval mode serves only blocks an inference runner owns (fused_block.own_eval).
This module is the forward-only plan of a frozen teacher's blocks, eight launches instead of ~55 (kernel sizes from {1, 3, 5, 7}; a 7 x 7
branch under fused_block's switch CAT_FUSED_K7: stage 1 as one cat_tstage1ws7_fwd at the teacher's widths, else one cat_tconv_fwd per kernel
size, cat_dwm7_fwd, the cat_tconv_fwd tail); its depthwise launches take
CAT_DWM_MAXQ quads (a plan that trains groups by CAT_DWM_MAXQ_BWD, the width of the backward kernel's argument arrays; one workgroup of
either kernel stages one quad group, so LDS bounds neither):

    stage 1   first convs of all branches -> Z1 + tile statistics                 (fused_unit.stage1: cat_tstage1ws_fwd, at kernel sizes 3 5 7
                                                                                  cat_tstage1ws7_fwd; CAT_STAGE1WS=0 / CAT_STAGE1WS7=0: cat_tconv_fwd)
    finalize  per-sample scale / shift of every stage-1 norm                      (cat_tnorm_finalize, G = N)
    dw        the depthwise convs, normalise + activation applied while staging, in BRANCH-ALIGNED launches of at most CAT_DWM_MAXQ
              channel quads (the teacher's 3 x 11 quads: 22 + 11)                 (cat_dwm_fwd)
    finalize
    stage 2   the branch sum, K-concatenated, normalise + activation applied while staging, pw_bn's statistics in the epilogue
                                                                                  (cat_tconv_fwd with f_s and stats, as the fused block)
              -- or, CAT_FROZEN_IN_TAIL=ksum, on the wide DMA tile with the staging function applied to the A fragments: the residual
              slices of Z1 as one segment each, ALL depthwise slices of Zd as ONE segment whose 1 x 1 filters are concatenated along K once
              per plan (cat_conv2d_ksum_norm_fwd); outside that kernel's domain (zero padding, planes off its lattice, narrow outputs,
              small grids) it is cat_tconv_fwd again.  The LDS-tile kernel measured faster at the teacher's shapes and is the default
    finalize, out = x + T * scale + shift                                         (cat_tnorm_finalize2 / cat_tnorm_finalize, cat_affine_res_fwd)

Only blocks somebody OWNS take it: BaseInceptionDistiller registers the blocks of its eval-mode InstanceNorm teacher.  The registry holds
the block objects weakly and nothing is written on the modules, so a copy.deepcopy of an owned network is not owned; every other network
-- students, BatchNorm teachers, an inference runner's blocks, the SPADE family -- issues the launches it always issued.
CAT_FROZEN_IN=0 (set_enabled) restores the general path; CAT_FROZEN_IN_TAIL=ksum (set_tail) moves stage 2 to the wide tile."""
import ctypes as C
import os
import weakref

import torch

from . import _lib as L
from . import derived
from . import fused_block
from . import fused_unit as U
from . import ksum
from . import nn as cnn
from . import ops
from . import optim
from . import tconv

FROZEN_IN = derived.slot('_cat_frozen_in')      # the K-concatenated depthwise second-conv filters, keyed on every parameter and buffer of the block
_ENABLED = os.environ.get('CAT_FROZEN_IN', '1') != '0'
# stage 2: 'tconv' = always the LDS-tile kernel; 'ksum' = the normalising wide DMA tile where its domain holds.  Measured at the teacher's
# shapes (tools/frozen_in_bench.py, profiles/frozen_in_bench.txt): 263 us per tail on cat_tconv_fwd, 273 us on cat_conv2d_ksum_norm_fwd --
# the LDS-tile kernel is the default, the wide tile stays reachable
_TAIL = os.environ.get('CAT_FROZEN_IN_TAIL', 'tconv')
# block -> (the owner's LDS-tile threshold for it: fewest 8 x 16 output tiles; None: ops' process-wide one,)
_OWNED = weakref.WeakKeyDictionary()


def set_enabled(on):
    global _ENABLED
    old, _ENABLED = _ENABLED, bool(on)
    return old


def set_tail(kind):
    global _TAIL
    if kind not in ('ksum', 'tconv'):
        raise ValueError('frozen_in: stage 2 runs on "ksum" or "tconv"')
    old, _TAIL = _TAIL, kind
    return old


def own(block, min_tiles=None):
    _OWNED[block] = (None if min_tiles is None else int(min_tiles),)


def disown(block):
    _OWNED.pop(block, None)


def owned(block):
    return block in _OWNED


def _norms(block):
    return [op[1][1] for op in block.res_ops] + [op[0][1] for op in block.dw_ops] + [op[2][1] for op in block.dw_ops] + [block.pw_bn]


def _stateless_instance(block):
    return all(type(m) is cnn.InstanceNorm2d and not m.track_running_stats for m in _norms(block))


def own_network(net, min_tiles=None):
    """Register every InvertedResidualChannels block of `net` whose norms are InstanceNorm2d without running statistics; -> the blocks."""
    from .inception_modules import InvertedResidualChannels
    blocks = [m for m in net.modules() if isinstance(m, InvertedResidualChannels) and len(m.res_ops) + len(m.dw_ops) > 0 and _stateless_instance(m)]
    for b in blocks:
        own(b, min_tiles)
    return blocks


def dw_launches(quads, maxq=L.DWM_MAXQ):
    """fused_unit.dw_launches with the forward kernel's launch width: this forward-only path's grouping (the teacher's 3 x 11 quads: 22 + 11)."""
    return U.dw_launches(quads, maxq)


def applicable(block, x):
    if not _ENABLED or block.training or torch.is_grad_enabled() or not x.is_cuda:
        return False
    owner = _OWNED.get(block)
    if owner is None or block.padding_type not in ('reflect', 'zero'):
        return False
    if len(block.res_ops) + len(block.dw_ops) == 0 or len(block.res_ops) + len(block.dw_ops) > L.TCONV_MAXSEG or not ops.is_act(x):
        return False
    n, c, h, w = x.shape
    if not ops.tconv_applicable(n, h, w, c, 3, 3, 1, 1, min_tiles=owner[0]):
        return False
    if not _stateless_instance(block) or any(m.training for m in _norms(block)):
        return False
    if fused_block._dropout(block) != (0.0, frozenset()):      # an active Dropout: general path
        return False
    first_act = block.res_ops[0][1][2] if len(block.res_ops) else block.dw_ops[0][0][2]
    if cnn._act_code(first_act)[0] not in (L.ACT_RELU, L.ACT_LRELU):
        return False
    ks = [op[1][0].kernel_size[0] for op in block.res_ops] + [op[2][0].kernel_size[0] for op in block.dw_ops]
    if any(k not in ((1, 3, 5, 7) if fused_block._K7 else (1, 3, 5)) for k in ks):      # 7 x 7 branches: under the fused block's own switch (CAT_FUSED_K7)
        return False
    if dw_launches([U.cs4(op[0][0].out_channels) // 4 for op in block.dw_ops]) is None:
        return False
    return not U.has_hooks(block.children())      # (hooks on the block itself -- the distiller's taps -- fire as always)


def dw_filter_segment(dws, cout, dev):
    """The 1 x 1 second convs of the depthwise branches as ONE K segment: [cout, hcd, 1, 1] in kernel layout with branch b's channels at
    its slot offset b['od'] of the depthwise buffer Zd and zeros in the slots' padding channels."""
    hcd = sum(U.cs4(b['m']) for b in dws)
    wcat = ops.padded_weight_like((cout, hcd, 1, 1), dev)
    for b in dws:
        wcat[:, b['od']:b['od'] + b['m']].copy_(b['conv2'].weight.detach())
    return wcat


def _dw_filters(block, p):
    key = optim.weights_key(list(block.parameters()) + list(block.buffers()))
    return derived.lookup(block, FROZEN_IN, key, lambda prev: dw_filter_segment(p.dws, p.Cout, p.dev))


def _wide_segs(block, p, z1, ss1, zd, ssd):
    """Stage 2 for the wide tile: one segment per residual branch (its slice of Z1), all depthwise slices of Zd as one."""
    slab = lambda buf, o, c: buf[..., o:o + c].permute(0, 3, 1, 2)
    aff = lambda ss, o, stride: dict(scale=ss[0].data_ptr() + 4 * o, shift=ss[1].data_ptr() + 4 * o, sstride=stride, act=p.act, slope=p.slope)
    res = {k: [ksum.NormSegment(slab(z1, b['o1'], b['m']), b['conv2'].weight, p.reflect and b['k'] > 1, **aff(ss1, b['o1'], p.hc1))
               for b in p.res if b['k'] == k] for k in (1, 3, 5)}
    dw = []
    if p.dws:
        dw = [ksum.NormSegment(slab(zd, 0, p.hcd), _dw_filters(block, p), False, cin=sum(b['m'] for b in p.dws), **aff(ssd, 0, p.hcd))]
    return res[1] + dw + res[3] + res[5]


def block_forward(block, x):
    x = ops.conform(x)
    p = fused_block.plan_for(block, x, L.DWM_MAXQ)      # forward only: launches of up to CAT_DWM_MAXQ quads, their filter frames cut by the plan
    p.prepare()
    p.shards = 1
    n, c, h, w = x.shape
    dev = x.device
    tiles = n * ((h + 7) // 8) * ((w + 15) // 16)
    run = fused_block._run
    # ---- stage 1 -> Z1, per-sample scale / shift
    z1 = torch.empty((n, h, w, p.hc1), device=dev, dtype=torch.float32)
    part1 = torch.empty((tiles, 2, p.hc1), device=dev, dtype=torch.float32)
    U.stage1(p, x, z1, part1, p.reflect)
    ss1 = run(U.finalize_g(p, part1, p.hc1, n, h, w, p.gamma1, p.beta1, [(b['o1'], b['m'], b['bn1']) for b in p.branches], sync=None))[0]
    # ---- depthwise stage -> Zd
    zd = ssd = None
    if p.dws:
        zd = torch.empty((n, h, w, p.hcd), device=dev, dtype=torch.float32)
        partd = torch.empty((tiles, 2, p.hcd), device=dev, dtype=torch.float32)
        U.dwm_fwd(p, z1, ss1[0], ss1[1], zd, partd, p.reflect, True)
        ssd = run(U.finalize_g(p, partd, p.hcd, n, h, w, p.gammad, p.betad, [(b['od'], b['m'], b['bn2']) for b in p.dws], sync=None))[0]
    # ---- stage 2: T = the branch sum, + pw_bn's statistics
    t = ops.empty_act(n, c, h, w, dev)
    pw = block.pw_bn
    bias2 = p.bias2 if p.has_bias2 else None
    # the wide tile's domain is kernel sizes 1, 3, 5: a plan with a 7 x 7 branch always takes the LDS-tile tail (conv_pk7.hip)
    wide = _wide_segs(block, p, z1, ss1, zd, ssd) if _TAIL == 'ksum' and all(b['k'] != 7 for b in p.res) else None
    if wide is not None and ksum.norm_applicable(wide, n, h, w, c):
        partp, th, tw = ksum.run_norm(wide, bias2, t)
        ssp = torch.empty((2, n, p.cs), device=dev, dtype=torch.float32)
        mrp = torch.empty((2, n, c), device=dev, dtype=torch.float32)
        gp, bp = (ops._p(pw.weight), ops._p(pw.bias)) if p.affine else (None, None)
        L.call('cat_tnorm_finalize2', ops._p(partp), p.cs, n, n, h, w, th, tw, 1, gp, bp, 1, U.slices([(0, c, pw)]), p.eps, p.momentum, ops._p(ssp[0]),
               ops._p(ssp[1]), ops._p(mrp[0]), ops._p(mrp[1]), c, ops._stream())
    else:
        segs = U.stage2_segs(p, z1, ss1, zd, ssd, p.reflect, True)
        partp = torch.empty((tiles, 2, p.cs), device=dev, dtype=torch.float32)
        tconv.run(segs, p.pack2, bias2, t, c, n, h, w, h, w, stats=partp, scs=p.cs)
        ssp = run(U.finalize_g(p, partp, p.cs, n, h, w, pw.weight, pw.bias, [(0, c, pw)], sync=None, mstride=c))[0]
    # ---- out = x + pw_bn(T)
    y = ops.empty_act(n, c, h, w, dev)
    L.call('cat_affine_res_fwd', ops._p(t), p.cs, ops._p(ssp[0]), ops._p(ssp[1]), p.cs, ops._p(x), ops.act_cs(x), ops._p(y), p.cs, n, h * w, p.cs,
           L.ACT_NONE, 0.0, ops._stream())
    return y
