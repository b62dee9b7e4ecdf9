"""Frozen-teacher fast path for InvertedResidualChannels (reference inception_modules.py:124-180, 230-236).

In the distillation step the teacher runs in eval mode under no_grad (base_inception_distiller.py:168, inception_distiller.py:
100-103).  With BatchNorm (running statistics) every norm of a block is a per-channel affine map, so the block

    x + pw_bn( sum_k res_k(x) + sum_k dw_k(x) )

collapses algebraically -- same values, different evaluation order -- into

    A   one 1x1 conv  x -> [h_res1 | g_dw1 | g_dw3 | g_dw5]   (the four 256->42 convs + BN + ReLU as ONE GEMM with N = 176)
    dw  three depthwise convs (+ BN + ReLU in the epilogue) reading / writing channel SLICES of the concatenated buffers
    F   one 1x1 conv  [h_res1 | h_dw1 | h_dw3 | h_dw5] -> C  (the four 42->256 convs as ONE GEMM with K = 176; pw_bn's scale folded
        into its weights, every bias of the block and pw_bn's shift folded into its bias)
    k>1 res branches keep their first conv (+ BN + ReLU folded) -- with one 5 x 5 and one 3 x 3 branch of the teacher's widths they and A are
        ONE launch that stages x once per 16-channel chunk (cat_tstage1w_fwd); their second convs (pw_bn's scale folded in), F and the skip
    connection become ONE K-concatenated LDS-tile launch (csrc/conv_pk.hip): out = x + [h | hid3 | hid5] * [F ; W3 ; W5] + bias,
    written once -- on planes too small for that kernel: out = add_n(x, F, k3, k5)

    3 5 7 the reference's default kernel sizes (CAT_FROZEN_K7): three wide residual branches and three depthwise ones -- A is 256 -> 132, the
        depthwise stage one launch on a 7 x 7 filter frame (cat_dwconv2d_multi7_fwd), A and the 7 x 7, 5 x 5 and 3 x 3 first convs ONE launch
        (cat_tstage1w7_fwd, csrc/conv_s1w7.hip); the tail is the LDS-tile launch on the wide patch (csrc/conv_pk7.hip)

instead of 12 convs + 3 activations + add_n(6) + affine + add_n(2): the 42->256 1x1 layers were epilogue-bound (K = 44: 27 TFLOP/s),
and 10 of 18 full-size tensor passes disappear.  One-time weight folding is cached per block (invalidated when a tensor changes).
InstanceNorm teachers (CycleGAN configs) cannot be folded: the blocks a distiller owns take the forward-only fused pipeline of
cat_amd/frozen_in.py, every other eval-mode InstanceNorm block the general path."""
import ctypes as C
import os

import torch

from . import _lib as L
from . import derived
from . import nn as cnn
from . import ops
from . import optim


FROZEN = derived.slot('_cat_frozen')      # R5: the block's plan, keyed on every parameter and buffer of the block
_STAGE1W = True      # stage 1 of the block as one launch (cat_tstage1w_fwd); A/B closed in round 6: teacher forward 11.51 -> 11.15 ms
# Blocks with a 7 x 7 branch (the reference's parser default --kernel_sizes 3 5 7): the depthwise stage on a 7 x 7 frame
# (cat_dwconv2d_multi7_fwd) and stage 1 as one launch (cat_tstage1w7_fwd).  CAT_FROZEN_K7=0 / set_k7(False): the launches such a block
# issued before -- the 1 x 1 GEMM, one cat_dwconv2d_fwd per depthwise branch, one padded first conv per residual branch.  Read at every
# forward (the plan holds both forms); blocks without a 7 x 7 branch never look at it.
_K7 = os.environ.get('CAT_FROZEN_K7', '1') != '0'


def set_k7(on):
    global _K7
    old, _K7 = _K7, bool(on)
    return old


_affine = cnn.bn_affine


def _foldable(bn):
    return isinstance(bn, cnn.BatchNorm2d) and bn.track_running_stats and not bn.training


def applicable(block, x):
    if torch.is_grad_enabled() or block.training or not x.is_cuda or len(block.res_ops) + len(block.dw_ops) == 0:
        return False
    if getattr(block, '_cat_frozen_off', False):
        return False
    norms = [op[1][1] for op in block.res_ops] + [op[0][1] for op in block.dw_ops] + [op[2][1] for op in block.dw_ops] + [block.pw_bn]
    if not all(_foldable(n) for n in norms):
        return False
    if block.padding_type not in ('reflect', 'zero'):      # 'replicate' is a materialised pad: general path
        return False
    if any(isinstance(m, cnn.Dropout) and m.training and m.p != 0 for m in block.modules()):
        return False        # (a Dropout in eval mode is the identity, whatever the block's dropout_rate)
    return len(block.dw_ops) + sum(1 for op in block.res_ops if op[1][0].kernel_size[0] == 1) >= 2


def _plan(block):
    # weights owned by a FusedAdam change under torch's feet (raw-pointer kernels): such blocks -- a BatchNorm student run in eval mode by
    # evaluate_model between training steps -- re-fold after every optimizer step; the frozen teacher (no optimizer) folds once
    return derived.lookup(block, FROZEN, optim.weights_key(list(block.parameters()) + list(block.buffers())), lambda prev: _build_plan(block))


def frame_row(fs, k, ky, kx):
    """row of tap (ky, kx) of a k x k depthwise filter in the [fs * fs][C] frame of side fs: centred"""
    o = fs // 2 - k // 2
    return (o + ky) * fs + o + kx


def _build_plan(block):
    dev = block.pw_bn.running_mean.device
    cin = block.input_dim
    s_pw, t_pw = _affine(block.pw_bn)
    pad_mode = L.PAD_REFLECT if block.padding_type == 'reflect' else L.PAD_ZERO
    slots, wide = [], []          # slots: branches whose LAST conv is 1x1 (res k=1, every dw branch); wide: res branches with k > 1
    for op in block.res_ops:
        (slots if op[1][0].kernel_size[0] == 1 else wide).append(('res', op))
    for op in block.dw_ops:
        slots.append(('dw', op))
    offs, off = [], 0
    for kind, op in slots:
        m = (op[1][0] if kind == 'res' else op[0][0]).out_channels
        offs.append((off, m, ops.cs_for(m)))
        off += ops.cs_for(m)
    hc = off
    w_a = ops.padded_weight_like((hc, cin, 1, 1), dev)
    b_a = torch.zeros(hc, device=dev)
    w_f = ops.padded_weight_like((cin, hc, 1, 1), dev)
    b_f = t_pw.clone()
    dws = []
    act_mod = None
    for (kind, op), (o, m, sz) in zip(slots, offs):
        first = op[1] if kind == 'res' else op[0]             # ConvBNReLU: conv, norm, act
        conv, bn, act_mod = first[0], first[1], first[2]
        s1, t1 = _affine(bn)
        w_a[o:o + m].copy_(conv.weight.detach() * s1.view(-1, 1, 1, 1))
        b_a[o:o + m] = (conv.bias.detach() * s1 if conv.bias is not None else 0) + t1
        last = op[4]
        w_f[:, o:o + m].copy_(last.weight.detach() * s_pw.view(-1, 1, 1, 1))
        if last.bias is not None:
            b_f += last.bias.detach() * s_pw
        if kind == 'dw':
            dconv, dbn = op[2][0], op[2][1]
            s2, t2 = _affine(dbn)
            k = dconv.kernel_size[0]
            dws.append(dict(off=o, m=m, sz=sz, k=k, pad=(k - 1) // 2,
                            w=(dconv.weight.detach() * s2.view(-1, 1, 1, 1)).contiguous(),
                            b=((dconv.bias.detach() * s2 if dconv.bias is not None else 0) + t2).contiguous()))
    wides = []
    for kind, op in wide:
        last = op[4]
        w2 = ops.padded_weight_like(tuple(last.weight.shape), dev)
        w2.copy_(last.weight.detach() * s_pw.view(-1, 1, 1, 1))
        if last.bias is not None:
            b_f += last.bias.detach() * s_pw
        fconv, fbn = op[1][0], op[1][1]
        wf, bf = cnn._folded_eval_bn(fconv, fbn, 0)
        wides.append(dict(op=op, w2=w2, k=last.kernel_size[0], m=fconv.out_channels, wf=wf, bf=bf, act=cnn._act_code(op[1][2])))
    act, slope = cnn._act_code(act_mod)
    # all depthwise convs (+ the copy of the k = 1 residual branch's hidden slice) as ONE launch (cat_dwconv2d_multi_fwd): filters in a 5 x 5
    # frame [25][hc], folded bias, kernel size per channel quad.  The copy is k = 1 with centre weight 1: act(h) = h for an activation
    # that is idempotent (ReLU; LeakyReLU is not: slope^2 on negative values) -- anything else keeps the separate launches.  A 7 x 7
    # depthwise branch, and only that, makes it a 7 x 7 frame [49][hc] (cat_dwconv2d_multi7_fwd; dwm['fs'] = 7)
    dwm = None
    if dws and hc // 4 <= L.DWMULTI_MAXQ and all(d['k'] in (1, 3, 5, 7) for d in dws) and act in (L.ACT_RELU, L.ACT_NONE):
        fs = 7 if any(d['k'] == 7 for d in dws) else 5
        frame = torch.zeros((fs * fs, hc), device=dev)
        fbias = torch.zeros(hc, device=dev)
        ks = [1] * (hc // 4)
        for (kind, _), (o, m, sz) in zip(slots, offs):
            if kind == 'res':
                frame[fs * fs // 2, o:o + m] = 1.0
        for d in dws:
            k = d['k']
            for ky in range(k):
                for kx in range(k):
                    frame[frame_row(fs, k, ky, kx), d['off']:d['off'] + d['m']] = d['w'][:, 0, ky, kx]
            fbias[d['off']:d['off'] + d['m']] = d['b']
            for q in range(d['off'] // 4, (d['off'] + d['sz']) // 4):
                ks[q] = k
        dwm = dict(frame=frame.contiguous(), bias=fbias.contiguous(), ks=ks, fs=fs)
    # stage 1 in one launch: exactly one residual branch per wide kernel size + the concatenated 1 x 1 convs, the teacher's widths
    s1w = _stage1_plan('s1w', wides, (act, slope), w_a, b_a, hc) if _STAGE1W else None
    s1w7 = _stage1_plan('s1w7', wides, (act, slope), w_a, b_a, hc)
    # the k = 1 res slots come first and are contiguous from lane 0: ONE copy of their whole range.  cat_slice_channels writes all ycs lanes
    # of every pixel, so a copy per slot into h2 + 4 * o zeroed o floats of the next pixel (the slots before it) and, behind the last pixel,
    # o floats past the buffer
    res_w = sum(sz for (kind, _), (o, m, sz) in zip(slots, offs) if kind == 'res')
    assert all(o < res_w for (kind, _), (o, m, sz) in zip(slots, offs) if kind == 'res')
    return dict(s1w=s1w, s1w7=s1w7, tail_pack=None, tail_offs=None, hc=hc, dwm=dwm, w_a=w_a, b_a=b_a.contiguous(), w_f=w_f, b_f=b_f.contiguous(), dws=dws, wides=wides, act=act, slope=slope,
                pad_mode=pad_mode, copies=[(0, res_w)] if res_w else [])


# The one-launch stage 1 of a frozen block, by plan key: (entry, width query, geometry struct, kernel sizes of the wide slots; the last
# slot is the concatenated 1 x 1 convs).  docs/CONV_VARIANTS.md, "Stage 1 in one launch"
_STAGE1 = {'s1w': ('cat_tstage1w_fwd', 'cat_tstage1w_supported', L.Stage1WGeom, (5, 3)),
           's1w7': ('cat_tstage1w7_fwd', 'cat_tstage1w7_supported', L.Stage1W7Geom, (7, 5, 3))}


def _stage1_plan(key, wides, act, w_a, b_a, hc):
    """The plan entry of _STAGE1[key], or None: the wide branches in slot order + the concatenated 1 x 1 convs (folded filters, folded
    biases, output channels; the packed filter streams are built at the first launch)."""
    _, query, _, sizes = _STAGE1[key]
    by_k = {wd['k']: wd for wd in wides}
    if len(wides) != len(sizes) or set(by_k) != set(sizes) or any(wd['act'] != act for wd in wides) or \
            not L.query(query, *[by_k[k]['m'] for k in sizes], hc):
        return None
    order = [by_k[k] for k in sizes]
    return dict(packs=None, ws=[wd['wf'] for wd in order] + [w_a], biases=[wd['bf'] for wd in order] + [b_a.contiguous()],
                m=[wd['m'] for wd in order] + [hc])


def _stage1_launch(key, p, x, refl):
    """Issues _STAGE1[key] on the plan entry p[key] -> (the concatenated 1 x 1 hidden buffer, {k: hidden buffer of the k x k branch})."""
    entry, _, geom, sizes = _STAGE1[key]
    s1 = p[key]
    if s1['packs'] is None:
        from . import tconv
        s1['packs'] = [tconv.pack(wt, tconv.FWD) for wt in s1['ws']]
    n, c, h, w = x.shape
    g = geom()
    g.N, g.H, g.W, g.xcs, g.cin = n, h, w, ops.act_cs(x), c
    g.reflect, g.act, g.slope = int(refl), p['act'], p['slope']
    bufs = [ops.empty_act(n, m, h, w, x.device) for m in s1['m']]
    for k, buf in enumerate(bufs):
        g.ycs[k], g.nvalid[k] = ops.act_cs(buf), s1['m'][k]
    arr = C.c_void_p * len(bufs)
    L.call(entry, C.byref(g), ops._p(x), arr(*[t.data_ptr() for t in s1['packs']]), arr(*[t.data_ptr() for t in s1['biases']]),
           arr(*[t.data_ptr() for t in bufs]), ops._stream())
    return bufs[-1], dict(zip(sizes, bufs))


def block_forward(block, x):
    p = _plan(block)
    x = ops.conform(x)
    n, c, h, w = x.shape
    hc = p['hc']
    m_pix = n * h * w
    refl = p['pad_mode'] == L.PAD_REFLECT
    # the 7 x 7 forms (CAT_FROZEN_K7): a mirrored 7 x 7 window needs a plane it fits in
    k7_ok = _K7 and (not refl or (h >= 7 and w >= 7))
    dwm = p['dwm'] if p['dwm'] is not None and (p['dwm']['fs'] == 5 or k7_ok) else None

    def dw_stage(hbuf):
        # every depthwise conv (+ folded BN + activation) and the k = 1 residual branch's copy as one launch
        h2 = ops.empty_act(n, hc, h, w, hbuf.device)
        gm = L.DwMulti()
        gm.N, gm.H, gm.W, gm.nq, gm.xcs, gm.ycs = n, h, w, hc // 4, hc, hc
        gm.reflect, gm.act, gm.slope = int(p['pad_mode'] == L.PAD_REFLECT), p['act'], p['slope']
        for q, k in enumerate(dwm['ks']):
            gm.ks[q] = k
        L.call('cat_dwconv2d_multi7_fwd' if dwm['fs'] == 7 else 'cat_dwconv2d_multi_fwd', C.byref(gm), ops._p(hbuf), ops._p(dwm['frame']),
               ops._p(dwm['bias']), ops._p(h2), ops._stream())
        return h2

    def concat_chain(xi):
        # A: every first-level 1x1 conv (+ folded BN + activation) as one GEMM
        stc = ops._stream()
        from . import ksum
        aseg = [ksum.Segment(xi, p['w_a'], False)]
        if ksum.applicable(aseg, n, h, w, hc):      # 176 wide: two 96-column tiles of the DMA-staged GEMM (8 % padding; 128-wide tiles: 31 %)
            hbuf = ksum.run(aseg, p['b_a'], ops.empty_act(n, hc, h, w, xi.device), act=p['act'], slope=p['slope'])
        else:
            hbuf = ops.Conv2dFn.apply(xi, p['w_a'], p['b_a'], 1, 0, L.PAD_ZERO, p['act'], p['slope'])
        if dwm is not None:
            h2 = dw_stage(hbuf)
            if fused_tail:
                return h2
            return ops.Conv2dFn.apply(h2, p['w_f'], p['b_f'], 1, 0, L.PAD_ZERO, L.ACT_NONE, 0.0)
        h2 = ops.empty_act(n, hc, h, w, xi.device)
        for o, sz in p['copies']:       # k = 1 res branch: its hidden activation already is the last conv's input
            L.call('cat_slice_channels', ops._p(hbuf), hc, o, sz, C.c_void_p(h2.data_ptr() + 4 * o), hc, m_pix, stc)
        for d in p['dws']:              # depthwise k x k (+ folded BN + activation) on a channel slice of the concatenated buffers
            g = ops._conv_geom(n, h, w, d['m'], hc, h, w, d['m'], hc, d['k'], d['k'], 1, d['pad'], p['pad_mode'], p['act'], p['slope'], d['sz'])
            L.call('cat_dwconv2d_fwd', C.byref(g), C.c_void_p(hbuf.data_ptr() + 4 * d['off']), ops._p(d['w']), ops._p(d['b']),
                   C.c_void_p(h2.data_ptr() + 4 * d['off']), stc)
        if fused_tail:
            return h2
        # F: every last 1x1 conv as one GEMM (pw_bn scale in the weights; all biases + pw_bn shift in the bias)
        return ops.Conv2dFn.apply(h2, p['w_f'], p['b_f'], 1, 0, L.PAD_ZERO, L.ACT_NONE, 0.0)

    def wide_chain(wd):
        def run(xi):
            op = wd['op']
            hid = op[1](op[0](xi))      # pad -> conv k x k with folded BN + activation (FusedSequential's frozen path)
            if fused_tail:
                return hid
            return ops.Conv2dFn.apply(hid, wd['w2'], None, 1, (wd['k'] - 1) // 2, p['pad_mode'], L.ACT_NONE, 0.0)
        return run

    fused_tail = ops.tconv_applicable(n, h, w, c, 3, 3, 1, 1) and 1 + len(p['wides']) <= L.TCONV_MAXSEG
    fns = [concat_chain] + [wide_chain(wd) for wd in p['wides']]
    s1 = 's1w7' if p['s1w7'] is not None and k7_ok else 's1w'
    if fused_tail and dwm is not None and p[s1] is not None:
        # every first conv of the block from one staging of x: the wide hidden buffers and the concatenated 1 x 1 one in one launch
        h1, hid = _stage1_launch(s1, p, x, refl)
        outs = [dw_stage(h1)] + [hid[wd['k']] for wd in p['wides']]
    elif ops.branch_streams_enabled() and len(fns) > 1:
        outs = ops.run_on_side_streams(fns, [x] * len(fns))
    else:
        outs = [fn(x) for fn in fns]
    if not fused_tail:
        return ops.AddNFn.apply(x, *outs)
    from . import ksum, tconv
    # wide output (the teacher's C = 256): the tail as ONE implicit GEMM on 128 x 128 tiles with both operands DMA-ed into LDS
    ksegs = [ksum.Segment(outs[0], p['w_f'], False)] + [ksum.Segment(hid, wd['w2'], refl) for wd, hid in zip(p['wides'], outs[1:])]
    if ksum.applicable(ksegs, n, h, w, c):
        return ksum.run(ksegs, p['b_f'], ops.empty_act(n, c, h, w, x.device), res=x)
    if p['tail_pack'] is None:      # packed filters of the fused tail (once per plan): segment 0 = F, then one segment per wide branch
        packs = [tconv.pack(p['w_f'], tconv.FWD)] + [tconv.pack(wd['w2'], tconv.FWD) for wd in p['wides']]
        offs, po = [], 0
        for pk in packs:
            offs.append(po)
            po += pk.numel()
        p['tail_pack'], p['tail_offs'] = torch.cat(packs), offs
    segs = [tconv.Segment(outs[0], 1, 0, False, p['tail_offs'][0])]
    for wd, hid, off in zip(p['wides'], outs[1:], p['tail_offs'][1:]):
        segs.append(tconv.Segment(hid, wd['k'], (wd['k'] - 1) // 2, refl, off))
    y = ops.empty_act(n, c, h, w, x.device)
    return tconv.run(segs, p['tail_pack'], p['b_f'], y, c, n, h, w, h, w, res=x)
