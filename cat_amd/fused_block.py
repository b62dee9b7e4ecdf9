"""Fused training-mode path of InvertedResidualChannels (reference models/modules/inception_modules.py:124-180, 230-236):

    x + pw_bn( sum_k conv2_k(relu(norm(conv1_k(x)))) + sum_k pw2_k(relu(norm(dw_k(relu(norm(pw1_k(x))))))) )

with train-mode BatchNorm2d / InstanceNorm2d in every position.  The general path launches ~55 kernels per block (12 convs, 10 norms
x 3, add_n, ...), most of them a few microseconds of HBM-bound work between dependent launches.  Here a block is 9 launches:

    stage 1   one LDS-tile conv launch per first-conv kernel size (the 1x1 convs of all branches as ONE N-concatenated GEMM) writing
              channel slices of one pre-norm buffer Z1 and the per-tile statistics of every branch           (cat_tconv_fwd + stats)
    finalize  scale / shift of all stage-1 norms + their running statistics                                   (cat_tnorm_finalize)
    dw        all depthwise convs as one launch; normalise + ReLU of stage 1 applied while staging            (cat_dwm_fwd)
    finalize
    stage 2   the branch sum: six second convs K-concatenated into one launch, normalise + ReLU applied while staging, output
              written once, statistics for pw_bn                                                              (cat_tconv_fwd)
    finalize, out = x + T * scale + shift                                                                     (cat_affine_res_fwd)

Filter streams, concatenated gamma / beta / bias vectors and the depthwise filter frame are refreshed by ONE table-driven launch per
block and optimizer step (cat_prep_run).  The backward pass re-materialises the two hidden activations (one pass each) and then runs
the branch-wise weight-gradient kernels on channel slices; the six first-conv input gradients are one K-concatenated launch.
The layout (`_Plan`), the operand preparation and the stages the block shares with the GauGAN generator's six-branch units live in
cat_amd/fused_unit.py; here: the closing pw_bn, InstanceNorm, reflect padding, dropout and the one-stream weight-gradient route.
Same arithmetic as the general path (same conv accumulation order per output, statistics merged pairwise instead of sequentially):
results agree to ~1e-6 relative; tests/test_fused_block_gpu.py pins both against the CPU oracle."""
import ctypes as C
import os

import torch

from . import _lib as L
from . import nn as cnn
from . import ops
from . import optim
from . import rng
from . import tconv
from . import fused_unit as U
from .fused_unit import prepare_many, prepare_plans      # noqa: F401  (the generator's per-step preparation: inception_generator.py)

_ENABLED = os.environ.get('CAT_FUSED_BLOCK', '1') != '0'


def set_enabled(on):
    global _ENABLED
    _ENABLED = bool(on)


def _dropout(block):
    """-> (p, {j of the branches whose Dropout is active}) -- Dropout j = res branches first, then dw branches -- or None when the active
    Dropouts of the block disagree on p (general path).  p == 0: no Dropout is active (eval mode or rate 0) and nothing is launched."""
    mods = [op[2] for op in block.res_ops] + [op[3] for op in block.dw_ops]
    act = {j: float(m.p) for j, m in enumerate(mods) if isinstance(m, cnn.Dropout) and m.training and m.p != 0}
    if len(set(act.values())) > 1:
        return None
    return (next(iter(act.values())) if act else 0.0), frozenset(act)


def applicable(block, x):
    if not _ENABLED or not block.training or not x.is_cuda or block.padding_type not in ('reflect', 'zero'):
        return False
    if _dropout(block) is None:
        return False
    if len(block.res_ops) + len(block.dw_ops) == 0 or not ops.is_act(x):
        return False
    n, c, h, w = x.shape
    if not ops.tconv_applicable(n, h, w, c, 3, 3, 1, 1):
        return False
    norms = [op[1][1] for op in block.res_ops] + [op[0][1] for op in block.dw_ops] + [op[2][1] for op in block.dw_ops] + [block.pw_bn]
    kind = type(norms[0])
    if kind not in (cnn.BatchNorm2d, cnn.InstanceNorm2d) or any(type(m) is not kind for m in norms):
        return False
    if kind is cnn.BatchNorm2d and any(m.momentum is None or not m.track_running_stats for m in norms):
        return False
    if kind is cnn.InstanceNorm2d and any(m.track_running_stats for m in norms):
        return False
    first_act = block.res_ops[0][1][2] if len(block.res_ops) else block.dw_ops[0][0][2]
    if cnn._act_code(first_act)[0] not in (L.ACT_RELU, L.ACT_LRELU):     # the staging paths apply ReLU / LeakyReLU only (nn.ReLU6: general path)
        return False
    ks = [op[1][0].kernel_size[0] for op in block.res_ops] + [op[2][0].kernel_size[0] for op in block.dw_ops]
    if any(k not in (1, 3, 5) for k in ks):
        return False
    if sum(U.cs4(op[0][0].out_channels) for op in block.dw_ops) > 4 * L.DWM_MAXQ_BWD or len(block.res_ops) + len(block.dw_ops) > L.TCONV_MAXSEG:
        return False
    return not U.has_hooks(block.children())


class _Plan(U.Plan):
    """The layout of one block (C_in = C_out = C) + what its closing pw_bn, padding and norm kind add."""
    what = 'fused block'

    def __init__(self, block, dev):
        self.block = block
        for m in block.modules():       # conv weights into the kernels' [O][kh][kw][round_up(I, 4)] storage (as Conv2d.forward does lazily)
            if isinstance(m, cnn.Conv2d) and m.groups == 1:
                cnn._to_channels_last_(m)
        self.reflect = block.padding_type == 'reflect'
        first_act = (block.res_ops[0][1][2] if len(block.res_ops) else block.dw_ops[0][0][2])
        self.act, self.slope = cnn._act_code(first_act)
        self.instance = isinstance(block.pw_bn, cnn.InstanceNorm2d)
        pw = block.pw_bn
        self.eps, self.momentum = float(pw.eps), float(pw.momentum if pw.momentum is not None else 0.0)
        self.affine = pw.weight is not None
        # j: the branch's Dropout index inside the block (res branches first, then dw branches; the general path's order)
        res = [dict(kind='res', j=i, k=op[1][0].kernel_size[0], m=op[1][0].out_channels, conv1=op[1][0], bn1=op[1][1], conv2=op[4])
               for i, op in enumerate(block.res_ops)]
        dws = [dict(kind='dw', j=len(res) + i, k=1, kd=op[2][0].kernel_size[0], m=op[0][0].out_channels, conv1=op[0][0], bn1=op[0][1],
                    dconv=op[2][0], bn2=op[2][1], conv2=op[4]) for i, op in enumerate(block.dw_ops)]
        super().__init__(res, dws, block.input_dim, block.input_dim, dev, list(block.parameters()))
        self.C, self.cs = self.Cin, self.csi

    def _merges_dw_dgrad(self):
        return len(self.dws) > 1

    def prepare(self, backward=False):
        """Refresh the derived operands if a weight changed since the last refresh (once per optimizer step)."""
        group = getattr(self, 'group', None)
        if backward and group is not None:
            prepare_many(group, backward=True)      # the first backward of the step refreshes every block of the generator in ONE launch
        self._prepare_own(backward)


def plan_for(block, x):
    p = getattr(block, '_cat_fused_plan', None)
    # the plan holds Parameter OBJECTS (gradient targets are keyed by identity): a parameter replaced by one of the same shape
    # (module.weight = nn.Parameter(...), weight transfer) invalidates it like a shape change does
    if p is None or p.dev != x.device or p.shapes != tuple(tuple(q.shape) for q in block.parameters()) or \
            p.ids != tuple(id(q) for q in block.parameters()):
        p = _Plan(block, x.device)
        block._cat_fused_plan = p
    return p


def _slices(pairs):
    arr = (L.NSlice * len(pairs))()
    for i, (c0, c, bn) in enumerate(pairs):
        arr[i].c0, arr[i].c = c0, c
        track = isinstance(bn, cnn.BatchNorm2d) and bn.training and bn.track_running_stats
        arr[i].running_mean = bn.running_mean.data_ptr() if track else None
        arr[i].running_var = bn.running_var.data_ptr() if track else None
        arr[i].num_batches = bn.num_batches_tracked.data_ptr() if track else None
    return arr


def _finalize(p, part, scs, n, h, w, gamma, beta, pairs, mstride=None):
    """-> (ss, mr): ss[0] / ss[1] = scale / shift [G][scs]; mr[0] / mr[1] = mean / rstd [G][mstride] (kept for the backward pass)."""
    G = n if p.instance else 1
    mstride = scs if mstride is None else mstride
    ss = torch.empty((2, G, scs), device=part.device, dtype=torch.float32)
    mr = torch.empty((2, G, mstride), device=part.device, dtype=torch.float32)
    sl = _slices(pairs)
    L.call('cat_tnorm_finalize', ops._p(part), scs, G, n, h, w, ops._p(gamma) if p.affine else None, ops._p(beta) if p.affine else None, len(pairs), sl,
           p.eps, p.momentum, ops._p(ss[0]), ops._p(ss[1]), ops._p(mr[0]), ops._p(mr[1]), mstride, ops._stream())
    return ss, mr


def forward(block, x, save=None):
    """The block's forward on the fused path.  `save`: dict that receives what the backward pass needs (None under no_grad)."""
    p = plan_for(block, x)
    p.prepare()
    n, c, h, w = x.shape
    dev = x.device
    tiles = n * ((h + 7) // 8) * ((w + 15) // 16)
    sstride_of = lambda scs: scs if p.instance else 0
    pdrop, djs = _dropout(block)
    ticket = rng.draw(dev) if pdrop else None       # one draw per block forward, as on the general path
    # ---- stage 1: first convs -> Z1 (pre-norm, concatenated) + tile statistics
    z1 = torch.empty((n, h, w, p.hc1), device=dev, dtype=torch.float32)
    part1 = torch.empty((tiles, 2, p.hc1), device=dev, dtype=torch.float32)
    U.stage1(p, x, z1, part1, p.reflect)
    st1 = _finalize(p, part1, p.hc1, n, h, w, p.gamma1, p.beta1, [(b['o1'], b['m'], b['bn1']) for b in p.branches])
    # ---- depthwise stage
    zd = std = None
    if p.dws:
        zd = torch.empty((n, h, w, p.hcd), device=dev, dtype=torch.float32)
        partd = torch.empty((tiles, 2, p.hcd), device=dev, dtype=torch.float32)
        U.dwm_fwd(p, z1, st1[0][0], st1[0][1], zd, partd, p.reflect, p.instance)
        std = _finalize(p, partd, p.hcd, n, h, w, p.gammad, p.betad, [(b['od'], b['m'], b['bn2']) for b in p.dws])
    # ---- dropout: the stage-2 operands are materialised (normalise + activation + mask) -- res slices of act(norm(Z1)) into A1, all of
    # act(norm(Zd)) into Ad -- and stage 2 stages them as they are
    a1 = ad = None
    if ticket is not None:
        a1, ad = _materialise(p, n, h, w, z1, st1, zd, std, pdrop, djs, ticket, dw_slices=False)
    # ---- stage 2: the branch sum, K-concatenated, normalise + activation applied while staging
    segs = U.stage2_segs(p, z1, st1[0], zd, std[0] if std is not None else None, p.reflect, p.instance, a1, ad)
    t = ops.empty_act(n, c, h, w, dev)
    partp = torch.empty((tiles, 2, p.cs), device=dev, dtype=torch.float32)
    tconv.run(segs, p.pack2, p.bias2 if p.has_bias2 else None, t, c, n, h, w, h, w, stats=partp, scs=p.cs)
    pw = block.pw_bn
    stp = _finalize(p, partp, p.cs, n, h, w, pw.weight, pw.bias, [(0, c, pw)], mstride=c)
    # ---- out = x + pw_bn(T)
    y = ops.empty_act(n, c, h, w, dev)
    G = n if p.instance else 1
    L.call('cat_affine_res_fwd', ops._p(t), p.cs, ops._p(stp[0][0]), ops._p(stp[0][1]), sstride_of(p.cs), ops._p(x), ops.act_cs(x), ops._p(y), p.cs, G,
           (n // G) * h * w, p.cs, L.ACT_NONE, 0.0, ops._stream())
    if save is not None:
        save.update(plan=p, z1=z1, zd=zd, t=t, st1=st1, std=std, stp=stp, drop=(pdrop, djs, ticket))
    return y


def _drop_segs(p, djs, kind):
    key = ('o1', 'res') if kind == 'res' else ('od', 'dw')
    return [(b[key[0]], b['m'], b['j']) for b in p.branches if b['kind'] == key[1] and b['j'] in djs]


def _materialise(p, n, h, w, z1, st1, zd, std, pdrop, djs, ticket, dw_slices):
    """A1 = act(norm(Z1)) with the res slices dropped (dw slices: written undropped iff dw_slices -- the backward pass's depthwise input
    gradient needs them, stage 2 does not) and Ad = act(norm(Zd)) dropped; one cat_dropout_apply launch each."""
    dev, npix = z1.device, n * h * w
    sstride_of = lambda scs: scs if p.instance else 0
    a1 = torch.empty((n, h, w, p.hc1), device=dev, dtype=torch.float32)
    rest = dw_slices or any(b['j'] not in djs for b in p.res)      # (res slices whose Dropout is off are written too)
    g = ops.dropout_geom(npix, p.hc1, p.hc1, p.hc1, pdrop, _drop_segs(p, djs, 'res'), mode=L.DROP_NORM, rest=int(rest), hw=h * w,
                         sstride=sstride_of(p.hc1), act=p.act, slope=p.slope)
    if p.res or dw_slices:
        ops.dropout_apply(g, z1, a1, ticket, st1[0][0], st1[0][1])
    ad = None
    if p.dws:
        ad = torch.empty((n, h, w, p.hcd), device=dev, dtype=torch.float32)
        g = ops.dropout_geom(npix, p.hcd, p.hcd, p.hcd, pdrop, _drop_segs(p, djs, 'dw'), mode=L.DROP_NORM, rest=1, hw=h * w, sstride=sstride_of(p.hcd),
                             act=p.act, slope=p.slope)
        ops.dropout_apply(g, zd, ad, ticket, std[0][0], std[0][1])
    return a1, ad


# ---------------------------------------------------------------------------------------------------------------- backward
def _norm_bwd(p, n, hw, c, cs, x, dy, gamma, beta, mr, act, slope, dgamma, dbeta, accumulate=0):
    """cat_norm_bwd over (a concatenation of) train-mode norms: dx, and d gamma / d beta into the given buffers."""
    g = L.NormGeom(n, hw, c, cs, L.NORM_INSTANCE if p.instance else L.NORM_BATCH, p.eps, p.momentum, act, slope)
    dx = torch.empty((n, hw, cs), device=x.device, dtype=torch.float32)
    ws = ops.workspace(L.query('cat_norm_ws_bytes', C.byref(g)), x.device)
    L.call('cat_norm_bwd', C.byref(g), ops._p(x), ops._p(dy), ops._p(gamma), ops._p(beta), ops._p(mr[0]), ops._p(mr[1]), ops._p(dx), ops._p(dgamma),
           ops._p(dbeta), accumulate, ops._p(ws), ops._stream())
    return dx


class _BlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, block, *params):
        x = ops.conform(x)
        save = {}
        y = forward(block, x, save)
        ctx.block, ctx.plan = block, save['plan']
        ctx.has_dw = save['zd'] is not None
        ctx.pdrop, ctx.djs, ticket = save['drop']
        tensors = [x, save['z1'], save['t'], save['st1'][0], save['st1'][1], save['stp'][0], save['stp'][1]]
        if ctx.has_dw:
            tensors += [save['zd'], save['std'][0], save['std'][1]]
        if ticket is not None:
            tensors.append(ticket)
        ctx.save_for_backward(*tensors)
        return y

    @staticmethod
    def backward(ctx, dy):
        p, block = ctx.plan, ctx.block
        saved = ctx.saved_tensors
        x, z1, t, ss1, mr1, ssp, mrp = saved[:7]
        zd, ssd, mrd = saved[7:10] if ctx.has_dw else (None, None, None)
        ticket = saved[-1] if ctx.pdrop else None
        dy = ops.conform(dy)
        p.prepare(backward=True)
        n, c, h, w = x.shape
        dev, hw, m_pix = x.device, h * w, n * h * w
        st = ops._stream()
        grads = {}
        pad_mode = L.PAD_REFLECT if p.reflect else L.PAD_ZERO

        side = ops.SideJobs(dev)      # the temporaries its launches read (a1, ad, dt, dz1) stay referenced by this frame until side.join()

        def put_side(param, kernel):       # weight-gradient launches: independent of the data-gradient chain -> side streams
            def job():
                grads[id(param)] = ops._write_param_grad(param, lambda dst_, acc: kernel(dst_, acc, ops._stream()))
            side.run(job)

        # one stream (the inception distillers' default): the weight-gradient producers run back to back at the end and their partial sums
        # are reduced by ONE launch (ops.WgradBatch); with side streams on they stay separate jobs
        batch = None if ops.branch_streams_enabled() else ops.WgradBatch(dev, grads)

        def put_wgrad(param, make):      # make(dst) -> (geometry, x pointer, dy pointer)
            if batch is not None:
                return batch.add(param, make)

            put_side(param, lambda dst_, acc, sst: U.wgrad(*make(dst_), dst_, acc, sst))

        def put_wgrad_into(dst, geom, xp, dyp):      # merged launches: destination = a gradient view of the plan, overwritten
            if batch is not None:
                return batch.add_into(dst, 0, geom, xp, dyp)
            side.run(lambda: U.wgrad(geom, xp, dyp, dst, 0, ops._stream()))

        # ---- 1. pw_bn: dT from dy (the skip connection's share of dy is added at the very end)
        pw = block.pw_bn
        if ops.act_cs(dy) != p.cs:
            raise RuntimeError('fused block backward: gradient pixel stride differs from the activation')
        if pw.weight is not None:
            sink = optim.claim([pw.weight, pw.bias], 'fused block backward')       # FusedAdam-owned: written (or accumulated) in place
            (dgp, dbp), acc = sink or ((torch.empty_like(pw.weight), torch.empty_like(pw.bias)), 0)
            dt = _norm_bwd(p, n, hw, c, p.cs, t, dy, pw.weight, pw.bias, mrp, L.ACT_NONE, 0.0, dgp, dbp, acc)
            if sink is None:
                grads[id(pw.weight)], grads[id(pw.bias)] = optim.deliver(pw.weight, dgp), optim.deliver(pw.bias, dbp)
        else:
            dt = _norm_bwd(p, n, hw, c, p.cs, t, dy, None, None, mrp, L.ACT_NONE, 0.0, None, None)
        # ---- 2. re-materialise the hidden activations (inputs of the second convs / of the depthwise convs); with dropout the forward's
        # masks are re-derived from its ticket: res slices of A1 and all of Ad dropped, the dw slices of A1 (depthwise inputs) not
        if ticket is not None:
            a1, ad = _materialise(p, n, h, w, z1, (ss1, None), zd, (ssd, None), ctx.pdrop, ctx.djs, ticket, dw_slices=True)
        else:
            a1 = U.rematerialise(p, z1, ss1, p.instance)
        da1 = torch.empty((n, h, w, p.hc1), device=dev, dtype=torch.float32)
        dad = None
        if ctx.has_dw:
            if ticket is None:
                ad = U.rematerialise(p, zd, ssd, p.instance)
            dad = torch.empty((n, h, w, p.hcd), device=dev, dtype=torch.float32)
        else:
            ad = None
        # ---- 3. second convs: weight gradients from (hidden activation slice, dT); input gradients into slices of dA1 / dAd
        side.fork()
        for b in p.branches:
            res = b['kind'] == 'res'
            k2, m, w1 = b['k2'], b['m'], b['w1']
            pad2 = (k2 - 1) // 2
            src, scs_, o = (a1, p.hc1, b['o1']) if res else (ad, p.hcd, b['od'])
            dst, dcs = (da1, p.hc1) if res else (dad, p.hcd)
            xptr = C.c_void_p(src.data_ptr() + 4 * o)
            mode2 = pad_mode if pad2 > 0 else L.PAD_ZERO
            conv2 = b['conv2']

            def kw(dst_, xptr=xptr, m=m, scs_=scs_, k2=k2, pad2=pad2, mode2=mode2):
                return ops._conv_geom(n, h, w, m, scs_, h, w, c, p.cs, k2, k2, 1, pad2, mode2, wcs=ops._grad_wcs(dst_)), xptr, ops._p(dt)
            if res or not p.merge2:
                put_wgrad(conv2.weight, kw)
            if not res and p.dpack2_dw is not None:
                continue            # input gradient: the merged launch below
            seg_pad = k2 - 1 - (0 if mode2 == L.PAD_REFLECT else pad2)
            seg = tconv.Segment(None, k2, seg_pad, False, b['d2off'], c4=p.cs, cin=c, xcs=p.cs, ptr=dt.data_ptr())
            if mode2 == L.PAD_REFLECT:
                dxp = torch.empty((n, h + 2 * pad2, w + 2 * pad2, w1), device=dev, dtype=torch.float32)
                tconv.run([seg], p.dpack2, None, dxp, m, n, h, w, h + 2 * pad2, w + 2 * pad2, ycs=w1, ycw=w1, yptr=dxp.data_ptr())
                L.call('cat_reflect_pad_bwd2', ops._p(dxp), w1, C.c_void_p(dst.data_ptr() + 4 * o), dcs, None, 0, n, h, w, w1, pad2, st)
            else:
                tconv.run([seg], p.dpack2, None, None, m, n, h, w, h, w, ycs=dcs, ycw=w1, yptr=dst.data_ptr() + 4 * o)
        if ctx.has_dw and p.dpack2_dw is not None:
            seg = tconv.Segment(None, 1, 0, False, 0, c4=p.cs, cin=c, xcs=p.cs, ptr=dt.data_ptr())
            tconv.run([seg], p.dpack2_dw, None, None, p.hcd, n, h, w, h, w, ycs=p.hcd, ycw=p.hcd, yptr=dad.data_ptr(), nvalid=sum(b['m'] for b in p.dws))
        if ticket is not None:      # gradients of the dropped activations -> of the activations: x keep * s (in place, before the norms)
            segs_r = _drop_segs(p, ctx.djs, 'res')
            if segs_r:
                ops.dropout_apply(ops.dropout_geom(m_pix, p.hc1, p.hc1, p.hc1, ctx.pdrop, segs_r, rest=0), da1, da1, ticket)
            segs_d = _drop_segs(p, ctx.djs, 'dw')
            if ctx.has_dw and segs_d:
                ops.dropout_apply(ops.dropout_geom(m_pix, p.hcd, p.hcd, p.hcd, ctx.pdrop, segs_d, rest=0), dad, dad, ticket)
        if p.merge2:      # d W2 of all depthwise branches: dT^T x Ad as ONE 1x1 weight-gradient launch over the concatenated hidden buffer
            put_wgrad_into(p.gv['w2'], ops._conv_geom(n, h, w, p.hcd, p.hcd, h, w, c, p.cs, 1, 1, 1, 0, L.PAD_ZERO, wcs=p.hcd), ops._p(ad), ops._p(dt))
        if p.has_bias2:
            U.channel_sum(dt, m_pix, c, p.cs, p.gv['c2'])
        # ---- 4. / 5. depthwise stage
        if ctx.has_dw:
            dzd = _norm_bwd(p, n, hw, p.hcd, p.hcd, zd, dad, p.gammad if p.affine else None, p.betad if p.affine else None, mrd, p.act, p.slope,
                            p.gv['gd'] if p.affine else None, p.gv['bd'] if p.affine else None)
            if p.has_biasd:
                U.channel_sum(dzd, m_pix, p.hcd, p.hcd, p.gv['cd'])
            U.dw_bwd(p, a1, da1, dzd, grads, p.reflect)
        # ---- 6. stage-1 norms (all branches at once)
        dz1 = _norm_bwd(p, n, hw, p.hc1, p.hc1, z1, da1, p.gamma1 if p.affine else None, p.beta1 if p.affine else None, mr1, p.act, p.slope,
                        p.gv['g1'] if p.affine else None, p.gv['b1'] if p.affine else None)
        if p.has_bias1:
            U.channel_sum(dz1, m_pix, p.hc1, p.hc1, p.gv['c1'])
        # ---- 7. first convs: weight gradients from (x, dZ1 slice)
        side.refork()
        if p.merge1 is not None:
            g1 = p.merge1
            put_wgrad_into(p.gv['w1'], ops._conv_geom(n, h, w, c, p.cs, h, w, g1['width'], p.hc1, 1, 1, 1, 0, L.PAD_ZERO, wcs=p.cs), ops._p(x),
                           C.c_void_p(dz1.data_ptr() + 4 * g1['off']))
        for b in p.branches:
            if p.merge1 is not None and b['k'] == 1:
                continue
            k, m = b['k'], b['m']
            pad1 = (k - 1) // 2
            mode1 = pad_mode if pad1 > 0 else L.PAD_ZERO
            dyp = C.c_void_p(dz1.data_ptr() + 4 * b['o1'])

            def kw1(dst_, dyp=dyp, m=m, k=k, pad1=pad1, mode1=mode1):
                return ops._conv_geom(n, h, w, c, p.cs, h, w, m, p.hc1, k, k, 1, pad1, mode1, wcs=ops._grad_wcs(dst_)), ops._p(x), dyp
            put_wgrad(b['conv1'].weight, kw1)
        if batch is not None:
            batch.flush()
        # ---- 8. first convs: the six input gradients as ONE K-concatenated launch (+ the skip connection's gradient)
        dx = None
        if ctx.needs_input_grad[0]:
            M = max((b['k'] - 1) // 2 for b in p.branches) if p.reflect else 0
            segs = U.dgrad1_segs(p, dz1, M)
            dx = ops.empty_act(n, c, h, w, dev)
            if M:
                dxp = torch.empty((n, h + 2 * M, w + 2 * M, p.cs), device=dev, dtype=torch.float32)
                tconv.run(segs, p.dpack1, None, dxp, c, n, h, w, h + 2 * M, w + 2 * M, ycs=p.cs, ycw=p.cs, yptr=dxp.data_ptr())
                L.call('cat_reflect_pad_bwd2', ops._p(dxp), p.cs, ops._p(dx), p.cs, ops._p(dy), ops.act_cs(dy), n, h, w, p.cs, M, st)
            else:
                tconv.run(segs, p.dpack1, None, dx, c, n, h, w, h, w, res=dy)
        side.join()
        # ---- 9. scatter the concatenated parameter gradients
        U.scatter_param_grads(p, grads)
        return (dx, None) + tuple(grads.get(id(q)) for q in block.parameters())


def apply(block, x):
    if not torch.is_grad_enabled():
        return forward(block, ops.conform(x))
    return _BlockFn.apply(x, block, *block.parameters())
