"""Fused training-mode path of the six-branch units of the GauGAN generator (reference models/modules/inception_modules.py:428-505,
549-562: SPADEInvertedResidualChannels; :648-700, 746-762: the gamma|beta net of InceptionSPADE):

    unit(x) = sum_k conv2_k(relu(bn(conv1_k(x)))) + sum_k pw2_k(relu(bn(dw_k(relu(bn(pw1_k(x))))))) [+ r]

with train-mode (Synchronized)BatchNorm2d in every position, zero ("same") padding, C_in != C_out in general and an optional addend r (the
block's shortcut).  The per-layer path launches ~45 kernels per unit (12 convs, 9 norms x 3, add_n); most of them HBM-bound passes over
hidden tensors of 1..13 channels on planes of up to 256 x 512 pixels.  Here a unit is the pipeline of cat_amd/fused_unit.py -- layout, operand
preparation and the stage sequence, forward and backward, defined once there and shared with the fused inception block:

    stage 1   first convs of all branches -> one concatenated pre-norm buffer Z1 + per-tile statistics   (cat_tstage1_fwd / cat_tconv_fwd;
              cat_tstage1n7_fwd for a unit with kernel sizes 3 5 7 under CAT_FUSED_SPADE_K7)
    finalize  scale / shift of all stage-1 norms + their running statistics                               (cat_tnorm_finalize)
    dw        all depthwise convs as one launch, norm + ReLU of stage 1 applied while staging             (cat_dwm_fwd)
    finalize
    stage 2   the branch sum: six second convs K-concatenated, norm + ReLU applied while staging, bias and the addend r in the epilogue

5 launches, no normalised tensor is ever written.  What this module gives the pipeline: zero padding and batch statistics (the plan's
defaults), the reducer of a SynchronizedBatchNorm over several ranks as its `sync` (one statistics exchange per stage and direction), the
folded running statistics as its `folded` (eval mode, no grad: 3 launches), never a dropout ticket, and p.s1d (the second convs' input
gradients as one launch).  What it keeps: when the path applies, the unit's plan, the stage-2 launch with the addend, the autograd
Functions and the drivers that perform the exchanges the pipeline asks for -- `_drive` for one unit, `_drive_many` for several
independent units in lockstep, their k-th exchanges merged into ONE collective (`prepass`: the gamma|beta nets of all SPADE layers).
Taken on planes of at least `ops._TCONV_MIN_TILES` 8 x 16 tiles (the 64 x 128 .. 256 x 512 stages at batch 4) and, under a multi-rank
reducer, for every unit the kernels can run; tests/test_spade_gpu.py::test_fused_spade_units_match_general_path pins it to the general path."""
import ctypes as C
import os

import torch

from . import _lib as L
from . import derived
from . import nn as cnn
from . import ops
from . import optim
from . import tconv
from . import fused_unit as U
from .fused_unit import Alloc      # what a unit generator asks its driver for (tests/test_host.py names it fused_spade.Alloc)

_ENABLED = os.environ.get('CAT_FUSED_SPADE', '1') != '0'      # A/B switch; 'train' / 'frozen' select one of the two forms
_ONLY = os.environ.get('CAT_FUSED_SPADE', '1') if os.environ.get('CAT_FUSED_SPADE', '1') in ('train', 'frozen') else None


_SYNC_FUSED = os.environ.get('CAT_FUSED_SPADE_SYNC', '1') != '0'      # fused units under SynchronizedBatchNorm over several ranks (round 4)
_S1_DGRAD = os.environ.get('CAT_FUSED_SPADE_S1_DGRAD', '1') != '0'     # A/B switch: the second convs' input gradients as one launch
# Units with a 7 x 7 branch (the reference's parser default --kernel_sizes 3 5 7) take this path under CAT_FUSED_SPADE_K7=1 / set_k7(True), in
# both forms: their 7 x 7 convs on the wide-patch LDS-tile kernels (csrc/conv_pk7.hip), their depthwise stage on the 7 x 7 frame
# (cat_dwm7_fwd / cat_dwm7_bwd), stage 1 and the second convs' input gradients as ONE launch each where the widths allow
# (cat_tstage1n7_fwd / cat_tstage1n7_dgrad, csrc/conv_s1n7.hip).  With it off such units run layer by layer, as they always did, and
# `applicable` is the function it was.  On by default: the graphed GauGAN distillation step with kernel sizes 3 5 7 at 512 x 256, batch 4,
# measured 73.52 ms on this path against 81.86 ms layer by layer (the parent commit), spreads 1.47 and 2.47 ms (profiles/spade_k7_bench.txt)
_K7 = os.environ.get('CAT_FUSED_SPADE_K7', '1') != '0'
_UNITS = os.environ.get('CAT_FUSED_SPADE_UNITS', 'all')      # A/B switch: 'gb' / 'main' = only the gamma|beta nets / only the main units
STATS = {'train_fwd': 0, 'frozen_fwd': 0, 'bwd': 0, 'collectives': 0}      # calls per form; statistics exchanges issued (tests / diagnostics)


def set_enabled(on):
    global _ENABLED
    _ENABLED = bool(on)


def set_k7(on):
    global _K7
    old, _K7 = _K7, bool(on)
    return old


def _conv_of(m):
    """nn.Conv2d behind a `Conv` wrapper (main branches) or the plain conv (gamma|beta nets)."""
    return m.conv if hasattr(m, 'conv') and not isinstance(m, cnn.Conv2d) else m


def _branches(res_ops, dw_ops):
    res = [dict(kind='res', k=op[0].conv.kernel_size[0], m=op[0].conv.out_channels, conv1=op[0].conv, bn1=op[0].norm, act=op[0].active,
                conv2=_conv_of(op[1])) for op in res_ops]
    dws = [dict(kind='dw', k=1, kd=op[1].conv.kernel_size[0], m=op[0].conv.out_channels, conv1=op[0].conv, bn1=op[0].norm, act=op[0].active,
                dconv=op[1].conv, bn2=op[1].norm, conv2=_conv_of(op[2])) for op in dw_ops]
    return res, dws


def applicable(res_ops, dw_ops, x, training):
    """training: the train-mode path (batch statistics, autograd).  not training: the frozen path -- eval-mode norms under no_grad (the
    teacher): the same three kernels with scale / shift folded from the running statistics, no statistics / finalize launches."""
    if not _ENABLED or not x.is_cuda or not ops.is_act(x):
        return False
    if _ONLY is not None and _ONLY != ('train' if training else 'frozen'):
        return False
    if training and ops.bn_sync() is not None and not _SYNC_FUSED:
        return False      # A/B switch: the per-layer path with one statistics exchange per norm layer
    if not training and torch.is_grad_enabled():
        return False
    if len(res_ops) + len(dw_ops) == 0 or len(res_ops) + len(dw_ops) > L.TCONV_MAXSEG:
        return False
    n, c, h, w = x.shape
    # planes too small to fill the chip run faster layer by layer on ONE GPU (split-K im2col kernels: 62.8 vs 60.9 images/s, round 3) -- but
    # layer by layer every norm is its own statistics exchange over the ranks (18 per unit against 4): under SynchronizedBatchNorm with
    # N > 1 ranks every unit the kernels can run is fused
    synced = training and ops.bn_sync() is not None and _SYNC_FUSED
    if not synced and not ops.tconv_applicable(n, h, w, 16, 3, 3, 1, 1):
        return False
    if c == 1:      # FusedAdam stores [m][1][1][1] weights unpadded (row stride 1): the merged first-conv gradient scatter writes cs4(Cin)-wide rows
        return False
    res, dws = _branches(res_ops, dw_ops)
    first = (res + dws)[0]
    act0 = cnn._act_code(first['act'])
    for b in res + dws:
        dw = b['kind'] == 'dw'
        convs = [b['conv1'], b['conv2']] + ([b['dconv']] if dw else [])
        if any('weight_orig' in cv._parameters or cv.stride[0] != 1 or cv.dilation != (1, 1) or cv.padding_mode != 'zeros' for cv in convs):
            return False      # spectral norm / strides / dilation: general path
        if b['conv1'].groups != 1 or b['conv2'].groups != 1 or (dw and b['dconv'].groups != b['m']):
            return False
        norms = [b['bn1']] + ([b['bn2']] if dw else [])
        if any(not isinstance(nm, cnn.BatchNorm2d) or nm.training != training or not nm.track_running_stats or nm.momentum is None for nm in norms):
            return False
        if training and any(nm.virtual_replicas > 1 for nm in norms):
            return False      # a BatchNorm2d stamped with virtual replicas takes its statistics per shard of the batch: the per-layer path
        # under a multi-rank reducer the fused stage finalize all-reduces the statistics and uses the clamp(var, eps) formula: that is
        # SynchronizedBatchNorm2d's arithmetic (sync_batchnorm/batchnorm.py:103-140).  A plain nn.BatchNorm2d (norm_G = 'spadebatch3x3') stays
        # per-replica in the reference (local statistics, var + eps): such units take the per-layer path, whose BatchNorm2d is never synced
        if synced and any(not isinstance(nm, cnn.SynchronizedBatchNorm2d) for nm in norms):
            return False
        # the plan keeps ONE (eps, momentum, activation) for the whole unit and assumes 'same' zero padding everywhere
        if any(float(nm.eps) != float(first['bn1'].eps) or float(nm.momentum) != float(first['bn1'].momentum) for nm in norms):
            return False
        if cnn._act_code(b['act']) != act0 or act0[0] not in (L.ACT_RELU, L.ACT_LRELU):
            return False
        k2 = 1 if dw else b['k']
        ks = [b['k'], b.get('kd', 1), b['conv2'].kernel_size[0]]
        if any(k not in ((1, 3, 5, 7) if _K7 else (1, 3, 5)) for k in ks) or b['conv2'].kernel_size[0] != k2:
            return False
        if b['conv1'].padding[0] != (b['k'] - 1) // 2 or b['conv2'].padding[0] != (k2 - 1) // 2:
            return False
        if dw and b['dconv'].padding[0] != (b.get('kd', 1) - 1) // 2:
            return False
    if sum(U.cs4(b['m']) for b in dws) > 4 * (L.DWM_MAXQ_BWD if training else L.DWM_MAXQ):
        return False
    return not U.has_hooks(list(res_ops) + list(dw_ops))


class _Plan(U.Plan):
    """The layout of one unit (C_in != C_out in general, 'same' zero padding, one (eps, momentum, activation) for all its norms)."""
    what = 'fused SPADE unit'
    GAMMA0 = 1.0      # non-affine norms (the depthwise branches' second norm of a SPADE block) read gamma = 1 / beta = 0 from the concatenated vectors

    def __init__(self, res_ops, dw_ops, cin, cout, dev):
        res, dws = _branches(res_ops, dw_ops)
        for b in res + dws:
            cnn._to_channels_last_(b['conv1'])
            cnn._to_channels_last_(b['conv2'])
        first = (res + dws)[0]
        self.act, self.slope = cnn._act_code(first['act'])
        self.eps, self.momentum = float(first['bn1'].eps), float(first['bn1'].momentum)
        params, seen = [], set()
        for m in list(res_ops) + list(dw_ops):
            for q in m.parameters():
                if id(q) not in seen:
                    seen.add(id(q))
                    params.append(q)
        # fused_unit.stage1 takes the narrow one-launch 3 5 7 kernel (cat_tstage1n7_fwd) only for plans that carry this
        self.stage1_n7 = _K7
        super().__init__(res, dws, cin, cout, dev, params)

    def _merges_dw_dgrad(self):
        """The second convs' input gradients as ONE launch (cat_tstage1_dgrad: dT is staged once for the 5 x 5 and the 3 x 3 residual branch
        and the N-concatenated 1 x 1 second convs of the depthwise branches; cat_tstage1n7_dgrad: the same with exactly one 7 x 7, one 5 x 5
        and one 3 x 3 residual branch, `s1d7`) where a kernel exists for the widths (fused_unit.STAGE1_DGRAD)."""
        for _, query, sizes, _, attr in U.STAGE1_DGRAD if _S1_DGRAD else ():
            rs = [[b for b in self.res if b['k'] == k] for k in sizes]
            if all(len(r) == 1 for r in rs) and self.dws and L.query(query, *[r[0]['w1'] for r in rs], self.hcd):
                setattr(self, attr, tuple(r[0] for r in rs))      # p.s1d7 / p.s1d: the residual branches of the launch, in slot order
                return True
        return False

    def prepare(self, backward=False):
        gref = getattr(self, 'group', None)      # weak reference to the generator that owns this unit (no cycle through the cached plans)
        group = gref() if gref is not None else None
        if group is not None and (self.bkey if backward else self.key) != self._epoch_key():
            # the first stale unit of a pass refreshes the operands of EVERY fused unit of the generator in one launch (round 4)
            U.prepare_plans(units_of(group), gref, backward)
        self._prepare_own(backward)


def units_of(generator):
    """Plans of every fused unit (main six-branch units and gamma|beta nets) built so far under `generator`, in module order."""
    out = []
    for m in generator.modules():
        for slot in (MAIN, GB):
            p = m.__dict__.get(slot)
            if p is not None:
                out.append(p)
    return out


MAIN, GB = derived.slot('_cat_fused_main'), derived.slot('_cat_fused_gb')      # R7: a block's main unit / a SPADE layer's gamma|beta net (the slot holds the plan)
EVAL_SS = derived.slot('eval_ss')      # R6: the eval scale / shift rows, on a unit's plan
PLAN_GEN = 0      # bumped whenever a unit plan is (re)built: generators regroup their units' operand preparation when it moves


def plan_for(owner, slot, res_ops, dw_ops, cin, cout, x):
    global PLAN_GEN
    p = getattr(owner, slot, None)
    params = [q for m in list(res_ops) + list(dw_ops) for q in m.parameters()]
    if p is None or p.dev != x.device or p.shapes != tuple(tuple(q.shape) for q in params) or p.ids != tuple(id(q) for q in params):
        p = _Plan(res_ops, dw_ops, cin, cout, x.device)
        setattr(owner, slot, p)
        PLAN_GEN += 1
    return p


def _drive(gen):
    """Run ONE unit generator to completion; every statistics exchange it asks for happens immediately (one collective each)."""
    try:
        req = next(gen)
        while True:
            if isinstance(req, Alloc):
                req = gen.send(torch.empty(req.n, device=req.device, dtype=torch.float32))
                continue
            ops.bn_sync().all_reduce_sum_(req)
            STATS['collectives'] += 1
            req = gen.send(None)
    except StopIteration as e:
        return e.value


def _drive_many(gens):
    """Run several INDEPENDENT unit generators in lockstep: the k-th exchanges of all of them travel as ONE collective (their buffers are
    summed element-wise either way: the same arithmetic per element as `_drive` on each; the reduction order is the backend's).  Units that
    ask for their buffer first (`Alloc`) get adjacent slices of one arena, and the collective is issued on the arena."""
    results, reqs = [None] * len(gens), {}
    for i, g in enumerate(gens):
        try:
            reqs[i] = next(g)
        except StopIteration as e:
            results[i] = e.value
    while reqs:
        allocs = [i for i in sorted(reqs) if isinstance(reqs[i], Alloc)]
        if allocs:
            dev = reqs[allocs[0]].device
            sizes = [(reqs[i].n + 3) // 4 * 4 for i in allocs]
            arena = torch.empty(sum(sizes), device=dev, dtype=torch.float32)
            o = 0
            for i, sz in zip(allocs, sizes):
                n = reqs[i].n
                try:
                    reqs[i] = gens[i].send(arena[o:o + n])
                except StopIteration as e:
                    results[i] = e.value
                    del reqs[i]
                o += sz
            continue
        order = sorted(reqs)
        ops.bn_sync().all_reduce_sum_many_([reqs[i] for i in order])
        STATS['collectives'] += 1
        nxt = {}
        for i in order:
            try:
                nxt[i] = gens[i].send(None)
            except StopIteration as e:
                results[i] = e.value
        reqs = nxt
    return results


def _branch_sum(p, x, segs, addend):
    """Stage 2: the K-concatenated branch sum over `segs`, bias and `addend` (NHWC activation [n, Cout, h, w], the block's shortcut, or None)
    in the epilogue."""
    n, _, h, w = x.shape
    y = ops.empty_act(n, p.Cout, h, w, x.device)
    tconv.run(segs, p.pack2, p.bias2 if p.has_bias2 else None, y, p.Cout, n, h, w, h, w, res=addend)
    return y


def _train_g(p, x, addend, save=None):
    """The train-mode unit as a generator over its statistics exchanges (U.finalize_g under the installed reducer, if any)."""
    STATS['train_fwd'] += 1
    p.prepare()
    z1, st1, zd, std, segs = yield from U.forward_g(p, x, sync=ops.bn_sync())
    if save is not None:
        save.update(z1=z1, zd=zd, st1=st1, std=std)
    return _branch_sum(p, x, segs, addend)


def forward(p, x, addend, save=None):
    """The unit's forward.  `addend`: NHWC activation [n, Cout, h, w] added in the epilogue (the block's shortcut) or None."""
    return _drive(_train_g(p, x, addend, save))


def _eval_affine(p):
    """scale / shift of every norm from its running statistics (eval mode), concatenated like the train-mode finalize output; cached until
    a tensor involved changes (the frozen teacher: once)."""
    tensors = []
    for b in p.branches:
        tensors += [b['bn1'].weight, b['bn1'].bias, b['bn1'].running_mean, b['bn1'].running_var]
    for b in p.dws:
        tensors += [b['bn2'].weight, b['bn2'].bias, b['bn2'].running_mean, b['bn2'].running_var]
    return derived.lookup(p, EVAL_SS, optim.weights_key(tensors), lambda prev: _fold_norms(p))


def _fold_norms(p):
    dev = p.dev
    ss1 = torch.zeros((2, max(p.hc1, 4)), device=dev, dtype=torch.float32)
    ssd = torch.zeros((2, max(p.hcd, 4)), device=dev, dtype=torch.float32)
    st = ops._stream()

    def fold(bn, dst, off, m):
        L.call('cat_bn_fold', ops._p(bn.weight), ops._p(bn.bias), ops._p(bn.running_mean), ops._p(bn.running_var), float(bn.eps), m,
               C.c_void_p(dst[0].data_ptr() + 4 * off), C.c_void_p(dst[1].data_ptr() + 4 * off), st)
    for b in p.branches:
        fold(b['bn1'], ss1, b['o1'], b['m'])
    for b in p.dws:
        fold(b['bn2'], ssd, b['od'], b['m'])
    return ss1, ssd


def forward_eval(p, x, addend):
    """The unit with eval-mode norms (no grad): stage 1 -> depthwise stage -> branch sum, the norms folded into the consumers' staging."""
    STATS['frozen_fwd'] += 1
    p.prepare()
    folded = _eval_affine(p)      # (held here until the branch sum that reads its rows is enqueued)
    return _branch_sum(p, x, _drive(U.forward_g(p, x, folded=folded))[4], addend)


class _UnitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, addend, plan, *params):
        x = ops.conform(x)
        if addend is not None:
            addend = ops.conform(addend)
        save = {}
        y = _drive(_train_g(plan, x, addend, save))
        ctx.plan = plan
        ctx.synced = ops.bn_sync() is not None      # statistics over all ranks: (a | b) saved instead of (mean | rstd)
        ctx.has_dw = save['zd'] is not None
        ctx.has_add = addend is not None
        tensors = [x, save['z1'], save['st1'][0], save['st1'][1]]
        if ctx.has_dw:
            tensors += [save['zd'], save['std'][0], save['std'][1]]
        ctx.save_for_backward(*tensors)
        return y

    @staticmethod
    def backward(ctx, dy):
        return _drive(_grad_g(ctx, dy))


def _grad_g(ctx, dy):
    """A unit's backward as a generator over its statistics exchanges.  `ctx`: anything with plan / synced / has_dw / has_add / saved_tensors /
    needs_input_grad (the autograd context of _UnitFn, or the per-unit record of _PrepassFn)."""
    p = ctx.plan
    STATS['bwd'] += 1
    saved = ctx.saved_tensors
    x, z1, ss1, mr1 = saved[:4]
    zd, ssd, mrd = saved[4:] if ctx.has_dw else (None, None, None)
    dt = ops.conform(dy)            # no closing norm: the gradient of the branch sum IS dy (and so is the addend's)
    if ops.act_cs(dt) != p.cso:
        raise RuntimeError('fused SPADE unit backward: gradient pixel stride differs from the activation')
    sync = ops.bn_sync() if ctx.synced else None
    if ctx.synced and sync is None:
        raise RuntimeError('fused SPADE unit backward: the forward ran under a SynchronizedBatchNorm reducer that is gone')
    p.prepare(backward=True)
    dx, grads = yield from U.backward_g(p, dt, x, z1, ss1, mr1, zd, ssd, mrd, need_dx=ctx.needs_input_grad[0], sync=sync)
    return (dx, dt if ctx.has_add else None, None) + tuple(grads.get(id(q)) for q in p.params)


class _Rec:
    """Per-unit stand-in for an autograd context inside _PrepassFn.backward (what _grad_g reads)."""
    __slots__ = ('plan', 'synced', 'has_dw', 'has_add', 'saved_tensors', 'needs_input_grad')


class _PrepassFn(torch.autograd.Function):
    """SEVERAL independent units as ONE autograd node (the gamma|beta nets of all SPADE layers of a generator: they read only the segmentation
    map, reference inception_modules.py:746-762).  Forward and backward run the units in lockstep (_drive_many): the k-th SynchronizedBatchNorm
    statistics exchanges of all units are one collective -- two per pass instead of two per unit -- and, being one node, the backward runs when
    the gradients of ALL outputs are there, so its exchanges batch the same way.  Arithmetic per unit is unchanged (bit-identical results)."""

    @staticmethod
    def forward(ctx, plans, nparams, *args):
        n = len(plans)
        xs = [ops.conform(t) for t in args[:n]]
        saves = [dict() for _ in plans]
        ys = _drive_many([_train_g(p, x, None, sv) for p, x, sv in zip(plans, xs, saves)])
        ctx.plans, ctx.nparams = plans, nparams
        ctx.synced = ops.bn_sync() is not None
        ctx.layout, tensors = [], []
        for x, sv in zip(xs, saves):
            t = [x, sv['z1'], sv['st1'][0], sv['st1'][1]]
            if sv['zd'] is not None:
                t += [sv['zd'], sv['std'][0], sv['std'][1]]
            ctx.layout.append(len(t))
            tensors += t
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)      # an output nobody used reaches backward as None (no dense NCHW zeros, no layout conversion)
        ctx.out_nhwc = [(y.shape[0], y.shape[2], y.shape[3], ops.act_cs(y), y.shape[1]) for y in ys]
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        saved, recs, o = ctx.saved_tensors, [], 0
        for p, cnt in zip(ctx.plans, ctx.layout):
            r = _Rec()
            r.plan, r.synced, r.has_dw, r.has_add = p, ctx.synced, cnt == 7, False
            r.saved_tensors, r.needs_input_grad = saved[o:o + cnt], (False, False)
            o += cnt
            recs.append(r)
        # an output nobody used arrives as None: its unit still has to step through the lockstep exchanges (every rank does the same)
        dys = [dy if dy is not None else torch.zeros(shape[:4], device=saved[0].device, dtype=torch.float32).permute(0, 3, 1, 2)[:, :shape[4]]
               for dy, shape in zip(dys, ctx.out_nhwc)]
        outs = _drive_many([_grad_g(r, dy) for r, dy in zip(recs, dys)])
        grads = []
        for out in outs:
            grads += list(out[3:])
        return (None, None) + (None,) * len(ctx.plans) + tuple(grads)


_PREPASS = os.environ.get('CAT_FUSED_SPADE_PREPASS', '1') != '0'      # A/B switch (round 5)


def set_prepass(on):
    global _PREPASS
    old, _PREPASS = _PREPASS, bool(on)
    return old


def prepass(units):
    """units: [(owner, res_ops, dw_ops, cin, cout, x)] of independent train-mode units whose input needs no gradient (gamma|beta nets on
    the segmentation pyramid).  Returns their outputs, computed in lockstep with merged statistics exchanges, or None if that does not apply
    (no multi-rank reducer, switch off, a unit the fused path does not take): the caller then runs the units one by one as before."""
    if not _PREPASS or ops.bn_sync() is None or not _SYNC_FUSED or _UNITS not in ('all', 'gb') or len(units) < 2:
        return None
    xs = [ops.conform(u[5]) for u in units]
    if any(x.requires_grad for x in xs) or not all(applicable(u[1], u[2], x, True) for u, x in zip(units, xs)):
        return None
    plans = tuple(plan_for(u[0], GB, u[1], u[2], u[3], u[4], x) for u, x in zip(units, xs))
    STATS['prepass'] = STATS.get('prepass', 0) + 1
    if not torch.is_grad_enabled():
        return _drive_many([_train_g(p, x, None, None) for p, x in zip(plans, xs)])
    params = [q for p in plans for q in p.params]
    return list(_PrepassFn.apply(plans, tuple(len(p.params) for p in plans), *xs, *params))


def apply(owner, slot, res_ops, dw_ops, cin, cout, x, addend=None):
    """Run the unit `owner`'s branches (res_ops, dw_ops) on x through the fused path; `slot` names the attribute that caches its plan."""
    p = plan_for(owner, slot, res_ops, dw_ops, cin, cout, ops.conform(x))
    if not torch.is_grad_enabled():
        fn = forward if p.branches[0]['bn1'].training else forward_eval
        return fn(p, ops.conform(x), None if addend is None else ops.conform(addend))
    return _UnitFn.apply(x, addend, p, *p.params)
