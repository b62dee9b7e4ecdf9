"""Fused training-mode path of InvertedResidualChannels (reference models/modules/inception_modules.py:124-180, 230-236):

    x + pw_bn( sum_k conv2_k(relu(norm(conv1_k(x)))) + sum_k pw2_k(relu(norm(dw_k(relu(norm(pw1_k(x))))))) )

with train-mode BatchNorm2d / InstanceNorm2d in every position.  The general path launches ~55 kernels per block (12 convs, 10 norms
x 3, add_n, ...), most of them a few microseconds of HBM-bound work between dependent launches.  Here a block is 9 launches:

    stage 1   one LDS-tile conv launch per first-conv kernel size (the 1x1 convs of all branches as ONE N-concatenated GEMM) writing
              channel slices of one pre-norm buffer Z1 and the per-tile statistics of every branch           (cat_tconv_fwd + stats)
              -- or ONE launch for all sizes where fused_unit.stage1 has a kernel for the plan's widths (cat_tstage1_fwd; the full-width
              blocks of CAT_FUSED_WIDE: cat_tstage1ws_fwd at kernel sizes 1 3 5, cat_tstage1ws7_fwd at 3 5 7)
    finalize  scale / shift of all stage-1 norms + their running statistics                                   (cat_tnorm_finalize)
    dw        all depthwise convs as one launch; normalise + ReLU of stage 1 applied while staging            (cat_dwm_fwd; cat_dwm7_fwd
              when a depthwise branch is 7 x 7: kernel sizes from {1, 3, 5, 7}, CAT_FUSED_K7)
    finalize
    stage 2   the branch sum: six second convs K-concatenated into one launch, normalise + ReLU applied while staging, output
              written once, statistics for pw_bn                                                              (cat_tconv_fwd)
    finalize, out = x + T * scale + shift                                                                     (cat_affine_res_fwd)

Filter streams, concatenated gamma / beta / bias vectors and the depthwise filter frame are refreshed by ONE table-driven launch per
block and optimizer step (cat_prep_run).  The backward pass re-materialises the two hidden activations (one pass each) and then runs
the branch-wise weight-gradient kernels on channel slices; the six first-conv input gradients are one K-concatenated launch.
The layout, the operand preparation and the stage sequence, forward and backward, are the GauGAN generator's six-branch units' too and
are defined once in cat_amd/fused_unit.py; here: when the path applies, the block's plan (reflect padding, InstanceNorm, the one-stream
weight-gradient batch), the stage-2 launch with the closing pw_bn and the residual, and pw_bn's backward in front of the shared one.
Same arithmetic as the general path (same conv accumulation order per output, statistics merged pairwise instead of sequentially):
results agree to ~1e-6 relative; tests/test_fused_block_gpu.py pins both against the CPU oracle."""
import os
import weakref

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
# Blocks whose depthwise branches sum to more than CAT_DWM_MAXQ_BWD channel quads (the full-width teachers: 3 x 11) take this path with the
# depthwise stage as branch-aligned launches of at most that many quads (fused_unit.dw_launches) with CAT_FUSED_WIDE=1 / set_wide(True).
# Off by default (such blocks run layer by layer, as they always did): the graphed CycleGAN teacher step at batch 4 measured 134.1 ms on
# this path against 126.1 ms layer by layer; launched eagerly it is 146.8 against 207.5 ms (profiles/wide_block_bench.txt)
_WIDE = os.environ.get('CAT_FUSED_WIDE', '0') != '0'
# Blocks with a 7 x 7 branch (the reference's parser default --kernel_sizes 3 5 7) take this path unless CAT_FUSED_K7=0 / set_k7(False): their
# 7 x 7 convs on the wide-patch LDS-tile kernels (csrc/conv_pk7.hip), their depthwise stage on the 7 x 7 frame (cat_dwm7_fwd / cat_dwm7_bwd).
# With it off such blocks run layer by layer, as they always did.  On by default: the graphed pix2pix distillation step with kernel sizes
# 3 5 7 at batch 16 measured 64.05 ms on this path against 71.58 ms layer by layer, spread 0.17 ms (profiles/k7_block_bench.txt)
_K7 = os.environ.get('CAT_FUSED_K7', '1') != '0'
# Per-block opt-in to this path in eval() mode: cat_amd.infer.StudentRunner registers the blocks of the network it owns.  An InstanceNorm2d
# without running statistics computes the same function in eval() as in train(), so forward(block, x, save=None) is the block's eval
# forward as it stands: per-sample statistics collected and finalized, no running statistics to touch (fused_unit.slices passes none).
# A block that is not registered takes, in eval mode, the path it always took.  The registry holds the block OBJECTS weakly and nothing is
# written on the module: a copy.deepcopy of an owned network (shrink_model, load_pretrained_student copy the teacher) is not owned.
# The value is the owner's LDS-tile threshold for this block (fewest 8 x 16 output tiles; None: ops' process-wide one).
_EVAL_OWNED = weakref.WeakKeyDictionary()


def own_eval(block, min_tiles=None):
    _EVAL_OWNED[block] = (None if min_tiles is None else int(min_tiles),)


def disown_eval(block):
    _EVAL_OWNED.pop(block, None)


def eval_owned(block):
    return block in _EVAL_OWNED


def set_enabled(on):
    global _ENABLED
    _ENABLED = bool(on)


def set_k7(on):
    global _K7
    old, _K7 = _K7, bool(on)
    return old


def set_wide(on):
    global _WIDE
    old, _WIDE = _WIDE, bool(on)
    return old


def _dw_quads(block):
    return [U.cs4(op[0][0].out_channels) // 4 for op in block.dw_ops]


def _dropout(block):
    """-> (p, {j of the branches whose Dropout is active}) -- Dropout j = res branches first, then dw branches -- or None when the active
    Dropouts of the block disagree on p (general path).  p == 0: no Dropout is active (eval mode or rate 0) and nothing is launched."""
    mods = [op[2] for op in block.res_ops] + [op[3] for op in block.dw_ops]
    act = {j: float(m.p) for j, m in enumerate(mods) if isinstance(m, cnn.Dropout) and m.training and m.p != 0}
    if len(set(act.values())) > 1:
        return None
    return (next(iter(act.values())) if act else 0.0), frozenset(act)


def applicable(block, x):
    if not _ENABLED or not x.is_cuda or block.padding_type not in ('reflect', 'zero'):
        return False
    owner = None if block.training else _EVAL_OWNED.get(block)
    if not block.training and (owner is None or torch.is_grad_enabled()):
        return False
    if _dropout(block) is None:
        return False
    if len(block.res_ops) + len(block.dw_ops) == 0 or not ops.is_act(x):
        return False
    n, c, h, w = x.shape
    if not ops.tconv_applicable(n, h, w, c, 3, 3, 1, 1, min_tiles=owner[0] if owner is not None else None):
        return False
    norms = [op[1][1] for op in block.res_ops] + [op[0][1] for op in block.dw_ops] + [op[2][1] for op in block.dw_ops] + [block.pw_bn]
    kind = type(norms[0])
    if kind not in (cnn.BatchNorm2d, cnn.InstanceNorm2d, cnn.SynchronizedBatchNorm2d) or any(type(m) is not kind for m in norms):
        return False
    if kind is cnn.SynchronizedBatchNorm2d:      # --norm syncbatch: replica-local layers are BatchNorm2d that never count batches (fused_unit.slices)
        if any(not m.replica_local for m in norms):
            return False
        kind = cnn.BatchNorm2d
    if kind is cnn.BatchNorm2d and any(m.momentum is None or not m.track_running_stats for m in norms):
        return False
    if kind is cnn.BatchNorm2d and any(m.virtual_replicas != norms[0].virtual_replicas for m in norms):
        return False      # one shard count per block (networks.set_virtual_replicas stamps a whole network): otherwise layer by layer
    if kind is cnn.InstanceNorm2d and any(m.track_running_stats for m in norms):
        return False
    if not block.training and (kind is not cnn.InstanceNorm2d or any(m.training for m in norms) or _dropout(block)[0] != 0):
        return False      # eval mode: only norms that keep no statistics compute train()'s function (BatchNorm: cat_amd/frozen.py)
    first_act = block.res_ops[0][1][2] if len(block.res_ops) else block.dw_ops[0][0][2]
    if cnn._act_code(first_act)[0] not in (L.ACT_RELU, L.ACT_LRELU):     # the staging paths apply ReLU / LeakyReLU only (nn.ReLU6: general path)
        return False
    ks = [op[1][0].kernel_size[0] for op in block.res_ops] + [op[2][0].kernel_size[0] for op in block.dw_ops]
    if any(k not in ((1, 3, 5, 7) if _K7 else (1, 3, 5)) for k in ks):
        return False
    if len(block.res_ops) + len(block.dw_ops) > L.TCONV_MAXSEG:
        return False
    quads = _dw_quads(block)
    if sum(quads) > L.DWM_MAXQ_BWD and (not _WIDE or U.dw_launches(quads, L.DWM_MAXQ_BWD) is None):
        return False      # more quads than one depthwise launch takes: several branch-aligned launches, unless one branch alone is too wide
    return not U.has_hooks(block.children())


class _Plan(U.Plan):
    """The layout of one block (C_in = C_out = C) + what its closing pw_bn, padding and norm kind add."""
    what = 'fused block'

    def __init__(self, block, dev, dw_maxq=L.DWM_MAXQ_BWD):
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
        super().__init__(res, dws, block.input_dim, block.input_dim, dev, list(block.parameters()), dw_maxq)
        self.C, self.cs = self.Cin, self.csi

    def live_shards(self):
        """virtual replicas as stamped on the closing norm NOW (networks.set_virtual_replicas may change it between steps).  forward() copies
        it into self.shards, which every stage reads; the backward pass restores the value ITS forward ran with (the saved tables have that
        shape), whatever was stamped or run in between."""
        return 1 if self.instance else int(self.block.pw_bn.virtual_replicas)

    wgrad_batch = True      # one stream (the inception distillers' default): the weight-gradient partial sums are reduced by ONE launch

    def _merges_dw_dgrad(self):
        return len(self.dws) > 1

    def prepare(self, backward=False):
        """Refresh the derived operands if a weight changed since the last refresh (once per optimizer step)."""
        group = getattr(self, 'group', None)
        if backward and group is not None:
            prepare_many(group, backward=True)      # the first backward of the step refreshes every block of the generator in ONE launch
        self._prepare_own(backward)


def plan_for(block, x, dw_maxq=L.DWM_MAXQ_BWD):
    """The block's plan.  dw_maxq: the widest depthwise launch the caller's kernels take -- the backward kernel's for a plan that trains (also
    its forward), CAT_DWM_MAXQ for the forward-only frozen teacher (cat_amd/frozen_in.py); a plan built for another grouping is rebuilt."""
    p = getattr(block, U.PLAN, None)
    # the plan holds Parameter OBJECTS (gradient targets are keyed by identity): a parameter replaced by one of the same shape
    # (module.weight = nn.Parameter(...), weight transfer) invalidates it like a shape change does
    if p is None or p.dev != x.device or p.shapes != tuple(tuple(q.shape) for q in block.parameters()) or \
            p.ids != tuple(id(q) for q in block.parameters()) or \
            (p.dw_maxq != dw_maxq and p.dw_spans != tuple(U.dw_launches(_dw_quads(block), dw_maxq) or ())):
        p = _Plan(block, x.device, dw_maxq)
        setattr(block, U.PLAN, p)
    return p


def _run(gen):
    """Drive a generator of the shared pipeline to its result.  The block always passes sync=None -- its norms keep per-replica statistics,
    also under a data-parallel reducer -- so no stage may ask for a statistics exchange over ranks."""
    try:
        next(gen)
    except StopIteration as e:
        return e.value
    raise RuntimeError('fused block: a stage asked for a statistics exchange over ranks')


def forward(block, x, save=None):
    """The block's forward on the fused path.  `save`: dict that receives what the backward pass needs (None under no_grad)."""
    p = plan_for(block, x)
    p.prepare()
    p.shards = p.live_shards()
    n, c, h, w = x.shape
    dev = x.device
    pdrop, djs = _dropout(block)
    ticket = rng.draw(dev) if pdrop else None       # one draw per block forward, as on the general path
    z1, st1, zd, std, segs = _run(U.forward_g(p, x, drop=(pdrop, djs, ticket) if ticket is not None else None))
    # ---- stage 2: the branch sum + the statistics of the closing pw_bn
    t = ops.empty_act(n, c, h, w, dev)
    partp = torch.empty((n * ((h + 7) // 8) * ((w + 15) // 16), 2, p.cs), device=dev, dtype=torch.float32)
    tconv.run(segs, p.pack2, p.bias2 if p.has_bias2 else None, t, c, n, h, w, h, w, stats=partp, scs=p.cs)
    pw = block.pw_bn
    stp = _run(U.finalize_g(p, partp, p.cs, n, h, w, pw.weight, pw.bias, [(0, c, pw)], sync=None, mstride=c))
    # ---- out = x + pw_bn(T)
    y = ops.empty_act(n, c, h, w, dev)
    G = n if p.per_sample else 1
    L.call('cat_affine_res_fwd', ops._p(t), p.cs, ops._p(stp[0][0]), ops._p(stp[0][1]), p.cs if p.per_sample else 0, ops._p(x), ops.act_cs(x), ops._p(y), p.cs,
           G, (n // G) * h * w, p.cs, L.ACT_NONE, 0.0, ops._stream())
    if save is not None:
        save.update(plan=p, z1=z1, zd=zd, t=t, st1=st1, std=std, stp=stp, drop=(pdrop, djs, ticket))
    return y


class _BlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, block, *params):
        x = ops.conform(x)
        save = {}
        y = forward(block, x, save)
        ctx.block, ctx.plan = block, save['plan']
        ctx.shards = ctx.plan.shards
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
        dy = ops.conform(dy)
        p.prepare(backward=True)
        p.shards = ctx.shards
        n, c, h, w = x.shape
        # ---- the closing pw_bn: dT from dy (the skip connection's share of dy is added by the pipeline's last launch)
        pw = block.pw_bn
        if ops.act_cs(dy) != p.cs:
            raise RuntimeError('fused block backward: gradient pixel stride differs from the activation')
        own = {}
        if pw.weight is not None:
            sink = optim.claim([pw.weight, pw.bias], 'fused block backward')       # FusedAdam-owned: written (or accumulated) in place
            (dgp, dbp), acc = sink or ((torch.empty_like(pw.weight), torch.empty_like(pw.bias)), 0)
            dt = _run(U.norm_bwd_g(p, n, h * w, c, p.cs, t, dy, pw.weight, pw.bias, mrp, L.ACT_NONE, 0.0, dgp, dbp, acc))
            if sink is None:
                own[id(pw.weight)], own[id(pw.bias)] = optim.deliver(pw.weight, dgp), optim.deliver(pw.bias, dbp)
        else:
            dt = _run(U.norm_bwd_g(p, n, h * w, c, p.cs, t, dy, None, None, mrp, L.ACT_NONE, 0.0, None, None))
        # ---- the branches: the shared backward pipeline from dT
        dx, grads = _run(U.backward_g(p, dt, x, z1, ss1, mr1, zd, ssd, mrd, need_dx=ctx.needs_input_grad[0], skip_grad=dy,
                                      drop=(ctx.pdrop, ctx.djs, saved[-1]) if ctx.pdrop else None))
        grads.update(own)
        return (dx, None) + tuple(grads.get(id(q)) for q in block.parameters())


def apply(block, x):
    if not torch.is_grad_enabled():
        return forward(block, ops.conform(x))
    return _BlockFn.apply(x, block, *block.parameters())
