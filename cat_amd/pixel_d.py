"""The fused path of discriminators.PixelDiscriminator (csrc/pixel_d.hip; reference models/modules/discriminators.py:82-126): the whole 1x1
network as cat_pixeld_fwd1 -> cat_tnorm_finalize2 -> cat_pixeld_fwd3, and its backward as cat_pixeld_bwd1 -> cat_pixeld_bwd2.  Only the
pre-norm tensor z [M][2 ndf] is written and kept; h1 is recomputed, the normalised / activated tensor never exists.

applicable() decides per call and never raises; everything it declines runs `net` layer by layer on the general kernels, and so does
everything when CAT_PIXELD=0 (import-time A/B switch, also settable through `pixel_d.ENABLED`)."""
import ctypes as C
import os
from types import SimpleNamespace

import torch
from torch import nn

from . import _lib as L
from . import nn as cnn
from . import ops
from . import optim

ENABLED = os.environ.get('CAT_PIXELD', '1') != '0'      # A/B switch: '0' = general kernels only
MAX_NDF = 128


def _layers(module):
    net = getattr(module, 'net', None)
    if not isinstance(net, cnn.FusedSequential) or len(net) != 6:
        return None
    c1, a1, c2, norm, a2, c3 = list(net)
    if not all(type(c) is cnn.Conv2d for c in (c1, c2, c3)) or not (isinstance(a1, nn.LeakyReLU) and isinstance(a2, nn.LeakyReLU)):
        return None
    return c1, a1, c2, norm, a2, c3


def applicable(module, x):
    """True iff this call can take the fused kernels: BatchNorm2d (the replica-local SynchronizedBatchNorm2d included) or InstanceNorm2d on
    batch / instance statistics, ndf % 16 == 0 and ndf <= 128, a CUDA fp32 input of at most 8 channels, no forward hooks, no spectral norm."""
    try:
        if not ENABLED or not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
            return False
        layers = _layers(module)
        if layers is None:
            return False
        c1, a1, c2, norm, a2, c3 = layers
        if cnn._hooked(module.net, *layers):
            return False
        for c in (c1, c2, c3):
            if 'weight_orig' in c._parameters or c.kernel_size != (1, 1) or c.stride != (1, 1) or c.padding != (0, 0) or c.groups != 1 or \
                    c.dilation != (1, 1) or not c.weight.is_cuda or c.weight.dtype != torch.float32:
                return False
        ndf = c1.out_channels
        if ndf % 16 or ndf > MAX_NDF or c2.in_channels != ndf or c2.out_channels != 2 * ndf or c3.in_channels != 2 * ndf or c3.out_channels != 1:
            return False
        if c1.in_channels > 8 or x.shape[1] != c1.in_channels or c1.bias is None or x.shape[0] * x.shape[2] * x.shape[3] >= (1 << 29):
            return False
        if c1.in_channels == 1:      # never re-housed (nn._to_channels_last_): the kernels take its row stride as it is, if it has one
            wcs = ops.weight_wcs(c1.weight)
            if wcs is None or not 1 <= wcs <= 8:
                return False
        if isinstance(norm, cnn.InstanceNorm2d):
            if norm.track_running_stats:      # running averages of instance statistics: the general path
                return False
        elif isinstance(norm, cnn.BatchNorm2d):
            if cnn._exchanges(norm) or not (norm.training or not norm.track_running_stats):
                return False
            if norm.training and norm.track_running_stats and norm.momentum is None:
                return False
            if norm.virtual_replicas > 1:      # statistics per shard of the batch: layer by layer (the kernels' tables are per batch or per sample)
                return False
        else:
            return False
        return norm.num_features == 2 * ndf
    except Exception:
        return False


def geometry(n, hw, c0, xcs, ndf, groups, docs=4, slope1=0.2, slope2=0.2, w1cs=None):
    """w1cs: floats per row of the first conv's weight as it is stored (default: the padded channels-last row, round_up(c0, 4); a 1-channel
    weight stays dense, row stride 1)."""
    return L.PixelDGeom(n, hw, c0, xcs, ndf, 2 * ndf, ops.cs_for(c0) if w1cs is None else w1cs, groups, docs, slope1, slope2)


def plan(g):
    """The launch plan of a geometry (cat_pixeld_plan): statistics entries, persistent grids, LDS and workspace sizes."""
    p = L.PixelDPlan()
    L.call('cat_pixeld_plan', C.byref(g), C.byref(p))
    return p


def forward(module, x):
    c1, a1, c2, norm, a2, c3 = _layers(module)
    for c in (c1, c2, c3):
        cnn._to_channels_last_(c)
    inst = isinstance(norm, cnn.InstanceNorm2d)
    track = (not inst) and norm.training and norm.track_running_stats
    cfg = SimpleNamespace(inst=inst, eps=float(norm.eps), momentum=float(norm.momentum if norm.momentum is not None else 0.0),
                          rm=norm.running_mean if track else None, rv=norm.running_var if track else None,
                          nbt=norm.num_batches_tracked if track and not isinstance(norm, cnn.SynchronizedBatchNorm2d) else None,
                          slope1=float(a1.negative_slope), slope2=float(a2.negative_slope))
    return PixelDFn.apply(x, c1.weight, c1.bias, c2.weight, c2.bias, norm.weight, norm.bias, c3.weight, c3.bias, cfg)


def _fresh_like(p):
    if p.dim() == 4 and p.shape[1] > 1:
        return ops.padded_weight_like(p.shape, p.device)
    return torch.empty(p.shape, device=p.device, dtype=p.dtype)


class PixelDFn(torch.autograd.Function):
    """x -> the 1-channel prediction.  Saved for backward: x, z and the norm's [groups][2 ndf] rows -- nothing else of size M."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, w3, b3, cfg):
        ops._require_cuda(x)
        x = ops.conform(x)
        n, c0, h, w = x.shape
        ndf = w1.shape[0]
        c2 = 2 * ndf
        w1c, w1cs = ops.weight_cl(w1)
        w2c, w2cs = ops.weight_cl(w2)
        w3c, _ = ops.weight_cl(w3)
        if not c0 <= w1cs <= 8 or w2cs != ndf:
            raise RuntimeError('pixel discriminator: conv weights are not in the channels-last layout')
        groups = n if cfg.inst else 1
        g = geometry(n, h * w, c0, ops.act_cs(x), ndf, groups, 4, cfg.slope1, cfg.slope2, w1cs)
        pl = plan(g)
        dev, st = x.device, ops._stream()
        z = torch.empty((n * h * w, c2), device=dev, dtype=torch.float32)
        table = torch.empty(pl.table_floats, device=dev, dtype=torch.float32)
        L.call('cat_pixeld_fwd1', C.byref(g), ops._p(x), ops._p(w1c), ops._p(b1), ops._p(w2c), ops._p(b2), ops._p(z), ops._p(table), st)
        mean = torch.empty((groups, c2), device=dev, dtype=torch.float32)
        rstd = torch.empty((groups, c2), device=dev, dtype=torch.float32)
        tiles = dict(table=table, plan=SimpleNamespace(th=1, tw=pl.tile_px), scs=c2, lat=(1, h * w), ncls=1)
        scale, shift = ops.norm_from_tiles(tiles, n, c2, groups, gamma, beta, cfg.rm, cfg.rv, cfg.nbt, cfg.eps, cfg.momentum, mean, rstd)
        out = ops.empty_act(n, 1, h, w, dev)
        L.call('cat_pixeld_fwd3', C.byref(g), ops._p(z), ops._p(scale), ops._p(shift), ops._p(w3c), ops._p(b3), ops._p(out), st)
        ctx.geom = (n, h * w, c0, ops.act_cs(x), ndf, groups, cfg.slope1, cfg.slope2, w1cs)
        ctx.params = (w1, b1, w2, b2, gamma, beta, w3, b3)
        ctx.save_for_backward(x, z, scale, shift, mean, rstd, w1c, b1, w2c, w3c)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, z, scale, shift, mean, rstd, w1c, b1, w2c, w3c = ctx.saved_tensors
        n, hw, c0, xcs, ndf, groups, slope1, slope2, w1cs = ctx.geom
        dout = ops.conform(dout)
        g = geometry(n, hw, c0, xcs, ndf, groups, ops.act_cs(dout), slope1, slope2, w1cs)
        pl = plan(g)
        dev, st = x.device, ops._stream()
        needs = ctx.needs_input_grad
        wanted = [p for p, need in zip(ctx.params, needs[1:9]) if p is not None and need]
        want_dx = needs[0]
        dst, acc = {}, 0
        if wanted:
            sink = optim.claim(wanted, 'pixel discriminator backward')
            if sink is not None:
                views, acc = sink
                dst = {id(p): v for p, v in zip(wanted, views)}
            else:
                dst = {id(p): _fresh_like(p) for p in wanted}
            for p in ctx.params[:3]:      # the weight-gradient kernel always produces net.0.weight, net.0.bias and net.2.weight
                if p is not None and id(p) not in dst:
                    dst[id(p)] = _fresh_like(p)
        w1, b1p, w2, b2, gamma, beta, w3, b3 = ctx.params
        if wanted and ops._grad_wcs(dst[id(w1)]) != w1cs:
            raise RuntimeError('pixel discriminator: the gradient of net.0.weight is not laid out like the weight')
        d = lambda p: None if p is None else ops._p(dst.get(id(p)))
        coef = torch.empty((groups, 7, 2 * ndf), device=dev, dtype=torch.float32)
        ws = ops.workspace(4 * max(pl.ws1_floats, pl.ws2_floats), dev)
        L.call('cat_pixeld_bwd1', C.byref(g), ops._p(z), ops._p(dout), ops._p(scale), ops._p(shift), ops._p(mean), ops._p(rstd), ops._p(w3c),
               ops._p(coef), d(w3), d(b3), d(gamma), d(beta), acc, ops._p(ws), st)
        dx = None
        if want_dx or wanted:
            if want_dx:
                dx = ops.empty_act(n, c0, x.shape[2], x.shape[3], dev, xcs)
            L.call('cat_pixeld_bwd2', C.byref(g), ops._p(x), ops._p(z), ops._p(dout), ops._p(coef), ops._p(w1c), ops._p(b1), ops._p(w2c),
                   ops._p(dx), 1 if wanted else 0, d(w1), d(b1p), d(w2), d(b2), acc, ops._p(ws), st)
        grads = []
        for p, need in zip(ctx.params, needs[1:9]):
            if p is None or not need:
                grads.append(None)
            elif optim.owned(p) and dst[id(p)] is p._cat_grad_view:
                grads.append(None)      # written (or accumulated) in place
            else:
                grads.append(optim.deliver(p, dst[id(p)]))
        return (dx, *grads, None)
