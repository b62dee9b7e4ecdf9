"""GPU: every cached derived operand of the hot path follows every way the weights really change.

The kernels update weights, Adam state and BatchNorm running statistics through raw pointers (torch's `_version` never moves), while the forward
and backward passes run on operands DERIVED from them and cached on the host: MFMA-order filter packs, transposed filters, bf16 planes, conv+BN
folds, the prep tables of the fused units ("Derived operands and their keys").  A stale entry raises nothing -- the next launch
silently computes with the weights of an earlier step.  This module is a table: a ROW is a derived operand with the smallest layer that takes
its path, a COLUMN is a way weights change in the product, and every applicable cell runs one protocol:

    1  build the layer with weights W0 (oracle.detfill), run it (forward, and backward where the operand is a backward operand): cache populated
    2  change the weights to W1 through the column's real mechanism, read W1 back to the host
    3  run the SAME objects again (warm)
    4  (a) warm == cold bit for bit, cold = a freshly built twin that received W1 by copy_ (load_state_dict) and never ran before
       (b) warm matches an fp64 host evaluation with W1 at the bar the kernel's own parity test holds: 1e-4 of the output's largest magnitude
           for the conv paths (tests/test_kernels_gpu.py TOL), 2e-5 of sum |terms| for the split-bf16 tiles (tests/test_split_gpu.py)
       (c) not vacuous: the fp64 results for W0 and W1 differ by more than 100 x that bar (upper quartile over the compared elements)
       (d) still a cache: one more call with nothing changed launches no derivation kernel and returns the same derived tensor objects

Columns: M1 eager FusedAdam.step after a real backward (raw pointers, epoch bump) | M2 load_state_dict (copy_, version bump) | M3 storage
move: first use BEFORE the optimizer flattens, zero_grad re-houses the parameters, then M1 | M3b `p.data = new_tensor` | M4 captured-step
replay through cat_amd.graph.GraphedStep | M5 running statistics moved by train-mode forwards of the library's own norm path with NO optimizer
step before the next eval forward (a net without an optimizer, and a FusedAdam-owned net between two steps) | M6 a second FusedAdam over the
same parameters (re-flattens, new gradient views)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import detfill

pytestmark = pytest.mark.gpu

TOL = 1e-4            # tests/test_kernels_gpu.py
SPLIT_TOL = 2e-5      # tests/test_split_gpu.py, of sum |terms|
SEPARATION = 100.0    # (c)
LR = 0.5              # Adam's first step moves every weight with a non-zero gradient by ~lr

# kernels that DERIVE an operand from weights / statistics: none of them may run in step (d)
DERIVE = ('cat_tconv_pack', 'cat_conv2d_weight_transpose', 'cat_prep_run', 'cat_bn_fold', 'cat_qconv_pack')


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


@pytest.fixture()
def small_planes():
    """The LDS-tile kernels (and the fused block built on them) and the wide-tile sum on planes of a few tiles, as the existing tests do."""
    from cat_amd import ksum, ops
    old_t, old_k = ops.set_tconv_min_tiles(1), ksum.set_min_workgroups(1)
    yield
    ops.set_tconv_min_tiles(old_t)
    ksum.set_min_workgroups(old_k)


class Launches(list):
    """Entry-point names in call order; `tables`: the job table (device address) of every cat_prep_run among them."""

    def __init__(self):
        super().__init__()
        self.tables = []

    def prepared(self, net):
        """The cat_prep_run launches that PREPARED operands: all but the fused units' gradient scatter into the optimizer's buffers, which
        goes through the same table-driven kernel (fused_unit.scatter_param_grads) once per unit and backward pass."""
        plans = [getattr(m, '_cat_fused_plan', None) for m in net.modules()]
        scatter = {p.scatter_jobs[0].data_ptr() for p in plans if p is not None and p.scatter_jobs is not None}
        return [t for t in self.tables if t not in scatter]


@contextlib.contextmanager
def launches():
    """The library entry points called inside the block (cat_amd._lib.call is the one door every launch goes through)."""
    from cat_amd import _lib
    names, real = Launches(), _lib.call

    def call(name, *args):
        names.append(name)
        if name == 'cat_prep_run':
            names.tables.append(args[0].value)
        return real(name, *args)
    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = real


def nhwc(t, dev):
    from cat_amd import ops
    return ops.to_nhwc(t.to(dev))


def host(t):
    return t.detach().cpu().double().contiguous()


def state_of(net):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone().contiguous() for k, v in net.state_dict().items()}


def kernel_layout(t, dev):
    """A NEW device tensor holding `t` in the storage the kernels read (conv weights: zero-padded channels_last)."""
    from cat_amd import ops
    if t.dim() == 4 and t.shape[1] > 1:
        new = ops.padded_weight_like(tuple(t.shape), dev)
        new.copy_(t.to(dev))
        return new
    return t.to(dev).contiguous().clone()


# ====================================================================================================================== rows
class Row:
    """One derived operand + the smallest layer on its path.  `train`: the warm / cold pass is forward + backward in train mode (the operand
    serves a training pass); otherwise an eval-mode no-grad forward (a fold), and `train_pass` is the train-mode forward + backward that gives
    Adam a real gradient in between."""
    train = True
    seed = 100
    lr = LR             # of the Adam columns
    uses = ()           # entry points the pass must go through (the path the row is about)
    derives = ()        # derivation kernels the warm pass must launch (the operand was re-derived, on the device)

    def fill(self, net, draw):
        net.load_state_dict(detfill.fill_state_dict(net.state_dict(), self.seed + 1000 * draw))

    def build(self, dev, draw=0):
        net = self.make()
        self.fill(net, draw)
        net = net.to(dev)
        return net.train() if self.train else net.eval()

    def state(self, draw):
        net = self.make()
        self.fill(net, draw)
        return {k: v.clone() for k, v in net.state_dict().items()}

    # -- device passes
    def grads_of(self, net, xg):
        out = {'dx': host(xg.grad)}
        for k, p in net.named_parameters():
            out['d.' + k] = host(p.grad)
        return out

    def train_pass(self, net, dev):
        was = net.training
        net.train()
        xg = nhwc(self.x, dev).detach().requires_grad_(True)
        y = self.forward(net, xg)
        y.backward(nhwc(self.gy, dev))
        torch.cuda.synchronize()
        out = dict(y=host(y), **self.grads_of(net, xg))
        net.train(was)
        return out

    def stats_pass(self, net, dev, times=8):
        """Forward-only train-mode passes: the norm kernels move the running statistics, nothing else changes."""
        net.train()
        with torch.no_grad():
            for _ in range(times):
                self.forward(net, nhwc(self.xs, dev))
        net.eval()
        torch.cuda.synchronize()

    def run(self, net, dev):
        if self.train:
            return self.train_pass(net, dev)
        with torch.no_grad():
            y = self.forward(net, nhwc(self.x, dev))
        torch.cuda.synchronize()
        return {'y': host(y)}

    def forward(self, net, x):
        return net(x)

    # -- fp64 on the host
    def ref(self, sd):
        twin = self.twin().double()
        twin.load_state_dict({k: v.double() for k, v in sd.items()})
        twin.train(self.train)
        if not self.train:
            with torch.no_grad():
                return {'y': twin(self.x.double())}, None
        xr = self.x.double().requires_grad_(True)
        y = twin(xr)
        y.backward(self.gy.double())
        out = {'y': y.detach(), 'dx': xr.grad}
        for k, p in twin.named_parameters():
            out['d.' + k] = p.grad
        return out, None

    def derived(self, net):
        return []

    def fold_keys(self, net):
        """The optim.weights_key values the row's folds are cached under right now (rows whose operand is a fold)."""
        return None


class Padded(nn.Module):
    """pad -> conv the way the generators write it (the pad is folded into the conv's gather)."""

    def __init__(self, pad, conv):
        super().__init__()
        self.pad, self.conv = pad, conv

    def forward(self, x):
        return self.conv(self.pad(x))


class ConvRow(Row):
    def __init__(self, name, cin, cout, k, stride, pad, shape, reflect=False, bias=True, uses=(), derives=(), seed=100):
        self.name, self.cin, self.cout, self.k, self.stride, self.pad, self.reflect, self.bias = name, cin, cout, k, stride, pad, reflect, bias
        self.uses, self.derives, self.seed = uses, derives, seed
        n, h, w = shape
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        self.x = detfill.normal((n, cin, h, w), seed + 1)
        self.gy = detfill.normal((n, cout, ho, wo), seed + 2)

    def make(self):
        from cat_amd import nn as cnn
        if self.reflect:
            return Padded(cnn.ReflectionPad2d(self.pad), cnn.Conv2d(self.cin, self.cout, self.k, stride=self.stride, padding=0, bias=self.bias))
        return Padded(cnn.Identity(), cnn.Conv2d(self.cin, self.cout, self.k, stride=self.stride, padding=self.pad, bias=self.bias))

    def twin(self):
        if self.reflect:
            return Padded(nn.ReflectionPad2d(self.pad), nn.Conv2d(self.cin, self.cout, self.k, stride=self.stride, padding=0, bias=self.bias))
        return Padded(nn.Identity(), nn.Conv2d(self.cin, self.cout, self.k, stride=self.stride, padding=self.pad, bias=self.bias))

    def derived(self, net):
        from cat_amd import derived, ops
        w = net.conv.weight
        out = [ent.value for ent in (derived.peek(w, ops.PK) or {}).values()]
        out += [derived.peek(w, a).value for a in (ops.WT, ops.WTP) if derived.peek(w, a) is not None]
        return out


class SplitRow(ConvRow):
    """The bf16 planes of the transposed filter (keyed through the transposed filter's key): the data gradient on the split-bf16 tile."""

    def ref(self, sd):
        out, _ = super().ref(sd)
        # what each sum is made of (tests/test_split_gpu.py): the same convolution over |x|, |w|, |gy|
        xa = self.x.double().abs().requires_grad_(True)
        wa = sd['conv.weight'].double().abs().requires_grad_(True)
        F.conv2d(xa, wa, None, self.stride, self.pad).backward(self.gy.double().abs())
        return out, {'dx': SPLIT_TOL * xa.grad, 'd.conv.weight': SPLIT_TOL * wa.grad}


class FoldRow(Row):
    """conv -> eval BatchNorm2d -> ReLU of a generator's down-sampling layer: one conv launch on the folded weights (nn._folded_eval_bn)."""
    train = False

    def __init__(self, name, seed=140):
        self.name, self.seed = name, seed
        self.x = detfill.normal((2, 8, 8, 8), seed + 1)
        self.xs = 2.0 * detfill.normal((2, 8, 8, 8), seed + 3) + 0.5
        self.gy = detfill.normal((2, 16, 4, 4), seed + 2)

    def make(self):
        from cat_amd import nn as cnn
        return cnn.FusedSequential(cnn.Conv2d(8, 16, 3, stride=2, padding=1, bias=True), cnn.BatchNorm2d(16), cnn.ReLU())

    def twin(self):
        return nn.Sequential(nn.Conv2d(8, 16, 3, stride=2, padding=1, bias=True), nn.BatchNorm2d(16), nn.ReLU())

    def derived(self, net):
        from cat_amd import nn as cnn
        with torch.no_grad():
            return list(cnn._folded_eval_bn(net[0], net[1], 0))

    def fold_keys(self, net):
        from cat_amd import derived, nn as cnn
        return [derived.peek(net[0], cnn.FOLD).key]


class TorchBlock(nn.Module):
    """InvertedResidualChannels out of stock torch.nn layers (the reference's own construction, inception_modules.py:124-180): same
    state_dict keys as the cat_amd module."""

    def __init__(self, c, res, dw, ks, reflect):
        super().__init__()
        pad = nn.ReflectionPad2d if reflect else nn.ZeroPad2d
        bn = lambda m: nn.BatchNorm2d(m, momentum=0.1, eps=1e-5)
        self.res_ops, self.dw_ops = nn.ModuleList(), nn.ModuleList()
        for m, k in zip(res, ks):
            if m:
                self.res_ops.append(nn.Sequential(pad((k - 1) // 2), nn.Sequential(nn.Conv2d(c, m, k, bias=False), bn(m), nn.ReLU()), nn.Dropout(0.0),
                                                  pad((k - 1) // 2), nn.Conv2d(m, c, k, bias=False)))
        for m, k in zip(dw, ks):
            if m:
                self.dw_ops.append(nn.Sequential(nn.Sequential(nn.Conv2d(c, m, 1, bias=False), bn(m), nn.ReLU()), pad((k - 1) // 2),
                                                 nn.Sequential(nn.Conv2d(m, m, k, groups=m, bias=False), bn(m), nn.ReLU()), nn.Dropout(0.0),
                                                 nn.Conv2d(m, c, 1, bias=False)))
        self.pw_bn = bn(c)

    def forward(self, x):
        return x + self.pw_bn(sum(op(x) for op in self.res_ops) + sum(op(x) for op in self.dw_ops))


def cat_block(c, res, dw, ks, reflect):
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    return InvertedResidualChannels(c, list(res), list(dw), 1, list(ks), list(ks), padding_type='reflect' if reflect else 'zero', use_bias=False,
                                    norm_layer=cnn.BatchNorm2d, norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))


class Chain(nn.Module):
    """Blocks in sequence; in train mode their operand preparation is merged the way InceptionGenerator.forward merges it."""

    def __init__(self, blocks, merged):
        super().__init__()
        self.blocks, self.merged = nn.ModuleList(blocks), merged

    def forward(self, x):
        if self.merged and self.training:
            from cat_amd import fused_block
            fused_block.prepare_many(list(self.blocks))
        for b in self.blocks:
            x = b(x)
        return x


class BlockRow(Row):
    def fill(self, net, draw):
        net.load_state_dict(detfill.fill_state_dict(net.state_dict(), self.seed + 1000 * draw, gamma_abs_normal=True))

    def make(self):
        return Chain([cat_block(self.c, self.res, self.dw, (1, 3, 5), True) for _ in range(self.nblocks)], True)

    def twin(self):
        return Chain([TorchBlock(self.c, self.res, self.dw, (1, 3, 5), True) for _ in range(self.nblocks)], False)

    def ref(self, sd):
        """Bars of tests/test_fused_block_gpu.py: 1e-4 forward, 2e-4 input gradient, 5e-4 per parameter gradient of max(its own largest
        magnitude, 1e-3 of the largest gradient) -- a gradient that is tiny next to the others is round-off in any implementation.
        Those bars, unchanged, are the bars of every column."""
        out, _ = super().ref(sd)
        if not self.train:
            return out, None
        top = max(float(v.abs().max()) for k, v in out.items() if k.startswith('d.'))
        bars = {k: 5e-4 * max(float(v.abs().max()), 1e-3 * top) for k, v in out.items() if k.startswith('d.')}
        bars['dx'] = 2e-4 * float(out['dx'].abs().max())
        return out, bars


class FrozenRow(BlockRow):
    """frozen._plan: one eval InvertedResidualChannels with BatchNorm at the teacher's branch widths (3 x 42 + 3 x 42 on 16 channels), the only
    widths whose first convs run as ONE launch on lazily packed filter streams (s1w); 16 output channels keep the tail on the LDS-tile launch
    with its lazily built tail_pack.  The fp64 reference is the general path's math (the block, layer by layer, in torch fp64)."""
    train, nblocks, c, res, dw, name, seed = False, 1, 16, (42, 42, 42), (42, 42, 42), 'R5 frozen._plan', 150
    uses = ('cat_tstage1w_fwd', 'cat_dwconv2d_multi_fwd', 'cat_tconv_fwd')
    derives = ('cat_tconv_pack',)      # the lazily packed streams are rebuilt with the plan

    def __init__(self):
        self.x = detfill.normal((2, 16, 8, 16), self.seed + 1)
        self.xs = 2.0 * detfill.normal((2, 16, 8, 16), self.seed + 3) + 0.5
        self.gy = detfill.normal((2, 16, 8, 16), self.seed + 2)

    def derived(self, net):
        from cat_amd import frozen
        p = frozen._plan(net.blocks[0])
        assert p['s1w'] is not None and p['s1w']['packs'] is not None and p['tail_pack'] is not None      # the lazily built operands exist
        return [p['w_a'], p['w_f'], p['b_f'], p['dwm']['frame'], p['tail_pack']] + list(p['s1w']['packs'])

    def fold_keys(self, net):
        from cat_amd import derived, frozen
        return [derived.peek(net.blocks[0], frozen.FROZEN).key]


class FusedRow(BlockRow):
    """The fused train-mode block's prep tables: `nblocks` blocks in sequence (two: both plans are stale after a step and the MERGED table
    runs; one: the single-stale branch, the plan's own table)."""
    c, res, dw, seed = 40, (7, 0, 9), (16, 5, 0), 170
    # The parity bars of tests/test_fused_block_gpu.py were set with weights of the scale detfill draws (N(0, 1 / fan_in): 0.16 for the
    # 1x1 convs on 40 channels, up to 0.45 for the narrow branches).  A first Adam step at lr 0.5 puts every weight +-0.5 from its draw,
    # several of those standard deviations out; the block's sums then cancel and single parameter gradients (a BatchNorm bias 100 x smaller
    # than the largest gradient) are round-off in fp32 whoever evaluates them.  0.1 moves every weight by a good part of its standard
    # deviation and keeps the step at the scale the bars were set for, so they hold UNCHANGED; (c) is asserted all the same.
    lr = 0.1
    uses =('cat_prep_run', 'cat_tnorm_finalize')
    derives = ('cat_prep_run',)

    def __init__(self, nblocks):
        self.nblocks, self.name = nblocks, 'R7 fused-unit prep tables x%d' % nblocks
        self.x = detfill.normal((2, 40, 8, 16), self.seed + 1)
        self.gy = detfill.normal((2, 40, 8, 16), self.seed + 2)

    def derived(self, net):
        plans = [b._cat_fused_plan for b in net.blocks]
        return [t for p in plans for t in (p.fwd_jobs[0], p.bwd_jobs[0], p.pack2, p.dpack1)]


class SpadeRow(Row):
    """fused_spade._eval_affine: one frozen (eval, no-grad) fused SPADE unit, the smallest (fin, fout) of
    tests/test_spade_gpu.py::test_fused_spade_units_frozen_match_general_path -- the main unit and its gamma|beta unit both fold their norms'
    running statistics into the consumers' staging (eval_ss).  fp64: the oracle's functional block (oracle/ref_spade_cpu.py) in float64."""
    train, name, seed = False, 'R6 fused_spade._eval_affine', 160
    uses = ('cat_tconv_fwd',)
    derives = ('cat_bn_fold',)
    folds_per_call = 1      # ops.spade_eval folds the param-free norm's statistics at EVERY call (nothing cached there)

    def __init__(self):
        n, c, h, w = 2, 24, 16, 24
        self.x = detfill.normal((n, c, h, w), self.seed + 1)
        self.xs = 2.0 * detfill.normal((n, c, h, w), self.seed + 3) + 0.5
        self.gy = detfill.normal((n, c, h, w), self.seed + 2)
        self.opt = None

    def options(self):
        if self.opt is None:
            import json
            from argparse import Namespace
            import helpers as H
            o = json.loads(str(H.load('spade_step.npz')['opt']))
            o.update(gpu_ids=[0], norm_G='spadesyncbatch3x3', channels=None)
            self.opt = Namespace(**o)
            n, _, h, w = self.x.shape
            self.seg = (detfill.normal((n, self.opt.semantic_nc, h // 4, w // 4), self.seed + 4) > 0.8).float().repeat_interleave(4, 2).repeat_interleave(4, 3)
        return self.opt

    def fill(self, net, draw):
        net.load_state_dict(detfill.fill_state_dict(net.state_dict(), self.seed + 1000 * draw, gamma_abs_normal=True))

    def make(self):
        from cat_amd.inception_modules import SPADEInvertedResidualChannels
        return SPADEInvertedResidualChannels(24, 24, self.options())

    def forward(self, net, x):
        return net(x, nhwc(self.seg, x.device))

    def ref(self, sd):
        from oracle import ref_spade_cpu as R
        self.options()
        with torch.no_grad():
            y = R.spade_inverted_residual_channels({'b.' + k: v.double().clone() for k, v in sd.items()}, 'b', self.x.double(), self.seg.double(), False, False)
        return {'y': y}, None

    def derived(self, net):
        from cat_amd import fused_spade
        plans = [net._cat_fused_main, net.spade._cat_fused_gb]
        return [t for p in plans for t in fused_spade._eval_affine(p)]

    def fold_keys(self, net):
        from cat_amd import derived, fused_spade
        return [derived.peek(p, fused_spade.EVAL_SS).key for p in (net._cat_fused_main, net.spade._cat_fused_gb)]


R1Z = ConvRow('R1 packed_filter zero pad', 12, 20, 3, 1, 1, (1, 8, 16), uses=('cat_tconv_fwd',), derives=('cat_tconv_pack',), seed=110)
R1R = ConvRow('R1 packed_filter reflect pad', 12, 20, 3, 1, 1, (1, 8, 16), reflect=True, uses=('cat_tconv_fwd',), derives=('cat_tconv_pack',), seed=115)
R2 = ConvRow('R2 transposed_filter', 100, 32, 1, 1, 0, (1, 9, 11), uses=('cat_conv2d_dgrad_t',), derives=('cat_conv2d_weight_transpose',), seed=120)
R3 = SplitRow('R3 split_transposed_filter', 128, 128, 4, 2, 1, (1, 8, 12), bias=False, uses=('cat_conv2d_dgrad_split',),
              derives=('cat_conv2d_weight_transpose',), seed=130)
R4 = FoldRow('R4 _folded_eval_bn')
R5 = FrozenRow()
R6 = SpadeRow()
R7A, R7B = FusedRow(2), FusedRow(1)


# ====================================================================================================================== the protocol
def clear_grads(net, opt):
    if opt is not None:
        opt.zero_grad()
    else:
        for p in net.parameters():
            p.grad = None


def adam(net, lr=LR):
    from cat_amd.optim import FusedAdam
    return FusedAdam(list(net.parameters()), lr=lr, betas=(0.5, 0.999))


def step_after_real_backward(row, net, opt, dev):
    clear_grads(net, opt)
    row.train_pass(net, dev)
    opt.step()


def mutate(col, row, net, dev):
    """Steps 1 and 2: populate the caches with W0, then change the weights the way `col` says.  -> (the optimizer that owns the net or None,
    the state the caches were last derived from where that is not the row's draw 0, else None, and for the M1 / M3 cells of a fold the
    optim.weights_key values it was cached under when populated)."""
    from cat_amd import optim
    opt = w0 = keys0 = None
    if col == 'M1':
        opt = adam(net, row.lr)
        opt.zero_grad()
        row.run(net, dev)
        keys0 = row.fold_keys(net)
        if row.train:
            opt.step()                                   # (the populating pass WAS the real backward)
        else:
            step_after_real_backward(row, net, opt, dev)
    elif col == 'M2':
        row.run(net, dev)
        net.load_state_dict(row.state(1))
    elif col == 'M3':
        row.run(net, dev)                                # first use BEFORE the optimizer flattens: caches keyed on the old storage
        keys0 = row.fold_keys(net)
        before = [p.data_ptr() for p in net.parameters()]
        assert not any(optim.owned(p) for p in net.parameters())
        opt = adam(net, row.lr)
        opt.zero_grad()                                  # re-houses every parameter in the flat buffer
        assert all(optim.owned(p) and p.data_ptr() != b for p, b in zip(net.parameters(), before))
        step_after_real_backward(row, net, opt, dev)
    elif col == 'M3b':
        row.run(net, dev)
        w1 = row.state(1)
        for k, p in net.named_parameters():
            p.data = kernel_layout(w1[k], dev)           # a new tensor behind the same Parameter: no version bump, new address
        for k, b in net.named_buffers():
            b.data = w1[k].to(dev)
    elif col in ('M5', 'M5owned'):
        assert not row.train
        if col == 'M5owned':
            opt = adam(net, row.lr)
            opt.zero_grad()
        # the net has been in use: its conv weights already live in kernel storage.  (On a net's very FIRST train-mode forward the lazy
        # re-housing of nn._to_channels_last_ moves the weights and so happens to change every key -- that accident is not the mechanism)
        row.stats_pass(net, dev, times=1)
        w0 = state_of(net)
        ptrs = [p.data_ptr() for p in net.parameters()]
        epoch = optim.weights_epoch()
        row.run(net, dev)
        row.stats_pass(net, dev)                         # statistics move; NO optimizer step before the next eval forward
        assert optim.weights_epoch() == epoch and ptrs == [p.data_ptr() for p in net.parameters()]
    elif col == 'M6':
        first = adam(net, row.lr)
        first.zero_grad()
        row.run(net, dev)
        if row.train:
            first.step()
        else:
            step_after_real_backward(row, net, first, dev)
        views = [p._cat_grad_view.data_ptr() for p in net.parameters()]
        opt = adam(net, row.lr)                          # the optimizer is rebuilt over the same parameters
        opt.zero_grad()
        assert all(p._cat_grad_view.data_ptr() != v for p, v in zip(net.parameters(), views))
        # the real backward below derives the operands from the weights the FIRST optimizer left: those are what a stale operand would
        # hold after the second one's step, so (c) is measured from them
        w0 = state_of(net)
        step_after_real_backward(row, net, opt, dev)
    else:
        raise AssertionError(col)
    return opt, w0, keys0


def bars_for(ref, given):
    return {k: (given[k] if given and k in given else TOL * float(v.abs().max())) for k, v in ref.items()}


def compare(what, got, ref, bars, note):
    worst = {}
    for k, r in ref.items():
        err = (got[k] - r).abs()
        worst[k] = float((err / bars[k]).max()) if torch.is_tensor(bars[k]) else float(err.max()) / bars[k]
    top = max(worst, key=worst.get)
    print('%s %s: worst %.3g of its bar (%s, %d tensors)' % (what, note, worst[top], top, len(worst)))
    for k, v in worst.items():
        if v > 1.0:
            print('    %s: %.3g of its bar; largest |fp64| %.3g, largest error %.3g' % (k, v, float(ref[k].abs().max()), float((got[k] - ref[k]).abs().max())))
    assert worst[top] <= 1.0, (what, note, {k: v for k, v in worst.items() if v > 1.0})


def upper_quartile(t):
    return float(torch.quantile(t.reshape(-1).double(), 0.75))


def separation(ref0, ref1, bars):
    """(c): per compared tensor, the upper quartile over its elements of |fp64(W0) - fp64(W1)| in units of the bar it is compared with: at
    least a quarter of the compared elements lie further apart than that.  (Not the median: behind a ReLU half of the elements are 0
    whatever the weights.)  check_cell asserts it for y and dx, the tensors computed FROM the derived operand: a convolution's own weight
    and bias gradients are sums over x and dy and read no weight at all (their separation is exactly 0 for the single-conv rows, and the
    last BatchNorm's bias gradient is 0 for the blocks), so they say nothing about a stale operand and are held to (a) and (b) only."""
    out = {}
    for k, r in ref1.items():
        d = (ref0[k] - r).abs()
        out[k] = upper_quartile(d / bars[k]) if torch.is_tensor(bars[k]) else upper_quartile(d) / bars[k]
    return out


def check_cell(row, col, dev, w0_ref):
    from cat_amd import ops
    net = row.build(dev)
    opt, w0, keys0 = mutate(col, row, net, dev)
    w1 = state_of(net)
    if w0 is not None:
        w0_ref = row.ref(w0)[0]
    # 3: the same objects again
    clear_grads(net, opt)
    split0 = ops.STATS.get('split_dgrad', 0)
    with launches() as names:
        warm = row.run(net, dev)
    for must in tuple(row.uses) + tuple(row.derives):
        assert must in names, (row.name, col, must, sorted(set(names)))
    if row is R3:
        assert ops.STATS.get('split_dgrad', 0) == split0 + 1
    if keys0 is not None:
        # M1 / M3 of a fold: the real backward between the two eval forwards runs the norms in train mode, which also bumps the statistics
        # count of the key -- the cell alone would pass on that part.  The step must show in the key's own EPOCH part (M1: one epoch on; M3:
        # -1, not owned, to the optimizer's epoch).  M4 isolates the same part under replay.
        keys1 = row.fold_keys(net)
        assert len(keys1) == len(keys0) and all(k1[1] != k0[1] for k0, k1 in zip(keys0, keys1)), (row.name, col, keys0, keys1)
    if isinstance(row, FusedRow):      # forward + backward tables, each ONE launch: the merged table for two stale plans, the plan's own for one
        assert len(names.prepared(net)) == 2, (len(names.prepared(net)), names.count('cat_prep_run'))
    # 4 (b), (c): fp64 on the host
    ref1, given = row.ref(w1)
    bars = bars_for(ref1, given)
    compare(row.name, warm, ref1, bars, col + ' warm vs fp64(W1)')
    sep = separation(w0_ref, ref1, bars)
    print('%s %s (c) upper quartile of |fp64(W0) - fp64(W1)| / bar: %s' % (row.name, col, {k: '%.3g' % v for k, v in sep.items() if k in ('y', 'dx')}))
    assert all(sep[k] > SEPARATION for k in ('y',) + (('dx',) if row.train else ())), sep
    # 4 (a): a twin that never ran, W1 by copy_
    cold_net = row.build(dev, draw=2)
    cold_net.load_state_dict(w1)
    cold = row.run(cold_net, dev)
    assert cold.keys() == warm.keys()
    for k in warm:
        assert torch.equal(warm[k], cold[k]), (row.name, col, k, float((warm[k] - cold[k]).abs().max()))
    # 4 (d): nothing changed -> nothing is derived again
    before = row.derived(net)
    assert before
    clear_grads(net, opt)
    with launches() as names:
        again = row.run(net, dev)
    rederived = [n for n in names if n in DERIVE and n != 'cat_prep_run'] + ['cat_prep_run'] * len(names.prepared(net))
    for _ in range(getattr(row, 'folds_per_call', 0)):
        rederived.remove('cat_bn_fold')
    assert not rederived, (row.name, col, rederived)
    after = row.derived(net)
    assert len(after) == len(before) and all(a is b for a, b in zip(after, before))
    assert all(torch.equal(again[k], warm[k]) for k in ('y',))
    return names


_REF0 = {}


def ref0(row):
    """fp64 result with W0: computed once per row, shared by its cells."""
    if row.name not in _REF0:
        _REF0[row.name] = row.ref(row.state(0))[0]
    return _REF0[row.name]


CELLS = [(R1Z, c) for c in ('M1', 'M2', 'M3', 'M3b', 'M6')] + [(R1R, c) for c in ('M1', 'M2', 'M3', 'M3b', 'M6')] + \
        [(R2, c) for c in ('M1', 'M2', 'M3', 'M3b')] + \
        [(R4, c) for c in ('M1', 'M2', 'M3', 'M3b', 'M5', 'M5owned')] + \
        [(R5, c) for c in ('M1', 'M2', 'M3', 'M3b', 'M5', 'M5owned')] + \
        [(R6, c) for c in ('M1', 'M2', 'M5', 'M5owned')] + \
        [(R7A, c) for c in ('M1', 'M2', 'M3', 'M3b', 'M6')] + [(R7B, c) for c in ('M1', 'M2', 'M3', 'M6')]


@pytest.mark.parametrize('row,col', CELLS, ids=['%s-%s' % (r.name.split()[0] + ('r' if r is R1R else '') + ('x1' if r is R7B else ''), c) for r, c in CELLS])
def test_cell(dev, small_planes, row, col):
    check_cell(row, col, dev, ref0(row))


@pytest.mark.parametrize('col', ['M5', 'M5owned'])
def test_fold_follows_statistics_on_the_general_norm_path(dev, col):
    """R4 x M5 once more WITHOUT the lowered tile threshold: on a plane this small the train-mode conv -> BatchNorm pair stays on the general
    kernels (cat_norm_fwd writes the running statistics) instead of the quad-granule conv + cat_tnorm_finalize2."""
    with launches() as names:
        check_cell(R4, col, dev, ref0(R4))
    assert 'cat_norm_fwd' in names and 'cat_tnorm_finalize2' not in names


@pytest.fixture()
def split():
    from cat_amd import ops
    old = ops.set_mfma_split(True)
    yield
    ops.set_mfma_split(old)


@pytest.mark.parametrize('col', ['M1', 'M2'])
def test_split_planes_cell(dev, split, col):
    """R3 under ops.set_mfma_split(True): 4 x 4 stride 2 pad 1, 128 -> 128, on an 8 x 12 plane (cat_conv2d_dgrad_split_applicable has no plane
    condition: one partial 128-row tile per stride class)."""
    from cat_amd import _lib as L
    from cat_amd import ops
    import ctypes as C
    g = ops._conv_geom(1, 8, 12, 128, 128, 4, 6, 128, 128, 4, 4, 2, 1, L.PAD_ZERO, wcs=128)
    assert L.query('cat_conv2d_dgrad_split_applicable', C.byref(g)) == 1
    check_cell(R3, col, dev, ref0(R3))


def test_transposed_filter_row_is_on_its_kernel(dev):
    """R2's layer is the conv_dgrad32dt case of tests/test_conv_variants_gpu.py: the data gradient reads the transposed filter copy."""
    from cat_amd import _lib as L
    from cat_amd import ops
    import ctypes as C
    g = ops._conv_geom(1, 9, 11, 100, 100, 9, 11, 32, 32, 1, 1, 1, 0, L.PAD_ZERO, wcs=100)
    assert L.query('cat_conv2d_dgrad_t_applicable', C.byref(g)) == 1


# ====================================================================================================================== R9: the metric networks' folds
@pytest.mark.parametrize('which', ['inception', 'drn'])
def test_metric_fold_follows_load_state_dict(dev, which):
    """R9 x M2: metric.inception.BasicConv2d._folded and metric.drn._folded (conv + eval BatchNorm + ReLU, 8 -> 8 3x3 on 1 x 9 x 9).  These
    networks are never trained: their weights change by load_state_dict only."""
    from cat_amd import _lib as L
    from cat_amd.metric import drn, inception
    eps = 0.001 if which == 'inception' else drn.BN_EPS

    class Pair(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv, self.bn = nn.Conv2d(8, 8, 3, padding=1, bias=False), nn.BatchNorm2d(8, eps=eps)

    def build(draw):
        m = inception.BasicConv2d(8, 8, 3, padding=1) if which == 'inception' else Pair()
        m.load_state_dict(detfill.fill_state_dict(m.state_dict(), 190 + 1000 * draw))
        return m.to(dev).eval()

    def run(m):
        with torch.no_grad():
            y = m(nhwc(x, dev)) if which == 'inception' else drn.conv_bn_act(nhwc(x, dev), m.conv, m.bn, L.ACT_RELU)
        torch.cuda.synchronize()
        return host(y)

    def ref(sd):
        sd = {k: v.double() for k, v in sd.items()}
        z = F.conv2d(x.double(), sd['conv.weight'], None, 1, 1)
        return F.relu(F.batch_norm(z, sd['bn.running_mean'], sd['bn.running_var'], sd['bn.weight'], sd['bn.bias'], False, 0.0, eps))

    folded = (lambda m: m._folded()) if which == 'inception' else (lambda m: drn._folded(m.conv, m.bn))
    x = detfill.normal((1, 8, 9, 9), 191)
    net = build(0)
    y0 = run(net)
    net.load_state_dict(detfill.fill_state_dict(net.state_dict(), 190 + 1000))
    w1 = state_of(net)
    warm = run(net)
    r0, r1 = ref(state_of(build(0))), ref(w1)
    bar = TOL * float(r1.abs().max())
    assert float((y0 - r0).abs().max()) <= TOL * float(r0.abs().max())
    print('R9 %s: warm vs fp64(W1) %.3g of the bar; (c) upper-quartile separation %.3g bars' % (which, float((warm - r1).abs().max()) / bar,
                                                                                              upper_quartile((r0 - r1).abs()) / bar))
    assert float((warm - r1).abs().max()) <= bar                                  # (b)
    assert upper_quartile((r0 - r1).abs()) > SEPARATION * bar                     # (c)
    cold = build(2)
    cold.load_state_dict(w1)
    assert torch.equal(run(cold), warm)                                           # (a)
    before = folded(net)
    assert torch.equal(run(net), warm)
    assert all(a is b for a, b in zip(folded(net), before))                       # (d)


# ====================================================================================================================== M4: captured-step replay
class StandIn:
    """The least a model must be for cat_amd.graph.GraphedStep: set_input, optimize_parameters, optimizers and a loss tensor.  One step is
    net (train mode) -> L1 loss (ops.LossFn) -> backward -> FusedAdam.step; the net's output is bound as Sfake_B, one of the attributes
    GraphedStep restores after an eager fallback step."""

    def __init__(self, net, dev):
        from cat_amd import loss as closs
        self.net, self.device, self.criterion = net, dev, closs.L1Loss()
        self.optimizer = adam(net, M4_LR)
        self.optimizers = [self.optimizer]

    def set_input(self, batch):
        from cat_amd import ops
        self.real_A, self.real_B = ops.to_nhwc(batch['A']), ops.to_nhwc(batch['B'])

    def optimize_parameters(self, steps):
        from cat_amd import lossvalue
        self.optimizer.zero_grad()
        self.Sfake_B = self.net(self.real_A)
        self.loss_G = self.criterion(self.Sfake_B, self.real_B)
        lossvalue.backward_terms([(1.0, self.loss_G)])
        self.optimizer.step()


def forward64(row, sd, x, train):
    twin = row.twin().double()
    twin.load_state_dict({k: v.double() for k, v in sd.items()})
    twin.train(train)
    with torch.no_grad():
        return twin(x.double())


M4_ROWS = {'R1': R1Z, 'R4': R4, 'R7': R7A}
# eight consecutive Adam steps (three warm-up, the replays, the eager one): at lr 0.5 they walk a BatchNorm's beta to about -3 and the ReLU
# behind it outputs zeros whatever the weights (measured: upper-quartile separation of consecutive steps 0).  0.1 a step still moves
# every weight by a good part of its standard deviation (detfill: N(0, 1 / fan_in), 0.1 .. 0.16 here), and (c) is asserted all the same
M4_LR = 0.1


@pytest.mark.parametrize('which', list(M4_ROWS))
def test_captured_step_replay(dev, small_planes, which):
    """M4.  Three eager warm-up steps and one capture (GraphedStep), then per replay k + 1: its output must be the fp64 train-mode forward with
    the weights read back after replay k -- the pack / prep launch sits INSIDE the graph and reads the weights the previous replay left.
    After the replays: one eager eval forward -- (a) against a twin that never ran, (b) against fp64 with the latest weights; then a batch of
    another shape (GraphedStep runs that step eagerly) and one more replay, same checks.  R4: the eager eval forward (conv + BatchNorm folded
    from the statistics the replays moved) also runs BETWEEN the replays.  One stream, a linear graph."""
    from cat_amd import optim
    from cat_amd.graph import GraphedStep
    row = M4_ROWS[which]
    net = row.build(dev).train()
    model = StandIn(net, dev)
    n, c, h, w = row.x.shape
    # targets above zero: an L1 loss against targets of both signs drives a ReLU output to all zeros within these few steps (measured:
    # the separation of consecutive steps fell 1060, 680, 300, 0 bars), and then no weight shows in the output any more
    target = lambda shape, seed: (detfill.normal(shape, seed).abs() + 0.5).to(dev)
    batches = [{'A': detfill.normal((n, c, h, w), 900 + i).to(dev), 'B': target(tuple(row.gy.shape), 950 + i)} for i in range(5)]
    odd = {'A': detfill.normal((n + 1, c, h, w), 980).to(dev), 'B': target((n + 1,) + tuple(row.gy.shape[1:]), 981)}
    step = GraphedStep(model, batches[0])
    seps = []

    def replay_and_check(batch, before):
        step(batch)
        torch.cuda.synchronize()
        got = host(model.Sfake_B)
        want = forward64(row, before, batch['A'].cpu(), True)
        bar = TOL * float(want.abs().max())
        ratio = float((got - want).abs().max()) / bar
        print('M4 %s replay %d vs fp64(weights after the previous step): %.3g of the bar' % (which, step.replays, ratio))
        assert ratio <= 1.0, (which, step.replays, ratio)
        after = state_of(net)
        seps.append(upper_quartile((forward64(row, after, batch['A'].cpu(), True) - want).abs()) / bar)
        return after

    def eager_eval_and_check(sd):
        """an eval-mode no-grad forward of the SAME net between / after replays: folds and forward packs re-derived outside the graph"""
        net.eval()
        with torch.no_grad():
            y = host(net(nhwc(row.x, dev)))
            again = host(net(nhwc(row.x, dev)))
        net.train()
        want = forward64(row, sd, row.x, False)
        bar = TOL * float(want.abs().max())
        assert float((y - want).abs().max()) <= bar, (which, float((y - want).abs().max()) / bar)
        cold = row.build(dev, draw=2)
        cold.load_state_dict(sd)
        cold.eval()
        with torch.no_grad():
            assert torch.equal(host(cold(nhwc(row.x, dev))), y) and torch.equal(again, y)

    sd = state_of(net)
    replays0 = step.replays
    for k in range(3):
        sd = replay_and_check(batches[1 + k], sd)
        if which == 'R4':
            eager_eval_and_check(sd)
    assert step.replays == replays0 + 3
    eager_eval_and_check(sd)
    epoch = optim.weights_epoch()
    step(odd)                                            # another batch size: GraphedStep runs this step eagerly
    assert step.replays == replays0 + 3 and optim.weights_epoch() == epoch + 1
    sd = state_of(net)
    sd = replay_and_check(batches[4], sd)
    eager_eval_and_check(sd)
    print('M4 %s (c) upper-quartile separation of consecutive steps: %s bars' % (which, ['%.3g' % s for s in seps]))
    assert min(seps) > SEPARATION, seps


# ====================================================================================================================== R10: the discriminator's stage plan
@pytest.fixture()
def branch_streams():
    """The distillers' constructors set the process-wide branch-stream preference: put it back."""
    from cat_amd import ops
    old = ops.branch_streams_enabled()
    yield
    ops.set_branch_streams(old)


def test_d_stage_plan_follows_a_rebuilt_optimizer(dev, branch_streams):
    """R10 x M6.  BaseInceptionDistiller.d_stage_plan caches float ranges of optimizer_D's flat gradient buffer, and its stages differentiate
    with torch.autograd.grad, which drops what a node returns for a parameter: the cut is right only while every discriminator parameter's
    gradient sink is its span of THAT buffer.  PatchGAN ndf 8 on 32 x 32.  After each change backward_D_stages must give plain backward_D's
    gradients bit for bit, or the plan must be None:
      - a second FusedAdam over the same parameters that the model does NOT adopt re-houses them and takes over their sinks: None;
      - a rebuilt optimizer the model adopts: a NEW plan over the new buffer, staged == plain;
    and while nothing changes the plan is the same object."""
    import helpers as H
    from cat_amd.distillers import create_distiller
    from cat_amd.optim import FusedAdam
    opt = H.make_opt(norm='batch', track=True, ndf=8, teacher_ngf=16, student_ngf=8)
    model = create_distiller(opt, verbose=False)
    model.netD.load_state_dict(detfill.fill_state_dict(model.netD.state_dict(), 410))
    model.netD.train()
    model.real_A, model.real_B = nhwc(detfill.images((2, 3, 32, 32), 411), dev), nhwc(detfill.images((2, 3, 32, 32), 412), dev)
    model.Sfake_B = nhwc(detfill.images((2, 3, 32, 32), 413), dev)

    def grads(staged):
        optimizer = model.optimizer_D
        optimizer.zero_grad()
        if staged:
            fns, slices = model.backward_D_stages()
            n = optimizer._flat[0]['n']
            assert sorted(slices) == sorted(model.d_stage_plan()[1]) and slices[-1][0] == 0 and slices[0][1] == n
            for fn in fns:
                fn()
        else:
            model.backward_D()
        torch.cuda.synchronize()
        g = optimizer.flat_grads()[0].detach().cpu().clone()
        assert float(g.abs().max()) > 0
        return g

    plan = model.d_stage_plan()
    assert plan is not None and model.d_stage_plan() is plan                       # (d)
    assert torch.equal(grads(True), grads(False))
    assert model.d_stage_plan() is plan
    # a second FusedAdam over the same parameters, not adopted by the model: the sinks now lie in ITS buffer
    other = FusedAdam(model.netD.parameters(), lr=opt.lr, betas=(opt.beta1, 0.999))
    other.zero_grad()
    assert model.d_stage_plan() is None
    # the model adopts the rebuilt optimizer: a new plan over the new buffer
    model.optimizer_D = other
    model.optimizers = [model.optimizer_G, other]
    plan2 = model.d_stage_plan()
    assert plan2 is not None and plan2 is not plan and model.d_stage_plan() is plan2
    staged, plain = grads(True), grads(False)
    assert torch.equal(staged, plain)
    # (b): the staged gradients against fp64 autograd of the same discriminator step (hinge loss, 0.5 / 0.5) on the host
    sd = {k: v.double() for k, v in state_of(model.netD).items()}
    layers, cin = [], 6
    for i, cout in enumerate((8, 16, 32, 64)):
        layers.append(nn.Conv2d(cin, cout, 4, stride=2 if i < 3 else 1, padding=1, bias=i == 0))
        layers += ([nn.BatchNorm2d(cout)] if i else []) + [nn.LeakyReLU(0.2)]
        cin = cout
    twin = nn.Sequential(*layers, nn.Conv2d(64, 1, 4, stride=1, padding=1)).double().train()
    twin.load_state_dict({k[len('model.'):]: v for k, v in sd.items()})
    a, b, f = (detfill.images((2, 3, 32, 32), 411 + i).double() for i in range(3))
    loss = 0.5 * F.relu(1.0 + twin(torch.cat([a, f], 1))).mean() + 0.5 * F.relu(1.0 - twin(torch.cat([a, b], 1))).mean()
    loss.backward()
    want = {'model.' + k: p.grad for k, p in twin.named_parameters()}
    top = max(float(v.abs().max()) for v in want.values())
    model.optimizer_D.zero_grad()
    for fn in model.backward_D_stages()[0]:
        fn()
    torch.cuda.synchronize()
    worst = {k: float((host(p.grad) - want[k]).abs().max()) / (TOL * max(float(want[k].abs().max()), 1e-3 * top))
             for k, p in model.netD.named_parameters()}
    print('R10 staged discriminator gradients vs fp64: worst %.3g of the bar' % max(worst.values()))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}
