"""The fused inception block (cat_amd/fused_block.py) and the fused six-branch SPADE unit (cat_amd/fused_spade.py) are ONE pipeline

    stage 1   first convs of all branches -> one concatenated pre-norm buffer Z1 + per-tile statistics   (one launch: the first STAGE1_FWD row that applies -- cat_tstage1_fwd /
              cat_tstage1ws_fwd / cat_tstage1ws7_fwd / cat_tstage1n7_fwd; else one cat_tconv_fwd per kernel size)
    finalize  scale / shift of all stage-1 norms + their running statistics                               (cat_tnorm_finalize)
    dw        all depthwise convs (one launch per <= 18 / 24 channel quads), norm + activation of stage 1 applied while staging   (cat_dwm_fwd;
              cat_dwm7_fwd for a plan with a 7 x 7 depthwise branch)
    finalize
    stage 2   the branch sum: the second convs K-concatenated, norm + activation applied while staging   (cat_tconv_fwd)

over one static layout, and both are defined here, once.  `Plan` is the layout -- channel slices, kernel-size groups, persistent operand
buffers, the table-driven operand preparation (cat_prep_run) and the concatenated parameter-gradient vectors with their scatter targets.
`forward_g` is the stage sequence up to the stage-2 segment list, `backward_g` the ten steps of the backward pass from the gradient of
the branch sum to the scattered parameter gradients; the stage functions they call follow the plan.  Five things distinguish the callers,
each a plan property or an argument, never "which caller":

    p.reflect         reflect padding (block) instead of 'same' zero padding
    p.instance        per-sample statistics (InstanceNorm) instead of batch statistics; p.affine: the norms have gamma / beta
    p.shards          virtual replicas of a BatchNorm plan (1: one group over the batch): statistics per torch.chunk(batch, shards) shard;
                      p.per_sample: the scale / shift tables are one row per sample (InstanceNorm, or shards > 1: the rows of a shard's
                      samples are equal), the form every apply / staging kernel takes through its `sstride`
    statistics        collected and finalized (train mode), or `folded`: the eval form on cached scale / shift, no statistics, no finalize
    sync              the finalize (and norm backward) to use: local, or with one statistics exchange over ranks per stage (the pipeline is
                      a generator over those exchanges; whoever drives it performs them)
    drop              an optional dropout ticket: the stage-2 operands are then materialised with their masks

plus, in the backward pass, p.s1d / p.s1d7 (the second convs' input gradients as one cat_tstage1_dgrad / cat_tstage1n7_dgrad launch),
p.wgrad_batch (weight-gradient partials reduced by one launch when there are no branch streams) and `skip_grad` (a skip connection's share
of the input gradient).  The callers keep their stage-2 launch and tail (the block's closing pw_bn and residual; the unit's epilogue addend), their plan subclass and
the autograd Functions."""
import ctypes as C
import os

import torch

from . import _lib as L
from . import derived
from . import nn as cnn
from . import ops
from . import optim
from . import tconv

PLAN = derived.slot('_cat_fused_plan')      # R7: a fused block's plan (the slot holds the Plan itself, which keeps its own keys)
# Stage 1 of a block whose widths cat_tstage1_fwd does not take (the full-width teacher: 42 / 42 / 176) as ONE statistics-writing launch
# (cat_tstage1ws_fwd, csrc/conv_s1ws.hip) instead of one cat_tconv_fwd per kernel size, each staging the same input.  CAT_STAGE1WS=0 /
# set_stage1_wide(False): the three launches (measurements: profiles/wide_block_bench.txt)
_STAGE1WS = os.environ.get('CAT_STAGE1WS', '1') != '0'


def set_stage1_wide(on):
    global _STAGE1WS
    old, _STAGE1WS = _STAGE1WS, bool(on)
    return old


# The same for the kernel sizes 3 5 7 (first convs {1, 3, 5, 7}; the full-width widths 44 / 44 / 44 / 132): ONE cat_tstage1ws7_fwd launch
# (csrc/conv_s1ws7.hip) instead of four cat_tconv_fwd.  Independent of CAT_STAGE1WS.  CAT_STAGE1WS7=0 / set_stage1ws7(False): the four
# launches (measurements: profiles/stage1ws7_bench.txt)
_STAGE1WS7 = os.environ.get('CAT_STAGE1WS7', '1') != '0'


def set_stage1ws7(on):
    global _STAGE1WS7
    old, _STAGE1WS7 = _STAGE1WS7, bool(on)
    return old


# The one-launch stage-1 kernels (docs/CONV_VARIANTS.md, "Stage 1 in one launch"), in priority order: (entry, width query, kernel size of
# each slot, geometry struct, gate read at every call or None, smallest plane of a mirrored window tested here -- the 5 3 1 entries refuse
# theirs themselves).  All share one argument list and one output contract: column slices of Z1 + per-tile statistics.
STAGE1_FWD = (
    ('cat_tstage1_fwd', 'cat_tstage1_supported', (5, 3, 1), L.Stage1Geom, None, 0),
    ('cat_tstage1ws_fwd', 'cat_tstage1ws_supported', (5, 3, 1), L.Stage1Geom, lambda p: _STAGE1WS, 0),      # the wide block's widths
    ('cat_tstage1ws7_fwd', 'cat_tstage1ws7_supported', (7, 5, 3, 1), L.Stage1S7Geom, lambda p: _STAGE1WS7, 7),      # ... with one more slot
    ('cat_tstage1n7_fwd', 'cat_tstage1n7_supported', (7, 5, 3, 1), L.Stage1S7Geom, lambda p: getattr(p, 'stage1_n7', False), 7),      # narrow widths
)
# The second convs' input gradients in one launch, first match wins: (entry, width query, kernel sizes of the residual slots -- exactly
# one branch each; the last slot is the depthwise branches' N-concatenated 1 x 1 convs --, geometry struct, the plan attribute that holds
# the residual branches).  Read by the planner (fused_spade.py) and by backward_g.
STAGE1_DGRAD = (
    ('cat_tstage1n7_dgrad', 'cat_tstage1n7_supported', (7, 5, 3), L.Stage1S7Geom, 's1d7'),
    ('cat_tstage1_dgrad', 'cat_tstage1_dgrad_supported', (5, 3), L.Stage1Geom, 's1d'),
)


def cs4(c):
    return (c + 3) // 4 * 4


def dw_launches(quads, maxq):
    """Branch-aligned grouping of the depthwise branches (quads[i] = channel quads of branch i) into launches of at most `maxq` quads, in
    order and greedily: -> [(first branch, one past the last)], or None when a single branch is wider than a launch.  The quads of a
    depthwise conv are independent and one workgroup of cat_dwm_fwd / cat_dwm_bwd stages one group of at most kDwGroup of them, so a
    launch's width is bounded only by the kernels' argument arrays (CAT_DWM_MAXQ forward, CAT_DWM_MAXQ_BWD backward)."""
    out, b0, acc = [], 0, 0
    for i, q in enumerate(quads):
        if q > maxq:
            return None
        if acc + q > maxq:
            out.append((b0, i))
            b0, acc = i, 0
        acc += q
    if quads:
        out.append((b0, len(quads)))
    return out


def has_hooks(mods):
    for m in mods:
        for s in m.modules():
            if s._forward_hooks or s._forward_pre_hooks or s._backward_hooks:
                return True
    return False


class Plan:
    """Static layout of one fused unit: channel slices, persistent operand buffers and the preparation job table.

    res / dws: branch dicts (kind, k, m, conv1, bn1, conv2; dw branches also kd, dconv, bn2) -- they receive their slice offsets here.
    params: the unit's parameters, ordered and de-duplicated (table sources and epoch key).  Subclasses set `what` (error messages) and
    `GAMMA0` (what a norm without gamma reads from the concatenated vectors) and say in `_merges_dw_dgrad` whether the depthwise
    branches' 1 x 1 second convs get an N-concatenated input-gradient filter stream (`dpack2_dw`).  What the pipeline reads beyond the
    layout, with the defaults a subclass overrides: `reflect` / `instance` / `affine` (padding, per-sample statistics, norms with
    gamma / beta), `s1d` (the two residual branches whose second-conv input gradients join the depthwise ones in ONE cat_tstage1_dgrad
    launch, or None), `s1d7` (the same for the three residual branches 7 x 7, 5 x 5, 3 x 3 of a 3 5 7 unit: ONE cat_tstage1n7_dgrad) and
    `wgrad_batch` (on one stream the weight-gradient partial sums are reduced by one launch, ops.WgradBatch)."""
    what = 'fused unit'
    GAMMA0 = 0.0
    reflect = instance = False
    shards = 1

    @property
    def per_sample(self):
        return self.instance or self.shards > 1
    affine = True
    s1d = None
    s1d7 = None
    wgrad_batch = False

    def __init__(self, res, dws, cin, cout, dev, params, dw_maxq=L.DWM_MAXQ_BWD):
        self.dev = dev
        self.params = params
        self.Cin, self.csi = cin, cs4(cin)
        self.Cout, self.cso = cout, cs4(cout)
        # stage-1 channel order: [res k=1 | dw ... | res k=3 | res k=5 | res k=7] so that same-kernel first convs are adjacent (N concat) and
        # the depthwise inputs are one contiguous slice range
        order = [b for b in res if b['k'] == 1] + dws + [b for b in res if b['k'] == 3] + [b for b in res if b['k'] == 5] + \
                [b for b in res if b['k'] == 7]
        off = 0
        for b in order:
            b['o1'], b['w1'] = off, cs4(b['m'])
            off += b['w1']
        self.hc1 = off
        off = 0
        for b in dws:
            b['od'] = off
            off += cs4(b['m'])
        self.hcd = off
        self.dw_in0 = dws[0]['o1'] if dws else 0
        # depthwise launches: branch-aligned groups of at most dw_maxq quads, ONE grouping for both directions of a training plan (the
        # backward one; a forward-only plan may ask for CAT_DWM_MAXQ).  Each launch reads its own contiguous filter frame
        # [ft][launch width] at float offset ft * (its first channel) of w25 -- one launch: the frame [ft][hcd] at offset 0.  A branch wider
        # than a launch is refused by the callers' `applicable`; such a plan keeps one launch, which the kernel refuses.
        # ONE frame side per plan: 5 (ft = 25; cat_dwm_fwd / cat_dwm_bwd), or 7 (ft = 49; cat_dwm7_fwd / cat_dwm7_bwd) iff some depthwise
        # branch is 7 x 7 -- a plan within {1, 3, 5} builds the buffers and issues the calls it always has
        self.fs = 7 if any(b['kd'] == 7 for b in dws) else 5
        self.ft = self.fs * self.fs
        self.dw_fwd_entry, self.dw_bwd_entry, self.dw_ws_entry, self.dw_prep_kind = \
            ('cat_dwm_fwd', 'cat_dwm_bwd', 'cat_dwm_bwd_ws_bytes', 2) if self.fs == 5 else ('cat_dwm7_fwd', 'cat_dwm7_bwd', 'cat_dwm7_bwd_ws_bytes', 5)
        self.dw_maxq = dw_maxq
        spans = dw_launches([cs4(b['m']) // 4 for b in dws], dw_maxq) or ([(0, len(dws))] if dws else [])
        self.dw_spans = tuple(spans)
        self.dw_groups = [(dws[b0:b1], dws[b0]['od'], dws[b1 - 1]['od'] + cs4(dws[b1 - 1]['m'])) for b0, b1 in spans]      # (branches, first channel, end)
        for bs, o, end in self.dw_groups:
            for b in bs:
                b['f0'], b['fcs'] = o, end - o
        self.branches, self.res, self.dws = order, res, dws
        # stage-1 launches: one per first-conv kernel size
        self.groups = []
        for k in (1, 3, 5, 7):
            bs = [b for b in order if b['k'] == k]
            if bs:
                g0, g1 = bs[0]['o1'], bs[-1]['o1'] + bs[-1]['w1']
                self.groups.append(dict(k=k, off=g0, width=g1 - g0, branches=bs))
        z = lambda n, v=0.0: torch.full((max(n, 4),), v, device=dev, dtype=torch.float32)
        # persistent operands
        for g in self.groups:
            g['pack'] = z(tconv.pack_floats(g['k'], self.csi, g['width']))
        self.gamma1, self.beta1, self.bias1 = z(self.hc1, self.GAMMA0), z(self.hc1), z(self.hc1)
        self.gammad, self.betad, self.biasd = z(self.hcd, self.GAMMA0), z(self.hcd), z(self.hcd)
        self.bias2 = z(self.cso)
        self.w25 = z(self.ft * max(self.hcd, 4))
        self.has_bias1 = any(b['conv1'].bias is not None for b in order)
        self.has_biasd = any(b['dconv'].bias is not None for b in dws)
        self.has_bias2 = any(b['conv2'].bias is not None for b in order)
        # stage-2 (branch sum) filter stream: one segment per branch
        po = 0
        for b in order:
            k2 = b['k'] if b['kind'] == 'res' else 1
            b['k2'], b['p2off'] = k2, po
            po += tconv.pack_floats(k2, b['w1'], cout)
        self.pack2 = z(po)
        # backward filter streams: input gradients of the second convs (per branch) and of the first convs (K-concatenated)
        po = 0
        for b in order:
            b['d2off'] = po
            po += tconv.pack_floats(b['k2'], self.cso, b['m'])
        self.dpack2 = z(po)
        # ... the 1 x 1 second convs of the depthwise branches N-concatenated: their input gradients are ONE launch over dT into dAd
        self.dpack2_dw = z(tconv.pack_floats(1, self.cso, self.hcd)) if self._merges_dw_dgrad() else None
        po = 0
        for b in order:
            b['d1off'] = po
            po += tconv.pack_floats(b['k'], b['w1'], cin)
        self.dpack1 = z(po)
        # concatenated parameter gradients (norm gamma / beta, conv biases) and where their slices go
        self.gv = dict(g1=z(self.hc1), b1=z(self.hc1), c1=z(self.hc1), gd=z(self.hcd), bd=z(self.hcd), cd=z(self.hcd), c2=z(self.cso))
        self.targets = []       # (vector name, offset, n, parameter)
        for b in order:
            if b['bn1'].weight is not None:
                self.targets += [('g1', b['o1'], b['m'], b['bn1'].weight), ('b1', b['o1'], b['m'], b['bn1'].bias)]
            if b['conv1'].bias is not None:
                self.targets.append(('c1', b['o1'], b['m'], b['conv1'].bias))
            if b['conv2'].bias is not None:
                self.targets.append(('c2', 0, cout, b['conv2'].bias))
        for b in dws:
            if b['bn2'].weight is not None:
                self.targets += [('gd', b['od'], b['m'], b['bn2'].weight), ('bd', b['od'], b['m'], b['bn2'].bias)]
            if b['dconv'].bias is not None:
                self.targets.append(('cd', b['od'], b['m'], b['dconv'].bias))
        # merged weight-gradient launches: the 1 x 1 first convs of all branches are ONE GEMM over the N-concatenated dZ1 slice (x is read
        # once instead of once per branch; rows of `w1` then go to the parameters), the 1 x 1 second convs of the depthwise branches one
        # K-concatenated GEMM over the whole depthwise hidden buffer (columns of `w2`)
        g1 = next((g for g in self.groups if g['k'] == 1), None)
        self.merge1 = g1 if (g1 is not None and len(g1['branches']) > 1) else None
        if self.merge1 is not None:
            self.gv['w1'] = z(g1['width'] * self.csi)
            for b in g1['branches']:
                self.targets.append(('w1', (b['o1'] - g1['off']) * self.csi, b['m'] * self.csi, b['conv1'].weight))
        self.merge2 = len(dws) > 1
        self.targets2d = []      # (vector, src offset, rows, cols, src stride, parameter): dst stride = the parameter's own wcs
        if self.merge2:
            self.gv['w2'] = z(cout * self.hcd)
            for b in dws:
                self.targets2d.append(('w2', b['od'], cout, cs4(b['m']), self.hcd, b['conv2'].weight))
        self.scatter_jobs = None
        self._build_jobs()
        self.key = self.bkey = None

    def _merges_dw_dgrad(self):
        raise NotImplementedError

    def __deepcopy__(self, memo):
        """A copied module builds its own plan at its first forward (plans hold device buffers, job tables with raw parameter addresses and
        the group they are prepared with: none of that belongs to the copy)."""
        return None

    # -- job tables ------------------------------------------------------------------------------------------------------
    def _jobs_to_dev(self, jobs):
        arr = (L.PrepJob * len(jobs))()
        blk = 0
        for i, j in enumerate(jobs):
            for f, v in j.items():
                if f == 'srcs':
                    for k, pv in enumerate(v):
                        arr[i].srcs[k] = pv
                elif f != 'threads':
                    setattr(arr[i], f, v)
            nb = max(1, (j['threads'] + 255) // 256)
            arr[i].block0, arr[i].nblocks = blk, nb
            blk += nb
        t = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.dev)
        self._last_arr = arr      # host copy (prepare_plans merges the tables of all units of a generator into one launch)
        return t, len(jobs), blk

    def _pack_job(self, w, dst_ptr, mode, nn, ck, ks, nt_total, col0):
        wcl, wcs = ops.weight_cl(w)
        if wcl.data_ptr() != w.data_ptr():
            raise RuntimeError(f'{self.what}: conv weights must be in kernel layout')
        taps = ks * ks
        c4 = cs4(ck)
        nfull, rem = c4 // 16, (c4 % 16) // 4
        groups = nfull * taps + ((taps * rem + 3) // 4 if rem else 0)
        ntw = (col0 + nn + 15) // 16 - col0 // 16
        return dict(kind=0, srcs=[w.data_ptr()], dst=dst_ptr, mode=mode, Nn=nn, Ck=ck, ks=ks, wcs=wcs, wn=taps * wcs, c4=c4, nt_total=nt_total, col0=col0,
                    threads=groups * ntw * 64)

    def _build_jobs(self):
        fwd, bwd = [], []
        vec = lambda dst, off, srcs, n: dict(kind=1, srcs=[s.data_ptr() for s in srcs], nsrc=len(srcs), dst=dst.data_ptr() + 4 * off, n=n, threads=n)
        for g in self.groups:
            nt = (g['width'] + 15) // 16
            for b in g['branches']:
                fwd.append(self._pack_job(b['conv1'].weight, g['pack'].data_ptr(), tconv.FWD, b['m'], self.Cin, g['k'], nt, b['o1'] - g['off']))
        nt2 = (self.Cout + 15) // 16
        nt1 = (self.Cin + 15) // 16
        for b in self.branches:
            if b['bn1'].weight is not None:
                fwd.append(vec(self.gamma1, b['o1'], [b['bn1'].weight], b['m']))
                fwd.append(vec(self.beta1, b['o1'], [b['bn1'].bias], b['m']))
            if b['conv1'].bias is not None:
                fwd.append(vec(self.bias1, b['o1'], [b['conv1'].bias], b['m']))
            fwd.append(self._pack_job(b['conv2'].weight, self.pack2.data_ptr() + 4 * b['p2off'], tconv.FWD, self.Cout, b['m'], b['k2'], nt2, 0))
            bwd.append(self._pack_job(b['conv2'].weight, self.dpack2.data_ptr() + 4 * b['d2off'], tconv.DGRAD, b['m'], self.Cout, b['k2'], (b['m'] + 15) // 16, 0))
            bwd.append(self._pack_job(b['conv1'].weight, self.dpack1.data_ptr() + 4 * b['d1off'], tconv.DGRAD, self.Cin, b['m'], b['k'], nt1, 0))
            if self.dpack2_dw is not None and b['kind'] == 'dw':
                bwd.append(self._pack_job(b['conv2'].weight, self.dpack2_dw.data_ptr(), tconv.DGRAD, b['m'], self.Cout, 1, (self.hcd + 15) // 16, b['od']))
        for b in self.dws:
            if b['bn2'].weight is not None:
                fwd.append(vec(self.gammad, b['od'], [b['bn2'].weight], b['m']))
                fwd.append(vec(self.betad, b['od'], [b['bn2'].bias], b['m']))
            if b['dconv'].bias is not None:
                fwd.append(vec(self.biasd, b['od'], [b['dconv'].bias], b['m']))
            kd = b['kd']
            wd = b['dconv'].weight
            if not wd.is_contiguous():
                raise RuntimeError(f'{self.what}: depthwise weights must be contiguous')
            fwd.append(dict(kind=self.dw_prep_kind, srcs=[wd.data_ptr()], dst=self.w25.data_ptr() + 4 * self.ft * b['f0'], Nn=b['m'], ks=kd,
                            col0=b['od'] - b['f0'], cs=b['fcs'], threads=b['m'] * kd * kd))
        b2 = [b['conv2'].bias for b in self.branches if b['conv2'].bias is not None]
        if b2:
            fwd.append(vec(self.bias2, 0, b2, self.Cout))
        self.ptrs = self.ptrs_now()
        self.shapes = tuple(tuple(q.shape) for q in self.params)
        self.ids = tuple(id(q) for q in self.params)
        self.fwd_jobs = self._jobs_to_dev(fwd)
        self.fwd_arr = self._last_arr
        self.bwd_jobs = self._jobs_to_dev(bwd)
        self.bwd_arr = self._last_arr
        self.tables_version = getattr(self, 'tables_version', 0) + 1

    def _epoch_key(self):
        return (optim.epoch_of(self.params), tuple(q._version for q in self.params))

    def ptrs_now(self):
        return tuple(q.data_ptr() for q in self.params)

    def _follow_params(self):
        """Parameter storage moved since the tables were built (FusedAdam flattens its parameters at its first zero_grad / step, i.e.
        between the first forward and the first backward): same layout, new source addresses."""
        if self.ptrs_now() != self.ptrs:
            self._build_jobs()
            self.key = self.bkey = self.scatter_jobs = None

    def _prepare_own(self, backward):
        """The tail of a subclass's prepare(): refresh this plan's derived operands if a weight changed since the last refresh (once per
        optimizer step, and only where the group's merged launch has not done it already)."""
        self._follow_params()
        key = self._epoch_key()
        if (self.bkey if backward else self.key) != key:
            t, n, blocks = self.bwd_jobs if backward else self.fwd_jobs
            L.call('cat_prep_run', ops._p(t), n, blocks, 0, ops._stream())
            if backward:
                self.bkey = key
            else:
                self.key = key


def prepare_many(blocks, backward=False):
    """prepare_plans over the plans of the fused blocks of a generator.  Blocks without a plan yet (first forward) are left to their own
    prepare()."""
    plans = [getattr(b, PLAN, None) for b in blocks]
    prepare_plans([p for p in plans if p is not None], blocks, backward)


def prepare_plans(plans, group, backward=False):
    """The per-step operand preparation (filter packing, parameter gathers) of ALL fused units of a generator as ONE table-driven launch
    instead of one ~12 us launch per unit (9 + 9 per step; 0.11 ms of the 2.97 ms student forward).  Plans whose operands are current are
    skipped; a single stale plan is left to its own prepare().  `group` is what every plan remembers as its group."""
    stale = []
    for p in plans:
        p._follow_params()
        key = p._epoch_key()
        if (p.bkey if backward else p.key) != key:
            stale.append((p, key))
        p.group = group
    if len(stale) < 2:
        return
    # the merged table lives on the first plan and holds the plans it was built from (their ids stay unique while it exists)
    sig = (tuple(id(p) for p, _ in stale), tuple(p.tables_version for p, _ in stale))
    cache = stale[0][0].__dict__.setdefault('_merged', {})
    ent = cache.get(backward)
    ent = ent[1] if ent is not None and ent[0] == sig else None
    if ent is None:
        arrs = [(p.bwd_arr if backward else p.fwd_arr) for p, _ in stale]
        total = sum(len(a) for a in arrs)
        merged = (L.PrepJob * total)()
        i, blk = 0, 0
        for a in arrs:
            for j in a:
                C.memmove(C.byref(merged[i]), C.byref(j), C.sizeof(L.PrepJob))
                merged[i].block0 = blk
                blk += j.nblocks
                i += 1
        t = torch.frombuffer(bytearray(bytes(merged)), dtype=torch.uint8).to(stale[0][0].dev)
        ent = (t, total, blk, tuple(p for p, _ in stale))
        cache[backward] = (sig, ent)
    t, n, nblk = ent[:3]
    L.call('cat_prep_run', ops._p(t), n, nblk, 0, ops._stream())
    for p, key in stale:
        if backward:
            p.bkey = key
        else:
            p.key = key


# ---------------------------------------------------------------------------------------------------------------- forward stages
def stage1(p, x, z1, part1, reflect=False):
    """First convs of all branches: x -> channel slices of Z1 (pre-norm) + tile statistics into part1.  part1 None: the eval form, no
    statistics (always one launch per kernel size).  The one-launch kernels (STAGE1_FWD: the first row whose sizes, gate, plane and width
    query all hold) take exactly the kernel sizes 5, 3 and 1, or 7, 5, 3 and 1 -- at
    the wide widths, or at narrow widths for a plan that carries `stage1_n7` (the GauGAN units under CAT_FUSED_SPADE_K7; the plans of
    fused_block.py and frozen_in.py do not carry it: their narrow 3 5 7 launch order, one launch per size, is pinned by their tests, and
    adopting the narrow kernel there is a later, measured decision).  A plan with another set of sizes runs one launch per size."""
    n, c, h, w = x.shape
    by_k = {g['k']: g for g in p.groups}
    for entry, query, sizes, geom, gate, plane in STAGE1_FWD if part1 is not None else ():
        if set(by_k) != set(sizes) or (gate is not None and not gate(p)) or (reflect and min(h, w) < plane) or \
                not L.query(query, *[by_k[k]['width'] for k in sizes]):
            continue
        # one launch: the kernel sizes share every staged input tile
        gs = geom()
        gs.N, gs.H, gs.W, gs.xcs, gs.cin, gs.reflect, gs.ycs, gs.scs = n, h, w, ops.act_cs(x), c, int(reflect), p.hc1, p.hc1
        packs = (C.c_void_p * len(sizes))()
        for slot, k in enumerate(sizes):
            g = by_k[k]
            gs.col0[slot], gs.width[slot], gs.nvalid[slot] = g['off'], g['width'], sum(b['m'] for b in g['branches'])
            packs[slot] = g['pack'].data_ptr()
        L.call(entry, C.byref(gs), ops._p(x), packs, ops._p(p.bias1) if p.has_bias1 else None, ops._p(z1), ops._p(part1), ops._stream())
        return
    for g in p.groups:
        pad = (g['k'] - 1) // 2
        seg = tconv.Segment(x, g['k'], pad, reflect and pad > 0, 0)
        stats = dict(stats=part1.data_ptr() + 4 * g['off'], scs=p.hc1) if part1 is not None else {}
        tconv.run([seg], g['pack'], (p.bias1.data_ptr() + 4 * g['off']) if p.has_bias1 else None, None, g['width'], n, h, w, h, w, ycs=p.hc1,
                  ycw=g['width'], yptr=z1.data_ptr() + 4 * g['off'], nvalid=sum(b['m'] for b in g['branches']), **stats)


def dwm_geom(p, n, h, w, reflect, group):
    """Geometry of ONE depthwise launch: group = (branches, first channel, end) of p.dw_groups; quads relative to the launch's first."""
    bs, o, end = group
    gd = L.DwmGeom()
    gd.N, gd.H, gd.W, gd.nq, gd.xcs, gd.ycs, gd.scs, gd.reflect = n, h, w, (end - o) // 4, p.hc1, p.hcd, p.hcd, int(reflect)
    for b in bs:
        for q in range((b['od'] - o) // 4, (b['od'] - o + cs4(b['m'])) // 4):
            gd.ks[q] = b['kd']
    return gd


def dwm_fwd(p, z1, scale, shift, zd, partd, reflect=False, per_sample=False):
    """All depthwise convs, one launch per group of the plan (one for up to dw_maxq quads): act(Z1 * scale + shift) of the dw slices,
    applied while staging, -> Zd (+ tile statistics into partd unless None).  A launch works on channel slices of Z1 / scale / shift /
    Zd / the statistics table and on its own filter frame.  per_sample: scale / shift are [n][hc1] (InstanceNorm) instead of one row."""
    n, h, w, _ = z1.shape
    at = lambda t, off: C.c_void_p(t.data_ptr() + 4 * off)
    for group in p.dw_groups:
        o = group[1]
        gd = dwm_geom(p, n, h, w, reflect, group)
        gd.sstride, gd.act, gd.slope = (p.hc1 if per_sample else 0), p.act, p.slope
        i = p.dw_in0 + o
        L.call(p.dw_fwd_entry, C.byref(gd), at(z1, i), at(scale, i), at(shift, i), at(p.w25, p.ft * o), at(p.biasd, o) if p.has_biasd else None,
               at(zd, o), at(partd, o) if partd is not None else None, ops._stream())


def stage2_segs(p, z1, ss1, zd, ssd, reflect=False, per_sample=False, a1=None, ad=None):
    """The K segments of the branch sum: res slices of Z1 and dw slices of Zd, (scale, shift) = ss1 / ssd and the activation applied while
    staging -- or, where the operands are already materialised (dropout), slices of A1 / Ad staged as they are."""
    segs = []
    for b in p.branches:
        res = b['kind'] == 'res'
        k = b['k2']
        if a1 is not None:
            src, o = (a1, b['o1']) if res else (ad, b['od'])
            aff = {}
        else:
            src, ss, o = (z1, ss1, b['o1']) if res else (zd, ssd, b['od'])
            aff = dict(scale=ss[0].data_ptr() + 4 * o, shift=ss[1].data_ptr() + 4 * o, act=p.act, slope=p.slope,
                       sstride=src.shape[-1] if per_sample else 0)
        # (the segment keeps `src` referenced: the buffer must outlive this function's caller until the launch that reads it is enqueued)
        segs.append(tconv.Segment(src, k, (k - 1) // 2, reflect and k > 1, b['p2off'], c4=b['w1'], cin=b['m'], xcs=src.shape[-1],
                                  ptr=src.data_ptr() + 4 * o, **aff))
    return segs


class Alloc:
    """A pipeline generator's request for the buffer of its next statistics exchange (n floats, n % 4 == 0).  A driver that runs several
    units in lockstep hands every unit of a round a slice of ONE arena, in unit order, so that the round's exchanges are one contiguous
    message: the collective runs on the arena itself, without the torch.cat / copy_ kernels a pack + unpack would launch."""
    __slots__ = ('n', 'device')

    def __init__(self, n, device):
        self.n, self.device = int(n), device


def slices(pairs):
    """(c0, c, norm module) per norm of a stage -> the finalize kernels' slice table.  Running-statistic pointers only for a BatchNorm2d in
    training mode with track_running_stats (never InstanceNorm2d); num_batches None for SynchronizedBatchNorm2d, whose forward bypasses
    _BatchNorm.forward and never advances num_batches_tracked (sync_batchnorm/batchnorm.py:68-101).  fused_spade.applicable admits a
    train-mode unit only if every norm is a BatchNorm2d with nm.training and nm.track_running_stats, so for those units the condition
    always holds and the pointers are the unconditional ones that path used to pass."""
    arr = (L.NSlice * len(pairs))()
    for i, (c0, c, bn) in enumerate(pairs):
        arr[i].c0, arr[i].c = c0, c
        track = isinstance(bn, cnn.BatchNorm2d) and bn.training and bn.track_running_stats
        if track:      # the finalize kernel this table goes to updates them in place: the folds derived from them re-fold (optim.weights_key)
            optim.note_stats_written(bn.running_mean, bn.running_var)
        arr[i].running_mean = bn.running_mean.data_ptr() if track else None
        arr[i].running_var = bn.running_var.data_ptr() if track else None
        arr[i].num_batches = bn.num_batches_tracked.data_ptr() if track and not isinstance(bn, cnn.SynchronizedBatchNorm2d) else None
    return arr


def finalize_g(p, part, scs, n, h, w, gamma, beta, pairs, *, sync, mstride=None):
    """-> (ss, mr): ss[0] / ss[1] = scale / shift [G][scs]; mr[0] / mr[1] = mean / rstd [G][mstride] (kept for the backward pass) of every
    norm of a stage, G = n for per-sample statistics.  `sync`: None, or the reducer of a SynchronizedBatchNorm over N > 1 ranks -- the
    caller's decision, never read here (an inception block under a data-parallel reducer keeps per-replica statistics).  With it the stage's
    statistics are exchanged ONCE: this rank's tile table -> [sum x | sum x^2] of the whole concatenation -> one all-reduce -> the
    reference's multi-replica formula (batchnorm.py:103-140: clamp(var, eps), unbiased running_var); mr then holds
    (a | b) = (inv_std | -mean * inv_std) for the split-phase backward.
    A GENERATOR: it yields an `Alloc` for the exchange buffer, then the buffer to be sum-reduced over the ranks, and continues once that
    has happened; without `sync` it yields nothing."""
    G = n if p.instance else 1
    mstride = scs if mstride is None else mstride
    gp, bp = (ops._p(gamma), ops._p(beta)) if p.affine else (None, None)
    if p.shards > 1 and not p.instance:
        # virtual replicas: one launch reduces per GROUP of samples (mr: [groups][mstride], what cat_norm_bwd with `shards` reads) and
        # writes the scale / shift rows per SAMPLE (ss: [n][scs]); running statistics from group 0
        if sync is not None:
            raise RuntimeError('fused unit: virtual replicas with a statistics exchange over ranks')
        per = ops.shard_bounds(n, p.shards)[0][1]
        ss = torch.empty((2, n, scs), device=part.device, dtype=torch.float32)
        mr = torch.empty((2, -(-n // per), mstride), device=part.device, dtype=torch.float32)
        L.call('cat_tnorm_finalize_groups', ops._p(part), scs, per, n, h, w, 8, 16, 1, gp, bp, len(pairs), slices(pairs), p.eps, p.momentum,
               ops._p(ss[0]), ops._p(ss[1]), ops._p(mr[0]), ops._p(mr[1]), mstride, ops._stream())
        return ss, mr
    ss = torch.empty((2, G, scs), device=part.device, dtype=torch.float32)
    mr = torch.empty((2, G, mstride), device=part.device, dtype=torch.float32)
    if sync is None:
        L.call('cat_tnorm_finalize', ops._p(part), scs, G, n, h, w, gp, bp, len(pairs), slices(pairs), p.eps, p.momentum, ops._p(ss[0]), ops._p(ss[1]),
               ops._p(mr[0]), ops._p(mr[1]), mstride, ops._stream())
        return ss, mr
    sums = yield Alloc(2 * scs, part.device)      # a slice of the round's arena under a lockstep driver: the merged exchange needs no pack / unpack
    L.call('cat_tnorm_sums', ops._p(part), scs, n, h, w, 8, 16, 1, ops._p(sums), ops._stream())
    yield sums
    count = float(n * h * w) * sync.world_size
    L.call('cat_tnorm_finalize_sums', ops._p(sums), count, scs, gp, bp, len(pairs), slices(pairs), p.eps, p.momentum, 1, ops._p(ss[0]), ops._p(ss[1]),
           ops._p(mr[0]), ops._p(mr[1]), ops._stream())
    return ss, mr


def drop_segs(p, djs, kind):
    key = ('o1', 'res') if kind == 'res' else ('od', 'dw')
    return [(b[key[0]], b['m'], b['j']) for b in p.branches if b['kind'] == key[1] and b['j'] in djs]


def materialise(p, z1, ss1, zd, ssd, drop, dw_slices):
    """A1 = act(norm(Z1)) with the res slices dropped (dw slices: written undropped iff dw_slices -- the backward pass's depthwise input
    gradient needs them, stage 2 does not) and Ad = act(norm(Zd)) dropped; one cat_dropout_apply launch each.  drop = (rate, {j of the
    branches whose Dropout is active}, ticket); every branch of the plan carries its Dropout index j."""
    pdrop, djs, ticket = drop
    n, h, w, _ = z1.shape
    dev, npix = z1.device, n * h * w
    sstride_of = lambda scs: scs if p.per_sample else 0
    a1 = torch.empty((n, h, w, p.hc1), device=dev, dtype=torch.float32)
    rest = dw_slices or any(b['j'] not in djs for b in p.res)      # (res slices whose Dropout is off are written too)
    g = ops.dropout_geom(npix, p.hc1, p.hc1, p.hc1, pdrop, drop_segs(p, djs, 'res'), mode=L.DROP_NORM, rest=int(rest), hw=h * w,
                         sstride=sstride_of(p.hc1), act=p.act, slope=p.slope)
    if p.res or dw_slices:
        ops.dropout_apply(g, z1, a1, ticket, ss1[0], ss1[1])
    ad = None
    if p.dws:
        ad = torch.empty((n, h, w, p.hcd), device=dev, dtype=torch.float32)
        g = ops.dropout_geom(npix, p.hcd, p.hcd, p.hcd, pdrop, drop_segs(p, djs, 'dw'), mode=L.DROP_NORM, rest=1, hw=h * w, sstride=sstride_of(p.hcd),
                             act=p.act, slope=p.slope)
        ops.dropout_apply(g, zd, ad, ticket, ssd[0], ssd[1])
    return a1, ad


def forward_g(p, x, *, sync=None, folded=None, drop=None):
    """The forward pipeline up to stage 2: stage 1 -> finalize -> depthwise stage -> finalize -> (dropout) -> the stage-2 segment list.
    -> (z1, st1, zd, std, segs) with st1 / std = (ss, mr) as finalize_g returns them (zd = std = None without depthwise branches); the
    caller launches stage 2 on `segs` with its own epilogue; the segments keep the buffers they read alive (with dropout: A1 / Ad, which
    are not returned), their scale / shift rows belong to st1 / std, which the caller holds until stage 2 is enqueued.  A generator over
    the statistics exchanges of finalize_g(sync=sync).
    folded = (ss1, ssd): the eval form -- scale / shift [2][hc] given (folded from the running statistics), so no statistics are
    collected and nothing is finalized (st1 / std = (ss, None)).
    drop = (rate, {j}, ticket): the stage-2 operands are materialised (normalise + activation + mask) -- res slices of act(norm(Z1)) into
    A1, all of act(norm(Zd)) into Ad -- and stage 2 stages them as they are."""
    n, c, h, w = x.shape
    dev = x.device
    tiles = n * ((h + 7) // 8) * ((w + 15) // 16)
    part_of = lambda hc: torch.empty((tiles, 2, hc), device=dev, dtype=torch.float32) if folded is None else None
    # ---- stage 1: first convs -> Z1 (pre-norm, concatenated) + tile statistics
    z1 = torch.empty((n, h, w, p.hc1), device=dev, dtype=torch.float32)
    part1 = part_of(p.hc1)
    stage1(p, x, z1, part1, p.reflect)
    if folded is None:
        st1 = yield from finalize_g(p, part1, p.hc1, n, h, w, p.gamma1, p.beta1, [(b['o1'], b['m'], b['bn1']) for b in p.branches], sync=sync)
    else:
        st1 = (folded[0], None)
    # ---- depthwise stage
    zd = std = None
    if p.dws:
        zd = torch.empty((n, h, w, p.hcd), device=dev, dtype=torch.float32)
        partd = part_of(p.hcd)
        dwm_fwd(p, z1, st1[0][0], st1[0][1], zd, partd, p.reflect, p.per_sample)
        if folded is None:
            std = yield from finalize_g(p, partd, p.hcd, n, h, w, p.gammad, p.betad, [(b['od'], b['m'], b['bn2']) for b in p.dws], sync=sync)
        else:
            std = (folded[1], None)
    a1 = ad = None
    if drop is not None:
        a1, ad = materialise(p, z1, st1[0], zd, std[0] if std is not None else None, drop, dw_slices=False)
    # ---- stage 2: the branch sum, K-concatenated, normalise + activation applied while staging
    segs = stage2_segs(p, z1, st1[0], zd, std[0] if std is not None else None, p.reflect, p.per_sample, a1, ad)
    return z1, st1, zd, std, segs


# ---------------------------------------------------------------------------------------------------------------- backward stages
def rematerialise(p, z, ss, per_sample=False):
    """act(z * scale + shift) of a whole hidden buffer [n, h, w, cs], written out: the backward pass's input of the second / depthwise convs."""
    n, h, w, cs = z.shape
    G = n if per_sample else 1
    a = torch.empty_like(z)
    L.call('cat_affine_res_fwd', ops._p(z), cs, ops._p(ss[0]), ops._p(ss[1]), cs if per_sample else 0, None, 0, ops._p(a), cs, G, (n // G) * h * w, cs,
           p.act, p.slope, ops._stream())
    return a


def norm_bwd_g(p, n, hw, c, cs, x, dy, gamma, beta, mr, act, slope, dgamma, dbeta, accumulate=0, sync=None):
    """Backward of (a concatenation of) train-mode norms + activation: -> dx, and d gamma / d beta into the given buffers.  `sync` None:
    one cat_norm_bwd.  `sync` a reducer (the forward saved (a | b) in mr): SynchronizedBatchNorm backward over ranks -- local
    [sum g | sum g * xhat] of the whole stage -> ONE all-reduce, requested from the driver like finalize_g's -> apply; the parameter
    gradients stay local sums (the gradient bucket all-reduce averages them), as in ops.SyncBNFn."""
    dx = torch.empty((n, hw, cs), device=x.device, dtype=torch.float32)
    if sync is not None:
        m = n * hw
        sums = yield Alloc(2 * cs, x.device)
        ws = ops.workspace(L.query('cat_bn_ws_bytes', m, cs), x.device)
        st = ops._stream()
        L.call('cat_bn_stats_bwd', ops._p(x), ops._p(dy), ops._p(gamma), ops._p(beta), ops._p(mr[0]), ops._p(mr[1]), m, c, cs, act, slope, ops._p(sums),
               ops._p(ws), st)
        local = sums.clone()
        yield sums
        L.call('cat_bn_apply_bwd', ops._p(x), ops._p(dy), ops._p(gamma), ops._p(beta), ops._p(mr[0]), ops._p(mr[1]), ops._p(sums),
               float(m * sync.world_size), ops._p(local), ops._p(dx), ops._p(dgamma), ops._p(dbeta), accumulate, m, c, cs, act, slope, st)
        return dx
    g = L.NormGeom(n, hw, c, cs, L.NORM_INSTANCE if p.instance else L.NORM_BATCH, p.eps, p.momentum, act, slope, 0 if p.instance else p.shards)
    ws = ops.workspace(L.query('cat_norm_ws_bytes', C.byref(g)), x.device)
    L.call('cat_norm_bwd', C.byref(g), ops._p(x), ops._p(dy), ops._p(gamma), ops._p(beta), ops._p(mr[0]), ops._p(mr[1]), ops._p(dx), ops._p(dgamma),
           ops._p(dbeta), accumulate, ops._p(ws), ops._stream())
    return dx


def channel_sum(src, m_pix, c, cs, dst):
    ws = ops.workspace(L.query('cat_channel_sum_ws_bytes', m_pix, cs), src.device)
    L.call('cat_channel_sum', ops._p(src), m_pix, c, cs, ops._p(dst), 0, ops._p(ws), ops._stream())


def wgrad(gw, xp, dyp, dst, acc, stream):
    """One cat_conv2d_wgrad launch: geometry gw, x / dy pointers, into dst (accumulated iff acc)."""
    ws = ops.workspace(L.query('cat_conv2d_wgrad_ws_bytes', C.byref(gw)), dst.device)
    L.call('cat_conv2d_wgrad', C.byref(gw), xp, dyp, ops._p(dst), acc, ops._p(ws), stream)


def dw_bwd(p, a1, da1, dzd, grads, reflect=False):
    """All depthwise convs, one launch per group of the plan: input gradient (reflect padding folded in the kernel) into the dw slices of
    dA1, filter gradients reduced straight into the parameters' gradient buffers (FusedAdam-owned) or into fresh tensors recorded in
    `grads`.  The sink is claimed ONCE for all branches; a launch gets its own branches' destinations, so every parameter is written
    (or accumulated into) by exactly one launch."""
    n, h, w, _ = a1.shape
    wts = [b['dconv'].weight for b in p.dws]
    sink = optim.claim(wts, f'{p.what} backward (depthwise)')
    dsts, acc_dw = sink or ([torch.empty_like(q) for q in wts], 0)
    dst_of = {id(b): d_ for b, d_ in zip(p.dws, dsts)}
    at = lambda t, off: C.c_void_p(t.data_ptr() + 4 * off)
    for group in p.dw_groups:
        bs, o, _ = group
        nb = len(bs)
        gd = dwm_geom(p, n, h, w, reflect, group)
        IA = C.c_int * nb
        wsd = ops.workspace(L.query(p.dw_ws_entry, C.byref(gd)), a1.device)
        L.call(p.dw_bwd_entry, C.byref(gd), at(a1, p.dw_in0 + o), at(dzd, o), at(p.w25, p.ft * o), at(da1, p.dw_in0 + o), p.hc1, nb,
               IA(*[b['od'] - o for b in bs]), IA(*[b['m'] for b in bs]), IA(*[b['kd'] for b in bs]),
               (C.c_void_p * nb)(*[dst_of[id(b)].data_ptr() for b in bs]), acc_dw, ops._p(wsd), ops._stream())
    for q, d_ in zip(wts, dsts):          # not all owned (tests): fresh tensors, copied / added into the views of those that are
        grads[id(q)] = None if sink is not None else optim.deliver(q, d_)


def dgrad1_segs(p, dz1, M=0):
    """The K segments of the first convs' input gradients (ONE K-concatenated launch over the slices of dZ1).  M: the reflect margin the
    output is computed with (0: 'same' zero padding)."""
    return [tconv.Segment(None, b['k'], M + (b['k'] - 1) // 2, False, b['d1off'], c4=b['w1'], cin=b['m'], xcs=p.hc1, ptr=dz1.data_ptr() + 4 * b['o1'])
            for b in p.branches]


def scatter_param_grads(p, grads):
    """Slices of the concatenated parameter-gradient vectors p.gv -> the parameters: one table-driven launch into the optimizer's gradient
    buffers when all targets are FusedAdam-owned, tensors recorded in `grads` (or copies into the owned views) otherwise."""
    dev = p.dev
    all_t = [q for _, _, _, q in p.targets] + [t2[5] for t2 in p.targets2d]
    sink = optim.claim(all_t, f'{p.what} backward')
    if sink is not None:
        views = tuple(gv.data_ptr() for gv in sink[0])
        if p.scatter_jobs is None or p.scatter_jobs[3] != views:
            dst = dict(zip(map(id, all_t), sink[0]))
            jobs = [dict(kind=3, srcs=[p.gv[v].data_ptr() + 4 * o, dst[id(q)].data_ptr()], nsrc=2, n=cnt, threads=cnt) for v, o, cnt, q in p.targets]
            # a one-channel conv weight is stored unpadded (wcs 1): never more columns than the destination row holds
            for v, o, rows, cols, sstr_, q in p.targets2d:
                wcs_q = ops._grad_wcs(dst[id(q)])
                cq = min(cols, wcs_q)
                jobs.append(dict(kind=4, srcs=[p.gv[v].data_ptr() + 4 * o, dst[id(q)].data_ptr()], nsrc=2, n=rows * cq, cs=cq, wn=sstr_,
                                 wcs=wcs_q, threads=rows * cq))
            p.scatter_jobs = p._jobs_to_dev(jobs) + (views,)
        tj, nj, nb, _ = p.scatter_jobs
        L.call('cat_prep_run', ops._p(tj), nj, nb, sink[1], ops._stream())
        grads.update((id(q), None) for q in all_t)
        return
    for v, o, cnt, q in p.targets:
        flat = p.gv[v][o:o + cnt]
        if q.dim() == 4:      # rows of a merged weight gradient: back into the parameter's [O][kh][kw][wcs] storage
            gq = ops.padded_weight_like(q.shape, dev)
            torch.as_strided(gq, (cnt,), (1,), gq.storage_offset()).copy_(flat)
        else:
            gq = flat.clone()
        grads[id(q)] = optim.deliver(q, gq)
    for v, o, rows, cols, sstr_, q in p.targets2d:
        gq = ops.padded_weight_like(q.shape, dev)
        cols = min(cols, ops.weight_wcs(gq))
        src2 = torch.as_strided(p.gv[v], (rows, cols), (sstr_, 1), o)
        torch.as_strided(gq, (rows, cols), (ops.weight_wcs(gq), 1), gq.storage_offset()).copy_(src2)
        grads[id(q)] = optim.deliver(q, gq)


def backward_g(p, dt, x, z1, ss1, mr1, zd, ssd, mrd, *, need_dx, skip_grad=None, drop=None, sync=None):
    """The backward pipeline: dT (the gradient of the branch sum, pixel stride p.cso) and what the forward saved -> (dx, grads), dx the
    input gradient (None unless need_dx) and grads {id(parameter): gradient tensor, or None where it was written into the optimizer's
    buffer}.  A generator over the statistics exchanges of norm_bwd_g(sync=sync).
    skip_grad: a skip connection's share of dx (an activation like x), added by the last launch.  drop = (rate, {j}, ticket): the
    forward's masks are re-derived from its ticket.  Weight-gradient launches are independent of the data-gradient chain: side-stream jobs
    with branch streams on; on one stream they run where they stand or, with p.wgrad_batch, back to back at the end of step 8 with their
    partial sums reduced by ONE launch (ops.WgradBatch)."""
    n, c, h, w = x.shape
    dev, hw, m_pix, xcs = x.device, h * w, n * h * w, ops.act_cs(x)
    st = ops._stream()
    grads = {}
    pad_mode = L.PAD_REFLECT if p.reflect else L.PAD_ZERO
    aff = lambda v: v if p.affine else None
    side = ops.SideJobs(dev)      # the temporaries its launches read (a1, ad, dt, dz1) stay referenced by this frame until side.join()
    batch = ops.WgradBatch(dev, grads) if p.wgrad_batch and not ops.branch_streams_enabled() else None

    def put_wgrad(param, make):      # make(dst) -> (geometry, x pointer, dy pointer)
        if batch is not None:
            return batch.add(param, make)

        def job():
            grads[id(param)] = ops._write_param_grad(param, lambda dst_, acc: wgrad(*make(dst_), dst_, acc, ops._stream()))
        side.run(job)

    def put_wgrad_into(dst, geom, xp, dyp):      # merged launches: destination = a gradient view of the plan, overwritten
        if batch is not None:
            return batch.add_into(dst, 0, geom, xp, dyp)
        side.run(lambda: wgrad(geom, xp, dyp, dst, 0, ops._stream()))

    # ---- 1. re-materialise the hidden activations (inputs of the second convs / of the depthwise convs); with dropout the forward's
    # masks are re-derived from its ticket: res slices of A1 and all of Ad dropped, the dw slices of A1 (depthwise inputs) not
    a1, ad = materialise(p, z1, ss1, zd, ssd, drop, dw_slices=True) if drop is not None else (rematerialise(p, z1, ss1, p.per_sample), None)
    da1 = torch.empty((n, h, w, p.hc1), device=dev, dtype=torch.float32)
    dad = None
    if p.dws:
        if drop is None:
            ad = rematerialise(p, zd, ssd, p.per_sample)
        dad = torch.empty((n, h, w, p.hcd), device=dev, dtype=torch.float32)
    # ---- 2. / 3. second convs: weight gradients from (hidden activation slice, dT); input gradients into slices of dA1 / dAd
    side.fork()
    for b in p.branches:
        res = b['kind'] == 'res'
        k2, m, w1 = b['k2'], b['m'], b['w1']
        pad2 = (k2 - 1) // 2
        src, scs_, o = (a1, p.hc1, b['o1']) if res else (ad, p.hcd, b['od'])
        dst, dcs = (da1, p.hc1) if res else (dad, p.hcd)
        xptr = C.c_void_p(src.data_ptr() + 4 * o)
        mode2 = pad_mode if pad2 > 0 else L.PAD_ZERO

        def kw(dst_, xptr=xptr, m=m, scs_=scs_, k2=k2, pad2=pad2, mode2=mode2):
            return ops._conv_geom(n, h, w, m, scs_, h, w, p.Cout, p.cso, k2, k2, 1, pad2, mode2, wcs=ops._grad_wcs(dst_)), xptr, ops._p(dt)
        if res or not p.merge2:
            put_wgrad(b['conv2'].weight, kw)
        if (not res and p.dpack2_dw is not None) or any(b is r for r in (p.s1d or ()) + (p.s1d7 or ())):
            continue            # input gradient: the merged launch below
        seg_pad = k2 - 1 - (0 if mode2 == L.PAD_REFLECT else pad2)
        seg = tconv.Segment(None, k2, seg_pad, False, b['d2off'], c4=p.cso, cin=p.Cout, xcs=p.cso, ptr=dt.data_ptr())
        if mode2 == L.PAD_REFLECT:
            dxp = torch.empty((n, h + 2 * pad2, w + 2 * pad2, w1), device=dev, dtype=torch.float32)
            tconv.run([seg], p.dpack2, None, dxp, m, n, h, w, h + 2 * pad2, w + 2 * pad2, ycs=w1, ycw=w1, yptr=dxp.data_ptr())
            L.call('cat_reflect_pad_bwd2', ops._p(dxp), w1, C.c_void_p(dst.data_ptr() + 4 * o), dcs, None, 0, n, h, w, w1, pad2, st)
        else:
            tconv.run([seg], p.dpack2, None, None, m, n, h, w, h, w, ycs=dcs, ycw=w1, yptr=dst.data_ptr() + 4 * o)
    # ---- 4. merged second-conv input gradients: dT staged once for the 5 x 5 and the 3 x 3 residual branch and the N-concatenated 1 x 1
    # second convs of the depthwise branches (p.s1d; p.s1d7: and the 7 x 7 one), or those 1 x 1 convs alone as ONE launch over dT into dAd
    nvalid_dw = sum(b['m'] for b in p.dws)
    s1d = [(getattr(p, attr), geom, entry) for entry, _, _, geom, attr in STAGE1_DGRAD if getattr(p, attr) is not None]
    if s1d:
        rs, geom, entry = s1d[0]
        ns = len(rs) + 1
        gs = geom()
        gs.N, gs.H, gs.W, gs.xcs, gs.cin, gs.reflect, gs.ycs, gs.scs = n, h, w, p.cso, p.Cout, 0, 0, 0
        packs, dxs, dxcs = (C.c_void_p * ns)(), (C.c_void_p * ns)(), (C.c_int * ns)(*([p.hc1] * len(rs) + [p.hcd]))
        slots = [(r['o1'], r['w1'], r['m'], p.dpack2.data_ptr() + 4 * r['d2off'], da1) for r in rs] + [(0, p.hcd, nvalid_dw, p.dpack2_dw.data_ptr(), dad)]
        for slot, (col0, width, nvalid, pk, dst) in enumerate(slots):
            gs.col0[slot], gs.width[slot], gs.nvalid[slot] = col0, width, nvalid
            packs[slot], dxs[slot] = pk, dst.data_ptr()
        L.call(entry, C.byref(gs), ops._p(dt), packs, dxs, dxcs, ops._stream())
    elif p.dws and p.dpack2_dw is not None:
        seg = tconv.Segment(None, 1, 0, False, 0, c4=p.cso, cin=p.Cout, xcs=p.cso, ptr=dt.data_ptr())
        tconv.run([seg], p.dpack2_dw, None, None, p.hcd, n, h, w, h, w, ycs=p.hcd, ycw=p.hcd, yptr=dad.data_ptr(), nvalid=nvalid_dw)
    if drop is not None:      # gradients of the dropped activations -> of the activations: x keep * s (in place, before the norms)
        for kind, d_, hc in (('res', da1, p.hc1), ('dw', dad, p.hcd)):
            segs_k = drop_segs(p, drop[1], kind)
            if segs_k:
                ops.dropout_apply(ops.dropout_geom(m_pix, hc, hc, hc, drop[0], segs_k, rest=0), d_, d_, drop[2])
    # ---- 5. d W2 of all depthwise branches: dT^T x Ad as ONE 1x1 weight-gradient launch over the concatenated hidden buffer; d bias2
    if p.merge2:
        put_wgrad_into(p.gv['w2'], ops._conv_geom(n, h, w, p.hcd, p.hcd, h, w, p.Cout, p.cso, 1, 1, 1, 0, L.PAD_ZERO, wcs=p.hcd), ops._p(ad), ops._p(dt))
    if p.has_bias2:
        channel_sum(dt, m_pix, p.Cout, p.cso, p.gv['c2'])
    # ---- 6. depthwise stage
    if p.dws:
        dzd = yield from norm_bwd_g(p, n, hw, p.hcd, p.hcd, zd, dad, aff(p.gammad), aff(p.betad), mrd, p.act, p.slope, aff(p.gv['gd']), aff(p.gv['bd']),
                                    sync=sync)
        if p.has_biasd:
            channel_sum(dzd, m_pix, p.hcd, p.hcd, p.gv['cd'])
        dw_bwd(p, a1, da1, dzd, grads, p.reflect)
    # ---- 7. stage-1 norms (all branches at once)
    dz1 = yield from norm_bwd_g(p, n, hw, p.hc1, p.hc1, z1, da1, aff(p.gamma1), aff(p.beta1), mr1, p.act, p.slope, aff(p.gv['g1']), aff(p.gv['b1']),
                                sync=sync)
    if p.has_bias1:
        channel_sum(dz1, m_pix, p.hc1, p.hc1, p.gv['c1'])
    # ---- 8. first convs: weight gradients from (x, dZ1 slice)
    side.refork()
    if p.merge1 is not None:
        g1 = p.merge1
        put_wgrad_into(p.gv['w1'], ops._conv_geom(n, h, w, c, xcs, h, w, g1['width'], p.hc1, 1, 1, 1, 0, L.PAD_ZERO, wcs=p.csi), ops._p(x),
                       C.c_void_p(dz1.data_ptr() + 4 * g1['off']))
    for b in p.branches:
        if p.merge1 is not None and b['k'] == 1:
            continue
        k, m = b['k'], b['m']
        pad1 = (k - 1) // 2
        mode1 = pad_mode if pad1 > 0 else L.PAD_ZERO
        dyp = C.c_void_p(dz1.data_ptr() + 4 * b['o1'])

        def kw1(dst_, dyp=dyp, m=m, k=k, pad1=pad1, mode1=mode1):
            return ops._conv_geom(n, h, w, c, xcs, h, w, m, p.hc1, k, k, 1, pad1, mode1, wcs=ops._grad_wcs(dst_)), ops._p(x), dyp
        put_wgrad(b['conv1'].weight, kw1)
    if batch is not None:
        batch.flush()
    # ---- 9. first convs: the input gradients as ONE K-concatenated launch (+ the skip connection's share)
    dx = None
    if need_dx:
        M = max((b['k'] - 1) // 2 for b in p.branches) if p.reflect else 0
        segs = dgrad1_segs(p, dz1, M)
        dx = ops.empty_act(n, c, h, w, dev)
        if M:
            dxp = torch.empty((n, h + 2 * M, w + 2 * M, p.csi), device=dev, dtype=torch.float32)
            tconv.run(segs, p.dpack1, None, dxp, c, n, h, w, h + 2 * M, w + 2 * M, ycs=p.csi, ycw=p.csi, yptr=dxp.data_ptr())
            L.call('cat_reflect_pad_bwd2', ops._p(dxp), p.csi, ops._p(dx), ops.act_cs(dx), ops._p(skip_grad),
                   ops.act_cs(skip_grad) if skip_grad is not None else 0, n, h, w, p.csi, M, st)
        else:
            tconv.run(segs, p.dpack1, None, dx, c, n, h, w, h, w, res=skip_grad)
    side.join()
    # ---- 10. scatter the concatenated parameter gradients
    scatter_param_grads(p, grads)
    return dx, grads
