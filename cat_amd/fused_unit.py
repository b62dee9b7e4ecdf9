"""What the fused inception block (cat_amd/fused_block.py) and the fused six-branch SPADE unit (cat_amd/fused_spade.py) share: one protocol

    stage 1   first convs of all branches -> one concatenated pre-norm buffer Z1 + per-tile statistics   (cat_tstage1_fwd / cat_tconv_fwd)
    dw        all depthwise convs as one launch, norm + activation of stage 1 applied while staging      (cat_dwm_fwd)
    stage 2   the branch sum: the second convs K-concatenated, norm + activation applied while staging   (cat_tconv_fwd)

over one static layout.  `Plan` is that layout -- channel slices, kernel-size groups, persistent operand buffers, the table-driven operand
preparation (cat_prep_run) and the concatenated parameter-gradient vectors with their scatter targets; the functions below it are the
stages, forward and backward, each defined once.  The two callers keep what is theirs: how the norms are finalised (the block's closing
pw_bn, InstanceNorm and reflect padding; the unit's statistics exchanges over ranks), dropout, and the autograd Functions."""
import ctypes as C

import torch

from . import _lib as L
from . import ops
from . import optim
from . import tconv


def cs4(c):
    return (c + 3) // 4 * 4


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
    branches' 1 x 1 second convs get an N-concatenated input-gradient filter stream (`dpack2_dw`)."""
    what = 'fused unit'
    GAMMA0 = 0.0

    def __init__(self, res, dws, cin, cout, dev, params):
        self.dev = dev
        self.params = params
        self.Cin, self.csi = cin, cs4(cin)
        self.Cout, self.cso = cout, cs4(cout)
        # stage-1 channel order: [res k=1 | dw ... | res k=3 | res k=5] so that same-kernel first convs are adjacent (N concat) and the
        # depthwise inputs are one contiguous slice range
        order = [b for b in res if b['k'] == 1] + dws + [b for b in res if b['k'] == 3] + [b for b in res if b['k'] == 5]
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
        self.branches, self.res, self.dws = order, res, dws
        # stage-1 launches: one per first-conv kernel size
        self.groups = []
        for k in (1, 3, 5):
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
        self.w25 = z(25 * max(self.hcd, 4))
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
            fwd.append(dict(kind=2, srcs=[wd.data_ptr()], dst=self.w25.data_ptr(), Nn=b['m'], ks=kd, col0=b['od'], cs=self.hcd, threads=b['m'] * kd * kd))
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
    plans = [getattr(b, '_cat_fused_plan', None) for b in blocks]
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
    statistics (always one launch per kernel size)."""
    n, c, h, w = x.shape
    by_k = {g['k']: g for g in p.groups}
    if part1 is not None and len(p.groups) == 3 and L.query('cat_tstage1_supported', by_k[5]['width'], by_k[3]['width'], by_k[1]['width']):
        # one launch: the three kernel sizes share every staged input tile
        gs = L.Stage1Geom()
        gs.N, gs.H, gs.W, gs.xcs, gs.cin, gs.reflect, gs.ycs, gs.scs = n, h, w, ops.act_cs(x), c, int(reflect), p.hc1, p.hc1
        packs = (C.c_void_p * 3)()
        for slot, k in enumerate((5, 3, 1)):
            g = by_k[k]
            gs.col0[slot], gs.width[slot], gs.nvalid[slot] = g['off'], g['width'], sum(b['m'] for b in g['branches'])
            packs[slot] = g['pack'].data_ptr()
        L.call('cat_tstage1_fwd', C.byref(gs), ops._p(x), packs, ops._p(p.bias1) if p.has_bias1 else None, ops._p(z1), ops._p(part1), ops._stream())
        return
    for g in p.groups:
        pad = (g['k'] - 1) // 2
        seg = tconv.Segment(x, g['k'], pad, reflect and pad > 0, 0)
        stats = dict(stats=part1.data_ptr() + 4 * g['off'], scs=p.hc1) if part1 is not None else {}
        tconv.run([seg], g['pack'], (p.bias1.data_ptr() + 4 * g['off']) if p.has_bias1 else None, None, g['width'], n, h, w, h, w, ycs=p.hc1,
                  ycw=g['width'], yptr=z1.data_ptr() + 4 * g['off'], nvalid=sum(b['m'] for b in g['branches']), **stats)


def dwm_geom(p, n, h, w, reflect):
    gd = L.DwmGeom()
    gd.N, gd.H, gd.W, gd.nq, gd.xcs, gd.ycs, gd.scs, gd.reflect = n, h, w, p.hcd // 4, p.hc1, p.hcd, p.hcd, int(reflect)
    for b in p.dws:
        for q in range(b['od'] // 4, (b['od'] + cs4(b['m'])) // 4):
            gd.ks[q] = b['kd']
    return gd


def dwm_fwd(p, z1, scale, shift, zd, partd, reflect=False, per_sample=False):
    """All depthwise convs as one launch: act(Z1 * scale + shift) of the dw slices, applied while staging, -> Zd (+ tile statistics into
    partd unless None).  per_sample: scale / shift are [n][hc1] (InstanceNorm) instead of one row."""
    n, h, w, _ = z1.shape
    gd = dwm_geom(p, n, h, w, reflect)
    gd.sstride, gd.act, gd.slope = (p.hc1 if per_sample else 0), p.act, p.slope
    o = 4 * p.dw_in0
    L.call('cat_dwm_fwd', C.byref(gd), C.c_void_p(z1.data_ptr() + o), C.c_void_p(scale.data_ptr() + o), C.c_void_p(shift.data_ptr() + o), ops._p(p.w25),
           ops._p(p.biasd) if p.has_biasd else None, ops._p(zd), ops._p(partd), ops._stream())


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
        segs.append(tconv.Segment(None, k, (k - 1) // 2, reflect and k > 1, b['p2off'], c4=b['w1'], cin=b['m'], xcs=src.shape[-1],
                                  ptr=src.data_ptr() + 4 * o, **aff))
    return segs


# ---------------------------------------------------------------------------------------------------------------- backward stages
def rematerialise(p, z, ss, per_sample=False):
    """act(z * scale + shift) of a whole hidden buffer [n, h, w, cs], written out: the backward pass's input of the second / depthwise convs."""
    n, h, w, cs = z.shape
    G = n if per_sample else 1
    a = torch.empty_like(z)
    L.call('cat_affine_res_fwd', ops._p(z), cs, ops._p(ss[0]), ops._p(ss[1]), cs if per_sample else 0, None, 0, ops._p(a), cs, G, (n // G) * h * w, cs,
           p.act, p.slope, ops._stream())
    return a


def channel_sum(src, m_pix, c, cs, dst):
    ws = ops.workspace(L.query('cat_channel_sum_ws_bytes', m_pix, cs), src.device)
    L.call('cat_channel_sum', ops._p(src), m_pix, c, cs, ops._p(dst), 0, ops._p(ws), ops._stream())


def wgrad(gw, xp, dyp, dst, acc, stream):
    """One cat_conv2d_wgrad launch: geometry gw, x / dy pointers, into dst (accumulated iff acc)."""
    ws = ops.workspace(L.query('cat_conv2d_wgrad_ws_bytes', C.byref(gw)), dst.device)
    L.call('cat_conv2d_wgrad', C.byref(gw), xp, dyp, ops._p(dst), acc, ops._p(ws), stream)


def dw_bwd(p, a1, da1, dzd, grads, reflect=False):
    """All depthwise convs at once: input gradient (reflect padding folded in the kernel) into the dw slices of dA1, filter gradients reduced
    straight into the parameters' gradient buffers (FusedAdam-owned) or into fresh tensors recorded in `grads`."""
    n, h, w, _ = a1.shape
    nb = len(p.dws)
    gd = dwm_geom(p, n, h, w, reflect)
    wts = [b['dconv'].weight for b in p.dws]
    sink = optim.claim(wts, f'{p.what} backward (depthwise)')
    dsts, acc_dw = sink or ([torch.empty_like(q) for q in wts], 0)
    IA = C.c_int * nb
    wsd = ops.workspace(L.query('cat_dwm_bwd_ws_bytes', C.byref(gd)), a1.device)
    L.call('cat_dwm_bwd', C.byref(gd), C.c_void_p(a1.data_ptr() + 4 * p.dw_in0), ops._p(dzd), ops._p(p.w25),
           C.c_void_p(da1.data_ptr() + 4 * p.dw_in0), p.hc1, nb, IA(*[b['od'] for b in p.dws]), IA(*[b['m'] for b in p.dws]),
           IA(*[b['kd'] for b in p.dws]), (C.c_void_p * nb)(*[d_.data_ptr() for d_ in dsts]), acc_dw, ops._p(wsd), ops._stream())
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
