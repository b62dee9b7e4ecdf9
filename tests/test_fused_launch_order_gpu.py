"""GPU: the launch sequence of the fused inception block (cat_amd/fused_block.py) and the fused six-branch SPADE unit (cat_amd/fused_spade.py),
pinned.  Both run through the one pipeline of cat_amd/fused_unit.py; which launches it issues, in which order and on which stream depends on
plan properties and arguments (padding, norm kind, merged gradients, dropout, weight-gradient batching, statistics exchanges over ranks).
Each case below takes a different arm.  One forward + backward of a single module runs with `cat_amd._lib.call` wrapped; per call the
entry-point name and whether its stream argument is the main stream ("m") or a side stream ("s") are recorded, and the list must equal
tests/golden/fused_launch_order.json, which was recorded with this file at the commit before the two callers were moved onto one pipeline
(`record_case` is what a recording script calls).  Statistics exchanges appear as "exchange" entries; a case under a reducer ends with the
number of collectives fused_spade counted."""
import functools
import json
import os
from argparse import Namespace

import pytest
import torch

from oracle import detfill

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fused_launch_order.json')
N, H, W = 2, 16, 32      # 2 x 2 tiles of 8 x 16 per image
C = 40


class _Recorder:
    """Wraps cat_amd._lib.call (every module reaches it as an attribute of _lib) while active."""

    def __init__(self):
        from cat_amd import _lib
        _lib.load()
        self.lib, self.calls = _lib, []

    def __enter__(self):
        main = torch.cuda.current_stream().cuda_stream
        real = self.real = self.lib.call

        def call(name, *args):
            stream = getattr(args[-1], 'value', args[-1])      # the stream is every entry point's last argument
            self.calls.append([name, 'm' if (stream or 0) == main else 's'])
            return real(name, *args)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.real


class _TwoIdenticalRanks:
    """What ops.set_bn_sync expects of a reducer; the other rank holds the same shard: sums double."""
    world_size = 2

    def __init__(self, calls):
        self.calls = calls

    def all_reduce_sum_(self, t):
        self.calls.append('exchange')
        return t.mul_(2.0)


def _names(calls):
    return [c[0] for c in calls if c != 'exchange']


def _block_case(norm='batch', padding='reflect', res=(7, 6, 9), dw=(16, 5, 0), streams=False, drop=0.0, owned=False):
    from test_fused_block_gpu import _block
    from cat_amd import fused_block, nn as cnn, ops, rng
    dev = torch.device('cuda:0')
    blk = _block(norm, dev, C, res, dw, padding)
    if drop:
        blk.dropout_rate = drop
        for m in blk.modules():
            if isinstance(m, cnn.Dropout):
                m.p = drop
        rng.set_state(77, 50, dev)
    if owned:
        from cat_amd.optim import FusedAdam
        FusedAdam(list(blk.parameters()), lr=0.0).zero_grad()
    x = ops.to_nhwc(detfill.normal((N, C, H, W), 5).to(dev)).detach().requires_grad_(True)
    gy = ops.to_nhwc(detfill.normal((N, C, H, W), 6).to(dev))
    rec = _Recorder()
    was, old = ops.branch_streams_enabled(), ops.set_tconv_min_tiles(1)
    ops.set_branch_streams(streams)
    try:
        assert fused_block.applicable(blk, x)
        with rec:
            blk(x).backward(gy)
            torch.cuda.synchronize()
    finally:
        ops.set_branch_streams(was)
        ops.set_tconv_min_tiles(old)
    p = blk._cat_fused_plan
    names = _names(rec.calls)
    ndw = sum(1 for m in dw if m)
    # the arms the case is here for
    assert (p.merge1 is not None) == (ndw + (res[0] > 0) > 1) and p.merge2 == (ndw > 1) and (p.dpack2_dw is not None) == (ndw > 1)
    assert ('cat_conv2d_wgrad_batch' in names) == (not streams) and ('cat_conv2d_wgrad' in names) == streams
    assert any(c[1] == 's' for c in rec.calls) == streams
    assert ('cat_dropout_apply' in names) == bool(drop) and ('cat_dwm_bwd' in names) == (ndw > 0)
    assert (names.count('cat_prep_run') == 3) == owned      # forward operands, backward operands, the gradient scatter
    return rec.calls


@functools.lru_cache(maxsize=None)
def _spade_opt():
    from test_spade_gpu import fixture
    return fixture()[1]


def _unit_case(fin, fout, channels, streams, mode='train', synced=False):
    from test_spade_gpu import nhwc
    from cat_amd import _lib, fused_spade, ops
    from cat_amd.inception_modules import SPADEInvertedResidualChannels
    o = Namespace(**vars(_spade_opt()))
    o.norm_G, o.channels = 'spadesyncbatch3x3', channels
    blk = SPADEInvertedResidualChannels(fin, fout, o)
    blk.load_state_dict(detfill.fill_state_dict(blk.state_dict(), 411, gamma_abs_normal=True))
    blk = blk.to(torch.device('cuda:0')).train(mode == 'train')
    x = detfill.normal((N, fin, H, W), 600)
    seg = (detfill.normal((N, o.semantic_nc, H // 4, W // 4), 413) > 0.8).float().repeat_interleave(4, 2).repeat_interleave(4, 3)
    gy = nhwc(detfill.normal((N, fout, H, W), 414))
    xa, sa = nhwc(x).detach().requires_grad_(mode == 'train'), nhwc(seg)
    rec = _Recorder()
    was, old = ops.branch_streams_enabled(), ops.set_tconv_min_tiles(1)
    ops.set_branch_streams(streams)
    ops.set_bn_sync(_TwoIdenticalRanks(rec.calls) if synced else None)
    before = dict(fused_spade.STATS)
    try:
        with torch.set_grad_enabled(mode == 'train'):
            assert fused_spade.applicable(blk.res_ops, blk.dw_ops, xa, mode == 'train')
            with rec:
                y = blk(xa, sa)
                if mode == 'train':
                    y.backward(gy)
                torch.cuda.synchronize()
    finally:
        ops.set_bn_sync(None)
        ops.set_branch_streams(was)
        ops.set_tconv_min_tiles(old)
    plans = fused_spade.units_of(blk)      # the main unit and the gamma|beta net of every SPADE layer of the block
    assert blk._cat_fused_main in plans and len(plans) >= 2
    names = _names(rec.calls)
    ran = {k: fused_spade.STATS[k] - before[k] for k in before}
    # which arm each plan took: the one-launch second-conv input gradient where the kernel exists for the plan's widths, and only there
    for p in plans:
        r5, r3 = [b for b in p.res if b['k'] == 5], [b for b in p.res if b['k'] == 3]
        want = len(r5) == 1 and len(r3) == 1 and bool(p.dws) and bool(_lib.query('cat_tstage1_dgrad_supported', r5[0]['w1'], r3[0]['w1'], p.hcd))
        assert (p.s1d is not None) == want and (p.dpack2_dw is not None) == want
    if mode == 'train':
        assert ran['train_fwd'] == ran['bwd'] == len(plans) and ran['frozen_fwd'] == 0
        assert names.count('cat_tstage1_dgrad') == sum(p.s1d is not None for p in plans)
        assert 'cat_conv2d_wgrad_batch' not in names      # the unit's weight gradients are not batched, with or without branch streams
        assert any(c[1] == 's' for c in rec.calls) == streams
    else:
        assert ran['frozen_fwd'] == len(plans) and ran['train_fwd'] == 0 and 'cat_tnorm_finalize' not in names
    assert (ran['collectives'] > 0) == synced and ('cat_tnorm_finalize_sums' in names) == synced and ('cat_bn_apply_bwd' in names) == synced
    return rec.calls + (['collectives:%d' % ran['collectives']] if synced else [])


CASES = {
    'block-batch-reflect-one-stream': lambda: _block_case(),
    'block-batch-reflect-branch-streams': lambda: _block_case(streams=True),
    'block-instance-zero': lambda: _block_case(norm='instance', padding='zero'),
    'block-single-res-branch': lambda: _block_case(res=(0, 6, 0), dw=(0, 0, 0)),
    'block-dropout': lambda: _block_case(drop=0.5),
    'block-owned-parameters': lambda: _block_case(owned=True),
    'unit-48-24-shortcut': lambda: _unit_case(48, 24, None, streams=True),
    'unit-40-16-pruned': lambda: _unit_case(40, 16, [30, 6, 12], streams=False),
    'unit-24-24-eval': lambda: _unit_case(24, 24, None, streams=True, mode='eval'),
    'unit-40-16-two-ranks': lambda: _unit_case(40, 16, [30, 6, 12], streams=True, synced=True),
}


def record_case(name):
    """The recorded list of one case (what the golden holds under `name`)."""
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_holds_exactly_the_cases():
    assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize('name', sorted(CASES))
def test_fused_launch_order(name):
    got, want = record_case(name), _golden()[name]
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    assert got == want, (len(got), len(want), first, got[first:first + 3], want[first:first + 3])
