"""The layout, pointwise, concat / slice, fill / axpy and replicate-pad kernels of csrc/elementwise.hip (everything in that file that is neither a
reduction nor the optimiser step; those are in test_streaming_kernels_gpu.py) through the C ABI against plain float64 torch on the host, at
their tile and grid edges.  Every other GPU test uploads through cat_nchw_to_nhwc and reads back through cat_nhwc_to_nchw: here the two are
held to `permute`, each on its own, so an error symmetric between them cannot cancel.

A (host): a coverage test over the case tables (ew_grid: under, at and over the cap of 8192 workgroups for every grid-stride kernel; the
          transposes' grid (cdiv(HW, 64), cdiv(cs, 64), N): 1, 2 and 3 tiles on both axes; the cs == 4 fast path taken and declined); the float32
          ATen twin of every reference that is not held exactly within a tenth of its bar; the copies of frozen._build_plan.
B (GPU):  cat_nchw_to_nhwc / cat_nhwc_to_nchw: tile edges, a stride wider than cs4(C), the one-lane-per-pixel path of cs == 4 and its fallback
          to the tile kernel when y is not 16-byte aligned, the grid-stride trip.
C (GPU):  cat_act_fwd / cat_act_bwd: all five codes on and beside their bounds, the size ladder, in place, n % 4 refused.
D (GPU):  cat_concat2 / cat_slice_channels: unequal strides, c0 % 4 != 0, the two halves of a 2N destination, the in-place-width form of
          frozen.py; the frozen block with two k = 1 residual branches (one copy of the whole residual range: a copy per slot wrote past h2).
E (GPU):  cat_fill, cat_axpy, cat_add_n with dst == srcs[0].
F (GPU):  cat_replicate_pad_fwd / _bwd: wide stride, pad == 0, pad > H, W == 1, the grid-stride trip; the gradient per border class.

Bars: exact equality wherever a kernel moves, selects or does one correctly rounded operation (B, D, cat_fill, F forward, C except TANH, cat_axpy
for a in {0, 1, -0.5}); rel() of test_kernels_gpu.py < 1e-6 for TANH, cat_axpy and cat_replicate_pad_bwd (the 1e-6 class of LOSS_BAR / ADAM_BAR /
ADDN_BAR and test_replication_pad), each reachable: the float32 twin is within 1e-7 of float64 on the host (two pad cases: PAD_BARS).  Fresh-write destinations start as
NaN, everything a kernel must not touch as the sentinel 7.0, 64 sentinels behind every buffer.  Out-of-contract arguments are only ever refused
(non-zero return, destination untouched), never launched.  Largest distances observed on an MI355X: C (TANH, forward and backward) 7.3e-8,
E (cat_axpy) 5.9e-8, F (cat_replicate_pad_bwd) 1.2e-7 (the float32 twin's own distance); the frozen block with two k = 1 residual branches
1.7e-7 from its float64 twin."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_kernels_gpu import rel
from test_streaming_kernels_gpu import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_RELU6, ACT_TANH, ADDN_SMALL, MAXREL, NAN, SENTINEL, SLOPE, _cmp, _host,
                                        _in, _lib, _out, _p, _same, _stream, _tail, cdiv, cs4, ew_grid)

CAP = 8192                        # kEwCap of csrc/elementwise.hip: workgroups of 256 lanes
AT = CAP * 256                    # items that fill the capped grid exactly once
OVER = CAP * 256 + 1000           # ... and a ragged second trip
ACTS = (ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH, ACT_RELU6)
# the 1e-6 class of LOSS_BAR / ADAM_BAR / ADDN_BAR; the float32 twins (torch.tanh, y + a * x, the autograd of F.pad) are within 1e-7 of
# float64 on the host (test_fp32_twin_of_every_reference_is_within_a_tenth_of_the_bar): tanh 7.2e-8, axpy 5.9e-8, the pad's gradient up to
# 9.8e-8 -- except for the two pad cases of PAD_BARS
TANH_BAR = AXPY_BAR = PAD_BAR = 1e-6
BLOCK_BAR = 1e-3                  # the project's bar for whole blocks (test_frozen_k7_gpu.py)


def _pattern(n, mul=1, mod=8191):
    """cheap, exactly representable and position dependent: every misplaced element is identifiable"""
    return ((torch.arange(n, dtype=torch.int64) * mul) % mod).to(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _refused(L, name, flat, *args):
    """an out-of-contract call: a non-zero return, the sentinel destination untouched"""
    rc = L.query(name, *args)
    torch.cuda.synchronize()
    assert rc != 0, (name, 'accepted')
    assert bool((flat == SENTINEL).all()), (name, 'a refused call wrote')


# ================================================================================================ case tables
# B: (N, C, H, W, cs); non-square planes: H and W cannot be swapped unnoticed
LAYOUT_TILE = ([(1 + 2 * (i % 2), c, 5, 13, cs4(c)) for i, c in enumerate((1, 5, 63, 64, 65, 130))]                    # every C edge at HW = 65
               + [(3 - 2 * (i % 2), 65, h, w, 68) for i, (h, w) in enumerate(((1, 1), (7, 9), (4, 16), (3, 43)))]       # every HW edge at C = 65
               + [(3, 130, 3, 43, 132)])
LAYOUT_WIDE = [(2, 62, 5, 13, 68),      # the padding lanes straddle the channel-tile boundary, the second channel tile is padding only
               (2, 3, 5, 13, 8)]
LAYOUT_FAST = [(3, c, h, w, 4) for c in (1, 2, 3, 4) for h, w in ((1, 1), (5, 13))]
LAYOUT_LARGE = [(1, 3, 1024, 2048, 4),      # N * HW == 8192 * 256: the capped grid exactly once
                (1, 3, 1288, 1629, 4)]      # HW == 8192 * 256 + 1000: the grid-stride trip of the fast path
LAYOUT_CASES = LAYOUT_TILE + LAYOUT_WIDE + LAYOUT_FAST + LAYOUT_LARGE


def layout_grid(case, to_nhwc):
    """the grid of the tile transposes: (cdiv(HW, 64), cdiv(cs, 64), N) to NHWC, (cdiv(HW, 64), cdiv(C, 64), N) back"""
    n, c, h, w, cs = case
    return cdiv(h * w, 64), cdiv(cs if to_nhwc else c, 64), n


def fast_path(case, aligned=True):
    """cat_nchw_to_nhwc: one lane per pixel for a 4-wide, 16-byte aligned destination"""
    return case[4] == 4 and aligned


# C: n of cat_act_fwd / cat_act_bwd (floats; the kernels walk n / 4 quads)
ACT_NS = (4, 4 * 255, 4 * 256, 4 * 257, 4 * OVER)
ACT_AT = (ACT_LRELU, 4 * AT)      # the capped grid exactly once: one code is enough, the walk is the same for all
_F32 = lambda v: np.float32(v)
_NA = lambda v, to: np.nextafter(np.float32(v), np.float32(to), dtype=np.float32)
ACT_EDGES = [_F32(v) for v in (0.0, -0.0, 6.0, _NA(6, np.inf), _NA(6, -np.inf), _NA(0, np.inf), _NA(0, -np.inf), 1e-30, -1e-30, 20.0, -20.0, 88.0,
                               -88.0, 1.0, -1.0, 3.0, -6.0, _NA(1, -np.inf), _NA(-1, np.inf), 0.5)]
E_ZERO, E_SIX, E_SIX_UP, E_SIX_DOWN, E_ZERO_UP, E_ZERO_DOWN, E_ONE = 0, 2, 3, 4, 5, 6, 13      # positions in ACT_EDGES
assert len(ACT_EDGES) % 4 == 0

# D: cat_concat2 (ca, acs, cb, bcs, ycs, M); cat_slice_channels (xcs, c0, c, ycs, M)
CONCAT_CASES = [(3, 4, 3, 4, 8, 77), (36, 36, 3, 4, 40, 77),
                (35, 36, 3, 8, 44, 77),          # a wide ycs: six zero lanes
                (0, 4, 5, 8, 8, 77), (5, 8, 0, 4, 8, 77), (1, 4, 1, 4, 4, 1),
                (5, 8, 3, 4, 8, AT // 8),        # M * ycs == 8192 * 256
                (7, 8, 3, 4, 12, 262147)]        # 3 145 764 lanes: the grid-stride trip
CONCAT_HALVES = (36, 36, 3, 4, 40, 2 * 5 * 7)    # DiscInputFn.forward: [sem | fake] and [sem | real] into the halves of a 2N batch
CONCAT_REFUSED = [(3, 4, 3, 4, 4, 77), (5, 8, 4, 4, 8, 77)]
SLICE_CASES = [(8, 0, 3, 4, 77), (8, 3, 3, 4, 77), (40, 36, 3, 4, 77),
               (40, 35, 5, 8, 77),               # c0 % 4 != 0, three zero lanes
               (44, 0, 44, 44, 77),
               (44, 0, 12, 44, 77),              # frozen.py: ycs == xcs, the lanes behind the copy are zeroed, nothing behind the buffer
               (88, 0, 24, 88, 77),              # ... and the whole residual range of a block with two k = 1 branches in one call
               (12, 5, 3, 8, AT // 8),           # M * ycs == 8192 * 256
               (16, 5, 7, 12, 262147)]           # the grid-stride trip
SLICE_REFUSED = [(8, 6, 3, 4, 77),               # c0 + c > xcs
                 (8, 0, 5, 4, 77)]               # c > ycs

# E
FILL_NS = (0, 1, 255, 256, 257, AT, OVER)
FILL_VALUES = (0.0, -0.0, 1.5)
AXPY_AS = (0.0, 1.0, -0.5, 1.0 / 3.0)
AXPY_EXACT = (0.0, 1.0, -0.5)      # a * x is exact (0, x, a power of two), so y + a * x is ONE correctly rounded operation, fused or not
ADDN_ALIAS = [(2, ADDN_SMALL), (8, ADDN_SMALL), (2, 4 * OVER)]

# F: (N, C, H, W, cs, pad)
PAD_CASES = [(2, 11, 9, 7, 12, 1), (1, 42, 6, 10, 44, 2), (3, 4, 1, 5, 4, 2),
             (2, 3, 5, 1, 8, 3),                 # a wide stride, W == 1, pad > W
             (1, 5, 2, 3, 8, 4),                 # pad > H
             (2, 5, 4, 6, 8, 0),                 # pad == 0: forward and backward are the identity
             (1, 4, 1022, 2046, 4, 1),           # the padded plane is 1024 x 2048: the forward's grid exactly once
             (1, 4, 1024, 2048, 4, 1),           # ... the backward's
             (1, 4, 1500, 1500, 4, 1)]           # both over the cap
# pad 3 on W == 1 and pad 4 on 2 x 3: a corner sums 28 / 25 terms, and the float32 autograd twin of F.pad is 1.2e-7 / 1.01e-7 from float64,
# not within a tenth of 1e-6.  Their bar is ten times the twin's distance, rounded up to one significant digit
PAD_BARS = {(2, 3, 5, 1, 8, 3): 2e-6, (1, 5, 2, 3, 8, 4): 2e-6}
PAD_REFUSED = [(2, 5, 4, 6, 6, 1),               # cs % 4 != 0
               (2, 5, 4, 6, 4, 1)]               # cs < C


def _large(numel):
    return numel > 1 << 18


def pad_items(case):
    """quads the forward and the backward kernel walk"""
    n, c, h, w, cs, pad = case
    return n * (h + 2 * pad) * (w + 2 * pad) * (cs // 4), n * h * w * (cs // 4)


# ================================================================================================ references (any dtype)
def _act_ref_fwd(x, act, dtype):
    """the formula of common.h's apply_act on float32 inputs carried in `dtype`; slope is the float32 the kernel receives"""
    x = x.to(dtype)
    zero = torch.zeros((), dtype=dtype)
    slope = torch.tensor(np.float32(SLOPE).item(), dtype=dtype)
    if act == ACT_RELU:
        return torch.where(x > 0, x, zero)
    if act == ACT_LRELU:
        return torch.where(x > 0, x, x * slope)
    if act == ACT_TANH:
        return torch.tanh(x)
    if act == ACT_RELU6:
        return torch.clamp(x, 0.0, 6.0)
    return x


def _act_ref_bwd(y, dy, act, dtype):
    """act_grad_from_out of common.h / ATen: 0 at y == 0 for RELU (threshold_backward), slope at y == 0 for LRELU (leaky_relu_backward), 0 at
    y == 0 and y == 6 for RELU6 (hardtanh_backward)"""
    y, dy = y.to(dtype), dy.to(dtype)
    one, zero = torch.ones((), dtype=dtype), torch.zeros((), dtype=dtype)
    slope = torch.tensor(np.float32(SLOPE).item(), dtype=dtype)
    if act == ACT_RELU:
        return dy * torch.where(y > 0, one, zero)
    if act == ACT_LRELU:
        return dy * torch.where(y > 0, one, slope)
    if act == ACT_TANH:
        return dy * (1.0 - y * y)
    if act == ACT_RELU6:
        return dy * torch.where((y > 0) & (y < 6), one, zero)
    return dy


@functools.lru_cache(maxsize=None)
def _act_inputs(n):
    """x (also the `y` the backward differentiates through: on and beside every bound) and dy; the bounds at both ends of the buffer"""
    edges = torch.from_numpy(np.array(ACT_EDGES, dtype=np.float32))
    if _large(n):
        x = (_pattern(n) - 4095.0) / 512.0                       # [-8, 8) in steps of 1 / 512: 0 and 6 are hit thousands of times
        dy = (_pattern(n, 7, 4093) - 2046.0) / 256.0
    else:
        x = 3.0 * detfill.normal((n,), 900)
        dy = detfill.normal((n,), 901)
    k = min(n, len(edges))
    x[:k] = edges[:k]
    x[n - k:] = edges[len(edges) - k:]
    return x, dy


def _tanh_ref(n, dtype):
    x, dy = _act_inputs(n)
    y = torch.tanh(x).clamp(-1.0, 1.0)       # the backward sees a float32 tanh output, its bounds +-1 included
    return {'y': _act_ref_fwd(x, ACT_TANH, dtype), 'dx': _act_ref_bwd(y, dy, ACT_TANH, dtype)}


def _axpy_inputs(n):
    if _large(n):
        return _pattern(n) / 64.0, _pattern(n, 5, 4093) / 32.0
    return detfill.normal((n,), 910), detfill.normal((n,), 911)


def _axpy_ref(n, a, dtype):
    y, x = _axpy_inputs(n)
    return {'y': y.to(dtype) + torch.tensor(np.float32(a).item(), dtype=dtype) * x.to(dtype)}


def _pad_inputs(case):
    n, c, h, w, cs, pad = case
    shp, shpp = (n, c, h, w), (n, c, h + 2 * pad, w + 2 * pad)
    if _large(n * c * h * w):
        return _pattern(n * c * h * w).view(shp), (_pattern(int(np.prod(shpp)), 3, 4093) / 16.0).view(shpp)
    return detfill.normal(shp, 920), detfill.normal(shpp, 921)


@functools.lru_cache(maxsize=None)
def _pad_ref64(case):
    return _pad_ref(case, torch.float64)


def _pad_ref(case, dtype):
    """F.pad(mode='replicate') and its autograd"""
    n, c, h, w, cs, pad = case
    x, gy = _pad_inputs(case)
    x = x.to(dtype).requires_grad_(True)
    y = F.pad(x, (pad,) * 4, mode='replicate')
    y.backward(gy.to(dtype))
    return {'y': y.detach(), 'dx': x.grad}


def _border_classes(h, w):
    """corner / edge / interior masks over [H, W]: a pixel on a border collects pad + 1 rows or columns, a corner both"""
    by = torch.zeros(h, 1, dtype=torch.bool)
    bx = torch.zeros(1, w, dtype=torch.bool)
    by[0], by[-1], bx[0, 0], bx[0, -1] = True, True, True, True
    return {'corner': by & bx, 'edge': by ^ bx, 'interior': ~(by | bx)}


def _pad_dist(got, want, h, w):
    """rel() over the tensor and over each non-empty border class"""
    out = {'all': rel(got, want)}
    for name, mask in _border_classes(h, w).items():
        if bool(mask.any()):
            out[name] = rel(got[:, :, mask], want[:, :, mask])
    return out


# ================================================================================================ A: host
def test_case_tables_reach_every_regime():
    """a table edit that loses a regime named for these kernels fails here, not silently on the GPU"""
    def cap_regimes(items, what):
        blocks = [cdiv(i, 256) for i in items]
        assert any(b < CAP for b in blocks) and any(b == CAP and i == AT for b, i in zip(blocks, items)) and any(b > CAP for b in blocks), what
        assert all(ew_grid(i) == max(1, min(b, CAP)) for i, b in zip(items, blocks))
    assert ew_grid(AT) == CAP == ew_grid(OVER) and ew_grid(AT - 256) == CAP - 1 and OVER % 256

    # B: tiles on both axes of both transposes, every edge the tables must hold, the fast path taken / declined / over the cap
    for to_nhwc in (True, False):
        tile = [c for c in LAYOUT_CASES if not (to_nhwc and fast_path(c))]
        grids = [layout_grid(c, to_nhwc) for c in tile]
        assert {1, 2, 3} <= {g[0] for g in grids} and {1, 2, 3} <= {g[1] for g in grids} and {1, 3} <= {g[2] for g in grids}, to_nhwc
        assert any(g[0] > 1 and g[1] > 1 and g[2] > 1 for g in grids)
    assert {c[1] for c in LAYOUT_CASES if c[2] * c[3] == 65} >= {1, 5, 63, 64, 65, 130}
    assert {c[2] * c[3] for c in LAYOUT_CASES if c[1] == 65} >= {1, 63, 64, 65, 129}
    assert (3, 130, 3, 43, 132) in LAYOUT_CASES and all(c[2] != c[3] or c[2] == 1 for c in LAYOUT_CASES)
    assert (2, 62, 5, 13, 68) in LAYOUT_CASES and 62 < 64 < 68 and layout_grid((2, 62, 5, 13, 68), True)[1] == 2
    assert any(c[4] > cs4(c[1]) and c[4] < 64 for c in LAYOUT_CASES)
    assert {(c[1], c[2] * c[3]) for c in LAYOUT_FAST} == {(ch, hw) for ch in (1, 2, 3, 4) for hw in (1, 65)} and all(fast_path(c) for c in LAYOUT_FAST)
    assert all(not fast_path(c, aligned=False) for c in LAYOUT_FAST) and not any(fast_path(c) for c in LAYOUT_TILE + LAYOUT_WIDE if c[1] > 1)
    cap_regimes([c[0] * c[2] * c[3] for c in LAYOUT_CASES if fast_path(c)], 'nchw_to_nhwc4')
    assert any(c[1] == 3 and c[0] * c[2] * c[3] == OVER for c in LAYOUT_LARGE)

    # C
    assert set(ACT_NS) == {4, 4 * 255, 4 * 256, 4 * 257, 4 * OVER} and all(n % 4 == 0 for n in ACT_NS)
    cap_regimes([n // 4 for n in ACT_NS + (ACT_AT[1],)], 'act')
    assert [ew_grid(n // 4) for n in ACT_NS[:4]] == [1, 1, 1, 2]
    edges = {float(v) for v in ACT_EDGES}
    assert {0.0, 6.0, 20.0, -20.0, 88.0, -88.0, float(_NA(6, np.inf)), float(_NA(6, -np.inf)), float(_NA(0, np.inf)), float(_NA(0, -np.inf)),
            float(_F32(1e-30)), float(_F32(-1e-30))} <= edges
    assert any(np.signbit(v) and v == 0 for v in map(np.float32, ACT_EDGES))
    for n in ACT_NS:      # the bounds the gradient switches on are in every input set that can hold them
        x, dy = _act_inputs(n)
        assert x.numel() == n and bool(torch.isfinite(x).all()) and bool(torch.isfinite(dy).all())
        if n >= len(ACT_EDGES):
            assert bool((x == 0).any()) and bool((x == 6).any())

    # D
    for want in ((3, 4, 3, 4, 8, 77), (36, 36, 3, 4, 40, 77), (35, 36, 3, 8, 44, 77), (0, 4, 5, 8, 8, 77), (5, 8, 0, 4, 8, 77), (1, 4, 1, 4, 4, 1),
                 (7, 8, 3, 4, 12, 262147)):
        assert want in CONCAT_CASES
    cap_regimes([c[5] * c[4] for c in CONCAT_CASES], 'concat2')
    assert any(c[1] != c[3] for c in CONCAT_CASES) and any(c[4] - c[0] - c[2] >= 6 for c in CONCAT_CASES)
    assert all(c[0] + c[2] > c[4] for c in CONCAT_REFUSED) and all(c[0] + c[2] <= c[4] and c[0] <= c[1] and c[2] <= c[3] for c in CONCAT_CASES)
    for want in ((8, 0, 3, 4, 77), (8, 3, 3, 4, 77), (40, 36, 3, 4, 77), (40, 35, 5, 8, 77), (44, 0, 44, 44, 77), (44, 0, 12, 44, 77)):
        assert want in SLICE_CASES
    cap_regimes([c[4] * c[3] for c in SLICE_CASES], 'slice_channels')
    assert any(c[1] % 4 for c in SLICE_CASES) and all(c[1] + c[2] <= c[0] and c[2] <= c[3] for c in SLICE_CASES)
    assert any(c[1] + c[2] > c[0] and c[2] <= c[3] for c in SLICE_REFUSED) and any(c[2] > c[3] and c[1] + c[2] <= c[0] for c in SLICE_REFUSED)

    # E
    assert {0, 1, 255, 256, 257, OVER} <= set(FILL_NS)
    cap_regimes([n for n in FILL_NS if n], 'fill / axpy')
    assert any(v == 0 and np.signbit(v) for v in FILL_VALUES) and set(AXPY_AS) == {0.0, 1.0, -0.5, 1.0 / 3.0}
    assert {k for k, n in ADDN_ALIAS} == {2, 8} and any(n // 4 > AT for k, n in ADDN_ALIAS)

    # F
    for want in ((2, 11, 9, 7, 12, 1), (1, 42, 6, 10, 44, 2), (3, 4, 1, 5, 4, 2), (2, 3, 5, 1, 8, 3), (1, 5, 2, 3, 8, 4), (2, 5, 4, 6, 8, 0),
                 (1, 4, 1500, 1500, 4, 1)):
        assert want in PAD_CASES
    cap_regimes([pad_items(c)[0] for c in PAD_CASES], 'replicate_pad_fwd')
    cap_regimes([pad_items(c)[1] for c in PAD_CASES], 'replicate_pad_bwd')
    assert any(c[4] > cs4(c[1]) for c in PAD_CASES) and any(c[5] == 0 for c in PAD_CASES) and any(c[5] > c[2] > 1 for c in PAD_CASES)
    assert any(c[3] == 1 and c[5] > 1 for c in PAD_CASES) and any(c[2] == 1 for c in PAD_CASES)
    assert any(c[4] % 4 for c in PAD_REFUSED) and any(c[4] % 4 == 0 and c[4] < c[1] for c in PAD_REFUSED)
    assert all(c[4] % 4 == 0 and c[4] >= c[1] for c in PAD_CASES)


def test_fp32_twin_of_every_reference_is_within_a_tenth_of_the_bar():
    """C (TANH), E (axpy) and F (backward) on the host: float32 ATen against float64 ATen, within a tenth of the bar each is held to on the GPU"""
    for n in ACT_NS + (ACT_AT[1],):
        _host('C-tanh', n, functools.partial(_tanh_ref, n), {'y': TANH_BAR, 'dx': TANH_BAR})
    for n in FILL_NS[1:]:
        for a in AXPY_AS:
            _host('E-axpy', (n, a), functools.partial(_axpy_ref, n, a), {'y': AXPY_BAR})
    for case in PAD_CASES:
        n, c, h, w, cs, pad = case
        r64, r32 = _pad_ref64(case), _pad_ref(case, torch.float32)
        assert torch.equal(r32['y'].double(), r64['y'])
        for name, d in _pad_dist(r32['dx'], r64['dx'], h, w).items():
            print('host F %s %s fp32-vs-fp64 rel %.3g' % (case, name, d))
            assert d <= PAD_BARS.get(case, PAD_BAR) / 10, (case, name, d)


def _frozen_block(res, ks, dw=(), dks=(), cin=16, seed=77):
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    blk = InvertedResidualChannels(cin, list(res), list(dw), 1, list(ks), list(dks), padding_type='reflect', use_bias=False, norm_layer=cnn.BatchNorm2d,
                                   norm_kwargs={'momentum': 0.1, 'eps': 1e-5}, active_fn=get_active_fn('nn.ReLU'))
    blk.load_state_dict(detfill.fill_state_dict(blk.state_dict(), seed, gamma_abs_normal=True))
    return blk.eval()


def test_frozen_plan_copies_only_at_offset_zero():
    """frozen.block_forward copies the k = 1 residual slots of the hidden buffer with cat_slice_channels(ycs == xcs == hc), which writes all hc
    lanes of every pixel: only a copy at lane 0 stays inside the buffer.  Res kernel sizes [1, 3, 5] give one k = 1 slot, at 0.  A block with
    two k = 1 residual branches and no depthwise one CAN be built and frozen.applicable admits it (two 1 x 1 slots); the plan used to hold a
    copy per slot, the second at o = 12 here: it zeroed the first slot of every following pixel and wrote 12 floats behind the buffer.  The
    plan now holds ONE copy of the whole residual range (the k = 1 slots come first and are contiguous);
    test_frozen_block_with_two_k1_residual_branches runs it."""
    from cat_amd import frozen
    with torch.no_grad():
        p = frozen._build_plan(_frozen_block((42, 42, 42), (1, 3, 5), (42, 42, 42), (1, 3, 5)))
        assert p['hc'] == 176 and p['copies'] == [(0, 44)] and all(o == 0 for o, sz in p['copies'])
        p = frozen._build_plan(_frozen_block((10, 6), (1, 1)))
        assert p['hc'] == 20 and p['dwm'] is None and p['copies'] == [(0, 20)]
        p = frozen._build_plan(_frozen_block((10, 6, 5), (1, 1, 3), (7,), (3,)))
        assert p['hc'] == 28 and p['copies'] == [(0, 20)] and [d['off'] for d in p['dws']] == [20]
        p = frozen._build_plan(_frozen_block((0, 42, 42), (1, 3, 5), (42, 42, 42), (1, 3, 5)))
        assert p['copies'] == []


# ================================================================================================ GPU plumbing
@pytest.fixture(scope='module')
def dev():
    _lib()
    return torch.device('cuda:0')


def _nhwc_host(x, cs, pad):
    """[N, C, H, W] -> [N, H, W, cs] with `pad` in the lanes [C, cs), by permute"""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, cs), pad, dtype=x.dtype)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return buf


def _layout_x(case):
    n, c, h, w, cs = case
    numel = n * c * h * w
    return _pattern(numel).view(n, c, h, w) if _large(numel) else detfill.normal((n, c, h, w), 930)


def _case_id(case):
    return '-'.join(str(v) for v in case)


# ================================================================================================ B: layout
def _to_nhwc(L, dev, case, xg, misalign=0):
    """-> (the whole destination buffer on the host, y [N, H, W, cs]); `misalign` floats in front of y stay NaN"""
    n, c, h, w, cs = case
    numel = n * h * w * cs
    flat, _ = _out((misalign + numel,), dev)
    L.call('cat_nchw_to_nhwc', _p(xg), _p(flat, misalign), n, c, h, w, cs, _stream())
    torch.cuda.synchronize()
    _tail(flat, (case, misalign))
    host = flat.cpu()
    assert bool(torch.isnan(host[:misalign]).all()), (case, 'wrote in front of y')
    return host[misalign:misalign + numel].view(n, h, w, cs)


@pytest.mark.gpu
@pytest.mark.parametrize('case', LAYOUT_CASES, ids=_case_id)
def test_nchw_to_nhwc(dev, case):
    """the channel lanes are the permuted input bit for bit, every lane in [C, cs) is exactly 0.0, nothing behind the buffer is written"""
    L = _lib()
    n, c, h, w, cs = case
    x = _layout_x(case)
    y = _to_nhwc(L, dev, case, _in(x, dev))
    assert torch.equal(_bits(y[..., :c]), _bits(x.permute(0, 2, 3, 1))), (case, 'channel lanes')
    assert torch.equal(_bits(y[..., c:]), torch.zeros(n, h, w, cs - c, dtype=torch.int32)), (case, 'padding lanes')


@pytest.mark.gpu
@pytest.mark.parametrize('case', LAYOUT_FAST, ids=_case_id)
def test_nchw_to_nhwc_declines_the_fast_path_for_an_unaligned_destination(dev, case):
    """y at base + 4 bytes: the tile kernel; bit for bit the aligned (one lane per pixel) run and the permuted input"""
    L = _lib()
    n, c, h, w, cs = case
    x = _layout_x(case)
    xg = _in(x, dev)
    fast, tile = _to_nhwc(L, dev, case, xg), _to_nhwc(L, dev, case, xg, misalign=1)
    assert torch.equal(_bits(tile), _bits(fast)), (case, 'tile kernel against the fast path')
    assert torch.equal(_bits(tile), _bits(_nhwc_host(x, cs, 0.0))), case


@pytest.mark.gpu
@pytest.mark.parametrize('case', LAYOUT_CASES, ids=_case_id)
def test_nhwc_to_nchw(dev, case):
    """the output is the permuted input bit for bit; the input's padding lanes hold NaN: a leak is visible"""
    L = _lib()
    n, c, h, w, cs = case
    x = _layout_x(case)
    xg = _in(_nhwc_host(x, cs, NAN), dev)
    yf, y = _out((n, c, h, w), dev)
    L.call('cat_nhwc_to_nchw', _p(xg), _p(y), n, c, h, w, cs, _stream())
    torch.cuda.synchronize()
    _tail(yf, case)
    assert torch.equal(_bits(y.cpu()), _bits(x)), case


@pytest.mark.gpu
def test_layout_refuses_a_stride_below_the_channel_count(dev):
    L = _lib()
    xg = _in(torch.zeros(2, 5, 3, 3), dev)
    of, o = _out((2, 3, 3, 8), dev, SENTINEL)
    _refused(L, 'cat_nchw_to_nhwc', of, _p(xg), _p(o), 2, 5, 3, 3, 4, _stream())
    _refused(L, 'cat_nhwc_to_nchw', of, _p(xg), _p(o), 2, 5, 3, 3, 4, _stream())


# ================================================================================================ C: activations
def _act_run(L, dev, n, act, xg, dyg, in_place=False, yg=None):
    """forward of xg; backward through the OUTPUT yg (the input set itself where none is given: on and beside every bound)"""
    if in_place:
        yf, y = _out((n,), dev)
        y.copy_(xg)
        src = y
    else:
        (yf, y), src = _out((n,), dev), xg
    L.call('cat_act_fwd', _p(src), _p(y), n, act, SLOPE, _stream())
    torch.cuda.synchronize()
    _tail(yf, (n, act, 'y'))
    if in_place:
        return {'y': y.cpu()}
    dxf, dx = _out((n,), dev)
    L.call('cat_act_bwd', _p(xg if yg is None else yg), _p(dyg), _p(dx), n, act, SLOPE, _stream())
    torch.cuda.synchronize()
    _tail(dxf, (n, act, 'dx'))
    return {'y': y.cpu(), 'dx': dx.cpu()}


@pytest.mark.gpu
@pytest.mark.parametrize('act,n', [(a, n) for a in ACTS for n in ACT_NS] + [ACT_AT])
def test_act_fwd_bwd(dev, act, n):
    """NONE / RELU / LRELU / RELU6: every result is one correctly rounded float32 operation (a select, or one product whose float64 value is
    exact), so the float64 formula rounded to float32 is the answer: torch.equal (-0.0 == 0.0).  TANH: rel() < 1e-6 against float64; its
    backward on y = tanh(x) in [-1, 1].  The forward in place (ksum.py) is bit for bit the out-of-place one."""
    L = _lib()
    x, dy = _act_inputs(n)
    xg, dyg = _in(x, dev), _in(dy, dev)
    if act == ACT_TANH:
        got = _act_run(L, dev, n, act, xg, dyg, yg=_in(torch.tanh(x).clamp(-1.0, 1.0), dev))
        _cmp('C', ('tanh', n), got, _tanh_ref(n, torch.float64), {'y': TANH_BAR, 'dx': TANH_BAR})
        assert float(got['y'].abs().max()) <= 1.0
    else:
        got = _act_run(L, dev, n, act, xg, dyg)
        want = {'y': _act_ref_fwd(x, act, torch.float64).float(), 'dx': _act_ref_bwd(x, dy, act, torch.float64).float()}
        for key in want:
            assert torch.equal(got[key], want[key]), (act, n, key, int((got[key] != want[key]).sum()), 'elements differ')
    assert torch.equal(_bits(_act_run(L, dev, n, act, xg, None, in_place=True)['y']), _bits(got['y'])), (act, n, 'in place')


@pytest.mark.gpu
@pytest.mark.parametrize('act', ACTS)
def test_act_on_and_beside_the_bounds(dev, act):
    """the whole bound set in one buffer (n = 4 holds four of them), value and gradient element by element"""
    L = _lib()
    n = len(ACT_EDGES)
    x = torch.from_numpy(np.array(ACT_EDGES, dtype=np.float32))
    dy = 0.5 + detfill.normal((n,), 902).abs()      # no zero: a gradient that must vanish is seen to
    got = _act_run(L, dev, n, act, _in(x, dev), _in(dy, dev))
    y64, dx64 = _act_ref_fwd(x, act, torch.float64), _act_ref_bwd(x, dy, act, torch.float64)
    for i in range(n):
        print('act %d x %.9g: y %.9g (want %.9g), dx / dy %.9g (want %.9g)' % (act, float(x[i]), float(got['y'][i]), float(y64[i]),
                                                                             float(got['dx'][i] / dy[i]), float(dx64[i] / dy[i])))
    if act == ACT_TANH:
        _cmp('C', ('tanh bounds', n), got, {'y': y64, 'dx': dx64}, {'y': TANH_BAR, 'dx': TANH_BAR})
        assert float(got['y'].abs().max()) <= 1.0                                                  # +-20 and +-88 saturate, never beyond 1
        assert float(got['dx'][E_ONE]) == 0.0 and float(got['dx'][E_ZERO]) == float(dy[E_ZERO])      # 1 - 1 * 1 and 1 - 0 * 0 are exact
        return
    assert torch.equal(got['y'], y64.float()) and torch.equal(got['dx'], dx64.float()), act
    # the gradient at the bounds, spelled out: dx is dy times exactly this factor, rounded once
    factor = lambda i, f: float(got['dx'][i]) == float((dy[i].double() * float(np.float32(f))).float())
    if act == ACT_RELU:
        assert factor(E_ZERO, 0.0) and factor(E_ZERO_UP, 1.0) and factor(E_ZERO_DOWN, 0.0)
    if act == ACT_LRELU:
        assert factor(E_ZERO, SLOPE) and factor(E_ZERO_UP, 1.0) and factor(E_ZERO_DOWN, SLOPE)
    if act == ACT_RELU6:
        assert factor(E_ZERO, 0.0) and factor(E_SIX, 0.0) and factor(E_SIX_UP, 0.0) and factor(E_SIX_DOWN, 1.0) and factor(E_ZERO_UP, 1.0)
        assert float(got['y'][E_SIX_UP]) == 6.0 and float(got['y'][E_SIX_DOWN]) == float(ACT_EDGES[E_SIX_DOWN])


@pytest.mark.gpu
def test_act_refuses_a_length_that_is_no_multiple_of_four(dev):
    L = _lib()
    xg = _in(torch.ones(8), dev)
    of, o = _out((8,), dev, SENTINEL)
    for n in (6, 1):
        _refused(L, 'cat_act_fwd', of, _p(xg), _p(o), n, ACT_RELU, SLOPE, _stream())
        _refused(L, 'cat_act_bwd', of, _p(xg), _p(xg), _p(o), n, ACT_RELU, SLOPE, _stream())


# ================================================================================================ D: concat / slice
def _lanes(m, cs, c, seed, c0=0):
    """host [M, cs]: values in the lanes [c0, c0 + c), NaN everywhere else"""
    buf = torch.full((m, cs), NAN)
    buf[:, c0:c0 + c] = _pattern(m * c, seed % 5 + 1).view(m, c) if _large(m * cs) else detfill.normal((m, c), seed)
    return buf


def _concat_check(case, y, a, b):
    ca, acs, cb, bcs, ycs, m = case
    want = torch.cat((a[:, :ca], b[:, :cb]), 1)
    assert torch.equal(_bits(y[:, :ca + cb]), _bits(want)), (case, 'channels')
    assert torch.equal(_bits(y[:, ca + cb:]), torch.zeros(m, ycs - ca - cb, dtype=torch.int32)), (case, 'lanes behind ca + cb')


@pytest.mark.gpu
@pytest.mark.parametrize('case', CONCAT_CASES, ids=_case_id)
def test_concat2(dev, case):
    """torch.cat bit for bit, the lanes [ca + cb, ycs) exactly 0; the sources carry NaN in their padding lanes"""
    L = _lib()
    ca, acs, cb, bcs, ycs, m = case
    a, b = _lanes(m, acs, ca, 940), _lanes(m, bcs, cb, 941)
    yf, y = _out((m, ycs), dev)
    ag, bg = _in(a, dev), _in(b, dev)
    L.call('cat_concat2', _p(ag), ca, acs, _p(bg), cb, bcs, _p(y), ycs, m, _stream())
    torch.cuda.synchronize()
    _tail(yf, case)
    _concat_check(case, y.cpu(), a, b)


@pytest.mark.gpu
def test_concat2_into_the_halves_of_a_2n_batch(dev):
    """DiscInputFn.forward: [sem | fake] into the first half, [sem | real] at y + half; the second call leaves the first half as it was"""
    L = _lib()
    ca, acs, cb, bcs, ycs, m = CONCAT_HALVES
    sem, fake, real = _lanes(m, acs, ca, 942), _lanes(m, bcs, cb, 943), _lanes(m, bcs, cb, 944)
    semg, fakeg, realg = _in(sem, dev), _in(fake, dev), _in(real, dev)
    yf, y = _out((2 * m, ycs), dev)
    L.call('cat_concat2', _p(semg), ca, acs, _p(fakeg), cb, bcs, _p(y), ycs, m, _stream())
    torch.cuda.synchronize()
    first = y.cpu()
    assert bool(torch.isnan(first[m:]).all()), 'the first call wrote into the second half'
    L.call('cat_concat2', _p(semg), ca, acs, _p(realg), cb, bcs, _p(y, m * ycs), ycs, m, _stream())
    torch.cuda.synchronize()
    _tail(yf, 'halves')
    both = y.cpu()
    assert torch.equal(_bits(both[:m]), _bits(first[:m])), 'the second call changed the first half'
    _concat_check(CONCAT_HALVES, both[:m], sem, fake)
    _concat_check(CONCAT_HALVES, both[m:], sem, real)


@pytest.mark.gpu
@pytest.mark.parametrize('case', SLICE_CASES, ids=_case_id)
def test_slice_channels(dev, case):
    """y[:, :c] is x[:, c0:c0 + c] bit for bit and y[:, c:ycs] exactly 0: the kernel writes all ycs lanes of every pixel and nothing behind the
    last; the lanes of x outside the range hold NaN"""
    L = _lib()
    xcs, c0, c, ycs, m = case
    x = _lanes(m, xcs, c, 950, c0)
    yf, y = _out((m, ycs), dev)
    xg = _in(x, dev)
    L.call('cat_slice_channels', _p(xg), xcs, c0, c, _p(y), ycs, m, _stream())
    torch.cuda.synchronize()
    _tail(yf, case)
    yc = y.cpu()
    assert torch.equal(_bits(yc[:, :c]), _bits(x[:, c0:c0 + c])), (case, 'channels')
    assert torch.equal(_bits(yc[:, c:]), torch.zeros(m, ycs - c, dtype=torch.int32)), (case, 'lanes behind c')


@pytest.mark.gpu
def test_concat2_and_slice_channels_refuse_a_range_that_does_not_fit(dev):
    L = _lib()
    for ca, acs, cb, bcs, ycs, m in CONCAT_REFUSED:
        of, o = _out((m, ycs), dev, SENTINEL)
        ag, bg = _in(torch.zeros(m, acs), dev), _in(torch.zeros(m, bcs), dev)
        _refused(L, 'cat_concat2', of, _p(ag), ca, acs, _p(bg), cb, bcs, _p(o), ycs, m, _stream())
    for xcs, c0, c, ycs, m in SLICE_REFUSED:
        of, o = _out((m, ycs), dev, SENTINEL)
        xg = _in(torch.zeros(m, xcs), dev)
        _refused(L, 'cat_slice_channels', of, _p(xg), xcs, c0, c, _p(o), ycs, m, _stream())


@pytest.mark.gpu
@pytest.mark.parametrize('res,ks,dw,dks', [((10, 6), (1, 1), (), ()), ((10, 6, 5), (1, 1, 3), (), ())], ids=['k11', 'k113'])
def test_frozen_block_with_two_k1_residual_branches(dev, res, ks, dw, dks):
    """an eval BatchNorm block frozen.applicable admits whose plan has no one-launch depthwise stage: the residual range of the hidden buffer is
    copied by cat_slice_channels.  Against the general path and the float64 twin out of stock torch.nn layers, the project's 1e-3 bar for
    blocks; with a copy per slot the first branch was lost for every pixel but the first."""
    import copy
    from cat_amd import frozen, ops
    from test_fused_block_gpu import _torch_twin
    blk = _frozen_block(res, ks, dw, dks).to(dev).eval()
    general = copy.deepcopy(blk)
    general._cat_frozen_off = True
    x = detfill.normal((2, 16, 7, 9), 5)
    xg = _in(_nhwc_host(x, 16, 0.0), dev).permute(0, 3, 1, 2)
    twin, fwd = _torch_twin(blk)
    twin.eval().double()
    with torch.no_grad():
        assert ops.is_act(xg) and frozen.applicable(blk, xg) and not frozen.applicable(general, xg)
        assert frozen._plan(blk)['dwm'] is None and frozen._plan(blk)['copies'] == [(0, 20)]
        y, y_g, y_t = blk(xg), general(xg), fwd(x.double())
    torch.cuda.synchronize()
    fig = {'frozen_twin': rel(y, y_t), 'general_twin': rel(y_g, y_t)}
    MAXREL['D-block'] = max(MAXREL.get('D-block', 0.0), fig['frozen_twin'])
    print('D frozen block %s: %s' % (ks, ', '.join('%s %.3g' % kv for kv in fig.items())))
    assert fig['frozen_twin'] < BLOCK_BAR and fig['general_twin'] < BLOCK_BAR, fig


# ================================================================================================ E: fill, axpy, add_n in place
@pytest.mark.gpu
@pytest.mark.parametrize('v', FILL_VALUES, ids=lambda v: repr(v))
@pytest.mark.parametrize('n', FILL_NS)
def test_fill_inside_a_larger_buffer(dev, n, v):
    """FusedAdam.zero_grad() and the None half of BatchHalvesFn.backward: n floats at an offset, both neighbours intact, the sign of -0.0 kept"""
    L = _lib()
    flat, _ = _out((64 + n,), dev, SENTINEL)
    L.call('cat_fill', _p(flat, 64), n, v, _stream())
    torch.cuda.synchronize()
    host = flat.cpu()
    assert bool((host[:64] == SENTINEL).all()), (n, v, 'in front')
    _tail(flat, (n, v))
    want = torch.full((n,), v)
    assert torch.equal(_bits(host[64:64 + n]), _bits(want)), (n, v)


@pytest.mark.gpu
@pytest.mark.parametrize('a', AXPY_AS, ids=lambda a: '%.3g' % a)
@pytest.mark.parametrize('n', FILL_NS)
def test_axpy(dev, n, a):
    """y += a * x against float64; exact where a * x is exact; n == 0 touches nothing"""
    L = _lib()
    y0, x = _axpy_inputs(n)
    yf, y = _out((n,), dev)
    y.copy_(y0.to(dev))
    xg = _in(x, dev)
    L.call('cat_axpy', _p(y), _p(xg), n, a, _stream())
    torch.cuda.synchronize()
    _tail(yf, (n, a))
    if n == 0:
        return
    got, want = {'y': y.cpu()}, _axpy_ref(n, a, torch.float64)
    _cmp('E', ('axpy', n, a), got, want, {'y': AXPY_BAR})
    if a in AXPY_EXACT:
        assert torch.equal(got['y'], want['y'].float()), (n, a)


@pytest.mark.gpu
@pytest.mark.parametrize('nsrc,n', ADDN_ALIAS, ids=lambda v: str(v))
def test_add_n_into_its_first_source(dev, nsrc, n):
    """FanoutFn.backward chains cat_add_n with dst == srcs[0]: bit for bit the same sum written to a fresh destination"""
    L = _lib()
    host = [_pattern(n, i + 1) / 8.0 for i in range(nsrc)] if _large(n) else [detfill.normal((n,), 960 + i) for i in range(nsrc)]
    srcs = [_in(t, dev) for t in host]
    of, out = _out((n,), dev)
    ptrs = lambda first: (C.c_void_p * nsrc)(*[t.data_ptr() for t in [first] + srcs[1:]])
    L.call('cat_add_n', ptrs(srcs[0]), nsrc, _p(out), n, _stream())
    af, acc = _out((n,), dev)
    acc.copy_(srcs[0])
    L.call('cat_add_n', ptrs(acc), nsrc, _p(acc), n, _stream())
    torch.cuda.synchronize()
    _tail(of, (nsrc, n))
    _tail(af, (nsrc, n, 'in place'))
    _same({'sum': _bits(acc.cpu())}, {'sum': _bits(out.cpu())}, (nsrc, n))
    for t, h in zip(srcs[1:], host[1:]):
        assert torch.equal(t.cpu(), h), 'a source changed'
    if _large(n):
        assert torch.equal(out.cpu(), (host[0].double() + host[1].double()).float())      # multiples of 1 / 8 below 2048: the sum is exact


# ================================================================================================ F: replicate pad
@pytest.mark.gpu
@pytest.mark.parametrize('case', PAD_CASES, ids=_case_id)
def test_replicate_pad_fwd_bwd(dev, case):
    """forward: F.pad(mode='replicate') bit for bit, the padding lanes of x are 0 and stay 0.  Backward: rel() < 1e-6 (PAD_BARS) against float64 autograd
    of the same pad, over the tensor and per border class (corner, edge, interior)"""
    L = _lib()
    n, c, h, w, cs, pad = case
    hp, wp = h + 2 * pad, w + 2 * pad
    x, gy = _pad_inputs(case)
    want = _pad_ref64(case)
    yf, y = _out((n, hp, wp, cs), dev)
    xg, dyg = _in(_nhwc_host(x, cs, 0.0), dev), _in(_nhwc_host(gy, cs, 0.0), dev)
    L.call('cat_replicate_pad_fwd', _p(xg), _p(y), n, h, w, c, cs, pad, _stream())
    torch.cuda.synchronize()
    _tail(yf, (case, 'y'))
    yc = y.cpu()
    assert torch.equal(_bits(yc), _bits(_nhwc_host(want['y'].float(), cs, 0.0))), (case, 'forward')
    dxf, dx = _out((n, h, w, cs), dev)
    L.call('cat_replicate_pad_bwd', _p(dyg), _p(dx), n, h, w, c, cs, pad, _stream())
    torch.cuda.synchronize()
    _tail(dxf, (case, 'dx'))
    dxc = dx.cpu()
    assert bool(torch.isfinite(dxc).all()) and bool((dxc[..., c:] == 0.0).all()), (case, 'padding lanes of dx')
    got = dxc[..., :c].permute(0, 3, 1, 2)
    bad = []
    for name, d in _pad_dist(got, want['dx'], h, w).items():
        MAXREL['F'] = max(MAXREL.get('F', 0.0), d)
        print('F %s dx %s rel %.3g (bar %.3g)' % (case, name, d, PAD_BARS.get(case, PAD_BAR)))
        if not d < PAD_BARS.get(case, PAD_BAR):
            bad.append((name, d))
    print('F largest rel so far %.3g' % MAXREL['F'])
    assert not bad, (case, bad)
    if pad == 0:
        assert torch.equal(_bits(yc[..., :c]), _bits(x.permute(0, 2, 3, 1))) and torch.equal(_bits(got), _bits(gy)), (case, 'identity')


@pytest.mark.gpu
def test_replicate_pad_refuses_a_bad_stride(dev):
    L = _lib()
    for n, c, h, w, cs, pad in PAD_REFUSED:
        xg = _in(torch.zeros(n * (h + 2 * pad) * (w + 2 * pad) * 8), dev)
        of, o = _out((n * (h + 2 * pad) * (w + 2 * pad) * 8,), dev, SENTINEL)
        for name in ('cat_replicate_pad_fwd', 'cat_replicate_pad_bwd'):
            _refused(L, name, of, _p(xg), _p(o), n, h, w, c, cs, pad, _stream())
