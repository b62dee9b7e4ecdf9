"""The vector-ALU convolutions of csrc/conv_smallco.hip -- fwd_kernel (Cout 1 / 3, k 4 / 7: the generators' 7 x 7 -> 3 output layer, the
PatchGAN and multiscale heads' 4 x 4 -> 1 layer), wgrad_kernel and dgrad_s2_kernel (the PatchGAN first layer's gradient into the image) --
through the C ABI against float64 ATen on the host, at the edges of their own plans: both tile forms of the forward, tile grids with more
than one tile along x and y, ragged channel chunks and idle channel groups, ragged and even channel splits with and without a workspace, a
NULL bias, the dense (wcs = Cin) filter layout, the weight gradient's grid-stride loop beyond its 256 blocks, both of its tile forms with
accumulate 0 / 1, and the lower bound and the masked last chunk of the image gradient.

A (host): Python mirrors of fwd_small_image, smallco_fwd_ksplit, small_image_cfg, smallco_wgrad_nblk, the three tile grids and
          smallci_dgrad_applicable, held to the library's pure-host workspace queries; a named list of regimes, each a predicate over (case,
          mirror): every regime is declared by a case, every declaration is confirmed by the mirror, and every case is the only one to declare
          at least one regime (dropping a case fails here without a GPU); the template argument lists of the dispatch text of conv_smallco.hip
          against the instantiations the cases claim to launch; the float32 ATen twin of every reference within TOL / 10 of the float64 one.
B (GPU):  forward into a channel slice of a sentinel buffer with a NaN workspace; split cases also without a workspace; NULL bias; dense filters
          with NaNs behind the tensor.
C (GPU):  weight gradient, accumulate 0 over NaNs and 1 over a gradient that is already there, NaN workspace, padding lanes exactly 0; one
          case into a dense dw with sentinels behind it.
D (GPU):  the first layer's image gradient into a channel slice of a sentinel buffer.  The padding lanes [Cout, round_up(Cout, 4)) of dy hold
          a finite non-zero value here: the kernel masks those lanes itself (the filter rows of co >= Cout are staged as zeros), and only a
          non-zero lane makes that mask visible.
E (GPU):  the far side of every clause of smallco_applicable and smallci_dgrad_applicable: parity, and no *_smallco / *_smallci family.

Bars: TOL = 1e-4 with rel() of test_kernels_gpu.py over the whole tensor AND per output channel of y, per output channel of dw and per input
channel of dx (chan_rel of test_streaming_kernels_gpu.py); exact equality for zero lanes, sentinels and padding lanes.  Every figure is
printed.  Largest distances observed on an MI355X: SMALLCO_OBSERVED below (records, not thresholds); the 79 GPU tests take 4.2 s there.

Two shapes are this file's own.  (7, 1, 4, ..., 9, 35) is the big-tile Cout 1 / k 4 case that the two <1, 32, 1, 2, 4, *> instantiations need.
The weight gradient's 8 x 8 second-trip case is (64, 1, 4, ..., 5, 61, 60), one input row more than a 60 x 60 plane with the same 320 tiles
of 8 x 8 and the same ragged edges: at 60 x 60 the bias gradient of its reference, a sum of 17405 unit normals that cancels to |db| = 7.3,
is 2.1e-5 from its float32 twin and misses the TOL / 10 of A; at 61 x 60 it is 1.1e-6 (y, dx and dw are below 2e-6 at either shape).

Hand mutations of conv_smallco.hip that the cases catch (values only, never committed): the forward without column group i = 3 (every case
with Wo > 24), the split walking from quad 0 instead of qbeg (every split case), lanes [CO, cw) left unwritten (every forward case); the
weight gradient stopping after its first trip (both second-trip cases) and staging with TI for ti (the k 4 case of the 16 x 16 form); the
image gradient without the co < Cout zeroing (the Cout 21 case) and with amy / amx swapped in the tile read (both cases)."""
import ctypes as C
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_conv_variants_gpu import (SENTINEL, _act64, _check_slice, _geom, _ids, _nan_ws, _padded_weight, _profiled, _reference,      # noqa: F401
                                    _sentinel_buffer, cs4, dev)      # (dev: fixture)
from test_kernels_gpu import TOL, rel
from test_streaming_kernels_gpu import chan_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALLCO_SRC = os.path.join(ROOT, 'cat_amd', 'csrc', 'conv_smallco.hip')
NAN = float('nan')
SMALLCO_OBSERVED = 'B (forward) 2.0e-06, C (weight gradient) 5.3e-07, D (image gradient) 3.2e-07, E (far sides) 4.2e-07'
MAXREL = {}      # section -> largest distance from the float64 reference seen in this process (printed by every case)


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ A1: mirrors of the host side of conv_smallco.hip
def out_hw(case):
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def smallco_applicable(case):
    cin, cout, k, stride = case[:4]
    return cout in (1, 3) and stride == 1 and k in (4, 7)


def fwd_small_image(cin, n, ho, wo):
    """the 8-row, 4-channel-group form of the forward: many channels, fewer than 256 tiles of 32 x 32"""
    return cin >= 64 and n * cdiv(ho, 32) * cdiv(wo, 32) < 256


def smallco_fwd_ksplit(cin, n, ho, wo):
    """slices of the input-channel range (of >= 2 chunks of 8 quads each) until ~512 workgroups exist; 1 = no split"""
    if not fwd_small_image(cin, n, ho, wo):
        return 1
    blocks = n * cdiv(ho, 8) * cdiv(wo, 32)
    chunks = cdiv(cs4(cin) // 4, 8)
    ks = min(cdiv(512, blocks), chunks // 2)
    if ks < 2:
        return 1
    ks = cdiv(chunks, cdiv(chunks, ks))
    return 1 if ks < 2 else ks


def small_image_cfg(cin, n, ho, wo, k):
    """the 8 x 8-tile, 16-quad-chunk form of the weight gradient"""
    return cin >= 64 and n * cdiv(ho, 16) * cdiv(wo, 16) < 512 and k <= 4


def smallco_wgrad_nblk(cin, n, ho, wo, k):
    sm = small_image_cfg(cin, n, ho, wo, k)
    tile, ckq = (8, 16) if sm else (16, 4)
    ntiles = n * cdiv(ho, tile) * cdiv(wo, tile)
    chunks = cdiv(cs4(cin) // 4, ckq)
    return max(1, min(cdiv(1024, chunks), ntiles, 256))


def smallci_dgrad_applicable(case, wcs=None, ycs=None):
    cin, cout, k, stride, pad, reflect = case[:6]
    wcs = cs4(cin) if wcs is None else (wcs or cin)
    ycs = cs4(cout) if ycs is None else ycs
    return cin in (3, 6) and stride == 2 and k == 4 and pad == 1 and not reflect and cout >= 16 and wcs >= cin and ycs % 4 == 0


@functools.lru_cache(maxsize=None)
def fwd_plan(case, ws=True, dense=False):
    """launch_fwd / smallco_fwd: tile form, grid, the channel split a workspace allows, the chunks fwd_kernel walks per slice (quads staged per
    chunk) and the template arguments of the kernel"""
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    ho, wo = out_hw(case)
    small = fwd_small_image(cin, n, ho, wo)
    th, cg, ckq = (8, 4, 8) if small else (32, 1, 2)
    quads = cs4(cin) // 4
    ksplit = smallco_fwd_ksplit(cin, n, ho, wo) if ws else 1
    if ksplit > 1:
        qchunk = cdiv(cdiv(quads, 8), ksplit) * 8
        slices = [(z * qchunk, min(quads, (z + 1) * qchunk)) for z in range(ksplit)]
    else:
        slices = [(0, quads)]
    assert all(b < e for b, e in slices), 'an empty channel slice would leave its partial sums unwritten'
    walk = [[min(ckq, e - q0) for q0 in range(b, e, ckq)] for b, e in slices]
    return dict(form='8-row' if small else 'big-tile', th=th, cg=cg, ckq=ckq, tiles_x=cdiv(wo, 32), tiles_y=cdiv(ho, th), ksplit=ksplit,
                walk=walk, ho=ho, wo=wo, inst=('fwd_kernel', cout, th, cg, ckq, k, 0 if dense else 1))


@functools.lru_cache(maxsize=None)
def wgrad_plan(case):
    """smallco_wgrad: tile form, blocks along x (each walks tiles t, t + nblk, ...), channel chunks along y"""
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    ho, wo = out_hw(case)
    sm = small_image_cfg(cin, n, ho, wo, k)
    tile, ckq, kmax = (8, 16, 4) if sm else (16, 4, 7)
    quads = cs4(cin) // 4
    per_sample = cdiv(ho, tile) * cdiv(wo, tile)
    return dict(form='8x8' if sm else '16x16', tile=tile, ckq=ckq, ti=tile + k - 1, TI=tile + kmax - 1, per_sample=per_sample,
                ntiles=n * per_sample, nblk=smallco_wgrad_nblk(cin, n, ho, wo, k), walk=[min(ckq, quads - q0) for q0 in range(0, quads, ckq)],
                ho=ho, wo=wo, inst=('wgrad_kernel', 4, tile, ckq, kmax))


@functools.lru_cache(maxsize=None)
def dgrad_plan(case):
    """smallci_dgrad: coarse (per parity class) tiles of 16 x 32, 16-channel chunks of dy"""
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    quads = cs4(cout) // 4
    return dict(tiles_x=cdiv(cdiv(w, 2), 32), tiles_y=cdiv(cdiv(h, 2), 16), walk=[min(4, quads - q0) for q0 in range(0, quads, 4)],
                masked=cs4(cout) - cout, inst=('dgrad_s2_kernel', cin, 4))


# ================================================================================================ the cases of B - D and the regimes they stand for
# A case is (cin, cout, k, stride, pad, reflect, act, N, H, W), as in test_conv_variants_gpu.py.
FWD_CASES = {
    (10, 3, 7, 1, 3, 1, 3, 2, 37, 33): ('fwd big-tile CO3 K7', 'fwd big-tile 2x2 tiles, N 2', 'fwd reflect halo beyond 2W-2 in the masked last tile',
                                        'fwd big-tile chunk with nq 1', 'fwd tanh'),
    (6, 1, 7, 1, 3, 0, 2, 1, 20, 40): ('fwd big-tile CO1 K7', 'fwd big-tile tiles_x 2, zero pad', 'fwd lrelu'),
    (5, 3, 4, 1, 1, 0, 0, 2, 34, 10): ('fwd big-tile CO3 K4', 'fwd big-tile tiles_y 2, N 2'),
    (8, 3, 7, 1, 3, 1, 0, 1, 4, 5): ('fwd big-tile CO3 K7', 'fwd plane smaller than the pad window on both sides'),
    # the only big-tile CO1 K4 shape (the two <1, 32, 1, 2, 4, *> instantiations); Cin % 4 != 0 serves the padded and the dense layout
    (7, 1, 4, 1, 1, 0, 2, 1, 9, 35): ('fwd big-tile CO1 K4', 'fwd big-tile tiles_x 2, zero pad', 'fwd lrelu'),
    (64, 3, 7, 1, 3, 1, 3, 2, 12, 35): ('fwd 8-row CO3 K7', 'fwd 8-row 2x2 tiles, N 2', 'fwd 8-row unsplit, two chunks', 'fwd tanh'),
    (214, 3, 7, 1, 3, 1, 0, 1, 9, 9): ('fwd 8-row CO3 K7', 'fwd 8-row ragged split: 7 chunks -> 3 3 1', 'fwd 8-row last slice a 6-quad chunk'),
    (70, 1, 7, 1, 3, 0, 0, 1, 10, 34): ('fwd 8-row CO1 K7', 'fwd 8-row last chunk nq 2: groups 2 and 3 idle', 'fwd 8-row tiles_x 2'),
    (96, 3, 4, 1, 1, 0, 2, 3, 9, 9): ('fwd 8-row CO3 K4', 'fwd 8-row N 3, three chunks, unsplit', 'fwd lrelu'),
    (160, 1, 4, 1, 1, 0, 0, 2, 17, 9): ('fwd 8-row CO1 K4', 'fwd 8-row ragged split: 5 chunks -> 3 2', 'fwd 8-row tiles_y 2'),
    (256, 3, 4, 1, 2, 0, 0, 1, 7, 7): ('fwd 8-row CO3 K4', 'fwd 8-row even split by 4', 'fwd pad 2'),
}
# the dense (wcs = Cin, Cin % 4 != 0) twin of every forward case: the same shape with Cin moved
DENSE_CIN = {10: 10, 6: 6, 5: 5, 8: 7, 7: 7, 64: 66, 214: 214, 70: 70, 96: 98, 160: 162, 256: 254}
NULL_BIAS_CASES = [(10, 3, 7, 1, 3, 1, 3, 2, 37, 33), (160, 1, 4, 1, 1, 0, 0, 2, 17, 9)]
WGRAD_CASES = {
    (16, 3, 7, 1, 3, 1, 0, 3, 150, 150): ('wgrad 16x16 K7 CO3', 'wgrad 16x16 second trip: 300 tiles over 256 blocks', 'wgrad second-trip tiles cross samples',
                                          'wgrad ragged 150 = 9 * 16 + 6', 'wgrad reflect'),
    (22, 1, 7, 1, 3, 0, 0, 2, 20, 37): ('wgrad 16x16 K7 CO1', 'wgrad 16x16 N 2 with a ragged tile grid', 'wgrad 16x16 last chunk 2 of 4 quads'),
    (20, 3, 4, 1, 1, 0, 0, 2, 18, 35): ('wgrad 16x16 K4 CO3 (ti 19 < TI 22)', 'wgrad 16x16 N 2 with a ragged tile grid'),
    (70, 3, 7, 1, 3, 1, 0, 1, 17, 17): ('wgrad 16x16 K7 CO3', 'wgrad 16x16 K7 with Cin >= 64, 5 chunks', 'wgrad reflect'),
    (64, 1, 4, 1, 1, 0, 0, 5, 61, 60): ('wgrad 8x8 CO1', 'wgrad 8x8 second trip: 320 tiles over 256 blocks'),
    (70, 3, 4, 1, 1, 0, 0, 2, 11, 13): ('wgrad 8x8 CO3', 'wgrad 8x8 chunk of 2 of 16 quads'),
}
WGRAD_DENSE_CASE = (22, 1, 7, 1, 3, 0, 0, 2, 20, 37)
DGRAD_CASES = {
    (3, 16, 4, 2, 1, 0, 0, 2, 35, 131): ('dgrad CI3', 'dgrad Cout 16: the lower bound, one full chunk', 'dgrad 2x3 coarse tiles', 'dgrad odd H and W, N 2'),
    (6, 21, 4, 2, 1, 0, 0, 1, 8, 8): ('dgrad CI6', 'dgrad second chunk nq 2, lanes 21..23 masked', 'dgrad single tile'),
}

_fp = fwd_plan
_fu = lambda c: fwd_plan(c, ws=False)      # noqa: E731
_wp = wgrad_plan
_dp = dgrad_plan
REGIMES = {
    'fwd big-tile CO3 K7': lambda c: _fp(c)['form'] == 'big-tile' and c[1] == 3 and c[2] == 7,
    'fwd big-tile CO1 K7': lambda c: _fp(c)['form'] == 'big-tile' and c[1] == 1 and c[2] == 7,
    'fwd big-tile CO3 K4': lambda c: _fp(c)['form'] == 'big-tile' and c[1] == 3 and c[2] == 4,
    'fwd big-tile CO1 K4': lambda c: _fp(c)['form'] == 'big-tile' and c[1] == 1 and c[2] == 4,
    'fwd 8-row CO3 K7': lambda c: _fp(c)['form'] == '8-row' and c[1] == 3 and c[2] == 7,
    'fwd 8-row CO1 K7': lambda c: _fp(c)['form'] == '8-row' and c[1] == 1 and c[2] == 7,
    'fwd 8-row CO3 K4': lambda c: _fp(c)['form'] == '8-row' and c[1] == 3 and c[2] == 4,
    'fwd 8-row CO1 K4': lambda c: _fp(c)['form'] == '8-row' and c[1] == 1 and c[2] == 4,
    'fwd big-tile 2x2 tiles, N 2': lambda c: _fp(c)['form'] == 'big-tile' and (_fp(c)['tiles_x'], _fp(c)['tiles_y'], c[7]) == (2, 2, 2),
    'fwd big-tile tiles_x 2, zero pad': lambda c: _fp(c)['form'] == 'big-tile' and _fp(c)['tiles_x'] == 2 and not c[5] and c[4] > 0,
    'fwd big-tile tiles_y 2, N 2': lambda c: _fp(c)['form'] == 'big-tile' and _fp(c)['tiles_y'] == 2 and c[7] == 2,
    # the last tile's staged columns reach input column ox0 - pad + 32 + k - 2 > 2W - 2, where one reflection is negative: no load
    'fwd reflect halo beyond 2W-2 in the masked last tile': lambda c: c[5] == 1 and _fp(c)['wo'] % 32 != 0 and
        (_fp(c)['tiles_x'] - 1) * 32 - c[4] + 32 + c[2] - 2 > 2 * c[9] - 2,
    'fwd plane smaller than the pad window on both sides': lambda c: c[5] == 1 and c[8] < c[2] and c[9] < c[2],
    'fwd big-tile chunk with nq 1': lambda c: _fp(c)['form'] == 'big-tile' and _fp(c)['walk'][-1][-1] == 1,
    'fwd tanh': lambda c: c[6] == 3,
    'fwd lrelu': lambda c: c[6] == 2,
    'fwd 8-row 2x2 tiles, N 2': lambda c: _fp(c)['form'] == '8-row' and (_fp(c)['tiles_x'], _fp(c)['tiles_y'], c[7]) == (2, 2, 2),
    'fwd 8-row unsplit, two chunks': lambda c: _fp(c)['form'] == '8-row' and _fp(c)['walk'] == [[8, 8]],
    'fwd 8-row ragged split: 7 chunks -> 3 3 1': lambda c: _fp(c)['form'] == '8-row' and [len(s) for s in _fp(c)['walk']] == [3, 3, 1] and
        len(_fu(c)['walk'][0]) == 7,
    'fwd 8-row last slice a 6-quad chunk': lambda c: _fp(c)['form'] == '8-row' and _fp(c)['ksplit'] > 1 and _fp(c)['walk'][-1] == [6],
    'fwd 8-row last chunk nq 2: groups 2 and 3 idle': lambda c: _fp(c)['form'] == '8-row' and _fp(c)['walk'][-1][-1] == 2 < _fp(c)['cg'],
    'fwd 8-row tiles_x 2': lambda c: _fp(c)['form'] == '8-row' and _fp(c)['tiles_x'] == 2,
    'fwd 8-row N 3, three chunks, unsplit': lambda c: _fp(c)['form'] == '8-row' and c[7] == 3 and _fp(c)['walk'] == [[8, 8, 8]],
    'fwd 8-row ragged split: 5 chunks -> 3 2': lambda c: _fp(c)['form'] == '8-row' and [len(s) for s in _fp(c)['walk']] == [3, 2] and
        len(_fu(c)['walk'][0]) == 5,
    'fwd 8-row tiles_y 2': lambda c: _fp(c)['form'] == '8-row' and _fp(c)['tiles_y'] == 2,
    'fwd 8-row even split by 4': lambda c: _fp(c)['form'] == '8-row' and [len(s) for s in _fp(c)['walk']] == [2, 2, 2, 2],
    'fwd pad 2': lambda c: c[4] == 2 and c[2] == 4,
    'wgrad 16x16 K7 CO3': lambda c: _wp(c)['form'] == '16x16' and c[2] == 7 and c[1] == 3,
    'wgrad 16x16 K7 CO1': lambda c: _wp(c)['form'] == '16x16' and c[2] == 7 and c[1] == 1,
    'wgrad 16x16 K4 CO3 (ti 19 < TI 22)': lambda c: _wp(c)['form'] == '16x16' and c[2] == 4 and c[1] == 3 and (_wp(c)['ti'], _wp(c)['TI']) == (19, 22),
    'wgrad 8x8 CO1': lambda c: _wp(c)['form'] == '8x8' and c[1] == 1,
    'wgrad 8x8 CO3': lambda c: _wp(c)['form'] == '8x8' and c[1] == 3,
    'wgrad 16x16 second trip: 300 tiles over 256 blocks': lambda c: _wp(c)['form'] == '16x16' and (_wp(c)['ntiles'], _wp(c)['nblk']) == (300, 256),
    'wgrad 8x8 second trip: 320 tiles over 256 blocks': lambda c: _wp(c)['form'] == '8x8' and (_wp(c)['ntiles'], _wp(c)['nblk']) == (320, 256),
    # a block's second tile (t + 256) lies in another sample than its first, at another position of that sample's tile grid
    'wgrad second-trip tiles cross samples': lambda c: _wp(c)['ntiles'] > _wp(c)['nblk'] and c[7] > 1 and _wp(c)['nblk'] % _wp(c)['per_sample'] != 0,
    'wgrad ragged 150 = 9 * 16 + 6': lambda c: _wp(c)['form'] == '16x16' and _wp(c)['ho'] == _wp(c)['wo'] == 150,
    'wgrad reflect': lambda c: c[5] == 1,
    'wgrad 16x16 N 2 with a ragged tile grid': lambda c: _wp(c)['form'] == '16x16' and c[7] == 2 and _wp(c)['ho'] % 16 != 0 and _wp(c)['wo'] % 16 != 0,
    'wgrad 16x16 last chunk 2 of 4 quads': lambda c: _wp(c)['form'] == '16x16' and _wp(c)['walk'][-1] == 2 and len(_wp(c)['walk']) > 1,
    'wgrad 16x16 K7 with Cin >= 64, 5 chunks': lambda c: _wp(c)['form'] == '16x16' and c[0] >= 64 and c[2] == 7 and len(_wp(c)['walk']) == 5 and
        small_image_cfg(c[0], c[7], _wp(c)['ho'], _wp(c)['wo'], 4),
    'wgrad 8x8 chunk of 2 of 16 quads': lambda c: _wp(c)['form'] == '8x8' and _wp(c)['walk'] == [16, 2],
    'dgrad CI3': lambda c: smallci_dgrad_applicable(c) and c[0] == 3,
    'dgrad CI6': lambda c: smallci_dgrad_applicable(c) and c[0] == 6,
    'dgrad Cout 16: the lower bound, one full chunk': lambda c: smallci_dgrad_applicable(c) and c[1] == 16 and _dp(c)['walk'] == [4] and
        not smallci_dgrad_applicable(c[:1] + (15,) + c[2:]),
    'dgrad 2x3 coarse tiles': lambda c: (_dp(c)['tiles_y'], _dp(c)['tiles_x']) == (2, 3),
    'dgrad odd H and W, N 2': lambda c: c[8] % 2 == 1 and c[9] % 2 == 1 and c[7] == 2,
    'dgrad second chunk nq 2, lanes 21..23 masked': lambda c: smallci_dgrad_applicable(c) and c[1] == 21 and _dp(c)['walk'] == [4, 2] and _dp(c)['masked'] == 3,
    'dgrad single tile': lambda c: (_dp(c)['tiles_y'], _dp(c)['tiles_x'], c[7]) == (1, 1, 1),
}
SECTIONS = (('fwd', FWD_CASES), ('wgrad', WGRAD_CASES), ('dgrad', DGRAD_CASES))

# E: one tiny plane per clause of the two predicates; (case, which clause it is the far side of)
FAR_CONV_CASES = [((8, 2, 7, 1, 3, 0, 0, 1, 9, 11), 'Cout 2'), ((8, 4, 4, 1, 1, 0, 0, 1, 9, 11), 'Cout 4'), ((8, 3, 5, 1, 2, 0, 0, 1, 9, 11), 'k 5'),
                  ((8, 1, 4, 2, 1, 0, 0, 1, 9, 11), 'stride 2')]
# (case, bias passed, activation passed, clause)
FAR_DGRAD_CASES = [((3, 15, 4, 2, 1, 0, 0, 1, 9, 11), 0, 0, 'Cout 15'), ((4, 16, 4, 2, 1, 0, 0, 1, 9, 11), 0, 0, 'Cin 4'),
                   ((3, 16, 4, 2, 0, 0, 0, 1, 10, 12), 0, 0, 'pad 0'), ((3, 16, 4, 2, 1, 0, 0, 1, 9, 11), 1, 0, 'bias'),
                   ((3, 16, 4, 2, 1, 0, 2, 1, 9, 11), 0, 1, 'activation')]


def dense_case(case):
    return (DENSE_CIN[case[0]],) + case[1:]


def _all_cases():
    """every geometry of B - E whose reference the GPU tests use"""
    out = list(FWD_CASES) + [dense_case(c) for c in FWD_CASES] + list(WGRAD_CASES) + list(DGRAD_CASES) + [c for c, _ in FAR_CONV_CASES]
    out += [c[:6] + (0,) + c[7:] for c, _, _, _ in FAR_DGRAD_CASES]
    return list(dict.fromkeys(out))


def _lib():
    from cat_amd import _build, _lib as L
    _build.build(verbose=False)
    return L


def _ksplit_of(L, case, ycs=None):
    """plan_fwd: ws_bytes = split * M * ycs * sizeof(float) when the plan splits the channel range, else 0"""
    n, (ho, wo) = case[7], out_hw(case)
    g = _geom(case, ycs=ycs)
    nb = int(L.query('cat_conv2d_fwd_ws_bytes', C.byref(g)))
    assert nb % (n * ho * wo * g.ycs * 4) == 0, (case, nb)
    return nb // (n * ho * wo * g.ycs * 4) or 1


def _nblk_of(L, case):
    """plan_wgrad: ws_bytes = split * Cout * K * sizeof(float), K = kh * kw * round_up(Cin, 4), split = smallco_wgrad_nblk"""
    cin, cout, k = case[:3]
    nb = int(L.query('cat_conv2d_wgrad_ws_bytes', C.byref(_geom(case))))
    assert nb % (cout * k * k * cs4(cin) * 4) == 0, (case, nb)
    return nb // (cout * k * k * cs4(cin) * 4)


# ================================================================================================ A: host tests
def test_plan_mirrors_match_the_workspace_queries():
    L = _lib()
    for case in list(FWD_CASES) + [dense_case(c) for c in FWD_CASES]:
        assert smallco_applicable(case)
        assert _ksplit_of(L, case) == fwd_plan(case)['ksplit'], case
        assert _ksplit_of(L, case, ycs=8 + cs4(case[1]) + 8) == fwd_plan(case)['ksplit'], case      # the sentinel buffer's pixel stride
    for case in WGRAD_CASES:
        assert smallco_applicable(case)
        assert _nblk_of(L, case) == wgrad_plan(case)['nblk'], case
    # both sides of the forward's 256-tile (32 x 32) and the weight gradient's 512-tile (16 x 16) thresholds, and planes well inside either
    planes = [(1, 9, 9), (2, 17, 35), (3, 64, 64), (16, 30, 30), (255, 32, 32), (256, 32, 32), (257, 20, 20), (15, 128, 128), (16, 128, 128),
              (511, 16, 16), (512, 16, 16), (2, 255, 240), (2, 256, 256), (1, 512, 512)]
    splits, forms = set(), set()
    for cin in (16, 63, 64, 70, 160, 214, 256, 1024):
        for k in (4, 7):
            for cout in (1, 3):
                for n, h, w in planes:
                    case = (cin, cout, k, 1, (k - 1) // 2, 0, 0, n, h, w)
                    ho, wo = out_hw(case)
                    ks, nblk = _ksplit_of(L, case), _nblk_of(L, case)
                    assert ks == smallco_fwd_ksplit(cin, n, ho, wo) == fwd_plan(case)['ksplit'], (case, ks)
                    assert nblk == smallco_wgrad_nblk(cin, n, ho, wo, k) == wgrad_plan(case)['nblk'], (case, nblk)
                    splits.add(ks > 1)
                    forms.add((fwd_plan(case)['form'], wgrad_plan(case)['form']))
    assert splits == {False, True} and len(forms) == 4, (splits, forms)      # the sweep reaches every form of both passes


def test_every_case_stands_for_the_regimes_it_declares():
    declared = {}
    for section, cases in SECTIONS:
        for case, names in cases.items():
            assert names, case
            for name in names:
                assert name.split()[0] == section and name in REGIMES, (case, name)
                assert REGIMES[name](case), 'case %s has left the regime %r' % (case, name)
                declared.setdefault(name, []).append(case)
    assert set(declared) == set(REGIMES), sorted(set(REGIMES) - set(declared))
    for section, cases in SECTIONS:
        for case, names in cases.items():
            assert any(declared[name] == [case] for name in names), 'case %s is the only declarer of none of its regimes' % (case,)
    # the cases the other tables draw from
    assert set(DENSE_CIN) == {c[0] for c in FWD_CASES} and all(v % 4 != 0 for v in DENSE_CIN.values())
    for case in FWD_CASES:
        a, b = fwd_plan(case), fwd_plan(dense_case(case))
        assert (a['form'], a['tiles_x'], a['tiles_y']) == (b['form'], b['tiles_x'], b['tiles_y']), case      # (the split may differ: 98 channels are 4 chunks)
    assert all(c in FWD_CASES for c in NULL_BIAS_CASES) and {fwd_plan(c)['form'] for c in NULL_BIAS_CASES} == {'big-tile', '8-row'}
    assert WGRAD_DENSE_CASE in WGRAD_CASES and WGRAD_DENSE_CASE[0] % 4 != 0
    for case, clause in FAR_CONV_CASES:
        assert not smallco_applicable(case), clause
    near = (3, 16, 4, 2, 1, 0, 0, 1, 9, 11)
    assert smallci_dgrad_applicable(near)
    for case, bias, act, clause in FAR_DGRAD_CASES:
        assert smallci_dgrad_applicable(case) == bool(bias or act), clause      # bias and activation are plan_dgrad's clauses, not the predicate's
        assert sum(a != b for a, b in zip(case[:6], near[:6])) == (0 if bias or act else 1), clause


def parse_instantiations(text):
    """the template argument lists of the dispatch text: launch_fwd's two fwd_kernel forms x launch_fwd_v's two WVEC arms x smallco_fwd's
    (CO, KW) arms, and the literal lists of smallco_wgrad and smallci_dgrad"""
    forms = re.findall(r'fwd_kernel<CO, (\d+), (\d+), (\d+), KW, WVEC><<<', text)
    wvec = re.findall(r'launch_fwd<CO, KW, (true|false)>\(', text)
    cokw = re.findall(r'launch_fwd_v<(\d+), (\d+)>\(', text)
    wgrad = re.findall(r'wgrad_kernel<(\d+), (\d+), (\d+), (\d+)><<<', text)
    dgrad = re.findall(r'dgrad_s2_kernel<(\d+), (\d+)><<<', text)
    assert len(forms) + len(wgrad) + len(dgrad) == text.count('<<<'), 'a launch this parser does not know'
    assert len(re.findall(r'__global__', text)) == 3 and len(wvec) == len(set(wvec)) and len(cokw) == len(set(cokw))
    out = {('fwd_kernel', int(co), int(th), int(cg), int(ckq), int(kw), int(v == 'true')) for th, cg, ckq in forms for v in wvec for co, kw in cokw}
    out |= {('wgrad_kernel',) + tuple(int(v) for v in m) for m in wgrad}
    out |= {('dgrad_s2_kernel',) + tuple(int(v) for v in m) for m in dgrad}
    return out


def claimed_instantiations():
    out = {fwd_plan(c)['inst'] for c in FWD_CASES} | {fwd_plan(dense_case(c), dense=True)['inst'] for c in FWD_CASES}
    return out | {wgrad_plan(c)['inst'] for c in WGRAD_CASES} | {dgrad_plan(c)['inst'] for c in DGRAD_CASES}


def test_every_instantiation_has_a_case():
    compiled, claimed = parse_instantiations(open(SMALLCO_SRC).read()), claimed_instantiations()
    assert compiled == claimed, (sorted(compiled - claimed), sorted(claimed - compiled))
    assert len(compiled) == 20


def _twin32(case):
    """_reference of test_conv_variants_gpu.py in float32: the same inputs through float32 ATen"""
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    x, wt, b, gy = _reference(case)[:4]
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, wt, b))
    xp = F.pad(xr, (pad,) * 4, mode='reflect') if reflect and pad else xr
    yr = _act64(F.conv2d(xp, wr, br, stride=stride, padding=0 if reflect else pad), act)
    yr.backward(gy)
    return yr.detach(), xr.grad, wr.grad, br.grad


@pytest.mark.parametrize('case', _all_cases(), ids=_ids)
def test_float32_aten_reaches_a_tenth_of_the_bar(case):
    """the bars of B - E are reachable: float32 ATen on the host agrees with the float64 reference within TOL / 10, over the whole tensor and
    per channel, for every geometry the GPU tests use"""
    y, dx, dw, db = _reference(case)[4:]
    y32, dx32, dw32, db32 = _twin32(case)
    figs = {'y': rel(y32, y), 'dx': rel(dx32, dx), 'dw': rel(dw32, dw), 'db': rel(db32, db), 'y/channel': chan_rel(y32, y, False),
            'dx/channel': chan_rel(dx32, dx, False), 'dw/channel': chan_rel(dw32.transpose(0, 1), dw.transpose(0, 1), False)}
    print(case, figs)
    assert max(figs.values()) < TOL / 10, figs


# ================================================================================================ GPU helpers
def _note(section, *figs):
    MAXREL[section] = max(MAXREL.get(section, 0.0), *figs)
    print('largest so far', section, '%.2e' % MAXREL[section])


def _held(section, what, got, want, per_dw=False):
    """rel() over the whole tensor and per channel (dim 1; dim 0 of a weight gradient), both printed, both < TOL"""
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    assert bool(torch.isfinite(got).all()), what
    d = rel(got, want)
    dc = chan_rel(got.transpose(0, 1), want.transpose(0, 1), False) if per_dw else chan_rel(got, want, False)
    print(what, 'rel', d, 'per channel', dc)
    _note(section, d, dc)
    assert d < TOL and dc < TOL, (what, d, dc)


def _slice_of(buf, c0, c):
    return buf.cpu()[..., c0:c0 + c].permute(0, 3, 1, 2)


def _fwd64(case, x, wt, b):
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    xp = F.pad(x.double(), (pad,) * 4, mode='reflect') if reflect and pad else x.double()
    return _act64(F.conv2d(xp, wt.double(), None if b is None else b.double(), stride=stride, padding=0 if reflect else pad), act)


def _run_fwd(dev, case, c0, wptr, bg, want, what, wcs=None, with_ws=True):
    """one forward through cat_conv2d_fwd_ws (NaN workspace) or cat_conv2d_fwd into the channel slice at lane c0 of a sentinel buffer: the
    family once, the slice and everything around it checked; returns the result as [N, Cout, Ho, Wo] on the host"""
    from cat_amd import _lib as L, ops
    cin, cout = case[:2]
    x = _reference(case)[0]
    xg = ops.to_nhwc(x.to(dev))
    cw, cs = cs4(cout) + 4, c0 + cs4(cout) + 8
    g = _geom(case, ycs=cs, ycw=cw, with_act=True)
    if wcs is not None:
        g.wcs = wcs
    flat, buf = _sentinel_buffer(case[7], g.Ho, g.Wo, cs, dev)
    yptr = C.c_void_p(buf.data_ptr() + 4 * c0)
    nb = int(L.query('cat_conv2d_fwd_ws_bytes', C.byref(g)))
    split = fwd_plan(case)['ksplit']
    assert nb == (split * case[7] * g.Ho * g.Wo * cs * 4 if split > 1 else 0), (nb, split)
    ws = _nan_ws(nb, dev)
    if with_ws:
        call = lambda: L.call('cat_conv2d_fwd_ws', C.byref(g), ops._p(xg), wptr, ops._p(bg), yptr, ops._p(ws), ops._stream())      # noqa: E731
    else:
        call = lambda: L.call('cat_conv2d_fwd', C.byref(g), ops._p(xg), wptr, ops._p(bg), yptr, ops._stream())      # noqa: E731
    _, fam = _profiled(call)
    assert fam.get('conv_fwd_smallco', 0) == 1, fam
    _check_slice(flat, buf, c0, cout, cw, want, what)
    got = _slice_of(buf, c0, cout)
    _held('B', what, got, want)
    return got


# ================================================================================================ B: forward
@pytest.mark.gpu
@pytest.mark.parametrize('c0', [0, 8])
@pytest.mark.parametrize('case', list(FWD_CASES), ids=_ids)
def test_fwd_slice_output_with_and_without_a_workspace(dev, case, c0):
    from cat_amd import ops
    x, wt, b, gy, yr = _reference(case)[:5]
    wg, bg = _padded_weight(wt, dev), b.to(dev)
    assert ops.weight_wcs(wg) == cs4(case[0])
    y_ws = _run_fwd(dev, case, c0, ops._p(wg), bg, yr, ('fwd ws', case, c0))
    if fwd_plan(case)['ksplit'] > 1:
        y_1 = _run_fwd(dev, case, c0, ops._p(wg), bg, yr, ('fwd unsplit', case, c0), with_ws=False)
        _held('B', ('fwd split against unsplit', case, c0), y_ws, y_1.double())


@pytest.mark.gpu
@pytest.mark.parametrize('c0', [0, 8])
@pytest.mark.parametrize('case', NULL_BIAS_CASES, ids=_ids)
def test_fwd_null_bias(dev, case, c0):
    from cat_amd import ops
    x, wt = _reference(case)[:2]
    wg = _padded_weight(wt, dev)
    want = _fwd64(case, x, wt, None)
    _run_fwd(dev, case, c0, ops._p(wg), None, want, ('fwd NULL bias', case, c0))
    if fwd_plan(case)['ksplit'] > 1:
        _run_fwd(dev, case, c0, ops._p(wg), None, want, ('fwd NULL bias unsplit', case, c0), with_ws=False)


@pytest.mark.gpu
@pytest.mark.parametrize('c0', [0, 8])
@pytest.mark.parametrize('case', [dense_case(c) for c in FWD_CASES], ids=_ids)
def test_fwd_dense_weights(dev, case, c0):
    """wcs = Cin with Cin % 4 != 0 (the WVEC = false instantiations): the filter is [Cout][k][k][Cin] with 64 NaNs right behind it, so the
    clamped reads of a tap's last quad must stay inside the tensor for y to be finite"""
    cin, cout, k = case[:3]
    x, wt, b, gy, yr = _reference(case)[:5]
    store = torch.cat([wt.permute(0, 2, 3, 1).reshape(-1), torch.full((64,), NAN)]).to(dev)
    assert store.numel() == cout * k * k * cin + 64 and cin % 4 != 0
    bg = b.to(dev)
    wptr = C.c_void_p(store.data_ptr())
    y_ws = _run_fwd(dev, case, c0, wptr, bg, yr, ('fwd dense', case, c0), wcs=cin)
    if fwd_plan(case)['ksplit'] > 1:
        y_1 = _run_fwd(dev, case, c0, wptr, bg, yr, ('fwd dense unsplit', case, c0), wcs=cin, with_ws=False)
        _held('B', ('fwd dense split against unsplit', case, c0), y_ws, y_1.double())


# ================================================================================================ C: weight gradient
def _run_wgrad(dev, case, accumulate, dense):
    from cat_amd import _lib as L, ops
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    assert act == 0
    x, wt, b, gy, _, _, dwr, _ = _reference(case)
    xg, gyg = ops.to_nhwc(x.to(dev)), ops.to_nhwc(gy.to(dev))
    wcs = cin if dense else cs4(cin)
    flat = torch.full((cout * k * k * wcs + 64,), SENTINEL, device=dev)
    raw = flat[:cout * k * k * wcs].view(cout, k, k, wcs)
    raw.zero_()
    dw = raw[..., :cin].permute(0, 3, 1, 2)      # the [Cout, Cin, k, k] view of padded_weight_like, over storage with sentinels behind it
    if accumulate:
        prev = detfill.normal((cout, cin, k, k), 9, float(dwr.abs().max()))      # as large as the gradient: neither term hides the other
        dw.copy_(prev)
        want = prev.double() + dwr
    else:
        dw.fill_(NAN)      # the real lanes only: the padding lanes [Cin, wcs) stay 0.0
        want = dwr
    g = _geom(case)
    g.wcs = wcs
    nb = int(L.query('cat_conv2d_wgrad_ws_bytes', C.byref(g)))
    assert nb == wgrad_plan(case)['nblk'] * cout * k * k * cs4(cin) * 4
    ws = _nan_ws(nb, dev)
    _, fam = _profiled(lambda: L.call('cat_conv2d_wgrad', C.byref(g), ops._p(xg), ops._p(gyg), ops._p(raw), accumulate, ops._p(ws), ops._stream()))
    assert fam.get('conv_wgrad_smallco', 0) == 1, fam
    _held('C', ('wgrad', case, accumulate, 'dense' if dense else 'padded'), dw.cpu(), want, per_dw=True)
    pad_lanes = raw.cpu()[..., cin:]
    assert pad_lanes.numel() == cout * k * k * (wcs - cin) and bool((pad_lanes == 0.0).all())
    assert bool((flat[-64:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize('accumulate', [1, 0])
@pytest.mark.parametrize('case', list(WGRAD_CASES), ids=_ids)
def test_wgrad_accumulate_and_fresh_write(dev, case, accumulate):
    _run_wgrad(dev, case, accumulate, dense=False)


@pytest.mark.gpu
@pytest.mark.parametrize('accumulate', [1, 0])
def test_wgrad_into_a_dense_gradient(dev, accumulate):
    """dw as a dense [Cout][49][22] tensor (wcs = Cin, Cin % 4 != 0): the reduce writes Cin lanes per tap and nothing behind the tensor"""
    _run_wgrad(dev, WGRAD_DENSE_CASE, accumulate, dense=True)


# ================================================================================================ D: the first layer's image gradient
def _dy_with_marked_padding(gy, cout, dev, value=1.0e3):
    """dy as an NHWC activation whose padding lanes [Cout, round_up(Cout, 4)) hold `value` instead of 0.0"""
    from cat_amd import ops
    gyg = ops.to_nhwc(gy.to(dev))
    n, _, ho, wo = gyg.shape
    if cs4(cout) > cout:
        assert ops.act_cs(gyg) == cs4(cout)
        torch.as_strided(gyg, (n, cs4(cout), ho, wo), gyg.stride())[:, cout:] = value
    return gyg


def _run_dgrad(dev, case, c0, with_ws, mark_padding, bias=None, want=None, family='conv_dgrad_smallci', section='D'):
    from cat_amd import _lib as L, ops
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    assert not reflect
    x, wt, b, gy, _, dxr, _, _ = _reference(case[:6] + (0,) + case[7:])
    want = dxr if want is None else want
    wg = _padded_weight(wt, dev)
    gyg = _dy_with_marked_padding(gy, cout, dev) if mark_padding else ops.to_nhwc(gy.to(dev))
    cw, cs = cs4(cin) + 4, c0 + cs4(cin) + 8
    g = _geom(case, with_act=True)
    flat, buf = _sentinel_buffer(n, h, w, cs, dev)
    dxptr = C.c_void_p(buf.data_ptr() + 4 * c0)
    assert int(L.query('cat_conv2d_dgrad_ws_bytes', C.byref(g), cs)) == 0      # stride 2: the plan never splits K
    ws = _nan_ws(0, dev)
    if with_ws:
        call = lambda: L.call('cat_conv2d_dgrad_ws', C.byref(g), ops._p(gyg), ops._p(wg), ops._p(bias), dxptr, cs, cw, ops._p(ws), ops._stream())      # noqa: E731
    else:
        call = lambda: L.call('cat_conv2d_dgrad', C.byref(g), ops._p(gyg), ops._p(wg), ops._p(bias), dxptr, cs, cw, ops._stream())      # noqa: E731
    _, fam = _profiled(call)
    what = ('dgrad', case, c0, 'ws' if with_ws else 'no ws', family)
    if section == 'D':
        assert fam.get(family, 0) == 1, fam
    else:
        assert 'conv_dgrad_smallci' not in fam and sum(v for f, v in fam.items() if f.startswith(family)) == 1, fam
    _check_slice(flat, buf, c0, cin, cw, want, what)
    _held(section, what, _slice_of(buf, c0, cin), want)


@pytest.mark.gpu
@pytest.mark.parametrize('with_ws', [True, False], ids=['ws', 'no-ws'])
@pytest.mark.parametrize('c0', [0, 8])
@pytest.mark.parametrize('case', list(DGRAD_CASES), ids=_ids)
def test_dgrad_slice_output(dev, case, c0, with_ws):
    _run_dgrad(dev, case, c0, with_ws, mark_padding=True)


# ================================================================================================ E: the predicates' far sides
@pytest.mark.gpu
@pytest.mark.parametrize('case,clause', FAR_CONV_CASES, ids=lambda v: v.replace(' ', '-') if isinstance(v, str) else _ids(v))
def test_far_side_of_smallco_applicable(dev, case, clause):
    from cat_amd import _lib as L, ops
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    x, wt, b, gy, yr, _, dwr, _ = _reference(case)
    xg, wg, bg, gyg = ops.to_nhwc(x.to(dev)), _padded_weight(wt, dev), b.to(dev), ops.to_nhwc(gy.to(dev))
    g = _geom(case)
    y = ops.empty_act(n, cout, g.Ho, g.Wo, dev)
    y.fill_(NAN)
    _, fam = _profiled(lambda: L.call('cat_conv2d_fwd', C.byref(g), ops._p(xg), ops._p(wg), ops._p(bg), ops._p(y), ops._stream()))
    assert fam and not any('smallco' in f for f in fam), fam
    _held('E', ('far fwd', clause, case), y.cpu(), yr)
    dw = ops.padded_weight_like((cout, cin, k, k), dev)
    dw.fill_(NAN)
    ws = _nan_ws(L.query('cat_conv2d_wgrad_ws_bytes', C.byref(g)), dev)
    _, fam = _profiled(lambda: L.call('cat_conv2d_wgrad', C.byref(g), ops._p(xg), ops._p(gyg), ops._p(dw), 0, ops._p(ws), ops._stream()))
    assert fam and not any('smallco' in f for f in fam), fam
    _held('E', ('far wgrad', clause, case), dw.cpu(), dwr, per_dw=True)


@pytest.mark.gpu
@pytest.mark.parametrize('case,bias,act,clause', FAR_DGRAD_CASES, ids=lambda v: v.replace(' ', '-') if isinstance(v, str) else (_ids(v) if isinstance(v, tuple) else str(v)))
def test_far_side_of_smallci_dgrad_applicable(dev, case, bias, act, clause):
    """the generic tile takes the layer (dx = act(conv^T(dy, w) + bias), as the transposed convolution's forward uses the entry point)"""
    cin, cout = case[:2]
    dxr = _reference(case[:6] + (0,) + case[7:])[5]
    bt = detfill.normal((cin,), 11, 0.5) if bias else None
    want = _act64(dxr + (bt.double().view(1, -1, 1, 1) if bias else 0.0), case[6])
    family = 'conv_dgrad_'      # a tile of CONV_TILES, whichever row the plan picks
    _run_dgrad(dev, case, 8, False, mark_padding=False, bias=None if bt is None else bt.to(dev), want=want, family=family, section='E')
