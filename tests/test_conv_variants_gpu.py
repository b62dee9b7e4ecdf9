"""Every tile variant of the implicit-GEMM convolution (csrc/conv_igemm.hip and the producers it dispatches to) in the PRODUCTION weight
layout -- ops.padded_weight_like storage, wcs = round_up(Cin, 4) -- against float64 ATen on the host, plus the two C-ABI contracts no other
kernel test checks: channel-slice output writes (ycw / dxcw below the pixel stride) and accumulate = 1 of the weight gradient.

A (host): the ROW(...) lines of CONV_TILES / WGRAD_TILES are parsed from the source text; the profiler family names the dispatch can emit
          must equal the keys of VARIANT_CASES exactly, so a new tile row without a parity case fails without a GPU.
B (GPU):  one Conv2dFn forward + backward per case with the profiler on and NaNs in the cached workspace; the family the case stands for must
          have been recorded exactly once (a moved dispatch fails the case instead of silently testing another kernel), then y / dx / dw / db
          parity at TOL.
C (GPU):  direct C-ABI calls with a NaN-filled workspace, a sentinel-filled wider output (slice and offset writes) and NaN / pre-filled
          weight-gradient buffers.
D (GPU):  cat_conv2d_fwd_rect (the FID network's 1x7 / 7x1 / 1x3 / 3x1 filters) into a channel slice.

Every bar is TOL = 1e-4 with rel() of test_kernels_gpu.py, or exact equality for zero and sentinel lanes."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detfill
from test_kernels_gpu import TOL, _families, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IGEMM_SRC = os.path.join(ROOT, 'cat_amd', 'csrc', 'conv_igemm.hip')
SENTINEL = 7.0

# A case is (cin, cout, k, stride, pad, reflect, act, N, H, W) for Conv2dFn, or ('T', cin, cout, N, H, W) for ConvTranspose2dFn (3 x 3, stride 2,
# pad 1, output_padding 1), whose forward is the only caller of cat_conv2d_dgrad on a layer the transposed-filter tile would otherwise take.
# A case is listed under every family it records, so each direction of each shape is pinned to its kernel.
VARIANT_CASES = {
    'conv_fwd_2x1x4x1': [(20, 8, 1, 1, 0, 0, 0, 1, 16, 16), (20, 16, 4, 1, 1, 0, 0, 1, 16, 16), (3, 13, 4, 1, 1, 0, 0, 1, 9, 11),
        (3, 16, 7, 1, 3, 1, 0, 2, 20, 24), (5, 5, 3, 2, 1, 0, 0, 1, 7, 9)],
    'conv_fwd_2x2x4x1': [(3, 17, 4, 2, 1, 0, 0, 1, 9, 11), (6, 20, 4, 2, 1, 0, 0, 1, 33, 37)],
    'conv_fwd_2x3x4x1': [(8, 40, 1, 1, 0, 0, 0, 1, 16, 16), (3, 35, 1, 1, 0, 0, 0, 1, 9, 11), (3, 35, 1, 1, 0, 0, 0, 1, 33, 37),
        (3, 35, 3, 1, 1, 0, 0, 2, 64, 64), (3, 35, 5, 1, 2, 1, 0, 2, 64, 64), (20, 35, 3, 1, 1, 0, 0, 2, 64, 64)],
    'conv_fwd_2x4x4x1': [(3, 54, 1, 1, 0, 0, 2, 1, 9, 11), (3, 54, 1, 1, 0, 0, 0, 1, 33, 37), (3, 64, 4, 2, 1, 0, 2, 2, 70, 50)],
    'conv_fwd_2x6x4x1': [(8, 80, 1, 1, 0, 0, 0, 1, 16, 16), (3, 77, 1, 1, 0, 0, 0, 1, 9, 11), (3, 77, 1, 1, 0, 0, 0, 1, 33, 37),
        (3, 77, 1, 1, 0, 0, 0, 2, 64, 64)],
    'conv_fwd_4x1x4x1': [(8, 8, 1, 1, 0, 0, 0, 3, 256, 256), (20, 8, 1, 1, 0, 0, 0, 3, 256, 256), (3, 7, 1, 1, 0, 0, 0, 3, 257, 255)],
    'conv_fwd_4x2x4x1': [(8, 24, 1, 1, 0, 0, 2, 3, 256, 256), (3, 17, 1, 1, 0, 0, 0, 3, 257, 255)],
    'conv_fwd_4x4x2x2': [(3, 100, 1, 1, 0, 0, 0, 1, 9, 11), (3, 100, 1, 1, 0, 0, 0, 1, 33, 37), (7, 512, 5, 1, 2, 0, 0, 4, 4, 8),
        (6, 128, 4, 2, 1, 0, 2, 2, 32, 32)],
    'conv_fwd_smallco': [(42, 1, 4, 1, 1, 0, 2, 1, 9, 11), (16, 3, 7, 1, 3, 1, 3, 1, 18, 18)],
    'conv_fwd32_2x1x4x1': [(54, 13, 1, 1, 0, 0, 0, 3, 9, 11), (130, 7, 1, 1, 0, 0, 0, 1, 128, 130), (100, 16, 1, 1, 0, 0, 0, 1, 9, 11),
        (42, 7, 3, 1, 1, 0, 0, 2, 64, 64)],
    'conv_fwd32_2x2x4x1': [(130, 17, 1, 1, 0, 0, 0, 1, 8, 8), (13, 17, 1, 1, 0, 0, 0, 1, 9, 11), (100, 32, 1, 1, 0, 0, 0, 1, 9, 11),
        (42, 17, 3, 1, 1, 0, 0, 2, 64, 64)],
    'conv_fwd32_2x3x4x1': [(30, 35, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_fwd32_2x4x4x1': [(13, 54, 5, 1, 2, 1, 0, 2, 16, 12), (77, 60, 1, 1, 0, 0, 0, 4, 64, 64), (13, 54, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_fwd32_2x6x4x1': [(16, 80, 1, 1, 0, 0, 0, 1, 16, 16), (13, 77, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_fwd32_4x1x4x1': [(16, 8, 1, 1, 0, 0, 0, 3, 256, 256), (13, 7, 1, 1, 0, 0, 0, 3, 257, 255), (30, 7, 1, 1, 0, 0, 0, 3, 257, 255)],
    'conv_fwd32_4x2x4x1': [(16, 24, 1, 1, 0, 0, 0, 3, 256, 256), (16, 32, 3, 2, 1, 0, 0, 1, 896, 896), (13, 30, 3, 2, 1, 0, 0, 1, 887, 889)],
    'conv_fwd32_4x4x2x2': [(42, 256, 3, 1, 1, 1, 0, 1, 12, 12), (13, 100, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_fwd32sk_2x1x4x1': [(64, 16, 4, 1, 1, 0, 0, 1, 16, 16), (54, 7, 5, 1, 2, 1, 0, 2, 16, 16), (130, 7, 3, 2, 1, 0, 0, 1, 9, 11),
        (30, 13, 4, 1, 1, 0, 0, 1, 9, 11), (42, 13, 4, 1, 1, 0, 0, 1, 9, 11), (54, 13, 4, 1, 1, 0, 2, 1, 9, 11), (77, 13, 4, 1, 1, 0, 0, 1, 9, 11),
        (130, 13, 4, 1, 1, 0, 0, 1, 9, 11), (42, 7, 5, 1, 2, 1, 0, 2, 64, 64)],
    'conv_fwd32sk_2x2x4x1': [(77, 17, 3, 2, 1, 0, 0, 1, 9, 11)],
    'conv_fwd32sk_2x3x4x1': [(30, 35, 4, 2, 1, 0, 2, 1, 9, 11)],
    'conv_fwd32sk_2x4x4x1': [(30, 54, 4, 2, 1, 0, 0, 1, 9, 11)],
    'conv_fwd32sk_2x6x4x1': [(32, 80, 4, 2, 1, 0, 0, 1, 16, 16), (30, 77, 4, 2, 1, 0, 0, 1, 9, 11)],
    'conv_fwd32sk_4x4x2x2': [(82, 100, 3, 1, 1, 0, 2, 1, 10, 10), (170, 1024, 3, 1, 1, 0, 0, 2, 8, 16), (512, 1024, 4, 1, 1, 0, 0, 1, 6, 7),
        (30, 100, 4, 2, 1, 0, 0, 1, 9, 11)],
    'conv_fwd32d_4x4x2x2': [(32, 100, 1, 1, 0, 0, 2, 1, 9, 11), (128, 100, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_dgrad_2x1x4x1': [(8, 40, 1, 1, 0, 0, 0, 1, 16, 16), (8, 80, 1, 1, 0, 0, 0, 1, 16, 16), (16, 80, 1, 1, 0, 0, 0, 1, 16, 16),
        (16, 3, 7, 1, 3, 1, 3, 1, 18, 18), (3, 100, 1, 1, 0, 0, 0, 1, 9, 11), (3, 54, 1, 1, 0, 0, 2, 1, 9, 11), (3, 35, 1, 1, 0, 0, 0, 1, 9, 11),
        (13, 17, 1, 1, 0, 0, 0, 1, 9, 11), (3, 77, 1, 1, 0, 0, 0, 1, 9, 11), (13, 54, 1, 1, 0, 0, 0, 1, 9, 11), (13, 77, 1, 1, 0, 0, 0, 1, 9, 11),
        (13, 100, 1, 1, 0, 0, 0, 1, 9, 11), (3, 35, 1, 1, 0, 0, 0, 1, 33, 37), (3, 54, 1, 1, 0, 0, 0, 1, 33, 37), (3, 77, 1, 1, 0, 0, 0, 1, 33, 37),
        (3, 100, 1, 1, 0, 0, 0, 1, 33, 37), (3, 77, 1, 1, 0, 0, 0, 2, 64, 64), (5, 5, 3, 2, 1, 0, 0, 1, 7, 9)],
    'conv_dgrad_2x2x4x1': [(32, 80, 4, 2, 1, 0, 0, 1, 16, 16), (20, 8, 1, 1, 0, 0, 0, 1, 16, 16), (30, 35, 1, 1, 0, 0, 0, 1, 9, 11),
        (30, 35, 4, 2, 1, 0, 2, 1, 9, 11), (30, 54, 4, 2, 1, 0, 0, 1, 9, 11), (32, 100, 1, 1, 0, 0, 2, 1, 9, 11), (30, 77, 4, 2, 1, 0, 0, 1, 9, 11),
        (30, 100, 4, 2, 1, 0, 0, 1, 9, 11)],
    'conv_dgrad_2x3x4x1': [(42, 1, 4, 1, 1, 0, 2, 1, 9, 11), (42, 7, 3, 1, 1, 0, 0, 2, 64, 64), (42, 17, 3, 1, 1, 0, 0, 2, 64, 64),
        (42, 7, 5, 1, 2, 1, 0, 2, 64, 64)],
    'conv_dgrad_2x4x4x1': [(54, 7, 5, 1, 2, 1, 0, 2, 16, 16), (54, 13, 1, 1, 0, 0, 0, 3, 9, 11)],
    'conv_dgrad_2x6x4x1': [(77, 60, 1, 1, 0, 0, 0, 4, 64, 64), (77, 17, 3, 2, 1, 0, 0, 1, 9, 11)],
    'conv_dgrad_4x1x4x1': [(8, 8, 1, 1, 0, 0, 0, 3, 256, 256), (8, 24, 1, 1, 0, 0, 2, 3, 256, 256), (16, 8, 1, 1, 0, 0, 0, 3, 256, 256),
        (16, 24, 1, 1, 0, 0, 0, 3, 256, 256), (16, 32, 3, 2, 1, 0, 0, 1, 896, 896), (13, 30, 3, 2, 1, 0, 0, 1, 887, 889),
        (3, 7, 1, 1, 0, 0, 0, 3, 257, 255), (3, 17, 1, 1, 0, 0, 0, 3, 257, 255), (13, 7, 1, 1, 0, 0, 0, 3, 257, 255)],
    'conv_dgrad_4x2x4x1': [(20, 8, 1, 1, 0, 0, 0, 3, 256, 256), (30, 7, 1, 1, 0, 0, 0, 3, 257, 255)],
    'conv_dgrad_4x4x2x2': [(130, 17, 1, 1, 0, 0, 0, 1, 8, 8), (130, 7, 1, 1, 0, 0, 0, 1, 128, 130), (130, 7, 3, 2, 1, 0, 0, 1, 9, 11),
        (128, 100, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_dgrad_smallci': [(3, 17, 4, 2, 1, 0, 0, 1, 9, 11), (3, 64, 4, 2, 1, 0, 2, 2, 70, 50), (6, 20, 4, 2, 1, 0, 0, 1, 33, 37),
        (6, 128, 4, 2, 1, 0, 2, 2, 32, 32)],
    'conv_dgradsk_2x1x4x1': [(13, 54, 5, 1, 2, 1, 0, 2, 16, 12), (3, 13, 4, 1, 1, 0, 0, 1, 9, 11), (3, 35, 3, 1, 1, 0, 0, 2, 64, 64),
        (3, 35, 5, 1, 2, 1, 0, 2, 64, 64), (3, 16, 7, 1, 3, 1, 0, 2, 20, 24), (7, 512, 5, 1, 2, 0, 0, 4, 4, 8)],
    'conv_dgradsk_2x2x4x1': [(20, 16, 4, 1, 1, 0, 0, 1, 16, 16), (30, 13, 4, 1, 1, 0, 0, 1, 9, 11), (20, 35, 3, 1, 1, 0, 0, 2, 64, 64)],
    'conv_dgradsk_2x3x4x1': [(42, 256, 3, 1, 1, 1, 0, 1, 12, 12), (42, 13, 4, 1, 1, 0, 0, 1, 9, 11)],
    'conv_dgradsk_2x4x4x1': [(64, 16, 4, 1, 1, 0, 0, 1, 16, 16), (54, 13, 4, 1, 1, 0, 2, 1, 9, 11)],
    'conv_dgradsk_2x6x4x1': [(82, 100, 3, 1, 1, 0, 2, 1, 10, 10), (77, 13, 4, 1, 1, 0, 0, 1, 9, 11)],
    'conv_dgradsk_4x4x2x2': [(170, 1024, 3, 1, 1, 0, 0, 2, 8, 16), (512, 1024, 4, 1, 1, 0, 0, 1, 6, 7), (130, 13, 4, 1, 1, 0, 0, 1, 9, 11)],
    'conv_dgrad32_4x4x2x2': [(100, 16, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_dgrad32d_4x4x2x2': [('T', 64, 128, 1, 5, 7)],
    'conv_dgrad32dt_4x4x2x2': [(100, 32, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_wgrad_1x4x1x4': [(20, 8, 1, 1, 0, 0, 0, 1, 16, 16), (20, 16, 4, 1, 1, 0, 0, 1, 16, 16), (64, 16, 4, 1, 1, 0, 0, 1, 16, 16),
        (54, 7, 5, 1, 2, 1, 0, 2, 16, 16), (54, 13, 1, 1, 0, 0, 0, 3, 9, 11), (3, 13, 4, 1, 1, 0, 0, 1, 9, 11), (130, 7, 3, 2, 1, 0, 0, 1, 9, 11),
        (100, 16, 1, 1, 0, 0, 0, 1, 9, 11), (30, 13, 4, 1, 1, 0, 0, 1, 9, 11), (42, 13, 4, 1, 1, 0, 0, 1, 9, 11), (54, 13, 4, 1, 1, 0, 2, 1, 9, 11),
        (77, 13, 4, 1, 1, 0, 0, 1, 9, 11), (130, 13, 4, 1, 1, 0, 0, 1, 9, 11), (3, 16, 7, 1, 3, 1, 0, 2, 20, 24), (5, 5, 3, 2, 1, 0, 0, 1, 7, 9)],
    'conv_wgrad_2x4x1x4': [(16, 32, 3, 2, 1, 0, 0, 1, 896, 896), (130, 17, 1, 1, 0, 0, 0, 1, 8, 8), (13, 30, 3, 2, 1, 0, 0, 1, 887, 889),
        (3, 17, 4, 2, 1, 0, 0, 1, 9, 11), (77, 17, 3, 2, 1, 0, 0, 1, 9, 11), (13, 17, 1, 1, 0, 0, 0, 1, 9, 11), (100, 32, 1, 1, 0, 0, 0, 1, 9, 11),
        (6, 20, 4, 2, 1, 0, 0, 1, 33, 37)],
    'conv_wgrad_3x4x1x4': [(8, 40, 1, 1, 0, 0, 0, 1, 16, 16), (30, 35, 1, 1, 0, 0, 0, 1, 9, 11), (3, 35, 1, 1, 0, 0, 0, 1, 9, 11),
        (30, 35, 4, 2, 1, 0, 2, 1, 9, 11), (3, 35, 1, 1, 0, 0, 0, 1, 33, 37)],
    'conv_wgrad_4x4x1x4': [(13, 54, 5, 1, 2, 1, 0, 2, 16, 12), (3, 54, 1, 1, 0, 0, 2, 1, 9, 11), (13, 54, 1, 1, 0, 0, 0, 1, 9, 11),
        (30, 54, 4, 2, 1, 0, 0, 1, 9, 11), (3, 54, 1, 1, 0, 0, 0, 1, 33, 37), (3, 64, 4, 2, 1, 0, 2, 2, 70, 50)],
    'conv_wgrad_4x4x2x2': [(42, 256, 3, 1, 1, 1, 0, 1, 12, 12), (82, 100, 3, 1, 1, 0, 2, 1, 10, 10), (170, 1024, 3, 1, 1, 0, 0, 2, 8, 16),
        (3, 100, 1, 1, 0, 0, 0, 1, 9, 11), (13, 100, 1, 1, 0, 0, 0, 1, 9, 11), (32, 100, 1, 1, 0, 0, 2, 1, 9, 11),
        (3, 100, 1, 1, 0, 0, 0, 1, 33, 37), (30, 100, 4, 2, 1, 0, 0, 1, 9, 11), (7, 512, 5, 1, 2, 0, 0, 4, 4, 8), (6, 128, 4, 2, 1, 0, 2, 2, 32, 32)],
    'conv_wgrad_6x2x1x4': [(8, 80, 1, 1, 0, 0, 0, 1, 16, 16), (16, 80, 1, 1, 0, 0, 0, 1, 16, 16), (32, 80, 4, 2, 1, 0, 0, 1, 16, 16),
        (3, 77, 1, 1, 0, 0, 0, 1, 9, 11), (13, 77, 1, 1, 0, 0, 0, 1, 9, 11), (3, 77, 1, 1, 0, 0, 0, 1, 33, 37), (30, 77, 4, 2, 1, 0, 0, 1, 9, 11)],
    'conv_wgrad_smallco': [(42, 1, 4, 1, 1, 0, 2, 1, 9, 11), (16, 3, 7, 1, 3, 1, 3, 1, 18, 18)],
    'conv_wgrad32d_4x4x2x2': [(512, 1024, 4, 1, 1, 0, 0, 1, 6, 7), (128, 100, 1, 1, 0, 0, 0, 1, 9, 11)],
    'conv_pwgrad': [(8, 8, 1, 1, 0, 0, 0, 3, 256, 256), (8, 24, 1, 1, 0, 0, 2, 3, 256, 256), (16, 8, 1, 1, 0, 0, 0, 3, 256, 256),
        (16, 24, 1, 1, 0, 0, 0, 3, 256, 256), (20, 8, 1, 1, 0, 0, 0, 3, 256, 256), (130, 7, 1, 1, 0, 0, 0, 1, 128, 130),
        (77, 60, 1, 1, 0, 0, 0, 4, 64, 64), (3, 77, 1, 1, 0, 0, 0, 2, 64, 64), (3, 7, 1, 1, 0, 0, 0, 3, 257, 255),
        (3, 17, 1, 1, 0, 0, 0, 3, 257, 255), (13, 7, 1, 1, 0, 0, 0, 3, 257, 255), (30, 7, 1, 1, 0, 0, 0, 3, 257, 255)],
    'conv_twgrad': [(3, 35, 3, 1, 1, 0, 0, 2, 64, 64), (3, 35, 5, 1, 2, 1, 0, 2, 64, 64), (42, 7, 3, 1, 1, 0, 0, 2, 64, 64),
        (20, 35, 3, 1, 1, 0, 0, 2, 64, 64), (42, 17, 3, 1, 1, 0, 0, 2, 64, 64), (42, 7, 5, 1, 2, 1, 0, 2, 64, 64)],
}
WGRAD_FORMS = {
    'conv_wgrad32d_4x4x2x2': {'direct': (512, 1024, 4, 1, 1, 0, 0, 1, 6, 7), 'reduce': (128, 100, 1, 1, 0, 0, 0, 1, 9, 11)},
    'conv_wgrad_1x4x1x4': {'direct': (20, 8, 1, 1, 0, 0, 0, 1, 16, 16), 'reduce': (54, 7, 5, 1, 2, 1, 0, 2, 16, 16)},
    'conv_wgrad_2x4x1x4': {'direct': (130, 17, 1, 1, 0, 0, 0, 1, 8, 8), 'reduce': (16, 32, 3, 2, 1, 0, 0, 1, 896, 896)},
    'conv_wgrad_3x4x1x4': {'direct': (8, 40, 1, 1, 0, 0, 0, 1, 16, 16), 'reduce': (3, 35, 1, 1, 0, 0, 0, 1, 33, 37)},
    'conv_wgrad_4x4x1x4': {'direct': (13, 54, 5, 1, 2, 1, 0, 2, 16, 12), 'reduce': (3, 54, 1, 1, 0, 0, 0, 1, 33, 37)},
    'conv_wgrad_4x4x2x2': {'direct': (42, 256, 3, 1, 1, 1, 0, 1, 12, 12), 'reduce': (3, 100, 1, 1, 0, 0, 0, 1, 33, 37)},
    'conv_wgrad_6x2x1x4': {'direct': (8, 80, 1, 1, 0, 0, 0, 1, 16, 16), 'reduce': (3, 77, 1, 1, 0, 0, 0, 1, 33, 37)},
}
TW_CASES = {1: (42, 7, 5, 1, 2, 1, 0, 2, 64, 64), 2: (3, 35, 5, 1, 2, 1, 0, 2, 64, 64), 3: (42, 7, 3, 1, 1, 0, 0, 2, 64, 64), 4: (3, 35, 3, 1, 1, 0, 0, 2, 64, 64), 5: (42, 17, 3, 1, 1, 0, 0, 2, 64, 64), 6: (20, 35, 3, 1, 1, 0, 0, 2, 64, 64)}
PW_CASES = {'cout_le_64': (8, 8, 1, 1, 0, 0, 0, 3, 256, 256), 'cout_gt_64': (3, 77, 1, 1, 0, 0, 0, 2, 64, 64)}

CONV_PREFIXES = ('conv_fwd_', 'conv_fwd32_', 'conv_fwd32sk_', 'conv_dgrad_', 'conv_dgradsk_')
SPLIT_PREFIXES = ('conv_fwd32sk_', 'conv_dgradsk_')
FIXED_NAMES = ('conv_fwd32d_4x4x2x2', 'conv_dgrad32_4x4x2x2', 'conv_dgrad32d_4x4x2x2', 'conv_dgrad32dt_4x4x2x2', 'conv_wgrad32d_4x4x2x2',
               'conv_fwd_smallco', 'conv_wgrad_smallco', 'conv_dgrad_smallci', 'conv_twgrad', 'conv_pwgrad')


def cs4(c):
    return (c + 3) // 4 * 4


def _rows(text, macro):
    """The integer arguments of the ROW(...) lines of `#define <macro>(ROW, ...)` (INT_MAX -> 2**31 - 1)."""
    lines = text.splitlines()
    start = [i for i, l in enumerate(lines) if l.startswith('#define %s(ROW, ...)' % macro)]
    assert len(start) == 1, macro
    rows = []
    for l in lines[start[0] + 1:]:
        m = re.match(r'\s*ROW\(([^)]*)\)', l)
        if not m:
            break
        args = [a.strip() for a in m.group(1).split(',') if a.strip() != '__VA_ARGS__']
        rows.append(tuple(2 ** 31 - 1 if a == 'INT_MAX' else int(a) for a in args))
    assert rows, macro
    return rows


def _derived_names(text):
    conv, wgrad = set(), set()
    for nmax, mt, mts, nt, wm, wn in _rows(text, 'CONV_TILES'):
        conv |= {'%s%dx%dx%dx%d' % (p, mts, nt, wm, wn) for p in CONV_PREFIXES}
        if mts != mt:
            # A row with a small-M tile of its own (the 16 / 32-wide rows) also launches its full-M tile, but never split: a K split needs
            # fewer than 128 tiles, and use_small_m() leaves the small-M tile only at 768 or more M tiles of the full-M size.
            conv |= {'%s%dx%dx%dx%d' % (p, mt, nt, wm, wn) for p in CONV_PREFIXES if p not in SPLIT_PREFIXES}
    for nmax, mt, nt, wm, wn in _rows(text, 'WGRAD_TILES'):
        wgrad.add('conv_wgrad_%dx%dx%dx%d' % (mt, nt, wm, wn))
    return conv, wgrad


def _tw_variant(case):
    """mirror of tw_variant() in csrc/conv_twgrad.hip (which instantiation of the LDS-tile weight gradient a layer takes; 0 = none)"""
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    tl = lambda c: (cs4(c) + 15) // 16
    if stride != 1 or k not in (3, 5) or pad != (k - 1) // 2 or max(cin, cout) > 80 or n * ((h + 7) // 8) * ((w + 7) // 8) < 128:
        return 0
    narrow, wide = sorted((tl(cin), tl(cout)))
    if narrow > (1 if k == 5 else 2) or wide < 3:
        return 0
    xwide = tl(cin) >= tl(cout)
    if k == 5:
        return 1 if xwide else 2
    return (3 if xwide else 4) if narrow == 1 else (5 if xwide else 6)


def _ragged(case):
    return case[0] != 'T' and case[0] % 4 != 0 and case[8] % 2 == 1 and case[9] % 2 == 1


def test_variant_table_covers_the_tile_tables():
    text = open(IGEMM_SRC).read()
    conv, wgrad = _derived_names(text)
    derived = conv | wgrad | set(FIXED_NAMES)
    have = set(VARIANT_CASES)
    assert derived == have, (sorted(derived - have), sorted(have - derived))
    assert all(len(v) >= 1 for v in VARIANT_CASES.values())
    # every generic tile also has a case with Cin % 4 != 0 on an odd plane (the edges where the masks matter)
    for name in sorted(conv | wgrad):
        assert any(_ragged(c) for c in VARIANT_CASES[name]), name
    # both forms of every weight-gradient tile, the six LDS-tile instantiations, both accumulator widths of the pixel-streaming kernel
    assert set(WGRAD_FORMS) == wgrad | {'conv_wgrad32d_4x4x2x2'}
    for name, forms in WGRAD_FORMS.items():
        assert set(forms) == {'direct', 'reduce'} and all(c in VARIANT_CASES[name] for c in forms.values()), name
    assert sorted(TW_CASES) == [1, 2, 3, 4, 5, 6]
    for v, case in TW_CASES.items():
        assert _tw_variant(case) == v and case in VARIANT_CASES['conv_twgrad'], (v, case)
    assert PW_CASES['cout_le_64'][1] <= 64 < PW_CASES['cout_gt_64'][1] and all(c in VARIANT_CASES['conv_pwgrad'] for c in PW_CASES.values())


# ------------------------------------------------------------------------------------------------ B: parity per variant
@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _act64(y, act):
    return {0: y, 1: F.relu(y), 2: F.leaky_relu(y, 0.2), 3: torch.tanh(y)}[act]


@functools.lru_cache(maxsize=1)
def _reference(case):
    """float32 inputs (detfill) and the float64 host reference of one conv case: x, w, b, gy, y, dx, dw, db"""
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    x = detfill.normal((n, cin, h, w), 1)
    wt = detfill.normal((cout, cin, k, k), 2, 1.0 / np.sqrt(cin * k * k))
    b = detfill.normal((cout,), 3, 0.1)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, wt, b))
    xp = F.pad(xr, (pad,) * 4, mode='reflect') if reflect and pad else xr
    yr = _act64(F.conv2d(xp, wr, br, stride=stride, padding=0 if reflect else pad), act)
    gy = detfill.normal(tuple(yr.shape), 4)
    yr.backward(gy.double())
    return x, wt, b, gy, yr.detach(), xr.grad, wr.grad, br.grad


def _padded_weight(wt, dev):
    from cat_amd import ops
    wg = ops.padded_weight_like(wt.shape, dev)
    wg.copy_(wt)
    return wg


def _pad_lanes(t, c):
    """largest magnitude in the padding lanes [c, stride) of an NHWC activation (0.0 when there are none)"""
    st = t.stride(3) if t.shape[3] > 1 else (t.stride(2) if t.shape[2] > 1 else t.stride(0))
    if st <= c or t.shape[0] * t.shape[2] * t.shape[3] == 1:
        return 0.0
    full = torch.as_strided(t, (t.shape[0], st, t.shape[2], t.shape[3]), t.stride())
    return float(full[:, c:].abs().max())


def _poison_workspace(dev):
    """NaNs in the cached per-stream scratch of ops.workspace (grown once so that no case re-allocates it): a split-K / split-pixel producer
    that leaves part of a partial-sum slice unwritten then reduces NaNs instead of an earlier call's values"""
    from cat_amd import ops
    ops.workspace(64 << 20, dev).fill_(float('nan'))


def _profiled(fn):
    from cat_amd import _lib
    lib = _lib.load()
    lib.cat_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
        fam = _families()
    finally:
        lib.cat_prof_enable(0)
    return out, fam


def _wgrad_slices(case):
    """partial-sum slices of the weight gradient's workspace (1 = the producer writes dw itself)"""
    from cat_amd import _lib as L
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    g = _geom(case)
    return int(L.query('cat_conv2d_wgrad_ws_bytes', C.byref(g))) // (cout * k * k * cs4(cin) * 4)


def _geom(case, ycs=None, ycw=0, with_act=False):
    from cat_amd import _lib as L, ops
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    return ops._conv_geom(n, h, w, cin, cs4(cin), ho, wo, cout, ycs or cs4(cout), k, k, stride, pad, L.PAD_REFLECT if reflect else L.PAD_ZERO,
                          act if with_act else 0, 0.2, ycw, cs4(cin))


@functools.lru_cache(maxsize=None)
def _run(case):
    """One forward + backward of the case on the GPU (each case runs once however many families list it): recorded families, the four
    distances from the float64 reference, the largest padding-lane magnitude of y."""
    from cat_amd import ops
    dev = torch.device('cuda:0')
    if case[0] == 'T':
        return _run_transposed(case, dev)
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    x, wt, b, gy, yr, dxr, dwr, dbr = _reference(case)
    xg = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
    wg, bg = _padded_weight(wt, dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    gyg = ops.to_nhwc(gy.to(dev))

    def step():
        _poison_workspace(dev)
        y = ops.Conv2dFn.apply(xg, wg, bg, stride, pad, 1 if reflect else 0, act, 0.2)
        _poison_workspace(dev)
        y.backward(gyg)
        return y
    y, fam = _profiled(step)
    assert tuple(y.shape) == tuple(yr.shape)
    return {'fam': fam, 'y': rel(y, yr), 'dx': rel(xg.grad, dxr), 'dw': rel(wg.grad, dwr), 'db': rel(bg.grad, dbr),
            'pad': _pad_lanes(y.detach(), cout)}


def _run_transposed(case, dev):
    from cat_amd import ops
    _, cin, cout, n, h, w = case
    x = detfill.normal((n, cin, h, w), 5)
    wt = detfill.normal((cin, cout, 3, 3), 6, 1.0 / np.sqrt(cin * 9))
    b = detfill.normal((cout,), 7, 0.1)
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, wt, b))
    yr = F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1)
    gy = detfill.normal(tuple(yr.shape), 8)
    yr.backward(gy.double())
    xg = ops.to_nhwc(x.to(dev)).detach().requires_grad_(True)
    wg, bg = _padded_weight(wt, dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    gyg = ops.to_nhwc(gy.to(dev))

    def step():
        y = ops.ConvTranspose2dFn.apply(xg, wg, bg, 2, 1, 1)
        _poison_workspace(dev)
        y.backward(gyg)
        return y
    y, fam = _profiled(step)
    return {'fam': fam, 'y': rel(y, yr), 'dx': rel(xg.grad, xr.grad), 'dw': rel(wg.grad, wr.grad), 'db': rel(bg.grad, br.grad),
            'pad': _pad_lanes(y.detach(), cout)}


def _ids(case):
    return '-'.join(str(v) for v in case)


@pytest.mark.gpu
@pytest.mark.parametrize('name,case', [(n, c) for n, cs in VARIANT_CASES.items() for c in cs], ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_variant_parity(dev, name, case):
    r = _run(case)
    print(name, case, {k: v for k, v in r.items() if k != 'fam'}, r['fam'])
    assert r['fam'].get(name, 0) == 1, (name, r['fam'])
    assert r['y'] < TOL and r['dx'] < TOL and r['dw'] < TOL and r['db'] < TOL, r
    assert r['pad'] == 0.0, r


@pytest.mark.gpu
@pytest.mark.parametrize('name,form', [(n, f) for n in WGRAD_FORMS for f in ('direct', 'reduce')])
def test_wgrad_tile_in_both_forms(dev, name, form):
    """every weight-gradient tile written by the producer itself (one slice) and through the partial-sum reduce (several)"""
    case = WGRAD_FORMS[name][form]
    slices = _wgrad_slices(case)
    assert (slices == 1) == (form == 'direct'), (case, slices)
    r = _run(case)
    print(name, form, case, slices, r['dw'])
    assert r['fam'].get(name, 0) == 1, (name, r['fam'])
    assert r['dw'] < TOL, r


@pytest.mark.gpu
@pytest.mark.parametrize('variant', sorted(TW_CASES))
def test_lds_tile_wgrad_instantiations(dev, variant):
    r = _run(TW_CASES[variant])
    assert r['fam'].get('conv_twgrad', 0) == 1, r['fam']
    assert r['dw'] < TOL, r


@pytest.mark.gpu
@pytest.mark.parametrize('which', sorted(PW_CASES))
def test_pixel_streaming_wgrad_accumulator_widths(dev, which):
    r = _run(PW_CASES[which])
    assert r['fam'].get('conv_pwgrad', 0) == 1, r['fam']
    assert r['dw'] < TOL, r


# ------------------------------------------------------------------------------------------------ C: poisoned buffers, direct C-ABI calls
def _nan_ws(nbytes, dev):
    return torch.full((max(int(nbytes), 16) // 4 + 4,), float('nan'), device=dev)


def _sentinel_buffer(n, h, w, cs, dev):
    """[N, H, W, cs] of sentinels with 64 more behind it: a write past the last pixel's lanes stays inside the allocation and is seen"""
    flat = torch.full((n * h * w * cs + 64,), SENTINEL, device=dev)
    return flat, flat[:n * h * w * cs].view(n, h, w, cs)


def _check_slice(flat, buf, c0, c, cw, want, what):
    """buf [N, H, W, cs] after a slice write at lane c0: [c0, c0 + c) the result, [c0 + c, c0 + cw) zeros, everything else the sentinel"""
    got = buf.cpu()
    res = got[..., c0:c0 + c].permute(0, 3, 1, 2)
    assert bool(torch.isfinite(res).all()), what
    d = rel(res, want)
    print(what, 'rel', d)
    assert d < TOL, (what, d)
    assert float(got[..., c0 + c:c0 + cw].abs().max()) == 0.0 if cw > c else True, what
    assert bool((got[..., :c0] == SENTINEL).all()), what            # the neighbour below the offset
    assert bool((got[..., c0 + cw:] == SENTINEL).all()), what       # lanes [cw, cs): never touched
    assert bool((flat[-64:] == SENTINEL).all()), what


FWD_PRODUCERS = [
    # family, case -- generic direct (narrow and 128-wide), fwd32, fwd32 split-K (narrow and 128-wide), direct-to-LDS, Cout <= 3 with and
    # without its channel split
    ('conv_fwd_2x1x4x1', (3, 13, 4, 1, 1, 0, 0, 1, 9, 11)),
    ('conv_fwd_4x4x2x2', (3, 100, 1, 1, 0, 0, 2, 1, 9, 11)),
    ('conv_fwd32_2x4x4x1', (13, 54, 5, 1, 2, 1, 0, 2, 16, 12)),
    ('conv_fwd32sk_2x1x4x1', (54, 7, 5, 1, 2, 1, 0, 2, 16, 16)),
    ('conv_fwd32sk_4x4x2x2', (82, 100, 3, 1, 1, 0, 2, 1, 10, 10)),
    ('conv_fwd32d_4x4x2x2', (128, 100, 1, 1, 0, 0, 0, 1, 9, 11)),
    ('conv_fwd_smallco', (16, 3, 7, 1, 3, 1, 3, 1, 18, 18)),
    ('conv_fwd_smallco', (128, 1, 4, 1, 1, 0, 0, 2, 9, 9)),
]


@pytest.mark.gpu
@pytest.mark.parametrize('c0', [0, 8])
@pytest.mark.parametrize('name,case', FWD_PRODUCERS, ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_fwd_poisoned_workspace_and_slice_output(dev, name, case, c0):
    from cat_amd import _lib as L, ops
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    x, wt, b, gy, yr, _, _, _ = _reference(case)
    xg, wg, bg = ops.to_nhwc(x.to(dev)), _padded_weight(wt, dev), b.to(dev)
    cw, cs = cs4(cout) + 4, c0 + cs4(cout) + 8
    g = _geom(case, ycs=cs, ycw=cw, with_act=True)
    flat, buf = _sentinel_buffer(n, g.Ho, g.Wo, cs, dev)
    yptr = C.c_void_p(buf.data_ptr() + 4 * c0)
    nb = int(L.query('cat_conv2d_fwd_ws_bytes', C.byref(g)))
    if case == (128, 1, 4, 1, 1, 0, 0, 2, 9, 9) or 'sk_' in name:
        assert nb > 0, 'the split form needs a workspace'
    ws = _nan_ws(nb, dev)

    def call():
        if nb:
            L.call('cat_conv2d_fwd_ws', C.byref(g), ops._p(xg), ops._p(wg), ops._p(bg), yptr, ops._p(ws), ops._stream())
        else:
            L.call('cat_conv2d_fwd', C.byref(g), ops._p(xg), ops._p(wg), ops._p(bg), yptr, ops._stream())
    _, fam = _profiled(call)
    assert fam.get(name, 0) == 1, fam
    _check_slice(flat, buf, c0, cout, cw, yr, (name, case, c0))


DGRAD_PRODUCERS = [
    # family, case, entry point -- generic (stride 2: four parity classes), split-K narrow and 128-wide, the 32-deep 128 x 128 tile, its
    # direct-to-LDS form with the filter as stored and transposed, the 3 / 6-channel image gradient
    ('conv_dgrad_2x2x4x1', (30, 35, 4, 2, 1, 0, 0, 1, 9, 11), 'ws'),
    ('conv_dgrad_4x4x2x2', (130, 7, 3, 2, 1, 0, 0, 1, 9, 11), 'ws'),
    ('conv_dgradsk_2x2x4x1', (30, 13, 4, 1, 1, 0, 0, 1, 9, 11), 'ws'),
    ('conv_dgradsk_4x4x2x2', (130, 13, 4, 1, 1, 0, 0, 1, 9, 11), 'ws'),
    ('conv_dgrad32_4x4x2x2', (100, 16, 1, 1, 0, 0, 0, 1, 9, 11), 'ws'),
    ('conv_dgrad32d_4x4x2x2', (100, 32, 1, 1, 0, 0, 0, 1, 9, 11), 'ws'),
    ('conv_dgrad32dt_4x4x2x2', (100, 32, 1, 1, 0, 0, 0, 1, 9, 11), 't'),
    ('conv_dgrad32d_4x4x2x2', (128, 64, 4, 2, 1, 0, 0, 1, 10, 14), 'ws'),
    ('conv_dgrad_smallci', (3, 17, 4, 2, 1, 0, 0, 1, 9, 11), 'ws'),
    ('conv_dgrad_smallci', (6, 20, 4, 2, 1, 0, 0, 1, 33, 37), 'ws'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('c0', [0, 8])
@pytest.mark.parametrize('name,case,entry', DGRAD_PRODUCERS, ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_dgrad_poisoned_workspace_and_slice_output(dev, name, case, entry, c0):
    from cat_amd import _lib as L, ops
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    assert act == 0 and not reflect
    x, wt, b, gy, _, dxr, _, _ = _reference(case)
    wg, gyg = _padded_weight(wt, dev), ops.to_nhwc(gy.to(dev))
    cw, cs = cs4(cin) + 4, c0 + cs4(cin) + 8
    g = _geom(case)
    flat, buf = _sentinel_buffer(n, h, w, cs, dev)
    dxptr = C.c_void_p(buf.data_ptr() + 4 * c0)
    st = ops._stream()
    if entry == 't':
        assert L.query('cat_conv2d_dgrad_t_applicable', C.byref(g)) == 1
        wt_t = torch.full((cout * cin * k * k,), float('nan'), device=dev)
        L.call('cat_conv2d_weight_transpose', C.byref(g), ops._p(wg), ops._p(wt_t), st)
        call = lambda: L.call('cat_conv2d_dgrad_t', C.byref(g), ops._p(gyg), ops._p(wg), ops._p(wt_t), None, dxptr, cs, cw, st)
    else:
        nb = int(L.query('cat_conv2d_dgrad_ws_bytes', C.byref(g), cs))
        assert (nb > 0) == ('sk_' in name), nb
        ws = _nan_ws(nb, dev)
        if nb:
            call = lambda: L.call('cat_conv2d_dgrad_ws', C.byref(g), ops._p(gyg), ops._p(wg), None, dxptr, cs, cw, ops._p(ws), st)
        else:
            call = lambda: L.call('cat_conv2d_dgrad', C.byref(g), ops._p(gyg), ops._p(wg), None, dxptr, cs, cw, st)
    _, fam = _profiled(call)
    assert fam.get(name, 0) == 1, fam
    _check_slice(flat, buf, c0, cin, cw, dxr, (name, case, entry, c0))


WGRAD_PRODUCERS = [(n, WGRAD_FORMS[n][f]) for n in sorted(WGRAD_FORMS) for f in ('direct', 'reduce')] + [
    ('conv_wgrad_smallco', (16, 3, 7, 1, 3, 1, 3, 1, 18, 18)), ('conv_wgrad_smallco', (42, 1, 4, 1, 1, 0, 2, 1, 9, 11)),
    ('conv_twgrad', TW_CASES[3]), ('conv_twgrad', TW_CASES[2]), ('conv_pwgrad', PW_CASES['cout_gt_64']), ('conv_pwgrad', (13, 7, 1, 1, 0, 0, 0, 3, 257, 255))]


@pytest.mark.gpu
@pytest.mark.parametrize('accumulate', [1, 0])
@pytest.mark.parametrize('name,case', WGRAD_PRODUCERS, ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_wgrad_accumulate_and_fresh_write(dev, name, case, accumulate):
    """accumulate = 1 into a gradient that is already there (the direct producers add in their epilogue, the others in the reduce) and
    accumulate = 0 over NaNs, with a NaN workspace; the padding lanes [Cin, wcs) of every tap -- part of FusedAdam's flat buffers -- end 0.0"""
    from cat_amd import _lib as L, ops
    cin, cout, k, stride, pad, reflect, act, n, h, w = case
    x, wt, b, gy, _, _, dwr, _ = _reference(case[:6] + (0,) + case[7:])      # the weight gradient of the plain (no activation) layer for dy = gy
    xg, gyg = ops.to_nhwc(x.to(dev)), ops.to_nhwc(gy.to(dev))
    dw = ops.padded_weight_like((cout, cin, k, k), dev)
    if accumulate:
        prev = detfill.normal((cout, cin, k, k), 9, float(dwr.abs().max()))      # as large as the gradient: neither term hides the other
        dw.copy_(prev)
        want = prev.double() + dwr
    else:
        dw.fill_(float('nan'))      # the real lanes only: padded_weight_like's view leaves [Cin, wcs) at 0.0
        want = dwr
    g = _geom(case)
    ws = _nan_ws(L.query('cat_conv2d_wgrad_ws_bytes', C.byref(g)), dev)
    _, fam = _profiled(lambda: L.call('cat_conv2d_wgrad', C.byref(g), ops._p(xg), ops._p(gyg), ops._p(dw), accumulate, ops._p(ws), ops._stream()))
    assert fam.get(name, 0) == 1, fam
    got = dw.cpu()
    assert bool(torch.isfinite(got).all())
    d = rel(got, want)
    print(name, case, accumulate, 'rel', d)
    assert d < TOL, d
    raw = torch.as_strided(dw, (cout * k * k, cs4(cin)), (cs4(cin), 1)).cpu()
    assert cs4(cin) == cin or (bool(torch.isfinite(raw[:, cin:]).all()) and float(raw[:, cin:].abs().max()) == 0.0)


# ------------------------------------------------------------------------------------------------ D: rectangular filters
@pytest.mark.gpu
@pytest.mark.parametrize('kh,kw,cin,cout,n,h,w', [(1, 7, 128, 192, 2, 17, 17), (7, 1, 160, 160, 2, 17, 17), (1, 3, 384, 384, 2, 8, 8),
                                                   (3, 1, 384, 384, 2, 8, 8)])
def test_conv2d_fwd_rect(dev, kh, kw, cin, cout, n, h, w):
    """cat_conv2d_fwd_rect: the factorised filters of InceptionC / InceptionE (different zero padding along H and W) + bias + ReLU against
    float64 F.conv2d(padding=(ph, pw)), written into a channel slice of a wider buffer like metric/inception.py does"""
    from cat_amd import _lib as L, ops
    ph, pw = (kh - 1) // 2, (kw - 1) // 2
    x = detfill.normal((n, cin, h, w), 31)
    wt = detfill.normal((cout, cin, kh, kw), 32, 1.0 / np.sqrt(cin * kh * kw))
    b = detfill.normal((cout,), 33, 0.1)
    want = F.relu(F.conv2d(x.double(), wt.double(), b.double(), padding=(ph, pw)))
    xg, wg, bg = ops.to_nhwc(x.to(dev)), _padded_weight(wt, dev), b.to(dev)
    c0, cw = 8, cout + 4
    cs = c0 + cout + 8
    flat, buf = _sentinel_buffer(n, h, w, cs, dev)
    g = ops._conv_geom(n, h, w, cin, cs4(cin), h, w, cout, cs, kh, kw, 1, ph, L.PAD_ZERO, L.ACT_RELU, 0.0, cw, cs4(cin))
    L.call('cat_conv2d_fwd_rect', C.byref(g), pw, ops._p(xg), ops._p(wg), ops._p(bg), C.c_void_p(buf.data_ptr() + 4 * c0), ops._stream())
    torch.cuda.synchronize()
    _check_slice(flat, buf, c0, cout, cw, want, ('rect', kh, kw))
