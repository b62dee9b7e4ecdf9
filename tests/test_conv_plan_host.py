"""CPU: the four host-side plan answers of the implicit-GEMM convolution (csrc/conv_igemm.hip) over a fixed grid of geometries against
tests/golden/conv_plan_sweep.npz, recorded from the library before the plans were gathered into one function per pass
(tools/make_golden_conv_plan.py).  Forward, input-gradient and weight-gradient workspace bytes and cat_conv2d_dgrad_t_applicable are pure
host functions, so a refactor of the dispatch that moves a geometry to another kernel, split or workspace size fails here without a GPU.

The grid is written here; the fixture holds only the answers, in sweep() order.  It crosses the 16 / 32 / 48 / 64 / 96 tile rows, Cout > 96,
Cin % 32 and Cin % 128, the Cout <= 3 and Cin <= 6 layers, the 128-tile split limit, the 768-tile small-M limit, the 8192-pixel limit of
the pixel-streaming weight gradient and the 2 GB offset limit of the direct-to-LDS tiles ((16, 256, 256) with 512 channels)."""
import ctypes as C
import itertools
import os

import numpy as np

from cat_amd import _build, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_plan_sweep.npz')

CIN = (3, 6, 8, 13, 16, 20, 32, 42, 64, 77, 96, 100, 128, 130, 256, 512)
COUT = (1, 3, 7, 16, 17, 32, 35, 48, 64, 77, 96, 97, 128, 129, 256, 1024)
FILTERS = ((1, 1, 0, 0), (3, 1, 1, 0), (3, 1, 1, 1), (3, 2, 1, 0), (4, 1, 1, 0), (4, 2, 1, 0), (5, 1, 2, 1), (7, 1, 3, 1))      # k, stride, pad, reflect
PLANES = ((1, 6, 7), (1, 9, 11), (2, 16, 16), (2, 64, 64), (4, 128, 128), (3, 257, 255), (16, 256, 256))      # N, H, W
# the A/B switches and tuning knobs of the plans: the library reads them once per process, so the recorded answers hold only with none set
PLAN_ENV = ('CAT_FWD_DIRECT', 'CAT_DGRAD_DIRECT', 'CAT_DGRAD_T', 'CAT_WGRAD_DIRECT', 'CAT_WGRAD_BLOCKS', 'CAT_WGRAD_MINCHUNK', 'CAT_WGRAD_MAXSPLIT')
KEYS = ('fwd_ws_bytes', 'dgrad_ws_bytes', 'wgrad_ws_bytes', 'dgrad_t_applicable')


def cs4(c):
    return (c + 3) // 4 * 4


def geometries():
    """(ConvGeom, dxcs) per grid point: pixel strides and wcs are round_up(C, 4), no activation, ycw = 0"""
    for cin, cout, (k, stride, pad, reflect), (n, h, w) in itertools.product(CIN, COUT, FILTERS, PLANES):
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        yield _lib.ConvGeom(n, h, w, cin, cs4(cin), ho, wo, cout, cs4(cout), k, k, stride, pad, _lib.PAD_REFLECT if reflect else _lib.PAD_ZERO,
                            0, 0.0, 0, cs4(cin)), cs4(cin)


def sweep():
    """the four answers of the loaded library for every geometry, as int64 arrays keyed like the fixture"""
    lib = _lib.load()
    rows = [(lib.cat_conv2d_fwd_ws_bytes(C.byref(g)), lib.cat_conv2d_dgrad_ws_bytes(C.byref(g), dxcs), lib.cat_conv2d_wgrad_ws_bytes(C.byref(g)),
             lib.cat_conv2d_dgrad_t_applicable(C.byref(g))) for g, dxcs in geometries()]
    cols = np.array(rows, dtype=np.int64).T
    return dict(zip(KEYS, cols))


def _where(i):
    cin, cout, f, p = list(itertools.product(CIN, COUT, FILTERS, PLANES))[i]
    return 'Cin %d Cout %d (k, stride, pad, reflect) %s (N, H, W) %s' % (cin, cout, f, p)


def test_conv_plans_match_the_recorded_sweep():
    set_vars = [v for v in PLAN_ENV if v in os.environ]
    assert not set_vars, 'unset %s: the conv plans read these once per process and the recorded answers are the defaults' % ', '.join(set_vars)
    _build.build(verbose=False)
    want = np.load(GOLDEN)
    got = sweep()
    assert sorted(want.files) == sorted(KEYS)
    n = len(CIN) * len(COUT) * len(FILTERS) * len(PLANES)
    for key in KEYS:
        assert want[key].shape == got[key].shape == (n,), key
        bad = np.flatnonzero(want[key] != got[key])
        assert bad.size == 0, '%s differs at %d geometries, first: %s -- recorded %d, library %d' % (
            key, bad.size, _where(int(bad[0])), want[key][bad[0]], got[key][bad[0]])
    # the sweep reaches the split and transposed-filter plans (a grid that no longer does would compare zeros with zeros)
    assert (want['fwd_ws_bytes'] > 0).sum() > 1000 and (want['dgrad_ws_bytes'] > 0).sum() > 1000 and want['dgrad_t_applicable'].sum() > 100
    assert (want['wgrad_ws_bytes'] > 0).all()
