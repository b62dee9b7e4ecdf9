"""tests/golden/conv_plan_sweep.npz: the host-side plan answers of THIS repository's library (forward / input-gradient / weight-gradient
workspace bytes and cat_conv2d_dgrad_t_applicable) over the grid of tests/test_conv_plan_host.py.

A regression fixture, not a reference: re-record it only with a change that moves a geometry to another kernel or split on purpose, and
say so in that change.  No GPU is needed (the four entry points are pure host functions); none of the CAT_* plan switches may be set.

    python tools/make_golden_conv_plan.py        # rewrites tests/golden/conv_plan_sweep.npz"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

import test_conv_plan_host as T  # noqa: E402


def main():
    set_vars = [v for v in T.PLAN_ENV if v in os.environ]
    assert not set_vars, 'unset %s first' % ', '.join(set_vars)
    out = T.sweep()
    np.savez_compressed(T.GOLDEN, **out)
    print('%d geometries: %d forward splits, %d input-gradient splits, %d transposed-filter tiles' % (
        len(out['fwd_ws_bytes']), (out['fwd_ws_bytes'] > 0).sum(), (out['dgrad_ws_bytes'] > 0).sum(), out['dgrad_t_applicable'].sum()))
    print('wrote', T.GOLDEN, os.path.getsize(T.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
