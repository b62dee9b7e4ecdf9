"""Plain float64 numpy restatement of what cat_kid_poly_sums computes, and the seeded features the KID tests and tests/golden/kid.npz share.

`poly_sums` builds the three polynomial kernels of every subset the way sklearn's `polynomial_kernel` does (K = A B^T; K *= gamma; K += coef0;
K **= degree) and takes the sums metric/kid_score.py:205-281 reads: the GPU tests' reference.  `features` regenerates the fixture's inputs
from numpy's frozen RandomState stream: non-negative like pool3 outputs, rounded through float32 like a network's output, widened back to
float64 like the reference holds them.  Only +, * on IEEE doubles: the values do not depend on a math library."""
import numpy as np

# the cases of tests/golden/kid.npz: (nx, ny, d, m, S), feature seed, np.random seed of the draws, kernel arguments
CASES = [
    dict(name='script_shape', nx=140, ny=120, d=2048, m=100, S=3, seed=1401, draw_seed=11, kernel={}),
    dict(name='ragged', nx=60, ny=50, d=64, m=37, S=3, seed=1402, draw_seed=12, kernel={}),
    dict(name='one_tile', nx=40, ny=40, d=768, m=16, S=2, seed=1403, draw_seed=13, kernel={}),
    dict(name='kernel_args', nx=60, ny=50, d=64, m=37, S=3, seed=1404, draw_seed=14, kernel=dict(degree=2, gamma=0.01, coef0=0.5)),
]
ESTIMATORS = ('biased', 'unbiased', 'u-statistic')


def features(seed, nx, ny, d):
    """(X [nx, d], Y [ny, d]) float64 holding float32 values in [0, 1) and [0, 1.1): two different distributions, so mmd2 is not ~0."""
    rs = np.random.RandomState(seed)
    x = rs.random_sample((nx, d)).astype(np.float32).astype(np.float64)
    y = (rs.random_sample((ny, d)) * 1.1).astype(np.float32).astype(np.float64)
    return x, y


def polynomial_kernel(a, b, degree=3, gamma=None, coef0=1):
    gamma = 1.0 / a.shape[1] if gamma is None else gamma
    k = a.astype(np.float64) @ b.astype(np.float64).T
    k *= gamma
    k += coef0
    k **= degree
    return k


def kernels(x, y, g, r, **kernel):
    """(K_XX, K_XY, K_YY) of one subset: rows g of x against rows r of y"""
    a, b = x[g], y[r]
    return polynomial_kernel(a, a, **kernel), polynomial_kernel(a, b, **kernel), polynomial_kernel(b, b, **kernel)


def sums_of(k_xx, k_xy, k_yy):
    return dict(rs_xx=k_xx.sum(axis=1), dg_xx=np.diagonal(k_xx).copy(), rs_yy=k_yy.sum(axis=1), dg_yy=np.diagonal(k_yy).copy(),
                rs_xy=k_xy.sum(axis=1), cs_xy=k_xy.sum(axis=0), tr_xy=np.trace(k_xy), sq_xx=(k_xx * k_xx).sum(), sq_yy=(k_yy * k_yy).sum(),
                sq_xy=(k_xy * k_xy).sum())


def poly_sums(x, y, gi, ri, **kernel):
    """dict of [S, m] / [S] float64 arrays, keyed like cat_amd.metric.kid_score.split_sums"""
    per = [sums_of(*kernels(x, y, g, r, **kernel)) for g, r in zip(gi, ri)]
    return {k: np.stack([np.asarray(p[k]) for p in per]) for k in per[0]}


def scale_of(sums, m):
    """mean K_XX + mean K_YY + 2 * mean K_XY per subset: the magnitude mmd2's terms have before they cancel"""
    return (sums['rs_xx'].sum(-1) + sums['rs_yy'].sum(-1) + 2 * sums['rs_xy'].sum(-1)) / (m * m)
