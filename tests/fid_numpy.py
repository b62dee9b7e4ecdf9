"""Plain float64 numpy yardsticks for FID's tail on the device, and the seeded features the FID tests and tests/golden/fid_frechet.npz share.

`features` regenerates a feature set from numpy's frozen RandomState stream: correlated columns (a low-rank mix plus noise), clipped at 0
like pool3 outputs, rounded through float32 like a network's output, widened back to float64 like the reference holds them.
`frechet_eigh` is the yardstick: Tr (S1 S2)^1/2 as the sum of the square roots of the eigenvalues of a symmetric positive semi-definite
matrix (np.linalg.eigvalsh, eigenvalues clipped at 0) -- the Gram form M = Xc S1 Xc^T / (n - 1) when the fake set has n <= d features, the
full form M = R S2 R with R = S1^1/2 from eigh otherwise.  Every matrix here is singular (centring alone gives a null vector), and eigh
returns a zero eigenvalue as +-n eps |M|, whose square root is 1e-8 sqrt|M|: clipped at exactly 0, the yardstick would carry up to 8e-9 of
Tr S1 + Tr S2 of its own noise.  So the clip is at numpy's rank tolerance n eps max(w) (np.linalg.matrix_rank's) instead: what eigh cannot
tell from 0 is 0.  With that floor the Gram form on the fake side, the Gram form on the real side and the full form agree to 2e-16 of
Tr S1 + Tr S2 on every case of the fixture where they can be compared, which is what makes it a yardstick.  `nsqrt_trace` restates the
coupled Newton-Schulz iteration the product runs, with its stopping rule; `frechet_ns` is the distance through it."""
import numpy as np

# the cases of tests/golden/fid_frechet.npz: real set (n1, seed1, shift1) against fake set (n2, seed2, shift2), d features each
CASES = [
    dict(name='gram_rank_deficient', n1=24, n2=20, d=64, seed1=2101, seed2=2102, shift1=0.0, shift2=0.2),
    dict(name='gram_small', n1=100, n2=30, d=64, seed1=2103, seed2=2104, shift1=0.0, shift2=0.2),
    dict(name='full_s1_singular', n1=30, n2=100, d=64, seed1=2105, seed2=2106, shift1=0.0, shift2=0.2),
    dict(name='full', n1=300, n2=250, d=192, seed1=2107, seed2=2108, shift1=0.0, shift2=0.2),
    dict(name='gram_production', n1=300, n2=120, d=2048, seed1=2109, seed2=2110, shift1=0.0, shift2=0.2),
    dict(name='gram_evaluate_model', n1=64, n2=4, d=2048, seed1=2111, seed2=2112, shift1=0.0, shift2=0.2),
    dict(name='identical', n1=40, n2=40, d=64, seed1=2113, seed2=2113, shift1=0.1, shift2=0.1),
]
MAX_STEPS = 100
REL_STEP = 1e-14


def features(seed, n, d, shift=0.0):
    """[n, d] float64 holding non-negative float32 values: relu(0.5 * (Z W / sqrt(q) + 0.5 E) + shift), Z [n, q], W [q, d], E [n, d]
    standard normal, q = max(4, d // 8)."""
    rs = np.random.RandomState(seed)
    q = max(4, d // 8)
    z, w, e = rs.standard_normal((n, q)), rs.standard_normal((q, d)), rs.standard_normal((n, d))
    x = 0.5 * (z.dot(w) / np.sqrt(q) + 0.5 * e) + shift
    return np.maximum(x, 0.0).astype(np.float32).astype(np.float64)


def case_features(c):
    return features(c['seed1'], c['n1'], c['d'], c['shift1']), features(c['seed2'], c['n2'], c['d'], c['shift2'])


def checksum(x):
    """one number per feature set, recorded in the fixture: a changed generator shows as a changed checksum, not as a wrong distance"""
    return float((x * (1.0 + (np.arange(x.size).reshape(x.shape) % 7))).sum())


def stats(x):
    return np.mean(x, axis=0), np.cov(x, rowvar=False)


def _sym(m):
    return (m + m.T) / 2


def clip_psd(w):
    """eigenvalues of a positive semi-definite matrix as eigh returns them, with what it cannot tell from 0 set to 0"""
    tol = len(w) * np.finfo(np.float64).eps * max(float(w.max()), 0.0)
    return np.where(w > tol, w, 0.0)


def sqrt_trace_eigh(m):
    return np.sqrt(clip_psd(np.linalg.eigvalsh(_sym(m)))).sum()


def sqrt_psd_eigh(s):
    w, v = np.linalg.eigh(_sym(s))
    return (v * np.sqrt(clip_psd(w))).dot(v.T)


def gram_matrix(s1, feats2):
    xc = feats2 - feats2.mean(axis=0)
    return _sym(xc.dot(s1).dot(xc.T) / (len(feats2) - 1)), (xc * xc).sum() / (len(feats2) - 1)


def full_matrix(s1, s2):
    r = sqrt_psd_eigh(s1)
    return _sym(r.dot(s2).dot(r))


def _frechet(mu1, s1, feats2, sqrt_trace):
    n, d = feats2.shape
    mu2 = feats2.mean(axis=0)
    if n <= d:
        m, tr2 = gram_matrix(s1, feats2)
    else:
        s2 = np.cov(feats2, rowvar=False)
        m, tr2 = full_matrix(s1, s2), np.trace(s2)
    diff = mu1 - mu2
    return diff.dot(diff) + np.trace(s1) + tr2 - 2.0 * sqrt_trace(m)


def frechet_eigh(mu1, s1, feats2):
    """the float64 yardstick"""
    return _frechet(mu1, s1, feats2, sqrt_trace_eigh)


def frechet_eigh_stats(mu1, s1, mu2, s2):
    """the same through the full form, from two pairs of statistics"""
    diff = mu1 - mu2
    return diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * sqrt_trace_eigh(full_matrix(s1, s2))


def nsqrt(m):
    """(Y with M^1/2 = sqrt(c) Y, c, Tr Y, steps, converged): Y0 = M / c, Z0 = I, c = |M|_F; T = 1.5 I - 0.5 Z Y, Y <- Y T, Z <- T Z; stop at
    the first step whose trace is not finite or does not exceed the previous one by more than 1e-14 relative, keep the iterate with the
    larger finite trace; the cap is 100 steps."""
    c = float(np.sqrt((m * m).sum()))
    n = len(m)
    if c == 0.0:
        return np.zeros_like(m), 0.0, 0.0, 0, True
    y, z, eye = m / c, np.eye(n), np.eye(n)
    best = np.trace(y)
    with np.errstate(all='ignore'):
        for step in range(1, MAX_STEPS + 1):
            t = 1.5 * eye - 0.5 * z.dot(y)
            y2, z2 = y.dot(t), t.dot(z)
            tr = np.trace(y2)
            if not np.isfinite(tr):
                return y, c, best, step, False
            if not tr > best * (1.0 + REL_STEP):
                return (y2, c, tr, step, True) if tr > best else (y, c, best, step, True)
            best, y, z = tr, y2, z2
    return y, c, best, MAX_STEPS, False


def nsqrt_trace(m):
    """(Tr M^1/2, steps, converged)"""
    _, c, tr, steps, ok = nsqrt(m)
    return np.sqrt(c) * tr, steps, ok


def frechet_ns(mu1, s1, feats2):
    """the distance through the iteration, both forms as the product takes them (the full form's root by the iteration as well)"""
    n, d = feats2.shape
    steps = []

    def tr(m):
        v, s, ok = nsqrt_trace(m)
        steps.append(s)
        assert ok
        return v
    if n <= d:
        return _frechet(mu1, s1, feats2, tr), steps
    y, c, _, s0, ok = nsqrt(_sym(s1))
    assert ok
    steps.append(s0)
    r = _sym(y) * np.sqrt(c)
    s2 = np.cov(feats2, rowvar=False)
    diff = mu1 - feats2.mean(axis=0)
    return diff.dot(diff) + np.trace(s1) + np.trace(s2) - 2.0 * tr(_sym(r.dot(s2).dot(r))), steps
