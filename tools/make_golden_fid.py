"""tests/golden/fid_frechet.npz: the REFERENCE's own Frechet distance on seeded feature sets.

Runs only in the build container (imports the reference through tools/ref_import.py).  What executes is the reference's
metric/fid_score.py `calculate_frechet_distance` (numpy + scipy.linalg.sqrtm) on np.mean / np.cov of tests/fid_numpy.features sets.  The
fixture holds seeds, shapes, one checksum per set and recorded scalars only: tests regenerate the features.

Per case: fd_reference (the reference's number), fd_eigh (tests/fid_numpy.frechet_eigh, the float64 yardstick), ref_gap = their distance --
on singular covariances scipy's sqrtm returns a complex root with imaginary parts around 1e-8, so the gap is the reference's own error --
and tr = Tr S1 + Tr S2, the scale the tolerances are written in.

    python tools/make_golden_fid.py        # rewrites tests/golden/fid_frechet.npz"""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402

import fid_numpy as FN  # noqa: E402
import ref_import  # noqa: E402


def main():
    ref_import.install()
    for name in [m for m in sys.modules if m == 'metric' or m.startswith('metric.')]:
        del sys.modules[name]
    fid = importlib.import_module('metric.fid_score')
    assert fid.__file__.startswith(ref_import.REF + '/'), fid.__file__
    out = dict(cases=json.dumps(FN.CASES))
    for c in FN.CASES:
        f1, f2 = FN.case_features(c)
        mu1, s1 = FN.stats(f1)
        mu2, s2 = FN.stats(f2)
        t0 = time.time()
        fd_ref = float(fid.calculate_frechet_distance(mu1, s1, mu2, s2))
        fd_eigh = float(FN.frechet_eigh(mu1, s1, f2))
        n = c['name']
        out.update({n + '_fd_reference': fd_ref, n + '_fd_eigh': fd_eigh, n + '_ref_gap': abs(fd_ref - fd_eigh),
                    n + '_tr': float(np.trace(s1) + np.trace(s2)), n + '_checksums': np.array([FN.checksum(f1), FN.checksum(f2)])})
        print('%-22s fd_reference %.12g  fd_eigh %.12g  gap %.2e  tr %.4g  (%.1f s)' % (n, fd_ref, fd_eigh, abs(fd_ref - fd_eigh),
                                                                                       out[n + '_tr'], time.time() - t0))
    path = os.path.join(ROOT, 'tests', 'golden', 'fid_frechet.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
