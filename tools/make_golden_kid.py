"""tests/golden/kid.npz: the REFERENCE's own kernel-inception-distance arithmetic on seeded features.

Runs only in the build container (imports /root/reference).  What executes is the reference's metric/kid_score.py: polynomial_mmd_averages
(numpy's global generator for the subsets, sklearn's polynomial_kernel, _mmd2_and_variance) and _mmd2_and_variance alone under its three
`mmd_est` values.  Its `from inception import InceptionV3` (the network is not used here) gets a stub module, as tools/make_golden_inception.py
stubs torchvision.  The fixture holds seeds, parameters and results only: tests regenerate the features with tests/kid_numpy.features.

    python tools/make_golden_kid.py        # rewrites tests/golden/kid.npz"""
import importlib.util
import io
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

import kid_numpy as KN  # noqa: E402

REF_FILE = '/root/reference/metric/kid_score.py'


def import_reference():
    stub = types.ModuleType('inception')
    stub.InceptionV3 = type('InceptionV3', (), {'BLOCK_INDEX_BY_DIM': {64: 0, 192: 1, 768: 2, 2048: 3}})
    sys.modules['inception'] = stub
    spec = importlib.util.spec_from_file_location('ref_kid_score', REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = import_reference()
    out = dict(cases=json.dumps(KN.CASES), estimators=json.dumps(KN.ESTIMATORS))
    for c in KN.CASES:
        x, y = KN.features(c['seed'], c['nx'], c['ny'], c['d'])
        np.random.seed(c['draw_seed'])
        mmds, vars_ = ref.polynomial_mmd_averages(x, y, n_subsets=c['S'], subset_size=c['m'], output=io.StringIO(), **c['kernel'])
        np.random.seed(c['draw_seed'])
        only = ref.polynomial_mmd_averages(x, y, n_subsets=c['S'], subset_size=c['m'], ret_var=False, output=io.StringIO(), **c['kernel'])
        assert np.array_equal(only, mmds)
        # the subsets that run used, drawn again the same way (the recorded tables pin the product's order of draws)
        np.random.seed(c['draw_seed'])
        gi, ri = [], []
        for _ in range(c['S']):
            gi.append(np.random.choice(len(x), c['m'], replace=False))
            ri.append(np.random.choice(len(y), c['m'], replace=False))
        gi, ri = np.array(gi, dtype=np.int32), np.array(ri, dtype=np.int32)
        m_all = min(len(x), len(y))
        est = np.zeros((c['S'], len(KN.ESTIMATORS), 2))
        for s in range(c['S']):
            k_xx, k_xy, k_yy = KN.kernels(x, y, gi[s], ri[s], **c['kernel'])
            sk = ref.polynomial_kernel(x[gi[s]], y[ri[s]], **c['kernel'])
            assert np.abs(sk - k_xy).max() <= 1e-13 * np.abs(sk).max()      # kid_numpy's kernel is sklearn's
            for e, name in enumerate(KN.ESTIMATORS):
                est[s, e] = ref._mmd2_and_variance(sk_xx(ref, x, gi[s], c), sk, sk_xx(ref, y, ri[s], c), mmd_est=name, var_at_m=m_all)
                assert ref._mmd2_and_variance(k_xx, k_xy, k_yy, mmd_est=name, var_at_m=m_all, ret_var=False) == \
                    ref._mmd2_and_variance(k_xx, k_xy, k_yy, mmd_est=name, var_at_m=m_all)[0]
            assert est[s, 1, 0] == mmds[s] and est[s, 1, 1] == vars_[s]      # 'unbiased' is what polynomial_mmd_averages reports
        n = c['name']
        out.update({n + '_mmds': mmds, n + '_vars': vars_, n + '_est': est})
        if n == 'ragged':
            out.update({n + '_gi': gi, n + '_ri': ri})
        print('%-12s mmd2 %s  var %s' % (n, mmds, vars_))
    path = os.path.join(ROOT, 'tests', 'golden', 'kid.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


def sk_xx(ref, feats, idx, c):
    return ref.polynomial_kernel(feats[idx], **c['kernel'])


if __name__ == '__main__':
    main()
