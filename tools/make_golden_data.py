"""Record the reference's own get_params draws (data/base_dataset.py:63-82) into tests/golden/data_params.json.

Runs on the build container only (tools/ref_import.py imports the reference, which the GPU box does not have).  Four option sets, each under
two seeds, 32 draws each, with the image size get_params was handed: tests/test_data_host.py replays them through cat_amd.data.get_params,
which pins the order and the count of the `random` calls."""
import json
import os
import random
import sys
from argparse import Namespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

SETS = [
    ('aligned_resize_and_crop', dict(preprocess='resize_and_crop', load_size=286, crop_size=256), (600, 600)),
    ('cityscapes_scale_width', dict(preprocess='scale_width', load_size=512, crop_size=512), (2048, 1024)),
    ('scale_width_and_crop', dict(preprocess='scale_width_and_crop', load_size=286, crop_size=256), (600, 400)),
    ('none', dict(preprocess='none', load_size=286, crop_size=256), (256, 256)),
]
SEEDS = (1, 20231)
DRAWS = 32


def main():
    ref_import.install()
    from data.base_dataset import get_params
    out = []
    for name, kw, size in SETS:
        for seed in SEEDS:
            random.seed(seed)
            draws = []
            for _ in range(DRAWS):
                p = get_params(Namespace(**kw), size)
                draws.append({'crop_pos': [int(v) for v in p['crop_pos']], 'flip': bool(p['flip']), 'crop_size': [int(v) for v in p['crop_size']]})
            out.append({'name': name, 'opt': kw, 'size': list(size), 'seed': seed, 'draws': draws})
    path = os.path.join(HERE, '..', 'tests', 'golden', 'data_params.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=None, separators=(',', ':'))
        f.write('\n')
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
