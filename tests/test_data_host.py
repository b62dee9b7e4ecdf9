"""CPU: the host side of cat_amd.data -- the reference's draws (against its own recorded results), the codes dataset under the stock DataLoader,
the deterministic PIL prefix of DeviceImageSet, and the refusals."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.utils.data
from PIL import Image

import data_host_ref as R
import helpers as H
from cat_amd import data


def test_get_params_reproduces_the_recorded_reference_draws():
    """tests/golden/data_params.json (tools/make_golden_data.py): the reference's get_params, 4 option sets x 2 seeds x 32 draws.  A missing,
    extra or reordered `random` call shifts every draw after the first."""
    with open(os.path.join(H.GOLDEN, 'data_params.json')) as f:
        recorded = json.load(f)
    assert sorted({r['name'] for r in recorded}) == ['aligned_resize_and_crop', 'cityscapes_scale_width', 'none', 'scale_width_and_crop']
    assert len(recorded) == 8
    for r in recorded:
        opt = Namespace(**r['opt'])
        random.seed(r['seed'])
        assert len(r['draws']) == 32
        for i, want in enumerate(r['draws']):
            got = data.get_params(opt, tuple(r['size']))
            assert list(got['crop_pos']) == want['crop_pos'] and bool(got['flip']) == want['flip'] and list(got['crop_size']) == want['crop_size'], \
                (r['name'], r['seed'], i, got, want)


def _aligned_loader(seed_opt):
    pairs = [R.rgb(20, 10, 40 + i) for i in range(5)]
    return data.DeviceLoader.aligned(seed_opt, pairs, device='cpu')


@pytest.mark.parametrize('serial', [False, True])
def test_codes_dataset_under_the_stock_dataloader(serial):
    """5 items, batch 2: batches of 2 + 2 + 1 in the order a stock DataLoader gives a plain range under the same seed (RandomSampler's, or
    0..4), each row holding get_params' draws made in that order; equal seeds give equal codes."""
    opt = R.data_opt(load_size=12, crop_size=8, batch_size=2, serial_batches=serial)
    loader = _aligned_loader(opt)
    assert len(loader) == 3 and len(loader.dataset) == 5 and loader.load_data() is loader
    R.seed_all(7)
    codes = list(loader.dataloader)
    assert [tuple(c.shape) for c in codes] == [(2, 8), (2, 8), (1, 8)] and all(c.dtype == torch.int32 for c in codes)
    R.seed_all(7)
    order = [int(i) for b in torch.utils.data.DataLoader(range(5), batch_size=2, shuffle=not serial) for i in b]
    assert sorted(order) == list(range(5)) and (order == list(range(5))) == serial
    rows = torch.cat(codes)
    assert rows[:, 0].tolist() == order and rows[:, 1].tolist() == order
    random.seed(7)
    for row in rows.tolist():
        p = data.get_params(opt, (10, 10))
        want = [p['crop_pos'][0], p['crop_pos'][1], int(p['flip'])]
        assert row[2:5] == want and row[5:8] == want
    assert (rows[:, 2] <= 4).all() and (rows[:, 3] <= 4).all() and rows[:, 2:4].max() > 0
    R.seed_all(7)
    again = list(_aligned_loader(opt).dataloader)
    assert all(torch.equal(a, b) for a, b in zip(codes, again))
    R.seed_all(8)
    assert not torch.equal(torch.cat(list(loader.dataloader)), rows)


def test_no_flip_zeroes_the_flip_code_but_still_draws():
    opt = R.data_opt(load_size=12, crop_size=8, batch_size=5, serial_batches=True, no_flip=True)
    loader = _aligned_loader(opt)
    R.seed_all(3)
    rows = next(iter(loader.dataloader))
    assert rows[:, 4].tolist() == [0] * 5
    random.seed(3)
    assert [list(data.get_params(opt, (10, 10))['crop_pos']) for _ in range(5)] == rows[:, 2:4].tolist()


SRC = R.rgb(23, 17, 5)      # odd sizes, not square


@pytest.mark.parametrize('preprocess, load, want_size', [('resize_and_crop', 12, (12, 12)), ('scale_width', 12, (12, 8)), ('scale_width', 23, (23, 17)),
                                                         ('scale_width_and_crop', 12, (12, 8)), ('none', 12, (24, 16)), ('crop', 12, (23, 17))])
def test_host_prefix_equals_pil_called_directly(preprocess, load, want_size):
    opt = R.data_opt(preprocess=preprocess, load_size=load, crop_size=8)
    s = data.DeviceImageSet(opt, [SRC], device='cpu')
    want = SRC.convert('RGB')
    if preprocess == 'resize_and_crop':
        want = want.resize((12, 12), Image.BICUBIC)
    elif preprocess.startswith('scale_width') and load != 23:
        want = want.resize((12, int(12 * 17 / 23)), Image.BICUBIC)
    elif preprocess == 'none':
        want = want.resize((24, 16), Image.BICUBIC)
    assert (s.width, s.height) == want.size == want_size and s.sizes == [(23, 17)]
    assert s.data.dtype == torch.uint8 and tuple(s.data.shape) == (1, want_size[1], want_size[0], 4)
    assert np.array_equal(s.data[0, :, :, :3].numpy(), np.asarray(want)) and not s.data[..., 3].any()
    assert s.nbytes == s.data.numel() == want_size[0] * want_size[1] * 4
    # one channel: Grayscale(1) BEFORE the resize, byte 0 of the dword
    g = data.DeviceImageSet(opt, [SRC], grayscale=True, device='cpu')
    wg = R.resize(opt, SRC.convert('RGB').convert('L'), Image.BICUBIC)
    assert g.channels == 1 and np.array_equal(g.data[0, :, :, 0].numpy(), np.asarray(wg)) and not g.data[..., 1:].any()


def test_host_prefix_splits_pairs_and_resizes_maps_with_nearest():
    opt = R.data_opt(preprocess='resize_and_crop', load_size=12, crop_size=8)
    a, b = (data.DeviceImageSet(opt, [SRC], side=s, device='cpu') for s in 'AB')
    assert a.sizes == [(11, 17)] and b.sizes == [(12, 17)]      # w2 = int(23 / 2)
    assert np.array_equal(a.data[0, :, :, :3].numpy(), np.asarray(SRC.crop((0, 0, 11, 17)).resize((12, 12), Image.BICUBIC)))
    assert np.array_equal(b.data[0, :, :, :3].numpy(), np.asarray(SRC.crop((11, 0, 23, 17)).resize((12, 12), Image.BICUBIC)))
    rs = np.random.RandomState(2)
    lab = Image.fromarray(rs.randint(0, 256, size=(17, 23), dtype=np.uint8))
    ins = Image.fromarray(rs.randint(0, 40000, size=(17, 23)).astype(np.int32))
    opt = R.data_opt(preprocess='scale_width', load_size=12)
    ls, is_ = data.DeviceImageSet(opt, [lab], data.LABEL, device='cpu'), data.DeviceImageSet(opt, [ins], data.INSTANCE, device='cpu')
    assert ls.data.dtype == torch.uint8 and is_.data.dtype == torch.int32
    assert np.array_equal(ls.data[0].numpy(), np.asarray(lab.resize((12, 8), Image.NEAREST)))
    assert np.array_equal(is_.data[0].numpy(), np.asarray(ins.resize((12, 8), Image.NEAREST)))
    assert is_.nbytes == 12 * 8 * 4 and ls.nbytes == 12 * 8
    # arrays and paths are sources too
    arr = data.DeviceImageSet(opt, [np.asarray(SRC)], device='cpu')
    assert torch.equal(arr.data, data.DeviceImageSet(opt, [SRC], device='cpu').data)


def test_paths_are_opened_and_reported(tmp_path):
    p = tmp_path / 'a.png'
    SRC.save(p)
    opt = R.data_opt(preprocess='none')
    s = data.DeviceImageSet(opt, [str(p)], device='cpu')
    assert s.paths == [str(p)] and torch.equal(s.data, data.DeviceImageSet(opt, [SRC], device='cpu').data)


def test_mixed_sizes_and_max_bytes_are_refused():
    opt = R.data_opt(preprocess='scale_width', load_size=12)
    with pytest.raises(ValueError, match=r'item 2 .*12 x 6.*12 x 8'):
        data.DeviceImageSet(opt, [SRC, SRC, R.rgb(24, 12, 1)], device='cpu')
    with pytest.raises(ValueError, match=r'768 bytes.*max_bytes = 767'):
        data.DeviceImageSet(opt, [SRC, SRC], device='cpu', max_bytes=767)
    assert data.DeviceImageSet(opt, [SRC, SRC], device='cpu', max_bytes=768).nbytes == 768
    with pytest.raises(ValueError, match='max_bytes'):      # the B side of the pairs takes what the A side left
        data.DeviceLoader.aligned(R.data_opt(load_size=12, crop_size=8), [R.rgb(20, 10, 1)], device='cpu', max_bytes=12 * 12 * 4 + 1)


def test_configurations_the_reference_gets_wrong_are_refused():
    pairs = [R.rgb(20, 10, 1)]
    with pytest.raises(NotImplementedError, match='empty image'):
        data.DeviceLoader.aligned(R.data_opt(preprocess='crop', load_size=12, crop_size=8), pairs, device='cpu')
    lab = [Image.fromarray(np.zeros((10, 20), dtype=np.uint8))]
    with pytest.raises(NotImplementedError, match='empty image'):
        data.DeviceLoader.cityscapes(R.data_opt(preprocess='crop', load_size=12, crop_size=8), lab, [R.rgb(20, 10, 2)], device='cpu')
    # a crop window that can leave the resized image.  get_params works with new_h = load * h // w, __scale_width with int(load * h / w); where
    # the two disagree the window's last row is outside.  At sizes a test can hold the two agree, so the check is handed such a size directly:
    # a 12 x 7 image where get_params assumes 12 x 8 (crop 8 x 5, y up to 3)
    opt = R.data_opt(preprocess='scale_width_and_crop', load_size=12, crop_size=8)
    assert data._param_geometry(opt, [(23, 17)], 12, 8) == (8, 5, True)
    with pytest.raises(NotImplementedError, match='pad it with black'):
        data._param_geometry(opt, [(23, 17)], 12, 7)
    # unaligned data: RandomCrop of more than the image is an error of the configuration, as in torchvision
    with pytest.raises(ValueError, match='larger than the image'):
        data.DeviceLoader.single(R.data_opt(preprocess='crop', crop_size=24), [SRC], device='cpu')


def test_codes_are_validated_on_the_host():
    opt = R.data_opt(load_size=12, crop_size=8, batch_size=2)
    loader = _aligned_loader(opt)
    ok = torch.tensor([[4, 4, 4, 4, 1, 4, 4, 1]], dtype=torch.int32)
    assert torch.equal(loader.validate(ok), ok)
    for col, bad in ((0, 5), (0, -1), (2, 5), (3, -1), (4, 2), (6, 5)):
        c = ok.clone()
        c[0, col] = bad
        with pytest.raises(ValueError, match='codes outside plane'):
            loader.validate(c)
    with pytest.raises(ValueError, match=r'\[n, 8\]'):
        loader.validate(torch.zeros((1, 5), dtype=torch.int32))


def test_eval_loader_applies_the_reference_overrides():
    opt = R.data_opt(dataset_mode='unaligned', load_size=12, crop_size=8, batch_size=4, eval_batch_size=2)
    ev = data.eval_loader(opt, [R.rgb(23, 17, i) for i in range(3)], device='cpu')
    assert ev.mode == 'single' and ev.batch_size == 2 and len(ev) == 2
    assert ev.opt.load_size == 8 and ev.opt.no_flip and ev.opt.serial_batches and opt.load_size == 12 and not opt.no_flip
    assert (ev.planes[0].set.width, ev.planes[0].set.height) == (8, 8)
    state = torch.get_rng_state()
    rows = torch.cat(list(ev.dataloader))
    assert rows.tolist() == [[i, 0, 0, 0, 0] for i in range(3)]
    # equal sizes and no_flip: the transform draws nothing (the stock DataLoader itself draws its base seed, once per iter())
    torch.set_rng_state(state)
    torch.empty((), dtype=torch.int64).random_()
    after = torch.get_rng_state()
    torch.set_rng_state(state)
    list(ev.dataloader)
    assert torch.equal(torch.get_rng_state(), after)
