"""cat_amd.data.DeviceLoader on the GPU against test-local host data sets (tests/data_host_ref.py) under the same seeds: the host side runs
the reference's chain per sample with PIL and torch and is batched by a stock DataLoader built as the reference builds its own.  Batches are
compared bit-exactly (torch.equal), the path lists and the short last batch included."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import data_host_ref as R
import helpers as H

pytestmark = pytest.mark.gpu


def _nchw(t):
    from cat_amd import ops
    assert ops.is_act(t)
    return ops.to_nchw(t).cpu()


def _both(seed, loader, host_set):
    """The loader's batches and the host data set's, each under the same seeds"""
    R.seed_all(seed)
    mine = list(loader)
    R.seed_all(seed)
    return mine, R.host_batches(loader.opt, host_set)


@pytest.mark.parametrize('no_flip', [False, True])
@pytest.mark.parametrize('serial', [False, True])
def test_aligned(serial, no_flip):
    """5 pairs of 20 x 10, load 12, crop 8, batch 2 (2 + 2 + 1); the B side has one channel (Grayscale before the resize)."""
    from cat_amd import data
    opt = R.data_opt(load_size=12, crop_size=8, batch_size=2, serial_batches=serial, no_flip=no_flip, output_nc=1)
    pairs = [R.rgb(20, 10, 100 + i) for i in range(5)]
    loader = data.DeviceLoader.aligned(opt, pairs)
    names = ['<memory:%d>' % i for i in range(5)]
    mine, host = _both(11, loader, R.HostAligned(opt, pairs, names))
    assert len(mine) == len(host) == len(loader) == 3 and [b['A'].shape[0] for b in mine] == [2, 2, 1]
    for m, h in zip(mine, host):
        assert sorted(m) == ['A', 'A_paths', 'B', 'B_paths']
        assert tuple(m['A'].shape) == tuple(h['A'].shape) and tuple(m['B'].shape) == tuple(h['B'].shape) and m['B'].shape[1] == 1
        assert torch.equal(_nchw(m['A']), h['A']) and torch.equal(_nchw(m['B']), h['B'])
        assert m['A_paths'] == list(h['A_paths']) and m['B_paths'] == list(h['B_paths'])
    order = [int(p.split(':')[1][:-1]) for m in mine for p in m['A_paths']]
    assert sorted(order) == list(range(5)) and (order == list(range(5))) == serial
    # a second epoch draws again: other crops, the same surface
    again = list(loader)
    assert [b['A'].shape[0] for b in again] == [2, 2, 1]


def test_unaligned_sides_crop_independently():
    from cat_amd import data
    opt = R.data_opt(dataset_mode='unaligned', load_size=12, crop_size=8, batch_size=2)
    A, B = [R.rgb(14, 11, 200 + i) for i in range(4)], [R.rgb(9, 16, 300 + i) for i in range(3)]
    loader = data.DeviceLoader.unaligned(opt, A, B)
    na, nb = ['<memory:%d>' % i for i in range(4)], ['<memory:%d>' % i for i in range(3)]
    host_set = R.HostUnaligned(opt, A, B, na, nb)
    mine, host = _both(12, loader, host_set)
    assert len(loader.dataset) == 4 and len(mine) == len(host) == 2
    for m, h in zip(mine, host):
        assert torch.equal(_nchw(m['A']), h['A']) and torch.equal(_nchw(m['B']), h['B'])
        assert m['A_paths'] == list(h['A_paths']) and m['B_paths'] == list(h['B_paths'])
    assert any(pa != pb for _, pa, pb in host_set.positions)      # the two sides drew their own windows
    # serial_batches: the partner is index % B_size, nothing is drawn for it
    opt = R.data_opt(dataset_mode='unaligned', load_size=12, crop_size=8, batch_size=4, serial_batches=True)
    loader = data.DeviceLoader.unaligned(opt, A, B)
    mine, host = _both(13, loader, R.HostUnaligned(opt, A, B, na, nb))
    assert mine[0]['B_paths'] == ['<memory:0>', '<memory:1>', '<memory:2>', '<memory:0>'] == list(host[0]['B_paths'])
    assert torch.equal(_nchw(mine[0]['A']), host[0]['A']) and torch.equal(_nchw(mine[0]['B']), host[0]['B'])


def _city_sources(n):
    rs = np.random.RandomState(9)
    labels, images, instances = [], [], []
    for i in range(n):
        lab = rs.randint(0, 34, size=(16, 32)).astype(np.uint8)
        lab[rs.rand(16, 32) < 0.1] = 255
        ins = rs.randint(0, 34, size=(16, 32)).astype(np.int32)
        ins[rs.rand(16, 32) < 0.2] = 33001
        labels.append(Image.fromarray(lab))
        instances.append(Image.fromarray(ins))
        images.append(R.rgb(32, 16, 400 + i))
    return labels, images, instances


def test_cityscapes():
    """scale_width with load 16 on 32 x 16 sources gives 16 x 8: label (NEAREST, 255 -> input_nc), image, instance (int32)."""
    from cat_amd import data
    opt = R.data_opt(dataset_mode='cityscapes', preprocess='scale_width', load_size=16, crop_size=16, batch_size=2, input_nc=35, direction='BtoA')
    labels, images, instances = _city_sources(3)
    loader = data.DeviceLoader.cityscapes(opt, labels, images, instances)
    names = ['<memory:%d>' % i for i in range(3)]
    with R.Launches() as log:
        mine, host = _both(14, loader, R.HostCityscapes(opt, labels, images, instances, names))
    assert log.names == ['cat_data_batch'] * 2
    for m, h in zip(mine, host):
        assert sorted(m) == ['image', 'instance', 'label', 'path'] and m['path'] == list(h['path'])
        n = len(m['path'])
        assert tuple(m['label'].shape) == (n, 1, 8, 16) and m['label'].dtype == torch.float32 and m['label'].is_contiguous()
        assert torch.equal(m['label'].cpu(), h['label']) and float(m['label'].max()) == 35.0
        assert m['instance'].dtype == torch.int32 and torch.equal(m['instance'].cpu(), h['instance'])
        assert torch.equal(_nchw(m['image']), h['image'])
    assert [len(m['path']) for m in mine] == [2, 1]
    # --no_instance: the reference's collated 0
    loader = data.DeviceLoader.cityscapes(opt, labels, images)
    R.seed_all(14)
    b = next(iter(loader))
    assert torch.equal(b['instance'], torch.zeros(2, dtype=torch.int64)) and torch.equal(b['label'], mine[0]['label'])


def test_eval_loader():
    """create_eval_dataloader's overrides on unaligned data: the `single` keys, no flip, serial order, load_size = crop_size."""
    from cat_amd import data
    opt = R.data_opt(dataset_mode='unaligned', load_size=12, crop_size=8, batch_size=4, eval_batch_size=2)
    A = [R.rgb(14, 11, 500 + i) for i in range(3)]
    loader = data.eval_loader(opt, A)
    names = ['<memory:%d>' % i for i in range(3)]
    mine, host = _both(15, loader, R.HostSingle(loader.opt, A, names))
    assert [sorted(m) for m in mine] == [['A', 'A_paths']] * 2 and [m['A_paths'] for m in mine] == [names[:2], names[2:]]
    for m, h in zip(mine, host):
        assert torch.equal(_nchw(m['A']), h['A']) and tuple(m['A'].shape[1:]) == (3, 8, 8)
    direct = torch.stack([R.normalize(R.to_tensor(a.resize((8, 8), Image.BICUBIC))) for a in A])
    assert torch.equal(torch.cat([_nchw(m['A']) for m in mine]), direct)


def _distiller():
    g = H.load('step_bn.npz')
    meta = json.loads(str(g['meta']))
    opt = H.make_opt(norm=meta['norm'], track=meta['track'], ndf=meta['ndf'], dataset_mode=meta['dataset_mode'], gan_mode=meta['gan_mode'],
                     lambda_recon=meta['lambda_recon'], lambda_distill=meta['lambda_distill'], student_ngf=16)
    return H.build_distiller(opt, g['student_shapes']), meta


def test_set_input_passes_a_loader_batch_through():
    """One set_input + optimize_parameters of the smallest distiller the step tests build (64 x 64, batch 2): fed a DeviceLoader batch, the losses
    are bit-identical to the same batch handed over as host NCHW tensors, and no layout launch is issued for the images."""
    from cat_amd import data
    (fed, meta), (hosted, _) = _distiller(), _distiller()
    s, n = meta['size'], meta['nbatch']
    opt = R.data_opt(load_size=s + 6, crop_size=s, batch_size=n)
    loader = data.DeviceLoader.aligned(opt, [R.rgb(40, 20, 600 + i) for i in range(n)])
    R.seed_all(16)
    batch = next(iter(loader))
    assert tuple(batch['A'].shape) == (n, 3, s, s)
    host_batch = {k: (_nchw(v) if torch.is_tensor(v) else v) for k, v in batch.items()}
    with R.Launches() as log:
        fed.set_input(batch)
    assert log.names == [] and fed.real_A is batch['A'] and fed.real_B is batch['B']
    with R.Launches() as log:
        hosted.set_input(host_batch)
    assert log.names == ['cat_nchw_to_nhwc'] * 2
    fed.optimize_parameters(0)
    hosted.optimize_parameters(0)
    lf, lh = fed.get_current_losses(), hosted.get_current_losses()
    assert lf and sorted(lf) == sorted(lh)
    for k in lf:
        assert lf[k] == lh[k], (k, lf[k], lh[k])


def test_graphed_step_takes_batches_filled_into_its_static_inputs():
    """GraphedStep over the small CycleGAN of tests/test_image_pool_gpu.py: the example batch comes from the loader, every later batch is written
    by fill(codes, out=step.static) -- no copy, no layout launch -- and the replays equal eager steps on the same batches (the criterion of
    tests/test_graph_gpu.py); what the static inputs hold is compared bit-exactly."""
    from cat_amd import data, ops
    from cat_amd.graph import GraphedStep
    from test_graph_gpu import _max_param_diff
    from test_image_pool_gpu import _cyclegan
    (eager, _, _), (graphed, _, _) = _cyclegan(2), _cyclegan(2)
    opt = R.data_opt(dataset_mode='unaligned', load_size=70, crop_size=64, batch_size=1)
    loader = data.DeviceLoader.unaligned(opt, [R.rgb(80, 72, 700 + i) for i in range(4)], [R.rgb(76, 90, 800 + i) for i in range(3)])
    R.seed_all(17)
    codes = list(loader.dataloader)
    assert len(codes) == 4 and not torch.equal(codes[1][:, 2:], codes[2][:, 2:])
    example = loader.fill(codes[0])
    for i in range(3):
        eager.set_input(example)
        eager.optimize_parameters(i)
    step = GraphedStep(graphed, example, warmup=3)
    assert ops.is_act(step.static['A']) and step.static['A'] is not example['A'] and torch.equal(step.static['A'], example['A'])
    for i, c in ((3, codes[1]), (4, codes[2])):
        b = loader.fill(c)
        eager.set_input(b)
        eager.optimize_parameters(i)
        with R.Launches() as log:
            filled = loader.fill(c, out=step.static)
        assert log.names == ['cat_data_batch'] and filled['A'] is step.static['A'] and filled['B'] is step.static['B']
        step(filled)
        assert torch.equal(step.static['A'], b['A']) and torch.equal(step.static['B'], b['B'])
        assert graphed.real_A is step.static['A']
        le, lg = eager.get_current_losses(), graphed.get_current_losses()
        assert len(le) == 8
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-5 * max(1.0, abs(le[k])), (i, k, le[k], lg[k])
    assert step.replays == 2
    for name in ('netG_A', 'netG_B', 'netD_A', 'netD_B'):
        assert _max_param_diff(getattr(graphed, name), getattr(eager, name)) < 1e-5, name
