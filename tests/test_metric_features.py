"""CPU: what the feature loops of FID and KID must keep (cat_amd/metric/features.py and its three callers), on a stand-in network: batching,
the short or dropped last batch, the in-place scaling, dtypes, the warnings, the checkpoint error and the shared command-line arguments."""
import argparse

import numpy as np
import pytest
import torch

from cat_amd.metric import features as FT
from cat_amd.metric import fid_score as F
from cat_amd.metric import kid_score as K

CPU = torch.device('cpu')
REPEAT = 2      # the stand-in's features: the 3 channel means, repeated
DIMS = 3 * REPEAT


class _Means(torch.nn.Module):
    """[x.mean((2, 3)).repeat(1, k)[..., None, None]] of a [B, 3, H, W] batch (size=1), or the same on a 2 x 2 map whose mean it is (size=2)"""

    def __init__(self, size=1):
        super().__init__()
        self.size, self.batches = size, []

    def forward(self, x):
        assert x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and not torch.is_grad_enabled()
        self.batches.append(x.shape[0])
        y = x.mean((2, 3)).repeat(1, REPEAT)[..., None, None]
        if self.size == 1:
            return [y]
        return [y * torch.tensor([[0.5, 1.5], [0.25, 1.75]])]      # the four factors average to 1


def _images():
    return np.random.RandomState(0).uniform(0, 255, size=(5, 6, 8, 3))      # NHWC float64 in [0, 255]


def _want(ims):
    return np.tile((ims / 255).transpose((0, 3, 1, 2)).astype(np.float32).mean(axis=(2, 3)), (1, REPEAT))


def test_fid_host_loop_scales_in_place_and_keeps_the_short_batch():
    ims, model = _images(), _Means()
    keep = ims.copy()
    act = F.get_activations_from_ims(ims, model, batch_size=2, dims=DIMS, device=CPU, use_tqdm=False)
    assert model.batches == [2, 2, 1] and not model.training
    assert np.array_equal(ims, keep / 255)                                  # the caller's array, divided in place
    assert act.shape == (5, DIMS) and act.dtype == np.float64
    assert np.abs(act - _want(keep)).max() < 1e-6


def test_fid_device_loop_returns_the_same_values_as_float32():
    ims, model = _images(), _Means()
    host = F.get_activations_from_ims(ims.copy(), _Means(), batch_size=2, dims=DIMS, device=CPU, use_tqdm=False)
    feats = F.get_activations_device(ims, model, batch_size=2, dims=DIMS, device=CPU)
    assert model.batches == [2, 2, 1]
    assert isinstance(feats, torch.Tensor) and feats.dtype == torch.float32 and feats.shape == (5, DIMS)
    assert np.array_equal(feats.numpy().astype(np.float64), host)


def test_kid_loop_drops_the_remainder_or_clamps_the_batch(capsys):
    ims = np.random.RandomState(1).randint(0, 256, size=(5, 6, 8, 3)).astype(np.uint8)
    want = np.tile((ims.astype(np.float32) / 255.).mean(axis=(1, 2)), (1, REPEAT))
    model = _Means()
    act = K._activations(K._load_uint8(ims), 5, model, 2, DIMS, CPU, False)
    text = capsys.readouterr().out
    assert 'not a multiple of the batch size' in text and 'Setting batch size to data size' not in text
    assert act.shape == (4, DIMS) and act.dtype == np.float64 and model.batches == [2, 2]
    assert np.abs(act - want[:4]).max() < 1e-6
    model = _Means()
    act = K._activations(K._load_uint8(ims), 5, model, 9, DIMS, CPU, False)
    text = capsys.readouterr().out
    assert 'Setting batch size to data size' in text
    assert act.shape == (5, DIMS) and model.batches == [5]
    assert np.abs(act - want).max() < 1e-6


def test_pooled_features_average_a_block_below_pool3():
    x = torch.from_numpy(np.random.RandomState(2).random_sample((3, 3, 4, 4)).astype(np.float32))
    flat = FT.pooled_features(_Means(), x)
    pooled = FT.pooled_features(_Means(size=2), x, pool=lambda t: t.mean((2, 3), keepdim=True))
    assert flat.shape == pooled.shape == (3, DIMS) and flat.dtype == pooled.dtype == torch.float32
    assert (flat - pooled).abs().max() < 1e-6
    batches = list(FT.feature_batches(lambda s, e: x[s:e].numpy(), 3, _Means(size=2), 2, CPU, pool=lambda t: t.mean((2, 3), keepdim=True)))
    assert [(s, e) for s, e, _ in batches] == [(0, 2), (2, 3)]
    assert list(FT.feature_batches(lambda s, e: x[s:e].numpy(), 3, _Means(), 2, CPU, full_only=True))[-1][:2] == (0, 2)


def test_load_inception_never_downloads_and_hands_a_module_back_in_eval_mode():
    with pytest.raises(RuntimeError, match='KID needs the FID InceptionV3 checkpoint'):
        FT.load_inception(2048, None, 'cpu')
    with pytest.raises(RuntimeError, match='FID needs the FID InceptionV3 checkpoint .*does not download'):
        FT.load_inception(2048, None, 'cpu', 'FID')
    model = _Means().train()
    assert FT.load_inception(2048, model, 'cpu') is model and not model.training
    assert K._inception_for(2048, model.train(), 'cpu') is model and not model.training


def test_both_command_lines_share_their_inception_arguments():
    for batch_size in (2, 32):
        parser = FT.add_inception_arguments(argparse.ArgumentParser(), batch_size=batch_size)
        a = parser.parse_args(['--inception-path', 'ckpt.pth'])
        assert (a.batch_size, a.dims, a.gpu, a.inception_path) == (batch_size, 2048, '0', 'ckpt.pth')
        with pytest.raises(SystemExit):
            parser.parse_args([])
    # what test_command_line_arguments (KID) and test_command_line_parses (FID) give the two command lines
    a = K.parse_args(['--real', 'R', '--fake', 'F1', 'F2', '--inception-path', 'ckpt.pth'])
    assert (a.real, a.fake, a.batch_size, a.dims, a.gpu, a.inception_path) == ('R', ['F1', 'F2'], 2, 2048, '0', 'ckpt.pth')
    a = K.parse_args(['--real', 'R', '--fake', 'F', '--batch-size', '8', '--dims', '768', '-c', '3', '--inception-path', 'p'])
    assert (a.batch_size, a.dims, a.gpu) == (8, 768, '3')
    a = F.parse_args(['--images', 'real', '--output', 'x.npz', '--inception-path', 'ckpt.pth'])
    assert (a.images, a.output, a.inception_path, a.batch_size, a.dims, a.gpu) == ('real', 'x.npz', 'ckpt.pth', 32, 2048, '0')
    a = F.parse_args(['--images', 'r.npy', '--output', 'x.npz', '--inception-path', 'c', '--batch-size', '4', '--dims', '192', '--gpu', '1'])
    assert (a.batch_size, a.dims, a.gpu) == (4, 192, '1')
    for parse, argv in ((K.parse_args, ['--real', 'R', '--fake', 'F', '--inception-path', 'p', '--dims', '100']),
                        (F.parse_args, ['--images', 'r', '--output', 'x', '--inception-path', 'c', '--dims', '100'])):
        with pytest.raises(SystemExit):
            parse(argv)
