"""What FID and KID share in front of their arithmetic: the InceptionV3 from a checkpoint, the loop that pushes batches of images through it and
the command-line arguments for both.  fid_score.py and kid_score.py keep what differs: how images are loaded and scaled, and what is returned."""
import os

import torch

from .inception import GlobalAvgPool, InceptionV3


def default_device(device):
    return torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())


def load_inception(dims, inception, device, metric='KID'):
    """The InceptionV3 of the `dims`-wide block on `device`, in eval mode.  inception: the torchvision-keyed FID checkpoint (path or state_dict)
    or a ready module; `metric` names the caller in the error for a missing checkpoint."""
    block_idx = InceptionV3.BLOCK_INDEX_BY_DIM[dims]
    if isinstance(inception, torch.nn.Module):
        return inception.to(device).eval()
    if inception is None:
        raise RuntimeError('%s needs the FID InceptionV3 checkpoint (pt_inception-2015-12-05-6726825d.pth, torchvision keys): pass its path '
                           'or state_dict; this package does not download it' % metric)
    if isinstance(inception, (str, bytes, os.PathLike)):
        inception = torch.load(inception, map_location='cpu')
    model = InceptionV3([block_idx])
    model.load_fid_state_dict(inception)
    return model.to(device).eval()


def pooled_features(model, batch, pool=None):
    """float32 [B, dims] features of a float32 [B, 3, H, W] device batch.  pool: what averages a block below pool3 (default: GlobalAvgPool)."""
    with torch.no_grad():
        pred = model(batch)[0]
    if pred.shape[2] != 1 or pred.shape[3] != 1:      # a block below pool3 was selected: adaptive_avg_pool2d(pred, (1, 1))
        pred = (pool or GlobalAvgPool())(pred)
    return pred.reshape(pred.shape[0], -1).float()


def feature_batches(load, n, model, batch_size, device, full_only=False, pool=None):
    """Yields (start, end, features) per batch of n images; load(start, end) returns the [B, 3, H, W] numpy batch as the network takes it, or
    the same batch as a float32 device tensor (DeviceImages.batch), which goes in as it is.
    full_only: images beyond the last full batch are dropped; otherwise the last batch may be short."""
    model.eval()
    stop = n - n % batch_size if full_only else n
    for start in range(0, stop, batch_size):
        end = min(start + batch_size, stop)
        batch = load(start, end)
        if not isinstance(batch, torch.Tensor):
            batch = torch.from_numpy(batch).type(torch.FloatTensor).to(device)
        yield start, end, pooled_features(model, batch, pool)


def add_inception_arguments(parser, batch_size):      # returns the parser
    parser.add_argument('--batch-size', type=int, default=batch_size, help='Batch size to use')
    parser.add_argument('--dims', type=int, default=2048, choices=list(InceptionV3.BLOCK_INDEX_BY_DIM),
                        help='Dimensionality of Inception features to use. By default, uses pool3 features')
    parser.add_argument('-c', '--gpu', default='0', type=str, help='GPU to use (there is no CPU path)')
    parser.add_argument('--inception-path', type=str, required=True,
                        help='the FID InceptionV3 checkpoint with torchvision keys (pt_inception-2015-12-05-6726825d.pth); never downloaded')
    return parser
