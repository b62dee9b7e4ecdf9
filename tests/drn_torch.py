"""Test helper: the DRN-D segmentation network of the cityscapes mIoU restated in plain torch functional ops, written from the architecture
(dilated residual network, architecture D; DRNSeg head = 1x1 classifier + grouped 16/8/4 transposed conv + log-softmax) over a state_dict with
the reference's keys.  It gives float64 ground truth on any input shape; tests/test_metric_drn.py pins it to the recorded run of the
reference (tests/golden/drn_miou.npz).  Also the seeded label generator that the fixture's generator and the tests share."""
import os

import numpy as np
import torch
import torch.nn.functional as F

LAYERS = {'drn_d_105': ('bottleneck', [1, 1, 3, 4, 23, 3, 1, 1]), 'drn_d_22': ('basic', [1, 1, 2, 2, 2, 2, 1, 1])}
EPS = 1e-5


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + '.running_mean'], sd[p + '.running_var'], sd[p + '.weight'], sd[p + '.bias'], False, 0.0, EPS)


def _conv_layers(sd, p, x, convs, stride, dil):
    for i in range(convs):
        x = F.conv2d(x, sd['%s.%d.weight' % (p, 3 * i)], None, stride if i == 0 else 1, dil, dil)
        x = F.relu(_bn(sd, '%s.%d' % (p, 3 * i + 1), x))
    return x


def _block(sd, p, x, kind, stride, dil):
    res = x
    if p + '.downsample.0.weight' in sd:
        res = _bn(sd, p + '.downsample.1', F.conv2d(x, sd[p + '.downsample.0.weight'], None, stride))
    if kind == 'bottleneck':
        out = F.relu(_bn(sd, p + '.bn1', F.conv2d(x, sd[p + '.conv1.weight'])))
        out = F.relu(_bn(sd, p + '.bn2', F.conv2d(out, sd[p + '.conv2.weight'], None, stride, dil[1], dil[1])))
        out = _bn(sd, p + '.bn3', F.conv2d(out, sd[p + '.conv3.weight']))
    else:
        out = F.relu(_bn(sd, p + '.bn1', F.conv2d(x, sd[p + '.conv1.weight'], None, stride, dil[0], dil[0])))
        out = _bn(sd, p + '.bn2', F.conv2d(out, sd[p + '.conv2.weight'], None, 1, dil[1], dil[1]))
    return F.relu(out + res)


def _stage(sd, p, x, kind, blocks, stride=1, dilation=1, new_level=True):
    first = (1, 1) if dilation == 1 else ((dilation // 2 if new_level else dilation), dilation)
    x = _block(sd, p + '.0', x, kind, stride, first)
    for b in range(1, blocks):
        x = _block(sd, '%s.%d' % (p, b), x, kind, 1, (dilation, dilation))
    return x


def drnseg_forward(sd, x, name='drn_d_105', dtype=torch.float64, head=True):
    """(log-softmax map [N, C, H, W], seg logits [N, C, H/8, W/8]) of DRNSeg(name, C) with the weights `sd`, computed in `dtype` on x's device."""
    kind, layers = LAYERS[name]
    sd = {k: (v.to(device=x.device, dtype=dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = x.to(dtype)
    with torch.no_grad():
        x = F.relu(_bn(sd, 'base.0.1', F.conv2d(x, sd['base.0.0.weight'], None, 1, 3)))
        x = _conv_layers(sd, 'base.1', x, layers[0], 1, 1)
        x = _conv_layers(sd, 'base.2', x, layers[1], 2, 1)
        x = _stage(sd, 'base.3', x, kind, layers[2], stride=2)
        x = _stage(sd, 'base.4', x, kind, layers[3], stride=2)
        x = _stage(sd, 'base.5', x, kind, layers[4], dilation=2, new_level=False)
        x = _stage(sd, 'base.6', x, kind, layers[5], dilation=4, new_level=False)
        x = _conv_layers(sd, 'base.7', x, layers[6], 1, 2)
        x = _conv_layers(sd, 'base.8', x, layers[7], 1, 1)
        logits = F.conv2d(x, sd['seg.weight'], sd['seg.bias'])
        if not head:      # the network up to the class logits only
            return None, logits
        c = logits.shape[1]
        up = F.conv_transpose2d(logits, sd['up.weight'], None, stride=8, padding=4, groups=c)
        return F.log_softmax(up, dim=1), logits


# SegList's constants, restated for the test inputs
MEAN = [0.29010095242892997, 0.32808144844279574, 0.28696394422942517]
STD = [0.1829540508368939, 0.18656561047509476, 0.18447508988480435]


def normalized_input(ims_u8):
    """uint8 [N, H, W, 3] -> float32 [N, 3, H, W]: / 255, then (x - mean) / std in float32."""
    x = torch.from_numpy(np.ascontiguousarray(ims_u8)).permute(0, 3, 1, 2).contiguous().float() / 255
    for c in range(3):
        x[:, c] = (x[:, c] - torch.tensor(MEAN[c], dtype=torch.float32)) / torch.tensor(STD[c], dtype=torch.float32)
    return x


def fakes_to_u8(fakes):
    """[-1, 1] NCHW float tensor -> uint8 NHWC with the truncating cast of the reference's tensor2im."""
    a = fakes.detach().cpu().float().numpy()
    return np.clip((np.transpose(a, (0, 2, 3, 1)) + 1) / 2.0 * 255.0, 0, 255).astype(np.uint8)


def make_labels(seed, n, classes, size=(1024, 2048), block=(64, 128)):
    """Blocky seeded label maps, uint8 [n, H, W]: every block of `block` pixels gets one entry of `classes` (which holds 255 = ignore)."""
    rng = np.random.default_rng(seed)
    gh, gw = size[0] // block[0], size[1] // block[1]
    idx = rng.integers(0, len(classes), size=(n, gh, gw))
    lab = np.asarray(classes, dtype=np.uint8)[idx]
    return np.repeat(np.repeat(lab, block[0], axis=1), block[1], axis=2)


def write_label_set(root, labels, names):
    """Label PNGs + table.txt (`<id> <label path> <image path>`, the layout the name matching reads) under `root`; returns the table path."""
    from PIL import Image
    os.makedirs(os.path.join(root, 'gtFine'), exist_ok=True)
    lines = []
    for i, (lab, name) in enumerate(zip(labels, names)):
        rel = os.path.join('gtFine', '%s_labelTrainIds.png' % name)
        Image.fromarray(lab).save(os.path.join(root, rel))
        lines.append('%d %s leftImg8bit/%s.png' % (i + 1000, rel, name))
    table = os.path.join(root, 'table.txt')
    with open(table, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return table


def bilinear_resize64(t, size):
    """float64 F.interpolate(mode='bilinear', align_corners=False): the half-pixel, clamped-edge form of PIL's bilinear enlargement."""
    return F.interpolate(t.double(), size=size, mode='bilinear', align_corners=False)
