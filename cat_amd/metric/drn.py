"""The cityscapes segmentation network of the mIoU metric on the HIP kernels: DRN-D (dilated residual network) + the DRNSeg head.

Reference: metric/drn.py (DRN, BasicBlock, Bottleneck, drn_d_22 / drn_d_105) and metric/mIoU_score.py:127-168 (DRNSeg), built by the distillers at
base_inception_distiller.py:226-232 / base_spade_distiller.py:166-170 as `DRNSeg('drn_d_105', 19, pretrained=False)`.

Inference only (the reference never trains it).  Every conv -> BatchNorm2d(eps 1e-5) [-> ReLU] is ONE implicit-GEMM launch of
cat_conv2d_fwd_ex: the running statistics are folded into the filters and a bias once (refreshed when a tensor changes), the ReLU is the
epilogue, the 3 x 3 filters of layers 5 - 8 run with their taps 2 / 4 pixels apart, and the last 1 x 1 of a bottleneck adds the shortcut
BEFORE the ReLU in the same epilogue (`out += residual; relu`, metric/drn.py:116-123) -- the shortcut is the block input, or the output of
the activation-free `downsample` conv.  The head (`up` + LogSoftmax) is csrc/seg_ops.hip's cat_seg_up_logsoftmax.

Module / parameter names are the reference's (`base.0.0.weight`, `base.5.3.bn2.running_var`, ..., `seg.bias`, `up.weight`: 651 entries for
drn_d_105), so `load_state_dict` takes the reference's `--drn_path` checkpoint unchanged.  The conv / norm sub-modules are parameter
holders: they are never called."""
import ctypes as C
import math

import torch
import torch.nn as nn

from .. import _lib as L
from .. import nn as cnn
from .. import ops

BN_EPS = 1e-5


def _folded(conv, bn):
    """(filters in the kernels' padded channels-last storage with the BatchNorm scale folded in, wcs, bias) of a conv + eval BatchNorm pair,
    or of a bare conv (bn None); cached on the conv holder, refreshed when a tensor changes."""
    return cnn.folded_metric_conv(conv, conv, bn)


def conv_bn_act(x, conv, bn, act, res=None):
    """act(BatchNorm(conv(x)) + res) in one launch.  x / res: NHWC activations; conv: the nn.Conv2d holder (square kernel, its own
    stride / padding / dilation); bn: the nn.BatchNorm2d holder or None."""
    w, wcs, bias = _folded(conv, bn)
    n, c, h, wd = x.shape
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = conv.kernel_size, conv.stride, conv.padding, conv.dilation
    if kh != kw or sh != sw or ph != pw or dh != dw or c != conv.in_channels or conv.groups != 1:
        raise ValueError('drn conv: geometry')
    ho, wo = (h + 2 * ph - dh * (kh - 1) - 1) // sh + 1, (wd + 2 * ph - dh * (kw - 1) - 1) // sh + 1
    cout = conv.out_channels
    y = ops.empty_act(n, cout, ho, wo, x.device)
    if res is not None and tuple(res.shape) != tuple(y.shape):
        raise ValueError('drn conv: residual shape %s vs output %s' % (tuple(res.shape), tuple(y.shape)))
    g = ops._conv_geom(n, h, wd, c, ops.act_cs(x), ho, wo, cout, ops.act_cs(y), kh, kw, sh, ph, L.PAD_ZERO, act, 0.0, ycw=ops.act_cs(y), wcs=wcs)
    L.call('cat_conv2d_fwd_ex', C.byref(g), dh, ops._p(x), ops._p(w), ops._p(bias), ops._p(res), ops.act_cs(res) if res is not None else 0, ops._p(y),
           ops._stream())
    return y


def _bn(c):
    return nn.BatchNorm2d(c, eps=BN_EPS)


def _shortcut(cin, cout, stride):
    """The projection on the shortcut of a stage's first block (1x1 conv, possibly strided, + BatchNorm, no activation) when the block changes
    the width or the resolution; None = the block input itself."""
    if stride == 1 and cin == cout:
        return None
    return nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride, bias=False), _bn(cout))


def _shortcut_value(block, x):
    return x if block.downsample is None else conv_bn_act(x, block.downsample[0], block.downsample[1], L.ACT_NONE)


class BasicBlock(nn.Module):
    """Two 3x3 convs (the first one strided), both at the stage's dilation; relu(bn2(conv2(.)) + shortcut) is the second launch's epilogue."""
    expansion = 1

    def __init__(self, cin, width, stride, dilation):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 3, stride=stride, padding=dilation, bias=False, dilation=dilation)
        self.bn1 = _bn(width)
        self.conv2 = nn.Conv2d(width, width, 3, padding=dilation, bias=False, dilation=dilation)
        self.bn2 = _bn(width)
        self.downsample = _shortcut(cin, width, stride)

    def forward(self, x):
        res = _shortcut_value(self, x)
        out = conv_bn_act(x, self.conv1, self.bn1, L.ACT_RELU)
        return conv_bn_act(out, self.conv2, self.bn2, L.ACT_RELU, res)


class Bottleneck(nn.Module):
    """1x1 -> 3x3 (strided / dilated) -> 1x1 to 4 x width; the shortcut is added before the last ReLU, in the third launch's epilogue."""
    expansion = 4

    def __init__(self, cin, width, stride, dilation):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = _bn(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=dilation, bias=False, dilation=dilation)
        self.bn2 = _bn(width)
        self.conv3 = nn.Conv2d(width, 4 * width, 1, bias=False)
        self.bn3 = _bn(4 * width)
        self.downsample = _shortcut(cin, 4 * width, stride)

    def forward(self, x):
        res = _shortcut_value(self, x)
        out = conv_bn_act(x, self.conv1, self.bn1, L.ACT_RELU)
        out = conv_bn_act(out, self.conv2, self.bn2, L.ACT_RELU)
        return conv_bn_act(out, self.conv3, self.bn3, L.ACT_RELU, res)


class ConvLayers(nn.Sequential):
    """A run of [Conv2d, BatchNorm2d, ReLU] triples (the state_dict numbers them 0, 1, 3, 4, ...); every triple is one launch."""

    def forward(self, x):
        mods = list(self)
        for i in range(0, len(mods), 3):
            x = conv_bn_act(x, mods[i], mods[i + 1], L.ACT_RELU)
        return x


def _conv_run(cin, width, count, k, stride, dilation):
    mods = []
    for i in range(count):
        mods += [nn.Conv2d(cin if i == 0 else width, width, k, stride=stride if i == 0 else 1, padding=dilation * (k - 1) // 2, bias=False,
                           dilation=dilation), _bn(width), nn.ReLU(inplace=True)]
    return ConvLayers(*mods)


# Architecture D after the 7x7 stem, stage by stage: (kind, width, stride of the stage's first layer, dilation of all its 3x3 convs).
# 'conv' = a run of 3x3 conv + BN + ReLU, 'res' = residual blocks (basic or bottleneck by depth).  Resolution: 1, 1/2, 1/4, 1/8, then the
# stride is traded for dilation 2 and 4, and two de-gridding conv runs (dilation 2, 1) close the network.
STAGES_D = (('conv', 16, 1, 1), ('conv', 32, 2, 1), ('res', 64, 2, 1), ('res', 128, 2, 1), ('res', 256, 1, 2), ('res', 512, 1, 4),
            ('conv', 512, 1, 2), ('conv', 512, 1, 1))
# depth -> (block, layers per stage)
DRN_D = {
    'drn_d_22': (BasicBlock, (1, 1, 2, 2, 2, 2, 1, 1)),
    'drn_d_105': (Bottleneck, (1, 1, 3, 4, 23, 3, 1, 1)),
}


def drn_d_stages(block, counts):
    """[stem, stage 1 ... stage 8] as modules, and the width of the last one."""
    stages, cin = [_conv_run(3, STAGES_D[0][1], 1, 7, 1, 1)], STAGES_D[0][1]
    for (kind, width, stride, dilation), count in zip(STAGES_D, counts):
        if kind == 'conv':
            stages.append(_conv_run(cin, width, count, 3, stride, dilation))
            cin = width
        else:
            blocks = []
            for i in range(count):
                blocks.append(block(cin, width, stride if i == 0 else 1, dilation))
                cin = width * block.expansion
            stages.append(nn.Sequential(*blocks))
    return stages, cin


def bilinear_up_weights(classes, k=16):
    """fill_up_weights (metric/mIoU_score.py:115-124): the same separable bilinear plane in every channel."""
    f = math.ceil(k / 2)
    c = (2 * f - 1 - f % 2) / (2.0 * f)
    v = torch.tensor([1 - math.fabs(i / f - c) for i in range(k)], dtype=torch.float64)
    return (v[:, None] * v[None, :]).float().expand(classes, 1, k, k).clone()


class DRNSeg(nn.Module):
    """metric/mIoU_score.py:127-168 with the reference's constructor surface (`pretrained*` / `use_torch_up` only in their evaluation
    settings: weights come from `load_state_dict`).  forward(x) -> (log-softmax map [N, classes, H, W], seg logits [N, classes, H/8, W/8])."""

    UP_STRIDE = 8

    def __init__(self, model_name, classes, pretrained_model=None, pretrained=False, use_torch_up=False):
        super().__init__()
        if model_name not in DRN_D:
            raise NotImplementedError('DRNSeg: %r is not built (architecture D only: %s)' % (model_name, ', '.join(sorted(DRN_D))))
        if pretrained or pretrained_model is not None or use_torch_up:
            raise NotImplementedError('DRNSeg is built as the distillers build it: pretrained=False, weights through load_state_dict')
        block, counts = DRN_D[model_name]
        stages, width = drn_d_stages(block, counts)
        self.base = nn.Sequential(*stages)
        self.seg = nn.Conv2d(width, classes, kernel_size=1, bias=True)
        self.softmax = nn.LogSoftmax(dim=1)
        for m in self.base.modules():      # the reference's initialisation (metric/drn.py:212-218, mIoU_score.py:145-148)
            if isinstance(m, nn.Conv2d):
                m.weight.data.normal_(0, math.sqrt(2.0 / (m.kernel_size[0] * m.kernel_size[1] * m.out_channels)))
        self.seg.weight.data.normal_(0, math.sqrt(2.0 / classes))
        self.seg.bias.data.zero_()
        self.up = nn.ConvTranspose2d(classes, classes, 2 * self.UP_STRIDE, stride=self.UP_STRIDE, padding=self.UP_STRIDE // 2, output_padding=0,
                                     groups=classes, bias=False)
        self.up.weight.data.copy_(bilinear_up_weights(classes, 2 * self.UP_STRIDE))
        self.classes = classes
        for p in self.parameters():
            p.requires_grad = False

    def optim_parameters(self, memo=None):
        raise NotImplementedError('This code is just for evaluation!!!')

    def features(self, x):
        """`base` + `seg`: the class logits at 1/8 resolution, [N, classes, H/8, W/8] (NHWC activation)."""
        if self.training or torch.is_grad_enabled():
            raise NotImplementedError('DRNSeg runs in eval mode under no_grad (metric/mIoU_score.py:225,234)')
        x = ops.to_nhwc(x.float())
        for stage in self.base:
            x = stage(x)
        return conv_bn_act(x, self.seg, None, L.ACT_NONE)

    def head(self, logits):
        """`up` + LogSoftmax in one launch: [N, classes, 8 h, 8 w] log-probabilities."""
        n, c, h, w = logits.shape
        s = self.UP_STRIDE
        y = ops.empty_act(n, c, h * s, w * s, logits.device)
        up_w = self.up.weight if self.up.weight.is_contiguous() else self.up.weight.contiguous()
        L.call('cat_seg_up_logsoftmax', ops._p(logits), ops.act_cs(logits), n, h, w, c, ops._p(up_w), s, ops._p(y), ops.act_cs(y), ops._stream())
        return y

    def forward(self, x):
        """x: [N, 3, H, W] normalised image batch on the GPU (NCHW as the reference passes it, or an NHWC activation); H, W multiples of 8."""
        logits = self.features(x)
        return self.head(logits), logits
