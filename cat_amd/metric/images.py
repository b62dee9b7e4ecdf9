"""DeviceImages: the generated image set of an evaluation as uint8 on the device (csrc/image_ops.hip).

The reference collects `fake.cpu()` per batch, quantises the concatenation with util.tensor2im on the host, widens it to float64 (FID) or float32
(mIoU) and uploads it again batch by batch.  Here cat_image_quantize turns every generated NHWC batch into bytes where it lies -- the same
bytes: clip((x + 1) / 2 * 255, 0, 255), truncated, every float32 operation rounded on its own -- and cat_image_normalize hands the metric
networks one batch at a time as the NHWC activation they take (`u8 / 255` for FID and KID, SegList's mean / std for the mIoU).  No float copy
of the set exists on either side, nothing syncs per batch, and only uint8 ever crosses to the host (the PNG dumps, `numpy`)."""
import numpy as np
import torch

from .. import _lib as L
from .. import ops


def quantize(act, out=None, offset=0):
    """NHWC float32 activation [N, C, H, W], C in 1..4 -> uint8 device tensor [N, H, W, 4] (bytes [C, 4) are 0).  out / offset: write the N
    images from image `offset` of a larger [M, H, W, 4] set on."""
    ops._require_cuda(act)
    if not ops.is_act(act):
        raise ValueError('quantize: an NHWC float32 activation is required (got shape %s, strides %s)' % (tuple(act.shape), act.stride()))
    n, c, h, w = act.shape
    if not 1 <= c <= 4:
        raise ValueError('quantize: 1 to 4 channels (got %d)' % c)
    if out is None:
        out, offset = torch.empty((n, h, w, 4), dtype=torch.uint8, device=act.device), 0
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.dim() != 4 or tuple(out.shape[1:]) != (h, w, 4) or offset < 0 or \
            offset + n > out.shape[0] or out.device != act.device:
        raise ValueError('quantize: out must be a contiguous uint8 [M, %d, %d, 4] tensor on %s with M >= %d' % (h, w, act.device, offset + n))
    with torch.cuda.device(act.device):
        L.call('cat_image_quantize', ops._p(act), ops.act_cs(act), n, h, w, c, ops._p(out), offset, ops._stream())
    return out


def tensor2im(t):
    """evaluation.tensor2im of a device tensor ([C, H, W] or [1, C, H, W], C = 1 or 3) through the kernel: HWC (or HW) uint8 numpy array."""
    t = t.detach()
    t = t[None] if t.dim() == 3 else t
    a = quantize(ops.to_nhwc(t.float()))[0].cpu().numpy()
    return a[:, :, 0] if t.shape[1] == 1 else a[:, :, :t.shape[1]]


class DeviceImages:
    """The generated set: uint8 [capacity, H, W, 4] on the device, `len(self)` images of it filled."""

    def __init__(self, device=None, capacity=64):
        self.device = torch.device(device) if device is not None else None
        self.buf, self.n, self.hw = None, 0, None
        self._capacity = max(1, int(capacity))

    def __len__(self):
        return self.n

    def _reserve(self, n, h, w, device):
        if self.buf is None:
            self.device, self.hw = self.device or device, (h, w)
            self.buf = torch.empty((max(self._capacity, n), h, w, 4), dtype=torch.uint8, device=self.device)
        elif self.n + n > self.buf.shape[0]:
            grown = torch.empty((max(2 * self.buf.shape[0], self.n + n), h, w, 4), dtype=torch.uint8, device=self.device)
            grown[:self.n].copy_(self.buf[:self.n])      # device to device, on the current stream
            self.buf = grown

    def append(self, act):
        """Quantise one generated batch ([B, 3, H, W] in [-1, 1] on the device; an NCHW tensor is laid out as NHWC first) into the set."""
        if not isinstance(act, torch.Tensor) or act.dim() != 4:
            raise ValueError('DeviceImages.append: a [B, 3, H, W] tensor is required')
        n, c, h, w = act.shape
        if c != 3:
            raise ValueError('DeviceImages.append: images have 3 channels (got %d)' % c)
        if self.hw is not None and (h, w) != self.hw:
            raise ValueError('DeviceImages.append: every batch must be %d x %d (got %d x %d)' % (self.hw + (h, w)))
        act = ops.to_nhwc(act.detach().float())
        if self.device is not None and act.device != self.device:
            raise ValueError('DeviceImages.append: the set lives on %s (got a batch on %s)' % (self.device, act.device))
        if n == 0:
            return
        self._reserve(n, h, w, act.device)
        quantize(act, self.buf, self.n)
        self.n += n

    def _range(self, start, end):
        start = 0 if start is None else start
        end = self.n if end is None else min(end, self.n)
        if not 0 <= start < end:
            raise ValueError('DeviceImages: images [%s, %s) of %d' % (start, end, self.n))
        return start, end

    def numpy(self, start=None, end=None):
        """uint8 [n, H, W, 3] on the host: metric.tensor2im_batch of the same floats."""
        start, end = self._range(start, end)
        return np.ascontiguousarray(self.buf[start:end].cpu().numpy()[..., :3])

    def batch(self, start, end, mean=None, std=None):
        """Images [start, end) as the NHWC float32 activation [n, 3, H, W] a metric network takes: ((u8 / 255) - mean) / std per channel;
        mean / std None = 0 / 1 (FID's and KID's `u8 / 255`)."""
        start, end = self._range(start, end)
        mean = [0.0, 0.0, 0.0] if mean is None else [float(m) for m in mean]
        std = [1.0, 1.0, 1.0] if std is None else [float(s) for s in std]
        if len(mean) != 3 or len(std) != 3:
            raise ValueError('DeviceImages.batch: mean and std have 3 entries')
        h, w = self.hw
        y = ops.empty_act(end - start, 3, h, w, self.device)
        with torch.cuda.device(self.device):
            L.call('cat_image_normalize', ops._p(self.buf), start, end - start, h, w, 3, *(mean + [0.0] + std + [1.0]), ops._p(y), ops.act_cs(y),
                   ops._stream())
        return y
