"""ImagePool (reference utils/image_pool.py:5-53): history buffer of generated images for the CycleGAN discriminators.  Same
algorithm and the same sequence of `random` draws as the reference (so a seeded run replays identically); images stay NHWC
activations on the device.

The draws stay on the host (`decide`), what they decide is applied on the device: the history is ONE buffer [pool_size][h][w][cs] and a
query is one cat_image_pool_query launch that reads the decisions of this batch as int32 codes from a persistent device tensor:

    -1      pass:  out[i] = images[i]
    s >= 0  swap:  out[i] = pool[s], then pool[s] = images[i]
    -2 - s  store: pool[s] = images[i], out[i] = images[i]      (the pool is still filling)

That launch can be captured (cat_amd.graph.GraphedStep): the capture records it without drawing, and before each replay `stage(n)` draws
for that step and uploads its codes.  A query of another image geometry (legal at batch 1, e.g. --preprocess scale_width) turns the pool
into a Python list of separately allocated images for good; that form cannot be captured."""
import ctypes as C
import random

import torch

from .. import _lib as L
from .. import ops

PASS = -1


def _copy(src):
    src = ops.conform(src)
    n, c, h, w = src.shape
    dst = ops.empty_act(n, c, h, w, src.device, ops.act_cs(src))
    arr = (C.c_void_p * 1)(src.data_ptr())
    L.call('cat_add_n', arr, 1, ops._p(dst), n * h * w * ops.act_cs(src), ops._stream())
    return dst


class ImagePool:
    def __init__(self, pool_size, rng=None):
        self.pool_size = pool_size
        self.rng = random if rng is None else rng
        if self.pool_size > 0:
            self.num_imgs = 0
            self.buffer = None      # [pool_size][h][w][cs], allocated by the first query
            self.geometry = None    # (c, h, w, cs) of the buffer
            self.codes = None       # int32 [n] on the device: the decisions of the current batch, read by the (captured) launch
            self.images = None      # the list form, after a query of another geometry

    def decide(self, n):
        """The reference loop's decisions for the next n images, as codes; advances num_imgs and draws exactly as that loop does."""
        codes = []
        for _ in range(n):
            if self.num_imgs < self.pool_size:
                codes.append(-2 - self.num_imgs)
                self.num_imgs += 1
            elif self.rng.uniform(0, 1) > 0.5:
                codes.append(self.rng.randint(0, self.pool_size - 1))
            else:
                codes.append(PASS)
        assert all(0 <= (c if c >= 0 else -2 - c) < self.pool_size for c in codes if c != PASS), codes
        return codes

    def _upload(self, codes, dst):
        # stream-ordered copy out of a fresh pageable tensor: the runtime stages it before returning, nothing is left to overwrite
        dst.copy_(torch.tensor(codes, dtype=torch.int32))

    def stage(self, n):
        """Before a graph replay of a step that queries this pool with n images: that step's draws, and its codes to the device."""
        if self.pool_size == 0:
            return
        if self.images is not None or self.codes is None or self.codes.numel() != n:
            raise RuntimeError('ImagePool.stage: no captured query of %d images to feed (the pool %s)' % (
                n, 'is in list form' if self.images is not None else 'was never queried with that batch size'))
        self._upload(self.decide(n), self.codes)

    def query(self, images):
        if self.pool_size == 0:
            return images
        images = ops.conform(images.detach())
        n, c, h, w = images.shape
        cs = ops.act_cs(images)
        capturing = torch.cuda.is_current_stream_capturing()
        if self.images is None and self.buffer is None:
            if capturing:
                raise RuntimeError('ImagePool: the first query cannot happen inside a graph capture (run a step eagerly first)')
            self.buffer = torch.empty((self.pool_size, h, w, cs), device=images.device, dtype=torch.float32)
            self.geometry = (c, h, w, cs)
            self.codes = torch.full((n,), PASS, device=images.device, dtype=torch.int32)
        if self.images is None and (c, h, w, cs) != self.geometry:
            self._to_list()
        if self.images is not None:
            if capturing:
                raise RuntimeError('ImagePool: images of more than one geometry were queried, the pool keeps them as a list; '
                                   'that form cannot be captured into a graph')
            return self._query_list(images, self.decide(n))
        if capturing:
            # a capture records and does not execute: no draw, no host state change, no upload -- stage() feeds every replay
            if self.codes.numel() != n:
                raise RuntimeError('ImagePool: a captured query has the batch size of the eager queries before it (%d, got %d)' % (self.codes.numel(), n))
            codes = self.codes
        else:
            codes = self.codes if self.codes.numel() == n else torch.empty((n,), device=images.device, dtype=torch.int32)
            self._upload(self.decide(n), codes)
        out = ops.empty_act(n, c, h, w, images.device, cs)
        L.call('cat_image_pool_query', ops._p(images), ops._p(self.buffer), ops._p(out), ops._p(codes), n, self.pool_size, h * w * cs, ops._stream())
        return out

    # -- the list form ------------------------------------------------------------------------------------------------------------------
    def _to_list(self):
        c, h, w, cs = self.geometry
        slot = lambda k: self.buffer[k:k + 1][..., :c].permute(0, 3, 1, 2)
        self.images = [_copy(slot(k)) for k in range(self.num_imgs)]
        self.buffer = self.codes = self.geometry = None

    def _query_list(self, images, codes):
        out = []
        for i, code in enumerate(codes):
            image = images[i:i + 1]
            if code == PASS:
                out.append(image)
            elif code >= 0:
                out.append(self.images[code])
                self.images[code] = _copy(image)
            else:
                self.images.append(_copy(image))        # slot -2 - code == len(self.images); the reference keeps a view of the batch
                out.append(image)
        if len(out) == 1:
            return out[0]
        n, c, h, w = images.shape
        cs = ops.act_cs(images)
        dst = ops.empty_act(n, c, h, w, images.device, cs)
        per = h * w * cs
        for i, t in enumerate(out):
            arr = (C.c_void_p * 1)(t.data_ptr())
            L.call('cat_add_n', arr, 1, C.c_void_p(dst.data_ptr() + 4 * i * per), per, ops._stream())
        return dst
