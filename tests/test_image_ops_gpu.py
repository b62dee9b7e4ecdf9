"""GPU: the two image kernels of csrc/image_ops.hip and cat_amd.metric.DeviceImages, bit for bit against the host formulas they replace.

A: cat_image_quantize against metric.tensor2im_batch (util.tensor2im: clip((x + 1) / 2 * 255, 0, 255), truncating cast), np.array_equal.
   The inputs hold the boundary set -- for k = 0..256 the float32 of k / 255 * 2 - 1 and its three float32 neighbours on each side, 1799
   values -- on which a fused x * 127.5 + 127.5 differs from numpy in 216 values and a rounding cast in 756 (restated on the CPU below, so the
   set is known to tell them apart), uniform values in [-1.2, 1.2] and +-inf.  NaN -> 0 is checked directly: numpy's cast of NaN is undefined.
B: cat_image_normalize over all 256 byte values x 3 channels against FID's `u.astype(float) / 255` -> float32, KID's float32 `u / 255` and
   miou.normalize_images, torch.equal; padding channel 0, channels beyond the quad untouched.
C: DeviceImages across a capacity growth, and what it refuses."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 5, 7), (3, 16, 17)]


@pytest.fixture(scope='module')
def dev():
    from cat_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _boundary_set():
    vals = []
    for k in range(257):
        x = np.float32(k / 255 * 2 - 1)
        lo = [x]
        hi = [x]
        for _ in range(3):
            lo.append(np.nextafter(lo[-1], np.float32(-np.inf)))
            hi.append(np.nextafter(hi[-1], np.float32(np.inf)))
        vals += lo[:0:-1] + [x] + hi[1:]
    return np.array(vals, dtype=np.float32)


_POOL = {}


def _pool():
    """boundary set, +-inf, uniform [-1.2, 1.2]: built once"""
    if 'v' not in _POOL:
        rs = np.random.RandomState(77)
        _POOL['v'] = np.concatenate([_boundary_set(), np.array([np.inf, -np.inf], dtype=np.float32), rs.uniform(-1.2, 1.2, 4096).astype(np.float32)])
    return _POOL['v']


def _values(n, c, h, w, start=0):
    """[N, C, H, W] float32 filled from the pool from `start` on (wrapping), so small shapes see different stretches of it"""
    return torch.from_numpy(np.resize(np.roll(_pool(), -start), n * c * h * w).reshape(n, c, h, w).copy())


def _quantize(x, xcs, dev, out=None, offset=0):
    """cat_image_quantize on the NCHW host tensor x laid out as an NHWC activation of pixel stride xcs (NaN in every other channel)"""
    from cat_amd import _lib as L, ops
    n, c, h, w = x.shape
    wide = ops.empty_act(n, xcs, h, w, dev, cs=xcs)
    wide.fill_(float('nan'))
    act = wide[:, :c]
    act.copy_(x.to(dev))
    if out is None:
        out = torch.full((n, h, w, 4), 0xAB, dtype=torch.uint8, device=dev)
    L.call('cat_image_quantize', ops._p(act), xcs, n, h, w, c, ops._p(out), offset, ops._stream())
    torch.cuda.synchronize()
    return out


def test_the_boundary_set_tells_the_wrong_kernels_apart():
    """the CPU restatement of the two mistakes the kernel must not make, on the 1799 values"""
    from cat_amd import metric
    b = _boundary_set()
    assert b.size == 1799
    want = metric.tensor2im_batch(torch.from_numpy(b).reshape(1, 1, 1, -1)).reshape(-1)
    fused = np.clip(b.astype(np.float64) * 127.5 + 127.5, 0, 255).astype(np.float32)      # one rounding, as a fused multiply-add has
    assert int((fused.astype(np.uint8) != want).sum()) == 216
    sep = np.clip((b + np.float32(1)) / np.float32(2) * np.float32(255), 0, 255)
    assert int((np.rint(sep).astype(np.uint8) != want).sum()) == 756


@pytest.mark.parametrize('c', [3, 1])
@pytest.mark.parametrize('xcs', [4, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d_h%d_w%d' % s)
def test_quantize_equals_tensor2im(dev, shape, xcs, c):
    from cat_amd import metric
    n, h, w = shape
    for start in ((0, 900, 1700) if n * h * w * c < 1801 else (0,)):
        x = _values(n, c, h, w, start)
        out = _quantize(x, xcs, dev).cpu().numpy()
        assert np.array_equal(out[..., :c], metric.tensor2im_batch(x)), (shape, xcs, c, start)
        assert not out[..., c:].any()                       # bytes [C, 4) are 0


def test_quantize_covers_the_whole_boundary_set(dev):
    """one launch over all 1799 boundary values and both infinities, 3 channels"""
    from cat_amd import metric
    x = _values(1, 3, 25, 25)
    assert x.numel() >= 1801
    out = _quantize(x, 4, dev).cpu().numpy()
    want = metric.tensor2im_batch(x)
    assert np.array_equal(out[..., :3], want)
    flat = x.permute(0, 2, 3, 1).reshape(-1).numpy()
    got = out[..., :3].reshape(-1)
    assert (got[flat == np.inf] == 255).all() and (got[flat == -np.inf] == 0).all() and int((flat == np.inf).sum()) == 1


def test_quantize_nan_is_zero(dev):
    x = _values(2, 3, 5, 7)
    x[0, 1, 2, 3] = float('nan')
    x[1, :, 4, 6] = float('nan')
    out = _quantize(x, 4, dev).cpu().numpy()
    assert out[0, 2, 3, 1] == 0 and not out[1, 4, 6].any()
    from cat_amd import metric
    ok = ~torch.isnan(x).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(out[..., :3][ok], metric.tensor2im_batch(torch.nan_to_num(x))[ok])


def test_quantize_at_an_image_offset_leaves_the_neighbours(dev):
    from cat_amd import metric
    x = _values(2, 3, 5, 7, 300)
    out = torch.full((5, 5, 7, 4), 0xAB, dtype=torch.uint8, device=dev)
    _quantize(x, 4, dev, out, 2)
    got = out.cpu().numpy()
    assert np.array_equal(got[2:4, ..., :3], metric.tensor2im_batch(x)) and not got[2:4, ..., 3].any()
    assert (got[:2] == 0xAB).all() and (got[4:] == 0xAB).all()


def test_quantize_refuses_bad_arguments(dev):
    from cat_amd import _lib as L, ops
    x = torch.zeros(64, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    for xcs, c, off in ((6, 3, 0), (4, 5, 0), (4, 0, 0), (4, 3, -1)):
        with pytest.raises(RuntimeError, match='image quantize'):
            L.call('cat_image_quantize', ops._p(x), xcs, 1, 2, 2, c, ops._p(out), off, ops._stream())
    with pytest.raises(RuntimeError, match='aligned'):
        L.call('cat_image_quantize', ops._p(x[1:]), 4, 1, 2, 2, 3, ops._p(out), 0, ops._stream())


# ---------------------------------------------------------------------------------------------------------------- B: normalise
def _bytes(n, h, w, base):
    """uint8 [N, H, W, 4]: pixel p holds (base + p, base + p + 85, base + p + 170) mod 256 and a fourth byte the kernel must ignore"""
    p = np.arange(n * h * w).reshape(n, h, w, 1)
    return ((base + p + np.array([0, 85, 170, 41])) % 256).astype(np.uint8)


def _normalize(u4, ycs, mean, std, dev):
    from cat_amd import _lib as L, ops
    n, h, w, _ = u4.shape
    wide = ops.empty_act(n, ycs, h, w, dev, cs=ycs)
    wide.fill_(float('nan'))
    ud = torch.from_numpy(u4).to(dev)
    L.call('cat_image_normalize', ops._p(ud), 0, n, h, w, 3, *(list(mean) + [0.0] + list(std) + [1.0]), ops._p(wide), ycs, ops._stream())
    torch.cuda.synchronize()
    return wide.cpu()


@pytest.mark.parametrize('ycs', [4, 8])
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 5, 7)], ids=lambda s: 'n%d_h%d_w%d' % s)
def test_normalize_equals_the_host_formulas_on_every_byte(dev, shape, ycs):
    from cat_amd.metric import miou
    n, h, w = shape
    npix = n * h * w
    seen = np.zeros((3, 256), dtype=bool)
    for base in range(0, 256, npix):
        u4 = _bytes(n, h, w, base)
        u = np.ascontiguousarray(u4[..., :3])
        for c in range(3):
            seen[c, u[..., c].reshape(-1)] = True
        fid = torch.from_numpy((u.astype(float) / 255).transpose((0, 3, 1, 2))).float()
        kid = torch.from_numpy((u.astype(np.float32) / 255.).transpose((0, 3, 1, 2)))
        got = _normalize(u4, ycs, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), dev)
        assert torch.equal(got[:, :3], fid) and torch.equal(got[:, :3], kid), (shape, ycs, base)
        assert bool((got[:, 3] == 0).all()) and bool(torch.isnan(got[:, 4:]).all())          # padding channel 0, nothing beyond the quad
        got = _normalize(u4, ycs, miou.MEAN, miou.STD, dev)
        assert torch.equal(got[:, :3], miou.normalize_images(u)), (shape, ycs, base)
        assert bool((got[:, 3] == 0).all()) and bool(torch.isnan(got[:, 4:]).all())
    assert seen.all()                                      # all 256 values in each of the 3 channels


def test_normalize_reads_at_an_image_offset(dev):
    from cat_amd import _lib as L, ops
    from cat_amd.metric import miou
    u4 = _bytes(4, 5, 7, 9)
    ud = torch.from_numpy(u4).to(dev)
    y = ops.empty_act(2, 3, 5, 7, dev)
    L.call('cat_image_normalize', ops._p(ud), 1, 2, 5, 7, 3, *(miou.MEAN + [0.0] + miou.STD + [1.0]), ops._p(y), 4, ops._stream())
    assert torch.equal(y.cpu(), miou.normalize_images(np.ascontiguousarray(u4[1:3, ..., :3])))
    with pytest.raises(RuntimeError, match='image normalize'):
        L.call('cat_image_normalize', ops._p(ud), 0, 2, 5, 7, 3, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, ops._p(y), 6, ops._stream())


# ---------------------------------------------------------------------------------------------------------------- C: DeviceImages
def test_device_images_across_a_capacity_growth(dev):
    from cat_amd import metric, ops
    from cat_amd.metric import DeviceImages, miou
    batches = [_values(b, 3, 5, 7, 500 * i) for i, b in enumerate((2, 1, 3))]
    s = DeviceImages(capacity=2)
    assert len(s) == 0
    for i, b in enumerate(batches):
        s.append(ops.to_nhwc(b.to(dev)) if i != 1 else b.to(dev))          # an NHWC activation, or the NCHW tensor of the same values
    assert len(s) == 6 and s.buf.shape[0] >= 6 and s.buf.dtype == torch.uint8 and s.buf.is_cuda
    want = metric.tensor2im_batch(torch.cat(batches, 0))
    got = s.numpy()
    assert got.dtype == np.uint8 and got.shape == (6, 5, 7, 3) and np.array_equal(got, want)
    assert np.array_equal(s.numpy(2, 5), want[2:5])
    assert not bool(s.buf[:6, ..., 3].any())
    y = s.batch(1, 4)
    assert ops.is_act(y) and torch.equal(y.cpu(), torch.from_numpy((want[1:4].astype(np.float32) / 255.).transpose((0, 3, 1, 2))))
    assert torch.equal(s.batch(4, 9, miou.MEAN, miou.STD).cpu(), miou.normalize_images(want[4:6]))          # the end is clipped, as a slice is


def test_device_images_refuses_other_sizes_and_channels(dev):
    from cat_amd.metric import DeviceImages
    s = DeviceImages()
    s.append(torch.zeros(2, 3, 5, 7, device=dev))
    with pytest.raises(ValueError, match='5 x 7'):
        s.append(torch.zeros(1, 3, 5, 8, device=dev))
    with pytest.raises(ValueError, match='5 x 7'):
        s.append(torch.zeros(1, 3, 6, 7, device=dev))
    with pytest.raises(ValueError, match='3 channels'):
        s.append(torch.zeros(1, 1, 5, 7, device=dev))
    with pytest.raises(ValueError, match='3 channels'):
        DeviceImages().append(torch.zeros(1, 4, 5, 7, device=dev))
    assert len(s) == 2
