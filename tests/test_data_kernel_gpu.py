"""cat_data_batch (csrc/data_ops.hip) against PIL and torch on the CPU: Image.crop, transpose(FLIP_LEFT_RIGHT) and
torch.from_numpy(...).permute(2, 0, 1).float().div(255).sub(0.5).div(0.5).  Every comparison is bit-exact: bytes, integers and float32 operations
that are rounded one by one leave no tolerance to choose."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

import data_host_ref as R

pytestmark = pytest.mark.gpu


def _nan_act(n, c, h, w, cs):
    buf = torch.full((n, h, w, cs), float('nan'), device='cuda')
    return buf, buf[..., :c].permute(0, 3, 1, 2)


def _run(planes, codes, n, unknown=0.0):
    """planes: [(src tensor, kind, C, dst tensor, cs, slot, Hc, Wc)]; codes: rows [idx0, idx1, (x, y, flip) per plane]"""
    from cat_amd import _lib as L
    from cat_amd import ops
    t = L.DataBatch()
    t.planes, t.N, t.unknown = len(planes), n, unknown
    for i, (src, kind, c, dst, cs, slot, hc, wc) in enumerate(planes):
        d = t.plane[i]
        d.src, d.dst = src.data_ptr(), dst.data_ptr()
        d.M, d.H, d.W = src.shape[:3]
        d.Hc, d.Wc, d.kind, d.C, d.cs, d.slot = hc, wc, kind, c, cs, slot
    dev_codes = torch.tensor(codes, dtype=torch.int32).cuda()
    assert tuple(dev_codes.shape) == (n, 2 + 3 * len(planes))
    L.call('cat_data_batch', C.byref(t), ops._p(dev_codes), ops._stream())
    torch.cuda.synchronize()


def _want_image(src, idx, x, y, flip, hc, wc, c):
    """src: uint8 numpy [M, H, W, 4] -> the [c, hc, wc] tensor the reference's chain gives"""
    img = Image.fromarray(src[idx, :, :, :3]) if c == 3 else Image.fromarray(src[idx, :, :, 0])
    img = img.crop((x, y, x + wc, y + hc))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return R.normalize(R.to_tensor(img))


@pytest.mark.parametrize('c, cs', [(3, 4), (1, 4), (3, 8)])
def test_all_256_byte_values(c, cs):
    """One 16 x 16 source holding every byte in every channel; the output is NaN first, so lanes [C, cs) are shown to be WRITTEN as 0."""
    from cat_amd import _lib as L
    from cat_amd import ops
    ramp = np.arange(256, dtype=np.uint8)
    src = np.zeros((1, 16, 16, 4), dtype=np.uint8)
    src[0, :, :, 0], src[0, :, :, 1], src[0, :, :, 2] = ramp.reshape(16, 16), ramp[::-1].reshape(16, 16), np.roll(ramp, 77).reshape(16, 16)
    buf, out = _nan_act(1, c, 16, 16, cs)
    assert ops.is_act(out) and ops.act_cs(out) == cs
    _run([(torch.from_numpy(src).cuda(), L.DATA_IMAGE, c, out, cs, 0, 16, 16)], [[0, 0, 0, 0, 0]], 1)
    want = _want_image(src, 0, 0, 0, False, 16, 16, c)
    assert all(set(src[0, :, :, k].ravel().tolist()) == set(range(256)) for k in range(3))
    assert torch.equal(out[0].cpu(), want)
    assert torch.equal(buf[..., c:].cpu(), torch.zeros(1, 16, 16, cs - c))
    assert float(out.min()) == -1.0 and float(out.max()) == 1.0


def test_crop_and_flip_at_the_edges():
    """10 x 13 sources (the width is no multiple of 4), M = 3, crop 6 x 7, N = 4: offsets (0, 0) and (max, max), an interior one, one sample
    index used twice, flip on and off."""
    from cat_amd import _lib as L
    src = np.random.RandomState(3).randint(0, 256, size=(3, 10, 13, 4), dtype=np.uint8)
    src[..., 3] = 0
    cases = [(0, 0, 0, 0), (2, 6, 4, 1), (1, 3, 2, 1), (2, 1, 1, 0)]      # (idx, x, y, flip); x <= 13 - 7, y <= 10 - 6
    buf, out = _nan_act(4, 3, 6, 7, 4)
    _run([(torch.from_numpy(src).cuda(), L.DATA_IMAGE, 3, out, 4, 0, 6, 7)], [[i, 0, x, y, f] for i, x, y, f in cases], 4)
    for n, (i, x, y, f) in enumerate(cases):
        assert torch.equal(out[n].cpu(), _want_image(src, i, x, y, f, 6, 7, 3)), (n, i, x, y, f)
    assert not buf[..., 3].any()
    # the same pixels through the other index slot
    buf2, out2 = _nan_act(4, 3, 6, 7, 4)
    _run([(torch.from_numpy(src).cuda(), L.DATA_IMAGE, 3, out2, 4, 1, 6, 7)], [[0, i, x, y, f] for i, x, y, f in cases], 4)
    assert torch.equal(buf2, buf)


def test_label_and_instance_planes_share_a_launch_and_its_codes():
    from cat_amd import _lib as L
    rs = np.random.RandomState(4)
    m, h, w, hc, wc = 2, 9, 11, 5, 6
    img = rs.randint(0, 256, size=(m, h, w, 4), dtype=np.uint8)
    img[..., 3] = 0
    lab = rs.randint(0, 36, size=(m, h, w)).astype(np.uint8)
    lab[0, 0, :4], lab[1, 4, 5:9] = [0, 34, 255, 255], [255, 0, 34, 255]
    ins = rs.randint(0, 40000, size=(m, h, w)).astype(np.int32)
    ins[0, 1, :3], ins[1, 4, 5:8] = [0, 33001, 26001], [33001, 0, 24000]
    cases = [(0, 0, 0, 1), (1, 5, 4, 0), (1, 2, 3, 1)]      # x <= 5, y <= 4
    n = len(cases)
    ibuf, iout = _nan_act(n, 3, hc, wc, 4)
    lout = torch.full((n, 1, hc, wc), float('nan'), device='cuda')
    nout = torch.full((n, 1, hc, wc), -7, dtype=torch.int32, device='cuda')
    with R.Launches() as log:
        _run([(torch.from_numpy(lab).cuda(), L.DATA_LABEL, 1, lout, 0, 0, hc, wc), (torch.from_numpy(img).cuda(), L.DATA_IMAGE, 3, iout, 4, 0, hc, wc),
              (torch.from_numpy(ins).cuda(), L.DATA_INT32, 1, nout, 0, 0, hc, wc)], [[i, i] + [x, y, f] * 3 for i, x, y, f in cases], n, unknown=35.0)
    assert log.names == ['cat_data_batch']
    seen = set()
    for k, (i, x, y, f) in enumerate(cases):
        assert torch.equal(iout[k].cpu(), _want_image(img, i, x, y, f, hc, wc, 3))
        pl = Image.fromarray(lab[i]).crop((x, y, x + wc, y + hc))
        pn = Image.fromarray(ins[i]).crop((x, y, x + wc, y + hc))
        if f:
            pl, pn = pl.transpose(Image.FLIP_LEFT_RIGHT), pn.transpose(Image.FLIP_LEFT_RIGHT)
        want = R.to_tensor(pl) * 255.0      # cityscapes_dataset.py:91-93
        seen |= set(want.ravel().tolist())
        want[want == 255] = 35
        assert torch.equal(lout[k].cpu(), want)
        wn = torch.from_numpy(np.array(pn))[None]
        assert wn.dtype == torch.int32 and torch.equal(nout[k].cpu(), wn)
    assert {0.0, 34.0, 255.0} <= seen
    assert {0, 33001} <= set(nout.cpu().ravel().tolist())


def _single_loader(batch_size):
    from cat_amd import data
    imgs = [R.rgb(13, 10, 60 + i) for i in range(3)]
    opt = R.data_opt(preprocess='crop', crop_size=7, batch_size=batch_size, serial_batches=True)
    return data.DeviceLoader.single(opt, imgs), imgs


def _want_single(imgs, rows):
    out = []
    for i, _, x, y, f in rows:
        img = imgs[i].crop((x, y, x + 7, y + 7))
        out.append(R.normalize(R.to_tensor(img.transpose(Image.FLIP_LEFT_RIGHT) if f else img)))
    return torch.stack(out)


def test_fill_under_capture_replays_with_the_uploaded_codes():
    """One torch.cuda.graph around a fill into fixed buffers (a single stream, no branches); the codes buffer is rewritten between the
    replays and each replay equals its own host expectation."""
    from cat_amd import ops
    loader, imgs = _single_loader(2)
    c0, c1, c2 = [[0, 0, 0, 0, 0], [1, 0, 6, 3, 1]], [[2, 0, 3, 1, 1], [2, 0, 0, 3, 0]], [[1, 0, 6, 0, 0], [0, 0, 2, 2, 1]]
    first = loader.fill(c0)
    assert ops.is_act(first['A']) and torch.equal(first['A'].cpu(), _want_single(imgs, c0))
    bufs = {'A': ops.empty_act(2, 3, 7, 7, 'cuda')}
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = loader.fill(c0, out=bufs)
    assert got['A'] is bufs['A']
    with pytest.MonkeyPatch.context() as mp:      # an upload is host work: inside a capture it is refused, not recorded
        mp.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        with pytest.raises(RuntimeError, match='before a replay'):
            loader.upload(c0)
    for codes in (c1, c2, c0):
        loader.upload(codes)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bufs['A'].cpu(), _want_single(imgs, codes)), codes


def test_one_launch_per_batch_and_nothing_else():
    loader, imgs = _single_loader(2)
    R.seed_all(5)
    with R.Launches() as log:
        batches = list(loader)
    assert log.names == ['cat_data_batch'] * 2 and [b['A'].shape[0] for b in batches] == [2, 1]
    assert [b['A_paths'] for b in batches] == [['<memory:0>', '<memory:1>'], ['<memory:2>']]


def test_entry_point_rejects_bad_tables():
    from cat_amd import _lib as L
    src = torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device='cuda')
    _, out = _nan_act(1, 3, 8, 8, 4)
    for planes, match in (([(src, L.DATA_IMAGE, 3, out, 6, 0, 8, 8)], 'channel stride'), ([(src, L.DATA_IMAGE, 2, out, 4, 0, 8, 8)], 'C 2'),
                          ([(src, L.DATA_IMAGE, 3, out, 4, 2, 8, 8)], 'slot'), ([(src, L.DATA_IMAGE, 3, out, 4, 0, 9, 8)], 'crop 9 x 8'),
                          ([(src, 7, 3, out, 4, 0, 8, 8)], 'kind 7'), ([], 'planes')):
        with pytest.raises(RuntimeError, match=match):
            _run(planes, [[0, 0] + [0, 0, 0] * len(planes)], 1)
