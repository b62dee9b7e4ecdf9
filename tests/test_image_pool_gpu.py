"""GPU: the graph-safe image pool.  (1) the kernel cat_image_pool_query, bit for bit against the interpreter of its code table
(tests/test_image_pool_host.py); (2) ImagePool.query against the reference's pool (oracle.ref_cpu.ImagePoolRef) with equal generators;
(3) a change of image geometry falls to the list form, which still equals the reference and refuses a capture; (4) the CycleGAN teacher step
replayed by cat_amd.graph.GraphedStep equals the eager step, swaps and passes included (the criterion of tests/test_graph_gpu.py)."""
import json
import random

import numpy as np
import pytest
import torch

import helpers as H
from oracle import detfill, ref_cpu
from test_image_pool_host import ORDER_BATCHES, ORDER_CODES, interpret, log_decisions

pytestmark = pytest.mark.gpu

POOL_CAP = 2048      # image_pool.hip kPoolCap: most workgroups of the element walk; 256 lanes each, one float4 (one 3-channel pixel) per lane and trip

# (pool_size, codes): hand-written, every row of the code table and every order within a batch that matters
CODE_LISTS = {
    'pass only': (2, [-1, -1, -1]),
    'store only': (3, [-2, -3]),                       # slot 2 is never written
    'swap distinct slots': (4, [2, 0, 3]),             # slot 1 is never written
    'same slot twice': (2, [1, 1, -1]),                # the second image receives the first
    'store then swap': (2, [-2, 0, -3, 1]),            # n = 4: both slots stored and swapped out again within the batch
    'n = 1 swap': (1, [0]),
    'n = 1 store': (2, [-3]),
    'n = 1 pass': (1, [-1]),
}
PLANES = {'5x7': (5, 7), '33x31': (33, 31)}           # 35 float4 items: part of one workgroup; 1023: four workgroups, the last one short
BIG = (725, 725)                                       # 525 625 items > POOL_CAP * 256 = 524 288: the first 1 337 lanes walk twice


def _run_kernel(pool_size, codes, h, w, seed):
    from cat_amd import _lib as L
    from cat_amd import ops
    n, per = len(codes), h * w * 4
    rng = np.random.default_rng(seed)
    images = rng.standard_normal((n, per), dtype=np.float32).view(np.int32)
    pool = (0x7fc00000 + (np.arange(pool_size * per, dtype=np.int64) % 0x10000)).astype(np.int32).reshape(pool_size, per)      # quiet NaNs, all different
    out = np.full((n, per), 0x7fa00001, np.int32)
    d_images, d_pool, d_out = (torch.from_numpy(a.copy()).cuda() for a in (images, pool, out))
    d_codes = torch.tensor(codes, dtype=torch.int32).cuda()
    L.call('cat_image_pool_query', ops._p(d_images), ops._p(d_pool), ops._p(d_out), ops._p(d_codes), n, pool_size, per, ops._stream())
    want_pool = pool.copy()
    want_out = interpret(codes, images, want_pool)
    assert np.array_equal(d_out.cpu().numpy(), want_out)
    assert np.array_equal(d_pool.cpu().numpy(), want_pool)
    assert np.array_equal(d_images.cpu().numpy(), images) and d_codes.cpu().tolist() == codes
    touched = {c if c >= 0 else -2 - c for c in codes if c != -1}
    for s in set(range(pool_size)) - touched:
        assert np.array_equal(want_pool[s], pool[s])      # (the interpreter's own sanity: an unnamed slot keeps its poison)


@pytest.mark.parametrize('plane', list(PLANES))
@pytest.mark.parametrize('case', list(CODE_LISTS))
def test_kernel_applies_the_code_table(case, plane):
    pool_size, codes = CODE_LISTS[case]
    _run_kernel(pool_size, codes, *PLANES[plane], seed=11)


def test_kernel_walks_a_plane_larger_than_its_grid():
    h, w = BIG
    assert POOL_CAP * 256 < h * w < 2 * POOL_CAP * 256
    _run_kernel(2, [-3, 1, 0], h, w, seed=12)


def test_kernel_rejects_bad_arguments():
    from cat_amd import _lib as L
    from cat_amd import ops
    lib = L.load()
    t = torch.zeros(16, device='cuda')
    c = torch.zeros(1, dtype=torch.int32, device='cuda')
    s = ops._stream()
    assert lib.cat_image_pool_query(None, None, None, None, 0, 1, 16, s) == 0            # n == 0: a no-op
    assert lib.cat_image_pool_query(ops._p(t), ops._p(t), ops._p(t), ops._p(c), -1, 1, 16, s) != 0
    assert lib.cat_image_pool_query(ops._p(t), ops._p(t), ops._p(t), ops._p(c), 1, 1, 6, s) != 0
    for k in range(4):
        args = [ops._p(t), ops._p(t), ops._p(t), ops._p(c)]
        args[k] = None
        assert lib.cat_image_pool_query(*args, 1, 1, 16, s) != 0
    torch.cuda.synchronize()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _query_both(mine, ref, x):
    from cat_amd import ops
    want = ref.query(x)
    got = mine.query(ops.to_nhwc(x.cuda()))
    assert tuple(got.shape) == tuple(want.shape)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('pool_size', [2, 3])
def test_query_equals_the_reference_pool(pool_size, batch):
    from cat_amd.models.image_pool import ImagePool
    r_mine, r_ref = random.Random(5), random.Random(5)
    mine, ref = ImagePool(pool_size, r_mine), ref_cpu.ImagePoolRef(pool_size, r_ref)
    log = log_decisions(mine)
    for q in range(12):
        _query_both(mine, ref, detfill.images((batch, 3, 8, 8), 800 + q))
        assert r_mine.getstate() == r_ref.getstate()
    assert mine.images is None and tuple(mine.buffer.shape) == (pool_size, 8, 8, 4)      # one buffer, never the list form
    flat = [c for codes in log for c in codes]
    assert len(log) == 12 and any(c >= 0 for c in flat) and -1 in flat
    # the history itself: slot by slot what the reference holds
    for k, img in enumerate(ref.images):
        assert torch.equal(_bits(mine.buffer[k, :, :, :3].permute(2, 0, 1)), _bits(img[0]))


def test_pool_size_zero_returns_its_input():
    from cat_amd import ops
    from cat_amd.models.image_pool import ImagePool
    x = ops.to_nhwc(detfill.images((2, 3, 8, 8), 820).cuda())
    assert ImagePool(0).query(x) is x
    ImagePool(0).stage(2)      # nothing to stage, nothing to draw


def _raises_under_capture(pool, x, match):
    from cat_amd.models import image_pool
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match=match):
        with torch.cuda.graph(graph):
            image_pool._copy(x)      # the capture holds one launch when the query refuses
            pool.query(x)


def test_geometry_change_falls_to_the_list_form():
    from cat_amd import ops
    from cat_amd.models.image_pool import ImagePool
    r_mine, r_ref = random.Random(5), random.Random(5)      # swaps at queries 2 - 5: two in buffer form, then an 8 x 8 image out for an 8 x 12 one and back
    mine, ref = ImagePool(2, r_mine), ref_cpu.ImagePoolRef(2, r_ref)
    log = log_decisions(mine)
    widths = [8, 8, 8, 8, 12, 8, 12, 12, 8, 12, 8, 12]      # full and swapping in buffer form before the first 8 x 12 image arrives
    for q, w in enumerate(widths):
        _query_both(mine, ref, detfill.images((1, 3, 8, w), 840 + q))
        assert r_mine.getstate() == r_ref.getstate()
        assert (mine.images is None) == (q < 4)
    assert any(c[0] >= 0 for c in log[2:4]) and any(c[0] >= 0 for c in log[4:])      # swaps before and after the change
    for a, b in zip(mine.images, ref.images):
        assert tuple(a.shape) == tuple(b.shape) and torch.equal(_bits(a), _bits(b))
    state = r_mine.getstate()
    _raises_under_capture(mine, ops.to_nhwc(detfill.images((1, 3, 8, 8), 860).cuda()), 'list')
    assert r_mine.getstate() == state and len(log) == 12
    # and the first query of a pool cannot be a captured one: the buffer must exist before the graph does
    _raises_under_capture(ImagePool(2, random.Random(1)), ops.to_nhwc(detfill.images((1, 3, 8, 8), 861).cuda()), 'first query')


def _cyclegan(pool_size):
    from cat_amd.models import create_model
    from test_train_models import _opt_for
    g = H.load('train_steps.npz')
    meta = json.loads(str(g['cyc_meta']))
    opt = _opt_for(meta, model='cycle_gan', dataset_mode='unaligned', lambda_A=meta['lambda_A'], lambda_B=meta['lambda_B'],
                   lambda_identity=meta['lambda_identity'], pool_size=pool_size)
    m = create_model(opt, verbose=False)
    gsh, dsh = H.sd_from_shapes(g['cyc_G_shapes']), H.sd_from_shapes(g['cyc_D_shapes'])
    m.netG_A.load_state_dict(detfill.fill_state_dict(gsh, 401))
    m.netG_B.load_state_dict(detfill.fill_state_dict(gsh, 402))
    m.netD_A.load_state_dict(detfill.fill_state_dict(dsh, 411))
    m.netD_B.load_state_dict(detfill.fill_state_dict(dsh, 412))
    m.setup(opt, verbose=False)
    rng = random.Random(1)
    m.fake_A_pool.rng = m.fake_B_pool.rng = rng      # one generator for both pools, as the module `random` is
    return m, log_decisions(m.fake_B_pool), log_decisions(m.fake_A_pool)


@pytest.mark.parametrize('pool_size', [2, 50])
def test_graph_replay_equals_eager_cyclegan(pool_size):
    """Steps 0-2 are GraphedStep's warm-up on the example batch, the capture draws nothing, steps 3, 4, 6, 7 are replays and step 5 (two
    images: another shape) is the graphed model's eager fallback.  pool_size 2: the replays swap and pass (ORDER_CODES); pool_size 50: every
    replay is still filling a pool whose graph was captured when it held three images."""
    from cat_amd.graph import GraphedStep
    from test_graph_gpu import _max_param_diff
    (eager, eb, ea), (graphed, gb, ga) = _cyclegan(pool_size), _cyclegan(pool_size)
    batches = [{'A': detfill.images((n, 3, 64, 64), 870 + i).cuda(), 'B': detfill.images((n, 3, 64, 64), 880 + i).cuda()}
               for i, n in enumerate(ORDER_BATCHES)]
    for i in range(3):
        eager.set_input(batches[0])
        eager.optimize_parameters(i)
    step = GraphedStep(graphed, batches[0], warmup=3)
    assert len(gb) == len(ga) == 3      # the capture itself drew nothing
    for i in range(3, len(batches)):
        eager.set_input(batches[i])
        eager.optimize_parameters(i)
        step(batches[i])
        le, lg = eager.get_current_losses(), graphed.get_current_losses()
        assert len(le) == 8
        for k in le:
            print('pool_size %d step %d %s: eager %.9g graphed %.9g' % (pool_size, i, k, le[k], lg[k]))
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-5 * max(1.0, abs(le[k])), (i, k, le[k], lg[k])
    assert step.replays == 4
    for name in ('netG_A', 'netG_B', 'netD_A', 'netD_B'):
        diff = _max_param_diff(getattr(graphed, name), getattr(eager, name))
        print('pool_size %d %s: parameter difference %.3g' % (pool_size, name, diff))
        assert diff < 1e-5, name
    assert gb == eb and ga == ea
    if pool_size == 2:
        assert list(zip(gb, ga)) == ORDER_CODES
        for log in (gb, ga):
            replayed = [c for i in (3, 4, 6, 7) for c in log[i]]
            assert any(c >= 0 for c in replayed) and -1 in replayed
    else:
        assert [c for codes in gb for c in codes] == [c for codes in ga for c in codes] == [-2 - k for k in range(sum(ORDER_BATCHES))]
