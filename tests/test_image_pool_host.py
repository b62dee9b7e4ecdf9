"""CPU: the host half of the graph-safe image pool (cat_amd/models/image_pool.py).  ImagePool.decide takes the reference loop's decisions
(utils/image_pool.py:27-53) with the reference's draws and writes them as codes; a ten-line interpreter of the code table, which is also what
the kernel cat_image_pool_query is compared with (tests/test_image_pool_gpu.py), turns them back into the reference's outputs."""
import random

import numpy as np
import pytest
import torch

from oracle import ref_cpu

SEED = 0      # chosen on the CPU: with it every case below that can repeat a slot within a batch does (asserted)


def interpret(codes, images, pool):
    """The code table of include/cat_hip.h, sequentially: images [n][...], pool [pool_size][...] (updated in place) -> out [n][...]."""
    out = np.empty_like(images)
    for i, code in enumerate(codes):
        if code == -1:
            out[i] = images[i]
        elif code >= 0:
            out[i] = pool[code]
            pool[code] = images[i]
        else:
            pool[-2 - code] = images[i]
            out[i] = images[i]
    return out


def slot_of(code):
    return code if code >= 0 else -2 - code


def repeats(log):
    """-> (a slot hit twice within one batch, a store followed by a swap of that slot within one batch) over the logged code lists"""
    twice = store_swap = False
    for codes in log:
        seen = {}
        for code in codes:
            if code == -1:
                continue
            s = slot_of(code)
            twice = twice or s in seen
            store_swap = store_swap or (code >= 0 and -2 - s in seen.get(s, []))
            seen.setdefault(s, []).append(code)
    return twice, store_swap


def log_decisions(pool):
    """Record every code list `pool.decide` returns (query and stage both go through it) -> the list they are appended to."""
    log, decide = [], pool.decide

    def logged(n):
        codes = decide(n)
        log.append(list(codes))
        return codes
    pool.decide = logged
    return log


@pytest.mark.parametrize('batch', [1, 3, 4])
@pytest.mark.parametrize('pool_size', [0, 1, 2, 50])
def test_decisions_replay_the_reference(pool_size, batch):
    from cat_amd.models.image_pool import ImagePool
    r_ref, r_mine = random.Random(SEED), random.Random(SEED)
    ref, mine = ref_cpu.ImagePoolRef(pool_size, r_ref), ImagePool(pool_size, r_mine)
    held = np.full((max(pool_size, 1),), -1.0, np.float32)
    log = []
    for q in range(12):
        ids = np.arange(q * batch, (q + 1) * batch, dtype=np.float32) + 1.0      # one id per image, never repeated
        want = ref.query(torch.from_numpy(ids).reshape(batch, 1, 1, 1)).reshape(-1).numpy()
        if pool_size == 0:
            x = torch.from_numpy(ids)
            assert mine.query(x) is x
            got = ids
        else:
            codes = mine.decide(batch)
            log.append(codes)
            assert all(0 <= slot_of(c) < pool_size for c in codes if c != -1)
            got = interpret(codes, ids, held)
            assert mine.num_imgs == ref.num_imgs
            assert [float(t) for t in ref.images] == list(held[:mine.num_imgs]), q
        assert list(got) == list(want), (q, got, want)
        assert r_mine.getstate() == r_ref.getstate(), q
    if pool_size in (1, 2) and batch > 1:
        # pool_size 1 at batch 4: every stored or swapped image of a batch meets slot 0; pool_size 2 at batch 3: the first batch goes
        # store, store, draw -- fill -> full inside a batch
        assert repeats(log) == (True, True), log
    if pool_size == 2 and batch == 3:
        assert log[0][:2] == [-2, -3] and log[0][2] >= -1
    if pool_size == 50:
        assert [c for codes in log for c in codes] == [-2 - k for k in range(12 * batch)]      # 48 images at most: still filling


# B pool then A pool, per step, on ONE generator: random.Random(1), pool_size 2
ORDER_BATCHES = [1, 1, 1, 1, 1, 2, 1, 1]
ORDER_CODES = [([-2], [-2]), ([-3], [-3]), ([-1], [0]), ([-1], [-1]), ([-1], [0]), ([-1, -1], [1, 0]), ([1], [0]), ([0], [0])]


def test_draw_order_across_the_two_pools():
    from cat_amd.models.image_pool import ImagePool
    rng = random.Random(1)
    pool_b, pool_a = ImagePool(2, rng), ImagePool(2, rng)
    got = [(pool_b.decide(n), pool_a.decide(n)) for n in ORDER_BATCHES]
    assert got == ORDER_CODES
    # ... which is the reference's sequence on a shared generator
    rng = random.Random(1)
    ref_b, ref_a = ref_cpu.ImagePoolRef(2, rng), ref_cpu.ImagePoolRef(2, rng)
    held_b, held_a, k = np.full((2,), -1.0, np.float32), np.full((2,), -1.0, np.float32), 0
    for n, (cb, ca) in zip(ORDER_BATCHES, ORDER_CODES):
        ids = np.arange(k, k + n, dtype=np.float32)
        k += n
        for ref, held, codes in ((ref_b, held_b, cb), (ref_a, held_a, ca)):
            want = ref.query(torch.from_numpy(ids).reshape(n, 1, 1, 1)).reshape(-1).numpy()
            assert list(interpret(codes, ids, held)) == list(want)


def test_decide_validates_its_slots():
    from cat_amd.models.image_pool import ImagePool
    for pool_size in (1, 2, 3, 7, 50):
        pool = ImagePool(pool_size, random.Random(pool_size))
        codes = [c for n in (1, 4, 3, 5) * 12 for c in pool.decide(n)]
        assert all(c == -1 or 0 <= slot_of(c) < pool_size for c in codes)
        stores = [c for c in codes if c < -1]
        assert stores == [-2 - k for k in range(pool_size)] and codes[:len(stores)] == stores      # the fill phase, slot by slot, first
        assert any(c >= 0 for c in codes) and -1 in codes

    class Broken(random.Random):
        def randint(self, a, b):
            return b + 1
    pool = ImagePool(2, Broken(3))
    with pytest.raises(AssertionError):
        for _ in range(16):
            pool.decide(4)


def test_stage_replay_is_a_no_op_but_for_the_cyclegan_model():
    from cat_amd.distillers.base_inception_distiller import BaseInceptionDistiller
    from cat_amd.distillers.base_spade_distiller import BaseSPADEDistiller
    from cat_amd.host import StepHost
    from cat_amd.models.base_model import BaseModel
    from cat_amd.models.cycle_gan_model import CycleGANModel
    for cls in (BaseInceptionDistiller, BaseSPADEDistiller, BaseModel):
        assert cls.stage_replay is StepHost.stage_replay
    stub = BaseInceptionDistiller.__new__(BaseInceptionDistiller)
    assert stub.stage_replay({'A': torch.zeros(2, 3, 4, 4)}) is None and vars(stub) == {}
    assert CycleGANModel.stage_replay is not StepHost.stage_replay
    # the CycleGAN model stages the B pool, then the A pool, each with its own batch size
    model, calls = CycleGANModel.__new__(CycleGANModel), []

    class Spy:
        def __init__(self, name):
            self.name = name

        def stage(self, n):
            calls.append((self.name, n))
    model.fake_A_pool, model.fake_B_pool = Spy('A'), Spy('B')
    model.stage_replay({'A': torch.zeros(2, 3, 4, 4), 'B': torch.zeros(3, 3, 4, 4)})
    assert calls == [('B', 2), ('A', 3)]
