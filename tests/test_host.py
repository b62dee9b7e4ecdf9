"""CPU: host-side logic of the drop-in boundary -- state_dict key / shape parity with the reference networks, the
distiller factory and flag surface, fused-Sequential structure, loud failure without a GPU."""
import argparse
import os

import pytest
import torch

import helpers as H


@pytest.mark.parametrize('tag,norm,track', [('in', 'instance', False), ('bn', 'batch', True)])
def test_state_dict_keys_match_reference(tag, norm, track):
    """tests/golden/forward_*.npz records the reference student's state_dict (keys, shapes) after shrink_model."""
    g = H.load(f'forward_{tag}.npz')
    shapes = H.sd_from_shapes(g['student_shapes'])
    opt = H.make_opt(norm=norm, track=track)
    net = H.student_from_shapes(opt, shapes)
    assert list(net.state_dict().keys()) == list(shapes.keys())
    from cat_amd import networks
    T = networks.define_G(3, 3, 64, 'inception_9blocks', norm, 0, 'normal', 0.02, [], opt=opt)
    tsd = T.state_dict()
    if track:   # BatchNorm: no conv bias in front of a norm (inception_generator.py:30-33), 95 norm layers with running stats
        assert 'down_sampling.1.bias' not in tsd and sum(k.endswith('running_var') for k in tsd) == 95
    else:
        assert len(tsd) == 472
    D = networks.define_D(6, 128, 'n_layers', 3, norm, 'normal', 0.02, [], opt=opt)
    assert [k for k in D.state_dict() if k.endswith('weight')][:2] == ['model.0.weight', 'model.2.weight']
    assert D.model[0].bias is not None and (D.model[2].bias is None) == (norm == 'batch')


def test_spadeinstance_generator_has_the_reference_state_dict():
    """norm_G = 'spadeinstance3x3' (reference inception_modules.py:414-415): hidden / shortcut / param-free norms are InstanceNorm2d (no
    running statistics in the state_dict), the gamma|beta nets keep SynchronizedBatchNorm2d -- keys and shapes as the reference's own
    generator recorded them (tests/golden/spade_instance_fwd.npz)."""
    import json
    from argparse import Namespace
    g = H.load('spade_instance_fwd.npz')
    o = json.loads(str(H.load('spade_step.npz')['opt']))
    o.update(gpu_ids=[], ngf=6, norm_G='spadeinstance3x3', data_height=128, data_width=256, data_channel=o['semantic_nc'])
    opt = Namespace(**o)
    from cat_amd import networks, nn as cnn
    G = networks.define_G(opt.input_nc, 3, 6, 'inception_spade', 'instance', 0, 'xavier', 0.02, [], opt=opt)
    assert [[k, list(v.shape)] for k, v in G.state_dict().items()] == json.loads(str(g['shapes']))
    assert type(G.up_3.spade.param_free_norm) is cnn.InstanceNorm2d and type(G.up_3.shortcut[0]) is cnn.InstanceNorm2d
    assert isinstance(G.up_3.spade.res_ops[0][0].norm, cnn.SynchronizedBatchNorm2d) and type(G.up_3.res_ops[0][0].norm) is cnn.InstanceNorm2d
    assert len(G.up_3.get_first_bn()) == 6


def test_weights_are_channels_last_after_flatten_rules():
    from cat_amd import nn as cnn, ops
    c = cnn.Conv2d(6, 4, 3)
    ref = c.weight.detach().clone()
    new = ops.padded_weight_like(c.weight.shape, c.weight.device)      # [O][kh][kw][round_up(I,4)], zero padded
    new.copy_(c.weight.data)
    c.weight.data = new
    assert ops.weight_wcs(c.weight) == 8 and c.weight.stride() == (72, 1, 24, 8)
    sd = c.state_dict()
    assert sd['weight'].shape == (4, 6, 3, 3) and torch.equal(sd['weight'], ref)   # logical OIHW is the checkpoint format
    assert ops.weight_wcs(ref.contiguous(memory_format=torch.channels_last)) == 6    # dense channels_last is accepted too
    assert ops.weight_wcs(ref) is None                                               # plain NCHW-contiguous is not


def test_weight_stride_of_single_row_and_single_channel_weights():
    """ops.weight_wcs for the layouts whose strides do not tell: a [1][I][1][1] row is padded only if its storage holds the padded row
    (FusedAdam re-houses the dense one), and a one-input-channel weight [O][1][1][1] has row stride 1 -- what the fused blocks' gradient
    scatter must respect (round 3: it wrote cs4 = 4 columns per row there and overwrote the next parameter's first gradient entry)."""
    from cat_amd import ops
    assert ops.weight_wcs(torch.zeros(1, 6, 1, 1)) is None                                # dense row, 6 floats of storage: not the padded layout
    assert ops.weight_wcs(torch.zeros(1, 8, 1, 1)) == 8
    padded = ops.padded_weight_like((1, 6, 1, 1), 'cpu')
    assert ops.weight_wcs(padded) == 8 and padded.shape == (1, 6, 1, 1)
    big = torch.zeros(4, 6, 1, 1)
    assert ops.weight_wcs(big[1:2]) is None      # a dense row INSIDE a larger storage (round 4: was taken for a padded one; neighbours got read / written)
    fa = torch.as_strided(torch.zeros(64), (1, 6, 1, 1), (8, 1, 8, 8), 16)
    assert ops.weight_wcs(fa) == 8               # FusedAdam's view of a padded row keeps the padded strides
    assert ops.weight_wcs(torch.zeros(1, 1, 1, 1)) == 1                                   # (a branch pruned to one channel on a one-channel input)
    one = torch.zeros(6, 1, 1, 1)
    assert ops.weight_wcs(one) == 1                                                       # what FusedAdam keeps for shape[1] == 1
    assert ops.weight_wcs(ops.padded_weight_like((6, 1, 1, 1), 'cpu')) == 4


def test_factory_and_flags():
    from cat_amd.distillers import find_distiller_using_name, get_option_setter
    cls = find_distiller_using_name('inception')
    assert cls.__name__ == 'InceptionDistiller'
    p = argparse.ArgumentParser()
    for flag in ('--norm', '--dataset_mode', '--log_dir'):
        p.add_argument(flag, default=None)
    get_option_setter('inception')(p, True)
    o = p.parse_args([])
    assert o.teacher_ngf == 64 and o.student_ngf == 48 and o.lambda_recon == 100 and o.distill_G_loss_type == 'mse'
    assert o.norm == 'instance' and o.dataset_mode == 'aligned' and o.pretrained_ngf == 64 and o.target_flops == 0
    with pytest.raises(NotImplementedError):
        find_distiller_using_name('munit')
    # --distiller spade: flags and defaults of base_spade_distiller.py:27-138 / spade_distiller.py:24-84 / discriminators.py:185-203
    assert find_distiller_using_name('spade').__name__ == 'SPADEDistiller'
    p = argparse.ArgumentParser()
    for flag, d in (('--netD', 'n_layers'), ('--ndf', 128), ('--dataset_mode', None), ('--batch_size', 1), ('--print_freq', 100),
                    ('--save_latest_freq', 1), ('--save_epoch_freq', 1), ('--nepochs', 1), ('--nepochs_decay', 1), ('--init_type', 'normal'),
                    ('--n_layers_D', 3)):
        p.add_argument(flag, default=d)
    get_option_setter('spade')(p, True)
    o = p.parse_args([])
    assert o.teacher_ngf == 64 and o.student_ngf == 48 and o.teacher_norm_G == 'spadesyncbatch3x3' and o.num_upsampling_layers == 'more'
    assert o.lambda_feat == 10 and o.lambda_vgg == 10 and o.lambda_distill == 10 and o.netD == 'multi_scale' and o.ndf == 64
    assert o.num_D == 2 and o.norm_D == 'spectralinstance' and o.n_layers_D == 4 and o.init_type == 'xavier' and o.prune_cin_lb == 1
    assert o.no_TTUR is False and o.batch_size == 16


def test_no_cpu_fallback():
    from cat_amd import ops
    from cat_amd import networks
    opt = H.make_opt()
    net = networks.define_G(3, 3, 16, 'inception_9blocks', 'instance', 0, 'normal', 0.02, [], opt=opt)
    with pytest.raises(RuntimeError, match='GPU only'):
        net(torch.zeros(1, 3, 32, 32))
    if not torch.cuda.is_available():
        from cat_amd.distillers import create_distiller
        with pytest.raises(RuntimeError, match='MI355X'):
            create_distiller(opt, verbose=False)


def test_loss_value_arithmetic():
    from cat_amd.distillers.base_inception_distiller import LossValue
    a, b = torch.tensor(2.0), torch.tensor(3.0)
    v = LossValue([(0.5, a), (0.5, b)])
    assert float(v) == 2.5 and float(v * 2) == 5.0 and float(v + LossValue([(1.0, a)]) + 0) == 4.5


def test_synthetic_fills_match_the_oracle_side_copy():
    """cat_amd.synthetic (bench / smoke inputs) and oracle/detfill.py (fixtures) are the same fills, kept apart so that nothing on
    the measured path imports oracle/."""
    from cat_amd import synthetic
    from oracle import detfill
    for seed in (1, 7):
        assert torch.equal(synthetic.images((2, 3, 8, 8), seed), detfill.images((2, 3, 8, 8), seed))
        assert torch.equal(synthetic.normal((5,), seed, 0.3), detfill.normal((5,), seed, 0.3))
    sd = {'a.weight': torch.zeros(4, 3, 3, 3), 'a.bias': torch.zeros(4), 'n.weight': torch.zeros(4), 'n.running_var': torch.zeros(4),
          'n.running_mean': torch.zeros(4), 'n.num_batches_tracked': torch.zeros((), dtype=torch.long)}
    for gam in (False, True):
        a, b = synthetic.fill_state_dict(sd, 5, gam), detfill.fill_state_dict(sd, 5, gam)
        assert all(torch.equal(a[k], b[k]) for k in sd)
    assert synthetic.SEED_TEACHER == H.SEED_T
    lab, ins = synthetic.label_maps(2, 32, 64, 3)
    assert lab.shape == (2, 1, 32, 64) and lab.dtype == torch.int32 and int(lab.max()) < 35 and int(ins.max()) < 1000
    assert bool((lab[:, :, :16, :16] == lab[:, :, :1, :1]).all())


def test_bench_measured_path_does_not_touch_the_oracle():
    """Only the cpu_baseline legs of bench.py may import oracle/ (and nothing may import tests/): checked on the AST."""
    import ast
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tree = ast.parse(open(os.path.join(root, 'bench.py')).read())

    def imports(node):
        out = []
        for x in ast.walk(node):
            if isinstance(x, ast.Import):
                out += [a.name.split('.')[0] for a in x.names]
            elif isinstance(x, ast.ImportFrom) and x.module:
                out.append(x.module.split('.')[0])
        return out
    for node in tree.body:
        names = imports(node)
        assert 'helpers' not in names and 'tests' not in names
        if 'oracle' in names:
            assert isinstance(node, ast.FunctionDef) and node.name.startswith('cpu_baseline'), getattr(node, 'name', node)
    # the product package never imports the oracle either
    pkg = os.path.join(root, 'cat_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                assert 'oracle' not in imports(ast.parse(open(os.path.join(dirpath, f)).read())), f


def test_bench_dump_outputs_writes_a_fixed_sample():
    """bench.py --dump-outputs (dump_outputs, host side): losses as float64 scalars, generated images (not the inputs) and the optimizers'
    parameters as float32, an array above DUMP_MAX_ELEMS as the same seeded sample in every run, 64 MB at most."""
    import tempfile
    import numpy as np
    import bench

    class Stub:
        def __init__(self):
            torch.manual_seed(3)
            self.netG, self.netD = torch.nn.Linear(10, 10), torch.nn.Linear(1100, bench.DUMP_MAX_ELEMS // 1000)
            self.optimizer_G, self.optimizer_D = torch.optim.Adam(self.netG.parameters()), torch.optim.Adam(self.netD.parameters())
            self.optimizers = [self.optimizer_G, self.optimizer_D]

        def finish_pending(self):
            pass

        def get_current_losses(self):
            return {'G_loss/G_gan': 1.5, 'D_loss/D_real': 0.25, 'Specific_loss/G_distill0': 2.0}

        def get_current_visuals(self):
            return {'real_A': torch.ones(2, 3, 8, 8), 'Sfake_B': torch.full((2, 3, 8, 8), 0.5, dtype=torch.float64)}

    got = []
    for _ in range(2):
        with tempfile.TemporaryDirectory() as d:
            bench.dump_outputs(Stub(), d)
            got.append({f: np.load(os.path.join(d, f)) for f in os.listdir(d)})
            assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= bench.DUMP_MAX_BYTES
    a, b = got
    assert sorted(a) == ['Sfake_B.npy', 'loss_D_real.npy', 'loss_G_distill0.npy', 'loss_G_gan.npy', 'params_D.npy', 'params_G.npy']
    assert a['loss_G_gan.npy'].dtype == np.float64 and float(a['loss_G_gan.npy']) == 1.5
    assert a['Sfake_B.npy'].dtype == np.float32 and a['Sfake_B.npy'].shape == (2, 3, 8, 8)
    net = Stub().netD
    full = torch.cat([net.weight.detach().reshape(-1), net.bias.detach()]).numpy()
    assert full.size > bench.DUMP_MAX_ELEMS and a['params_D.npy'].shape == (bench.DUMP_MAX_ELEMS,)
    assert np.isin(a['params_D.npy'], full).all()
    assert a['params_G.npy'].shape == (110,)
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_no_undefined_names_in_gpu_only_code():
    """Most of cat_amd/ only executes on an MI355X; a scope-aware undefined-name pass over the sources (tools/lint_names.py) keeps
    typos in those branches from surfacing first on the GPU box."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('lint_names', os.path.join(root, 'tools', 'lint_names.py'))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    bad = []
    for top in ('cat_amd', 'bench.py', '__graft_entry__.py', 'oracle', 'tests'):
        path = os.path.join(root, top)
        files = [path] if path.endswith('.py') else [os.path.join(d, f) for d, _, fs in os.walk(path) for f in fs if f.endswith('.py')]
        for f in files:
            bad += [(os.path.relpath(f, root), line, name) for line, name in lint.check(f)]
    assert not bad, bad


def test_frozen_plan_cache_follows_optimizer_steps():
    """The kernels update weights through raw pointers (torch's _version never moves): a block whose parameters belong to a FusedAdam --
    a BatchNorm student run in eval mode by evaluate_model between training steps -- must re-fold its weights after every optimizer
    step, while the frozen teacher folds once (cat_amd/frozen.py::_plan; folding itself is plain tensor arithmetic, so it runs here)."""
    from cat_amd import frozen, networks, optim
    opt = H.make_opt(norm='batch', track=True)
    net = networks.define_G(3, 3, 16, 'inception_9blocks', 'batch', 0, 'normal', 0.02, [], opt=opt)
    net.eval()
    blk = net.features[0]
    p1 = frozen._plan(blk)
    assert frozen._plan(blk) is p1
    w = blk.res_ops[0][1][0].weight
    w.data.mul_(2.0)                                     # what the Adam kernel does: no version bump
    assert frozen._plan(blk) is p1                       # not optimizer-owned (the teacher): folded once
    w._cat_grad_view = torch.zeros(1)                    # as FusedAdam registers its parameters
    p2 = frozen._plan(blk)
    assert p2 is not p1 and frozen._plan(blk) is p2
    optim._bump_weights_epoch()                          # FusedAdam.step / note_graph_replay
    p3 = frozen._plan(blk)
    assert p3 is not p2 and not torch.equal(p3['w_a'], p1['w_a'])
    # same rule for the conv + eval-BatchNorm fold of the down / up-sampling layers (cat_amd/nn.py::_folded_eval_bn)
    from cat_amd import nn as cnn
    conv, bn = net.down_sampling[4], net.down_sampling[5]
    with torch.no_grad():
        w1, _ = cnn._folded_eval_bn(conv, bn, 0)
        conv.weight.data.mul_(2.0)
        assert cnn._folded_eval_bn(conv, bn, 0)[0] is w1
        conv.weight._cat_grad_view = torch.zeros(1)
        w2, _ = cnn._folded_eval_bn(conv, bn, 0)
        optim._bump_weights_epoch()
        w3, _ = cnn._folded_eval_bn(conv, bn, 0)
    assert w2 is not w1 and w3 is not w2 and torch.allclose(w3, 2 * w1)


def test_remove_spectral_norm_matches_torch():
    """cnn.remove_spectral_norm bakes weight_orig / sigma with the current u, v exactly like torch.nn.utils.remove_spectral_norm
    (the export path, reference inception_modules.py:314-315)."""
    import torch
    from cat_amd import nn as cnn
    torch.manual_seed(5)
    mine = cnn.spectral_norm(cnn.Conv2d(6, 5, 3, padding=1))
    twin = torch.nn.utils.spectral_norm(torch.nn.Conv2d(6, 5, 3, padding=1))
    with torch.no_grad():
        twin.weight_orig.copy_(mine.weight_orig)
        twin.bias.copy_(mine.bias)
        twin.weight_u.copy_(mine.weight_u)
        twin.weight_v.copy_(mine.weight_v)
    twin.eval()
    torch.nn.utils.remove_spectral_norm(twin)
    cnn.remove_spectral_norm(mine)
    assert sorted(mine.state_dict().keys()) == sorted(twin.state_dict().keys()) == ['bias', 'weight']
    assert isinstance(mine.weight, torch.nn.Parameter)
    assert torch.allclose(mine.weight, twin.weight, rtol=1e-6, atol=1e-7)
    import pytest
    with pytest.raises(ValueError):
        cnn.remove_spectral_norm(mine)


def test_split_bf16_emulation_properties():
    """tools/bf16x3_numerics.py restates split-bf16 matrix arithmetic with fp32 convolutions (exploratory).  What that rests on:
    the bf16 parts of an fp32 number sum back to it exactly (three parts) or to 2^-16 (two), products of parts are exact in fp32, and the
    1 / 3 / 6-product forms of a dot product land in the error classes 2^-8 / 2^-16 / 2^-24 of sum |a b|."""
    import importlib.util
    import torch.nn.functional as F
    spec = importlib.util.spec_from_file_location('bf16x3_numerics', os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                                'tools', 'bf16x3_numerics.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4096, generator=g) * torch.logspace(-6, 6, 4096)
    a1, a2, a3 = m.split(x, 3)
    assert torch.equal(a1 + a2 + a3, x)                                   # three bf16 parts carry all 24 bits
    h1, h2 = m.split(x, 2)
    assert float(((h1 + h2 - x).abs() / x.abs()).max()) <= 2.0 ** -16
    for t in (a1, a2, a3):
        assert torch.equal(t.to(torch.bfloat16).to(torch.float32), t)     # each part IS a bf16 value
    p = (a1.double() * a2.double())
    assert torch.equal((a1 * a2).double(), p)                             # 8-bit x 8-bit mantissas: the fp32 product is exact
    a = torch.randn(8, 64, 9, 9, generator=g)
    w = torch.randn(16, 64, 3, 3, generator=g)
    exact = F.conv2d(a.double(), w.double())
    scale = F.conv2d(a.double().abs(), w.double().abs())
    err = {}
    for terms in (1, 3, 6):
        m.TERMS = terms
        y = m.combine(lambda u, v: F.conv2d(u, v), a, w)
        err[terms] = float(((y.double() - exact).abs() / scale).max())
    assert 2.0 ** -12 < err[1] < 2.0 ** -7 and err[3] < 2.0 ** -15 and err[6] < 2.0 ** -20 and err[6] < err[3] < err[1], err


def test_lockstep_driver_merges_the_kth_exchanges():
    """fused_spade._drive / _drive_many (round 5): unit forwards / backwards are generators that yield the buffer of each statistics exchange.
    _drive performs every exchange on the spot; _drive_many advances several independent units in lockstep and sends their k-th exchanges as ONE
    collective -- units with fewer exchanges simply finish earlier.  Pure host logic: checked with stand-in generators and a recording reducer."""
    import torch
    from cat_amd import fused_spade, ops

    class Recorder:
        world_size = 2

        def __init__(self):
            self.calls = []

        def all_reduce_sum_(self, t):
            self.calls.append([t])
            return t.mul_(2.0)

        def all_reduce_sum_many_(self, ts):
            self.calls.append(list(ts))
            for t in ts:
                t.mul_(2.0)
            return ts

    def unit(tag, nexch):
        total = 0.0
        for k in range(nexch):
            buf = torch.full((3,), float(10 * tag + k))
            yield buf
            total += float(buf.sum())          # the reduced values are what the unit continues with
        return tag, total

    rec = Recorder()
    ops.set_bn_sync(rec)
    try:
        before = fused_spade.STATS['collectives']
        assert fused_spade._drive(unit(1, 2)) == (1, 2 * 3 * (10 + 11))
        assert [len(c) for c in rec.calls] == [1, 1] and fused_spade.STATS['collectives'] == before + 2
        rec.calls.clear()
        res = fused_spade._drive_many([unit(1, 2), unit(2, 1), unit(3, 2), unit(4, 0)])
        assert res == [(1, 2 * 3 * 21.0), (2, 2 * 3 * 20.0), (3, 2 * 3 * 61.0), (4, 0.0)]
        assert [len(c) for c in rec.calls] == [3, 2]                       # first exchanges of units 1, 2, 3 together; second ones of 1 and 3
        assert fused_spade.STATS['collectives'] == before + 4
    finally:
        ops.set_bn_sync(None)


def test_lockstep_driver_hands_out_one_arena_per_round():
    """Units that ask for their exchange buffer first (fused_spade.Alloc, what the fused GauGAN units do) get adjacent slices of ONE arena per
    lockstep round, in unit order: the merged collective can run on the arena itself (DataParallelReducer.all_reduce_sum_many_ detects the
    adjacency) instead of packing with torch.cat and unpacking with copy_ (round-5 verdict, robustness #15)."""
    import torch
    from cat_amd import fused_spade, ops

    class Recorder:
        world_size = 2

        def __init__(self):
            self.rounds = []

        def all_reduce_sum_(self, t):
            self.rounds.append([t])
            return t.mul_(2.0)

        def all_reduce_sum_many_(self, ts):
            self.rounds.append(list(ts))
            for t in ts:
                t.mul_(2.0)
            return ts

    def unit(tag, sizes):
        total = 0.0
        for k, n in enumerate(sizes):
            buf = yield fused_spade.Alloc(n, torch.device('cpu'))
            assert buf.numel() == n and buf.is_contiguous()
            buf.fill_(float(10 * tag + k))
            yield buf
            total += float(buf.sum())
        return tag, total

    rec = Recorder()
    ops.set_bn_sync(rec)
    try:
        assert fused_spade._drive(unit(1, [8, 16])) == (1, 2 * (8 * 10 + 16 * 11))
        rec.rounds.clear()
        res = fused_spade._drive_many([unit(1, [8, 16]), unit(2, [24]), unit(3, [8, 8]), unit(4, [])])
        assert res == [(1, 2.0 * (8 * 10 + 16 * 11)), (2, 2.0 * 24 * 20), (3, 2.0 * (8 * 30 + 8 * 31)), (4, 0.0)]
        assert [len(r) for r in rec.rounds] == [3, 2]
        for r in rec.rounds:       # one storage, back to back, in unit order
            assert len({t.untyped_storage().data_ptr() for t in r}) == 1
            for a, b in zip(r, r[1:]):
                assert a.data_ptr() + 4 * a.numel() == b.data_ptr()
    finally:
        ops.set_bn_sync(None)
