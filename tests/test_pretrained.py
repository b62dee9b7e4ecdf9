"""CPU: loading a compressed student checkpoint (cat_amd/pretrained.py), Profiler and conv_macs (cat_amd/profiler.py) against what the
reference's own load_pretrained_student / load_pretrained_spade_student left behind (tests/golden/pretrained_student.npz, written by
tools/make_golden_pretrained.py).  The distillers are assembled with __new__ (their constructors need a GPU); nothing here launches a kernel."""
import copy
import itertools
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import helpers as H
from oracle import detfill

G = H.load('pretrained_student.npz')
INCEPTION = ['bn', 'in', 'bn_pruned', 'in_pruned']
SPADE = ['spade', 'spade_pruned']


def rec(tag, key):
    return json.loads(str(G[f'{tag}:{key}']))


def checkpoint(tag, tmp_path):
    """The checkpoint of a case: the recorded shapes filled by detfill with the recorded seed, saved the way save_networks saves."""
    sd = detfill.fill_state_dict(H.sd_from_shapes(G[f'{tag}:shapes']), int(G[f'{tag}:seed']))
    for k in rec(tag, 'head_keys'):      # the head conv at the recorded power of two: the closing tanh stays out of saturation
        sd[k] = sd[k] * float(G[f'{tag}:head_scale'])
    path = os.path.join(str(tmp_path), f'{tag}_net_G.pth')
    torch.save(sd, path)
    return path, sd


def inception_stub(tag, tmp_path, isTrain=True):
    """An InceptionDistiller as its constructor leaves it, on the host: canonical teacher, the ngf-20 student, four netAs, hooks installed."""
    from cat_amd import networks
    from cat_amd import nn as cnn
    from cat_amd.distillers.inception_distiller import InceptionDistiller
    from cat_amd.optim import FusedAdam
    o = rec(tag, 'opt')
    opt = H.make_opt(norm=o['norm'], track=o['track'], target_flops=o['target_flops'], dataset_mode=o['dataset_mode'], gan_mode=o['gan_mode'],
                     ndf=o['ndf'], gpu_ids=[])
    opt.pretrained_student_G_path, sd = checkpoint(tag, tmp_path)
    m = InceptionDistiller.__new__(InceptionDistiller)
    m.opt, m.isTrain, m.device = opt, isTrain, torch.device('cpu')
    m.netG_teacher = networks.define_G(3, 3, 64, 'inception_9blocks', opt.norm, 0, 'normal', 0.02, [], opt=opt).eval()
    m.netG_student = networks.define_G(3, 3, 20, 'inception_9blocks', opt.norm, 0, 'normal', 0.02, [], opt=opt)
    m.netD = cnn.Conv2d(3, 4, 1)
    m.mapping_layers = ['down_sampling.9'] + ['features.%d' % i for i in range(2, 11, 3)]
    m.netAs = [cnn.Conv2d(80, 256, 1) for _ in m.mapping_layers]
    m.Tacts, m.Sacts, m.mapping_hooks = {}, {}, []
    m.optimizer_G = FusedAdam([{'params': m.netG_student.parameters()}, {'params': itertools.chain(*[a.parameters() for a in m.netAs])}],
                              lr=opt.lr, betas=(opt.beta1, 0.999))
    m.optimizer_D = FusedAdam(m.netD.parameters(), lr=opt.lr, betas=(opt.beta1, 0.999))
    m.optimizers = [m.optimizer_G, m.optimizer_D]
    m.add_mapping_hook()
    return m, opt, sd


def spade_stub(tag, tmp_path, **kw):
    from cat_amd.distillers.base_spade_distiller import BaseSPADEDistiller
    from cat_amd.spade_modules import SPADEDistillerModules
    o = rec(tag, 'opt')
    o.update(gpu_ids=[], vgg_width_div=16)
    o.update(kw)
    opt = Namespace(**o)
    opt.pretrained_student_G_path, sd = checkpoint(tag, tmp_path)
    m = BaseSPADEDistiller.__new__(BaseSPADEDistiller)
    m.opt, m.isTrain, m.device = opt, True, torch.device('cpu')
    m.modules = m.modules_on_one_gpu = SPADEDistillerModules(opt)
    m.optimizer_G, m.optimizer_D = m.modules.create_optimizers()
    m.optimizers = [m.optimizer_G, m.optimizer_D]
    return m, opt, sd


def check_common(tag, model, student, net_as, sd, opt):
    loaded = student.state_dict()
    assert [[k, list(v.shape)] for k, v in loaded.items()] == rec(tag, 'loaded_shapes')          # keys, order, shapes: the reference's record
    assert [[k, list(v.shape)] for k, v in loaded.items()] == [[k, list(v.shape)] for k, v in sd.items()]      # ... and the checkpoint's
    assert all(torch.equal(loaded[k], v) for k, v in sd.items())
    assert student.n_macs == int(G[f'{tag}:n_macs'])
    assert [list(a.weight.shape) for a in net_as] == rec(tag, 'netA')
    groups = model.optimizer_G.param_groups
    assert [dict(n=len(g['params']), lr=g['lr'], betas=[float(b) for b in g['betas']]) for g in groups] == rec(tag, 'optim')
    owned = [id(p) for g in groups for p in g['params']]
    want = [id(p) for p in student.parameters()] + [id(p) for a in net_as for p in a.parameters()]
    assert owned == want                                                     # exactly the new parameters, student first
    assert model.optimizers[0] is model.optimizer_G and model.optimizers[1] is model.optimizer_D
    assert len(model.schedulers) == 2 and [s.optimizer for s in model.schedulers] == model.optimizers


@pytest.mark.parametrize('tag', INCEPTION)
def test_load_pretrained_student_matches_the_reference(tag, tmp_path, capsys):
    from cat_amd.pretrained import load_pretrained_student
    m, opt, sd = inception_stub(tag, tmp_path)
    old_student, old_hooks = m.netG_student, list(m.mapping_hooks)
    teacher_sd = copy.deepcopy(m.netG_teacher.state_dict())
    load_pretrained_student(m, opt)
    S = m.netG_student
    assert S is not old_student
    assert [[b.res_channels, b.res_kernel_sizes, b.dw_channels, b.dw_kernel_sizes] for b in S.features] == rec(tag, 'blocks')
    out = capsys.readouterr().out.splitlines()
    assert [ln for ln in out if ln.startswith('features.')] == rec(tag, 'prints')      # the two lines per block, the checkpoint's order
    assert out[-1] == 'Pretrained studentG state is loaded.'
    check_common(tag, m, S, m.netAs, sd, opt)
    # hooks: removed from the old network, on the new one (and still on the teacher)
    named_new = dict(S.named_modules())
    assert len(m.mapping_hooks) == 2 * len(m.mapping_layers) and not set(map(id, old_hooks)) & set(map(id, m.mapping_hooks))
    for n in m.mapping_layers:
        assert len(named_new[n]._forward_hooks) == 1 and len(dict(old_student.named_modules())[n]._forward_hooks) == 0
        assert len(dict(m.netG_teacher.named_modules())[n]._forward_hooks) == 1
    assert all(torch.equal(v, teacher_sd[k]) for k, v in m.netG_teacher.state_dict().items())      # the teacher is only copied from
    if tag.endswith('_pruned'):
        blocks = rec(tag, 'blocks')
        assert blocks[1][0] == [] and blocks[1][2] != [] and blocks[2] == [[], [], [], []] and blocks[3][2][0] == 1
        assert len(S.features[1].res_ops) == 0 and len(S.features[2].res_ops) + len(S.features[2].dw_ops) == 0
        assert S.features[3].dw_ops[0][2][0].weight.shape[:2] == (1, 1)


def test_schedulers_are_rebuilt_only_when_training(tmp_path):
    from cat_amd.pretrained import load_pretrained_student
    m, opt, _ = inception_stub('in', tmp_path, isTrain=False)
    load_pretrained_student(m, opt)
    assert not hasattr(m, 'schedulers')
    m, opt, _ = inception_stub('in', tmp_path, isTrain=True)
    load_pretrained_student(m, opt)
    assert len(m.schedulers) == 2


@pytest.mark.parametrize('tag', SPADE)
def test_load_pretrained_spade_student_matches_the_reference(tag, tmp_path):
    from cat_amd.pretrained import load_pretrained_spade_student
    m, opt, sd = spade_stub(tag, tmp_path)
    mods = m.modules_on_one_gpu
    old_student = mods.netG_student
    load_pretrained_spade_student(m, opt)
    S = mods.netG_student
    assert S is not old_student
    got = {}
    for name, blk in S.get_named_block_list().items():
        got[name] = dict(input_dim=blk.input_dim, output_dim=blk.output_dim, res=[blk.res_channels, blk.res_kernel_sizes],
                         dw=[blk.dw_channels, blk.dw_kernel_sizes], spade_res=[blk.spade.res_channels, blk.spade.res_kernel_sizes],
                         spade_dw=[blk.spade.dw_channels, blk.spade.dw_kernel_sizes], shortcut=blk.shortcut is not None)
    want = rec(tag, 'blocks')
    assert list(got) == list(want) and got == want
    check_common(tag, m, S, list(mods.netAs), sd, opt)
    assert isinstance(mods.netAs, torch.nn.ModuleList)
    if tag.endswith('_pruned'):
        assert want['G_middle_0']['res'] == [[], []] and want['G_middle_1']['res'] == want['G_middle_1']['dw'] == [[], []]
        assert want['up_0']['dw'][0][0] == 1


def test_spade_loader_refuses_what_the_reference_refuses(tmp_path):
    from cat_amd.pretrained import load, load_pretrained_spade_student
    m, opt, _ = spade_stub('spade', tmp_path)
    opt.teacher_norm_G = 'syncbatch'                       # does not start with 'spade'
    with pytest.raises(NotImplementedError):
        load_pretrained_spade_student(m, opt)
    m, opt, _ = spade_stub('spade', tmp_path)
    opt.pretrained_netG = 'inception_9blocks'              # profiler.py:85-86: a spade teacher needs a spade student and pretrained_netG
    with pytest.raises(AssertionError):
        load(m, opt)
    opt.pretrained_netG, opt.student_netG = 'inception_spade', 'inception_9blocks'
    with pytest.raises(AssertionError):
        load(m, opt)


@pytest.mark.parametrize('tag', INCEPTION + SPADE)
def test_reference_twin_of_the_loaded_student_reproduces_the_recorded_forward(tag, tmp_path, capsys):
    """export.to_reference_module (what export_onnx traces) of the loaded student, on the host in fp32, against the float64 forward the
    reference's loaded student gave: test_export.py's bar for a twin against a recorded reference forward (2e-5)."""
    from cat_amd import export, pretrained
    m, opt, _ = (spade_stub if tag in SPADE else inception_stub)(tag, tmp_path)
    pretrained.load(m, opt)
    S = getattr(m, 'modules_on_one_gpu', m).netG_student
    twin = export.to_reference_module(S).eval()
    x = rec(tag, 'x')
    inp = (detfill.normal(tuple(x['shape']), x['seed']) > 0.8).float() if tag in SPADE else detfill.images(tuple(x['shape']), x['seed'])
    with torch.no_grad():
        y = twin(inp)
    got = y.double()[:, :, ::x['sub'], ::x['sub']].numpy()
    e32, e64 = H.rel_err(got, G[f'{tag}:out32']), H.rel_err(got, G[f'{tag}:out'])
    print(f'{tag}: twin vs the reference forward in fp32 {e32:.3e}, in float64 {e64:.3e}')
    assert e32 < 2e-5              # like for like: both are fp32 torch forwards of the same layers (test_export.py's fixtures are fp32 too)
    assert e64 < 1e-3              # the project's fp32-against-oracle bar


def test_conv_macs_reproduces_the_survey_numbers():
    """true conv MACs of the canonical S_2.6, S_4.6 and teacher at 256 x 256 (the configurations of
    test_prune.py::test_survey_canonical_students_are_reproduced): 2 159.4 M, 3 977.7 M, 36 242.6 M."""
    from cat_amd import networks, prune
    from cat_amd.profiler import conv_macs

    def canonical(norm, track, target):
        opt = H.make_opt(norm=norm, track=track, target_flops=target, prune_cin_lb=16)
        torch.manual_seed(233)
        T = networks.define_G(3, 3, 64, 'inception_9blocks', norm, 0, 'normal', 0.02, [], opt=opt)
        gen = torch.Generator().manual_seed(7)
        with torch.no_grad():
            for m in T.modules():
                if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.InstanceNorm2d)) and getattr(m, 'weight', None) is not None:
                    m.weight.copy_(torch.randn(m.weight.shape, generator=gen).abs())
        T.eval()
        thr, _ = prune.search_threshold(T, target, opt)
        S = copy.deepcopy(T)
        prune._apply_structure(S, T, thr, opt, copy_weights=True)
        return T, S

    T, S26 = canonical('instance', False, 2.6e9)
    _, S46 = canonical('batch', True, 4.6e9)
    shape = (1, 3, 256, 256)
    # The survey derives each figure as a sum of three terms it had rounded to 0.1 M (S_2.6: 2 557.5 - 530.8 + 132.7), so a headline figure
    # can be off by up to 0.15 M from the exact count: that is the bound.  The terms themselves are pinned exactly: the reference's conv
    # count the survey prints in full (2 557 476 864), and the transposed convs moving from their output plane to their input plane (/ 4).
    def terms(net):
        convs = sum(m.n_macs for m in net.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)))
        return convs, sum(m.n_macs for m in net.modules() if isinstance(m, torch.nn.ConvTranspose2d))

    for net, headline, ref_count in ((S26, 2159.4, 2557476864), (S46, 3977.7, 4591284224), (T, 36242.6, 43490402304)):
        got = conv_macs(net, shape)
        convs, transposed = terms(net)
        assert convs == ref_count and transposed % 4 == 0 and got == convs - transposed + transposed // 4, (headline, got)
        assert abs(got / 1e6 - headline) < 0.15, (headline, got)
    assert terms(S26)[1] == 530841600 and terms(T)[1] == 9663676416        # 530.8 M and 9 663.7 M in the survey's text
    assert S26.n_macs == 2566197248                       # conv_macs leaves n_macs as model_profiling sets it
    assert conv_macs(S26, (2, 3, 256, 256)) == 2 * conv_macs(S26, shape)


# ------------------------------------------------------------------------------------------------ Profiler on stubs
class _Logger:
    def __init__(self):
        self.calls = []

    def print_info(self, text):
        self.calls.append(('print_info', text))

    def print_current_metrics(self, epoch, i, metrics, t):
        self.calls.append(('print_current_metrics', epoch, i, dict(metrics)))


class _Loader(list):
    dataset = list(range(7))


def _profiler_stub(tag, tmp_path, events, **optkw):
    m, opt, _ = inception_stub(tag, tmp_path)
    from cat_amd import prune
    opt.log_dir, opt.tensorboard_dir, opt.phase, opt.seed = str(tmp_path), None, 'train', 233
    opt.__dict__.update(optkw)
    prune.model_profiling(m.netG_teacher, 64, 96)
    prune.model_profiling(m.netG_student, 64, 96)
    m.setup = lambda o: events.append('setup')
    m.evaluate_model = lambda step, save_image=False: events.append(('evaluate_model', step, save_image)) or {'metric/fid': 1.5}
    loader = _Loader([{'A': torch.zeros(2, 3, 64, 96), 'B': torch.zeros(2, 3, 32, 32)}])
    return m, opt, loader


def test_profiler_sequence_on_stubs(tmp_path, capsys):
    from cat_amd import profiler as P
    events, logger = [], _Logger()
    m, opt, loader = _profiler_stub('in', tmp_path, events)
    times = iter([100.0 + i for i in range(15)])

    def shrink(model, o):
        assert model is m and o is opt
        events.append('shrink')
        model.netG_student = 'shrunk'           # start() must bring the pretrained student back afterwards
        return next(times)

    prof = P.Profiler('distill', opt=opt, dataloader=loader, logger=logger, create_model=lambda o: m, shrink=shrink)
    assert (opt.data_channel, opt.data_height, opt.data_width) == (3, 64, 96) and opt.iters_per_epoch == 1 and opt.tensorboard_dir == str(tmp_path)
    assert open(os.path.join(str(tmp_path), 'opt.txt')).read().endswith('\n')
    S = m.netG_student
    assert events == ['setup'] and [list(v.shape) for v in S.state_dict().values()] == [s for _, s in rec('in', 'loaded_shapes')]
    n_t, n_s = m.netG_teacher.n_macs, S.n_macs
    params = [sum(p.numel() for p in net.parameters()) for net in (m.netG_teacher, S)]
    shape = (1, 3, 64, 96)
    assert logger.calls == [
        ('print_info', f'netG teacher FLOPs: {n_t}.'),
        ('print_info', f'netG student FLOPs: {n_s}.'),
        ('print_info', f'netG teacher FLOPs: {P.conv_macs(copy.deepcopy(m.netG_teacher), shape)} (true conv MACs); Params: {params[0]}.'),
        ('print_info', f'netG student FLOPs: {P.conv_macs(copy.deepcopy(S), shape)} (true conv MACs); Params: {params[1]}.')]
    assert (m.netG_teacher.n_macs, S.n_macs) == (n_t, n_s)
    del logger.calls[:]
    capsys.readouterr()
    prof.start()
    assert events == ['setup'] + ['shrink'] * 15 + [('evaluate_model', 0, True)]
    out = capsys.readouterr().out
    assert 'Average pruning time for 10 experiments: %.2fs.' % np.mean([105.0 + i for i in range(10)]) in out      # the LAST ten of fifteen
    assert m.netG_student is not S and m.netG_student != 'shrunk'
    assert [list(v.shape) for v in m.netG_student.state_dict().values()] == [s for _, s in rec('in', 'loaded_shapes')]
    assert logger.calls == [('print_current_metrics', 0, 0, {'metric/fid': 1.5}), ('print_info', 'Model evaluated.')]


@pytest.mark.parametrize('tag', SPADE)
def test_profiler_and_conv_macs_on_a_spade_distiller(tag, tmp_path):
    """The GauGAN side of Profiler: the cityscapes data shape, the SPADE loader picked by teacher_netG, the four lines.  A
    `spadesyncbatch` generator has no transposed conv and its norms keep running statistics (counted 0 by model_profiling), so conv_macs
    must equal n_macs -- also for the hand-pruned student, whose branch-less block never reaches its SPADE's convs."""
    from cat_amd import profiler as P
    from cat_amd import prune
    m, opt, sd = spade_stub(tag, tmp_path)
    opt.log_dir, opt.tensorboard_dir, opt.phase, opt.seed, opt.dataset_mode = str(tmp_path), None, 'train', 1, 'cityscapes'
    h, w, c = opt.data_height, opt.data_width, opt.data_channel
    del opt.data_height, opt.data_width, opt.data_channel
    prune.model_profiling(m.modules.netG_teacher, h, w, channel=c)
    m.setup = lambda o: None
    loader = _Loader([{'label': torch.zeros(1, 1, h, w), 'instance': torch.zeros(1, 1, h, w), 'image': torch.zeros(1, 3, h, w)}])
    logger = _Logger()
    P.Profiler('distill', opt=opt, dataloader=loader, logger=logger, create_model=lambda o: m)
    assert (opt.data_channel, opt.data_height, opt.data_width) == (c, h, w) == (opt.input_nc + 1, 128, 256)
    T, S = m.modules.netG_teacher, m.modules.netG_student
    assert [[k, list(v.shape)] for k, v in S.state_dict().items()] == rec(tag, 'loaded_shapes') and S.n_macs == int(G[f'{tag}:n_macs'])
    params = [sum(p.numel() for p in net.parameters()) for net in (T, S)]
    assert logger.calls == [
        ('print_info', f'netG teacher FLOPs: {T.n_macs}.'), ('print_info', f'netG student FLOPs: {S.n_macs}.'),
        ('print_info', f'netG teacher FLOPs: {T.n_macs} (true conv MACs); Params: {params[0]}.'),
        ('print_info', f'netG student FLOPs: {S.n_macs} (true conv MACs); Params: {params[1]}.')]
    assert P.conv_macs(S, (2, c, h, w)) == 2 * int(G[f'{tag}:n_macs'])


def test_a_copy_of_an_owned_network_is_not_owned(tmp_path):
    """An inference runner's ownership of eval-mode blocks (fused_block.own_eval) lives in a weak registry, not on the modules: the student
    that load_pretrained_student deep-copies out of an owned teacher belongs to nobody."""
    import gc
    from cat_amd import fused_block
    from cat_amd.pretrained import load_pretrained_student
    m, opt, _ = inception_stub('in', tmp_path)
    for b in m.netG_teacher.features:
        fused_block.own_eval(b, 1)
    before = {k for b in m.netG_teacher.features for k in vars(b)}
    load_pretrained_student(m, opt)
    assert all(fused_block.eval_owned(b) for b in m.netG_teacher.features)
    assert not any(fused_block.eval_owned(mod) for mod in m.netG_student.modules())
    assert not any(fused_block.eval_owned(mod) for mod in copy.deepcopy(m.netG_teacher).modules())
    fused_block.disown_eval(m.netG_teacher.features[0])
    assert not fused_block.eval_owned(m.netG_teacher.features[0]) and fused_block.eval_owned(m.netG_teacher.features[1])
    assert {k for b in m.netG_teacher.features for k in vars(b)} == before          # nothing was written on the modules
    blk = copy.deepcopy(m.netG_teacher.features[1])
    fused_block.own_eval(blk)
    n = len(fused_block._EVAL_OWNED)
    del blk
    gc.collect()
    assert len(fused_block._EVAL_OWNED) == n - 1                     # the registry does not keep a block alive


def test_profiler_refuses_unknown_task_and_dataset_mode(tmp_path):
    from cat_amd import profiler as P
    with pytest.raises(NotImplementedError, match='Unknown task'):
        P.Profiler('test')
    events = []
    m, opt, loader = _profiler_stub('in', tmp_path, events, dataset_mode='single')
    with pytest.raises(NotImplementedError):
        P.Profiler('distill', opt=opt, dataloader=loader, logger=_Logger(), create_model=lambda o: m)
    assert events == []                                     # raised before the model was created


def test_profiler_infers_the_cityscapes_data_shape(tmp_path):
    """profiler.py:65-72: label plane size, input_nc (+ 1 with a dontcare label) (+ the instance map's channels); task 'train' logs nothing."""
    from cat_amd import profiler as P
    opt = Namespace(log_dir=str(tmp_path), tensorboard_dir='tb', phase='val', seed=1, dataset_mode='cityscapes', input_nc=5,
                    contain_dontcare_label=True, no_instance=False)
    loader = _Loader([{'label': torch.zeros(1, 1, 16, 32), 'instance': torch.zeros(1, 1, 16, 32)}] * 3)
    model, logger = Namespace(setup=lambda o: None), _Logger()
    with pytest.warns(UserWarning, match='not using training set'):
        prof = P.Profiler('train', opt=opt, dataloader=loader, logger=logger, create_model=lambda o: model)
    assert (opt.data_channel, opt.data_height, opt.data_width, opt.iters_per_epoch, opt.tensorboard_dir) == (7, 16, 32, 3, 'tb')
    assert prof.model is model and logger.calls == []
