"""CPU: the host classes that drive a training step share one base and one loss path -- one LossValue / seed cache / seeded backward
(cat_amd/lossvalue.py), one Trainer-facing base (cat_amd/host.py::StepHost), the GauGAN halves (cat_amd/spade_modules.py::SPADEStep,
SPADEModules) and one GAN-mode table (loss.GANLoss.kind) -- without moving a checkpoint file name, a state_dict key or a parameter.
The step classes are assembled with __new__ (their constructors need a GPU); the GauGAN modules are the product's own, narrow, on the CPU,
and are never run forward."""
import json
import os
from argparse import Namespace

import pytest
import torch

import helpers as H


# ------------------------------------------------------------------------------------------------ one LossValue, one seed cache
def test_there_is_one_loss_value_class():
    from cat_amd import lossvalue, spade_modules
    from cat_amd.distillers import base_inception_distiller
    assert base_inception_distiller.LossValue is lossvalue.LossValue and spade_modules.LossValue is lossvalue.LossValue


def test_loss_value_is_the_superset():
    from cat_amd.lossvalue import LossValue
    a, b = torch.tensor(2.0), torch.tensor(3.0)
    v = LossValue([(0.5, a), (0.5, b)])
    assert float(v) == 2.5 and v.item() == 2.5 and float(v / 2) == 1.25 and float(v * 2) == float(2 * v) == 5.0
    assert v.mean() is v and v.detach() is v and (0 + v) is v and (v + 0) is v
    assert float(v + a) == 4.5 and float(sum([v, LossValue([(1.0, a)])])) == 4.5


def test_seeds_are_cached_per_device_and_value():
    from cat_amd import lossvalue
    cpu = torch.device('cpu')
    s = lossvalue.seed(cpu, 0.5)
    assert lossvalue.seed(cpu, 0.5) is s and lossvalue.seed(torch.tensor(1.0).device, 0.5) is s
    assert lossvalue.seed(cpu, 0.25) is not s
    assert s.shape == () and s.dtype == torch.float32 and float(s) == 0.5 and float(lossvalue.seed(cpu, 0.25)) == 0.25


def test_backward_terms_seeds_with_the_weights_and_skips_constants(monkeypatch):
    from cat_amd import lossvalue, ops
    joins = []
    monkeypatch.setattr(ops, 'sync_side_streams', lambda: joins.append(float(x.grad)))      # (needs a GPU stream) called AFTER the pass
    x, y = torch.tensor(3.0, requires_grad=True), torch.tensor(5.0, requires_grad=True)
    const = torch.tensor(7.0)                      # does not require grad: dropped, not an autograd error
    lossvalue.backward_terms([(0.5, x * x), (100.0, const), (-2.0, 4.0 * y)])
    assert float(x.grad) == 0.5 * 2 * 3.0 and float(y.grad) == -2.0 * 4.0
    lossvalue.LossValue([(0.25, x * 2.0), (1.0, const)]).backward()      # LossValue.backward is the same path; gradients accumulate
    assert float(x.grad) == 3.0 + 0.5 and joins == [3.0, 3.5]


# ------------------------------------------------------------------------------------------------ one host base
def _step_classes():
    from cat_amd.distillers.base_inception_distiller import BaseInceptionDistiller
    from cat_amd.distillers.base_spade_distiller import BaseSPADEDistiller
    from cat_amd.models.base_model import BaseModel
    from cat_amd.models.spade_model import SPADEModel
    return BaseModel, BaseInceptionDistiller, BaseSPADEDistiller, SPADEModel


def test_the_bookkeeping_methods_are_one_function():
    from cat_amd.distillers.base_inception_distiller import BaseInceptionDistiller
    from cat_amd.host import StepHost
    for name in ('get_current_losses', 'set_requires_grad', 'update_learning_rate', 'get_current_visuals', 'save_networks', 'print_networks',
                 'save_optimizers', 'restore_optimizers', 'seed', 'finish_pending'):
        for cls in _step_classes():
            assert getattr(cls, name) is getattr(StepHost, name), (cls.__name__, name)
    assert [cls.setup is StepHost.setup for cls in _step_classes()] == [True, False, True, True]     # the inception distiller adds its hooks
    assert BaseInceptionDistiller.setup is not StepHost.setup


# loss names as the classes declare them (cat_amd/distillers/*.py, cat_amd/models/*.py)
LOSS_NAMES = {
    'inception distiller': ['G_gan', 'G_distill', 'G_recon', 'D_fake', 'D_real'] + ['G_distill%d' % i for i in range(4)],
    'spade distiller': ['G_gan', 'G_feat', 'G_vgg', 'G_distill', 'D_real', 'D_fake'] + ['G_distill%d' % i for i in range(3)],
    'pix2pix': ['G_gan', 'G_recon', 'D_real', 'D_fake', 'G_comp_cost'],
    'cycle_gan': ['D_A', 'G_A', 'G_cycle_A', 'G_idt_A', 'D_B', 'G_B', 'G_cycle_B', 'G_idt_B'],
    'spade model': ['G_gan', 'G_feat', 'G_vgg', 'D_real', 'D_fake'],
}


@pytest.mark.parametrize('who', sorted(LOSS_NAMES))
def test_current_losses_keys(who):
    """Both historic forms of get_current_losses (unknown prefix asserts / falls through to G_loss/) give these keys for every declared name."""
    from cat_amd.distillers.base_spade_distiller import BaseSPADEDistiller
    m = BaseSPADEDistiller.__new__(BaseSPADEDistiller)
    m.loss_names = LOSS_NAMES[who] + ['G_never_set']
    for i, n in enumerate(LOSS_NAMES[who]):
        setattr(m, 'loss_' + n, torch.tensor(float(i)))
    want = [('Specific_loss/' if any(c.isdigit() for c in n) else 'D_loss/' if n.startswith('D_') else 'G_loss/') + n for n in LOSS_NAMES[who]]
    got = m.get_current_losses()
    assert list(got) == want and list(got.values()) == [float(i) for i in range(len(want))]
    m.loss_names = ['fake']
    m.loss_fake = 0.0
    with pytest.raises(AssertionError):
        m.get_current_losses()


def test_no_gpu_message_keeps_each_class_wording():
    models, inception, spade, teacher = _step_classes()
    assert (models._NOUN, inception._NOUN, spade._NOUN, teacher._NOUN) == ('models', 'distillers', 'distillers', 'models')
    if not torch.cuda.is_available():
        from cat_amd.models.pix2pix_model import Pix2PixModel
        opt = Namespace(isTrain=True, gpu_ids=[0])
        with pytest.raises(RuntimeError, match='cat_amd distillers need an MI355X'):
            spade(opt)
        with pytest.raises(RuntimeError, match='cat_amd models need an MI355X'):
            Pix2PixModel(opt)


# ------------------------------------------------------------------------------------------------ the GauGAN halves on CPU modules
def spade_opt(log_dir):
    """The recorded GauGAN options (tests/golden/spade_model_step.npz: teacher and distiller flags), narrow, 16 x 32, no device."""
    o = json.loads(str(H.load('spade_model_step.npz')['opt']))
    o.update(gpu_ids=[], teacher_ngf=8, student_ngf=4, ngf=8, ndf=8, vgg_width_div=16, data_height=16, data_width=32, crop_size=32,
             data_channel=o['semantic_nc'], log_dir=str(log_dir), restore_G_path=None, restore_O_path=None)
    return Namespace(**o)


def spade_modules(kind, opt):
    torch.manual_seed(11)
    if kind == 'distiller':
        from cat_amd.spade_modules import SPADEDistillerModules
        return SPADEDistillerModules(opt)
    from cat_amd.spade_model_modules import SPADEModelModules
    return SPADEModelModules(opt)


def layout(modules):
    return {'state_dict': list(modules.state_dict()), 'parameters': [list(p.shape) for p in modules.parameters()]}


def _stub(kind, tmp_path):
    from cat_amd.distillers.base_spade_distiller import BaseSPADEDistiller
    from cat_amd.models.spade_model import SPADEModel
    opt = spade_opt(tmp_path)
    m = (BaseSPADEDistiller if kind == 'distiller' else SPADEModel).__new__(BaseSPADEDistiller if kind == 'distiller' else SPADEModel)
    m.opt, m.isTrain = opt, True
    m.save_dir = os.path.join(str(tmp_path), 'checkpoints')
    m.modules = m.modules_on_one_gpu = spade_modules(kind, opt)
    m.model_names = ['G_student', 'G_teacher', 'D'] if kind == 'distiller' else ['G', 'D']
    m.optimizer_G, m.optimizer_D = m.modules.create_optimizers()
    m.optimizers = [m.optimizer_G, m.optimizer_D]
    return m, opt


@pytest.mark.parametrize('kind', ['distiller', 'teacher'])
def test_gaugan_checkpoint_names_and_module_layout(kind, tmp_path, capsys):
    m, opt = _stub(kind, tmp_path)
    mods = m.modules
    # registration order: state_dict keys and parameter order as the parent commit built them (tests/golden/spade_modules_layout.json)
    want = json.load(open(os.path.join(H.GOLDEN, 'spade_modules_layout.json')))[kind]
    got = layout(mods)
    assert got['state_dict'] == want['state_dict'] and got['parameters'] == want['parameters']
    m.save_networks('latest')
    nets = {'distiller': ['latest_net_A-0.pth', 'latest_net_A-1.pth', 'latest_net_A-2.pth', 'latest_net_D.pth', 'latest_net_G.pth'],
            'teacher': ['latest_net_D.pth', 'latest_net_G.pth']}[kind]
    assert sorted(os.listdir(m.save_dir)) == nets + ['latest_optim-0.pth', 'latest_optim-1.pth']
    saved = {'latest_net_G.pth': mods.netG_student if kind == 'distiller' else mods.netG, 'latest_net_D.pth': mods.netD}
    if kind == 'distiller':
        saved.update({'latest_net_A-%d.pth' % i: a for i, a in enumerate(mods.netAs)})
    for f, net in saved.items():
        sd = torch.load(os.path.join(m.save_dir, f))
        assert list(sd) == list(net.state_dict()) and all(v.is_contiguous() and v.device.type == 'cpu' for v in sd.values()), f
        assert all(torch.equal(v, net.state_dict()[k]) for k, v in sd.items()), f
    # TTUR: one rule for both modules, (beta1, beta2, G_lr, D_lr)
    assert mods._ttur() == (0.0, 0.9, opt.lr / 2, opt.lr * 2)
    assert m.optimizer_G.param_groups[0]['lr'] == opt.lr / 2 and m.optimizer_D.param_groups[0]['lr'] == opt.lr * 2
    assert m.optimizer_G.param_groups[0]['betas'] == (0.0, 0.9)
    mods.opt.no_TTUR = True
    assert mods._ttur() == (opt.beta1, opt.beta2, opt.lr, opt.lr)
    # the frozen parts stay in eval mode through train()
    mods.train()
    assert mods.training and not mods.criterionVGG.training and (kind == 'teacher' or not mods.netG_teacher.training)
    # the networks come back through load_networks under the restore_* flags of each class
    b, optb = _stub(kind, tmp_path / 'b')
    g_flag = 'restore_student_G_path' if kind == 'distiller' else 'restore_G_path'
    for o in (b.opt, b.modules.opt):
        setattr(o, g_flag, os.path.join(m.save_dir, 'latest_net_G.pth'))
        o.restore_D_path = os.path.join(m.save_dir, 'latest_net_D.pth')
        if kind == 'distiller':
            o.restore_A_path = os.path.join(m.save_dir, 'latest_net_A')
            o.restore_teacher_G_path = None
    with torch.no_grad():
        for p in b.modules.netD.parameters():
            p.add_(1.0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')      # the distiller warns that no teacher checkpoint is set
        b.load_networks(verbose=True)
    assert capsys.readouterr().out.count('Load network at') == len(nets)
    for f, net in saved.items():
        twin = {'latest_net_G.pth': b.modules.netG_student if kind == 'distiller' else b.modules.netG, 'latest_net_D.pth': b.modules.netD}.get(f)
        if twin is None:
            twin = b.modules.netAs[int(f[len('latest_net_A-')])]
        for (k, va), (_, vb) in zip(net.state_dict().items(), twin.state_dict().items()):
            assert torch.equal(va, vb), (f, k)
    # print_networks: the lines each class prints
    m.print_networks()
    out = capsys.readouterr().out
    names = ['G_student', 'G_teacher', 'D'] if kind == 'distiller' else ['G', 'D']
    assert [ln.split(']')[0] for ln in out.splitlines()] == ['[Network ' + n for n in names]


# ------------------------------------------------------------------------------------------------ one GAN-mode table
def test_gan_loss_kind_is_the_one_mode_table():
    """(kind, target) per mode x real / fake x for_discriminator, as SPADEModelModules._gan_kind returned them before GANLoss.kind replaced it."""
    from cat_amd import _lib as L
    from cat_amd.loss import GANLoss
    table = {
        ('lsgan', True, True): (L.LOSS_LSGAN, 1.0), ('lsgan', False, True): (L.LOSS_LSGAN, 0.0),
        ('lsgan', True, False): (L.LOSS_LSGAN, 1.0), ('lsgan', False, False): (L.LOSS_LSGAN, 0.0),
        ('vanilla', True, True): (L.LOSS_BCE_LOGITS, 1.0), ('vanilla', False, True): (L.LOSS_BCE_LOGITS, 0.0),
        ('vanilla', True, False): (L.LOSS_BCE_LOGITS, 1.0), ('vanilla', False, False): (L.LOSS_BCE_LOGITS, 0.0),
        ('wgangp', True, True): (L.LOSS_NEG_MEAN, 0.0), ('wgangp', False, True): (L.LOSS_MEAN, 0.0),
        ('wgangp', True, False): (L.LOSS_NEG_MEAN, 0.0), ('wgangp', False, False): (L.LOSS_MEAN, 0.0),
        ('hinge', True, True): (L.LOSS_HINGE_D_REAL, 0.0), ('hinge', False, True): (L.LOSS_HINGE_D_FAKE, 0.0),
        ('hinge', True, False): (L.LOSS_NEG_MEAN, 0.0),
    }
    for (mode, real, for_d), want in table.items():
        assert GANLoss(mode).kind(real, for_d) == want, (mode, real, for_d)
    with pytest.raises(AssertionError):
        GANLoss('hinge').kind(False, False)      # the generator never scores a fake as fake
    assert GANLoss('lsgan', 0.9, 0.1).kind(True) == (L.LOSS_LSGAN, 0.9) and GANLoss('lsgan', 0.9, 0.1).kind(False) == (L.LOSS_LSGAN, 0.1)
    from cat_amd.spade_model_modules import SPADEModelModules
    assert not hasattr(SPADEModelModules, '_gan_kind')
