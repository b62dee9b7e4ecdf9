"""CPU: the GauGAN teacher model's host-side surface -- the model factory finds SPADEModel, its option setter yields the reference's defaults
(models/spade_model.py:24-94), the loss-head entry points are in the header / the ctypes table / cat_loss_term_t's ctypes mirror, and the
golden vectors of tools/make_golden_spade_model.py load with the keys the GPU test reads."""
import argparse
import ctypes as C
import json
import os
import subprocess

import pytest

import helpers as H
from cat_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_factory_finds_the_spade_model():
    from cat_amd.models import find_model_using_name, get_option_setter
    cls = find_model_using_name('spade')
    assert cls.__name__ == 'SPADEModel'
    assert get_option_setter('spade') == cls.modify_commandline_options


def base_parser():
    """The base flags (options/base_options.py, train_options.py) that the model's option setter overrides, with the base defaults."""
    p = argparse.ArgumentParser()
    p.add_argument('--netG', type=str, default='inception_9blocks')
    p.add_argument('--netD', type=str, default='n_layers')
    p.add_argument('--ndf', type=int, default=128)
    p.add_argument('--n_layers_D', type=int, default=3)
    p.add_argument('--dataset_mode', type=str, default='aligned')
    p.add_argument('--batch_size', type=int, default=1)
    p.add_argument('--print_freq', type=int, default=100)
    p.add_argument('--save_latest_freq', type=int, default=20000)
    p.add_argument('--save_epoch_freq', type=int, default=5)
    p.add_argument('--nepochs', type=int, default=5)
    p.add_argument('--nepochs_decay', type=int, default=15)
    p.add_argument('--init_type', type=str, default='normal')
    p.add_argument('--active_fn', type=str, default='nn.ReLU')
    return p


def test_option_setter_yields_the_reference_defaults():
    from cat_amd.models import get_option_setter
    parser = get_option_setter('spade')(base_parser(), True)
    with pytest.raises(SystemExit):
        parser.parse_args([])                                   # --real_stat_path is required
    opt = parser.parse_args(['--real_stat_path', 'stat.npz'])
    want = dict(netG='inception_spade', norm_G='spadesyncbatch3x3', num_upsampling_layers='more', netD='multi_scale', ndf=64, batch_size=16,
                init_type='xavier', lambda_gan=1, lambda_feat=10, lambda_vgg=10, beta2=0.999, no_TTUR=False, nepochs=100, nepochs_decay=100,
                save_epoch_freq=10, active_fn='nn.LeakyReLU', dataset_mode='cityscapes', print_freq=50, save_latest_freq=10000000000,
                restore_G_path=None, restore_D_path=None, no_fid=False, no_mIoU=False, real_stat_path='stat.npz',
                num_D=2, norm_D='spectralinstance', n_layers_D=4)
    for k, v in want.items():
        assert getattr(opt, k) == v, (k, getattr(opt, k), v)
    # test mode: only the generator's flags
    topt = get_option_setter('spade')(base_parser(), False).parse_args([])
    assert topt.netG == 'inception_spade' and topt.norm_G == 'spadesyncbatch3x3' and not hasattr(topt, 'lambda_feat') and topt.netD == 'n_layers'


def test_loss_multi_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, 'include', 'cat_hip.h')).read()
    for name in ('cat_loss_multi_ws_bytes', 'cat_loss_multi_fwd', 'cat_loss_multi_bwd'):
        assert name + '(' in text, name
        assert name in _lib.SIGNATURES, name
    assert 'cat_loss_term_t' in text
    assert 'loss_multi.hip' in __import__('cat_amd._build', fromlist=['SOURCES']).SOURCES
    from cat_amd import ops
    assert hasattr(ops, 'MultiLossFn')


def test_loss_term_struct_matches_its_ctypes_mirror(tmp_path):
    """sizeof / offsetof of cat_loss_term_t and the table capacity as the C compiler sees include/cat_hip.h, against cat_amd/_lib.py."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cat_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(cat_loss_term_t));', '  printf("max %d\\n", CAT_LOSS_MULTI_MAX);']
    for fname, _ in _lib.LossTerm._fields_:
        lines.append(f'  printf("{fname} %zu\\n", offsetof(cat_loss_term_t, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / 'probe.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(_lib.LossTerm)
    assert int(got['max']) == _lib.LOSS_MULTI_MAX >= 16
    for fname, _ in _lib.LossTerm._fields_:
        assert int(got[fname]) == getattr(_lib.LossTerm, fname).offset, fname


def test_golden_fixture_loads_with_the_keys_the_step_test_reads():
    g = H.load('spade_model_step.npz')
    opt = json.loads(str(g['opt']))
    assert (int(g['n']), int(g['h']), int(g['w'])) == (2, 128, 256)
    assert (opt['ngf'], opt['ndf'], opt['num_D'], opt['n_layers_D'], opt['input_nc'], opt['semantic_nc']) == (8, 8, 2, 4, 5, 6)
    assert (opt['norm_G'], opt['norm_D'], opt['gan_mode'], opt['no_TTUR']) == ('spadesyncbatch3x3', 'spectralinstance', 'hinge', False)
    assert (opt['lambda_gan'], opt['lambda_feat'], opt['lambda_vgg']) == (1.0, 10.0, 10.0)
    for step in (1, 2):
        assert sorted(json.loads(str(g['losses%d' % step]))) == ['D_fake', 'D_real', 'G_feat', 'G_gan', 'G_vgg']
        for k in ('G_rm_step%d', 'G_rv_step%d', 'D_u_step%d'):
            assert g[k % step].ndim == 1
    assert g['fake_B_sub'].shape == (2, 3, 32, 64)
    for tag in ('G', 'D'):
        keys = [k for k, _ in json.loads(str(g[tag + '_shapes']))]
        probes = json.loads(str(g['probe_' + tag]))
        assert probes and set(probes) <= set(keys)
        assert float(g[tag + '_gmax']) > 0
        for k in probes:
            assert g['%s_grad/%s' % (tag, k)].shape == g['%s_after/%s' % (tag, k)].shape and float(g['%s_gnorm/%s' % (tag, k)]) >= 0
    # the running statistics a single advance would give are recorded too, and are far from the recorded (twice-advanced) ones
    assert g['G_rm_single'].shape == g['G_rm_step1'].shape and g['G_rv_single'].shape == g['G_rv_step1'].shape
    assert min(g['single_vs_double']) > 1e-2
    # the reference's own float32-vs-float64 distance in step 2 (what the step-2 bars are held against)
    assert sorted(json.loads(str(g['losses2_f32_vs_f64']))) == sorted(json.loads(str(g['losses2_f64']))) == sorted(json.loads(str(g['losses2'])))
    assert g['stats2_f32_vs_f64'].shape == (2,)
    assert os.path.getsize(os.path.join(H.GOLDEN, 'spade_model_step.npz')) < os.path.getsize(os.path.join(H.GOLDEN, 'shrink_bn.npz'))
