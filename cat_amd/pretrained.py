"""Load a compressed student checkpoint: the architecture of a released student exists only in the tensor shapes of its state_dict
(`--pretrained_student_G_path`), and the network is rebuilt from them before the weights go in.

    load_pretrained_student        utils/common.py:49-180    inception generators (pix2pix / CycleGAN students)
    load_pretrained_spade_student  utils/common.py:183-312   GauGAN students

Same order of side effects as the reference: hooks off, teacher deep-copied and re-dimensioned layer by layer from the checkpoint,
strict load_state_dict, n_macs profiled, netAs re-created at the student's trunk width, hooks back on the new modules, optimizer_G /
optimizers / schedulers rebuilt.  The branch lists of a block are read in the checkpoint's KEY ORDER (the reference iterates the
state_dict), not in sorted order.  Host-side only: nothing here launches a kernel."""
import copy
import itertools
import re

import torch
from torch import nn

from . import nn as cnn
from .optim import FusedAdam
from .prune import _clone_conv, _new_norm, _norm_cls, _norm_indices, model_profiling


def _read_checkpoint(opt):
    return torch.load(opt.pretrained_student_G_path, map_location='cpu')


def _branch_lists(state, scope, tail):
    """(channels, kernel sizes) of the keys that contain `scope` and `tail`, in the checkpoint's key order."""
    channels, kernel_sizes = [], []
    for k, v in state.items():
        if scope in k and tail in k:
            ch_, _, k_, _ = v.shape
            channels.append(ch_)
            kernel_sizes.append(k_)
    return channels, kernel_sizes


def load_pretrained_student(model, opt):
    state = _read_checkpoint(opt)
    model.remove_mapping_hook()
    cls = _norm_cls(opt)
    net = copy.deepcopy(model.netG_teacher).cpu()
    ds_idx, us_idx = _norm_indices(net.down_sampling, cls), _norm_indices(net.up_sampling, cls)
    in_channels = None
    for idx in ds_idx:
        out_channels = state[f'down_sampling.{idx}.weight'].shape[0]
        old = net.down_sampling[idx - 1]
        if in_channels is None:
            in_channels = old.in_channels
        net.down_sampling[idx] = _new_norm(opt, out_channels)
        net.down_sampling[idx - 1] = _clone_conv(old, in_channels, out_channels)
        in_channels = out_channels
    ngf_netA = in_channels
    for idx, layer in enumerate(net.features):
        layer.input_dim = in_channels
        layer.res_channels, layer.res_kernel_sizes = _branch_lists(state, f'features.{idx}.res_ops.', '.1.0.weight')
        layer.dw_channels, layer.dw_kernel_sizes = _branch_lists(state, f'features.{idx}.dw_ops.', '.2.0.weight')
        print(f'features.{idx}.res_ops', layer.res_channels, layer.res_kernel_sizes)
        print(f'features.{idx}.dw_ops', layer.dw_channels, layer.dw_kernel_sizes)
        layer.res_ops, layer.dw_ops, layer.pw_bn = layer._build()
    for idx in us_idx:
        out_channels = state[f'up_sampling.{idx}.weight'].shape[0]
        net.up_sampling[idx] = _new_norm(opt, out_channels)
        net.up_sampling[idx - 1] = _clone_conv(net.up_sampling[idx - 1], in_channels, out_channels, transposed=True)
        in_channels = out_channels
    last = net.up_sampling[-2]
    net.up_sampling[-2] = _clone_conv(last, in_channels, last.out_channels)

    net.load_state_dict(state)

    model.netG_student = net.to(model.device)
    model_profiling(model.netG_student, opt.data_height, opt.data_width)
    net_as, g_params = [], []
    for net_a in model.netAs:
        new_a = cnn.Conv2d(in_channels=ngf_netA, out_channels=net_a.out_channels, kernel_size=net_a.kernel_size).to(model.device)
        g_params.append(new_a.parameters())
        net_as.append(new_a)
    model.netAs = net_as
    model.add_mapping_hook()

    model.optimizer_G = FusedAdam([{'params': model.netG_student.parameters()}, {'params': itertools.chain(*g_params)}],
                                  lr=opt.lr, betas=(opt.beta1, 0.999))
    model.optimizers = [model.optimizer_G, model.optimizer_D]
    if model.isTrain:
        from . import networks
        model.schedulers = [networks.get_scheduler(o, opt) for o in model.optimizers]
    print('Pretrained studentG state is loaded.')


def load_pretrained_spade_student(model, opt):
    state = _read_checkpoint(opt)
    m = model.modules_on_one_gpu
    net = copy.deepcopy(m.netG_teacher).cpu()
    spade_config_str = opt.teacher_norm_G.replace('spectral', '')
    if spade_config_str.startswith('spade'):
        parsed = re.search(r'spade(\D+)(\d)x\d', spade_config_str)
        param_free_norm_type = str(parsed.group(1))
    else:
        raise NotImplementedError
    norm_layer = {'instance': cnn.InstanceNorm2d, 'batch': cnn.BatchNorm2d, 'syncbatch': cnn.SynchronizedBatchNorm2d}[param_free_norm_type]

    out_channels = state['fc.weight'].shape[0]
    net.fc = _clone_conv(net.fc, net.fc.in_channels, out_channels)
    out_channels = state['fc_norm.weight'].shape[0]
    net.fc_norm = norm_layer(out_channels, affine=True)
    ngf_stu = out_channels // 16
    in_channels = out_channels

    features = ['head_0', 'G_middle_0', 'G_middle_1'] + ['up_%d' % i for i in range(5 if opt.num_upsampling_layers == 'most' else 4)]
    for layer_name in features:
        layer = getattr(net, layer_name)
        layer.input_dim = in_channels
        out_channels = in_channels // 2 if 'up' in layer_name else in_channels
        layer.output_dim = out_channels
        # (`{name}.spade.res_ops...` does not contain `{name}.res_ops`: the block's scan never meets its SPADE's keys)
        layer.res_channels, layer.res_kernel_sizes = _branch_lists(state, f'{layer_name}.res_ops', '.0.conv.weight')
        layer.dw_channels, layer.dw_kernel_sizes = _branch_lists(state, f'{layer_name}.dw_ops', '.1.conv.weight')
        layer.spade.output_dim = layer.input_dim
        layer.spade.res_channels, layer.spade.res_kernel_sizes = _branch_lists(state, f'{layer_name}.spade.res_ops', '.0.conv.weight')
        layer.spade.dw_channels, layer.spade.dw_kernel_sizes = _branch_lists(state, f'{layer_name}.spade.dw_ops', '.1.conv.weight')
        layer.res_ops, layer.dw_ops, layer.shortcut, layer.spade = layer._build(build_only=True)
        in_channels = out_channels
    net.conv_img = _clone_conv(net.conv_img, in_channels, net.conv_img.out_channels)

    net.load_state_dict(state)

    m.netG_student = net.to(model.device)
    model_profiling(m.netG_student, opt.data_height, opt.data_width, channel=opt.data_channel)

    net_as = nn.ModuleList()
    for mapping_layer in m.mapping_layers:
        if mapping_layer != 'up_1':
            fs, ft = ngf_stu * 16, opt.teacher_ngf * 16
        else:
            fs, ft = ngf_stu * 4, opt.teacher_ngf * 4
        net_as.append(cnn.Conv2d(in_channels=fs, out_channels=ft, kernel_size=1))
    m.netAs = net_as.to(model.device)

    if opt.no_TTUR:
        beta1, beta2, g_lr = opt.beta1, opt.beta2, opt.lr
    else:
        beta1, beta2, g_lr = 0.0, 0.9, opt.lr / 2
    g_params = list(m.netG_student.parameters())
    for net_a in m.netAs:
        g_params += list(net_a.parameters())
    model.optimizer_G = FusedAdam(g_params, lr=g_lr, betas=(beta1, beta2))
    model.optimizers = [model.optimizer_G, model.optimizer_D]
    if model.isTrain:
        from . import networks
        model.schedulers = [networks.get_scheduler(o, opt) for o in model.optimizers]


def load(model, opt):
    """The dispatch of profiler.py:83-89 (and onnx_exporter.py:88-93): by the teacher's generator kind, with the reference's two asserts."""
    if 'spade' in opt.teacher_netG:
        assert 'spade' in opt.student_netG
        assert 'spade' in opt.pretrained_netG
        return load_pretrained_spade_student(model, opt)
    return load_pretrained_student(model, opt)
