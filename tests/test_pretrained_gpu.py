"""GPU: a student loaded from a compressed checkpoint (cat_amd/pretrained.py) on the HIP kernels, and the inference runner
(cat_amd/infer.py) with the eval-mode InstanceNorm blocks on the fused pipeline.  References: the float64 eval forward of the REFERENCE's
loaded student (tests/golden/pretrained_student.npz, tools/make_golden_pretrained.py), bar 1e-3 relative (README: fp32 against the
oracle).  The inception input is 2 x 3 x 196 x 516: trunk planes 49 x 129 (odd, no multiple of the 8 x 16 tile), 126 tiles for the batch of
two -- the LDS-tile kernels' minimum is 96, so the fused / frozen block paths run -- and 63 for one sample, which they refuse: batch 1
takes the general path."""
import json
import os
import warnings
from argparse import Namespace

import numpy as np
import pytest
import torch

import helpers as H
from oracle import detfill

pytestmark = pytest.mark.gpu
G = H.load('pretrained_student.npz')
BAR = 1e-3
_CACHE = {}


def rec(tag, key):
    return json.loads(str(G[f'{tag}:{key}']))


def dev():
    return torch.device('cuda:0')


def state_dict_of(tag):
    sd = detfill.fill_state_dict(H.sd_from_shapes(G[f'{tag}:shapes']), int(G[f'{tag}:seed']))
    for k in rec(tag, 'head_keys'):      # the head conv at the recorded power of two: the closing tanh stays out of saturation
        sd[k] = sd[k] * float(G[f'{tag}:head_scale'])
    return sd


def checkpoint(tag, d):
    sd = state_dict_of(tag)
    path = os.path.join(str(d), f'{tag}_net_G.pth')
    torch.save(sd, path)
    return path


def x_of(tag):
    x = rec(tag, 'x')
    if tag.startswith('spade'):
        return (detfill.normal(tuple(x['shape']), x['seed']) > 0.8).float()
    return detfill.images(tuple(x['shape']), x['seed'])


def sub(y):
    s = rec('bn', 'x')['sub']
    return y.detach().cpu().double()[:, :, ::s, ::s].numpy()


def loaded(tag, tmp, fresh=False, **optkw):
    """(model, opt) with the checkpoint of `tag` loaded by the package's loader; cached per tag unless `fresh` (tests that change weights)."""
    if not fresh and tag in _CACHE:
        return _CACHE[tag]
    from cat_amd.distillers import create_distiller
    from cat_amd import pretrained
    o = rec(tag, 'opt')
    if tag.startswith('spade'):
        o.update(gpu_ids=[0], vgg_width_div=16, log_dir=str(tmp), isTrain=True)
        o.update(optkw)
        opt = Namespace(**o)
    else:
        kw = dict(norm=o['norm'], track=o['track'], target_flops=o['target_flops'], dataset_mode=o['dataset_mode'], gan_mode=o['gan_mode'], ndf=8,
                  log_dir=str(tmp))
        kw.update(optkw)
        opt = H.make_opt(**kw)
    opt.pretrained_student_G_path = checkpoint(tag, tmp)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')          # no teacher checkpoint: the teacher keeps its initialisation
        model = create_distiller(opt, verbose=False)
        model.setup(opt, verbose=False)
    pretrained.load(model, opt)
    if not fresh:
        _CACHE[tag] = (model, opt)
    return model, opt


def student_of(model):
    return getattr(model, 'modules_on_one_gpu', model).netG_student


def eval_forward(net, x):
    from cat_amd import ops
    net.eval()
    with torch.no_grad():
        y = net(ops.to_nhwc(x.to(dev())))
    torch.cuda.synchronize()
    return y


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp('pretrained')


# ------------------------------------------------------------------------------------------------ forward parity
@pytest.mark.parametrize('tag', ['bn', 'in', 'spade', 'bn_pruned', 'in_pruned', 'spade_pruned'])
def test_loaded_student_forward_matches_the_reference(tag, tmp):
    model, opt = loaded(tag, tmp)
    S = student_of(model)
    assert [[k, list(v.shape)] for k, v in S.state_dict().items()] == rec(tag, 'loaded_shapes') and S.n_macs == int(G[f'{tag}:n_macs'])
    assert next(S.parameters()).is_cuda
    x, want = x_of(tag), G[f'{tag}:out']
    e2 = H.rel_err(sub(eval_forward(S, x)), want)
    e1 = H.rel_err(sub(eval_forward(S, x[:1])), want[:1])          # eval mode: no statistic crosses samples in any of the three families
    print(f'{tag}: loaded student eval forward vs float64 reference: batch 2 {e2:.3e}, batch 1 {e1:.3e}')
    assert e2 < BAR and e1 < BAR


# ------------------------------------------------------------------------------------------------ the runner against the general path
class _Launches:
    """Profiler-free launch log: wraps cat_amd._lib.call (every module reaches it as an attribute of _lib) while active and records the
    entry-point names."""

    def __init__(self):
        from cat_amd import _lib
        _lib.load()
        self.lib, self.names = _lib, []

    def __enter__(self):
        real = self.real = self.lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        self.lib.call = call
        return self

    def __exit__(self, *exc):
        self.lib.call = self.real


def _launches(net, x):
    with _Launches() as log:
        eval_forward(net, x)
    return log.names


def _instance_block(track):
    import functools
    from cat_amd import nn as cnn
    from cat_amd.inception_modules import InvertedResidualChannels, get_active_fn
    nl = functools.partial(cnn.InstanceNorm2d, affine=True, track_running_stats=track)
    blk = InvertedResidualChannels(40, [7, 6, 9], [16, 5, 0], 1, [1, 3, 5], [1, 3, 5], norm_layer=nl, norm_kwargs={'momentum': 0.1, 'eps': 1e-5},
                                   active_fn=get_active_fn('nn.ReLU'))
    blk.load_state_dict(detfill.fill_state_dict(blk.state_dict(), 77))
    return blk.to(dev()).eval()


def test_runner_puts_only_its_own_instance_norm_blocks_on_the_fused_path(tmp):
    import copy
    from cat_amd import fused_block, ops
    from cat_amd.infer import StudentRunner
    model, opt = loaded('in', tmp)
    S = student_of(model)
    other = student_of(loaded('in', tmp, fresh=True)[0])      # a network no runner owns
    x, want = x_of('in'), G['in:out']
    y_general = eval_forward(S, x)
    eval_forward(other, x)                                     # (the first forward also packs filters: the logs below are steady-state ones)
    before_other, before_own = _launches(other, x), _launches(S, x)
    assert 'cat_tnorm_finalize' not in before_own             # eval mode without a runner: the general path, as before
    floor = ops._TCONV_MIN_TILES
    runner = StudentRunner(S, x, min_tiles=None)              # the package's LDS-tile threshold, so that one sample stays on the general path
    try:
        assert all(fused_block.eval_owned(b) for b in S.features)
        assert not any(fused_block.eval_owned(m) for m in other.modules())
        assert not any(fused_block.eval_owned(m) for m in copy.deepcopy(S.features[0]).modules())      # ownership does not travel with a copy
        assert _launches(other, x) == before_other            # ... and a network no runner owns issues the launches it issued before
        xg = ops.to_nhwc(x.to(dev()))
        with torch.no_grad():
            trunk = S.down_sampling(xg)
            assert all(fused_block.applicable(b, trunk) for b in S.features)
            assert not any(fused_block.applicable(b, trunk) for b in other.features)
        with torch.enable_grad():
            assert not any(fused_block.applicable(b, trunk) for b in S.features)      # grad enabled: not admitted
        y_runner = runner(x)
        torch.cuda.synchronize()
        own = _launches(S, x)
        print(f'launches of one eval forward (batch 2): general {len(before_own)}, runner {len(own)}')
        assert own.count('cat_tnorm_finalize') >= 3 * len(S.features) - 1 and len(own) < len(before_own)
        e_r, e_g = H.rel_err(sub(y_runner), want), H.rel_err(sub(y_general), want)
        mutual = H.rel_err(y_runner.cpu().numpy(), y_general.cpu().numpy())
        print(f'in: runner vs reference {e_r:.3e}, general path vs reference {e_g:.3e}, runner vs general {mutual:.3e}')
        assert e_r < BAR and e_g < BAR and mutual < BAR
        # per-sample statistics: sample 0 of the batch of two against the batch-1 run of the same image -- on the general path (one sample does
        # not fill the LDS-tile kernels) and, with the blocks' own threshold at 1, on the fused path itself
        y1_general = runner(x[:1])
        assert 'cat_tnorm_finalize' not in _launches(S, x[:1])
        for b in S.features:
            fused_block.own_eval(b, 1)
        y1_fused = runner(x[:1])
        assert _launches(S, x[:1]).count('cat_tnorm_finalize') >= 3 * len(S.features) - 1
        assert ops._TCONV_MIN_TILES == floor        # the blocks' threshold is theirs: the process-wide one never moved
        torch.cuda.synchronize()
        d_g, d_f = H.rel_err(y1_general.cpu().numpy(), y_runner[:1].cpu().numpy()), H.rel_err(y1_fused.cpu().numpy(), y_runner[:1].cpu().numpy())
        print(f'in: sample 0 of batch 2 vs batch 1: general path {d_g:.3e}, fused path {d_f:.3e} (bitwise: {bool(torch.equal(y1_fused, y_runner[:1]))})')
        assert d_g < BAR and d_f < BAR
        assert H.rel_err(sub(y1_fused), want[:1]) < BAR
    finally:
        runner.release()
    assert not any(fused_block.eval_owned(m) for m in S.modules())
    eval_forward(S, x)        # (the batch-1 runs above re-housed shape-keyed filter packs: one forward at this shape settles them again)
    assert _launches(S, x) == before_own


def test_tracked_instance_norm_and_batch_norm_stay_where_they_are(tmp):
    """The opt-in admits only norms without running statistics: a BatchNorm student keeps the frozen path, and an InstanceNorm2d with
    track_running_stats=True (eval: running statistics) is refused."""
    from cat_amd import fused_block, ops
    from cat_amd.infer import StudentRunner
    model, opt = loaded('bn', tmp)
    S = student_of(model)
    x = x_of('bn')
    eval_forward(S, x)
    before = _launches(S, x)
    runner = StudentRunner(S, x)
    try:
        assert _launches(S, x) == before and 'cat_tnorm_finalize' not in before
    finally:
        runner.release()
    tracked, plain = _instance_block(True), _instance_block(False)
    xb = ops.to_nhwc(detfill.normal((8, 40, 32, 48), 5).to(dev()))
    for b in (tracked, plain):
        fused_block.own_eval(b)
    with torch.no_grad():
        assert not fused_block.applicable(tracked, xb) and fused_block.applicable(plain, xb)
        assert not fused_block.applicable(plain, xb[:4])       # 48 tiles: under the package's threshold ...
        fused_block.own_eval(plain, 48)
        assert fused_block.applicable(plain, xb[:4])           # ... and admitted under the owner's
    fused_block.disown_eval(plain)
    with torch.no_grad():
        assert not fused_block.applicable(plain, xb)


# ------------------------------------------------------------------------------------------------ hipGraph
@pytest.mark.parametrize('tag', ['in', 'bn'])
def test_runner_graph_replays_follow_inputs_and_weights(tag, tmp):
    from cat_amd import ops
    from cat_amd.infer import StudentRunner
    model, opt = loaded(tag, tmp, fresh=True)
    assert not ops.branch_streams_enabled() or 'CAT_BRANCH_STREAMS' in os.environ      # the inception distillers' default: one stream
    S = student_of(model)
    x, want = x_of(tag), G[f'{tag}:out']
    x_b = detfill.images(tuple(x.shape), 912)
    runner = StudentRunner(S, x, graph=True)
    assert runner.min_tiles == 1
    try:
        def eager(inp):        # the same path, launched eagerly (the runner owns the blocks: eval + no_grad takes the runner's path)
            return eval_forward(S, inp).clone()

        y = runner(x).clone()
        assert runner.captures == 1 and runner.replays == 1
        assert torch.equal(y, eager(x)) and H.rel_err(sub(y), want) < BAR                  # replay == eager, bitwise
        y_b = runner(x_b).clone()
        assert torch.equal(y_b, eager(x_b)) and not torch.equal(y_b, y)                    # another input: that input's result
        assert torch.equal(runner(x), y) and runner.captures == 1
        # in-place weight change through FusedAdam.step(): the next call, with no refresh(), gives the new weights' result
        optG = model.optimizer_G
        optG.zero_grad()
        for f in optG._ensure_flat():
            f['g'].fill_(0.05)
        for grp in optG.param_groups:
            grp['lr'] = 1e-2
        optG.step()
        y_step = runner(x).clone()
        assert runner.captures == 2 and torch.equal(y_step, eager(x)) and not torch.equal(y_step, y)
        assert H.rel_err(y_step.cpu().numpy(), y.cpu().numpy()) > 1e-3                     # (the step moved every weight by ~lr)
        # ... and through load_state_dict
        S.load_state_dict(state_dict_of(tag))
        y_back = runner(x).clone()
        assert runner.captures == 3 and torch.equal(y_back, eager(x))
        assert H.rel_err(sub(y_back), want) < BAR                                          # the checkpoint's weights again: the recorded forward
        runner.refresh()
        assert runner.captures == 4 and torch.equal(runner(x), y_back)
        # another shape: eager fallback, said once
        with pytest.warns(UserWarning, match='runs eagerly'):
            y1 = runner(x[:1]).clone()
        assert runner.eager_calls == 1 and H.rel_err(sub(y1), want[:1]) < BAR
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            runner(x[:1])
        # the fallback replaced operands that are cached per layer AND per input shape (the edge convs' packed filter streams): the replay
        # after it must not read what the capture baked in -- the runner re-captures, and the result is the eager run's, bitwise
        y_after = runner(x_b).clone()
        assert runner.captures == 5 and torch.equal(y_after, eager(x_b))
        assert torch.equal(runner(x), y_back) and runner.captures == 5
        # a forward of the same network OUTSIDE the runner at another shape: the runner cannot see it, but what the graph reads is pinned
        eager(x[:1])
        torch.cuda.empty_cache()
        filler = [torch.full((1 << 18,), float('nan'), device=dev()) for _ in range(64)]      # re-use whatever the allocator got back
        assert torch.equal(runner(x_b), eager(x_b)) and runner.captures == 5
        del filler
        ms = runner.latency(iters=3, warmup=1)
        assert ms > 0 and np.isfinite(ms)
    finally:
        runner.release()


def test_runner_on_the_spade_student(tmp):
    """The GauGAN student (side-stream branches, fused SPADE units' frozen form): the runner's eager output is the plain eval forward's, the
    captured graph replays it bitwise and follows a weight change."""
    from cat_amd.infer import StudentRunner
    model, opt = loaded('spade', tmp, fresh=True)
    S = student_of(model)
    x, want = x_of('spade'), G['spade:out']
    x_b = torch.roll(x, 3, dims=3)
    y_plain = eval_forward(S, x).clone()
    runner = StudentRunner(S, x, graph=True)
    try:
        assert runner.blocks == []                                                         # no inception block in this generator: nothing to own
        y = runner(x).clone()
        assert torch.equal(y, y_plain) and H.rel_err(sub(y), want) < BAR
        assert torch.equal(runner(x_b).clone(), eval_forward(S, x_b)) and not torch.equal(runner(x_b), y)
        S.load_state_dict({k: (v * 0.5 if k == 'conv_img.weight' else v) for k, v in state_dict_of('spade').items()})
        y_half = runner(x).clone()
        assert runner.captures == 2 and torch.equal(y_half, eval_forward(S, x)) and not torch.equal(y_half, y)
        with pytest.warns(UserWarning, match='runs eagerly'):
            y1 = runner(x[:1]).clone()
        assert torch.equal(y1, eval_forward(S, x[:1]))
        assert torch.equal(runner(x), y_half) and runner.captures == 3
    finally:
        runner.release()


# ------------------------------------------------------------------------------------------------ continue distilling, evaluate
def _snapshot(nets):
    return [p.detach().clone() for net in nets for p in net.parameters()]


def test_distilling_continues_from_the_loaded_student(tmp, tmp_path):
    # (the BatchNorm student: its convs carry no bias.  A conv bias in front of an InstanceNorm has an identically zero gradient and Adam
    # leaves it where it is, so "every parameter moved" is a statement about the BatchNorm family)
    model, opt = loaded('bn', tmp, fresh=True, distill_G_loss_type='mse', log_dir=str(tmp_path))
    S, T = model.netG_student, model.netG_teacher
    s0, a0, t0 = _snapshot([S]), _snapshot(model.netAs), _snapshot([T])
    S.train()
    for step in range(2):
        model.set_input({'A': detfill.images((2, 3, 64, 64), 930 + step), 'B': detfill.images((2, 3, 64, 64), 940 + step), 'A_paths': [], 'B_paths': []})
        model.optimize_parameters(step)
        losses = model.get_current_losses()
        assert losses and all(np.isfinite(v) for v in losses.values()), losses
    torch.cuda.synchronize()
    assert all(not torch.equal(a, b) for a, b in zip(s0, _snapshot([S])))                  # every student parameter moved,
    assert all(not torch.equal(a, b) for a, b in zip(a0, _snapshot(model.netAs)))          # every netA parameter moved,
    assert all(torch.equal(a, b) for a, b in zip(t0, _snapshot([T])))                      # the teacher did not
    model.save_networks('latest')
    saved = {k: v.clone() for k, v in S.state_dict().items()}
    with torch.no_grad():
        for p in S.parameters():
            p.add_(1.0)
    opt.restore_student_G_path = os.path.join(model.save_dir, 'latest_net_G.pth')
    opt.restore_A_path = os.path.join(model.save_dir, 'latest_net_A')
    opt.restore_D_path = os.path.join(model.save_dir, 'latest_net_D.pth')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model.load_networks(verbose=False)
    assert list(S.state_dict()) == list(saved) and all(torch.equal(v.cpu(), saved[k].cpu()) for k, v in S.state_dict().items())
    assert [[k, list(v.shape)] for k, v in torch.load(opt.restore_student_G_path).items()] == rec('bn', 'loaded_shapes')


def test_evaluate_model_on_the_loaded_student(tmp, tmp_path):
    model, opt = loaded('bn', tmp, fresh=True, log_dir=str(tmp_path))
    opt.eval_batch_size = 2
    sizes = (2, 1)                                                                         # the last batch is ragged
    model.eval_dataloader = [{'A': detfill.images((n, 3, 64, 64), 950 + i), 'B': detfill.images((n, 3, 64, 64), 960 + i),
                              'A_paths': ['/d/e%d_%d.png' % (i, j) for j in range(n)], 'B_paths': ['/d/e%d_%d.png' % (i, j) for j in range(n)]}
                             for i, n in enumerate(sizes)]
    seen = []
    model.fid_fn = lambda fakes: seen.append([tuple(f.shape) for f in fakes]) or 7.0
    ret = model.evaluate_model(0, save_image=True)
    assert list(ret) == ['metric/fid', 'metric/fid-mean', 'metric/fid-best'] and ret['metric/fid'] == 7.0
    assert seen == [[(2, 3, 64, 64), (1, 3, 64, 64)]]
    assert sorted(os.listdir(os.path.join(str(tmp_path), 'eval', '0', 'Sfake'))) == ['e0_0.png', 'e0_1.png', 'e1_0.png']
