"""GPU: cat_loss_multi_fwd / cat_loss_multi_bwd through ops.MultiLossFn -- T mean-reduced scalar losses over unrelated NHWC tensors in one
forward call and one backward call -- against a float64 evaluation of the same inputs on the host and against ops.LossFn term by term.

Inputs are NHWC buffers whose pad lanes (channels C .. cs-1) hold 1e30: a kernel that reads them into a sum fails loudly.  Bars: 1e-6 relative
to max(1, |f64|) for the means (the bar test_gan_and_recon_losses holds; a float32 sum of <= 8192 terms in wave-tree order is good to a few
1e-7), 1e-6 relative for the gradients (one multiply per element)."""
import pytest
import torch

from oracle import detfill

pytestmark = pytest.mark.gpu

L1, LSGAN, HINGE_D_REAL, HINGE_D_FAKE, NEG_MEAN, MSE = 0, 1, 2, 3, 4, 5
# (kind, C, M as (n, h, w), has b): the forward cases, all in one call
CASES = [(L1, 8, (2, 16, 32), True),        # M 1024, 2048 quads: several workgroups
         (L1, 5, (1, 37, 1), True),         # cs 8, M 37
         (L1, 64, (3, 1, 1), True),         # M 3
         (NEG_MEAN, 1, (2, 15, 7), False),  # cs 4, M 210
         (HINGE_D_REAL, 1, (2, 15, 7), False),
         (HINGE_D_FAKE, 1, (1, 1, 1), False),
         (MSE, 3, (1, 3, 43), True)]        # M 129


def dev():
    return torch.device('cuda', 0)


def padded(x, fill=1e30):
    """NCHW host tensor -> NHWC activation on the device whose pad lanes hold `fill`."""
    n, c, h, w = x.shape
    cs = (c + 3) // 4 * 4
    buf = torch.full((n, h, w, cs), fill, dtype=torch.float32)
    buf[..., :c] = x.permute(0, 2, 3, 1)
    return buf.to(dev())[..., :c].permute(0, 3, 1, 2)


def f64_term(kind, a, b):
    """(mean, d mean / d a) in float64."""
    a = a.double().clone().requires_grad_(True)
    b = None if b is None else b.double()
    v = {L1: lambda: (a - b).abs(), MSE: lambda: (a - b) ** 2, NEG_MEAN: lambda: -a, HINGE_D_REAL: lambda: -torch.clamp(a - 1, max=0),
         HINGE_D_FAKE: lambda: -torch.clamp(-a - 1, max=0)}[kind]().mean()
    v.backward()
    return float(v), a.grad


def relerr(got, ref):
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def make_terms(cases, seed):
    host = []
    for i, (kind, c, (n, h, w), has_b) in enumerate(cases):
        a = detfill.normal((n, c, h, w), seed + 2 * i) * 1.5
        b = detfill.normal((n, c, h, w), seed + 2 * i + 1) if has_b else None
        host.append((kind, a, b))
    return host


def run_multi(host, no_grad_term=None):
    from cat_amd import ops
    spec, flat, leaves, raw = [], [], [], {}
    for t, (kind, a, b) in enumerate(host):
        ga = padded(a)
        if t != no_grad_term:
            ga.requires_grad_(True)
            ga.register_hook(lambda grad, t=t: raw.__setitem__(t, grad))      # the kernel's own buffer, before autograd re-lays it out for .grad
        leaves.append(ga)
        spec.append((kind, 0.0))
        flat += [ga, None if b is None else padded(b)]
    outs = ops.MultiLossFn.apply(tuple(spec), *flat)
    return outs, leaves, flat, raw


def test_forward_matches_float64_and_lossfn():
    from cat_amd import ops
    host = make_terms(CASES, 500)
    outs, leaves, flat, _ = run_multi(host)
    assert len(outs) == len(CASES)
    for t, (kind, a, b) in enumerate(host):
        ref, _ = f64_term(kind, a, b)
        got = float(outs[t])
        single = float(ops.LossFn.apply(flat[2 * t].detach(), flat[2 * t + 1], kind, 0.0))
        print('term %d kind %d: multi %.9g  f64 %.9g  LossFn %.9g' % (t, kind, got, ref, single))
        assert abs(got - ref) <= 1e-6 * max(1.0, abs(ref)), (t, got, ref)
        assert abs(got - single) <= 1e-6 * max(1.0, abs(ref)), (t, got, single)


def grad_buffer(g):
    """The whole [N][H][W][cs] buffer behind an activation (gradient), pad lanes included."""
    from cat_amd import ops
    n, c, h, w = g.shape
    cs = ops.act_cs(g)
    return torch.as_strided(g, (n, h, w, cs), (h * w * cs, w * cs, cs, 1))


def test_backward_matches_float64_pad_lanes_and_skips_terms_without_gradient():
    from cat_amd import ops
    host = make_terms(CASES, 600)
    skip = 1
    outs, leaves, flat, raw = run_multi(host, no_grad_term=skip)
    seeds = [torch.full((), 0.25 + 0.5 * t, device=dev()) for t in range(len(host))]
    live = [t for t in range(len(host)) if t != skip]
    before = leaves[skip].detach().clone()
    torch.autograd.backward([outs[t] for t in live], [seeds[t] for t in live])
    for t, (kind, a, b) in enumerate(host):
        if t == skip:
            assert leaves[t].grad is None and t not in raw
            continue
        _, gref = f64_term(kind, a, b)
        gref = gref * (0.25 + 0.5 * t)
        got = leaves[t].grad.detach().double().cpu()
        err = relerr(got, gref)
        print('term %d kind %d: gradient relative error %.3g' % (t, kind, err))
        assert err < 1e-6, (t, err)
        buf = grad_buffer(raw[t]).cpu()
        c = a.shape[1]
        assert buf.shape[-1] % 4 == 0 and torch.count_nonzero(buf[..., c:]) == 0       # pad lanes exactly as cat_loss_bwd leaves them
        single, cap = padded(a).requires_grad_(True), []
        single.register_hook(cap.append)
        ops.LossFn.apply(single, flat[2 * t + 1], kind, 0.0).backward(seeds[t])
        assert torch.equal(grad_buffer(cap[0]).cpu(), buf), t
    assert torch.equal(leaves[skip].detach(), before)


def test_term_without_gradient_writes_no_buffer():
    """Straight through the C ABI: the `da` of a term that needs no gradient is NULL, and a sentinel-filled buffer standing where its
    gradient would go (and its inputs) come back untouched."""
    import ctypes as C
    from cat_amd import _lib as L
    from cat_amd import ops
    host = make_terms(CASES[:3], 650)
    dev_a = [padded(a) for _, a, _ in host]
    dev_b = [padded(b) for _, _, b in host]
    das = [torch.full_like(grad_buffer(x), -7.0) for x in dev_a]
    keep = [x.clone() for x in [grad_buffer(a) for a in dev_a]]
    tab = (L.LossTerm * 3)()
    gout = torch.tensor([1.0, 2.0, 3.0], device=dev())
    seeds = (C.c_void_p * 3)()
    for t, (kind, a, _) in enumerate(host):
        n, c, h, w = a.shape
        e = tab[t]
        e.a, e.b, e.da = dev_a[t].data_ptr(), dev_b[t].data_ptr(), (None if t == 1 else das[t].data_ptr())
        e.M, e.kind, e.C, e.cs, e.target, e.scale = n * h * w, kind, c, ops.act_cs(dev_a[t]), 0.0, 1.0
        seeds[t] = gout[t].data_ptr()
    L.call('cat_loss_multi_bwd', tab, 3, seeds, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.all(das[1] == -7.0)
    assert not torch.any(das[0] == -7.0) and not torch.any(das[2] == -7.0)
    for t in range(3):
        assert torch.equal(grad_buffer(dev_a[t]), keep[t])


def test_chunking_17_terms():
    """One more term than the kernel's table holds: two chunks, same references."""
    cases = [(L1 if i % 3 else MSE, 3 + i % 4, (1, 5, 7 + i), True) for i in range(16)] + [(HINGE_D_FAKE, 1, (2, 6, 9), False)]
    host = make_terms(cases, 700)
    outs, leaves, _, _ = run_multi(host)
    assert len(outs) == 17
    torch.autograd.backward(list(outs), [torch.full((), 1.0, device=dev()) for _ in outs])
    for t, (kind, a, b) in enumerate(host):
        ref, gref = f64_term(kind, a, b)
        assert abs(float(outs[t]) - ref) <= 1e-6 * max(1.0, abs(ref)), (t, float(outs[t]), ref)
        got = leaves[t].grad.detach().double().cpu()
        assert relerr(got, gref) < 1e-6, t


def _eager(host):
    outs, leaves, _, raw = run_multi(host)
    torch.autograd.backward(list(outs), [torch.full((), 1.0 + t, device=dev()) for t in range(len(outs))])
    return torch.stack([o.detach() for o in outs]).cpu(), [grad_buffer(raw[t]).cpu().clone() for t in range(len(leaves))]


def test_two_eager_runs_are_bit_identical():
    host = make_terms(CASES, 800)
    o1, g1 = _eager(host)
    o2, g2 = _eager(host)
    assert torch.equal(o1, o2)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_graph_capture_replays_bit_identically():
    """Forward + backward captured once on one stream, replayed twice after overwriting the inputs in place: each replay equals the eager
    result for the inputs it saw, bit for bit (no host synchronisation and no device allocation inside the calls)."""
    from cat_amd import ops
    sets = [make_terms(CASES, 900), make_terms(CASES, 950)]
    eager = [_eager(h) for h in sets]
    spec = tuple((kind, 0.0) for kind, _, _ in sets[0])
    stat_a = [padded(a) for _, a, _ in sets[0]]
    stat_b = [None if b is None else padded(b) for _, _, b in sets[0]]
    seeds = [torch.full((), 1.0 + t, device=dev()) for t in range(len(spec))]

    def step():
        leaves, raw = [x.detach().requires_grad_(True) for x in stat_a], {}
        for t, x in enumerate(leaves):
            x.register_hook(lambda grad, t=t: raw.__setitem__(t, grad))
        flat = []
        for x, b in zip(leaves, stat_b):
            flat += [x, b]
        outs = ops.MultiLossFn.apply(spec, *flat)
        torch.autograd.backward(list(outs), seeds)
        return torch.stack([o.detach() for o in outs]), [grad_buffer(raw[t]) for t in range(len(leaves))]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                   # warm-up: workspace and allocator pools exist before the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        g_out, g_grads = step()
    for which in (1, 0):
        for t, (_, a, b) in enumerate(sets[which]):
            grad_buffer(stat_a[t]).copy_(grad_buffer(padded(a)))
            if b is not None:
                grad_buffer(stat_b[t]).copy_(grad_buffer(padded(b)))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_out.cpu(), eager[which][0]), which
        for t in range(len(spec)):
            assert torch.equal(g_grads[t].cpu(), eager[which][1][t]), (which, t)
