"""StudentRunner: inference of a (loaded) student generator on its fastest path, optionally as one hipGraph.

    runner = StudentRunner(netG, example_input, graph=True)     # inception or SPADE generator
    y = runner(x)                 # (SPADE: x is the semantic input the generator takes)
    runner.refresh()              # after weights changed (the runner also notices by itself)
    runner.latency(iters, warmup) # ms per batch, HIP events

The network is put in eval() and run under no_grad, on the fastest path that is arithmetically the general path's:
  BatchNorm blocks      the frozen fold of cat_amd/frozen.py (what evaluate_model takes already);
  InstanceNorm blocks   the fused block pipeline of cat_amd/fused_block.py, admitted in eval mode for the blocks THIS runner owns
                        (fused_block.own_eval; ~9 launches per block instead of ~55).  Networks no runner owns keep their launches.
  SPADE units           as without a runner: fused_spade admits BatchNorm units only; `spadeinstance` units stay on the per-layer path.
graph=True captures one forward at the example's shape with cat_amd.graph.capture (warm-up on a side stream, static input / output
buffers).  The graph holds raw pointers to folded / packed operands, and three things keep them good:
  * it is re-captured when optim.weights_key of the network's parameters and buffers has moved -- the rule frozen._plan follows -- or on
    refresh();
  * it is re-captured after every eager fallback of the runner itself: some operands are cached one per layer and keyed on the input
    shape too (the edge convs' packed filter streams, qconv.Layer.run), so a forward at another shape replaces them;
  * the runner keeps every cached operand that existed at the capture alive (`_pinned`), so that a forward of the same network made
    OUTSIDE the runner at another shape cannot hand memory the graph still reads back to the allocator.  What such a forward replaces
    stays valid for the captured shape as long as the weights stand; still, call refresh() after one if you can.
A call at another shape runs eagerly (and says so once).  The graph's output is a static buffer: it is valid until the next call."""
import warnings

import torch

from . import derived, fused_block, graph as cgraph, ops, optim
from .inception_modules import InvertedResidualChannels, forget_seg_pyramid


def _static_like(x):
    """An NHWC activation buffer of x's shape with zeroed padding lanes (what ops.conform builds)."""
    n, c, h, w = x.shape
    y = ops.empty_act(n, c, h, w, x.device)
    torch.as_strided(y, (n, ops.act_cs(y), h, w), y.stride()).zero_()
    y.copy_(x)
    return y


def _cached_tensors(net):
    """Every tensor reachable from a derived-operand slot (cat_amd/derived.py) of the network's modules, parameters and buffers: Entry
    values, per-mode dicts, plans and layer holders, which carry slots of their own."""
    found, seen = [], set()

    def walk(obj, depth):
        if id(obj) in seen or depth > 6 or obj is None or isinstance(obj, (str, bytes, int, float, bool, torch.nn.Module)):
            return
        seen.add(id(obj))
        if torch.is_tensor(obj):
            found.append(obj)
        elif isinstance(obj, dict):
            for v in obj.values():
                walk(v, depth + 1)
        elif isinstance(obj, (tuple, list, set, frozenset)):
            for v in obj:
                walk(v, depth + 1)
        elif type(obj).__module__.startswith('cat_amd') and hasattr(obj, '__dict__'):
            walk(vars(obj), depth + 1)

    for holder in [*net.modules(), *net.parameters(), *net.buffers()]:
        for slot in derived.SLOTS:
            walk(holder.__dict__.get(slot), 0)
    return found


class StudentRunner:
    def __init__(self, netG, *example, graph=False, warmup=3, min_tiles='auto'):
        """min_tiles: the LDS-tile threshold of the runner's own fused InstanceNorm blocks (fewest 8 x 16 output tiles at which they take
        the fused path); None keeps the package's (ops.set_tconv_min_tiles: 96; a 64 x 64 plane has 32 per sample).  That threshold keeps
        planes that cannot fill the chip off the LDS-tile kernels: right for a training step, which is throughput-bound, wrong for a
        batch-1 inference, which is launch-bound (profiles/student_infer_bench.txt).  'auto' (default): 1.  It is a property of the
        owned blocks (fused_block.own_eval): nothing process-wide changes, and the stem / head layers and BatchNorm blocks (frozen fold)
        keep the package's threshold."""
        if not example or not all(torch.is_tensor(t) for t in example):
            raise TypeError('StudentRunner(netG, example_input, ...): the example inputs are tensors')
        self.net = netG.eval()
        self.device = next(netG.parameters()).device
        if self.device.type != 'cuda':
            raise RuntimeError('StudentRunner needs the network on the GPU (HIP kernels only; there is no CPU path)')
        self.blocks = [m for m in netG.modules() if isinstance(m, InvertedResidualChannels)]
        self.min_tiles = 1 if min_tiles == 'auto' else (None if min_tiles is None else int(min_tiles))
        self.own()
        self.static_in = [_static_like(t.to(self.device, dtype=torch.float32)) for t in example]
        self.want_graph, self.warmup = bool(graph), int(warmup)
        self.graph = self.static_out = self._key = None
        self._pinned = []
        self.captures = self.replays = self.eager_calls = 0
        self._warned = False
        if self.want_graph:
            self._capture()

    # -- ownership ------------------------------------------------------------------------------------------------------------
    def own(self):
        """Take the network's blocks -- the constructor does; again after a release()."""
        for b in self.blocks:
            fused_block.own_eval(b, self.min_tiles)

    def release(self):
        """Give the network back: its eval-mode blocks take the path they took before the runner (a graph is dropped with it)."""
        for b in self.blocks:
            fused_block.disown_eval(b)
        self.graph = self.static_out = None
        self._pinned = []

    # -- the forward ----------------------------------------------------------------------------------------------------------
    def _weights_key(self):
        # the tensor OBJECTS are listed once per capture (walking the module tree per call costs more than a small graph's replay): in-place
        # changes -- optimizer steps, load_state_dict, FusedAdam re-housing the storage -- move the key; after replacing a Parameter object
        # (module.weight = nn.Parameter(...)) call refresh()
        return optim.weights_key(self._tensors)

    def _forward(self, inputs):
        if self.net.training:      # (an evaluation loop's net.train() afterwards; walking ~500 modules per call is a millisecond)
            self.net.eval()
        with torch.no_grad():
            return self.net(*inputs)

    def _capture(self):
        self.graph = self.static_out = None       # the old graph's pool goes back before the new one is recorded
        self._pinned = []
        def run(i):
            for s in self.static_in:      # (a SPADE generator caches resized copies of its input ON the input: the capture must hold the resize)
                forget_seg_pyramid(s)
            return self._forward(self.static_in)
        with torch.cuda.device(self.device):
            self.graph, self.static_out = cgraph.capture(run, max(self.warmup, 1))
        self._pinned = _cached_tensors(self.net)
        self._tensors = list(self.net.parameters()) + list(self.net.buffers())
        self._key = self._weights_key()
        self.captures += 1

    def refresh(self):
        """After weights changed, or after a forward of this network outside the runner at another shape: re-fold / re-pack (the eager
        paths do that by their own keys) and re-capture."""
        if self.want_graph:
            self._capture()

    def __call__(self, *inputs):
        if len(inputs) != len(self.static_in):
            raise TypeError('StudentRunner: %d inputs given, the example had %d' % (len(inputs), len(self.static_in)))
        if not self.want_graph or any(tuple(a.shape) != tuple(s.shape) for a, s in zip(inputs, self.static_in)):
            if self.want_graph and not self._warned:
                self._warned = True
                warnings.warn('StudentRunner: input shape %s differs from the captured %s: this call runs eagerly' %
                              ([tuple(a.shape) for a in inputs], [tuple(s.shape) for s in self.static_in]))
            self.eager_calls += 1
            if self.want_graph:
                self._key = None      # shape-keyed operands were replaced under the graph: the next call at the captured shape re-captures
            return self._forward([ops.to_nhwc(a.to(self.device, dtype=torch.float32)) for a in inputs])
        if self.graph is None or self._key is None or self._key != self._weights_key():
            self._capture()
        for a, s in zip(inputs, self.static_in):
            if a is not s:
                s.copy_(a, non_blocking=True)
        self.graph.replay()
        self.replays += 1
        return self.static_out

    def latency(self, iters=20, warmup=5):
        """Milliseconds per batch of the example's shape, by HIP events around `iters` calls."""
        for _ in range(warmup):
            self(*self.static_in)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(iters):
            self(*self.static_in)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / iters
