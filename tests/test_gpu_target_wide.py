"""
Wide target networks on the native layers (tests/wide_cases.py): layers above 512 channels -- 1024 for squeeze-and-excitation --
which the `wide` evaluation split of DeepNets-1M reaches and the sampled training stream never does.

  1. op level against fp64 torch: the dense-convolution family with batch statistics, without a norm and with frozen statistics
     up to C_out = 4096 and C_in = 16384; the stand-alone depthwise op (depthwise_relu) up to C = 16384; squeeze-and-excitation up
     to C = 4096.  Measure, variants (buffers as the allocator hands them out / pre-filled with NaN) and the two runs for equal
     bits are those of tests/test_gpu_target_edges.py.  Tolerances: the project's gates for the convolution family (2e-4 outputs
     and statistics, 3e-4 gradients; three-piece products at K = 16384: about sqrt(K) 6e-8 = 8e-6 expected); the
     squeeze-and-excitation gates (1e-5 / 2e-5) for the depthwise op -- a sum of at most 49 fp32 products stays below 3e-6 --
     and for squeeze-and-excitation itself.
  2. module level against the stock layers (GHN3_NATIVE_OPS=0), both flavours, three norm modes: the autograd graph holds
     Depthwise + a dense-convolution node and no stock convolution / batch-norm node, running statistics move exactly as the
     stock BatchNorm moves them (same tolerance as the outputs), GHN3_NATIVE_WIDE=0 restores the stock graph.
  3. one network per flavour with 544 channels in its last stage against the stock path, without a stock Conv2d / BatchNorm2d
     call.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recipe
import target_edge_cases as E
import wide_cases as Wd
from test_gpu_target_edges import buffers, _measure, _report, _graph_nodes, _leaves, _se_reference    # noqa: F401 (`buffers`: fixture)
from test_gpu_target_edges import OUT_TOL, GRAD_TOL, SE_TOL, SE_PARAM_TOL

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


# ---- 1a. dense convolution ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_reference(row, member):
    """Inputs and the fp64 results of a CONV row for one member: (inputs, out, gradients, pre-norm result)."""
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    x, w, gamma, beta, up, rm, rv = Wd.conv_inputs(row, member)
    eps = Wd.conv_eps(row)
    ref_in = _leaves((x, w) if member == 'none' else (x, w, gamma, beta), torch.float64)
    z = F.conv2d(F.relu(ref_in[0]) if relu else ref_in[0], ref_in[1], None, st, pad, dil)
    if member == 'norm':
        ref = F.batch_norm(z, None, None, ref_in[2], ref_in[3], True, 0.1, eps)
    elif member == 'frozen':
        ref = F.batch_norm(z, rm.double(), rv.double(), ref_in[2], ref_in[3], False, 0.1, eps)
    else:
        ref = z
    (ref * up.double()).sum().backward()
    return (x, w, gamma, beta, up, rm, rv), ref.detach(), [t.grad for t in ref_in], z.detach()


@pytest.mark.parametrize('member', ['norm', 'none', 'frozen'])
@pytest.mark.parametrize('row', Wd.CONV_ROWS, ids=str)
def test_wide_conv_rows_against_fp64(row, member, buffers):
    from ghn3_amd import target_ops as T
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    (x, w, gamma, beta, up, rm, rv), ref, ref_grads, z = _conv_reference(row, member)
    var = z.var((0, 2, 3), unbiased=False)
    if member == 'norm':
        assert float(var.min()) >= E.VAR_FLOOR, float(var.min())
    runs = []
    for _ in range(2):
        dev_in = _leaves((x, w) if member == 'none' else (x, w, gamma, beta))
        stats = None
        if member == 'norm':
            assert T.ConvBn.applicable(*dev_in)
            out, stats = T.conv_bn(*dev_in, stride=st, padding=pad, dilation=dil, relu=relu, eps=Wd.conv_eps(row))
        elif member == 'none':
            assert T.ConvOnly.applicable(*dev_in)
            out = T.conv_only(*dev_in, stride=st, padding=pad, dilation=dil, relu=relu)
        else:
            assert T.ConvBnEval.applicable(*dev_in, rm.cuda(), rv.cuda(), st, pad, dil)
            out = T.conv_bn_eval(*dev_in, rm.cuda(), rv.cuda(), stride=st, padding=pad, dilation=dil, relu=relu, eps=Wd.conv_eps(row))
        assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
        (out * up.cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().cpu(), None if stats is None else stats.cpu(), [t.grad.cpu() for t in dev_in]))
    (out, stats, grads), (out2, stats2, grads2) = runs
    names = ('dx', 'dw', 'dgamma', 'dbeta')
    assert torch.equal(out2, out)
    for name, a, b in zip(names, grads, grads2):
        assert torch.equal(a, b), name
    label, worst = 'conv_' + member, {}
    _measure(label, 'out', out, ref, E.ACT_AXES, OUT_TOL, worst)
    if member == 'norm':
        assert torch.equal(stats, stats2)
        _measure(label, 'mean', stats[:Co], z.mean((0, 2, 3)), E.VEC_AXES, OUT_TOL, worst)
        _measure(label, 'var', stats[2 * Co:], var, E.VEC_AXES, OUT_TOL, worst)
    _measure(label, 'dx', grads[0], ref_grads[0], E.ACT_AXES, GRAD_TOL, worst)
    _measure(label, 'dw', grads[1], ref_grads[1], E.WGRAD_AXES, GRAD_TOL, worst)
    for name, a, b in zip(names[2:], grads[2:], ref_grads[2:]):
        _measure(label, name, a, b, E.VEC_AXES, GRAD_TOL, worst)
    _report(label, row, worst)


# ---- 1b. the stand-alone depthwise op ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dw_reference(row):
    N, C, H, W, ks, st, pad, dil = row
    x, w_dw, up = Wd.dw_inputs(row)
    ref_in = _leaves((x, w_dw), torch.float64)
    ref = F.conv2d(F.relu(ref_in[0]), ref_in[1], None, st, pad, dil, groups=C)
    (ref * up.double()).sum().backward()
    return (x, w_dw, up), ref.detach(), [t.grad for t in ref_in]


@pytest.mark.parametrize('row', Wd.DW_ROWS, ids=str)
def test_depthwise_rows_against_fp64(row, buffers):
    from ghn3_amd import target_ops as T
    N, C, H, W, ks, st, pad, dil = row
    (x, w_dw, up), ref, ref_grads = _dw_reference(row)
    runs = []
    for _ in range(2):
        dev_in = _leaves((x, w_dw))
        assert T.Depthwise.applicable(dev_in[0], dev_in[1], st, pad, dil)
        out = T.depthwise_relu(dev_in[0], dev_in[1], stride=st, padding=pad, dilation=dil)
        assert type(out.grad_fn).__name__ == 'DepthwiseBackward'
        assert len(out.grad_fn.saved_tensors) == 2                        # x and the weight: nothing else of any size is kept
        assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
        (out * up.cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().cpu(), [t.grad.cpu() for t in dev_in]))
    (out, grads), (out2, grads2) = runs
    assert torch.equal(out2, out) and torch.equal(grads2[0], grads[0]) and torch.equal(grads2[1], grads[1])
    worst = {}
    _measure('depthwise', 'out', out, ref, E.ACT_AXES, SE_TOL, worst)
    _measure('depthwise', 'dx', grads[0], ref_grads[0], E.ACT_AXES, SE_TOL, worst)
    _measure('depthwise', 'dw_dw', grads[1], ref_grads[1], E.WGRAD_AXES, SE_PARAM_TOL, worst)
    assert torch.equal(grads[0][x <= 0], torch.zeros_like(grads[0][x <= 0]))   # the ReLU's mask, exactly
    _report('depthwise', row, worst)


# ---- 1c. squeeze-and-excitation through its module -----------------------------------------------------------------------
@pytest.mark.parametrize('row', Wd.SE_ROWS, ids=str)
def test_wide_squeeze_excitation_rows_against_fp64(row, buffers):
    from ghn3_amd import ops, target_ops as T
    N, C, H, W, stride = row
    x, up, state, ref, ref_dx, ref_params = _se_reference(row)
    runs = []
    for _ in range(2):
        m = ops.ChannelSELayer(C, stride=stride)
        m.load_state_dict(state)
        m = m.cuda()
        xd = x.cuda().requires_grad_(True)
        assert T.SqueezeExcite.applicable(xd, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)
        out = m(xd)
        assert 'SqueezeExcite' in _graph_nodes(out), _graph_nodes(out)
        (out * up.cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().cpu(), xd.grad.cpu(), [p.grad.cpu() for p in m.parameters()]))
    (out, dx, params), (out2, dx2, params2) = runs
    assert torch.equal(out2, out) and torch.equal(dx2, dx) and all(torch.equal(a, b) for a, b in zip(params, params2))
    worst = {}
    _measure('se', 'out', out, ref, E.ACT_AXES, SE_TOL, worst)
    _measure('se', 'dx', dx, ref_dx, E.ACT_AXES, SE_TOL, worst)
    for a, (name, b) in zip(params, ref_params):
        _measure('se', name, a, b, E.MAT_AXES if b.dim() == 2 else E.VEC_AXES, SE_PARAM_TOL, worst)
    _report('se', row, worst)


# ---- 2. module level, both flavours, three norm modes --------------------------------------------------------------------
NATIVE = ('DepthwiseBackward', 'ConvBnBackward', 'ConvOnlyBackward', 'ConvBnEvalBackward', 'DwPwBnBackward', 'DwPwBackward',
          'DwPwBnEvalBackward')
# mode -> (the dense-convolution node behind Depthwise, the `norm` argument per flavour)
MODES = {'batch': 'ConvBnBackward', 'none': 'ConvOnlyBackward', 'eval': 'ConvBnEvalBackward'}
# module -> (Depthwise nodes, dense-convolution nodes)
NODES = {'sep_conv_520': (2, 2), 'dil_conv_12_1028': (1, 1), 'conv_1x1_1028_516': (0, 1)}


def _build(name, light, mode):
    """(module, parameter leaves, norm layers) on the GPU: seeded weights and running statistics, the same in every run."""
    from ghn3_amd import ops
    kind, args, _ = Wd.MODULES[name]
    norm = None if mode == 'none' else ('bn' if light else 'bn-track')
    torch.manual_seed(13)
    m = getattr(ops, kind + ('Light' if light else ''))(*args, norm=norm)
    gen = torch.Generator().manual_seed(17)
    if not light:
        m = m.cuda()
        leaves = list(m.parameters())
    else:
        leaves = []
        for _, sub in m.named_modules():
            for n, p in list(sub.__dict__['_parameters'].items()):
                if isinstance(p, (list, tuple)):
                    t = torch.randn(*p, generator=gen) / float(np.prod(p[1:])) ** 0.5
                    if len(p) == 1:
                        t = (1 + 0.3 * t) if n == 'weight' else 0.2 * t         # a norm layer's affine pair
                    t = t.cuda().requires_grad_(True)
                    setattr(sub, n, t)
                    leaves.append(t)
    norms = [sub for _, sub in m.named_modules() if type(sub).__name__ == 'BatchNorm2d']
    assert bool(norms) == (mode != 'none')
    for bn in norms:
        C = bn.num_features
        mean, var = 0.5 * torch.randn(C, generator=gen), 0.5 + 1.5 * torch.rand(C, generator=gen)
        if light:
            if mode == 'eval':                                 # (the light BatchNorm does not track: statistics as attributes)
                bn.running_mean, bn.running_var = mean.cuda(), var.cuda()
        else:
            with torch.no_grad():
                bn.running_mean.copy_(mean)
                bn.running_var.copy_(var)
    m.eval() if mode == 'eval' else m.train()
    return m, leaves, norms


def _run_module(name, light, mode):
    m, leaves, norms = _build(name, light, mode)
    assert leaves
    x = torch.randn(2, Wd.MODULES[name][2], 4, 4, generator=torch.Generator().manual_seed(21)).cuda().requires_grad_(True)
    assert x.is_contiguous()
    y = m(x)
    up = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).cuda()
    (y * up).sum().backward()
    torch.cuda.synchronize()
    bufs = [None if t is None else t.detach().cpu().clone() for bn in norms
            for t in (getattr(bn, 'running_mean', None), getattr(bn, 'running_var', None), getattr(bn, 'num_batches_tracked', None))]
    return y.detach().cpu(), x.grad.cpu(), [p.grad.cpu() for p in leaves], _graph_nodes(y), bufs


def _stock_graph(nodes, mode):
    return 'ConvolutionBackward0' in nodes and (mode == 'none' or 'BatchNormBackward' in nodes) and \
        not any(n in nodes for n in NATIVE)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
@pytest.mark.parametrize('name', list(Wd.MODULES))
def test_wide_blocks_run_on_the_native_nodes(name, light, mode, monkeypatch):
    monkeypatch.delenv('GHN3_NATIVE_WIDE', raising=False)
    monkeypatch.setenv('GHN3_NATIVE_OPS', '0')
    stock = _run_module(name, light, mode)
    monkeypatch.setenv('GHN3_NATIVE_OPS', '1')
    fused = _run_module(name, light, mode)
    monkeypatch.setenv('GHN3_NATIVE_WIDE', '0')
    off = _run_module(name, light, mode)
    assert _stock_graph(stock[3], mode), stock[3]
    n_dw, n_conv = NODES[name]
    assert fused[3].count('DepthwiseBackward') == n_dw and fused[3].count(MODES[mode]) == n_conv, fused[3]
    assert sum(fused[3].count(n) for n in NATIVE) == n_dw + n_conv, fused[3]
    assert 'ConvolutionBackward0' not in fused[3] and 'BatchNormBackward' not in fused[3], fused[3]
    assert _stock_graph(off[3], mode), off[3]
    assert torch.equal(off[0], stock[0])
    assert fused[0].shape == stock[0].shape
    print(name, 'light' if light else 'torch', mode, 'out %.2e dx %.2e' % (_rel(fused[0], stock[0]), _rel(fused[1], stock[1])),
          'params', ' '.join('%.2e' % _rel(a, b) for a, b in zip(fused[2], stock[2])))
    assert _rel(fused[0], stock[0]) < 2e-4
    assert _rel(fused[1], stock[1]) < 5e-4
    for a, b in zip(fused[2], stock[2]):
        assert a.shape == b.shape and _rel(a, b) < 5e-4, _rel(a, b)
    # running statistics: moved by a training-mode step exactly as the stock BatchNorm moves them, untouched in eval mode
    assert len(fused[4]) == len(stock[4])
    for a, b in zip(fused[4], stock[4]):
        assert (a is None) == (b is None)
        if a is not None and not a.is_floating_point():
            assert torch.equal(a, b)                            # num_batches_tracked
        elif a is not None and mode == 'eval':
            assert torch.equal(a, b)
        elif a is not None:
            assert _rel(a, b) < 2e-4, _rel(a, b)
    if mode == 'batch' and not light:
        assert any(a is not None and a.is_floating_point() for a in fused[4])


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
def test_wide_channel_se_layer_runs_on_the_native_node(light, monkeypatch):
    from ghn3_amd import ops

    def run():
        torch.manual_seed(5)
        m = (ops.ChannelSELayerLight if light else ops.ChannelSELayer)(2048)
        gen = torch.Generator().manual_seed(17)
        if light:
            leaves = []
            for _, sub in m.named_modules():
                for n, p in list(sub.__dict__['_parameters'].items()):
                    if isinstance(p, (list, tuple)):
                        t = (torch.randn(*p, generator=gen) / float(p[-1]) ** 0.5).cuda().requires_grad_(True)
                        setattr(sub, n, t)
                        leaves.append(t)
        else:
            m = m.cuda()
            leaves = list(m.parameters())
        x = torch.randn(2, 2048, 4, 4, generator=torch.Generator().manual_seed(21)).cuda().requires_grad_(True)
        y = m(x)
        up = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).cuda()
        (y * up).sum().backward()
        torch.cuda.synchronize()
        return y.detach().cpu(), x.grad.cpu(), [p.grad.cpu() for p in leaves], _graph_nodes(y)

    monkeypatch.delenv('GHN3_NATIVE_WIDE', raising=False)
    monkeypatch.setenv('GHN3_NATIVE_OPS', '0')
    stock = run()
    monkeypatch.setenv('GHN3_NATIVE_OPS', '1')
    fused = run()
    monkeypatch.setenv('GHN3_NATIVE_WIDE', '0')
    off = run()
    assert 'SqueezeExcite' not in stock[3] and 'SqueezeExcite' not in off[3] and fused[3].count('SqueezeExciteBackward') == 1
    assert torch.equal(off[0], stock[0])
    assert _rel(fused[0], stock[0]) < 1e-5 and _rel(fused[1], stock[1]) < 1e-5
    for a, b in zip(fused[2], stock[2]):
        assert a.shape == b.shape and _rel(a, b) < 2e-5, _rel(a, b)


# ---- 3. a whole wide network per flavour ---------------------------------------------------------------------------------
class _Calls:
    """Counts the stock convolution / batch-norm calls: the forward of the light Conv2d / BatchNorm2d modules (as
    tools/diag/stock_layer_census.py counts them) and torch.nn.functional.conv2d / batch_norm (what the torch.nn flavour ends in)."""

    def __init__(self, monkeypatch):
        from ghn3_amd import light_ops
        self.n = 0
        for attr in ('conv2d', 'batch_norm'):
            monkeypatch.setattr(F, attr, self._counted(getattr(F, attr)))
        for cls in (light_ops.Conv2d, light_ops.BatchNorm2d):
            monkeypatch.setattr(cls, 'forward', self._counted(cls.forward))

    def _counted(self, fn):
        def call(*args, **kwargs):
            self.n += 1
            return fn(*args, **kwargs)
        return call


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
def test_a_wide_network_runs_without_a_stock_convolution(light, monkeypatch):
    """C = 136 with C_mult = 2: 544 channels in the last stage, 2176 into its preprocessing layers.  Filled in and bounded as
    test_gpu_target_ops.test_networks_on_the_fused_layers_match_the_stock_path, with one difference: the stock path runs in
    float64.  Two 8 x 8 images leave 8 pixels per channel in the last stage, where a BatchNorm amplifies the rounding of what
    it reads by |z| / sigma; between two fp32 paths the worst parameter gradient then moves with the algorithms MIOpen happens to
    pick (below 2e-3 in one run and 2.1e-3 in the next, of the same tree); against float64 only the native path's own rounding
    is left and the figure is the same in every run.  (The classifier stays fp32: the network casts its input.)"""
    import network_cases
    from ghn3_amd import ops
    g = ops.Genotype(**network_cases._CONV)
    kw = dict(C=136, C_mult=2, num_classes=10, n_cells=3, is_imagenet_input=False, norm='bn')
    monkeypatch.delenv('GHN3_NATIVE_WIDE', raising=False)
    calls = _Calls(monkeypatch)
    res = {}
    for mode in ('stock', 'fused'):
        monkeypatch.setenv('GHN3_NATIVE_OPS', '0' if mode == 'stock' else '1')
        torch.manual_seed(0)
        net = (ops.NetworkLight if light else ops.Network)(genotype=g, **kw)
        dt = torch.float64 if mode == 'stock' else torch.float32
        x = torch.from_numpy(recipe.seeded_images((2, 3, 8, 8), seed=7)).cuda().to(dt)
        if light:
            table = {}
            for cell in net._layered_modules:
                table.update(cell)
            shapes = [(n, tuple(e['sz'])) for n, e in table.items()]
            params = recipe.seeded_net_params(shapes, seed=4)
            # two flat buffers: the classifier's tensors stay fp32 in every mode (the network casts its input to fp32)
            head = [n.startswith('classifier') for n, _ in shapes]
            assert any(head) and not all(head)
            leaves = []
            for is_head, dtype in ((False, dt), (True, torch.float32)):
                part = [(n, s) for (n, s), h in zip(shapes, head) if h == is_head]
                flat = torch.zeros(sum(int(np.prod(s)) for _, s in part), device='cuda', dtype=dtype, requires_grad=True)
                off = 0
                with torch.no_grad():
                    for n, s in part:
                        k = int(np.prod(s))
                        flat[off:off + k] = torch.from_numpy(params[n]).reshape(-1).cuda().to(dtype)
                        off += k
                off = 0
                for n, s in part:
                    e, k = table[n], int(np.prod(s))
                    setattr(e['module'], 'weight' if e['is_w'] else 'bias', flat[off:off + k].view(tuple(s)))
                    off += k
                leaves.append(flat)
        else:
            net = net.cuda().to(dt)
            net.classifier.float()                             # (the network casts the classifier's input to fp32)
            params = recipe.seeded_net_params([(n, tuple(p.shape)) for n, p in net.named_parameters()], seed=4)
            with torch.no_grad():
                for n, p in net.named_parameters():
                    p.copy_(torch.from_numpy(params[n]))
            leaves = [p for _, p in net.named_parameters()]
        net.train()
        torch.manual_seed(123)
        calls.n = 0
        logits, aux = net(x)
        assert aux is None
        n_calls = calls.n
        logits.square().mean().backward()
        torch.cuda.synchronize()
        res[mode] = (logits.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu() for p in leaves], n_calls)
    (l0, g0, n0), (l1, g1, n1) = res['stock'], res['fused']
    print('light' if light else 'torch', 'stock conv2d / batch_norm calls: %d on the stock path, %d native' % (n0, n1),
          'logits %.2e' % _rel(l1, l0))
    assert n0 > 0 and n1 == 0, (n0, n1)
    assert torch.isfinite(l0).all() and float(l0.norm()) > 0
    assert _rel(l1, l0) < 1e-3, _rel(l1, l0)
    worst = 0.0
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if a is not None and float(b.norm()) > 0:
            worst = max(worst, _rel(a, b))
    print('worst parameter gradient %.2e' % worst)
    assert worst < 2e-3, worst
