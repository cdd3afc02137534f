"""
Target-network blocks whose BatchNorm normalises with RUNNING statistics (a tracking BatchNorm in eval mode) on the native HIP
layers: target_ops.conv_bn_eval (ghn3_conv_frozen_fwd / _bwd) and target_ops.dwpw_bn_eval (ghn3_dwpw_frozen_fwd / _bwd).

  1. op level against torch in fp64 at the edge rows of tests/target_edge_cases.py -- out, dx, the weight gradients, dgamma, dbeta
     under tests/util_parity.slice_errors, 2e-4 / 3e-4 (the project's bounds for these two families) --, twice for equal bits,
     and once more with NaN-filled buffers;
  2. exact properties: a zero gamma, no_grad against grad mode, untouched statistics;
  3. the batch-statistics members' own statistics fed back as running statistics reproduce their output;
  4. every block of the search space in eval mode, both flavours, against the same module on the stock layers, with the new
     nodes -- and no stock convolution or batch-norm node -- in its autograd graph; GHN3_NATIVE_EVALBN=0 restores the stock graph;
  5. whole default-norm networks in eval mode, fused against stock, with no call of F.conv2d / F.batch_norm on the fused path.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recipe
import target_edge_cases as E
from util_parity import slice_errors

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = 2e-4, 3e-4
EPS = 1e-5

DENSE_ROWS = E.CONV_ROWS + [E.CONV_ONLY_ROWS[-1]]            # (the last one: a single output pixel, which batch statistics cannot have)
BIG_DENSE = (len(E.CONV_ROWS) - 2, len(E.CONV_ROWS) - 1)     # 0.59 M and 1.1 M activations: not run with NaN-filled buffers


class _GarbageTorch:
    """Stands in for the `torch` global of ghn3_amd.target_ops: every buffer the ops allocate (outputs, gradients, scratch)
    starts as NaN instead of whatever the allocator holds."""

    def __init__(self):
        self.spoiled = 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def _spoil(self, t):
        self.spoiled += 1
        return t.fill_(float('nan') if t.is_floating_point() else 255)

    def empty(self, *args, **kw):
        return self._spoil(torch.empty(*args, **kw))

    def empty_like(self, *args, **kw):
        return self._spoil(torch.empty_like(*args, **kw))


@pytest.fixture
def buffers(request, monkeypatch):
    """The op's buffers as the caching allocator hands them out ('allocator'), or pre-filled with NaN ('nan-filled')."""
    if request.param == 'allocator':
        yield None
        return
    from ghn3_amd import target_ops as T
    proxy = _GarbageTorch()
    monkeypatch.setattr(T, 'torch', proxy)
    yield proxy
    assert proxy.spoiled >= 2, 'the ops no longer allocate through torch.empty / empty_like: the variant checks nothing'


def _variants(n_rows, allocator_only=()):
    return [pytest.param(k, v, id='%d-%s' % (k, v)) for k in range(n_rows) for v in ('allocator', 'nan-filled')
            if not (v == 'nan-filled' and k in allocator_only)]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _graph_nodes(t):
    """Names of the autograd nodes between t and its leaves."""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo += [f for f, _ in fn.next_functions]
    return names


def _running_stats(k, C_out):
    """Seeded running statistics of row index k (dense rows: k; dwpw rows: 100 + k; pointwise rows: 200 + k)."""
    g = torch.Generator().manual_seed(4242 + k)
    return 0.5 * torch.randn(C_out, generator=g), 0.5 + 1.5 * torch.rand(C_out, generator=g)


# ---- 1. op level, against fp64 torch ---------------------------------------------------------------------------------------
# family -> (inputs of row k as a dict, the convolution's arguments): x, weights, gamma, beta, up on the CPU in fp32
def _case(family, k):
    if family == 'dense':
        row = DENSE_ROWS[k]
        x, w, gamma, beta, up = E.conv_inputs(row)
        cfg = dict(stride=row[6], padding=row[7], dilation=row[8], relu=row[9])
        weights, seed = {'w': w}, k
    elif family == 'dwpw':
        row = E.DWPW_ROWS[k]
        x, w_dw, w_pw, gamma, beta, up = E.dwpw_inputs(row)
        cfg = dict(stride=row[6], padding=row[7], dilation=row[8])
        weights, seed = {'w_dw': w_dw, 'w_pw': w_pw}, 100 + k
    else:
        row = E.PW_ROWS[k]
        x, w_pw, gamma, beta, up = E.pw_inputs(row)
        cfg = dict(stride=row[5], padding=0, dilation=1)
        weights, seed = {'w_pw': w_pw}, 200 + k
    rm, rv = _running_stats(seed, gamma.numel())
    return dict(x=x, **weights, gamma=gamma, beta=beta), (rm, rv), up, cfg


def _stock(family, t, rm, rv, cfg, eps=EPS):
    """The stock expression in the dtype of its inputs."""
    x = t['x']
    if family == 'dense':
        z = F.conv2d(F.relu(x) if cfg['relu'] else x, t['w'], None, cfg['stride'], cfg['padding'], cfg['dilation'])
    elif family == 'dwpw':
        y = F.conv2d(F.relu(x), t['w_dw'], None, cfg['stride'], cfg['padding'], cfg['dilation'], groups=x.shape[1])
        z = F.conv2d(y, t['w_pw'])
    else:
        z = F.conv2d(F.relu(x), t['w_pw'], None, cfg['stride'])
    return F.batch_norm(z, rm, rv, t['gamma'], t['beta'], False, 0.1, eps)


@functools.lru_cache(maxsize=None)
def _reference(family, k):
    """(inputs, statistics, upstream gradient, arguments, fp64 output, fp64 gradients by name): computed once per row."""
    t, (rm, rv), up, cfg = _case(family, k)
    leaves = {n: v.clone().double().requires_grad_(True) for n, v in t.items()}
    ref = _stock(family, leaves, rm.double(), rv.double(), cfg)
    (ref * up.double()).sum().backward()
    return t, (rm, rv), up, cfg, ref.detach(), {n: v.grad for n, v in leaves.items()}


def _native(family, dev, rm, rv, cfg, eps=EPS):
    from ghn3_amd import target_ops as T
    if family == 'dense':
        assert T.ConvBnEval.applicable(dev['x'], dev['w'], dev['gamma'], dev['beta'], rm, rv, cfg['stride'], cfg['padding'],
                                       cfg['dilation'])
        return T.conv_bn_eval(dev['x'], dev['w'], dev['gamma'], dev['beta'], rm, rv, cfg['stride'], cfg['padding'], cfg['dilation'],
                              relu=cfg['relu'], eps=eps)
    w_dw = dev.get('w_dw')
    assert T.DwPwBnEval.applicable(dev['x'], w_dw, dev['w_pw'], dev['gamma'], dev['beta'], rm, rv,
                                   1 if w_dw is None else w_dw.shape[-1])
    return T.dwpw_bn_eval(dev['x'], w_dw, dev['w_pw'], dev['gamma'], dev['beta'], rm, rv, cfg['stride'], cfg['padding'],
                          cfg['dilation'], eps=eps)


NODE = {'dense': 'ConvBnEvalBackward', 'dwpw': 'DwPwBnEvalBackward', 'pw': 'DwPwBnEvalBackward'}
AXES = dict(x=E.ACT_AXES, w=E.WGRAD_AXES, w_dw=E.WGRAD_AXES, w_pw=E.WGRAD_AXES, gamma=E.VEC_AXES, beta=E.VEC_AXES)


def _run(family, t, rm, rv, up, cfg):
    """One forward + backward on the GPU: (out, gradients by name) on the CPU, and the statistics as the op left them."""
    dev = {n: v.cuda().requires_grad_(True) for n, v in t.items()}
    rmd, rvd = rm.cuda(), rv.cuda()
    out = _native(family, dev, rmd, rvd, cfg)
    assert type(out.grad_fn).__name__ == NODE[family]
    assert out.is_contiguous(memory_format=torch.channels_last)
    (out * up.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)          # constants: never written
    return out.detach().cpu(), {n: v.grad.cpu() for n, v in dev.items()}


def _check_row(family, k):
    t, (rm, rv), up, cfg, ref, ref_grads = _reference(family, k)
    (out, grads), (out2, grads2) = _run(family, t, rm, rv, up, cfg), _run(family, t, rm, rv, up, cfg)
    assert torch.equal(out2, out)                                   # deterministic: the same bits again,
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), n                  # ... the fixed-order reductions of the gradients included
    assert out.shape == ref.shape, (out.shape, ref.shape)
    v, where = slice_errors(out, ref, E.ACT_AXES)
    print('%s row %d out per-slice error %.2e' % (family, k, v))
    assert v <= OUT_TOL, (family, k, 'out', v, where)
    for n, got in grads.items():
        assert got.shape == ref_grads[n].shape, (n, got.shape)
        v, where = slice_errors(got, ref_grads[n], AXES[n])
        print('%s row %d d%s per-slice error %.2e' % (family, k, n, v))
        assert v <= GRAD_TOL, (family, k, 'd' + n, v, where)


@pytest.mark.parametrize('k,buffers', _variants(len(DENSE_ROWS), BIG_DENSE), indirect=['buffers'])
def test_conv_bn_eval_rows_against_fp64(k, buffers):
    _check_row('dense', k)


@pytest.mark.parametrize('k,buffers', _variants(len(E.DWPW_ROWS)), indirect=['buffers'])
def test_dwpw_bn_eval_rows_against_fp64(k, buffers):
    _check_row('dwpw', k)


@pytest.mark.parametrize('k,buffers', _variants(len(E.PW_ROWS)), indirect=['buffers'])
def test_pointwise_bn_eval_rows_against_fp64(k, buffers):
    _check_row('pw', k)


def test_applicable_mirrors_the_limits_of_the_c_side():
    from ghn3_amd import target_ops as T, _lib as L
    c = lambda *s: torch.empty(*s, device='cuda')
    x, w = c(1, 8, 4, 4), c(12, 8, 3, 3)
    g, b, rm, rv = c(12), c(12), c(12), c(12)
    assert T.ConvBnEval.applicable(x, w, g, b, rm, rv, 1, 1, 1)
    assert not T.ConvBnEval.applicable(x, w, g, b, None, rv, 1, 1, 1)                  # a missing statistic
    assert not T.ConvBnEval.applicable(x, w, g, b, rm, c(8), 1, 1, 1)                  # ... or one of another length
    assert not T.ConvBnEval.applicable(x, w, g, b, rm.double(), rv, 1, 1, 1)
    assert not T.ConvBnEval.applicable(x, w, g, b, rm.cpu(), rv, 1, 1, 1)
    assert not T.ConvBnEval.applicable(c(1, 6, 4, 4), c(12, 6, 3, 3), g, b, rm, rv, 1, 1, 1)   # C_in % 4
    # output pixels x C_out = 2^31 (a padded 1 x 1 kernel: 2048 x 2048 outputs of a 2046 x 2046 image) while input pixels x C_out
    # and x.numel() stay below: check_cdesc's second rule alone
    xl, wl = c(1, 4, 2046, 2046), c(512, 4, 1, 1)
    big = [c(512) for _ in range(4)]
    assert T.ConvBn.applicable(xl, wl, big[0], big[1])
    assert T.ConvBnEval.applicable(xl, wl, *big, 1, 0, 1)
    assert not T.ConvBnEval.applicable(xl, wl, *big, 1, 1, 1)
    assert not T.ConvBnEval.applicable(c(1, 4, 2048, 2048), wl, *big, 2, 0, 1)         # the first rule: input pixels x C_out
    lib = L.load()
    for pad, want in ((0, True), (1, False)):                                          # the C side agrees
        d = T._conv_desc(xl, wl, 1, pad, 1, True, 1e-5)
        assert (int(lib.ghn3_conv_frozen_scratch_floats(ctypes.byref(d), 0)) >= 0) == want
    xd, wd, wp = c(1, 8, 4, 4), c(8, 1, 3, 3), c(12, 8)
    assert T.DwPwBnEval.applicable(xd, wd, wp, g, b, rm, rv, 3)
    assert not T.DwPwBnEval.applicable(xd, wd, wp, g, b, rm, None, 3)
    assert not T.DwPwBnEval.applicable(xd, wd, wp, g, b, rm.half(), rv, 3)
    assert not T.DwPwBnEval.applicable(xd, wd, c(10, 8), c(10), c(10), c(10), c(10), 3)    # C_out % 4
    dn = T._conv_desc(x, w, 1, 1, 1, True, 1e-5, no_norm=True)                         # GHN3_CONV_NO_NORM has no meaning here
    out = c(1, 12, 4, 4)
    scratch = c(int(L.load().ghn3_conv_frozen_scratch_floats(ctypes.byref(dn), 0)))
    with pytest.raises(L.Ghn3Error):
        L._check(L.load().ghn3_conv_frozen_fwd(ctypes.byref(dn), x.data_ptr(), w.data_ptr(), g.data_ptr(), b.data_ptr(),
                                               rm.data_ptr(), rv.data_ptr(), None, out.data_ptr(), scratch.data_ptr(), None),
                 'ghn3_conv_frozen_fwd')


# ---- 2. exact properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family', ['dense', 'dwpw'])
def test_a_zero_gamma_silences_its_channel_exactly(family):
    t, (rm, rv), up, cfg = _case(family, 0)
    ch = 19
    t = dict(t, gamma=t['gamma'].clone())
    t['gamma'][ch] = 0.0
    out, grads = _run(family, t, rm, rv, up, cfg)
    assert torch.equal(out[:, ch], t['beta'][ch].expand_as(out[:, ch]))
    assert bool(torch.isfinite(grads['gamma'][ch]))
    up0 = up.clone()
    up0[:, ch] = 0.0
    _, grads0 = _run(family, t, rm, rv, up0, cfg)
    assert float(grads['x'].abs().max()) > 0
    assert torch.equal(grads['x'], grads0['x'])                      # the channel's upstream gradient reaches dx nowhere
    for n in t:
        if n.startswith('w'):
            assert torch.equal(grads[n], grads0[n]), n


@pytest.mark.parametrize('family', ['dense', 'dwpw'])
def test_no_grad_output_equals_the_grad_mode_output_and_saves_nothing(family, monkeypatch):
    from ghn3_amd import target_ops as T
    t, (rm, rv), up, cfg = _case(family, 0)
    proxy = _GarbageTorch()
    monkeypatch.setattr(T, 'torch', proxy)
    dev = {n: v.cuda().requires_grad_(True) for n, v in t.items()}
    rmd, rvd = rm.cuda(), rv.cuda()
    out = _native(family, dev, rmd, rvd, cfg)
    with_grad = proxy.spoiled
    with torch.no_grad():
        quiet = _native(family, dev, rmd, rvd, cfg)
    without = proxy.spoiled - with_grad
    frozen = _native(family, {n: v.detach() for n, v in dev.items()}, rmd, rvd, cfg)   # grad mode on, nothing to differentiate
    assert quiet.grad_fn is None and frozen.grad_fn is None and out.grad_fn is not None
    assert torch.equal(quiet, out) and torch.equal(frozen, out)
    assert without == with_grad - 1, (with_grad, without)            # the pre-norm tensor z is not even allocated
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)


# ---- 3. against the batch-statistics members -------------------------------------------------------------------------------
@pytest.mark.parametrize('family,k', [('dense', 0), ('dense', 2), ('dense', 9), ('dwpw', 0), ('dwpw', 4)])
def test_the_batch_members_own_statistics_reproduce_their_output(family, k):
    from ghn3_amd import target_ops as T
    t, _, _, cfg = _case(family, k)
    dev = {n: v.cuda() for n, v in t.items()}
    C = t['gamma'].numel()
    with torch.no_grad():
        if family == 'dense':
            want, stats = T.conv_bn(dev['x'], dev['w'], dev['gamma'], dev['beta'], cfg['stride'], cfg['padding'], cfg['dilation'],
                                    relu=cfg['relu'], eps=EPS)
        else:
            want, stats = T.dwpw_bn(dev['x'], dev['w_dw'], dev['w_pw'], dev['gamma'], dev['beta'], cfg['stride'], cfg['padding'],
                                    cfg['dilation'], eps=EPS)
        got = _native(family, dev, stats[:C].clone(), stats[2 * C:].clone(), cfg)      # mean and BIASED variance
    v, where = slice_errors(got.cpu(), want.cpu(), E.ACT_AXES)
    print('%s row %d frozen against batch statistics %.2e' % (family, k, v))
    assert v <= 1e-5, (v, where)


# ---- 4. module level, both flavours ----------------------------------------------------------------------------------------
def _stems():
    from ghn3_amd import ops
    plan = dict(C=16, num_classes=10, n_steps=2, n_cells=3, ks=3, is_imagenet_input=False, imagenet_stride=4, is_vit=False,
                preproc=True, C_mult=2, fc_layers=1, fc_dim=0, glob_avg=True, multiplier=(2, 2))
    simple = ops.network_plan(stem_pool=True, stem_type=0, **plan)['stems']
    two = ops.network_plan(stem_pool=False, stem_type=1, **plan)['stems']
    return {'stem': simple['stem'], 'stem0': two['stem0'], 'stem1': two['stem1']}


# name -> (constructor name, arguments, input channels, {native node: how many of it})
BLOCKS = {
    'dil_conv_3x3_s2': ('DilConv', (12, 16, 3, 2, 2, 2), 12, {'DwPwBnEvalBackward': 1}),
    'sep_conv_5x5': ('SepConv', (12, 16, 5, 1, 2), 12, {'DwPwBnEvalBackward': 2}),
    'conv_1x1_s2': ('ReLUConvBN', (12, 16, 1, 2, 0), 12, {'DwPwBnEvalBackward': 1}),
    'conv_3x3': ('ReLUConvBN', (8, 16, 3, 1, 1), 8, {'ConvBnEvalBackward': 1}),
    'conv_1x7_7x1_s2': ('ReLUConvBN', (12, 12, 7, 2, 3), 12, {'ConvOnlyBackward': 1, 'ConvBnEvalBackward': 1}),
    'factorized_reduce': ('FactorizedReduce', (12, 16), 12, {'ConvBnEvalBackward': 1}),
    'stem': ('seq', 'stem', 3, {'ConvBnEvalBackward': 1}),
    'stem0': ('seq', 'stem0', 3, {'ConvBnEvalBackward': 2}),
    'stem1': ('seq', 'stem1', 16, {'ConvBnEvalBackward': 1}),
}
NATIVE_NODES = ('DwPwBnEvalBackward', 'ConvBnEvalBackward', 'ConvOnlyBackward', 'DwPwBnBackward', 'ConvBnBackward')


def _norm_layers(m):
    return [sub for _, sub in m.named_modules() if type(sub).__name__ == 'BatchNorm2d']


def _build(name, light):
    """(module in eval mode, its parameter leaves, its norm layers) on the GPU: seeded weights and seeded running statistics,
    the same in every mode.  The torch.nn flavour is built with 'bn-track'; the light flavour's BatchNorm refuses to track, so
    it is built with 'bn' and given the statistics as attributes.  (Both flavours get seeded statistics: the initial mean 0 /
    variance 1 of a tracking BatchNorm would hide a swapped pair.)"""
    from ghn3_amd import ops
    kind, args = BLOCKS[name][:2]
    norm = 'bn' if light else 'bn-track'
    torch.manual_seed(13)
    if kind == 'seq':
        m = ops._layer_seq(ops._LightLayers if light else ops._TorchLayers, norm, _stems()[args])
    else:
        kw = dict(norm=norm, double=True) if name.startswith('conv_1x7') else dict(norm=norm)
        m = getattr(ops, kind + ('Light' if light else ''))(*args, **kw)
    gen = torch.Generator().manual_seed(17)
    if not light:
        m = m.cuda()
        leaves = list(m.parameters())
    else:
        leaves = []
        for _, sub in m.named_modules():
            for n, p in list(sub.__dict__['_parameters'].items()):
                if isinstance(p, (list, tuple)):
                    t = (torch.randn(*p, generator=gen) / float(np.prod(p[1:])) ** 0.5).cuda().requires_grad_(True)
                    setattr(sub, n, t)
                    leaves.append(t)
    norms = _norm_layers(m)
    assert norms
    for bn in norms:
        C = bn.num_features
        mean, var = 0.5 * torch.randn(C, generator=gen), 0.5 + 1.5 * torch.rand(C, generator=gen)
        if light:
            bn.running_mean, bn.running_var = mean.cuda(), var.cuda()
        else:
            with torch.no_grad():
                bn.running_mean.copy_(mean)
                bn.running_var.copy_(var)
    m.eval()
    return m, leaves, norms


def _buffers_of(norms):
    return [None if t is None else t.detach().cpu().clone()
            for bn in norms for t in (bn.running_mean, bn.running_var, getattr(bn, 'num_batches_tracked', None))]


def _run_block(name, light):
    from ghn3_amd import ops
    m, leaves, norms = _build(name, light)
    assert leaves
    before = _buffers_of(norms)
    x0 = torch.randn(4, BLOCKS[name][2], 8, 8, generator=torch.Generator().manual_seed(21)).cuda().requires_grad_(True)
    x = x0 * 1.0                                               # (a non-leaf: stem1's in-place ReLU rewrites it)
    y = ops.Network._run_stem(m, x) if BLOCKS[name][0] == 'seq' else m(x)
    up = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).cuda()
    ((y * up).sum() + (x * x).sum()).backward()                # (x enters the loss AFTER the block: sees an in-place ReLU)
    torch.cuda.synchronize()
    for a, b in zip(before, _buffers_of(norms)):               # running_mean, running_var, num_batches_tracked: bit-unchanged
        assert (a is None and b is None) or torch.equal(a, b)
    return y.detach().cpu(), x.detach().cpu(), x0.grad.cpu(), [p.grad.cpu() for p in leaves], _graph_nodes(y)


def _stock_graph(nodes):
    return 'ConvolutionBackward0' in nodes and any('BatchNormBackward' in n for n in nodes) and \
        not any(n in nodes for n in NATIVE_NODES)


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
@pytest.mark.parametrize('name', list(BLOCKS))
def test_eval_mode_blocks_run_on_the_native_nodes(name, light, monkeypatch):
    want = BLOCKS[name][3]
    monkeypatch.setenv('GHN3_NATIVE_EVALBN', '1')
    monkeypatch.setenv('GHN3_NATIVE_OPS', '0')
    stock = _run_block(name, light)
    monkeypatch.setenv('GHN3_NATIVE_OPS', '1')
    fused = _run_block(name, light)
    monkeypatch.setenv('GHN3_NATIVE_EVALBN', '0')
    off = _run_block(name, light)
    assert _stock_graph(stock[4]), stock[4]
    for node, count in want.items():
        assert fused[4].count(node) == count, (node, fused[4])
    assert sum(fused[4].count(n) for n in NATIVE_NODES) == sum(want.values()), fused[4]
    assert 'ConvolutionBackward0' not in fused[4] and not any('BatchNormBackward' in n for n in fused[4]), fused[4]
    assert _stock_graph(off[4]), off[4]
    assert torch.equal(off[0], stock[0])
    assert fused[0].shape == stock[0].shape
    print(name, 'light' if light else 'torch', 'out %.2e dx %.2e' % (_rel(fused[0], stock[0]), _rel(fused[2], stock[2])),
          'params', ' '.join('%.2e' % _rel(a, b) for a, b in zip(fused[3], stock[3])))
    assert _rel(fused[0], stock[0]) < 2e-4
    assert torch.equal(fused[1], stock[1])                     # what an in-place ReLU left in the caller's tensor
    assert _rel(fused[2], stock[2]) < 5e-4
    for a, b in zip(fused[3], stock[3]):
        assert a.shape == b.shape and _rel(a, b) < 5e-4, _rel(a, b)


# ---- 5. whole networks, torch.nn flavour -----------------------------------------------------------------------------------
def _network_cases():
    import network_cases
    return {'conv': (network_cases._CONV, dict(C=8, num_classes=10, n_cells=3, is_imagenet_input=False)),
            'plain': (network_cases._PLAIN, dict(C=8, num_classes=10, n_cells=3, is_imagenet_input=False, preproc=False, C_mult=1))}


class _Calls:
    """Counts the calls of torch.nn.functional.conv2d / batch_norm (what every stock Conv2d / BatchNorm2d of either flavour ends in)."""

    def __init__(self, monkeypatch):
        self.n = 0
        for attr in ('conv2d', 'batch_norm'):
            monkeypatch.setattr(F, attr, self._counted(getattr(F, attr)))

    def _counted(self, fn):
        def call(*args, **kwargs):
            self.n += 1
            return fn(*args, **kwargs)
        return call


@pytest.mark.parametrize('case', ['conv', 'plain'])
def test_default_norm_networks_in_eval_mode_run_without_a_stock_layer(case, monkeypatch):
    """Bounds as test_gpu_target_nonorm.test_bn_free_networks_run_without_a_stock_convolution."""
    from ghn3_amd import ops
    geno, kw = _network_cases()[case]
    g = ops.Genotype(**geno)
    x = torch.from_numpy(recipe.seeded_images((4, 3, 32, 32), seed=7)).cuda()

    def fresh():
        torch.manual_seed(0)
        net = ops.Network(genotype=g, **kw).cuda()
        params = recipe.seeded_net_params([(n, tuple(p.shape)) for n, p in net.named_parameters()], seed=len(case))
        with torch.no_grad():
            for n, p in net.named_parameters():
                p.copy_(torch.from_numpy(params[n]))
        return net

    # running statistics: two training-mode forwards on the stock path
    monkeypatch.setenv('GHN3_NATIVE_OPS', '0')
    net = fresh().train()
    with torch.no_grad():
        net(x)
        net(x.flip(0) * 0.5)
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    assert any(k.endswith('running_var') and float((v - 1).abs().max()) > 0 for k, v in state.items())

    calls = _Calls(monkeypatch)
    res = {}
    for mode, (native, evalbn) in dict(stock=('0', '1'), fused=('1', '1'), off=('1', '0')).items():
        monkeypatch.setenv('GHN3_NATIVE_OPS', native)
        monkeypatch.setenv('GHN3_NATIVE_EVALBN', evalbn)
        net = fresh()
        net.load_state_dict(state)
        net.eval()
        calls.n = 0
        logits, aux = net(x)
        assert aux is None
        n_calls = calls.n
        logits.square().mean().backward()
        with torch.no_grad():
            quiet = net(x)[0]
        torch.cuda.synchronize()
        if mode == 'fused':
            assert quiet.grad_fn is None and torch.equal(quiet, logits)
        after = net.state_dict()
        for k, v in state.items():
            if 'running_' in k or 'num_batches' in k:
                assert torch.equal(after[k], v), k
        res[mode] = (logits.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu() for p in net.parameters()], n_calls)
    (l0, g0, n0), (l1, g1, n1), (_, _, n2) = res['stock'], res['fused'], res['off']
    print(case, 'stock conv2d / batch_norm calls: %d on the stock path, %d fused, %d with GHN3_NATIVE_EVALBN=0' % (n0, n1, n2),
          'logits %.2e' % _rel(l1, l0))
    assert n0 > 0 and n1 == 0 and n2 > 0, (n0, n1, n2)
    assert torch.isfinite(l0).all() and float(l0.norm()) > 0
    assert torch.isfinite(l1).all() and float(l1.norm()) > 0
    assert _rel(l1, l0) < 1e-3, _rel(l1, l0)
    worst = 0.0
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if a is not None and float(b.norm()) > 0:
            worst = max(worst, _rel(a, b))
            assert _rel(a, b) < 2e-3, _rel(a, b)
    print(case, 'worst parameter-gradient deviation %.2e' % worst)
