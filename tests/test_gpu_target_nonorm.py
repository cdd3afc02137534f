"""
Target networks built with norm=None (`bn_layer`, ops.py:91-96: every norm slot an Identity) on the native HIP layers:

  * the depthwise + pointwise family without a norm layer (target_ops.dwpw on ghn3_dwpw_plain_fwd / _bwd) against torch in fp64
    at the rows of tests/nonorm_cases.py -- output, dx, dw_dw, dw_pw under tests/util_parity.slice_errors, 2e-4 / 3e-4 (the
    project's bounds for this family), twice for equal bits, with NaN-filled buffers, after `DwPw.applicable`;
  * every block of the search space with an Identity norm, both flavours, against the same module on the stock layers, with the
    native nodes -- and no ConvolutionBackward -- in its autograd graph; GHN3_NATIVE_NONORM=0 restores the stock graph;
  * whole BN-free networks, both flavours, fused against stock, with no call of F.conv2d / F.batch_norm on the fused path;
  * BN-free networks trained through the GHN against the CPU oracle, and two Trainer steps on a BN-free stream.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nonorm_cases as C
import recipe
import target_edge_cases as E
from util_parity import make_models, slice_errors

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = 2e-4, 3e-4
GHN_SEED = 7                                     # loader seed of the GHN and Trainer tests: finite oracle loss (see there)


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


@pytest.fixture(params=['allocator', 'nan-filled'])
def buffers(request, monkeypatch):
    """The op's buffers as the caching allocator hands them out, or pre-filled with NaN."""
    if request.param == 'allocator':
        yield None
        return
    from ghn3_amd import target_ops as T
    proxy = _GarbageTorch()
    monkeypatch.setattr(T, 'torch', proxy)
    yield proxy
    assert proxy.spoiled >= 2, 'the ops no longer allocate through torch.empty / empty_like: the variant checks nothing'


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


# ---- 4. op level, against fp64 torch ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(row, depthwise):
    if depthwise:
        x, w_dw, w_pw, up, (ks, st, pad, dil) = C.dwpw_case(row)
    else:
        (x, w_pw, up, st), w_dw, ks, pad, dil = C.pw_case(row), None, 1, 0, 1
    leaves = [None if t is None else t.clone().double().requires_grad_(True) for t in (x, w_dw, w_pw)]
    y = F.relu(leaves[0])
    if depthwise:
        ref = F.conv2d(F.conv2d(y, leaves[1], None, st, pad, dil, groups=x.shape[1]), leaves[2])
    else:
        ref = F.conv2d(y, leaves[2], None, st)
    (ref * up.double()).sum().backward()
    return (x, w_dw, w_pw, up), (ks, st, pad, dil), ref.detach(), [None if t is None else t.grad for t in leaves]


def _run_op(row, depthwise):
    from ghn3_amd import target_ops as T
    (x, w_dw, w_pw, up), (ks, st, pad, dil), ref, ref_grads = _reference(row, depthwise)
    label = 'dwpw' if depthwise else 'pointwise'
    runs = []
    for _ in range(2):
        dev = [None if t is None else t.cuda().requires_grad_(True) for t in (x, w_dw, w_pw)]
        assert T.DwPw.applicable(dev[0], dev[1], dev[2], ks)
        out = T.dwpw(dev[0], dev[1], dev[2], stride=st, padding=pad, dilation=dil)
        assert type(out.grad_fn).__name__ == 'DwPwBackward'
        assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
        (out * up.cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().cpu(), [None if t is None else t.grad.cpu() for t in dev]))
    (out, grads), (out2, grads2) = runs
    names = ('dx', 'dw_dw', 'dw_pw')
    assert torch.equal(out2, out)                                   # deterministic: the same bits again,
    for name, a, b in zip(names, grads, grads2):
        assert a is None or torch.equal(a, b), name                # ... the fixed-order reductions of the gradients included
    worst = {}
    for name, got, want, axes, tol in [('out', out, ref, E.ACT_AXES, OUT_TOL), ('dx', grads[0], ref_grads[0], E.ACT_AXES, GRAD_TOL),
                                       ('dw_dw', grads[1], ref_grads[1], E.WGRAD_AXES, GRAD_TOL),
                                       ('dw_pw', grads[2], ref_grads[2], E.WGRAD_AXES, GRAD_TOL)]:
        if want is None:
            continue
        assert got.shape == want.shape, (label, name, got.shape, want.shape)
        v, where = slice_errors(got, want, axes)
        worst[name] = v
        print('%s %s %s per-slice error %.2e' % (label, row, name, v))
        assert v <= tol, (label, name, v, where)


@pytest.mark.parametrize('row', C.DWPW_ROWS, ids=str)
def test_dwpw_rows_against_fp64(row, buffers):
    _run_op(row, True)


@pytest.mark.parametrize('row', C.PW_ROWS, ids=str)
def test_pointwise_rows_against_fp64(row, buffers):
    _run_op(row, False)


def test_dwpw_refuses_cpu_tensors_and_bad_descriptors():
    from ghn3_amd import target_ops as T, _lib as L
    with pytest.raises(L.Ghn3Error):
        T.dwpw(torch.randn(1, 8, 4, 4), torch.randn(8, 1, 3, 3), torch.randn(8, 8), padding=1)
    x = torch.randn(1, 6, 4, 4, device='cuda')
    assert not T.DwPw.applicable(x, torch.randn(6, 1, 3, 3, device='cuda'), torch.randn(8, 6, device='cuda'), 3)
    with pytest.raises(L.Ghn3Error):          # C % 4 != 0 straight through the ABI
        T.dwpw(x, torch.randn(6, 1, 3, 3, device='cuda'), torch.randn(8, 6, device='cuda'), padding=1)


# ---- 5. module level, both flavours ----------------------------------------------------------------------------------------
def _stems():
    from ghn3_amd import ops
    plan = dict(C=16, num_classes=10, n_steps=2, n_cells=3, ks=3, is_imagenet_input=False, imagenet_stride=4, is_vit=False,
                preproc=True, C_mult=2, fc_layers=1, fc_dim=0, glob_avg=True, multiplier=(2, 2))
    simple = ops.network_plan(stem_pool=True, stem_type=0, **plan)['stems']
    two = ops.network_plan(stem_pool=False, stem_type=1, **plan)['stems']
    return {'stem': simple['stem'], 'stem0': two['stem0'], 'stem1': two['stem1']}


# name -> (constructor name, arguments, input channels, native node, how many of it)
BLOCKS = {
    'dil_conv_3x3_s2': ('DilConv', (12, 16, 3, 2, 2, 2), 12, 'DwPwBackward', 1),
    'sep_conv_5x5': ('SepConv', (12, 16, 5, 1, 2), 12, 'DwPwBackward', 2),
    'conv_1x1_s2': ('ReLUConvBN', (12, 16, 1, 2, 0), 12, 'DwPwBackward', 1),
    'conv_3x3': ('ReLUConvBN', (8, 16, 3, 1, 1), 8, 'ConvOnlyBackward', 1),
    'conv_1x7_7x1_s2': ('ReLUConvBN', (12, 12, 7, 2, 3), 12, 'ConvOnlyBackward', 2),
    'factorized_reduce': ('FactorizedReduce', (12, 16), 12, 'ConvOnlyBackward', 1),
    'stem': ('seq', 'stem', 3, 'ConvOnlyBackward', 1),
    'stem0': ('seq', 'stem0', 3, 'ConvOnlyBackward', 2),
    'stem1': ('seq', 'stem1', 16, 'ConvOnlyBackward', 1),
}


def _build(name, light):
    """(module, its parameter leaves) on the GPU: seeded weights, the same in every mode."""
    from ghn3_amd import ops
    kind, args, _, _, _ = BLOCKS[name]
    torch.manual_seed(13)
    if kind == 'seq':
        m = ops._layer_seq(ops._LightLayers if light else ops._TorchLayers, None, _stems()[args])
    else:
        kw = dict(norm=None, double=True) if name.startswith('conv_1x7') else dict(norm=None)
        m = getattr(ops, kind + ('Light' if light else ''))(*args, **kw)
    if not light:
        m = m.cuda().train()
        return m, list(m.parameters())
    gen, leaves = torch.Generator().manual_seed(17), []
    for _, sub in m.named_modules():
        for n, p in list(sub.__dict__['_parameters'].items()):
            if isinstance(p, (list, tuple)):
                t = (torch.randn(*p, generator=gen) / float(np.prod(p[1:])) ** 0.5).cuda().requires_grad_(True)
                setattr(sub, n, t)
                leaves.append(t)
    return m, leaves


def _run_block(name, light):
    from ghn3_amd import ops
    m, leaves = _build(name, light)
    assert leaves
    x0 = torch.randn(4, BLOCKS[name][2], 8, 8, generator=torch.Generator().manual_seed(21)).cuda().requires_grad_(True)
    x = x0 * 1.0                                               # (a non-leaf: stem1's in-place ReLU rewrites it)
    y = ops.Network._run_stem(m, x) if BLOCKS[name][0] == 'seq' else m(x)
    up = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).cuda()
    ((y * up).sum() + (x * x).sum()).backward()                # (x enters the loss AFTER the block: sees an in-place ReLU)
    torch.cuda.synchronize()
    return y.detach().cpu(), x.detach().cpu(), x0.grad.cpu(), [p.grad.cpu() for p in leaves], _graph_nodes(y)


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
@pytest.mark.parametrize('name', list(BLOCKS))
def test_blocks_with_an_identity_norm_run_on_the_native_nodes(name, light, monkeypatch):
    node, count = BLOCKS[name][3:]
    monkeypatch.setenv('GHN3_NATIVE_OPS', '0')
    stock = _run_block(name, light)
    monkeypatch.setenv('GHN3_NATIVE_OPS', '1')
    fused = _run_block(name, light)
    monkeypatch.setenv('GHN3_NATIVE_NONORM', '0')
    off = _run_block(name, light)
    assert 'ConvolutionBackward0' in stock[4] and node not in stock[4], stock[4]
    assert fused[4].count(node) == count and 'ConvolutionBackward0' not in fused[4], fused[4]
    assert 'ConvolutionBackward0' in off[4] and 'DwPwBackward' not in off[4] and 'ConvOnlyBackward' not in off[4], off[4]
    assert fused[0].shape == stock[0].shape
    print(name, 'light' if light else 'torch', 'out %.2e dx %.2e' % (_rel(fused[0], stock[0]), _rel(fused[2], stock[2])),
          'params', ' '.join('%.2e' % _rel(a, b) for a, b in zip(fused[3], stock[3])))
    assert _rel(fused[0], stock[0]) < 2e-4
    assert torch.equal(fused[1], stock[1])                     # what an in-place ReLU left in the caller's tensor
    assert _rel(fused[2], stock[2]) < 5e-4
    for a, b in zip(fused[3], stock[3]):
        assert a.shape == b.shape and _rel(a, b) < 5e-4, _rel(a, b)
    assert torch.equal(off[0], stock[0])


# ---- 6. whole BN-free networks ---------------------------------------------------------------------------------------------
def _bn_free_cases():
    import network_cases
    return {'conv': (network_cases._CONV, dict(C=8, num_classes=10, n_cells=3, is_imagenet_input=False, norm=None)),
            'plain': (network_cases._PLAIN, dict(C=8, num_classes=10, n_cells=3, is_imagenet_input=False, norm=None,
                                                 preproc=False, C_mult=1))}


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


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
@pytest.mark.parametrize('case', ['conv', 'plain'])
def test_bn_free_networks_run_without_a_stock_convolution(case, light, monkeypatch):
    """Filled in as test_gpu_target_ops.test_networks_on_the_fused_layers_match_the_stock_path; bounds as there."""
    from ghn3_amd import ops
    geno, kw = _bn_free_cases()[case]
    g = ops.Genotype(**geno)
    calls = _Calls(monkeypatch)
    res = {}
    for mode in ('stock', 'fused'):
        monkeypatch.setenv('GHN3_NATIVE_OPS', '0' if mode == 'stock' else '1')
        torch.manual_seed(0)
        net = (ops.NetworkLight if light else ops.Network)(genotype=g, **kw)
        x = torch.from_numpy(recipe.seeded_images((4, 3, 32, 32), seed=7)).cuda()
        if light:
            table = {}
            for cell in net._layered_modules:
                table.update(cell)
            shapes = [(n, tuple(e['sz'])) for n, e in table.items()]
            params = recipe.seeded_net_params(shapes, seed=len(case))
            flat = torch.zeros(sum(int(np.prod(s)) for _, s in shapes), device='cuda', requires_grad=True)
            off = 0
            with torch.no_grad():
                for n, s in shapes:
                    k = int(np.prod(s))
                    flat[off:off + k] = torch.from_numpy(params[n]).reshape(-1).cuda()
                    off += k
            off = 0
            for n, e in table.items():
                k = int(np.prod(e['sz']))
                setattr(e['module'], 'weight' if e['is_w'] else 'bias', flat[off:off + k].view(tuple(e['sz'])))
                off += k
            leaves = [flat]
        else:
            net = net.cuda()
            params = recipe.seeded_net_params([(n, tuple(p.shape)) for n, p in net.named_parameters()], seed=len(case))
            with torch.no_grad():
                for n, p in net.named_parameters():
                    p.copy_(torch.from_numpy(params[n]))
            leaves = [p for _, p in net.named_parameters()]
        net.train()
        torch.manual_seed(123)
        calls.n = 0
        logits, aux = net(x)
        assert aux is None
        logits.square().mean().backward()
        torch.cuda.synchronize()
        res[mode] = (logits.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu() for p in leaves], calls.n)
    (l0, g0, n0), (l1, g1, n1) = res['stock'], res['fused']
    print(case, 'light' if light else 'torch', 'stock conv2d / batch_norm calls: %d on the stock path, %d fused' % (n0, n1),
          'logits %.2e' % _rel(l1, l0))
    assert n0 > 0 and n1 == 0, (n0, n1)
    assert torch.isfinite(l0).all() and float(l0.norm()) > 0
    assert _rel(l1, l0) < 1e-3, _rel(l1, l0)
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if a is not None and float(b.norm()) > 0:
            assert _rel(a, b) < 2e-3, _rel(a, b)


# ---- 7. through the GHN ----------------------------------------------------------------------------------------------------
def test_bn_free_light_networks_trained_through_the_ghn_vs_oracle():
    """test_gpu_networks.test_light_networks_trained_through_the_ghn_vs_oracle on two norm=None architectures: loss and GHN
    gradients against the CPU oracle GHN driving the same light networks, that test's bounds.  GHN_SEED is a loader seed at
    which the oracle's loss is finite (the networks have no norm layer to rescale what the untrained GHN predicts)."""
    from oracle import ghn3_ref as R
    from ghn3_amd.deepnets1m import SampledNets
    hip, oracle = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
    hip.train()
    oracle.train()
    gen = torch.Generator().manual_seed(3)
    images = torch.randn(4, 3, 32, 32, generator=gen)
    labels = torch.tensor([2, 0, 9, 4])
    gb = next(SampledNets.loader(meta_batch_size=2, seed=GHN_SEED, max_nodes=120, bn_free_prob=1.0))
    gb_o = next(SampledNets.loader(meta_batch_size=2, seed=GHN_SEED, max_nodes=120, bn_free_prob=1.0))
    assert all(a['norm'] is None for a in gb.net_args)

    nets = hip(gb.nets, gb.to_device('cuda'), keep_grads=True)
    loss = 0.
    for net in nets:
        net.eval()
        logits, aux = net(images.cuda())
        assert aux is None and logits.shape == (4, 10)
        loss = loss + F.cross_entropy(logits, labels.cuda())
    loss.backward()
    torch.cuda.synchronize()

    gbr = R.GraphBatchRef([R.GraphRef(nf, ni, A) for nf, ni, A in zip(gb_o.node_feat, gb_o.node_info, gb_o.edges)])
    nets_o, _ = oracle(gb_o.nets, gbr, keep_grads=True)
    for net_o in nets_o:
        net_o.eval()
    loss_o = sum(F.cross_entropy(net(images)[0], labels) for net in nets_o)
    loss_o.backward()
    assert np.isfinite(loss_o.item()), loss_o.item()
    print('loss %.6f oracle %.6f' % (loss.item(), loss_o.item()))
    assert abs(loss.item() - loss_o.item()) < 2e-4 * max(1.0, abs(loss_o.item())), (loss.item(), loss_o.item())
    po = dict(oracle.named_parameters())
    seen, worst = 0, 0.0
    for k, p in hip.named_parameters():
        go = po[k].grad
        if go is None or float(go.norm()) < 1e-7:
            continue
        assert p.grad is not None, k
        err = float((p.grad.cpu().double() - go.double()).norm())
        worst = max(worst, err / float(go.norm()))
        assert err < 2e-3 * float(go.norm()) + 1e-6, (k, err, float(go.norm()))
        seen += 1
    print('GHN gradients: %d compared, worst relative error %.2e' % (seen, worst))
    assert seen > 20


# ---- 8. trainer ------------------------------------------------------------------------------------------------------------
def test_trainer_steps_on_a_bn_free_stream():
    from ghn3_amd import Trainer
    from ghn3_amd.deepnets1m import SampledNets
    hip, _ = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
    gen = torch.Generator().manual_seed(1)
    images = torch.randn(4, 3, 32, 32, generator=gen)
    targets = torch.tensor([1, 7, 3, 9])
    tr = Trainer(hip, 'adamw', {'lr': 1e-3, 'weight_decay': 1e-2}, 'cosine', n_batches=2, grad_clip=5, device='cuda',
                 log_interval=1, predparam_wd=3e-5, epochs=2)
    queue = SampledNets.loader(meta_batch_size=2, seed=GHN_SEED, max_nodes=120, bn_free_prob=1.0)
    before = hip._flat.detach().clone()
    for step in range(2):
        gb = next(queue)
        assert all(a['norm'] is None for a in gb.net_args)
        m = tr.update(images, targets, graphs=gb)
    avg = m.avg()
    print('metrics', avg, 'skipped', tr.skipped_updates)
    assert np.isfinite(avg['loss']) and 0.0 <= avg['top1'] <= 100.0 and tr.skipped_updates == 0
    assert not torch.equal(before, hip._flat)
