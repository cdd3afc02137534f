"""
The `msa` op of the target networks (the pre-LN transformer layer of the ViT-style networks, ops._TransformerLayer with
edge_dim = 0) on the fused HIP op family ghn3_msa_fwd / _bwd (ghn3_amd/csrc/tnet_msa.hip, target_ops.MsaLayer): the layer
against the same layer in float64 on the CPU (output, input gradient, every parameter gradient), determinism, the cases that
keep the stock path, whole ViT-style networks against the stock path and a GHN trained through a predicted ViT network.

Tolerances: every product is an exact fp32 product with fp32 accumulation (fp32 matrix cores), in another summation order
than torch's: 2e-5 of the output's scale, 1e-4 of a gradient's.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _has_msa_node(t):
    """True when the msa autograd node is t's grad_fn or one of its first two ancestors (a layout copy may follow it)."""
    fns = [t.grad_fn]
    for _ in range(2):
        nxt = []
        for f in fns:
            if f is None:
                continue
            if type(f).__name__ == 'MsaLayerBackward':
                return True
            nxt += [g for g, _ in f.next_functions if g is not None]
        fns = nxt
    return any(type(f).__name__ == 'MsaLayerBackward' for f in fns)


def _layer(C, stride, seed, mlp_ratio=1, qkv_bias=False):
    """ops.TransformerLayer (torch.nn flavour) in float64 with seeded parameters (LayerNorm affine terms away from 1 / 0)."""
    from ghn3_amd import ops
    torch.manual_seed(seed)
    layer = ops.TransformerLayer(C, stride=stride, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias).double()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if n.startswith(('ln1', 'ln2')):
                p.copy_((1.0 if n.endswith('weight') else 0.0) + 0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64))
            elif n.endswith('bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    return layer


CASES = [   # B, C, H, W, stride, channels_last, mlp_ratio, qkv_bias
    (64, 32, 11, 11, 1, False, 1, False),
    (64, 64, 11, 11, 1, True, 1, False),
    (64, 128, 11, 11, 1, False, 1, False),
    (8, 128, 14, 14, 1, True, 1, False),
    (4, 256, 7, 7, 2, False, 1, False),       # head dim 32, stride 2
    (3, 48, 5, 7, 2, True, 1, False),         # head dim 6, odd grid
    (2, 64, 1, 1, 1, False, 1, False),        # a single token
    (6, 64, 8, 8, 1, True, 4, False),         # mlp_ratio 4: hidden 256
    (5, 32, 9, 9, 1, False, 1, True),         # QKV bias
]


def _run(layer, x, up):
    x = x.clone().requires_grad_(True)
    out = layer(x)
    (out * up).sum().backward()
    return out, x.grad, [p.grad for _, p in layer.named_parameters()]


@pytest.mark.parametrize('case', CASES)
def test_msa_layer_matches_float64(case):
    B, C, H, W, s, cl, ratio, qb = case
    ref = _layer(C, s, seed=sum(case[:5]), mlp_ratio=ratio, qkv_bias=qb)
    dev = copy.deepcopy(ref).float().cuda()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    up = torch.randn(B, C, Ho, Wo, generator=g, dtype=torch.float64)
    o_ref, dx_ref, g_ref = _run(ref, x, up)
    xd = x.float().cuda()
    if cl:
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_(True)
    out = dev(xd)
    assert _has_msa_node(out), 'the layer did not run on the fused op'
    (out * up.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == o_ref.shape
    assert _rel(out.detach().cpu(), o_ref.detach()) < 2e-5, _rel(out.detach().cpu(), o_ref.detach())
    assert _rel(xd.grad.cpu(), dx_ref) < 1e-4, _rel(xd.grad.cpu(), dx_ref)
    names = [n for n, _ in ref.named_parameters()]
    assert len(names) == 11 + int(qb)
    for n, a, b in zip(names, [p.grad for _, p in dev.named_parameters()], g_ref):
        assert a is not None and a.data_ptr() != xd.grad.data_ptr(), n
        assert _rel(a.cpu(), b) < 1e-4, (n, _rel(a.cpu(), b))


def test_msa_layer_is_deterministic_and_inference_matches():
    ref = _layer(64, 1, seed=3)
    dev = copy.deepcopy(ref).float().cuda()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(16, 64, 11, 11, generator=g).cuda()
    up = torch.randn(16, 64, 11, 11, generator=g).cuda()
    runs = []
    for _ in range(2):
        dev.zero_grad(set_to_none=True)
        out, dx, grads = _run(dev, x, up)
        torch.cuda.synchronize()
        runs.append((out.detach().clone(), dx.clone(), [t.clone() for t in grads]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    with torch.no_grad():
        y = dev(x)
    assert torch.equal(y, runs[0][0])


def _fallback(monkeypatch, layer, x, env=None, autocast=False):
    """(fused-setting output, stock output) of the same layer and input; asserts the fused op was not used."""
    res = []
    for mode in ('fused', 'stock'):
        monkeypatch.setenv('GHN3_NATIVE_OPS', '1' if mode == 'fused' else '0')
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        torch.manual_seed(11)
        with torch.autocast('cuda', enabled=autocast):
            y = layer(x)
        assert not _has_msa_node(y)
        res.append(y.detach().float())
    return res


def test_msa_layers_outside_the_op_keep_the_stock_path(monkeypatch):
    from ghn3_amd import ops
    g = torch.Generator().manual_seed(2)
    # head dim 64
    wide = ops.TransformerLayer(512).cuda()
    x = torch.randn(2, 512, 4, 4, generator=g).cuda().requires_grad_(True)
    a, b = _fallback(monkeypatch, wide, x)
    assert torch.equal(a, b)
    # dropout p > 0 while training
    layer = ops.TransformerLayer(64).cuda().train()
    layer.ff.net[2] = torch.nn.Dropout(0.3)
    x = torch.randn(4, 64, 6, 6, generator=g).cuda().requires_grad_(True)
    a, b = _fallback(monkeypatch, layer, x)
    assert torch.equal(a, b)
    # GHN3_NATIVE_MSA=0
    layer = ops.TransformerLayer(64).cuda()
    a, b = _fallback(monkeypatch, layer, x, env={'GHN3_NATIVE_MSA': '0'})
    assert torch.equal(a, b)
    monkeypatch.delenv('GHN3_NATIVE_MSA')
    # autocast with GHN3_NATIVE_AMP=0
    a, b = _fallback(monkeypatch, layer, x, env={'GHN3_NATIVE_AMP': '0'}, autocast=True)
    assert torch.equal(a, b)


def _light_params(net, seed):
    """Seeded tensors assigned as a GHN assigns its prediction: views of one flat buffer (the leaf)."""
    import recipe
    table = {}
    for cell in net._layered_modules:
        table.update(cell)
    shapes = [(n, tuple(e['sz'])) for n, e in table.items()]
    params = recipe.seeded_net_params(shapes, seed=seed)
    total = sum(int(np.prod(s)) for _, s in shapes)
    flat = torch.zeros(total, device='cuda')
    off = 0
    for n, s in shapes:
        k = int(np.prod(s))
        flat[off:off + k] = torch.from_numpy(params[n]).reshape(-1).cuda()
        off += k
    flat.requires_grad_(True)
    off = 0
    for n, e in table.items():
        k = int(np.prod(e['sz']))
        setattr(e['module'], 'weight' if e['is_w'] else 'bias', flat[off:off + k].view(tuple(e['sz'])))
        off += k
    leaves = [flat]
    if hasattr(net, 'auxiliary_head'):
        net.auxiliary_head.cuda()
        leaves += list(net.auxiliary_head.parameters())
    return leaves


def _count_msa(net):
    return sum(1 for _, m in net.named_modules() if type(m).__name__.startswith('TransformerLayer'))


def _compare_net(monkeypatch, make, x, seed, light):
    res = {}
    for mode in ('stock', 'fused'):
        monkeypatch.setenv('GHN3_NATIVE_OPS', '0' if mode == 'stock' else '1')
        net = make()
        if light:
            leaves = _light_params(net, seed)
        else:
            import recipe
            net = net.cuda()
            params = recipe.seeded_net_params([(n, tuple(p.shape)) for n, p in net.named_parameters()], seed=seed)
            with torch.no_grad():
                for n, p in net.named_parameters():
                    p.copy_(torch.from_numpy(params[n]))
            leaves = [p for _, p in net.named_parameters()]
        net.train()
        hits = []
        import ghn3_amd.target_ops as T
        orig = T.MsaLayer.apply

        def counted(*a):
            hits.append(1)
            return orig(*a)
        monkeypatch.setattr(T.MsaLayer, 'apply', counted)
        torch.manual_seed(123)
        logits, aux = net(x)
        monkeypatch.setattr(T.MsaLayer, 'apply', orig)
        loss = logits.square().mean() + (aux.square().mean() if aux is not None else 0.)
        loss.backward()
        torch.cuda.synchronize()
        res[mode] = (logits.detach().cpu(), [p.grad.detach().cpu() if p.grad is not None else None for p in leaves], len(hits))
    (l0, g0, n0), (l1, g1, n1) = res['stock'], res['fused']
    assert n0 == 0 and n1 > 0, (n0, n1)
    assert _rel(l1, l0) < 1e-3, _rel(l1, l0)
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if a is not None and float(b.norm()) > 0:
            assert _rel(a, b) < 2e-3, _rel(a, b)


@pytest.mark.parametrize('light', [False, True])
def test_vit_network_case_matches_the_stock_path(light, monkeypatch):
    import network_cases
    import recipe
    from ghn3_amd import ops
    geno, kw, img = network_cases.CASES['vit']
    g = ops.Genotype(**geno)
    kws = {k: ('bn' if (k == 'norm' and v and light) else v) for k, v in kw.items()}
    x = torch.from_numpy(recipe.seeded_images(img, seed=7)).cuda()
    _compare_net(monkeypatch, lambda: (ops.NetworkLight if light else ops.Network)(genotype=g, **kws), x, len('vit'), light)


@pytest.mark.parametrize('k', [38, 39])
def test_sampled_vit_architectures_match_the_stock_path(k, monkeypatch):
    import recipe
    from ghn3_amd.deepnets1m import SampledNets
    assert _count_msa(SampledNets(large_images=False, seed=0, max_nodes=400)[k].net) > 0
    x = torch.from_numpy(recipe.seeded_images((8, 3, 32, 32), seed=3)).cuda()
    _compare_net(monkeypatch, lambda: SampledNets(large_images=False, seed=0, max_nodes=400)[k].net, x, 100 + k, True)


def test_imagenet_input_vit_matches_the_stock_path(monkeypatch):
    """The vit case's genotype on 224 x 224 images: 14 x 14 tokens per map."""
    import network_cases
    import recipe
    from ghn3_amd import ops
    geno, kw, _ = network_cases.CASES['vit']
    g = ops.Genotype(**geno)
    kws = dict(kw, is_imagenet_input=True, num_classes=1000)
    x = torch.from_numpy(recipe.seeded_images((2, 3, 224, 224), seed=4)).cuda()
    _compare_net(monkeypatch, lambda: ops.NetworkLight(genotype=g, **kws), x, 17, True)


def test_ghn_gradients_through_a_predicted_vit_network(monkeypatch):
    import recipe
    from util_parity import make_models
    from ghn3_amd import GraphBatch
    from ghn3_amd.deepnets1m import SampledNets
    x = torch.from_numpy(recipe.seeded_images((8, 3, 32, 32), seed=3)).cuda()
    y = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7]).cuda()
    grads = {}
    for native in ('1', '0'):
        monkeypatch.setenv('GHN3_NATIVE_MSA', native)
        hip, _ = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
        hip.train()
        graph = SampledNets(large_images=False, seed=0, max_nodes=400)[38]
        gb = GraphBatch([graph], dense=True)
        torch.manual_seed(5)                       # (the same draws of every random layer in both runs)
        models = hip([graph.net], gb.to_device('cuda'), bn_track_running_stats=True, keep_grads=True, reduce_graph=True)
        assert _count_msa(models[0]) > 0
        logits = models[0](x)[0]
        torch.nn.functional.cross_entropy(logits, y).backward()
        torch.cuda.synchronize()
        grads[native] = {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters() if p.grad is not None}
    assert grads['1'].keys() == grads['0'].keys() and len(grads['1']) > 0
    # (over all GHN parameters at once: some tensors' exact gradient is zero -- a bias added to every attention score of a row --
    # and what the runs leave there is rounding noise of either path)
    names = sorted(grads['0'])
    a = torch.cat([grads['1'][n].reshape(-1) for n in names])
    b = torch.cat([grads['0'][n].reshape(-1) for n in names])
    assert _rel(a, b) < 2e-4, _rel(a, b)
