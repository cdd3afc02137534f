"""
The wide msa path (ghn3_attn_wide_* / ghn3_msa_wide_*, ghn3_amd/csrc/tnet_msa_wide.hip; target_ops.WideAttention, MsaWideLayer
under GHN3_NATIVE_MSA_WIDE=1): the attention for head dims 33 .. 64 against the float64 reference of msa_lean_cases.py, its
d <= 32 route against lean_attention bit for bit, the layer against the same layer in float64 on the CPU, determinism and the
inference forward, the routing under the switch, a sampled wide ViT-style network against the stock path and a GHN trained
through it.

Tolerances: those of tests/test_gpu_target_msa.py and test_gpu_target_msa_lean.py -- exact fp32 products with fp32
accumulation in another summation order than the reference's: relative L2 error 2e-5 for outputs (lse is one), 1e-4 for
gradients, the attention also per (b, head, 32-row block) slice on the whole tensor's scale.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

import msa_wide_cases as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))

GUARD = 4096


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _nodes(t, depth=3):
    """Names of t's grad_fn and of its ancestors up to `depth` steps back (a layout copy may follow the layer's node)."""
    fns, names = [t.grad_fn], set()
    for _ in range(depth + 1):
        nxt = []
        for f in fns:
            if f is None:
                continue
            names.add(type(f).__name__)
            nxt += [g for g, _ in f.next_functions if g is not None]
        fns = nxt
    return names


def _guarded(n):
    """n floats of NaN sentinel followed by a guard region of GUARD more."""
    return torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device='cuda')


def _entry_points(B, H, N, d, qkv, dO):
    """One forward and backward through the C entry points into sentinel-filled, guarded buffers: out, lse, dqkv."""
    from ghn3_amd import _lib as L
    from ghn3_amd import target_ops as T
    C = H * d
    lib = L.load()
    out, lse, dqkv = _guarded(B * N * C), _guarded(B * H * N), _guarded(B * N * 3 * C)
    L._check(lib.ghn3_attn_wide_fwd(out.data_ptr(), lse.data_ptr(), qkv.data_ptr(), B, N, C, H, T._stream()), 'ghn3_attn_wide_fwd')
    L._check(lib.ghn3_attn_wide_bwd(dqkv.data_ptr(), dO.data_ptr(), qkv.data_ptr(), lse.data_ptr(), out.data_ptr(), B, N, C, H,
                                    T._stream()), 'ghn3_attn_wide_bwd')
    torch.cuda.synchronize()
    for name, t in (('out', out), ('lse', lse), ('dqkv', dqkv)):
        assert not bool(torch.isnan(t[:-GUARD]).any()), '%s: an element was not written' % name
        assert bool(torch.isnan(t[-GUARD:]).all()), '%s: the guard region was written' % name
    return out[:-GUARD].view(B, N, C), lse[:-GUARD].view(B, H, N), dqkv[:-GUARD].view(B, N, 3 * C)


@pytest.mark.parametrize('case', M.OP_CASES)
def test_wide_attention_matches_float64(case):
    from ghn3_amd import target_ops as T
    B, H, N, d, _ = case
    C = H * d
    q, k, v, g = M.inputs(case)
    ref = M.reference(case)
    qkv = torch.from_numpy(M.pack_qkv(q, k, v)).cuda()
    dO = torch.from_numpy(M.pack_heads(g)).cuda()
    out, lse, dqkv = _entry_points(B, H, N, d, qkv, dO)
    # the public op: the same kernels behind autograd, and a rerun
    x = qkv.clone().requires_grad_(True)
    y = T.wide_attention(x, H)
    y.backward(dO)
    torch.cuda.synchronize()
    assert y.shape == (B, N, C) and torch.equal(y.detach(), out) and torch.equal(x.grad, dqkv)
    with torch.no_grad():
        assert torch.equal(T.wide_attention(qkv, H), out)

    slices = M.ref_slices(case)
    sel = lambda t, b, h, o: t[b, :, o + h * d:o + (h + 1) * d].cpu().numpy()      # noqa: E731
    got = {'out': [sel(out, b, h, 0) for b, h in slices], 'lse': [lse[b, h].cpu().numpy()[:, None] for b, h in slices],
           'dq': [sel(dqkv, b, h, 0) for b, h in slices], 'dk': [sel(dqkv, b, h, C) for b, h in slices],
           'dv': [sel(dqkv, b, h, 2 * C) for b, h in slices]}
    want = {n: [ref[s][i] if n != 'lse' else ref[s][i][:, None] for s in slices]
            for i, n in enumerate(('out', 'lse', 'dq', 'dk', 'dv'))}
    failures = []
    for n in ('out', 'lse', 'dq', 'dk', 'dv'):
        tol = M.OUT_TOL if n in ('out', 'lse') else M.GRAD_TOL
        if N == 1 and n in ('dq', 'dk'):
            # exact zeros in float64: an absolute bound on the scale of the terms that cancel (as the lean test)
            bound = 1e-5 * float(np.abs(g).max()) * float(np.abs(v).max()) * float(np.abs(k).max()) * d
            worst = max(float(np.abs(a).max()) for a in got[n])
            print('%s %s: max |value| %.2e (bound %.2e)' % (case, n, worst, bound))
            if not worst <= bound:
                failures.append((n, worst, bound))
            continue
        e, eb = M.rel_l2(got[n], want[n]), M.worst_block(got[n], want[n])
        print('%s %s: rel L2 %.2e, worst 32-row block %.2e (bound %.0e)' % (case, n, e, eb, tol))
        if not (e <= tol and eb <= tol):
            failures.append((n, e, eb, tol))
    assert not failures, failures


@pytest.mark.parametrize('shape', M.LEAN_EQUAL)
def test_wide_entry_points_equal_lean_attention_up_to_32_columns(shape):
    from ghn3_amd import target_ops as T
    B, H, N, d = shape
    g = torch.Generator().manual_seed(d)
    qkv = torch.randn(B, N, 3 * H * d, generator=g).cuda()
    dO = torch.randn(B, N, H * d, generator=g).cuda()
    out, lse, dqkv = _entry_points(B, H, N, d, qkv, dO)
    x = qkv.clone().requires_grad_(True)
    y = T.lean_attention(x, H)
    y.backward(dO)
    torch.cuda.synchronize()
    assert torch.equal(y.detach(), out) and torch.equal(x.grad, dqkv)


# ---- the layer ------------------------------------------------------------------------------------------------------------
def _layer(C, heads, stride, seed, mlp_ratio=1, qkv_bias=False):
    """ops.TransformerLayer (torch.nn flavour) in float64 with seeded parameters (LayerNorm affine terms away from 1 / 0)."""
    from ghn3_amd import ops
    torch.manual_seed(seed)
    layer = ops.TransformerLayer(C, num_heads=heads, stride=stride, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias).double()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if n.startswith(('ln1', 'ln2')):
                p.copy_((1.0 if n.endswith('weight') else 0.0) + 0.3 * torch.randn(p.shape, generator=g, dtype=torch.float64))
            elif n.endswith('bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    return layer


def _run(layer, x, up):
    x = x.clone().requires_grad_(True)
    out = layer(x)
    (out * up).sum().backward()
    return out, x.grad, [p.grad for _, p in layer.named_parameters()]


@pytest.mark.parametrize('case', M.LAYER_CASES)
def test_wide_msa_layer_matches_float64(case, monkeypatch):
    monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', '1')
    B, C, heads, H, W, s, cl, ratio, qb = case
    ref = _layer(C, heads, s, seed=sum(case[:6]), mlp_ratio=ratio, qkv_bias=qb)
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
    names = _nodes(out)
    assert 'MsaWideLayerBackward' in names and 'MsaLayerBackward' not in names, names
    (out * up.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert out.shape == o_ref.shape
    errs = {'out': _rel(out.detach().cpu(), o_ref.detach()), 'dx': _rel(xd.grad.cpu(), dx_ref)}
    pnames = [n for n, _ in ref.named_parameters()]
    assert len(pnames) == 11 + int(qb)
    for n, a, b in zip(pnames, [p.grad for _, p in dev.named_parameters()], g_ref):
        assert a is not None and a.data_ptr() != xd.grad.data_ptr(), n
        errs[n] = _rel(a.cpu(), b)
    print(case, ' '.join('%s %.1e' % kv for kv in errs.items()))
    assert errs['out'] < 2e-5, errs
    assert all(v < 1e-4 for k, v in errs.items() if k != 'out'), errs


def test_wide_msa_layer_is_deterministic_and_inference_matches(monkeypatch):
    monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', '1')
    dev = _layer(512, 8, 1, seed=3).float().cuda()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 512, 6, 6, generator=g).cuda()
    up = torch.randn(4, 512, 6, 6, generator=g).cuda()
    runs = []
    for _ in range(2):
        dev.zero_grad(set_to_none=True)
        out, dx, grads = _run(dev, x, up)
        torch.cuda.synchronize()
        assert 'MsaWideLayerBackward' in _nodes(out)
        runs.append((out.detach().clone(), dx.clone(), [t.clone() for t in grads]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))
    with torch.no_grad():
        y = dev(x)
    assert torch.equal(y, runs[0][0])


# ---- routing ----------------------------------------------------------------------------------------------------------------
def _stock_pair(monkeypatch, layer, x, env=None, autocast=False):
    """(output under GHN3_NATIVE_OPS=1, output under =0) of the same layer and input; asserts no msa node ran in either."""
    res = []
    for ops_on in ('1', '0'):
        monkeypatch.setenv('GHN3_NATIVE_OPS', ops_on)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        torch.manual_seed(11)
        with torch.autocast('cuda', enabled=autocast):
            y = layer(x)
        assert not {'MsaWideLayerBackward', 'MsaLayerBackward'} & _nodes(y)
        res.append(y.detach().float())
    monkeypatch.delenv('GHN3_NATIVE_OPS')
    return res


def test_routing_under_the_switch(monkeypatch):
    from ghn3_amd import ops
    g = torch.Generator().manual_seed(2)
    wide = ops.TransformerLayer(512).cuda()
    x = torch.randn(2, 512, 4, 4, generator=g).cuda().requires_grad_(True)
    # unset or 0: the stock path, bit for bit
    monkeypatch.delenv('GHN3_NATIVE_MSA_WIDE', raising=False)
    a, b = _stock_pair(monkeypatch, wide, x)
    assert torch.equal(a, b)
    monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', '0')
    a, b = _stock_pair(monkeypatch, wide, x)
    assert torch.equal(a, b)
    # 1: the wide node -- unless something else keeps the stock path
    monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', '1')
    assert 'MsaWideLayerBackward' in _nodes(wide(x))
    dropped = ops.TransformerLayer(512).cuda().train()
    dropped.ff.net[2] = torch.nn.Dropout(0.3)
    a, b = _stock_pair(monkeypatch, dropped, x)
    assert torch.equal(a, b)
    a, b = _stock_pair(monkeypatch, wide, x, env={'GHN3_NATIVE_MSA': '0'})
    assert torch.equal(a, b)
    monkeypatch.delenv('GHN3_NATIVE_MSA')
    a, b = _stock_pair(monkeypatch, wide, x, env={'GHN3_NATIVE_AMP': '0'}, autocast=True)
    assert torch.equal(a, b)
    monkeypatch.delenv('GHN3_NATIVE_AMP')
    # a narrow layer still runs the narrow op
    narrow = ops.TransformerLayer(64).cuda()
    xn = torch.randn(4, 64, 6, 6, generator=g).cuda().requires_grad_(True)
    names = _nodes(narrow(xn))
    assert 'MsaLayerBackward' in names and 'MsaWideLayerBackward' not in names, names


# ---- a whole network ------------------------------------------------------------------------------------------------------
WIDE_NET = dict(large_images=False, seed=0, max_nodes=400, width_mult=4)
WIDE_NET_INDEX = 96                       # C = 512, one msa layer, 3.0 M parameters


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


def test_sampled_wide_vit_network_matches_the_stock_path(monkeypatch):
    import recipe
    import ghn3_amd.target_ops as T
    from ghn3_amd.deepnets1m import SampledNets
    monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', '1')
    x = torch.from_numpy(recipe.seeded_images((8, 3, 32, 32), seed=3)).cuda()
    res = {}
    for mode in ('stock', 'fused'):
        monkeypatch.setenv('GHN3_NATIVE_OPS', '0' if mode == 'stock' else '1')
        net = SampledNets(**WIDE_NET)[WIDE_NET_INDEX].net
        assert _count_msa(net) > 0
        leaves = _light_params(net, 100 + WIDE_NET_INDEX)
        net.train()
        hits = []
        orig = T.MsaWideLayer.apply
        monkeypatch.setattr(T.MsaWideLayer, 'apply', lambda *a: (hits.append(1), orig(*a))[1])
        torch.manual_seed(123)
        logits, aux = net(x)
        monkeypatch.setattr(T.MsaWideLayer, 'apply', orig)
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


def test_ghn_gradients_through_a_predicted_wide_vit_network(monkeypatch):
    import recipe
    from util_parity import make_models
    from ghn3_amd import GraphBatch
    from ghn3_amd.deepnets1m import SampledNets
    x = torch.from_numpy(recipe.seeded_images((8, 3, 32, 32), seed=3)).cuda()
    y = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7]).cuda()
    grads = {}
    for wide in ('1', '0'):
        monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', wide)
        hip, _ = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
        hip.train()
        graph = SampledNets(**WIDE_NET)[WIDE_NET_INDEX]
        gb = GraphBatch([graph], dense=True)
        torch.manual_seed(5)                       # (the same draws of every random layer in both runs)
        models = hip([graph.net], gb.to_device('cuda'), bn_track_running_stats=True, keep_grads=True, reduce_graph=True)
        assert _count_msa(models[0]) > 0
        logits = models[0](x)[0]
        torch.nn.functional.cross_entropy(logits, y).backward()
        torch.cuda.synchronize()
        grads[wide] = {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters() if p.grad is not None}
    assert grads['1'].keys() == grads['0'].keys() and len(grads['1']) > 0
    names = sorted(grads['0'])
    a = torch.cat([grads['1'][n].reshape(-1) for n in names])
    b = torch.cat([grads['0'][n].reshape(-1) for n in names])
    assert _rel(a, b) < 2e-4, _rel(a, b)
