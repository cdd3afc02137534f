"""
The lean attention of the target networks' msa layers (ghn3_attn_lean_fwd / _bwd, ghn3_amd/csrc/tnet_attn.hip) and the msa
layer on it (ghn3_msa_lean_*, target_ops.MsaLayer under target_ops.msa_lean): the op against the float64 reference of
msa_lean_cases.py, the layer against the same layer in float64 on the CPU, the memory the forward keeps, a shape the saved-P
path refuses, and a whole ViT-style network under GHN3_MSA_LEAN=1 against =0.

Tolerances: those of tests/test_gpu_target_msa.py -- exact fp32 products with fp32 accumulation, in another summation order
than the reference's: relative L2 error 2e-5 for outputs (lse is one), 1e-4 for gradients; the same formula in numpy float32
stays below 1.7e-6 / 9.5e-6 on these inputs (test_msa_lean_cpu.py prints it).  Each tensor is also held to the same bound
per (b, head, 32-row block) slice on the whole tensor's scale (msa_lean_cases.worst_block).
"""
import copy
import ctypes
import gc
import os
import sys

import numpy as np
import pytest
import torch

import msa_lean_cases as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))

GUARD = 4096


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _has_msa_node(t):
    """True when the msa autograd node is t's grad_fn or one of its first two ancestors (a layout copy may follow it)."""
    fns = [t.grad_fn]
    for _ in range(3):
        nxt = []
        for f in fns:
            if f is None:
                continue
            if type(f).__name__ == 'MsaLayerBackward':
                return True
            nxt += [g for g, _ in f.next_functions if g is not None]
        fns = nxt
    return False


def _guarded(n):
    """n floats of NaN sentinel followed by a guard region of GUARD more."""
    return torch.full((n + GUARD,), float('nan'), dtype=torch.float32, device='cuda')


def _entry_points(case, qkv, dO):
    """One forward and backward through the C entry points into sentinel-filled, guarded buffers: out, lse, dqkv."""
    from ghn3_amd import _lib as L
    from ghn3_amd import target_ops as T
    B, H, N, d, _ = case
    C = H * d
    lib = L.load()
    out, lse, dqkv = _guarded(B * N * C), _guarded(B * H * N), _guarded(B * N * 3 * C)
    L._check(lib.ghn3_attn_lean_fwd(out.data_ptr(), lse.data_ptr(), qkv.data_ptr(), B, N, C, H, T._stream()), 'ghn3_attn_lean_fwd')
    L._check(lib.ghn3_attn_lean_bwd(dqkv.data_ptr(), dO.data_ptr(), qkv.data_ptr(), lse.data_ptr(), out.data_ptr(), B, N, C, H,
                                    T._stream()), 'ghn3_attn_lean_bwd')
    torch.cuda.synchronize()
    for name, t in (('out', out), ('lse', lse), ('dqkv', dqkv)):
        assert not bool(torch.isnan(t[:-GUARD]).any()), '%s: an element was not written' % name
        assert bool(torch.isnan(t[-GUARD:]).all()), '%s: the guard region was written' % name
    return out[:-GUARD].view(B, N, C), lse[:-GUARD].view(B, H, N), dqkv[:-GUARD].view(B, N, 3 * C)


@pytest.mark.parametrize('case', M.OP_CASES)
def test_lean_attention_matches_float64(case):
    from ghn3_amd import target_ops as T
    B, H, N, d, _ = case
    C = H * d
    q, k, v, g = M.inputs(case)
    ref = M.reference(case)
    qkv = torch.from_numpy(M.pack_qkv(q, k, v)).cuda()
    dO = torch.from_numpy(M.pack_heads(g)).cuda()
    out, lse, dqkv = _entry_points(case, qkv, dO)
    out2, lse2, dqkv2 = _entry_points(case, qkv, dO)
    assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2)
    # the public op: the same kernels behind autograd
    x = qkv.clone().requires_grad_(True)
    y = T.lean_attention(x, H)
    y.backward(dO)
    torch.cuda.synchronize()
    assert y.shape == (B, N, C) and torch.equal(y.detach(), out) and torch.equal(x.grad, dqkv)
    with torch.no_grad():
        assert torch.equal(T.lean_attention(qkv, H), out)

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
            # exact zeros in float64: an absolute bound on the scale of the terms that cancel
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


# ---- the layer ------------------------------------------------------------------------------------------------------------
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


def _run(layer, x, up):
    x = x.clone().requires_grad_(True)
    out = layer(x)
    (out * up).sum().backward()
    return out, x.grad, [p.grad for _, p in layer.named_parameters()]


LAYER_CASES = [   # B, C, H, W, stride, channels_last, mlp_ratio, qkv_bias
    (64, 32, 11, 11, 1, False, 1, False),
    (4, 256, 7, 7, 2, False, 1, False),       # head dim 32, stride 2
    (3, 48, 5, 7, 2, True, 1, False),         # head dim 6, odd grid
    (2, 64, 1, 1, 1, False, 1, False),        # a single token
    (6, 64, 8, 8, 1, True, 4, False),         # mlp_ratio 4: hidden 256
    (5, 32, 9, 9, 1, False, 1, True),         # QKV bias
]


@pytest.mark.parametrize('case', LAYER_CASES)
def test_lean_msa_layer_matches_float64(case, monkeypatch):
    monkeypatch.setenv('GHN3_MSA_LEAN', '1')
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
    import ghn3_amd.target_ops as T
    calls = []
    orig = T._scratch_floats
    monkeypatch.setattr(T, '_scratch_floats', lambda fn, d, b: (calls.append(fn), orig(fn, d, b))[1])
    out = dev(xd)
    assert _has_msa_node(out), 'the layer did not run on the fused op'
    (out * up.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    assert calls == ['ghn3_msa_lean_scratch_floats'] * 2, calls          # (forward and backward took the lean entry points)
    assert out.shape == o_ref.shape
    assert _rel(out.detach().cpu(), o_ref.detach()) < 2e-5, _rel(out.detach().cpu(), o_ref.detach())
    assert _rel(xd.grad.cpu(), dx_ref) < 1e-4, _rel(xd.grad.cpu(), dx_ref)
    names = [n for n, _ in ref.named_parameters()]
    assert len(names) == 11 + int(qb)
    for n, a, b in zip(names, [p.grad for _, p in dev.named_parameters()], g_ref):
        assert a is not None and a.data_ptr() != xd.grad.data_ptr(), n
        assert _rel(a.cpu(), b) < 1e-4, (n, _rel(a.cpu(), b))
    # the inference forward takes the same attention kernel: bit-equal; and a second run repeats the first
    with torch.no_grad():
        assert torch.equal(dev(xd), out.detach())
    dx1 = xd.grad.clone()
    xd.grad = None
    out_b = dev(xd)
    (out_b * up.float().cuda()).sum().backward()
    assert torch.equal(out_b.detach(), out.detach()) and torch.equal(xd.grad, dx1)


def test_lean_forward_keeps_no_square_matrix(monkeypatch):
    """Layer (B = 8, C = 32, 32 x 32 maps): P would be 8 * 8 * 1024^2 floats = 256 MB."""
    import ghn3_amd.target_ops as T
    from ghn3_amd import _lib as L
    B, C, H, W = 8, 32, 32, 32
    dev = _layer(C, 1, seed=9).float().cuda()
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(1)).cuda().requires_grad_(True)
    d = T._MsaDesc(B, H, W, C, M.HEADS, C, 1, H, W, 0, 1e-5, 0)
    scratch = int(L.load().ghn3_msa_lean_scratch_floats(ctypes.byref(d), 0))
    assert scratch > 0
    p_bytes = 4 * B * M.HEADS * (H * W) ** 2
    assert p_bytes == 256 * 2 ** 20
    # (unreachable cycles that earlier tests left hold device memory until the collector runs: were that inside a measured
    # forward, what it frees would be taken off that forward's growth)
    gc.collect()
    grown = {}
    for mode in ('1', '0'):
        monkeypatch.setenv('GHN3_MSA_LEAN', mode)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        out = dev(x)
        torch.cuda.synchronize()
        grown[mode] = torch.cuda.memory_allocated() - before
        assert _has_msa_node(out)
        del out
    allowed = 4 * scratch + 4 * B * C * H * W + x.numel() * 4 + 8 * 2 ** 20
    print('forward keeps %.1f MB lean (allowed %.1f MB), %.1f MB with P saved' % (grown['1'] / 2 ** 20, allowed / 2 ** 20,
                                                                             grown['0'] / 2 ** 20))
    assert allowed < p_bytes / 4
    assert grown['1'] <= allowed, (grown['1'], allowed)
    assert grown['0'] >= p_bytes, grown['0']            # the control: the measure sees P when it is there


def test_lean_reaches_a_shape_the_saved_p_path_refuses(monkeypatch):
    """Layer (B = 16, C = 32, 64 x 64 maps) under the default setting: B heads N^2 = 2^31.  The layer is per-sample, so its
    first two samples must agree with the layer run on those two alone on the saved-P path (1 GB of P): 4e-5 / 2e-4, twice the
    float64 bounds, since either path is within one of them."""
    import ghn3_amd.target_ops as T
    monkeypatch.delenv('GHN3_MSA_LEAN', raising=False)
    B, C, H, W = 16, 32, 64, 64
    assert B * M.HEADS * (H * W) ** 2 >= 2 ** 31 and T.msa_lean(B, M.HEADS, H * W)
    dev = _layer(C, 1, seed=4).float().cuda()
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, C, H, W, generator=g).cuda()
    up = torch.randn(B, C, H, W, generator=g).cuda()
    xa = x.clone().requires_grad_(True)
    out = dev(xa)
    assert _has_msa_node(out), 'the layer did not run on the fused op'
    (out * up).sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(xa.grad).all())
    out2, dx2 = out.detach()[:2].clone(), xa.grad[:2].clone()
    del out, xa
    monkeypatch.setenv('GHN3_MSA_LEAN', '0')
    xb = x[:2].clone().requires_grad_(True)
    o_ref = dev(xb)
    assert _has_msa_node(o_ref)
    (o_ref * up[:2]).sum().backward()
    torch.cuda.synchronize()
    e_out, e_dx = _rel(out2, o_ref.detach()), _rel(dx2, xb.grad)
    print('lean (B = 16) against saved-P (B = 2): out %.2e, dx %.2e' % (e_out, e_dx))
    assert e_out < 4e-5 and e_dx < 2e-4, (e_out, e_dx)


# ---- a whole network --------------------------------------------------------------------------------------------------------
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


def test_vit_network_lean_matches_saved_p(monkeypatch):
    """The light ViT-style network of test_gpu_target_msa.py's whole-network test, forward and backward, under GHN3_MSA_LEAN=1
    against =0, at that test's fused-versus-stock tolerance."""
    import network_cases
    import recipe
    import ghn3_amd.target_ops as T
    from ghn3_amd import ops
    geno, kw, img = network_cases.CASES['vit']
    kws = {k: ('bn' if (k == 'norm' and v) else v) for k, v in kw.items()}
    x = torch.from_numpy(recipe.seeded_images(img, seed=7)).cuda()
    res = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('GHN3_MSA_LEAN', mode)
        net = ops.NetworkLight(genotype=ops.Genotype(**geno), **kws)
        leaves = _light_params(net, len('vit'))
        net.train()
        calls = []
        orig = T._scratch_floats
        monkeypatch.setattr(T, '_scratch_floats', lambda fn, d, b, orig=orig: (calls.append(fn), orig(fn, d, b))[1])
        torch.manual_seed(123)
        logits, aux = net(x)
        loss = logits.square().mean() + (aux.square().mean() if aux is not None else 0.)
        loss.backward()
        torch.cuda.synchronize()
        monkeypatch.setattr(T, '_scratch_floats', orig)
        res[mode] = (logits.detach().cpu(), [p.grad.detach().cpu() if p.grad is not None else None for p in leaves],
                     sum(1 for c in calls if c == 'ghn3_msa_lean_scratch_floats'),
                     sum(1 for c in calls if c == 'ghn3_msa_scratch_floats'))
    (l0, g0, lean0, saved0), (l1, g1, lean1, saved1) = res['0'], res['1']
    assert lean0 == 0 and saved0 > 0 and lean1 == saved0 and saved1 == 0, (lean0, saved0, lean1, saved1)
    assert _rel(l1, l0) < 1e-3, _rel(l1, l0)
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if a is not None and float(b.norm()) > 0:
            assert _rel(a, b) < 2e-3, _rel(a, b)
