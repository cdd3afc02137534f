"""
The patch embedding of the ImageNet-sized ViT-style networks on the native op (ghn3_patch_fwd / _bwd, target_ops.PatchEmbed;
rows: tests/patch_cases.py).

  1. op level against torch.nn.functional.conv2d in float64 on the same inputs.  Measure, gates (2e-4 for the output, 3e-4 for dx
     and dw: the conv_only family's own) and the variant with every buffer pre-filled with NaN are those of
     tests/test_gpu_target_edges.py.  Every row runs with x.requires_grad on and off, twice for equal bits, and under
     torch.no_grad; pixels no window reaches have dx == 0 exactly.
  2. the layer alone through run_conv_layer, both flavours: the new node and no stock convolution in the graph, GHN3_NATIVE_STEM=0
     and GHN3_NATIVE_OPS=0 restore the stock graph and bits, the CIFAR patch embedding keeps the dense-convolution node and its bits.
  3. one ImageNet-sized ViT-style network per flavour against the stock path in float64, without a stock convolution call.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import patch_cases as Pc
import recipe
import target_edge_cases as E
from test_gpu_target_edges import buffers, _measure, _report, _graph_nodes    # noqa: F401 (`buffers`: fixture)
from test_gpu_target_edges import OUT_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


# ---- 1. op rows ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(row, dead=None):
    """Inputs and the fp64 results of a row: (x, w, up), z, dx, dw."""
    x, w, up = Pc.inputs(row, dead)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv2d(xr, wr, None, row[5])
    (ref * up.double()).sum().backward()
    return (x, w, up), ref.detach(), xr.grad, wr.grad


def _run_row(row, dead=None):
    from ghn3_amd import target_ops as T
    N, Ci, H, W, k, st, Co, cl = row
    (x, w, up), ref, ref_dx, ref_dw = _reference(row, dead)
    gaps = ~Pc.covered(row)
    worst, first = {}, None
    for x_grad in (True, False):
        runs = []
        for _ in range(2):
            xd = x.cuda().contiguous(memory_format=torch.channels_last) if cl else x.cuda()
            xd.requires_grad_(x_grad)
            wd = w.cuda().requires_grad_(True)
            assert T.PatchEmbed.applicable(xd, wd, st, 0, 1) and not T.ConvOnly.applicable(xd, wd)
            out = T.patch_embed(xd, wd, st)
            assert type(out.grad_fn).__name__ == 'PatchEmbedBackward'
            assert len(out.grad_fn.saved_tensors) == 2                         # x and the weight: nothing else is kept
            assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
            (out * up.cuda()).sum().backward()
            torch.cuda.synchronize()
            if x_grad:
                assert xd.grad.stride() == xd.stride()                         # dx in the image's own layout
            else:
                assert xd.grad is None
            assert wd.grad.is_contiguous() and wd.grad.untyped_storage().nbytes() == 4 * wd.numel()   # a tensor of its own
            runs.append((out.detach().cpu(), None if xd.grad is None else xd.grad.cpu(), wd.grad.cpu()))
        (out, dx, dw), (out2, dx2, dw2) = runs
        assert torch.equal(out2, out) and torch.equal(dw2, dw) and (dx is None or torch.equal(dx2, dx))
        if first is not None:
            assert torch.equal(out, first[0]) and torch.equal(dw, first[1])    # the same bits with and without dx
        first = (out, dw)
        _measure('patch', 'out', out, ref, E.ACT_AXES, OUT_TOL, worst)
        _measure('patch', 'dw', dw, ref_dw, E.WGRAD_AXES, GRAD_TOL, worst)
        if x_grad:
            _measure('patch', 'dx', dx, ref_dx, E.ACT_AXES, GRAD_TOL, worst)
            assert torch.equal(dx[:, :, gaps], torch.zeros_like(dx[:, :, gaps]))          # exactly 0 where no window reaches
        if dead is not None:
            assert torch.equal(out[:, dead], torch.zeros_like(out[:, dead]))
    with torch.no_grad():
        xd = x.cuda().contiguous(memory_format=torch.channels_last) if cl else x.cuda()
        out = T.patch_embed(xd, w.cuda(), st)
        assert out.grad_fn is None and torch.equal(out.cpu(), first[0])
    _report('patch', row, worst)
    return first


@pytest.mark.parametrize('row', Pc.ROWS, ids=str)
def test_patch_rows_against_fp64(row, buffers):
    _run_row(row)


def test_patch_with_a_zero_output_channel(buffers):
    """A zero weight channel: z is exactly 0 there (asserted in the row's run), and under a loss that reaches the weight through z
    alone -- sum(up z^2) / 2, dz = up z -- that channel's dz and with it its dw = sum_p dz[p][co] x[p] are exactly 0."""
    from ghn3_amd import target_ops as T
    row, dead = Pc.DEAD
    _run_row(row, dead)
    x, w, up = Pc.inputs(row, dead)
    xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    out = T.patch_embed(xd, wd, row[5])
    (0.5 * out.square() * up.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(out[:, dead].cpu(), torch.zeros_like(up[:, dead]))
    assert torch.equal(wd.grad[dead].cpu(), torch.zeros_like(w[dead]))
    assert float(wd.grad.abs().sum()) > 0 and torch.isfinite(wd.grad).all() and torch.isfinite(xd.grad).all()


# ---- 2. the layer alone ----------------------------------------------------------------------------------------------------
def _run_layer(light, k, st, pad, side):
    from ghn3_amd import light_ops, target_ops as T
    gen = torch.Generator().manual_seed(31)
    w = torch.randn(32, 3, k, k, generator=gen) / float(3 * k * k) ** 0.5
    if light:
        conv = light_ops.Conv2d(3, 32, k, stride=st, padding=pad, bias=False)
        flat = torch.zeros(3 + w.numel(), device='cuda')
        flat[3:] = w.reshape(-1).cuda()
        flat.requires_grad_(True)                                              # the leaf: the weight is a view of it, 12 bytes in
        conv.weight = flat[3:].view(w.shape)
        leaf = flat
    else:
        conv = torch.nn.Conv2d(3, 32, k, stride=st, padding=pad, bias=False).cuda()
        with torch.no_grad():
            conv.weight.copy_(w)
        leaf = conv.weight
    x = torch.randn(2, 3, side, side, generator=gen).cuda().requires_grad_(True)
    y = T.run_conv_layer(conv, x)
    up = torch.randn(y.shape, generator=gen).cuda()
    (y * up).sum().backward()
    torch.cuda.synchronize()
    assert y.is_contiguous()                                                   # the layout pos_enc is handed today
    return y.detach().cpu(), x.grad.cpu(), leaf.grad.cpu(), _graph_nodes(y), (conv, x)


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
def test_the_imagenet_patch_embedding_runs_on_the_native_node(light, monkeypatch):
    for var in ('GHN3_NATIVE_OPS', 'GHN3_NATIVE_STEM', 'GHN3_NATIVE_CONV'):
        monkeypatch.delenv(var, raising=False)
    fused = _run_layer(light, 16, 16, 0, 32)
    monkeypatch.setenv('GHN3_NATIVE_OPS', '0')
    stock = _run_layer(light, 16, 16, 0, 32)
    monkeypatch.delenv('GHN3_NATIVE_OPS')
    monkeypatch.setenv('GHN3_NATIVE_STEM', '0')
    off = _run_layer(light, 16, 16, 0, 32)
    assert fused[3].count('PatchEmbedBackward') == 1 and 'ConvolutionBackward0' not in fused[3], fused[3]
    for res in (stock, off):
        assert 'ConvolutionBackward0' in res[3] and 'PatchEmbed' not in res[3] and 'ConvOnly' not in res[3], res[3]
    for a, b in zip(off[:3], stock[:3]):
        assert torch.equal(a, b)
    print('light' if light else 'torch', 'out %.2e dx %.2e dw %.2e' % tuple(_rel(a, b) for a, b in zip(fused[:3], stock[:3])))
    assert fused[0].shape == stock[0].shape and _rel(fused[0], stock[0]) < 2e-4
    assert _rel(fused[1], stock[1]) < 5e-4 and _rel(fused[2], stock[2]) < 5e-4
    if light:
        assert torch.equal(fused[2][:3], torch.zeros(3))                       # the leaf's elements outside the view


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
def test_the_cifar_patch_embedding_keeps_the_dense_convolution_node(light, monkeypatch):
    from ghn3_amd import target_ops as T
    for var in ('GHN3_NATIVE_OPS', 'GHN3_NATIVE_STEM', 'GHN3_NATIVE_CONV'):
        monkeypatch.delenv(var, raising=False)
    y, dx, dw, nodes, (conv, x) = _run_layer(light, 3, 3, 1, 32)
    assert nodes.count('ConvOnlyBackward') == 1 and 'PatchEmbed' not in nodes and 'ConvolutionBackward0' not in nodes, nodes
    with torch.no_grad():
        want = T.conv_only(F.pad(x, (0, 0, 0, 0, 0, 1)), F.pad(conv.weight, (0, 0, 0, 0, 0, 1)), 3, 1, 1, relu=False)
    assert torch.equal(y, want.contiguous(memory_format=torch.contiguous_format).cpu())


# ---- 3. a whole ImageNet-sized ViT-style network per flavour -----------------------------------------------------------------
class _ConvCalls:
    """Counts the stock convolution calls: torch.nn.functional.conv2d (what both flavours' Conv2d end in) and the forward of the
    light Conv2d (as tools/diag/stock_layer_census.py counts them)."""

    def __init__(self, monkeypatch):
        from ghn3_amd import light_ops
        self.n = 0
        monkeypatch.setattr(F, 'conv2d', self._counted(F.conv2d))
        monkeypatch.setattr(light_ops.Conv2d, 'forward', self._counted(light_ops.Conv2d.forward))

    def _counted(self, fn):
        def call(*args, **kwargs):
            self.n += 1
            return fn(*args, **kwargs)
        return call


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
def test_an_imagenet_vit_network_runs_without_a_stock_convolution(light, monkeypatch):
    """C = 32, one cell (msa + skip), two 224 x 224 images: 16 x 16 patches -> 14 x 14 tokens.  Filled in and bounded as
    test_gpu_target_wide.test_a_wide_network_runs_without_a_stock_convolution: the stock path (GHN3_NATIVE_OPS=0) runs in float64
    (the classifier stays fp32: the network casts its input), logits within 1e-3, every parameter gradient within 2e-3.
    Measured on an MI355X: see DESIGN 3, "patch embedding of ImageNet-sized ViT-style networks"."""
    import network_cases
    from ghn3_amd import ops
    g = ops.Genotype(**network_cases._VIT)
    kw = dict(C=32, num_classes=10, n_cells=1, is_imagenet_input=True, norm='bn', preproc=False, C_mult=1)
    for var in ('GHN3_NATIVE_STEM', 'GHN3_NATIVE_CONV'):
        monkeypatch.delenv(var, raising=False)
    calls = _ConvCalls(monkeypatch)
    res = {}
    for mode in ('stock', 'fused'):
        monkeypatch.setenv('GHN3_NATIVE_OPS', '0' if mode == 'stock' else '1')
        torch.manual_seed(0)
        net = (ops.NetworkLight if light else ops.Network)(genotype=g, **kw)
        assert net._is_vit and net.expected_input_sz == 224
        dt = torch.float64 if mode == 'stock' else torch.float32
        x = torch.from_numpy(recipe.seeded_images((2, 3, 224, 224), seed=7)).cuda().to(dt)
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
        n_calls, nodes = calls.n, _graph_nodes(logits)
        logits.square().mean().backward()
        torch.cuda.synchronize()
        res[mode] = (logits.detach().cpu(), [None if p.grad is None else p.grad.detach().cpu() for p in leaves], n_calls, nodes)
    (l0, g0, n0, nodes0), (l1, g1, n1, nodes1) = res['stock'], res['fused']
    print('light' if light else 'torch', 'stock conv2d calls: %d on the stock path, %d native' % (n0, n1), 'logits %.2e' % _rel(l1, l0))
    assert n0 > 0 and n1 == 0, (n0, n1)
    assert 'ConvolutionBackward0' in nodes0 and 'ConvolutionBackward0' not in nodes1, nodes1
    assert nodes1.count('PatchEmbedBackward') == 1, nodes1
    assert torch.isfinite(l0).all() and float(l0.norm()) > 0
    assert _rel(l1, l0) < 1e-3, _rel(l1, l0)
    worst = 0.0
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if a is not None and float(b.norm()) > 0:
            worst = max(worst, _rel(a, b))
    print('worst parameter gradient %.2e' % worst)
    assert worst < 2e-3, worst
