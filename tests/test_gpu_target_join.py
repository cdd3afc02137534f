"""GPU checks of the target-network joins: target_ops.pair_sum / cell_concat / join / pos_enc (ghn3_join_fwd / _bwd,
ghn3_posenc_bwd; ghn3_amd/csrc/tnet_join.hip) and their wiring into ops._Cell / ops._PosEnc.

Every output element of a join is one fp32 add or a copy, so the comparisons with the torch expressions are bit for bit
(tolerance zero, derived); only the positional encoding's weight gradient is a sum, bounded by the worst case of an fp32 sum of
N terms."""

import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NCHW, NHWC = 0, 1
LAYOUTS = [(a, b, o) for a in (NCHW, NHWC) for b in (NCHW, NHWC) for o in (NCHW, NHWC)]


def _store(t, layout):
    return t.contiguous(memory_format=torch.channels_last if layout else torch.contiguous_format)


def _tensor(shape, layout, seed, special=True):
    """Seeded normals with one inf and one -0.0 at pixels every step-2 read keeps, stored in `layout`, requiring a gradient."""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    if special:
        t[0, 0, 0, 0] = float('inf')
        t[-1, -1, 0, 0] = -0.0
    return _store(t.cuda(), layout).requires_grad_(True)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _is_layout(t, layout):
    return t.is_contiguous(memory_format=torch.channels_last if layout else torch.contiguous_format)


def _check_join(slices, lo):
    """T.join of `slices` against the torch expression: output and, for dout in either layout, every source's gradient."""
    from ghn3_amd import target_ops as T
    y = T.join(slices, nhwc=bool(lo))
    assert y is not None and _is_layout(y, lo)
    ref = torch.cat([a[:, :, ::sa, ::sa] + b[:, :, ::sb, ::sb] if b is not None else a[:, :, ::sa, ::sa]
                     for a, b, sa, sb in slices], dim=1)
    assert _same(y, ref)
    srcs = []
    for a, b, _, _ in slices:
        srcs += [t for t in (a, b) if t is not None and not any(t is u for u in srcs)]
    up = torch.randn(ref.shape, generator=torch.Generator().manual_seed(99))
    up[0, 0, 0, 0] = -0.0
    want = torch.autograd.grad(ref, srcs, up.cuda())
    for dlo in (NCHW, NHWC):
        got = torch.autograd.grad(y, srcs, _store(up.cuda(), dlo), retain_graph=True)
        for t, g, w in zip(srcs, got, want):
            assert _same(g, w)                                       # (zeros at the pixels a step-2 read skipped included)
            assert g.is_contiguous() or g.is_contiguous(memory_format=torch.channels_last)
    return y


SUM_SHAPES = [(2, 12, 3, 3), (3, 36, 9, 9), (3, 4, 9, 9)]


@pytest.mark.parametrize('la,lb,lo', LAYOUTS)
@pytest.mark.parametrize('shape', SUM_SHAPES)
def test_pair_sum_is_exact(shape, la, lb, lo):
    from ghn3_amd import target_ops as T
    a, b = _tensor(shape, la, 1), _tensor(shape, lb, 2)
    _check_join([(a, b, 1, 1)], lo)
    y = T.pair_sum(a, b, nhwc=bool(lo))
    assert _same(y, a + b) and float(y.detach()[-1, -1, 0, 0]) == 0.0 and _bits(y.detach())[-1, -1, 0, 0] == -2 ** 31     # -0.0 + -0.0
    assert type(y.grad_fn).__name__.startswith('Join')


@pytest.mark.parametrize('la,lb,lo', LAYOUTS)
@pytest.mark.parametrize('side', [3, 4])
def test_pair_sum_reads_at_step_two(side, la, lb, lo):
    """`[:, :, ::2, ::2]` of a 3 x 3 and of a 4 x 4 source (the odd and the even rounding) added to a 2 x 2 tensor, and of
    both sources; the gradient of a strided source is dout spread over zeros."""
    a, b = _tensor((2, 8, side, side), la, 3), _tensor((2, 8, 2, 2), lb, 4)
    _check_join([(a, b, 2, 1)], lo)
    _check_join([(b, a, 1, 2)], lo)
    _check_join([(a, _tensor((2, 8, 7 - side, 7 - side), lb, 5), 2, 2)], lo)    # (a 3 x 3 with a 4 x 4 and the reverse)
    big = _tensor((3, 20, 4 * side + 1, 4 * side + 1), la, 6)                   # (more than one workgroup at step 2)
    _check_join([(big, _tensor((3, 20, 2 * side + 1, 2 * side + 1), lb, 7), 2, 1)], lo)


@pytest.mark.parametrize('la,lb,lo', LAYOUTS)
@pytest.mark.parametrize('N,side,Cs', [(2, 3, (4, 8, 12)), (3, 9, (36, 4, 20))])
def test_cell_concat_is_exact(N, side, Cs, la, lb, lo):
    from ghn3_amd import target_ops as T
    states = [_tensor((N, C, side, side), (la, lb, la)[j], 10 + j) for j, C in enumerate(Cs)]
    _check_join([(t, None, 1, 1) for t in states], lo)
    y = T.cell_concat(states, nhwc=bool(lo))
    assert _same(y, torch.cat(states, dim=1)) and _is_layout(y, lo)


@pytest.mark.parametrize('la,lb,lo', LAYOUTS)
def test_single_and_two_source_slices_side_by_side(la, lb, lo):
    a0, b0 = _tensor((3, 36, 9, 9), la, 20), _tensor((3, 36, 9, 9), lb, 21)
    a1 = _tensor((3, 4, 9, 9), lb, 22)
    a2, b2 = _tensor((3, 20, 9, 9), lb, 23), _tensor((3, 20, 17, 17), la, 24)
    _check_join([(a0, b0, 1, 1), (a1, None, 1, 1), (a2, b2, 1, 2)], lo)
    _check_join([(a1, None, 1, 1), (a0, b0, 1, 1)], lo)


@pytest.mark.parametrize('la,lo', [(a, o) for a in (NCHW, NHWC) for o in (NCHW, NHWC)])
def test_the_same_tensor_on_both_sides_of_a_sum(la, lo):
    from ghn3_amd import target_ops as T
    a = _tensor((2, 12, 3, 3), la, 30)
    y = T.pair_sum(a, a, nhwc=bool(lo))
    assert _same(y, a + a)
    up = torch.randn(a.shape, generator=torch.Generator().manual_seed(31)).cuda()
    for dlo in (NCHW, NHWC):
        g, = torch.autograd.grad(y, [a], _store(up, dlo), retain_graph=True)
        assert _same(g, 2 * up)


def test_a_sum_hands_dout_itself_to_a_source_of_its_layout():
    """The backward of a sum launches nothing for a source stored as dout is and read at step 1: it receives dout itself."""
    from ghn3_amd import target_ops as T
    a, b = _tensor((2, 8, 5, 5), NHWC, 40), _tensor((2, 8, 5, 5), NCHW, 41)
    seen = {}
    a.register_hook(lambda g: seen.__setitem__('a', g.data_ptr()))
    b.register_hook(lambda g: seen.__setitem__('b', g.data_ptr()))
    up = _store(torch.randn(2, 8, 5, 5, device='cuda'), NHWC)
    T.pair_sum(a, b, nhwc=True).backward(up)
    assert seen['a'] == up.data_ptr() and seen['b'] != up.data_ptr()
    assert _same(a.grad, up) and _same(b.grad, up) and b.grad.is_contiguous()


@pytest.mark.parametrize('lx,lo', [(a, o) for a in (NCHW, NHWC) for o in (NCHW, NHWC)])
@pytest.mark.parametrize('C,ks', [(8, 3), (32, 11)])
@pytest.mark.parametrize('N', [1, 2, 64])
def test_pos_enc(N, C, ks, lx, lo):
    from ghn3_amd import target_ops as T
    x = _tensor((N, C, ks, ks), lx, 50)
    # (the weight as the GHN assigns it: a view of a flat buffer that starts on no particular boundary)
    flat = torch.randn(C * ks * ks + 3, generator=torch.Generator().manual_seed(51)).cuda().requires_grad_(True)
    w = flat[3:].view(1, C, ks, ks)
    y = T.pos_enc(x, w, nhwc=bool(lo))
    assert y is not None and _same(y, x + w) and _is_layout(y, lo)
    assert _is_layout(T.pos_enc(x, w), lx)                           # (stored as x is unless told otherwise)
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(52)).cuda()
    exact = dy.double().sum(0, keepdim=True)
    bound = N * 2.0 ** -24 * dy.double().abs().sum(0, keepdim=True)  # worst case of an fp32 sum of N terms
    runs = []
    for dlo in (NCHW, NHWC, NCHW):
        dx, dflat = torch.autograd.grad(y, [x, flat], _store(dy, dlo), retain_graph=True)
        assert _same(dx, dy)
        assert float(dflat[:3].abs().max()) == 0.0
        dw = dflat[3:].view(1, C, ks, ks)
        err = (dw.double() - exact).abs()
        print('pos_enc dw N=%d C=%d ks=%d: max err %.3e, max err / bound %.3f' % (N, C, ks, float(err.max()),
                                                                                float((err / bound).max())))
        assert bool((err <= bound).all())
        runs.append(dw.clone())
    assert _same(runs[0], runs[1]) and _same(runs[0], runs[2])       # fixed summation order: bit-identical in every run
    if N == 1:
        assert _same(runs[0], dy)


# ---- wiring ----------------------------------------------------------------------------------------------------------------
_CONV_GENO = dict(normal=[('sep_conv_3x3', 0), ('skip_connect', 1), ('max_pool_3x3', 0), ('sep_conv_3x3', 2)],
                  normal_concat=[2, 3],
                  reduce=[('skip_connect', 0), ('max_pool_3x3', 1), ('sep_conv_3x3', 0), ('skip_connect', 2)],
                  reduce_concat=[2, 3])
_CONV_KW = dict(C=16, num_classes=10, n_cells=3, is_imagenet_input=False, norm='bn')
_VIT_GENO = dict(normal=[('msa', 0), ('skip_connect', 1)], normal_concat=[2], reduce=[('msa', 0), ('msa', 1)], reduce_concat=[2])
_VIT_KW = dict(C=32, num_classes=10, n_cells=3, is_imagenet_input=False, norm='bn', preproc=False, C_mult=1)


def _build(light, geno, kw, seed):
    """A network with seeded weights, filled in as test_gpu_target_ops.test_networks_on_the_fused_layers_match_the_stock_path
    does (light flavour: views of one flat buffer, as a GHN assigns them); returns (net, leaves)."""
    import recipe
    from ghn3_amd import ops
    net = (ops.NetworkLight if light else ops.Network)(genotype=ops.Genotype(**geno), **kw)
    if light:
        table = {}
        for cell in net._layered_modules:
            table.update(cell)
        shapes = [(n, tuple(e['sz'])) for n, e in table.items()]
        params = recipe.seeded_net_params(shapes, seed=seed)
        flat = torch.cat([torch.from_numpy(params[n]).reshape(-1) for n, _ in shapes]).cuda().requires_grad_(True)
        off = 0
        for n, s in shapes:
            k = int(np.prod(s))
            e = table[n]
            setattr(e['module'], 'weight' if e['is_w'] else 'bias', flat[off:off + k].view(s))
            off += k
        return net, [flat]
    net = net.cuda()
    params = recipe.seeded_net_params([(n, tuple(p.shape)) for n, p in net.named_parameters()], seed=seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(params[n]))
    return net, [p for _, p in net.named_parameters()]


def _strided_vit(net):
    """`msa` at stride 2 in the reduction cells of a ViT-style network (the search space strides only convolutional networks):
    cell 1 halves both of its inputs, cell 2 the older one (cell 0's output, still at full size)."""
    net.cells[1]._ops[0].stride = net.cells[1]._ops[1].stride = net.cells[2]._ops[0].stride = 2
    return net


def _run(light, geno, kw, monkeypatch, native, prepare=None):
    import recipe
    from ghn3_amd import ops
    monkeypatch.setenv('GHN3_NATIVE_JOIN', '1' if native else '0')
    net, leaves = _build(light, geno, kw, seed=3)
    if prepare is not None:
        prepare(net)
    net.train()
    x = torch.from_numpy(recipe.seeded_images((4, 3, 32, 32), seed=7)).cuda().requires_grad_(True)
    cats, cell_outs = [], []
    real_cat, real_forward = torch.cat, ops._Cell.forward

    def counted_cat(*args, **kwargs):
        fr = sys._getframe(1)
        if fr.f_code is real_forward.__code__:
            cats.append(1)
        return real_cat(*args, **kwargs)

    def watched_forward(self, *args, **kwargs):
        y = real_forward(self, *args, **kwargs)
        cell_outs.append(y)
        return y
    monkeypatch.setattr(torch, 'cat', counted_cat)
    monkeypatch.setattr(ops._Cell, 'forward', watched_forward)
    torch.manual_seed(123)
    logits, _ = net(x)
    monkeypatch.setattr(torch, 'cat', real_cat)
    monkeypatch.setattr(ops._Cell, 'forward', real_forward)
    logits.square().mean().backward()
    torch.cuda.synchronize()
    grads = [x.grad] + [p.grad for p in leaves]
    return logits.detach(), grads, len(cats), cell_outs


def _assert_same_run(r1, r0):
    assert torch.equal(r1[0], r0[0])
    assert len(r1[1]) == len(r0[1])
    for a, b in zip(r1[1], r0[1]):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a, b)


@pytest.mark.parametrize('light', [False, True])
def test_convolutional_network_with_native_joins_equals_the_stock_glue(light, monkeypatch):
    """C = 16, three cells (the search space reduces in cells 1 and 2 of three), 32 x 32 input, batch 4; a `skip_connect` at
    stride 2, a `max_pool` and a `sep_conv` in the genotype: logits, input gradient and every parameter gradient with
    GHN3_NATIVE_JOIN=1 are those with =0, no torch.cat is called from a cell, and every cell's output is stored as the next
    layers take it (channels_last in the light flavour, plain NCHW in the torch.nn one)."""
    r0 = _run(light, _CONV_GENO, _CONV_KW, monkeypatch, native=False)
    r1 = _run(light, _CONV_GENO, _CONV_KW, monkeypatch, native=True)
    assert r0[2] == 3 and r1[2] == 0
    _assert_same_run(r1, r0)
    assert len(r1[3]) == 3
    for y in r1[3]:
        assert type(y.grad_fn).__name__.startswith('Join')
        assert _is_layout(y, NHWC if light else NCHW) and not _is_layout(y, NCHW if light else NHWC)


@pytest.mark.parametrize('light', [False, True])
def test_vit_network_with_native_joins_equals_the_stock_glue(light, monkeypatch):
    """A ViT-style network (patch stem, PosEnc, `msa` cells, `msa` at stride 2 in the reduction cells)."""
    r0 = _run(light, _VIT_GENO, _VIT_KW, monkeypatch, native=False, prepare=_strided_vit)
    r1 = _run(light, _VIT_GENO, _VIT_KW, monkeypatch, native=True, prepare=_strided_vit)
    assert r0[2] == 3 and r1[2] == 0
    _assert_same_run(r1, r0)
    assert [tuple(y.shape[2:]) for y in r1[3]] == [(11, 11), (6, 6), (6, 6)]
    for y in r1[3]:
        assert _is_layout(y, NHWC if light else NCHW) and not _is_layout(y, NCHW if light else NHWC)


def test_pos_enc_module_runs_on_the_native_node(monkeypatch):
    from ghn3_amd import ops
    pe = ops.PosEnc(32, 11).cuda()
    x = torch.randn(4, 32, 11, 11, device='cuda', requires_grad=True)
    y = pe(x)
    assert type(y.grad_fn).__name__.startswith('PosEnc') and torch.equal(y, x + pe.weight) and y.is_contiguous()
    monkeypatch.setenv('GHN3_NATIVE_JOIN', '0')
    assert type(pe(x).grad_fn).__name__.startswith('Add')


# ---- fallback --------------------------------------------------------------------------------------------------------------
def _glue_cell(C):
    """A torch.nn-flavour cell without preprocessing: state 2 = max_pool(s0) + s1, state 3 = s0 + state 2, out = cat(2, 3)."""
    from ghn3_amd import ops
    geno = ops.Genotype(normal=[('max_pool_3x3', 0), ('skip_connect', 1), ('skip_connect', 0), ('skip_connect', 2)],
                        normal_concat=[2, 3], reduce=[('skip_connect', 0), ('skip_connect', 1)], reduce_concat=[2])
    return ops.Cell(geno, C, C, C, C, reduction=False, reduction_prev=False, preproc=False)


def _glue_reference(s0, s1):
    st2 = torch.nn.functional.max_pool2d(s0, 3, 1, 1) + s1
    return torch.cat([st2, s0 + st2], dim=1)


def test_glue_cell_takes_the_native_nodes_where_they_apply():
    s0, s1 = torch.randn(2, 8, 6, 6, device='cuda'), torch.randn(2, 8, 6, 6, device='cuda')
    y = _glue_cell(8)(s0.requires_grad_(True), s1)
    assert type(y.grad_fn).__name__.startswith('Join') and torch.equal(y, _glue_reference(s0, s1))


def test_half_precision_sources_keep_the_stock_expressions():
    from ghn3_amd import target_ops as T
    s0, s1 = torch.randn(2, 8, 6, 6, device='cuda').half(), torch.randn(2, 8, 6, 6, device='cuda').half()
    assert T.pair_sum(s0, s1) is None and T.cell_concat([s0, s1]) is None
    assert T.pos_enc(s0, torch.randn(1, 8, 6, 6, device='cuda').half()) is None
    y = _glue_cell(8)(s0.requires_grad_(True), s1)
    assert y.dtype == torch.float16 and type(y.grad_fn).__name__.startswith('Cat') and torch.equal(y, _glue_reference(s0, s1))


def test_six_channel_slices_keep_the_stock_expressions():
    from ghn3_amd import target_ops as T
    s0, s1 = torch.randn(2, 6, 6, 6, device='cuda'), torch.randn(2, 6, 6, 6, device='cuda')
    assert T.pair_sum(s0, s1) is None and T.cell_concat([s0, s1]) is None
    assert T.join([(torch.randn(2, 8, 6, 6, device='cuda'), None, 1, 1), (s0, None, 1, 1)]) is None
    y = _glue_cell(6)(s0.requires_grad_(True), s1)
    assert type(y.grad_fn).__name__.startswith('Cat') and torch.equal(y, _glue_reference(s0, s1))
