"""
The "bias" member of the dense-convolution family -- conv + bias [+ skip] [-> ReLU] as one node, ghn3_conv_bias_act_*
(ghn3_amd/csrc/target_ops.hip) -- and ghn3_amd.nativize(biased=True) on the GPU.

Every case of tests/bias_cases.py runs against the stock layers in fp64 (tests/util_parity.slice_errors, the slicings of
tests/target_edge_cases.py) at the tolerances the project states for this family: 2e-4 for out, 3e-4 for dx, dw, dbias and dres.
The upstream gradient is zero where the fp64 pre-activation lies within 2e-3 of the ReLU's kink (bias_cases: a condition on the
cases).  Each case runs twice for equal bits, once more with every buffer the op allocates pre-filled with NaN, and after
asserting `applicable(...)`, so that no case tests the stock fallback.

Whole networks: the two networks of the case file, nativized with biased=True, against the same modules on the stock GPU path
at the tolerances of tests/test_gpu_networks.py (loss 2e-4 relative, every gradient within 2e-3 of its norm), the generator
seeded identically before each path so that the Dropout draws coincide (run_classifier_head draws its keep masks with torch's
own dropout kernel, in the order the stock layers do); the plain Trainer branch with native_layers and native_biased against
without.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import bias_cases as B
import target_edge_cases as E
from util_gpu import _graph_nodes, buffers                  # noqa: F401 (buffers: a fixture, asked for by name)
from util_parity import slice_errors

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = 2e-4, 3e-4
CASES = B.all_cases()
CL = torch.channels_last


def _run_once(c, row, relu, res_layout='nhwc', res_grad=True, w=None):
    """One forward and backward of a case on the device: (out, {name: gradient}) on the CPU."""
    from ghn3_amd import target_ops as T
    st, pad, dil, relu_in = row[6], row[7], row[8], row[9]
    x, w, bias = [t.cuda().requires_grad_(True) for t in (c['x'], c['w'] if w is None else w, c['bias'])]
    res = None
    if c['res'] is not None:
        res = c['res'].cuda()
        if res_layout == 'nhwc':
            res = res.contiguous(memory_format=CL)
        res.requires_grad_(res_grad)
    assert T.ConvBiasAct.applicable(x, w, bias, res, st, pad, dil)
    out = T.conv_bias_act(x, w, bias, res, st, pad, dil, relu, relu_in)
    assert 'ConvBiasAct' in _graph_nodes(out) and 'ConvolutionBackward' not in _graph_nodes(out)
    assert out.shape == c['out'].shape and out.is_contiguous(memory_format=CL)
    (out * c['up'].cuda()).sum().backward()
    torch.cuda.synchronize()
    grads = dict(dx=x.grad, dw=w.grad, dbias=bias.grad)
    if res is not None:
        grads['dres'] = res.grad
    return out.detach().cpu(), {k: None if v is None else v.cpu() for k, v in grads.items()}


def _measure(label, name, got, ref, axes, tol):
    assert got.shape == ref.shape, (label, name, got.shape, ref.shape)
    v, where = slice_errors(got, ref, axes)
    print('%s %s %.3e' % (label, name, v))
    assert v <= tol, (label, name, v, where)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_bias_cases_against_fp64(case, buffers):
    name, row, with_res, relu, special = case
    c = B.bias_case(row, with_res, relu, special)
    Co = row[2]
    (out, grads), (out2, grads2) = _run_once(c, row, relu), _run_once(c, row, relu)
    assert torch.equal(out, out2)                                       # deterministic: the same bits again,
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k                      # ... the fixed-order reductions of the gradients included
    assert all(torch.isfinite(t).all() for t in [out] + list(grads.values()))
    assert ('dres' in grads) == with_res                                # without a skip tensor no dres is produced
    keep = torch.ones(Co, dtype=torch.bool)
    if special:
        keep[B.MASKED_CH] = False
        # a fully masked channel: no gradient reaches its parameters, exactly
        for k, t in (('out', out[:, B.MASKED_CH]), ('dbias', grads['dbias'][B.MASKED_CH]), ('dw', grads['dw'][B.MASKED_CH])):
            assert float(t.abs().max()) == 0.0, k
        assert bool((out[:, B.OPEN_CH] > 0).all())
        # ... nor x through it: with that channel's weights zero (its bias keeps it masked) dx has the same bits
        w0 = c['w'].clone()
        w0[B.MASKED_CH] = 0
        out0, grads0 = _run_once(c, row, relu, w=w0)
        assert float(out0[:, B.MASKED_CH].abs().max()) == 0.0 and torch.equal(grads0['dx'], grads['dx'])
    _measure(name, 'out', B.kept('out', out, keep), B.kept('out', c['out'], keep), E.ACT_AXES, OUT_TOL)
    for k, axes in (('dx', E.ACT_AXES), ('dw', E.WGRAD_AXES), ('dbias', E.VEC_AXES)) + ((('dres', E.ACT_AXES),) if with_res else ()):
        _measure(name, k, B.kept(k, grads[k], keep), B.kept(k, c[k], keep), axes, GRAD_TOL)
    if with_res and relu:                                               # dres = dout 1[out > 0]: where the reference masks, exactly 0
        assert bool((grads['dres'][c['out'] == 0] == 0).all())
    if row[9]:                                                          # relu_in: dx is masked by x > 0 and by nothing else
        assert bool((grads['dx'][c['x'] <= 0] == 0).all())


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'norelu'])
def test_a_residual_without_a_gradient_and_one_in_nchw_storage(relu):
    row = B.ROWS[0]
    c = B.bias_case(row, True, relu)
    out, grads = _run_once(c, row, relu)
    out_n, grads_n = _run_once(c, row, relu, res_grad=False)            # dres is NULL: the other results do not move
    assert grads_n['dres'] is None and torch.equal(out_n, out)
    assert all(torch.equal(grads_n[k], grads[k]) for k in ('dx', 'dw', 'dbias'))
    out_p, grads_p = _run_once(c, row, relu, res_layout='nchw')         # an NCHW-contiguous skip tensor: the same bits
    assert torch.equal(out_p, out) and all(torch.equal(grads_p[k], grads[k]) for k in grads)
    v, where = slice_errors(grads_p['dres'], c['dres'], E.ACT_AXES)
    assert v <= GRAD_TOL, (v, where)


def test_what_is_not_applicable_and_no_grad_saves_nothing():
    from ghn3_amd import target_ops as T
    row = B.ROWS[0]
    c = B.bias_case(row, True, True)
    x, w, bias, res = [c[k].cuda() for k in ('x', 'w', 'bias', 'res')]
    args = (row[6], row[7], row[8])
    assert T.ConvBiasAct.applicable(x, w, bias, res, *args)
    assert not T.ConvBiasAct.applicable(x, w, bias, res[:, :-4], *args)                    # not the output's shape
    assert not T.ConvBiasAct.applicable(x, w, bias, res.double(), *args)
    assert not T.ConvBiasAct.applicable(x, w, bias, res.cpu(), *args)
    assert not T.ConvBiasAct.applicable(x, w, bias.cpu(), res, *args)
    assert not T.ConvBiasAct.applicable(x, w, bias[:-4], res, *args)
    assert not T.ConvBiasAct.applicable(x, w, bias, res, row[6], (0, 0), 3)                # no output pixel left
    assert not T.ConvBiasAct.applicable(x[:, :-1], w[:, :-1], bias, None, *args)           # C_in not a multiple of 4
    with torch.no_grad():
        out = T.conv_bias_act(x.requires_grad_(True), w, bias, res, *args)
    assert out.grad_fn is None and not out.requires_grad
    v, where = slice_errors(out.cpu(), c['out'], E.ACT_AXES)
    assert v <= OUT_TOL, (v, where)


@pytest.mark.parametrize('row', [B.ROWS[0], B.R.ROWS[7]], ids=['row0', 'stem'])
def test_runner_gradients_own_their_storage_and_the_switch(row, monkeypatch):
    """run_conv_bias_act on leaf Parameters: every .grad is a tensor of its own (not a view of a buffer shared with the scratch
    area); GHN3_NATIVE_BIAS=0 keeps the layer stock."""
    from ghn3_amd import target_ops as T
    c = B.bias_case(row, True, True)
    conv = torch.nn.Conv2d(row[1], row[2], row[5], row[6], row[7], row[8], bias=True)
    with torch.no_grad():
        conv.weight.copy_(c['w'][:, :row[1]])
        conv.bias.copy_(c['bias'])
    conv = conv.cuda()
    conv_s = copy.deepcopy(conv)
    x = c['x'][:, :row[1]].contiguous().cuda()                                       # (the stem row: the 3-channel image, padded by the runner)
    res = c['res'].cuda().contiguous(memory_format=CL)
    out = T.run_conv_bias_act(conv, x, True, res)
    assert out is not None and 'ConvBiasAct' in _graph_nodes(out)
    (out * c['up'].cuda()).sum().backward()
    ref = F.relu(conv_s(x) + res.contiguous())
    (ref * c['up'].cuda()).sum().backward()
    torch.cuda.synchronize()
    for p in (conv.weight, conv.bias):
        assert p.grad is not None and p.grad.shape == p.shape
        assert p.grad.untyped_storage().nbytes() == p.grad.numel() * 4, (tuple(p.shape), p.grad.untyped_storage().nbytes())
    for a, b in ((conv.weight, conv_s.weight), (conv.bias, conv_s.bias)):
        v, where = slice_errors(a.grad.cpu(), b.grad.cpu(), E.WGRAD_AXES if a.dim() == 4 else E.VEC_AXES)
        assert v <= GRAD_TOL, (tuple(a.shape), v, where)
    monkeypatch.setenv('GHN3_NATIVE_BIAS', '0')
    assert T.run_conv_bias_act(conv, x, True, res) is None


# ---- whole networks -------------------------------------------------------------------------------------------------------------
# (a BatchNorm2d on the stock path of a ROCm build may run on MIOpen: its node is named after it)
CONV_NODES = ('ConvolutionBackward',)
STOCK_NODES = CONV_NODES + ('ReluBackward', 'NativeBatchNormBackward', 'MaxPool2DWithIndicesBackward', 'MiopenBatchNormBackward',
                            'CudnnBatchNormBackward', 'AvgPool2DBackward', 'AddmmBackward', 'CatBackward', 'NativeDropoutBackward')
NET_CASES = [(B.VggNet, 'resnet', STOCK_NODES), (B.FireNet, 'resnet', CONV_NODES), (B.FireNet, 'all', STOCK_NODES)]


@pytest.mark.parametrize('cls,windows,absent', NET_CASES, ids=['VggNet', 'FireNet', 'FireNet-all'])
@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
def test_nativized_networks_against_the_stock_gpu_path(cls, windows, absent, train):
    import ghn3_amd
    net = B.make_net(cls).cuda()
    ref = copy.deepcopy(net)
    nat = ghn3_amd.nativize(net, strict=True, windows=windows, biased=True)
    rep = nat.report()
    assert rep['windows'] == B.expected_windows(cls, windows, True) and rep['stock_convs'] == {}, str(rep)
    x, y = [t.cuda() for t in B.net_batch(cls)]
    nat.train(train)
    ref.train(train)
    torch.manual_seed(77)                                               # (the same Dropout draws on both paths)
    loss = F.cross_entropy(nat(x), y)
    torch.manual_seed(77)
    loss_ref = F.cross_entropy(ref(x), y)
    nodes = _graph_nodes(loss)
    assert 'ConvBiasAct' in nodes and not any(s in nodes for s in absent), nodes
    assert all(s in _graph_nodes(loss_ref) for s in STOCK_NODES[:2])
    loss.backward()
    loss_ref.backward()
    torch.cuda.synchronize()
    print('%s %s %s: loss %.6f / %.6f' % (cls.__name__, windows, 'train' if train else 'eval', loss.item(), loss_ref.item()))
    assert abs(loss.item() - loss_ref.item()) < 2e-4 * max(1.0, abs(loss_ref.item())), (loss.item(), loss_ref.item())
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert p.grad is not None, k
        err, norm = float((p.grad.double() - q.grad.double()).norm()), float(q.grad.double().norm())
        assert err < 2e-3 * norm + 1e-6, (k, err, norm)
    for (k, b), c in zip(net.named_buffers(), ref.buffers()):
        if train:
            assert torch.allclose(b.float(), c.float(), rtol=1e-4, atol=1e-6), k
        else:
            assert torch.equal(b, c), k


# ---- the plain Trainer branch ---------------------------------------------------------------------------------------------------
def test_trainer_native_biased_against_the_default():
    from ghn3_amd import Trainer
    losses = {}
    for native in (False, True):
        net = B.make_net(B.VggNet)
        tr = Trainer(net, opt='sgd', opt_args={'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4}, scheduler='cosine', n_batches=3,
                     grad_clip=5, device='cuda', label_smoothing=0.1, epochs=2, log_interval=1, native_layers=native,
                     native_biased=native)
        assert tr._model is net
        losses[native] = []
        for k in range(3):
            torch.manual_seed(60 + k)                                   # (the same Dropout draws on both paths)
            tr.update(*B.net_batch(B.VggNet, seed=30 + k))
            losses[native].append(float(tr.metrics.avg()['loss']))
        assert (tr._forward_model is not None) == native
        if native:
            rep = tr._forward_model.report()
            assert rep['windows']['conv_bias_relu'] == 3 and rep['windows']['mlp_head'] == 1 and rep['stock_convs'] == {}
    print('running mean of the loss, stock / native layers: %s / %s' % (losses[False], losses[True]))
    for a, b in zip(losses[True], losses[False]):
        assert abs(a - b) < 2e-4 * max(1.0, abs(b)), (losses[True], losses[False])
