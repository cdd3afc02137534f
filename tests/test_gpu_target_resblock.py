"""
The "act" member of the dense-convolution family -- conv -> BatchNorm [-> + skip] -> ReLU as one node, ghn3_conv_bn_act_* and
ghn3_conv_frozen_act_* (ghn3_amd/csrc/target_ops.hip) -- and ghn3_amd.nativize on the GPU.

Every case of tests/resblock_cases.py runs against the stock layers in fp64 (tests/util_parity.slice_errors, the slicings of
tests/target_edge_cases.py) at the tolerances the project states for this family: 2e-4 for out, mean and variance, 3e-4 for dx,
dw, dgamma, dbeta and dres.  The upstream gradient is zero where the fp64 pre-activation lies within 2e-3 of the ReLU's kink
(resblock_cases: a condition on the cases).  Each case runs twice for equal bits, once more with every buffer the op allocates
pre-filled with NaN, and after asserting `applicable(...)`, so that no case tests the stock fallback.

Whole networks: the three networks of the case file, nativized, against the same modules on the stock GPU path at the
tolerances of tests/test_gpu_networks.py (loss 2e-4 relative, every gradient within 2e-3 of its norm); the plain Trainer branch
with native_layers against without.
"""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import resblock_cases as R
import target_edge_cases as E
from util_gpu import _graph_nodes, buffers                  # noqa: F401 (buffers: a fixture, asked for by name)
from util_parity import slice_errors

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = 2e-4, 3e-4
CASES = R.all_cases()
CL = torch.channels_last


def _run_once(c, row, frozen, res_layout='nhwc', res_grad=True):
    """One forward and backward of a case on the device: (out, stats, {name: gradient}) on the CPU."""
    from ghn3_amd import target_ops as T
    st, pad, dil, relu_in = row[6], row[7], row[8], row[9]
    x, w, gamma, beta = [c[k].cuda().requires_grad_(True) for k in ('x', 'w', 'gamma', 'beta')]
    res = None
    if c['res'] is not None:
        res = c['res'].cuda()
        if res_layout == 'nhwc':
            res = res.contiguous(memory_format=CL)
        res.requires_grad_(res_grad)
    if frozen:
        rm, rv = [t.cuda() for t in c['running']]
        before = (rm.clone(), rv.clone())
        assert T.ConvBnActEval.applicable(x, w, gamma, beta, rm, rv, res, st, pad, dil)
        out, stats = T.conv_bn_act_eval(x, w, gamma, beta, rm, rv, res, st, pad, dil, relu_in), None
    else:
        assert T.ConvBnAct.applicable(x, w, gamma, beta, res, st, pad, dil)
        out, stats = T.conv_bn_act(x, w, gamma, beta, res, st, pad, dil, relu_in)
    assert 'ConvBnAct' in _graph_nodes(out) and 'ConvolutionBackward' not in _graph_nodes(out)
    assert out.shape == c['out'].shape and out.is_contiguous(memory_format=CL)
    (out * c['up'].cuda()).sum().backward()
    torch.cuda.synchronize()
    if frozen:
        assert torch.equal(rm, before[0]) and torch.equal(rv, before[1])             # read only
    grads = dict(dx=x.grad, dw=w.grad, dgamma=gamma.grad, dbeta=beta.grad)
    if res is not None:
        grads['dres'] = res.grad
    return out.detach().cpu(), None if stats is None else stats.cpu(), {k: None if v is None else v.cpu() for k, v in grads.items()}


def _measure(label, name, got, ref, axes, tol, worst):
    assert got.shape == ref.shape, (label, name, got.shape, ref.shape)
    v, where = slice_errors(got, ref, axes)
    worst[name] = v
    print('%s %s %.3e' % (label, name, v))
    assert v <= tol, (label, name, v, where)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_act_cases_against_fp64(case, buffers):
    name, row, with_res, special, frozen = case
    c = R.act_case(row, with_res, special, frozen)
    Co = row[2]
    (out, stats, grads), (out2, stats2, grads2) = _run_once(c, row, frozen), _run_once(c, row, frozen)
    assert torch.equal(out, out2)                                       # deterministic: the same bits again,
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k                      # ... the fixed-order reductions of the gradients included
    assert all(torch.isfinite(t).all() for t in [out] + list(grads.values()))
    keep = torch.ones(Co, dtype=torch.bool)
    if special:
        keep[R.MASKED_CH] = False
        # a fully masked channel: no gradient reaches its parameters, exactly
        for k, t in (('out', out[:, R.MASKED_CH]), ('dgamma', grads['dgamma'][R.MASKED_CH]), ('dbeta', grads['dbeta'][R.MASKED_CH]),
                     ('dw', grads['dw'][R.MASKED_CH])):
            assert float(t.abs().max()) == 0.0, k
        assert bool((out[:, R.OPEN_CH] > 0).all())
    worst = {}
    _measure(name, 'out', R.kept('out', out, keep), R.kept('out', c['out'], keep), E.ACT_AXES, OUT_TOL, worst)
    if not frozen:
        _measure(name, 'mean', stats[:Co], c['z'].mean((0, 2, 3)), E.VEC_AXES, OUT_TOL, worst)
        _measure(name, 'var', stats[2 * Co:], c['z'].var((0, 2, 3), unbiased=False), E.VEC_AXES, OUT_TOL, worst)
    for k, axes in (('dx', E.ACT_AXES), ('dw', E.WGRAD_AXES), ('dgamma', E.VEC_AXES), ('dbeta', E.VEC_AXES)) + \
            ((('dres', E.ACT_AXES),) if with_res else ()):
        _measure(name, k, R.kept(k, grads[k], keep), R.kept(k, c[k], keep), axes, GRAD_TOL, worst)
    if with_res:                                                        # dres = dout 1[out > 0]: where the reference masks, exactly 0
        assert bool((grads['dres'][c['out'] == 0] == 0).all())


def test_a_residual_without_a_gradient_and_one_in_nchw_storage():
    row = R.ROWS[0]
    c = R.act_case(row, True)
    out, _, grads = _run_once(c, row, False)
    out_n, _, grads_n = _run_once(c, row, False, res_grad=False)        # dres is NULL: the other results do not move
    assert grads_n['dres'] is None and torch.equal(out_n, out)
    assert all(torch.equal(grads_n[k], grads[k]) for k in ('dx', 'dw', 'dgamma', 'dbeta'))
    out_p, _, grads_p = _run_once(c, row, False, res_layout='nchw')     # an NCHW-contiguous skip tensor: the same bits
    assert torch.equal(out_p, out) and all(torch.equal(grads_p[k], grads[k]) for k in grads)
    v, where = slice_errors(grads_p['dres'], c['dres'], E.ACT_AXES)
    assert v <= GRAD_TOL, (v, where)


def test_what_is_not_applicable():
    from ghn3_amd import target_ops as T
    row = R.ROWS[0]
    c = R.act_case(row, True)
    x, w, gamma, beta, res = [c[k].cuda() for k in ('x', 'w', 'gamma', 'beta', 'res')]
    args = (row[6], row[7], row[8])
    assert T.ConvBnAct.applicable(x, w, gamma, beta, res, *args)
    assert not T.ConvBnAct.applicable(x, w, gamma, beta, res[:, :-4], *args)              # not the output's shape
    assert not T.ConvBnAct.applicable(x, w, gamma, beta, res.double(), *args)
    assert not T.ConvBnAct.applicable(x, w, gamma, beta, res.cpu(), *args)
    assert not T.ConvBnAct.applicable(x, w, gamma, beta, res, row[6], (0, 0), 3)           # no output pixel left
    assert not T.ConvBnAct.applicable(x[:, :-1], w[:, :-1], gamma, beta, None, *args)      # C_in not a multiple of 4
    assert not T.ConvBnAct.applicable(x, w, gamma, beta, res, *args, training_stats=False)


def test_no_grad_saves_nothing(monkeypatch):
    from ghn3_amd import target_ops as T
    row = R.EVAL_ROWS[0]
    c = R.act_case(row, True, False, True)
    seen = []
    inner = T._conv_act_forward

    def spy(ctx, frozen, *a, **kw):
        seen.append(a[-1] if frozen else True)                          # (`keep`, the last positional argument of the frozen member)
        return inner(ctx, frozen, *a, **kw)
    monkeypatch.setattr(T, '_conv_act_forward', spy)
    x, w, gamma, beta, res = [c[k].cuda().requires_grad_(True) for k in ('x', 'w', 'gamma', 'beta', 'res')]
    rm, rv = [t.cuda() for t in c['running']]
    with torch.no_grad():
        out = T.conv_bn_act_eval(x, w, gamma, beta, rm, rv, res, row[6], row[7], row[8])
    assert seen == [False] and out.grad_fn is None and not out.requires_grad
    v, where = slice_errors(out.cpu(), c['out'], E.ACT_AXES)
    assert v <= OUT_TOL, (v, where)
    out = T.conv_bn_act_eval(x, w, gamma, beta, rm, rv, res, row[6], row[7], row[8])
    assert seen == [False, True] and out.grad_fn is not None


def _layer(row, seed=0):
    c = R.act_case(row, True)
    conv = nn.Conv2d(row[1], row[2], row[5], row[6], row[7], row[8], bias=False)
    bn = nn.BatchNorm2d(row[2])
    with torch.no_grad():
        conv.weight.copy_(c['w'][:, :row[1]])
        bn.weight.copy_(c['gamma'])
        bn.bias.copy_(c['beta'])
    return c, conv.cuda(), bn.cuda()


@pytest.mark.parametrize('row', [R.ROWS[0], R.ROWS[7]], ids=['row0', 'stem'])
def test_runner_gradients_own_their_storage_and_running_statistics_follow(row):
    """run_conv_bn_act on leaf Parameters: every .grad is a tensor of its own (not a view of a buffer shared with the scratch
    area), and the BatchNorm2d's running statistics move as torch's do."""
    from ghn3_amd import target_ops as T
    c, conv, bn = _layer(row)
    conv_s, bn_s = copy.deepcopy(conv), copy.deepcopy(bn)
    x = c['x'][:, :row[1]].contiguous().cuda()                                       # (the stem row: the 3-channel image, padded by the runner)
    res = c['res'].cuda().contiguous(memory_format=CL)
    out = T.run_conv_bn_act(conv, bn, x, res)
    assert out is not None and 'ConvBnAct' in _graph_nodes(out)
    (out * c['up'].cuda()).sum().backward()
    ref = F.relu(bn_s(conv_s(x)) + res.contiguous())
    (ref * c['up'].cuda()).sum().backward()
    torch.cuda.synchronize()
    for p in (conv.weight, bn.weight, bn.bias):
        assert p.grad is not None and p.grad.shape == p.shape
        assert p.grad.untyped_storage().nbytes() == p.grad.numel() * 4, (tuple(p.shape), p.grad.untyped_storage().nbytes())
    for a, b in ((conv.weight, conv_s.weight), (bn.weight, bn_s.weight), (bn.bias, bn_s.bias)):
        axes = E.WGRAD_AXES if a.dim() == 4 else E.VEC_AXES
        v, where = slice_errors(a.grad.cpu(), b.grad.cpu(), axes)
        assert v <= GRAD_TOL, (tuple(a.shape), v, where)
    assert int(bn.num_batches_tracked) == int(bn_s.num_batches_tracked) == 1
    assert torch.allclose(bn.running_mean, bn_s.running_mean, rtol=1e-4, atol=1e-6)
    assert torch.allclose(bn.running_var, bn_s.running_var, rtol=1e-4, atol=1e-6)
    # eval mode: the frozen member, statistics untouched
    bn.eval()
    before = (bn.running_mean.clone(), bn.running_var.clone())
    out = T.run_conv_bn_act(conv, bn, x, res)
    assert out is not None and 'ConvBnActEval' in _graph_nodes(out)
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])


def test_the_switch_keeps_the_layers_stock(monkeypatch):
    from ghn3_amd import target_ops as T
    c, conv, bn = _layer(R.ROWS[0])
    x = c['x'].cuda()
    assert T.run_conv_bn_act(conv, bn, x) is not None
    monkeypatch.setenv('GHN3_NATIVE_ACT', '0')
    assert T.run_conv_bn_act(conv, bn, x) is None


# ---- whole networks -------------------------------------------------------------------------------------------------------------
# (a BatchNorm2d on the stock path of a ROCm build may run on MIOpen: its node is named after it)
STOCK_NODES = ('ConvolutionBackward', 'ReluBackward', 'NativeBatchNormBackward', 'MaxPool2DWithIndicesBackward',
               'MiopenBatchNormBackward', 'CudnnBatchNormBackward', 'AvgPool2DBackward')


@pytest.mark.parametrize('cls', R.NETS, ids=lambda c: c.__name__)
@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
def test_nativized_networks_against_the_stock_gpu_path(cls, train):
    import ghn3_amd
    net = R.make_net(cls).cuda()
    ref = copy.deepcopy(net)
    nat = ghn3_amd.nativize(net, strict=True)
    assert nat.report()['windows'] == cls.windows
    x, y = [t.cuda() for t in R.net_batch(cls)]
    nat.train(train)
    ref.train(train)
    loss = F.cross_entropy(nat(x), y)
    loss_ref = F.cross_entropy(ref(x), y)
    nodes = _graph_nodes(loss)
    assert not any(s in nodes for s in STOCK_NODES), nodes
    assert all(s in _graph_nodes(loss_ref) for s in STOCK_NODES[:2])
    loss.backward()
    loss_ref.backward()
    torch.cuda.synchronize()
    print('%s %s: loss %.6f / %.6f' % (cls.__name__, 'train' if train else 'eval', loss.item(), loss_ref.item()))
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
def _trainer(model, **kw):
    from ghn3_amd import Trainer
    args = dict(opt='sgd', opt_args={'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4}, scheduler='cosine', n_batches=3, grad_clip=5,
                device='cuda', label_smoothing=0.1, epochs=2, log_interval=1)
    args.update(kw)
    return Trainer(model, **args)


def test_trainer_native_layers_against_the_default_and_checkpoints_cross(tmp_path):
    losses, trainers = {}, {}
    for name in ('stock', 'native'):
        (tmp_path / name).mkdir()
    for native in (False, True):
        net = R.make_net(R.StemNet)
        tr = _trainer(net, native_layers=native, save_dir=str(tmp_path / ('native' if native else 'stock')))
        assert tr._model is net
        losses[native] = []
        for k in range(3):
            tr.update(*R.net_batch(R.StemNet, n=8, seed=30 + k))
            losses[native].append(float(tr.metrics.avg()['loss']))
        assert (tr._forward_model is not None) == native
        tr.save(0, 2, {})
        trainers[native] = tr
    print('running mean of the loss, stock / native layers: %s / %s' % (losses[False], losses[True]))
    for a, b in zip(losses[True], losses[False]):
        assert abs(a - b) < 2e-4 * max(1.0, abs(b)), (losses[True], losses[False])
    # a checkpoint written by one setting resumes in the other
    for native in (False, True):
        net = R.make_net(R.StemNet, seed=99)
        tr = _trainer(net, native_layers=native, save_dir=str(tmp_path / ('stock' if native else 'native')))
        assert tr.start_epoch == 1 and tr.start_step == 0
        src = trainers[not native]._model.state_dict()
        assert all(torch.equal(v, src[k]) for k, v in net.state_dict().items())
        tr.reset_metrics(1)
        tr.update(*R.net_batch(R.StemNet, n=8, seed=40))
        assert torch.isfinite(torch.tensor(tr.metrics.avg()['loss']))
