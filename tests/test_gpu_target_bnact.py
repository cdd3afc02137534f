"""
The stand-alone BatchNorm [+ ReLU] -- ghn3_bn_act_* (ghn3_amd/csrc/tnet_bnact.hip), target_ops.BnAct / BnActEval / run_bn_act --
and ghn3_amd.nativize(windows='all') on the GPU.

Every case of tests/bnact_cases.py runs against the stock layers in fp64 (tests/util_parity.slice_errors) at the tolerances the
project states for the family: 2e-4 for out, mean and variance, 3e-4 for dx, dgamma and dbeta; the kernels are plain fp32, and
the measured values are printed.  The upstream gradient is zero where the fp64 pre-activation lies within 2e-3 of the ReLU's kink
(bnact_cases: a condition on the cases).  Each case runs after asserting `applicable`, twice for equal bits, with x stored NHWC,
NCHW and 4 bytes into a buffer (the same bits again), and once more with every buffer the op allocates pre-filled with NaN.

Whole networks: the two networks of the case file, nativized with windows='all', against the same modules on the stock GPU path
at the tolerances of tests/test_gpu_networks.py (loss 2e-4 relative, every gradient within 2e-3 of its norm), and the plain
Trainer branch with native_layers='all' against without.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import bnact_cases as B
import target_edge_cases as E
from util_gpu import _graph_nodes, buffers                  # noqa: F401 (buffers: a fixture, asked for by name)
from util_parity import slice_errors

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = 2e-4, 3e-4
CASES = B.all_cases()
CL = torch.channels_last


def _stored(x, how):
    """x on the device, dense in NHWC or NCHW order, or NHWC starting 4 bytes into a buffer (not on 16 bytes)."""
    x = x.cuda()
    if how == 'nchw':
        return x.contiguous()
    if how == 'nhwc':
        return x.contiguous(memory_format=CL)
    N, C, H, W = x.shape
    buf = torch.empty(x.numel() + 4, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + x.numel()].view(N, H, W, C).permute(0, 3, 1, 2)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous(memory_format=CL)
    return v


def _run_once(c, relu, frozen, how='nhwc'):
    """One forward and backward of a case on the device: (out, stats, {name: gradient}) on the CPU."""
    from ghn3_amd import target_ops as T
    x = _stored(c['x'], how).requires_grad_(True)
    gamma, beta = [c[k].cuda().requires_grad_(True) for k in ('gamma', 'beta')]
    if frozen:
        rm, rv = [t.cuda() for t in c['running']]
        before = (rm.clone(), rv.clone())
        assert T.BnActEval.applicable(x, gamma, beta, rm, rv)
        out, stats = T.bn_act_eval(x, gamma, beta, rm, rv, relu, B.EPS), None
    else:
        assert T.BnAct.applicable(x, gamma, beta)
        out, stats = T.bn_act(x, gamma, beta, relu, B.EPS)
    nodes = _graph_nodes(out)
    assert 'BnAct' in nodes and 'NativeBatchNormBackward' not in nodes and 'ReluBackward' not in nodes, nodes
    assert out.shape == c['out'].shape and out.is_contiguous(memory_format=CL)
    (out * c['up'].cuda()).sum().backward()
    torch.cuda.synchronize()
    if frozen:
        assert torch.equal(rm, before[0]) and torch.equal(rv, before[1])             # frozen statistics are read only
    grads = dict(dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad)
    assert all(g is not None for g in grads.values())
    return out.detach().cpu(), None if stats is None else stats.cpu(), {k: v.cpu().contiguous() for k, v in grads.items()}


def _measure(label, name, got, ref, axes, tol):
    assert got.shape == ref.shape, (label, name, got.shape, ref.shape)
    v, where = slice_errors(got, ref, axes)
    print('%s %s %.3e' % (label, name, v))
    assert v <= tol, (label, name, v, where)


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_cases_against_fp64(case, buffers):
    label, name, relu, frozen = case
    c = B.case(name, relu, frozen)
    C = B.SHAPES[name][3]
    out, stats, grads = _run_once(c, relu, frozen)
    # the same bits on a second run, and with x stored in NCHW order or 4 bytes into a buffer
    for how in ('nhwc', 'nchw', 'offset'):
        out2, stats2, grads2 = _run_once(c, relu, frozen, how)
        assert torch.equal(out, out2), how
        assert stats is None or torch.equal(stats, stats2), how
        for k in grads:
            assert torch.equal(grads[k], grads2[k]), (how, k)
    assert all(torch.isfinite(t).all() for t in [out] + list(grads.values()) + ([] if stats is None else [stats]))
    if name == 'special':
        if not frozen:                                                                  # a constant channel: variance 0, out = beta
            assert float(stats[2 * C + B.CONST_CH]) == 0.0 and float(stats[B.CONST_CH]) == B.CONST_VALUE
            assert float((out[:, B.CONST_CH] - 0.3).abs().max()) < 1e-6
        if relu:
            # a fully masked channel: no gradient reaches it, exactly
            for k, t in (('out', out[:, B.MASKED_CH]), ('dx', grads['dx'][:, B.MASKED_CH]), ('dgamma', grads['dgamma'][B.MASKED_CH]),
                         ('dbeta', grads['dbeta'][B.MASKED_CH])):
                assert float(t.abs().max()) == 0.0, k
            assert bool((out[:, B.OPEN_CH] > 0).all())
    _measure(label, 'out', out, c['out'], E.ACT_AXES, OUT_TOL)
    if not frozen:
        _measure(label, 'mean', stats[:C], c['mean'], E.VEC_AXES, OUT_TOL)
        _measure(label, 'var', stats[2 * C:], c['var'], E.VEC_AXES, OUT_TOL)
        if name == 'special':                                                           # the far channel on its own scale
            v = abs(float(stats[2 * C + B.FAR_CH]) - float(c['var'][B.FAR_CH])) / float(c['var'][B.FAR_CH])
            print('%s var of the channel at 100 sigma: relative error %.3e' % (label, v))
            assert v <= OUT_TOL, v
    for k, axes in (('dx', E.ACT_AXES), ('dgamma', E.VEC_AXES), ('dbeta', E.VEC_AXES)):
        _measure(label, k, grads[k], c[k], axes, GRAD_TOL)
    if relu and frozen:                                                                 # dx = g gamma rstd: where the reference masks, exactly 0
        assert bool((grads['dx'][c['out'] == 0] == 0).all())


@pytest.mark.parametrize('momentum', [0.1, None], ids=['momentum', 'cumulative'])
def test_running_statistics_after_one_training_call_equal_torchs(momentum):
    from ghn3_amd import target_ops as T
    c = B.case('blocks', True, False)
    C = B.SHAPES['blocks'][3]
    bn = torch.nn.BatchNorm2d(C, momentum=momentum).cuda()
    with torch.no_grad():
        bn.weight.copy_(c['gamma'])
        bn.bias.copy_(c['beta'])
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
    ref = copy.deepcopy(bn)
    x = c['x'].cuda()
    out = T.run_bn_act(bn, x, True)
    assert out is not None and 'BnAct' in _graph_nodes(out)
    ref_out = F.relu(ref(x))
    torch.cuda.synchronize()
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 1
    assert torch.allclose(bn.running_mean, ref.running_mean, rtol=1e-6, atol=1e-6)
    assert torch.allclose(bn.running_var, ref.running_var, rtol=1e-6, atol=1e-6)
    v, where = slice_errors(out.detach().cpu(), ref_out.detach().cpu(), E.ACT_AXES)
    assert v <= OUT_TOL, (v, where)
    # leaf Parameters: every .grad is a tensor of its own
    (out * c['up'].cuda()).sum().backward()
    for p in (bn.weight, bn.bias):
        assert p.grad is not None and p.grad.untyped_storage().nbytes() == p.grad.numel() * 4
    # eval mode: the frozen member, statistics untouched
    bn.eval()
    before = (bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked))
    out = T.run_bn_act(bn, x, False)
    assert out is not None and 'BnActEval' in _graph_nodes(out)
    assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1]) and int(bn.num_batches_tracked) == before[2]


def test_what_is_not_applicable_and_the_switches(monkeypatch):
    from ghn3_amd import target_ops as T
    c = B.case('p65', True, True)
    x, gamma, beta = [c[k].cuda() for k in ('x', 'gamma', 'beta')]
    rm, rv = [t.cuda() for t in c['running']]
    bn = torch.nn.BatchNorm2d(x.shape[1]).cuda()
    assert T.BnAct.applicable(x, gamma, beta) and T.BnActEval.applicable(x, gamma, beta, rm, rv)
    assert not T.BnAct.applicable(x, gamma, beta, training_stats=False)
    assert not T.BnAct.applicable(x[:, :-2], gamma[:-2], beta[:-2])                        # C % 4
    assert not T.BnAct.applicable(x[:1, :, :1, :1], gamma, beta)                           # one value per channel ...
    assert T.BnActEval.applicable(x[:1, :, :1, :1], gamma, beta, rm, rv)                   # ... is fine with frozen statistics
    assert not T.BnAct.applicable(x.double(), gamma, beta) and not T.BnAct.applicable(x, gamma.cpu(), beta)
    assert not T.BnActEval.applicable(x, gamma, beta, rm[:-4], rv)
    with pytest.raises(ValueError):                                                         # torch raises for P == 1: the stock layer has to
        assert T.run_bn_act(bn, x[:1, :, :1, :1], True) is None
        bn(x[:1, :, :1, :1])
    assert T.run_bn_act(bn, x, True) is not None
    with torch.autocast('cuda', dtype=torch.float16):
        assert T.run_bn_act(bn, x, True) is not None
        monkeypatch.setenv('GHN3_NATIVE_AMP', '0')
        assert T.run_bn_act(bn, x, True) is None
    monkeypatch.delenv('GHN3_NATIVE_AMP')
    for switch in ('GHN3_NATIVE_BNACT', 'GHN3_NATIVE_OPS'):
        monkeypatch.setenv(switch, '0')
        assert T.run_bn_act(bn, x, True) is None and T.bn_act_refusal(x, gamma, beta) == 'switch'
        monkeypatch.delenv(switch)
    assert T.run_bn_act(bn, x.half(), True) is None
    assert T.run_bn_act(torch.nn.BatchNorm2d(x.shape[1], affine=False).cuda(), x, True) is None


def test_no_grad_saves_nothing(monkeypatch):
    from ghn3_amd import target_ops as T
    c = B.case('p63', True, False)
    seen = []
    inner = T._bn_act_forward

    def spy(ctx, frozen, x, norm, relu, eps, keep):
        seen.append(keep)
        return inner(ctx, frozen, x, norm, relu, eps, keep)
    monkeypatch.setattr(T, '_bn_act_forward', spy)
    x, gamma, beta = [c[k].cuda().requires_grad_(True) for k in ('x', 'gamma', 'beta')]
    rm, rv = [t.cuda() for t in B.running_of('p63', c['x'])]
    with torch.no_grad():
        out, _ = T.bn_act(x, gamma, beta, True, B.EPS)
        out_e = T.bn_act_eval(x, gamma, beta, rm, rv, True, B.EPS)
    assert seen == [False, False] and out.grad_fn is None and out_e.grad_fn is None
    v, where = slice_errors(out.cpu(), c['out'], E.ACT_AXES)
    assert v <= OUT_TOL, (v, where)
    out, _ = T.bn_act(x, gamma, beta, True, B.EPS)
    assert seen == [False, False, True] and out.grad_fn is not None
    out, _ = T.bn_act(x.detach(), gamma.detach(), beta.detach(), True, B.EPS)           # no input requires a gradient
    assert seen[-1] is False


# ---- whole networks -------------------------------------------------------------------------------------------------------------
# (a BatchNorm2d on the stock path of a ROCm build may run on MIOpen: its node is named after it)
STOCK_NODES = ('ConvolutionBackward', 'NativeBatchNormBackward', 'CatBackward', 'AddBackward', 'ReluBackward',
               'MiopenBatchNormBackward', 'CudnnBatchNormBackward', 'AvgPool2DBackward')


@pytest.mark.parametrize('cls', B.NETS, ids=lambda c: c.__name__)
@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
def test_nativized_networks_against_the_stock_gpu_path(cls, train):
    import ghn3_amd
    net = B.make_net(cls).cuda()
    ref = copy.deepcopy(net)
    nat = ghn3_amd.nativize(net, strict=True, windows='all')
    rep = nat.report()
    assert rep['windows'] == B.windows_all(cls) and rep['stock_convs'] == {}, str(rep)
    x, y = [t.cuda() for t in B.net_batch(cls)]
    nat.train(train)
    ref.train(train)
    loss = F.cross_entropy(nat(x), y)
    loss_ref = F.cross_entropy(ref(x), y)
    nodes = _graph_nodes(loss)
    assert not any(s in nodes for s in STOCK_NODES), nodes
    assert 'BnAct' in nodes and 'ConvOnly' in nodes and 'Join' in nodes, nodes
    assert 'ConvolutionBackward' in _graph_nodes(loss_ref)
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


def test_the_default_windows_leave_the_new_layers_stock():
    """nativize(net) without the argument is what it was: the leading BatchNorm, the bare convolutions and the joins of a dense
    layer stay on the stock path."""
    import ghn3_amd
    net = B.make_net(B.DenseNetBC).cuda()
    nat = ghn3_amd.nativize(net, strict=True)
    assert nat.report()['windows'] == B.DenseNetBC.windows
    x, y = [t.cuda() for t in B.net_batch(B.DenseNetBC)]
    nodes = _graph_nodes(F.cross_entropy(nat(x), y))
    assert 'ConvolutionBackward' in nodes and 'CatBackward' in nodes and 'BnAct' not in nodes.replace('ConvBnAct', ''), nodes


# ---- the plain Trainer branch ---------------------------------------------------------------------------------------------------
def test_two_trainer_steps_with_all_windows_against_the_stock_layers():
    from ghn3_amd import Trainer
    losses = {}
    for native in (False, 'all'):
        net = B.make_net(B.DenseNetBC)
        tr = Trainer(net, opt='sgd', opt_args={'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4}, scheduler='cosine', n_batches=3,
                     grad_clip=5, device='cuda', label_smoothing=0.1, epochs=2, log_interval=1, native_layers=native)
        assert tr._model is net
        losses[native] = []
        for k in range(2):
            tr.update(*B.net_batch(B.DenseNetBC, n=8, seed=30 + k))
            losses[native].append(float(tr.metrics.avg()['loss']))
        assert (tr._forward_model is not None) == bool(native)
        if native:
            assert tr._forward_model.report()['windows'] == B.windows_all(B.DenseNetBC)
        losses[native].append([p.detach().double().cpu() for p in net.parameters()])
    print('running mean of the loss, stock / all windows: %s / %s' % (losses[False][:2], losses['all'][:2]))
    for a, b in zip(losses['all'][:2], losses[False][:2]):
        assert abs(a - b) < 2e-4 * max(1.0, abs(b)), (losses['all'][:2], losses[False][:2])
    for p, q in zip(losses['all'][2], losses[False][2]):
        assert float((p - q).norm()) < 2e-3 * float(q.norm()) + 1e-6
