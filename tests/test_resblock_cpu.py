"""CPU checks around the "act" member of the dense-convolution family and ghn3_amd.nativize (no GPU):

 * the cases of tests/resblock_cases.py are well conditioned -- variance floor, the share of the upstream gradient zeroed near
   the ReLU's kink -- and the stock fp32 layers meet, against fp64, the tolerances tests/test_gpu_target_resblock.py asks of the
   kernels: the reference alone is good for them;
 * nativize on three plain networks: window counts, shared Parameters and buffers, and on the CPU -- where every window runs the
   very modules it replaced -- outputs, gradients and running statistics equal to the original's bit for bit;
 * what it leaves on the stock layers and why; a model torch.fx cannot trace;
 * the plain Trainer branch refuses what it refused.
"""
import copy

import pytest
import torch
import torch.nn as nn

import resblock_cases as R
import target_edge_cases as E
from util_parity import slice_errors

import ghn3_amd
from ghn3_amd import native_net, target_ops as T

OUT_TOL, GRAD_TOL = 2e-4, 3e-4
CASES = R.all_cases()


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_cases_are_well_conditioned_and_stock_fp32_meets_the_tolerances(case):
    name, row, with_res, special, frozen = case
    c = R.act_case(row, with_res, special, frozen)
    Co = row[2]
    if not frozen:
        var = c['z'].var((0, 2, 3), unbiased=False)
        assert float(var.min()) >= R.VAR_FLOOR, float(var.min())
    assert c['share'] <= R.MASK_SHARE, c['share']
    assert bool((c['up'][c['y'].abs() < R.MASK_BAND] == 0).all())
    keep = torch.ones(Co, dtype=torch.bool)
    if special:
        keep[R.MASKED_CH] = False
        assert float(c['out'][:, R.MASKED_CH].abs().max()) == 0.0          # fully masked in the reference as well,
        assert bool((c['y'][:, R.OPEN_CH] > 0).all())                      # ... and never masked
    # stock fp32 against fp64
    leaves = [c[k].clone().requires_grad_(True) for k in ('x', 'w', 'gamma', 'beta')]
    res = c['res'].clone().requires_grad_(True) if with_res else None
    out = T.conv_act_reference(*leaves, res, row[6], row[7], row[8], row[9], 1e-5,
                               *(c['running'] if frozen else (None, None)))
    (out * c['up']).sum().backward()
    worst = {}
    for key, got, axes, tol in (('out', out.detach(), E.ACT_AXES, OUT_TOL), ('dx', leaves[0].grad, E.ACT_AXES, GRAD_TOL),
                                ('dw', leaves[1].grad, E.WGRAD_AXES, GRAD_TOL), ('dgamma', leaves[2].grad, E.VEC_AXES, GRAD_TOL),
                                ('dbeta', leaves[3].grad, E.VEC_AXES, GRAD_TOL)) + \
            ((('dres', res.grad, E.ACT_AXES, GRAD_TOL),) if with_res else ()):
        got, ref = R.kept(key, got, keep), R.kept(key, c[key], keep)
        v, where = slice_errors(got, ref, axes)
        worst[key] = v
        assert v <= tol, (name, key, v, where)
    print(name, 'zeroed share %.4f %%' % (100 * c['share']), ', '.join('%s %.1e' % kv for kv in worst.items()))


def test_the_case_list_has_what_the_kernels_need():
    rows = [c[1] for c in CASES]
    assert any(r[2] // 4 > 256 for r in rows)                                           # the looping arm of the partial sums
    assert any(r is R.GRID_ROW for r in rows) and R.GRID_ROW[0] * R.GRID_ROW[2] * R.GRID_ROW[3] * R.GRID_ROW[4] // 4 > R.ACT_GRID_CAP * 256
    assert any(r[5] == (7, 7) and r[1] == 3 for r in rows) and any(r[9] for r in rows)
    for row in R.ROWS:                                                                  # every row with and without a skip tensor
        assert {c[2] for c in CASES if c[1] is row and not c[3] and not c[4]} == {False, True}
    text = open(T.__file__.replace('target_ops.py', 'csrc/target_ops.hip')).read()
    assert 'constexpr int ACT_GRID_CAP = %d;' % R.ACT_GRID_CAP in text


# ---- nativize ---------------------------------------------------------------------------------------------------------------------
def _step(model, x, y, train=True):
    model.train(train)
    out = model(x)
    if train:
        nn.functional.cross_entropy(out, y).backward()
    return out.detach()


@pytest.mark.parametrize('cls', R.NETS, ids=lambda c: c.__name__)
def test_nativize_on_the_cpu_is_the_original_bit_for_bit(cls):
    net = R.make_net(cls)
    ref = copy.deepcopy(net)
    keys = list(net.state_dict())
    nat = ghn3_amd.nativize(net, strict=True)
    rep = nat.report()
    assert rep['windows'] == cls.windows and rep['stock_convs'] == {}, str(rep)
    # the same Parameters and buffers, under the same names; the original is untouched
    # (torch.fx registers the layers in the order the forward calls them: the same keys, possibly in another order)
    assert sorted(nat.state_dict()) == sorted(keys) and keys == list(net.state_dict())
    mine = dict(net.named_parameters())
    assert all(p is mine[k] for k, p in nat.named_parameters()) and len(list(nat.parameters())) == len(mine)
    mine = dict(net.named_buffers())
    assert all(b is mine[k] for k, b in nat.named_buffers()) and len(list(nat.buffers())) == len(mine)
    assert not any(isinstance(m, native_net._Window) for m in net.modules())
    x, y = R.net_batch(cls)
    out, out_ref = _step(nat, x, y), _step(ref, x, y)
    assert torch.equal(out, out_ref)
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
    for (k, b), c in zip(net.named_buffers(), ref.buffers()):               # running statistics and the batch counters
        assert torch.equal(b, c), k
    assert any('running_mean' in k and float(b.abs().max()) > 0 for k, b in net.named_buffers())
    with torch.no_grad():
        assert torch.equal(_step(nat, x, y, train=False), _step(ref, x, y, train=False))
    # eval() on the nativized module reaches the shared layers
    assert not nat.training and not any(m.training for m in net.modules() if isinstance(m, nn.BatchNorm2d))


@pytest.mark.parametrize('kind', sorted(R.REFUSALS))
def test_refusals_stay_on_the_stock_layers_and_the_report_says_why(kind):
    torch.manual_seed(3)
    net = R.Refused(kind)
    ref = copy.deepcopy(net)
    nat = ghn3_amd.nativize(net, strict=True)
    rep = nat.report()
    assert sum(rep['windows'].values()) == 0 and list(rep['stock_convs']) == ['conv'], str(rep)
    assert R.REFUSALS[kind] in rep['stock_convs']['conv'], rep['stock_convs']
    assert R.REFUSALS[kind] in str(rep)
    x = torch.randn(3, 4, 6, 6, generator=torch.Generator().manual_seed(4))
    assert torch.equal(nat(x), ref(x))


def test_a_window_that_is_refused_does_not_spoil_its_neighbours():
    """A biased convolution between two fusable ones: two windows, one stock layer, the same result."""
    torch.manual_seed(5)
    net = nn.Sequential(nn.Conv2d(4, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU(),
                        nn.Conv2d(8, 8, 3, 1, 1, bias=True), nn.BatchNorm2d(8), nn.ReLU(),
                        nn.Conv2d(8, 8, 1, bias=False), nn.BatchNorm2d(8), nn.ReLU(inplace=True))
    ref = copy.deepcopy(net)
    nat = ghn3_amd.nativize(net)
    assert nat.report()['windows']['conv_bn_relu'] == 2 and list(nat.report()['stock_convs']) == ['3']
    x = torch.randn(3, 4, 6, 6, generator=torch.Generator().manual_seed(4))
    assert torch.equal(nat(x), ref(x))


def test_a_model_that_cannot_be_traced_is_returned_unchanged(capsys):
    net = R.Branchy()
    assert ghn3_amd.nativize(net) is net
    assert 'cannot be traced' in capsys.readouterr().out
    with pytest.raises(Exception) as err:
        ghn3_amd.nativize(net, strict=True)
    assert 'control flow' in str(err.value) or 'Proxy' in str(err.value)


def test_switch_and_runner_on_cpu_tensors(monkeypatch):
    conv, bn = nn.Conv2d(4, 8, 3, 1, 1, bias=False), nn.BatchNorm2d(8)
    x = torch.randn(2, 4, 5, 5)
    assert T.run_conv_bn_act(conv, bn, x) is None                          # (a CPU tensor: the caller keeps its stock layers)
    assert not T.ConvBnAct.applicable(x, conv.weight, bn.weight, bn.bias)
    assert T.act_enabled()
    monkeypatch.setenv('GHN3_NATIVE_ACT', '0')
    assert not T.act_enabled()
    with pytest.raises(ghn3_amd._lib.Ghn3Error):
        T.conv_bn_act(x, conv.weight, bn.weight, bn.bias)                  # no CPU implementation, as for conv_bn


def test_trainer_native_layers_on_the_cpu_and_the_old_refusals():
    from ghn3_amd import Trainer
    for bad in (dict(opt='adamw'), dict(bce=True), dict(mixup=True)):
        args = dict(opt='sgd', bce=False, mixup=False, compile_mode=None)
        args.update(bad)
        with pytest.raises(NotImplementedError):
            Trainer._check_plain(**args)
    Trainer._check_plain('sgd', False, False, None)
    losses = {}
    for native in (False, True):
        net = R.make_net(R.BasicNet)
        tr = Trainer(net, opt='sgd', opt_args={'lr': 0.05, 'momentum': 0.9}, scheduler='cosine', n_batches=4, device='cpu',
                     epochs=2, log_interval=1, native_layers=native)
        assert tr._model is net
        for k in range(2):
            tr.update(*R.net_batch(R.BasicNet, seed=20 + k))
        losses[native] = (tr.metrics.avg()['loss'], [p.detach().clone() for p in net.parameters()])
        assert (tr._forward_model is not None) == native
    assert losses[True][0] == losses[False][0]
    assert all(torch.equal(a, b) for a, b in zip(losses[True][1], losses[False][1]))
    with pytest.raises(NotImplementedError):                               # (the refusals come before the new argument is read)
        Trainer(R.make_net(R.BasicNet), opt='adamw', opt_args={'lr': 0.1}, scheduler='cosine', n_batches=4, device='cpu',
                native_layers=True)
