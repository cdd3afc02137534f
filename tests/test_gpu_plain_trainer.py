"""GPU tests of the plain-network branch of ghn3_amd.Trainer (the train_ddp.py recipe): updates against a stock loop, the
skipped step, the GHN-predicted initial parameters with and without noise, and a network on the native layers."""

import copy

import pytest
import torch
import torch.nn as nn

import recipe
from util_parity import make_models

pytestmark = pytest.mark.gpu
OPT_ARGS = {'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4}


def _batch(k=0, n=8):
    g = torch.Generator().manual_seed(70 + k)
    return torch.randn(n, 3, 32, 32, generator=g), torch.randint(0, 10, (n,), generator=g)


def _resnet():
    import graph_nets
    torch.manual_seed(11)
    return graph_nets.ResNetTiny()


def _trainer(model, **kw):
    from ghn3_amd import Trainer
    args = dict(opt='sgd', opt_args=dict(OPT_ARGS), scheduler='mstep', scheduler_args={'milestones': [1], 'gamma': 0.1},
                n_batches=4, grad_clip=5, device='cuda', label_smoothing=0.1, epochs=2, log_interval=1)
    args.update(kw)
    return Trainer(model, **args)


def _cat(model):
    return torch.cat([p.detach().reshape(-1).double() for p in model.parameters()])


@pytest.mark.parametrize('fused', ['1', '0'])
def test_three_updates_equal_the_stock_loop(fused, monkeypatch):
    """Same initial state, same batches: concatenated parameters within 3e-6 (relative L2), loss and top-1 to 1e-5."""
    from ghn3_amd import optim as O
    monkeypatch.setenv('GHN3_FUSED_SGD', fused)
    net = _resnet()
    ref = copy.deepcopy(net).cuda()
    tr = _trainer(net)
    assert isinstance(tr._optimizer, O.FusedSGD if fused == '1' else O.StockSGD)
    opt = torch.optim.SGD(ref.parameters(), **OPT_ARGS)
    crit = nn.CrossEntropyLoss(label_smoothing=0.1)
    losses, top1 = [], []
    for k in range(3):
        x, y = _batch(k)
        tr.update(x, y)
        x, y = x.cuda(), y.cuda()
        ref.train()
        opt.zero_grad()
        out = ref(x)
        loss = crit(out, y)
        loss.backward()
        nn.utils.clip_grad_norm_(ref.parameters(), 5)
        opt.step()
        losses.append(float(loss.detach()))
        top1.append(100.0 * float((out.argmax(1) == y).float().mean()))
    a, b = _cat(net), _cat(ref)
    err = float((a - b).norm() / b.norm())
    avg = tr.metrics.avg()
    print('plain trainer (GHN3_FUSED_SGD=%s) against the stock loop: parameters %.3e, loss %.6f / %.6f, top-1 %.4f / %.4f'
          % (fused, err, avg['loss'], sum(losses) / 3, avg['top1'], sum(top1) / 3))
    assert err <= 3e-6
    assert avg['loss'] == pytest.approx(sum(losses) / 3, rel=1e-5, abs=1e-5)
    assert avg['top1'] == pytest.approx(sum(top1) / 3, rel=1e-5, abs=1e-5)
    for (k, v), w in zip(net.state_dict().items(), ref.state_dict().values()):
        if 'running' in k:
            assert torch.allclose(v, w, rtol=1e-4, atol=1e-6), k


def test_a_nan_batch_changes_nothing():
    net = _resnet()
    tr = _trainer(net)
    tr.update(*_batch(0))
    before = [p.detach().clone() for p in net.parameters()]
    mom = tr._optimizer.momentum_buffer.clone()
    x, y = _batch(1)
    x[3, 1, 5, 5] = float('nan')
    tr.update(x, y)
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), before))
    assert torch.equal(tr._optimizer.momentum_buffer, mom)
    tr.update(*_batch(2))                                                 # the next clean batch trains again
    assert not any(torch.equal(p, q) for p, q in zip(net.parameters(), before))
    assert float(tr.metrics.cnt) == 16


@pytest.fixture(scope='module')
def ghn_ckpt(tmp_path_factory):
    """A GHN3(**TINY_CFG) checkpoint with seeded weights, in the format from_pretrained reads."""
    hip, _ = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
    path = str(tmp_path_factory.mktemp('ghn') / 'tiny_ghn.pt')
    torch.save({'state_dict': {k: v.detach().cpu() for k, v in hip.state_dict().items()}, 'config': dict(recipe.TINY_CFG)}, path)
    return path


@pytest.fixture(scope='module')
def predicted(ghn_ckpt):
    """What the checkpoint's GHN predicts for a ResNetTiny: the parameters GHN-init must set."""
    from ghn3_amd import from_pretrained
    ghn = from_pretrained(ghn_ckpt).to('cuda')
    net = _resnet().cuda()
    with torch.no_grad():
        ghn(net, bn_track_running_stats=True, keep_grads=False, reduce_graph=False)
    return [p.detach().clone() for p in net.parameters()]


def test_ghn_init_without_noise_sets_the_predicted_parameters(ghn_ckpt, predicted):
    net = _resnet()
    start = [p.detach().clone().cuda() for p in net.parameters()]
    tr = _trainer(net, ckpt=ghn_ckpt, beta=0)
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), predicted))
    assert not all(torch.equal(p, q) for p, q in zip(net.parameters(), start))
    assert all(p.is_cuda and p.requires_grad and p.is_leaf for p in net.parameters())
    tr.update(*_batch(0))                                                 # and the network trains from there
    assert torch.isfinite(torch.tensor(tr.metrics.avg()['loss']))


def test_ghn_init_noise_is_seeded_and_spares_vectors(ghn_ckpt, predicted):
    runs = []
    for _ in range(2):
        net = _resnet()
        torch.manual_seed(123)
        _trainer(net, ckpt=ghn_ckpt, beta=1e-2)
        runs.append([p.detach().clone() for p in net.parameters()])
    assert all(torch.equal(p, q) for p, q in zip(*runs))
    n_multi = 0
    for p, q in zip(runs[0], predicted):
        if p.dim() > 1:
            n_multi += 1
            assert not torch.equal(p, q)
            assert float((p - q).std()) == pytest.approx(1e-2, rel=0.5)
        else:
            assert torch.equal(p, q)
    assert n_multi > 0


def test_a_network_on_the_native_layers_trains():
    import network_cases
    from ghn3_amd import ops
    torch.manual_seed(5)
    net = ops.Network(genotype=ops.Genotype(**network_cases._CONV), C=8, num_classes=10, n_cells=3, is_imagenet_input=False)
    tr = _trainer(net)
    before = [p.detach().clone() for p in net.parameters()]
    x, y = _batch(0, n=4)
    tr.update(x, y)
    tr.update(x, y)
    assert torch.isfinite(torch.tensor(tr.metrics.avg()['loss'])) and float(tr.metrics.cnt) == 8
    state = tr._optimizer.state_dict()['state']
    with_grad = [p.grad is not None for p in net.parameters()]
    assert sum(with_grad) > len(with_grad) // 2
    for k, (p, q) in enumerate(zip(net.parameters(), before)):
        if not with_grad[k]:
            assert torch.equal(p, q) and k not in state
            continue
        assert state[k]['momentum_buffer'].shape == p.shape
        if float(p.grad.abs().sum()) > 0:                                 # (an all-zero gradient moves nothing)
            assert not torch.equal(p, q), k
            assert float(state[k]['momentum_buffer'].abs().sum()) > 0
