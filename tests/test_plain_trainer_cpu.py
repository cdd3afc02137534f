"""The plain-network branch of ghn3_amd.Trainer (the train_ddp.py recipe) on CPU tensors: three updates against a hand-written
loop with stock torch, the schedule, the checkpoint round trip, and what the branch refuses."""

import copy
import math

import pytest
import torch
import torch.nn as nn

import ghn3_amd
from ghn3_amd import Trainer
from ghn3_amd import trainer as trainer_module

OPT_ARGS = {'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4}
N_BATCHES = 4


def tiny_net():
    torch.manual_seed(7)
    return nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.BatchNorm2d(6), nn.ReLU(), nn.AdaptiveAvgPool2d(2), nn.Flatten(),
                         nn.Linear(24, 10))


def batch(k):
    g = torch.Generator().manual_seed(50 + k)
    return torch.randn(8, 3, 8, 8, generator=g), torch.randint(0, 10, (8,), generator=g)


def make_trainer(model, **kw):
    args = dict(opt='sgd', opt_args=dict(OPT_ARGS), scheduler='mstep', scheduler_args={'milestones': [1], 'gamma': 0.1},
                n_batches=N_BATCHES, grad_clip=5, device='cpu', label_smoothing=0.1, epochs=3, log_interval=1)
    args.update(kw)
    return Trainer(model, **args)


class StockLoop:
    """The hand-written loop: CrossEntropyLoss(label_smoothing), clip_grad_norm_, torch.optim.SGD."""

    def __init__(self, model):
        self.model = model
        self.opt = torch.optim.SGD(model.parameters(), **OPT_ARGS)
        self.crit = nn.CrossEntropyLoss(label_smoothing=0.1)
        self.losses, self.top1 = [], []

    def update(self, x, y):
        self.model.train()
        self.opt.zero_grad()
        out = self.model(x)
        loss = self.crit(out, y)
        loss.backward()
        nn.utils.clip_grad_norm_(self.model.parameters(), 5)
        self.opt.step()
        self.losses.append(float(loss.detach()))
        self.top1.append(100.0 * float((out.argmax(1) == y).float().mean()))


def assert_same_state(a, b, rtol=1e-6):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert torch.allclose(sa[k].double(), sb[k].double(), rtol=rtol, atol=1e-7), k


def test_three_updates_equal_the_stock_loop_and_the_schedule_steps():
    net = tiny_net()
    ref = StockLoop(copy.deepcopy(net))
    tr = make_trainer(net)
    assert isinstance(tr._optimizer, ghn3_amd.FusedSGD)
    for k in range(3):
        tr.update(*batch(k))
        ref.update(*batch(k))
    assert_same_state(net, ref.model)                                    # parameters AND BatchNorm buffers
    avg = tr.metrics.avg()
    assert avg['loss'] == pytest.approx(sum(ref.losses) / 3, rel=1e-6)
    assert avg['top1'] == pytest.approx(sum(ref.top1) / 3, rel=1e-6, abs=1e-9)
    assert len(ref.opt.state_dict()['state']) == len(tr._optimizer.state_dict()['state']) == 6
    assert tr.get_lr() == pytest.approx(0.05)
    tr.scheduler_step()
    assert tr.get_lr() == pytest.approx(0.005)


def test_save_and_resume_continue_the_uninterrupted_run(tmp_path):
    net = tiny_net()
    whole = make_trainer(copy.deepcopy(net))
    for k in range(3):
        whole.update(*batch(k))
    tr = make_trainer(net, save_dir=str(tmp_path))
    tr.update(*batch(0))
    tr.update(*batch(1))
    tr.save(0, 1, {'note': 'x'}, save_freq=2)                             # (step + 1) % save_freq == 0
    state = torch.load(str(tmp_path / 'checkpoint.pt'), map_location='cpu')
    assert {'state_dict', 'optimizer', 'epoch', 'step', 'note'} <= set(state)
    assert (tmp_path / 'checkpoint_epoch1.pt').exists()
    assert set(state['optimizer']['state'][0]) == {'momentum_buffer'}
    # a new Trainer on the same directory: the checkpoint wins over `ckpt`, the reference's resume rule gives the next step
    resumed = make_trainer(tiny_net(), save_dir=str(tmp_path), ckpt='no-such-ghn.pt')
    assert (resumed.start_epoch, resumed.start_step) == (0, 2)
    assert torch.equal(resumed._optimizer.momentum_buffer, tr._optimizer.momentum_buffer)
    resumed.update(*batch(2))
    assert_same_state(resumed._model, whole._model, rtol=0)
    # the last step of an epoch resumes at the next epoch
    tr.save(0, N_BATCHES - 1, {})
    nxt = make_trainer(tiny_net(), save_dir=str(tmp_path))
    assert (nxt.start_epoch, nxt.start_step) == (1, 0)
    # the stock optimizer reads the same file
    stock = torch.optim.SGD(tiny_net().parameters(), **OPT_ARGS)
    stock.load_state_dict(state['optimizer'])
    assert torch.equal(stock.state_dict()['state'][0]['momentum_buffer'], state['optimizer']['state'][0]['momentum_buffer'])


def test_the_stock_switch_gives_the_same_run(monkeypatch):
    monkeypatch.setenv('GHN3_FUSED_SGD', '0')
    net = tiny_net()
    ref = StockLoop(copy.deepcopy(net))
    tr = make_trainer(net)
    assert isinstance(tr._optimizer, ghn3_amd.optim.StockSGD)
    for k in range(3):
        tr.update(*batch(k))
        ref.update(*batch(k))
    assert_same_state(net, ref.model, rtol=0)
    tr.scheduler_step()
    assert tr.get_lr() == pytest.approx(0.005)


def test_a_nan_batch_is_skipped():
    net = tiny_net()
    tr = make_trainer(net)
    tr.update(*batch(0))
    before = copy.deepcopy(net.state_dict())
    mom = tr._optimizer.momentum_buffer.clone()
    x, y = batch(1)
    x[0, 0, 0, 0] = float('nan')
    tr.update(x, y)
    for k, v in net.state_dict().items():
        if 'running' not in k and 'num_batches' not in k:                # (the forward did update the BatchNorm statistics)
            assert torch.equal(v, before[k]), k
    assert torch.equal(tr._optimizer.momentum_buffer, mom)
    assert math.isfinite(tr.metrics.avg()['loss']) and float(tr.metrics.cnt) == 8     # the step is not in the averages


def test_what_the_plain_branch_refuses(monkeypatch):
    for kw in ({'bce': True}, {'mixup': True}, {'opt': 'lamb'}, {'opt': 'adamw'}):
        with pytest.raises(NotImplementedError):
            make_trainer(tiny_net(), **kw)
    monkeypatch.setattr(trainer_module, 'is_ddp', lambda: True)           # a data-parallel run
    with pytest.raises(NotImplementedError):
        make_trainer(tiny_net())


def test_compile_mode_is_accepted():
    tr = make_trainer(tiny_net(), compile_mode='max-autotune')
    tr.update(*batch(0))


def test_a_ghn_with_sgd_still_raises():
    import recipe
    ghn = ghn3_amd.GHN3(**recipe.TINY_CFG)
    with pytest.raises(NotImplementedError, match='AdamW'):
        make_trainer(ghn)
