"""Shared builders of the data-parallel plain-Trainer tests (test_plain_ddp_cpu.py, test_gpu_plain_ddp.py): networks, batches,
the float64 oracle, and the gloo workers of the world-2 runs (mp.spawn needs them importable by name)."""

import atexit
import copy
import functools
import os
import shutil
import socket
import tempfile

import torch
import torch.nn as nn
import torch.nn.functional as F

OPT_ARGS = {'lr': 0.05, 'momentum': 0.9, 'weight_decay': 1e-4}
GRAD_CLIP, SMOOTH, N_BATCHES = 5, 0.1, 8
# How far the world-2 fp32 run may be from the float64 oracle, in units of the one-process fp32 run's own distance: both are
# fp32 roundings of the same sums in another order.  Measured after three steps: 4.69e-8 against 4.68e-8 for the parameters,
# 1.90e-7 against 2.01e-7 for the momentum -- a ratio of 1; 2 holds with room to spare (the issue allows up to 4).
MARGIN = 2.0


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def norm_free_net(seed=7):
    """conv, ReLU, conv, global pool, linear: no BatchNorm, so two half batches and the whole batch compute the same function."""
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.ReLU(), nn.Conv2d(6, 8, 3, padding=1), nn.AdaptiveAvgPool2d(1),
                         nn.Flatten(), nn.Linear(8, 10))


def bn_net(seed=7):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.BatchNorm2d(6), nn.ReLU(), nn.AdaptiveAvgPool2d(2), nn.Flatten(),
                         nn.Linear(24, 10))


def batch(k, n=8, scale=4.0):
    """(scale 4: the gradient norm of the first steps is above GRAD_CLIP, so the clip coefficient takes part)"""
    g = torch.Generator().manual_seed(50 + k)
    return scale * torch.randn(n, 3, 8, 8, generator=g), torch.randint(0, 10, (n,), generator=g)


def make_trainer(model, **kw):
    from ghn3_amd import Trainer
    args = dict(opt='sgd', opt_args=dict(OPT_ARGS), scheduler='mstep', scheduler_args={'milestones': [1], 'gamma': 0.1},
                n_batches=N_BATCHES, grad_clip=GRAD_CLIP, device='cpu', label_smoothing=SMOOTH, epochs=3, log_interval=1)
    args.update(kw)
    return Trainer(model, **args)


def init_group(rank, world, port):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from ghn3_amd.ddp_utils import setup_ddp
    return setup_ddp()


def spawn(worker, world, *args):
    """One process per rank under gloo; what every rank left in the shared dict, by rank."""
    import torch.multiprocessing as mp
    ret = mp.Manager().dict()
    mp.spawn(worker, args=(world, free_port(), ret) + args, nprocs=world, join=True)
    assert sorted(ret.keys()) == list(range(world))
    return dict(ret)


def cat(ts):
    return torch.cat([t.detach().reshape(-1).double().cpu() for t in ts])


def rel(a, b):
    """Relative L2 distance over the concatenation of two tensor lists (b: the reference)."""
    a, b = cat(a), cat(b)
    return float((a - b).norm() / b.norm())


def state_of(tr):
    """(parameters, momentum buffers) of a plain Trainer as CPU clones."""
    ps = [p.detach().clone().cpu() for p in tr._model.parameters()]
    return ps, [tr._optimizer._buf(i).detach().clone().cpu() for i in range(len(ps))]


def state_of_model(tr):
    return [v.detach().clone().cpu() for v in tr._model.state_dict().values()]


def oracle64(net, steps):
    """`steps` whole-batch updates in float64: cross entropy with label smoothing, sgd_reference_ on a double() copy."""
    from ghn3_amd.optim import sgd_reference_
    m = copy.deepcopy(net).double()
    ps = list(m.parameters())
    bufs = [torch.zeros_like(p) for p in ps]
    for k in steps:
        x, y = batch(k)
        loss = F.cross_entropy(m(x.double()), y, label_smoothing=SMOOTH)
        grads = torch.autograd.grad(loss, ps)
        with torch.no_grad():
            sgd_reference_(ps, grads, bufs, OPT_ARGS['lr'], OPT_ARGS['momentum'], OPT_ARGS['weight_decay'], False,
                           float(GRAD_CLIP), 1.0)
    return [p.detach() for p in ps], bufs


# ---------------------------------------------------------------------------------------------------------------------
# world-2 workers
# ---------------------------------------------------------------------------------------------------------------------
def halves_worker(rank, world, port, ret, save_dir):
    """Three steps, each rank on its half of the batch of 8; rank 0 writes a checkpoint after the second."""
    import torch.distributed as dist
    init_group(rank, world, port)
    try:
        tr = make_trainer(norm_free_net(), data_parallel=True, save_dir=save_dir)
        for k in range(3):
            x, y = batch(k)
            lo = rank * 4
            tr.update(x[lo:lo + 4], y[lo:lo + 4])
            if k == 1:
                tr.save(0, 1, {}, save_freq=2)
                dist.barrier()
        ret[rank] = state_of(tr) + (tr.metrics.avg(),)
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def halves_run():
    """(per-rank results of halves_worker, the directory rank 0 saved its checkpoint to) -- run once, shared by the tests."""
    d = tempfile.mkdtemp(prefix='plain_ddp_')
    atexit.register(shutil.rmtree, d, True)
    return spawn(halves_worker, 2, d), d


def replica_worker(rank, world, port, ret):
    """For both exchanges: a BatchNorm network built from ANOTHER seed per rank (rank 1 also ran a forward, so its
    num_batches_tracked differs), its state after construction, four steps on different data per rank with every step's
    parameters, momentum and norm, then the buffers before / after scheduler_step()."""
    import torch.distributed as dist
    from ghn3_amd.ddp_utils import FlatGradReducer
    init_group(rank, world, port)
    try:
        out = {}
        for algo in ('rsag', 'mesh'):
            net = bn_net(seed=7 + 13 * rank)
            if rank == 1:
                net.train()
                net(batch(99)[0])
            tr = make_trainer(net, data_parallel=True)
            assert type(tr._optimizer.reducer) is FlatGradReducer and tr._optimizer.reducer.compress is None
            tr._optimizer.reducer = FlatGradReducer(algo=algo)
            rec = {'start': {k: v.clone() for k, v in net.state_dict().items()}, 'steps': []}
            for k in range(4):
                x, y = batch(10 * rank + k)
                # (the Trainer's own step, with the optimizer's norm kept: update() returns the metrics)
                norm_box = []
                step = tr._optimizer.step
                tr._optimizer.step = lambda **kw: norm_box.append(step(**kw)) or norm_box[-1]
                tr.update(x, y)
                tr._optimizer.step = step
                rec['steps'].append(state_of(tr) + (float(norm_box[0]),))
            rec['buffers_before'] = [b.clone() for b in net.buffers()]
            tr.scheduler_step()
            rec['buffers_after'] = [b.clone() for b in net.buffers()]
            out[algo] = rec
        ret[rank] = out
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def replica_run():
    return spawn(replica_worker, 2)


def poison_worker(rank, world, port, ret):
    """One clean step, then one in which rank 1 alone has a NaN in one gradient element."""
    import torch.distributed as dist
    init_group(rank, world, port)
    try:
        net = bn_net()
        tr = make_trainer(net, data_parallel=True)
        armed = []
        w = next(net.parameters())

        def hook(g):
            if armed and rank == 1:
                g = g.clone()
                g.view(-1)[3] = float('nan')
            return g
        w.register_hook(hook)
        tr.update(*batch(20 + rank))
        before = state_of(tr)
        armed.append(1)
        tr.update(*batch(30 + rank))
        after = state_of(tr)
        tr._sync_skips()
        ret[rank] = (before, after, tr.skipped_updates, float(tr.metrics.cnt))
    finally:
        dist.destroy_process_group()
