"""Micro-benchmark of the end of a target network -- global average pool + classifier `Linear [ReLU Dropout Linear]` + the
label-smoothed cross-entropy -- on the fused op families ghn3_head_* / ghn3_xent_* against the stock ATen layers
(GHN3_NATIVE_HEAD=0): forward + backward per network on the training stream's shapes (NHWC features as the fused cells leave
them, dropout active), timed with device events after warm-up, the two paths alternated round by round (median of the rounds).
Per shape: ms per network for each path, device kernel launches per network (torch.profiler; HEAD_BENCH_COUNT=0 skips the
count) and the largest relative deviation of the native loss and gradients from the stock ones with the dropout off.
    python tools/tnet_head_bench.py            (REPS=20 iterations per timing, ROUNDS=5)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
from ghn3_amd import ops, target_ops

SHAPES = [   # B, C, H=W, K, fc_layers, fc_dim
    (64, 256, 8, 10, 1, 64), (64, 256, 8, 10, 2, 64), (64, 256, 8, 10, 2, 256), (64, 512, 7, 1000, 1, 64),
    (64, 512, 7, 1000, 2, 64), (64, 512, 7, 1000, 2, 256)]
REPS = int(os.environ.get('REPS', '20'))
ROUNDS = int(os.environ.get('ROUNDS', '5'))
COUNT = os.environ.get('HEAD_BENCH_COUNT', '1') != '0'


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def make_head(C, K, fc_layers, fc_dim, p):
    dims = [C] + [fc_dim] * (fc_layers - 1) + [K]           # (ops.network_plan's head table)
    spec = []
    for k in range(len(dims) - 1):
        spec += ([('relu',), ('dropout',)] if k else []) + [('linear', dims[k], dims[k + 1])]
    head = ops._layer_seq(ops._TorchLayers, 'bn', spec).cuda().train()
    for m in head:
        if isinstance(m, torch.nn.Dropout):
            m.p = p
    return torch.nn.AdaptiveAvgPool2d(1), head


def step(pool, head, x, y, native):
    os.environ['GHN3_NATIVE_HEAD'] = '1' if native else '0'
    head.zero_grad(set_to_none=True)
    x.grad = None
    logits = target_ops.run_classifier_head(pool, head, x) if native else None
    if logits is None:
        logits = head(pool(x.contiguous()).reshape(x.shape[0], -1))
    ce, _ = target_ops.meta_cross_entropy([logits], y, 0.1)
    ce.sum().backward()
    return ce


def timed(pool, head, x, y, native):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        step(pool, head, x, y, native)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def launches(pool, head, x, y, native):
    if not COUNT:
        return -1
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step(pool, head, x, y, native)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:                         # (no device tracing in this build)
        return -1


def main():
    assert torch.cuda.is_available(), 'tnet_head_bench measures on the GPU'
    print('%-28s %10s %10s %8s %10s %10s %10s' % ('B C HxW K fc_layers fc_dim', 'native ms', 'stock ms', 'ratio', 'launches n',
                                                   'launches s', 'max dev'))
    rows = []
    for B, C, H, K, fl, fd in SHAPES:
        torch.manual_seed(0)
        x = torch.randn(B, C, H, H, device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_(True)
        y = torch.randint(0, K, (B,), device='cuda')
        pool, head = make_head(C, K, fl, fd, 0.0)
        res = {}
        for native in (True, False):
            for _ in range(3):
                ce = step(pool, head, x, y, native)
            torch.cuda.synchronize()
            res[native] = [ce.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in head.parameters()]
        dev = max(rel(a, b) for a, b in zip(res[True], res[False]))
        for m in head:
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.5                     # (timed and counted as trained: dropout active)
        t = {True: [], False: []}
        for _ in range(ROUNDS):
            for native in (True, False):
                t[native].append(timed(pool, head, x, y, native))
        tn, ts = statistics.median(t[True]), statistics.median(t[False])
        ln, ls = launches(pool, head, x, y, True), launches(pool, head, x, y, False)
        name = '%d %d %dx%d K%d fc%d %d' % (B, C, H, H, K, fl, fd)
        print('%-28s %10.3f %10.3f %8.2f %10d %10d %10.2e' % (name, tn, ts, tn / ts, ln, ls, dev))
        rows.append(dict(B=B, C=C, H=H, W=H, K=K, fc_layers=fl, fc_dim=fd, native_ms=round(tn, 4), stock_ms=round(ts, 4),
                         native_launches=ln, stock_launches=ls, max_rel_dev=dev,
                         native_rounds_ms=[round(v, 4) for v in t[True]], stock_rounds_ms=[round(v, 4) for v in t[False]]))
    os.environ['GHN3_NATIVE_HEAD'] = '1'
    print(json.dumps({'tool': 'tnet_head_bench', 'reps': REPS, 'rounds': ROUNDS, 'shapes': rows}))


if __name__ == '__main__':
    main()
