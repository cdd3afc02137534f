"""Micro-benchmark of eval-mode BatchNorm blocks (a tracking BatchNorm that is not in training mode normalises with its running
statistics): the forward under torch.no_grad() of torch.nn-flavour blocks and of one whole network, in two settings of the SAME
call:
  native  GHN3_NATIVE_EVALBN=1: target_ops.dwpw_bn_eval / conv_bn_eval (ghn3_dwpw_frozen_fwd, ghn3_conv_frozen_fwd);
  stock   GHN3_NATIVE_EVALBN=0: the stock ATen / MIOpen layers, layer by layer (what such a block ran on before the ops existed).
Both take and return NCHW tensors, as a torch.nn-flavour network hands them over (the native setting pays its two layout copies).
Timed with device events after warm-up, the settings alternated round by round: median of the rounds and their spread
(max - min).  Shapes: the 18 depthwise + pointwise shapes of tools/tnet_nonorm_bench.py, the dense shapes of
tools/tnet_conv_bench.py, and the DARTS-like network of tests/golden/network_cases.py at C = 32, batch 64, 32 x 32.
    python tools/tnet_evalbn_bench.py            (REPS=20 iterations per timing, ROUNDS=5)"""
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import torch
from torch import nn
from ghn3_amd import ops, target_ops as T

DWPW_SHAPES = [(64, C, H, ks) for H in (32, 16, 8) for C in (32, 64, 128) for ks in (3, 5)]      # N, C, H = W, ks
CONV_SHAPES = [  # C_in, C_out, H, (kh, kw), stride, pad   (batch 64)
    (32, 32, 16, (3, 3), 1, 1), (64, 64, 8, (3, 3), 1, 1), (128, 128, 4, (3, 3), 1, 1), (256, 256, 4, (3, 3), 1, 1),
    (64, 64, 16, (5, 5), 1, 2), (128, 128, 8, (5, 5), 1, 2), (64, 64, 8, (1, 7), 1, (0, 3)), (128, 128, 8, (7, 1), 1, (3, 0)),
    (48, 48, 32, (3, 3), 2, 1), (96, 96, 16, (7, 7), 1, 3), (256, 256, 8, (3, 3), 1, 1), (64, 128, 16, (2, 2), 2, 0),
]
REPS = int(os.environ.get('REPS', '20'))
ROUNDS = int(os.environ.get('ROUNDS', '5'))
SETTINGS = ('native', 'stock')


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def seeded_eval(m, seed):
    """The module on the GPU in eval mode, its norm layers with seeded affine pairs and running statistics."""
    g = torch.Generator().manual_seed(seed)
    m = m.cuda()
    with torch.no_grad():
        for sub in m.modules():
            if isinstance(sub, nn.BatchNorm2d):
                C = sub.num_features
                sub.running_mean.copy_(0.5 * torch.randn(C, generator=g))
                sub.running_var.copy_(0.5 + 1.5 * torch.rand(C, generator=g))
                sub.weight.copy_(1 + 0.3 * torch.randn(C, generator=g))
                sub.bias.copy_(0.2 * torch.randn(C, generator=g))
    return m.eval()


def call(setting, fn):
    os.environ['GHN3_NATIVE_EVALBN'] = '1' if setting == 'native' else '0'
    with torch.no_grad():
        return fn()


def timed(setting, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        call(setting, fn)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(label, fn, reps):
    res = {}
    for s in SETTINGS:
        for _ in range(3):
            out = call(s, fn)
        torch.cuda.synchronize()
        res[s] = out.detach().clone()
    ms = {s: [] for s in SETTINGS}
    for _ in range(ROUNDS):
        for s in SETTINGS:
            ms[s].append(timed(s, fn, reps))
    med = {s: statistics.median(ms[s]) for s in SETTINGS}
    spread = {s: max(ms[s]) - min(ms[s]) for s in SETTINGS}
    slower = bool(med['native'] > med['stock'] + max(spread.values()))
    dev = rel(res['native'], res['stock'])
    print('%-28s %s %12.2f %10.2e %s' % (label, ' '.join('%13.4f (%6.4f)' % (med[s], spread[s]) for s in SETTINGS),
                                         med['native'] / med['stock'], dev, 'SLOWER' if slower else ''))
    return dict(shape=label, native_over_stock=round(med['native'] / med['stock'], 3), max_rel_dev_vs_stock=dev,
                native_slower_beyond_spread=slower, **{s + '_ms': round(med[s], 4) for s in SETTINGS},
                **{s + '_spread_ms': round(spread[s], 4) for s in SETTINGS},
                **{s + '_rounds_ms': [round(v, 4) for v in ms[s]] for s in SETTINGS})


def main():
    assert torch.cuda.is_available(), 'tnet_evalbn_bench measures on the GPU'
    assert T.enabled(), 'GHN3_NATIVE_OPS=0 leaves nothing to compare'
    print('%-28s %22s %22s %12s %10s' % ('shape', 'native ms (spread)', 'stock ms (spread)', 'native/stock', 'max dev'))
    rows = {'dwpw': [], 'conv': [], 'network': []}
    for N, C, H, ks in DWPW_SHAPES:
        torch.manual_seed(N + C + H + ks)
        layers = list(seeded_eval(nn.Sequential(nn.ReLU(), nn.Conv2d(C, C, ks, 1, ks // 2, groups=C, bias=False),
                                                nn.Conv2d(C, C, 1, bias=False), nn.BatchNorm2d(C)), C + H + ks))
        x = torch.randn(N, C, H, H, device='cuda')
        rows['dwpw'].append(measure('dwpw %d %d %dx%d k%d' % (N, C, H, H, ks), lambda: T.run_block(layers, x), REPS))
    for ci, co, hw, ks, st, pad in CONV_SHAPES:
        torch.manual_seed(ci + co + hw + sum(ks))
        layers = list(seeded_eval(nn.Sequential(nn.ReLU(), nn.Conv2d(ci, co, ks, st, pad, bias=False), nn.BatchNorm2d(co)),
                                  ci + co + hw))
        x = torch.randn(64, ci, hw, hw, device='cuda')
        rows['conv'].append(measure('conv %d->%d %dx%d k%s s%d' % (ci, co, hw, hw, 'x'.join(map(str, ks)), st),
                                    lambda: T.run_conv_block(layers, x), REPS))
    import network_cases
    torch.manual_seed(0)
    net = seeded_eval(ops.Network(genotype=ops.Genotype(**network_cases._CONV), C=32, num_classes=10, n_cells=5,
                                  is_imagenet_input=False), 1)
    images = torch.randn(64, 3, 32, 32, device='cuda')
    rows['network'].append(measure('network C=32 64x3x32x32', lambda: net(images)[0], max(1, REPS // 4)))
    slower = [r['shape'] for k in rows for r in rows[k] if r['native_slower_beyond_spread']]
    print('native slower than stock beyond the spread: %s' % (', '.join(slower) if slower else 'no shape'))
    print(json.dumps({'tool': 'tnet_evalbn_bench', 'reps': REPS, 'rounds': ROUNDS, 'slower_beyond_spread': slower, **rows}))


if __name__ == '__main__':
    main()
