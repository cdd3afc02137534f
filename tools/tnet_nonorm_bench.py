"""Micro-benchmark of the depthwise + pointwise block WITHOUT a norm layer (`DilConv` / one half of `SepConv` of a norm=None
network: ReLU -> depthwise k x k convolution -> 1 x 1 convolution), forward + backward of one block per shape, in three settings:
  plain   target_ops.dwpw     (ghn3_dwpw_plain_fwd / _bwd), channels_last input;
  stock   the three stock ATen / MIOpen layers (what such a block ran on before the op existed, GHN3_NATIVE_OPS=0), NCHW input;
  bn      target_ops.dwpw_bn  (the with-norm member of the family at the same shape: the plain op does a subset of its work).
Timed with device events after warm-up, the settings alternated round by round: median of the rounds and their spread
(max - min).  Shapes: the training shapes quoted in DESIGN section 3 -- batch 64 at 32 x 32 / 16 x 16 / 8 x 8, C = 32 / 64 / 128,
ks 3 / 5.
    python tools/tnet_nonorm_bench.py            (REPS=20 iterations per timing, ROUNDS=5)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
import torch.nn.functional as F
from ghn3_amd import target_ops as T

SHAPES = [(64, C, H, ks) for H in (32, 16, 8) for C in (32, 64, 128) for ks in (3, 5)]      # N, C, H = W, ks
REPS = int(os.environ.get('REPS', '20'))
ROUNDS = int(os.environ.get('ROUNDS', '5'))
SETTINGS = ('plain', 'stock', 'bn')


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def step(setting, t, up, pad):
    x = t['x_nchw'] if setting == 'stock' else t['x']
    for p in (x, t['w_dw'], t['w_pw'], t['gamma'], t['beta']):
        p.grad = None
    if setting == 'plain':
        out = T.dwpw(x, t['w_dw'], t['w_pw'], padding=pad)
    elif setting == 'bn':
        out = T.dwpw_bn(x, t['w_dw'], t['w_pw'], t['gamma'], t['beta'], padding=pad)[0]
    else:
        out = F.conv2d(F.conv2d(F.relu(x), t['w_dw'], None, 1, pad, 1, groups=x.shape[1]), t['w_pw'])
    out.backward(up)
    return out, x


def timed(setting, t, up, pad):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        step(setting, t, up, pad)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def main():
    assert torch.cuda.is_available(), 'tnet_nonorm_bench measures on the GPU'
    print('%-16s %22s %22s %22s %12s %12s %10s' % ('N C HxW ks', 'plain ms (spread)', 'stock ms (spread)', 'bn ms (spread)',
                                                  'plain/stock', 'plain/bn', 'max dev'))
    rows = []
    for N, C, H, ks in SHAPES:
        g = torch.Generator().manual_seed(N + C + H + ks)
        pad = ks // 2
        x = torch.randn(N, C, H, H, generator=g).cuda()
        t = dict(x=x.contiguous(memory_format=torch.channels_last).requires_grad_(True), x_nchw=x.clone().requires_grad_(True),
                 w_dw=(torch.randn(C, 1, ks, ks, generator=g) / ks).cuda().requires_grad_(True),
                 w_pw=(torch.randn(C, C, 1, 1, generator=g) / C ** 0.5).cuda().requires_grad_(True),
                 gamma=torch.ones(C, device='cuda', requires_grad=True), beta=torch.zeros(C, device='cuda', requires_grad=True))
        up = torch.randn(N, C, H, H, generator=g).cuda()
        up_cl = up.contiguous(memory_format=torch.channels_last)
        ups = {'plain': up_cl, 'bn': up_cl, 'stock': up}
        res = {}
        for s in SETTINGS:
            for _ in range(3):
                out, xin = step(s, t, ups[s], pad)
            torch.cuda.synchronize()
            res[s] = [out.detach().clone(), xin.grad.clone(), t['w_dw'].grad.clone(), t['w_pw'].grad.clone()]
        dev = max(rel(a, b) for a, b in zip(res['plain'], res['stock']))
        ms = {s: [] for s in SETTINGS}
        for _ in range(ROUNDS):
            for s in SETTINGS:
                ms[s].append(timed(s, t, ups[s], pad))
        med = {s: statistics.median(ms[s]) for s in SETTINGS}
        spread = {s: max(ms[s]) - min(ms[s]) for s in SETTINGS}
        print('%-16s %s %12.2f %12.2f %10.2e' % (
            '%d %d %dx%d k%d' % (N, C, H, H, ks), ' '.join('%13.4f (%6.4f)' % (med[s], spread[s]) for s in SETTINGS),
            med['plain'] / med['stock'], med['plain'] / med['bn'], dev))
        rows.append(dict(N=N, C=C, H=H, W=H, ks=ks, max_rel_dev_vs_stock=dev,
                         **{s + '_ms': round(med[s], 4) for s in SETTINGS}, **{s + '_spread_ms': round(spread[s], 4) for s in SETTINGS},
                         **{s + '_rounds_ms': [round(v, 4) for v in ms[s]] for s in SETTINGS},
                         plain_within_bn_plus_spread=bool(med['plain'] <= med['bn'] + spread['bn'])))
    print(json.dumps({'tool': 'tnet_nonorm_bench', 'reps': REPS, 'rounds': ROUNDS, 'shapes': rows}))


if __name__ == '__main__':
    main()
