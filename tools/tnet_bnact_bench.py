"""The stand-alone BatchNorm + ReLU node (ghn3_bn_act_fwd / _bwd, target_ops.bn_act) against the stock `batch_norm + relu`, forward
+ backward, in one process on one MI355X:
    python tools/tnet_bnact_bench.py [--reps 20] [--rounds 5]
Part 1, the node: the BatchNorm inputs of a DenseNet-121 at batch 32 (C = 64 ... 1024 at 56^2, 28^2, 14^2, 7^2).  native = the
node on channels_last tensors (what it sees inside a nativized network); stock = the two ATen / MIOpen layers on NCHW tensors.
Both are warmed; the timed rounds alternate between the two (device events around `reps` calls, the median of `rounds` rounds and
their spread = max - min); max dev = the largest relative L2 deviation of the node's output and gradients from the stock layers'.
Beside them the achieved bytes/s of the kernels, timed through the C entry points (no autograd, no allocation in the loop):
  apply    the forward's streaming kernel alone (the frozen forward is that one launch): reads x, writes out = 2 P C 4 bytes;
  fwd      both forward launches: x twice, out once = 3 P C 4 bytes;
  bwd      both backward launches (partial sums + the dx kernel): dout and x twice, dx once = 5 P C 4 bytes;
against the 6.3 TB/s the HBM is good for.  A tensor that fits the 256 MiB Infinity Cache can exceed that figure.
Part 2, modules: a dense layer and a pre-activation block, stock / nativize() / nativize(windows='all'), forward + backward.
The last line is the same as JSON."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ghn3_amd  # noqa: E402
from ghn3_amd import _lib as L  # noqa: E402
from ghn3_amd import target_ops as T  # noqa: E402

HBM_TBS = 6.3
SHAPES = [  # N, C, H: the norm layers' inputs along DenseNet-121 (growth 32; blocks of 6, 12, 24, 16 layers)
    (32, 64, 56), (32, 128, 56), (32, 256, 56), (32, 128, 28), (32, 256, 28), (32, 512, 28),
    (32, 256, 14), (32, 512, 14), (32, 1024, 14), (32, 512, 7), (32, 1024, 7)]


def rounds_of(fns, reps, rounds):
    """Per function the times (ms per call) of `rounds` rounds of `reps` calls; the functions alternate within a round."""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b) / reps)
    return times


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def kernel_rates(x, gamma, beta, up, reps, rounds):
    """TB/s of (apply alone, both forward launches, both backward launches) through the C entry points."""
    lib = L.load()
    N, C, H, W = x.shape
    d = T._BnActDesc(N * H * W, C, 1, 1e-5)
    out, dx = torch.empty_like(x), torch.empty_like(x)
    stats = torch.empty(3 * C, device='cuda')
    mean, var = torch.zeros(C, device='cuda'), torch.ones(C, device='cuda')
    dg, db = torch.empty(C, device='cuda'), torch.empty(C, device='cuda')
    scratch = torch.empty(T._scratch_floats(T._BNACT_SCRATCH, d, 1), device='cuda')
    s = T._stream()
    ref = ctypes.byref(d)

    def apply():
        L._check(lib.ghn3_bn_act_frozen_fwd(ref, *T._ptrs(x, gamma, beta, mean, var, out), s), 'apply')

    def fwd():
        L._check(lib.ghn3_bn_act_fwd(ref, *T._ptrs(x, gamma, beta, out, stats, scratch), s), 'fwd')

    def bwd():
        L._check(lib.ghn3_bn_act_bwd(ref, *T._ptrs(up, x, stats, gamma, beta, dx, dg, db, scratch), s), 'bwd')
    fwd()
    times = rounds_of([apply, fwd, bwd], reps, rounds)
    nbytes = x.numel() * 4
    return [round(k * nbytes / (statistics.median(t) * 1e-3) / 1e12, 3) for k, t in zip((2, 3, 5), times)]


class DenseLayer(nn.Module):
    def __init__(self, cin, growth=32, bn_size=4):
        super().__init__()
        self.norm1, self.conv1 = nn.BatchNorm2d(cin), nn.Conv2d(cin, bn_size * growth, 1, bias=False)
        self.norm2, self.conv2 = nn.BatchNorm2d(bn_size * growth), nn.Conv2d(bn_size * growth, growth, 3, 1, 1, bias=False)

    def forward(self, x):
        y = self.conv1(F.relu(self.norm1(x)))
        return torch.cat([x, self.conv2(F.relu(self.norm2(y)))], 1)


class PreActBlock(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.bn1, self.conv1 = nn.BatchNorm2d(c), nn.Conv2d(c, c, 3, 1, 1, bias=False)
        self.bn2, self.conv2 = nn.BatchNorm2d(c), nn.Conv2d(c, c, 3, 1, 1, bias=False)

    def forward(self, x):
        y = self.conv1(F.relu(self.bn1(x)))
        return self.conv2(F.relu(self.bn2(y))) + x


MODULES = [('dense layer 256 -> 288 at 28^2, N 32', lambda: DenseLayer(256), (32, 256, 28, 28)),
           ('dense layer 512 -> 544 at 14^2, N 32', lambda: DenseLayer(512), (32, 512, 14, 14)),
           ('pre-act block 64 at 32^2, N 64', lambda: PreActBlock(64), (64, 64, 32, 32)),
           ('pre-act block 256 at 8^2, N 64', lambda: PreActBlock(256), (64, 256, 8, 8))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tnet_bnact_bench measures on an MI355X: no GPU here, nothing measured')
    cl = torch.channels_last
    print('%-16s %10s %8s %10s %8s %7s %9s | %8s %8s %8s  (TB/s; HBM %.1f)' % ('N C HxW', 'native ms', 'spread', 'stock ms', 'spread',
                                                                               'ratio', 'max dev', 'apply', 'fwd', 'bwd', HBM_TBS))
    rows = []
    for (N, C, H) in SHAPES:
        g = torch.Generator(device='cuda').manual_seed(1)
        x = torch.randn(N, C, H, H, device='cuda', generator=g)
        params = [1 + 0.3 * torch.randn(C, device='cuda', generator=g), 0.2 * torch.randn(C, device='cuda', generator=g)]
        up = torch.randn(N, C, H, H, device='cuda', generator=g)
        xs, ps = x.clone().requires_grad_(True), [p.clone().requires_grad_(True) for p in params]
        xn, pn = x.contiguous(memory_format=cl).requires_grad_(True), [p.clone().requires_grad_(True) for p in params]
        upn = up.contiguous(memory_format=cl)
        assert T.BnAct.applicable(xn, *pn)

        def stock():
            out = T.bn_act_reference(xs, *ps)
            return [out] + list(torch.autograd.grad(out, [xs] + ps, up))

        def native():
            out, _ = T.bn_act(xn, *pn)
            return [out] + list(torch.autograd.grad(out, [xn] + pn, upn))
        dev = max(rel(a, b) for a, b in zip(native(), stock()))
        tn, ts = rounds_of([native, stock], args.reps, args.rounds)
        rates = kernel_rates(xn.detach(), pn[0].detach(), pn[1].detach(), upn, args.reps, args.rounds)
        row = dict(N=N, C=C, H=H, native_ms=round(statistics.median(tn), 4), stock_ms=round(statistics.median(ts), 4),
                   native_spread_ms=round(max(tn) - min(tn), 4), stock_spread_ms=round(max(ts) - min(ts), 4), max_rel_dev=dev,
                   apply_tbs=rates[0], fwd_tbs=rates[1], bwd_tbs=rates[2], mbytes=round(x.numel() * 4 / 2 ** 20, 1))
        rows.append(row)
        print('%-16s %10.3f %8.3f %10.3f %8.3f %7.2f %9.2e | %8.2f %8.2f %8.2f' % (
            '%d %d %dx%d' % (N, C, H, H), row['native_ms'], row['native_spread_ms'], row['stock_ms'], row['stock_spread_ms'],
            row['native_ms'] / row['stock_ms'], dev, *rates))
    print()
    print('%-40s %10s %12s %10s %9s %9s' % ('module, forward + backward', 'stock ms', 'nativize ms', "'all' ms", 'default/s', "'all'/s"))
    mods = []
    for name, make, shape in MODULES:
        torch.manual_seed(2)
        net = make().cuda()
        x = torch.randn(*shape, device='cuda').requires_grad_(True)
        variants = [net, ghn3_amd.nativize(net, strict=True), ghn3_amd.nativize(net, strict=True, windows='all')]
        params = list(net.parameters())

        def runner(m):
            with torch.no_grad():
                up = torch.ones_like(m(x))               # (dense, in the layout of the variant's own output)

            def run():
                out = m(x)
                return [out] + list(torch.autograd.grad(out, [x] + params, up))
            return run
        fns = [runner(m) for m in variants]
        devs = [max(rel(a, b) for a, b in zip(fn(), fns[0]())) for fn in fns[1:]]
        times = [statistics.median(t) for t in rounds_of(fns, args.reps, args.rounds)]
        row = dict(module=name, stock_ms=round(times[0], 4), nativize_ms=round(times[1], 4), all_ms=round(times[2], 4),
                   windows_all=variants[2].report()['windows'], max_rel_dev=devs)
        mods.append(row)
        print('%-40s %10.3f %12.3f %10.3f %9.2f %9.2f' % (name, times[0], times[1], times[2], times[1] / times[0], times[2] / times[0]))
    print(json.dumps({'tool': 'tnet_bnact_bench', 'reps': args.reps, 'rounds': args.rounds, 'hbm_tbs': HBM_TBS, 'shapes': rows,
                      'modules': mods}))


if __name__ == '__main__':
    main()
