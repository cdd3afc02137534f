"""The "act" node of the dense-convolution family (conv -> BatchNorm [-> + skip] -> ReLU: ghn3_conv_bn_act_fwd / _bwd) against
the stock `conv2d + batch_norm (+ add) + relu`, forward + backward, in one process on one MI355X:
    python tools/tnet_resblock_bench.py [--reps 20] [--rounds 5]
Shapes: the 3 x 3 convolutions of a ResNet-18 at 32 x 32 inputs, batch 64, and bottleneck shapes at batch 32.  Each shape runs
with and without a skip tensor.  native = the node on channels_last tensors (what it sees inside a nativized network); stock = the
three or four ATen / MIOpen layers on NCHW tensors.  Both are warmed; the timed rounds alternate between the two (device events
around `reps` calls, the median of `rounds` rounds and their spread = max - min); max dev = the largest relative L2 deviation of
the node's output and gradients from the stock layers' on the timed inputs.  The last line is the same as JSON."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ghn3_amd import target_ops as T  # noqa: E402

SHAPES = [  # N, C_in, C_out, H, k, stride
    (64, 64, 64, 32, 3, 1), (64, 128, 128, 16, 3, 1), (64, 256, 256, 8, 3, 1), (64, 512, 512, 4, 3, 1),
    (32, 64, 256, 56, 1, 1), (32, 128, 128, 28, 3, 1), (32, 1024, 2048, 7, 1, 1)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tnet_resblock_bench measures on an MI355X: no GPU here, nothing measured')
    print('%-30s %10s %8s %10s %8s %7s %9s' % ('N C_in C_out HxW k skip', 'native ms', 'spread', 'stock ms', 'spread', 'ratio', 'max dev'))
    rows = []
    for (N, Ci, Co, H, k, st) in SHAPES:
        for skip in (False, True):
            g = torch.Generator(device='cuda').manual_seed(1)
            pad = k // 2
            x = torch.randn(N, Ci, H, H, device='cuda', generator=g)
            params = [torch.randn(Co, Ci, k, k, device='cuda', generator=g) / (Ci * k * k) ** 0.5,
                      1 + 0.3 * torch.randn(Co, device='cuda', generator=g), 0.2 * torch.randn(Co, device='cuda', generator=g)]
            Ho = (H + 2 * pad - k) // st + 1
            res = torch.randn(N, Co, Ho, Ho, device='cuda', generator=g) if skip else None
            up = torch.randn(N, Co, Ho, Ho, device='cuda', generator=g)
            xs, ps = x.clone().requires_grad_(True), [p.clone().requires_grad_(True) for p in params]
            rs = res.clone().requires_grad_(True) if skip else None
            cl = torch.channels_last
            xn, pn = x.contiguous(memory_format=cl).requires_grad_(True), [p.clone().requires_grad_(True) for p in params]
            rn = res.contiguous(memory_format=cl).requires_grad_(True) if skip else None
            upn = up.contiguous(memory_format=cl)
            assert T.ConvBnAct.applicable(xn, pn[0], pn[1], pn[2], rn, st, pad, 1)

            def stock():
                out = T.conv_act_reference(xs, *ps, rs, st, pad)
                return [out] + list(torch.autograd.grad(out, [xs] + ps + ([rs] if skip else []), up))

            def native():
                out, _ = T.conv_bn_act(xn, *pn, rn, st, pad)
                return [out] + list(torch.autograd.grad(out, [xn] + pn + ([rn] if skip else []), upn))
            dev = max(rel(a, b) for a, b in zip(native(), stock()))
            tn, ts = rounds_of([native, stock], args.reps, args.rounds)
            row = dict(N=N, C_in=Ci, C_out=Co, H=H, k=k, stride=st, skip=skip, native_ms=round(statistics.median(tn), 4),
                       stock_ms=round(statistics.median(ts), 4), native_spread_ms=round(max(tn) - min(tn), 4),
                       stock_spread_ms=round(max(ts) - min(ts), 4), max_rel_dev=dev,
                       native_rounds_ms=[round(t, 4) for t in tn], stock_rounds_ms=[round(t, 4) for t in ts])
            rows.append(row)
            print('%-30s %10.3f %8.3f %10.3f %8.3f %7.2f %9.2e' % ('%d %d %d %dx%d %d %s' % (N, Ci, Co, H, H, k, 'skip' if skip else '-'),
                                                                    row['native_ms'], row['native_spread_ms'], row['stock_ms'],
                                                                    row['stock_spread_ms'], row['native_ms'] / row['stock_ms'], dev))
    print(json.dumps({'tool': 'tnet_resblock_bench', 'reps': args.reps, 'rounds': args.rounds, 'shapes': rows}))


if __name__ == '__main__':
    main()
