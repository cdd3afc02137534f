#!/usr/bin/env python3
"""
Times the optimizer step of a plain network on one MI355X: ghn3_amd.FusedSGD.step (two launches over a tensor table) against
stock nn.utils.clip_grad_norm_ + torch.optim.SGD (foreach), on the parameter lists of a ResNet-50 (161 tensors, 25.6 M floats)
and a ResNet-18 (62 tensors, 11.7 M floats) with random gradients.

    python tools/sgd_step_bench.py [--blocks 8] [--steps 30] [--warmup 20]

Both optimizers run in ONE process in alternating blocks of `steps` steps after a warm-up of each; every step is timed with a
pair of device events (what the step occupies the stream for, launch gaps included) and every block with a host clock around a
synchronise (what a training loop pays, host time of the step included).  Reported: medians over all steps / all blocks.
The fused step moves 24 bytes per parameter (4 for the norm, 20 for the update); the bandwidth figure is that over the event time.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def resnet_shapes(bottleneck, layers, num_classes=1000):
    """Parameter shapes of torchvision's ResNet layout, in module order."""
    shapes = [(64, 3, 7, 7), (64,), (64,)]
    inplanes = 64
    for i, (planes, n) in enumerate(zip((64, 128, 256, 512), layers)):
        out = planes * 4 if bottleneck else planes
        for b in range(n):
            if bottleneck:
                convs = [(planes, inplanes, 1, 1), (planes, planes, 3, 3), (out, planes, 1, 1)]
            else:
                convs = [(planes, inplanes, 3, 3), (planes, planes, 3, 3)]
            for c in convs:
                shapes += [c, (c[0],), (c[0],)]
            if b == 0 and (i > 0 or inplanes != out):
                shapes += [(out, inplanes, 1, 1), (out,), (out,)]
            inplanes = out
    return shapes + [(num_classes, inplanes), (num_classes,)]


NETS = {'resnet50': (True, (3, 4, 6, 3), 161, 25557032), 'resnet18': (False, (2, 2, 2, 2), 62, 11689512)}
HYPER = dict(lr=0.05, momentum=0.9, weight_decay=1e-4)
MAX_NORM = 5.0


def make_params(name, seed):
    bottleneck, layers, n_tensors, n_floats = NETS[name]
    shapes = resnet_shapes(bottleneck, layers)
    assert len(shapes) == n_tensors and sum(torch.Size(s).numel() for s in shapes) == n_floats, name
    g = torch.Generator(device='cuda').manual_seed(seed)
    ps = [torch.randn(s, device='cuda', generator=g).mul_(0.05).requires_grad_() for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device='cuda', generator=g)
    return ps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=8)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the benchmark needs the GPU: a CPU time says nothing about it'
    assert args.blocks * args.steps >= 200, 'at least 200 timed steps per optimizer'
    from ghn3_amd import FusedSGD
    print('device: %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    results = {}
    for name in NETS:
        fused_p, stock_p = make_params(name, 1), make_params(name, 1)
        fused = FusedSGD(fused_p, max_grad_norm=MAX_NORM, **HYPER)
        stock = torch.optim.SGD(stock_p, foreach=True, **HYPER)

        def stock_step():
            torch.nn.utils.clip_grad_norm_(stock_p, MAX_NORM, foreach=True)
            stock.step()
        steps = {'fused': fused.step, 'stock': stock_step}
        ev_ms, blk_ms = {k: [] for k in steps}, {k: [] for k in steps}
        for fn in steps.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.blocks):
            for k, fn in steps.items():
                events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for a, b in events:
                    a.record()
                    fn()
                    b.record()
                torch.cuda.synchronize()
                blk_ms[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
                ev_ms[k] += [a.elapsed_time(b) for a, b in events]
        n_floats = NETS[name][3]
        res = {}
        for k in steps:
            ev, blk = statistics.median(ev_ms[k]), statistics.median(blk_ms[k])
            res[k] = {'event_ms_median': ev, 'event_ms_min': min(ev_ms[k]), 'block_ms_per_step_median': blk,
                      'block_ms_per_step_min': min(blk_ms[k]), 'block_ms_per_step_max': max(blk_ms[k]), 'steps': len(ev_ms[k])}
            print('%-9s %-6s %3d tensors %5.1f M floats: %.4f ms per step (device events, median of %d; min %.4f)   '
                  '%.4f ms per step (host clock per block of %d, median of %d; %.4f .. %.4f)'
                  % (name, k, NETS[name][2], n_floats / 1e6, ev, len(ev_ms[k]), min(ev_ms[k]), blk, args.steps, args.blocks,
                     min(blk_ms[k]), max(blk_ms[k])))
        res['fused_bytes_per_step'] = 24 * n_floats
        res['fused_tb_per_s'] = 24 * n_floats / (res['fused']['event_ms_median'] * 1e-3) / 1e12
        res['stock_over_fused_events'] = res['stock']['event_ms_median'] / res['fused']['event_ms_median']
        res['stock_over_fused_blocks'] = res['stock']['block_ms_per_step_median'] / res['fused']['block_ms_per_step_median']
        print('%-9s fused: %.2f TB/s of its 24 bytes per parameter; stock / fused = %.2f (events), %.2f (blocks)'
              % (name, res['fused_tb_per_s'], res['stock_over_fused_events'], res['stock_over_fused_blocks']))
        results[name] = res
    print(json.dumps(results))


if __name__ == '__main__':
    main()
