"""Micro-benchmark of the `msa` op of the target networks (ops._TransformerLayer, the pre-LN transformer layer of the ViT-style
networks) on the fused op family ghn3_msa_fwd / _bwd against the stock ATen layers (GHN3_NATIVE_MSA=0): forward + backward of
one layer per shape, timed with device events after warm-up, the two paths alternated round by round (median of the rounds).
Per shape: ms per layer for each path, device kernel launches per layer (torch.profiler; MSA_BENCH_COUNT=0 skips the count,
e.g. under rocprofv3) and the largest relative deviation of the native output and gradients from the stock ones.
    python tools/tnet_msa_bench.py            (REPS=20 iterations per timing, ROUNDS=5)
    python tools/tnet_msa_bench.py --wide     also the wide layers (C <= 1024, head dim <= 64: target_ops.MsaWideLayer under
                                              GHN3_NATIVE_MSA_WIDE=1) against the stock path, with the spread of the rounds"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
from ghn3_amd import ops

SHAPES = [(64, 32, 11, 1), (64, 64, 11, 1), (64, 128, 11, 1), (16, 32, 14, 1), (16, 64, 14, 1), (16, 128, 14, 1)]   # B, C, H=W, stride
WIDE_SHAPES = [(64, 512, 8, 11, 1), (64, 512, 8, 8, 1), (16, 512, 8, 14, 1), (8, 768, 12, 14, 4), (8, 1024, 16, 14, 4)]   # B, C, heads, H=W, mlp_ratio
REPS = int(os.environ.get('REPS', '20'))
ROUNDS = int(os.environ.get('ROUNDS', '5'))
COUNT = os.environ.get('MSA_BENCH_COUNT', '1') != '0'


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def step(layer, x, up, native):
    os.environ['GHN3_NATIVE_MSA'] = '1' if native else '0'
    layer.zero_grad(set_to_none=True)
    x.grad = None
    out = layer(x)
    out.backward(up)
    return out


def timed(layer, x, up, native):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        step(layer, x, up, native)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def launches(layer, x, up, native):
    if not COUNT:
        return -1
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step(layer, x, up, native)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception:                         # (no device tracing in this build)
        return -1


def main():
    assert torch.cuda.is_available(), 'tnet_msa_bench measures on the GPU'
    print('%-22s %10s %10s %8s %10s %10s %10s' % ('B C HxW stride', 'native ms', 'stock ms', 'ratio', 'launches n', 'launches s',
                                                   'max dev'))
    rows = []
    for B, C, H, s in SHAPES:
        torch.manual_seed(0)
        layer = ops.TransformerLayer(C, stride=s).cuda().train()
        x = torch.randn(B, C, H, H, device='cuda', requires_grad=True)
        Ho = (H - 1) // s + 1
        up = torch.randn(B, C, Ho, Ho, device='cuda')
        res = {}
        for native in (True, False):
            for _ in range(3):
                out = step(layer, x, up, native)
            torch.cuda.synchronize()
            res[native] = [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
        dev = max(rel(a, b) for a, b in zip(res[True], res[False]))
        t = {True: [], False: []}
        for _ in range(ROUNDS):
            for native in (True, False):
                t[native].append(timed(layer, x, up, native))
        tn, ts = statistics.median(t[True]), statistics.median(t[False])
        ln, ls = launches(layer, x, up, True), launches(layer, x, up, False)
        print('%-22s %10.3f %10.3f %8.2f %10d %10d %10.2e' % ('%d %d %dx%d s%d' % (B, C, H, H, s), tn, ts, tn / ts, ln, ls, dev))
        rows.append(dict(B=B, C=C, H=H, W=H, stride=s, native_ms=round(tn, 4), stock_ms=round(ts, 4),
                         native_launches=ln, stock_launches=ls, max_rel_dev=dev,
                         native_rounds_ms=[round(v, 4) for v in t[True]], stock_rounds_ms=[round(v, 4) for v in t[False]]))
    print(json.dumps({'tool': 'tnet_msa_bench', 'reps': REPS, 'rounds': ROUNDS, 'shapes': rows}))
    if '--wide' in sys.argv[1:]:
        wide()


def wide():
    """The wide layers: native = MsaWideLayer (GHN3_NATIVE_MSA_WIDE=1), stock = GHN3_NATIVE_MSA=0; spread = max - min."""
    os.environ['GHN3_NATIVE_MSA_WIDE'] = '1'
    print('%-24s %10s %8s %10s %8s %8s %10s %10s %10s' % ('B C heads HxW ratio', 'native ms', 'spread', 'stock ms', 'spread',
                                                          'ratio', 'launches n', 'launches s', 'max dev'))
    rows = []
    for B, C, heads, H, ratio in WIDE_SHAPES:
        torch.manual_seed(0)
        layer = ops.TransformerLayer(C, num_heads=heads, mlp_ratio=ratio).cuda().train()
        x = torch.randn(B, C, H, H, device='cuda', requires_grad=True)
        up = torch.randn(B, C, H, H, device='cuda')
        res = {}
        for native in (True, False):
            for _ in range(3):
                out = step(layer, x, up, native)
            torch.cuda.synchronize()
            fns = [out.grad_fn] + [f for f, _ in out.grad_fn.next_functions if f is not None]    # (a layout copy may follow the node)
            assert any(type(f).__name__ == 'MsaWideLayerBackward' for f in fns) == native, fns
            res[native] = [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
        dev = max(rel(a, b) for a, b in zip(res[True], res[False]))
        t = {True: [], False: []}
        for _ in range(ROUNDS):
            for native in (True, False):
                t[native].append(timed(layer, x, up, native))
        tn, ts = statistics.median(t[True]), statistics.median(t[False])
        sn, ss = max(t[True]) - min(t[True]), max(t[False]) - min(t[False])
        ln, ls = launches(layer, x, up, True), launches(layer, x, up, False)
        print('%-24s %10.3f %8.3f %10.3f %8.3f %8.2f %10d %10d %10.2e' % ('%d %d %d %dx%d r%d' % (B, C, heads, H, H, ratio), tn, sn,
                                                                          ts, ss, tn / ts, ln, ls, dev))
        rows.append(dict(B=B, C=C, heads=heads, H=H, W=H, mlp_ratio=ratio, native_ms=round(tn, 4), stock_ms=round(ts, 4),
                         native_spread_ms=round(sn, 4), stock_spread_ms=round(ss, 4), native_launches=ln, stock_launches=ls,
                         max_rel_dev=dev, native_rounds_ms=[round(v, 4) for v in t[True]],
                         stock_rounds_ms=[round(v, 4) for v in t[False]]))
    print(json.dumps({'tool': 'tnet_msa_bench --wide', 'reps': REPS, 'rounds': ROUNDS, 'shapes': rows}))


if __name__ == '__main__':
    main()
