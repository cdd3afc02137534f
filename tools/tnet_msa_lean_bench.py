"""Micro-benchmark of the msa layer's two attention paths (ops._TransformerLayer on target_ops.MsaLayer): GHN3_MSA_LEAN=1 -- the
lean attention of tnet_attn.hip, which saves one float per query row and recomputes P in the backward -- against =0, the
saved-P path.  Forward + backward of one layer per shape, timed with device events after warm-up, the two settings alternated
round by round; per shape and setting the median over the rounds, the spread (max - min) between the rounds, and the peak of
torch.cuda.max_memory_allocated over a step on top of what was allocated before it.  Shapes whose P has 2^31 elements or more
run lean only.  The threshold of `auto` (target_ops.MSA_LEAN_THRESHOLD) follows from the table as tnet_msa_lean_bench's last
line says: the smallest power of two >= 2^24 such that at every measured shape with B heads N^2 at or above it the lean median
is no more than the saved-P median plus the larger of the two spreads at that shape; 2^31 when there is none.
    python tools/tnet_msa_lean_bench.py [--saved-only]      (REPS=5 iterations per timing, ROUNDS=5)
--saved-only times GHN3_MSA_LEAN=0 alone (also on a tree that has no lean path, where the variable is ignored)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
from ghn3_amd import ops

SHAPES = [(64, 64, 11, 11), (8, 128, 14, 14), (64, 128, 16, 16), (128, 64, 28, 28), (64, 32, 32, 32), (16, 32, 64, 64)]   # B, C, H, W
HEADS = 8
REPS = int(os.environ.get('REPS', '5'))
ROUNDS = int(os.environ.get('ROUNDS', '5'))


def step(layer, x, up, lean):
    os.environ['GHN3_MSA_LEAN'] = '1' if lean else '0'
    layer.zero_grad(set_to_none=True)
    x.grad = None
    out = layer(x)
    assert 'MsaLayerBackward' in (type(out.grad_fn).__name__, type(out.grad_fn.next_functions[0][0]).__name__), \
        'the layer left the fused op'
    out.backward(up)
    return out


def timed(layer, x, up, lean):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        step(layer, x, up, lean)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def peak(layer, x, up, lean):
    layer.zero_grad(set_to_none=True)
    x.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step(layer, x, up, lean)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    assert torch.cuda.is_available(), 'tnet_msa_lean_bench measures on the GPU'
    saved_only = '--saved-only' in sys.argv
    print('%-16s %8s | %9s %8s %9s | %9s %8s %9s | %6s' % ('B C HxW', 'P elems', 'lean ms', 'spread', 'peak MB', 'saved ms', 'spread',
                                                         'peak MB', 'ratio'))
    rows = []
    for B, C, H, W in SHAPES:
        p_elems = B * HEADS * (H * W) ** 2
        modes = [m for m in (True, False) if not (m and saved_only) and not (not m and p_elems >= 2 ** 31)]
        if not modes:
            continue
        torch.manual_seed(0)
        layer = ops.TransformerLayer(C).cuda().train()
        x = torch.randn(B, C, H, W, device='cuda', requires_grad=True)
        up = torch.randn(B, C, H, W, device='cuda')
        for m in modes:
            for _ in range(2):
                step(layer, x, up, m)
        t = {m: [] for m in modes}
        for _ in range(ROUNDS):
            for m in modes:
                t[m].append(timed(layer, x, up, m))
        row = dict(B=B, C=C, H=H, W=W, p_elems=p_elems)
        for m in modes:
            k = 'lean' if m else 'saved'
            row[k + '_ms'] = round(statistics.median(t[m]), 4)
            row[k + '_spread_ms'] = round(max(t[m]) - min(t[m]), 4)
            row[k + '_peak_mb'] = round(peak(layer, x, up, m), 1)
            row[k + '_rounds_ms'] = [round(v, 4) for v in t[m]]
        f = lambda k, w, p: ('%*.*f' % (w, p, row[k])) if k in row else ' ' * (w - 1) + '-'      # noqa: E731
        ratio = '%6.2f' % (row['lean_ms'] / row['saved_ms']) if len(modes) == 2 else '     -'
        print('%-16s %8.1e | %s %s %s | %s %s %s | %s' % ('%d %d %dx%d' % (B, C, H, W), p_elems, f('lean_ms', 9, 3),
                                                       f('lean_spread_ms', 8, 3), f('lean_peak_mb', 9, 1), f('saved_ms', 9, 3),
                                                       f('saved_spread_ms', 8, 3), f('saved_peak_mb', 9, 1), ratio))
        rows.append(row)
        del layer, x, up
        torch.cuda.empty_cache()
    both = [r for r in rows if 'lean_ms' in r and 'saved_ms' in r]
    threshold = None
    if both:
        threshold = 2 ** 31
        for e in range(24, 31):
            at = [r for r in both if r['p_elems'] >= 2 ** e]
            if at and all(r['lean_ms'] <= r['saved_ms'] + max(r['lean_spread_ms'], r['saved_spread_ms']) for r in at):
                threshold = 2 ** e
                break
        print('threshold by the rule: 2^%d' % (threshold.bit_length() - 1))
    print(json.dumps({'tool': 'tnet_msa_lean_bench', 'reps': REPS, 'rounds': ROUNDS, 'saved_only': saved_only,
                      'threshold': threshold, 'shapes': rows}))


if __name__ == '__main__':
    main()
