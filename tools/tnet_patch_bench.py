"""Micro-benchmark of the patch-embedding op (ghn3_patch_fwd / _bwd, target_ops.patch_embed) on the layer of the ImageNet-sized
ViT-style networks: Conv2d(3, C, 16, stride=16, bias=False) on 64 x 3 x 224 x 224 images, C in {32, 64, 128}.  Forward + backward
of the layer as the network runs it (the image batch needs no gradient, the weight does; the result is handed on NCHW) on the
native op and on the stock Conv2d, alternated round by round: median of ROUNDS=5 rounds of REPS calls with max - min.  The stock
layer is WARM in those rounds; its first forward + backward per shape -- MIOpen's find step, which the training loop pays on the
first visit of every channel count -- is timed once, before anything else touches the shape (wall clock around a synchronise)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
import torch.nn.functional as F
from ghn3_amd import target_ops as T

REPS, ROUNDS = int(os.environ.get('REPS', '20')), int(os.environ.get('ROUNDS', '5'))
N, SIDE, K = 64, 224, 16


def timed(fn):
    fn(); fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / REPS


torch.zeros(1, device='cuda')
torch.cuda.synchronize()
print('%-26s %22s %22s %8s %16s' % ('layer (batch %d, %d x %d)' % (N, SIDE, SIDE), 'native fwd+bwd us', 'stock fwd+bwd us (warm)',
                                    'ratio', 'stock first ms'))
for C in (32, 64, 128):
    torch.manual_seed(C)
    x = torch.randn(N, 3, SIDE, SIDE, device='cuda')
    w = (torch.randn(C, 3, K, K, device='cuda') / (3 * K * K) ** 0.5).requires_grad_(True)
    up = torch.randn(N, C, SIDE // K, SIDE // K, device='cuda')
    assert T.PatchEmbed.applicable(x, w, K, 0, 1)

    def stock():
        w.grad = None
        F.conv2d(x, w, None, K).backward(up)

    def native():
        w.grad = None
        T.patch_embed(x, w, K).contiguous(memory_format=torch.contiguous_format).backward(up)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stock()
    torch.cuda.synchronize()
    first = 1e3 * (time.perf_counter() - t0)
    ref = w.grad.clone()
    native()
    err = float((w.grad - ref).norm() / ref.norm())
    res = {'native': [], 'stock': []}
    for _ in range(ROUNDS):
        res['native'].append(timed(native))
        res['stock'].append(timed(stock))
    med = {k: statistics.median(v) for k, v in res.items()}
    print('%-26s %12.1f +- %-7.1f %12.1f +- %-7.1f %8.2f %16.1f   (dw against stock %.1e)' % (
        '3 -> %d, 16 x 16 / 16' % C, med['native'], max(res['native']) - min(res['native']), med['stock'],
        max(res['stock']) - min(res['stock']), med['stock'] / med['native'], first, err))
