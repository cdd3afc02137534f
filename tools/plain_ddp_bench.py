#!/usr/bin/env python3
"""
What the data-parallel plain-network step adds on one MI355X, on the parameter lists of tools/sgd_step_bench.py (ResNet-50: 161
tensors, ResNet-18: 62 tensors, random gradients):

  pack   ghn3_mt_pack (the gradients' pointer table through the pinned ring + one launch) against the same gather by the stock
         expressions: torch.cat(..., out=flat) and torch._foreach_copy_(views of flat, gradients);
  step   FusedSGD.step with FlatGradReducer(force=True) in a 1-rank RCCL group (pack, the collectives on the communication
         stream, norm + update from the flat buffer) against FusedSGD.step without a reducer.

    python tools/plain_ddp_bench.py [--blocks 8] [--steps 30] [--warmup 20]

All candidates of a comparison run in ONE process in alternating blocks after a warm-up of each.  Per call: the host time to
ISSUE it (host clock around a block of calls, no synchronise inside; the stream is empty when the block starts) and the device
time (a pair of events around every call).  Medians over all blocks / all calls.  Multi-GPU figures need a second GPU: with
one, the script says so and measures nothing of the kind.
"""
import argparse
import ctypes
import json
import os
import socket
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def compare(fns, args):
    """{name: (host issue ms per call, device ms per call)} -- medians; alternating blocks."""
    host, dev = {k: [] for k in fns}, {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.blocks):
        for k, fn in fns.items():
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for a, b in events:
                a.record()
                fn()
                b.record()
            host[k].append(1e3 * (time.perf_counter() - t0) / args.steps)
            torch.cuda.synchronize()
            dev[k] += [a.elapsed_time(b) for a, b in events]
    return {k: (statistics.median(host[k]), statistics.median(dev[k])) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=8)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the benchmark needs the GPU: a CPU time says nothing about it'
    import torch.distributed as dist
    from sgd_step_bench import NETS, HYPER, MAX_NORM, make_params
    from ghn3_amd import FusedSGD, _lib as L, optim as O
    from ghn3_amd.ddp_utils import FlatGradReducer
    from ghn3_amd.nn import pinned_ring
    print('device: %s, torch %s, %d GPU(s) visible' % (torch.cuda.get_device_name(0), torch.__version__, torch.cuda.device_count()))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(s.getsockname()[1]))
    s.close()
    dist.init_process_group('nccl', rank=0, world_size=1)
    results = {}
    lib = L.load()
    try:
        for name in NETS:
            ps = make_params(name, 1)
            grads = [p.grad for p in ps]
            sizes = [g.numel() for g in grads]
            offs = O.flat_layout(sizes)
            flat = torch.zeros(int(offs[-1]), device='cuda')
            dense = torch.zeros(sum(sizes), device='cuda')
            rec, chunks, n_chunks = O._mt_tables(flat.data_ptr(), offs, sizes, 'cuda')
            views = [flat[int(o):int(o) + n].view(g.shape) for o, n, g in zip(offs, sizes, grads)]
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            ptrs = np.asarray([g.data_ptr() for g in grads], dtype=np.int64)

            def mt_pack():
                tab = pinned_ring('cuda').upload(ptrs, 'cuda')
                lib.ghn3_mt_pack(rec.data_ptr(), tab.data_ptr(), chunks.data_ptr(), n_chunks, stream)

            def cat():
                torch.cat([g.reshape(-1) for g in grads], out=dense)

            def foreach():
                torch._foreach_copy_(views, grads)
            mt_pack()
            foreach_flat = flat.clone()
            flat.zero_()
            foreach()
            assert torch.equal(flat, foreach_flat), 'the three gathers must agree'
            res = {'pack': compare({'ghn3_mt_pack': mt_pack, 'torch.cat': cat, 'foreach_copy': foreach}, args)}
            for k, (h, d) in res['pack'].items():
                print('%-9s pack  %-13s %3d tensors %5.1f M floats: host %.4f ms per call, device %.4f ms per call (%.2f TB/s of 8 '
                      'bytes per float)' % (name, k, len(sizes), sum(sizes) / 1e6, h, d, 8 * sum(sizes) / (d * 1e-3) / 1e12))
            del flat, dense, views
            plain_p, red_p = make_params(name, 1), make_params(name, 1)
            plain = FusedSGD(plain_p, max_grad_norm=MAX_NORM, **HYPER)
            steps = {'no reducer': plain.step}
            for algo in ('rsag', 'allreduce'):
                steps['reducer ' + algo] = FusedSGD(make_params(name, 1) if algo != 'rsag' else red_p, max_grad_norm=MAX_NORM,
                                                    reducer=FlatGradReducer(force=True, algo=algo), **HYPER).step
            res['step'] = compare(steps, args)
            for k, (h, d) in res['step'].items():
                print('%-9s step  %-17s host %.4f ms per step, device %.4f ms per step' % (name, k, h, d))
            results[name] = res
    finally:
        dist.destroy_process_group()
    if torch.cuda.device_count() < 2:
        print('one GPU visible: the two-rank step (examples/train_ddp.py under torchrun, 2 ranks against 1) and the exchange\'s '
              'share of it are UNMEASURED')
    print(json.dumps(results))


if __name__ == '__main__':
    main()
