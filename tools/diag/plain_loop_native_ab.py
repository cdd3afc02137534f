"""The plain-network loop of examples/train_ddp.py (SmallResNet, batch 64, 32 x 32 seeded random images, SGD through
ghn3_amd.Trainer) with and without native_layers, each from a cold start -- a fresh process per measurement:
    python tools/diag/plain_loop_native_ab.py [--steps 40] [--repeats 2]
Per process: `first` = the first update, from the call to the end of a device synchronise (it includes loading code objects and,
on the stock path, MIOpen's choice of algorithms; for native_layers also the torch.fx trace), `steady` = the mean of the
following updates after three more warm-up steps, synchronised at both ends.  The processes alternate between the two settings.
The child prints one JSON line; the parent repeats them and a summary line.  `--census`: instead of timing, print what
ghn3_amd.nativize did with the network (its report) and the autograd nodes of one training step by name -- which layers of a
nativized plain network still run on stock ATen / MIOpen kernels."""
import argparse
import collections
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'examples'))


def _setup(native):
    import torch
    from ghn3_amd import Trainer
    from train_ddp import SmallResNet
    torch.manual_seed(0)
    model = SmallResNet(10)
    tr = Trainer(model, opt='sgd', opt_args={'lr': 0.025, 'weight_decay': 3e-5, 'momentum': 0.9}, scheduler='cosine', n_batches=1000,
                 grad_clip=5, device='cuda', log_interval=1000, label_smoothing=0.1, epochs=1, native_layers=native)
    gen = torch.Generator().manual_seed(1)
    return torch, tr, torch.randn(64, 3, 32, 32, generator=gen).cuda(), torch.randint(0, 10, (64,), generator=gen).cuda()


def child(native, steps):
    torch, tr, images, targets = _setup(native)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.update(images, targets)
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    for _ in range(3):
        tr.update(images, targets)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.update(images, targets)
    torch.cuda.synchronize()
    steady = (time.perf_counter() - t0) / steps
    print(json.dumps({'native_layers': bool(native), 'first_ms': round(1e3 * first, 2), 'steady_ms': round(1e3 * steady, 3), 'steps': steps,
                      'loss': round(float(tr.metrics.avg()['loss']), 5)}))


def census():
    torch, tr, images, targets = _setup(True)
    nat = tr._plain_forward_model()
    print(nat.report())
    nat.train()
    loss = torch.nn.functional.cross_entropy(nat(images), targets)
    seen, todo, names = set(), [loss.grad_fn], collections.Counter()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names[type(fn).__name__] += 1
        todo += [f for f, _ in fn.next_functions]
    for name, n in sorted(names.items()):
        print('%4d %s' % (n, name))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=2)
    ap.add_argument('--child', type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument('--census', action='store_true')
    args = ap.parse_args()
    if args.census:
        return census()
    if args.child is not None:
        return child(args.child, args.steps)
    rows = []
    for _ in range(args.repeats):
        for native in (0, 1):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', str(native), '--steps', str(args.steps)],
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
            if out.returncode != 0 or not line:
                print(out.stdout)
                raise SystemExit('the measurement process failed (exit status %d): nothing more is started' % out.returncode)
            print(line[-1])
            rows.append(json.loads(line[-1]))
    for native in (False, True):
        mine = [r for r in rows if r['native_layers'] == native]
        print('native_layers=%-5s first %s ms, steady %s ms per step' % (native, [r['first_ms'] for r in mine], [r['steady_ms'] for r in mine]))


if __name__ == '__main__':
    main()
