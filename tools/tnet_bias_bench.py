"""The "bias" node of the dense-convolution family (conv + bias [+ skip] -> ReLU: ghn3_conv_bias_act_fwd / _bwd) against the
stock `conv2d(bias) + relu`, in one process on one MI355X, and the example loop with and without it in fresh processes:
    python tools/tnet_bias_bench.py [--reps 20] [--rounds 5] [--steps 30] [--skip-loop]
1. accuracy: the node's out, dx, dw, dbias against the stock layers in fp64 (computed on the CPU), worst per-slice error (a
   slice's L2 error over the RMS slice norm of the reference; slices: per channel, per position, per sample / per C_out, per C_in,
   per tap), at VGG-16's convolution shapes for 32 x 32 inputs, batch 32;
2. time: forward + backward at VGG-16's convolution shapes, batch 32, 32 x 32 and 224 x 224 inputs.  native = the node on
   channels_last tensors (what it sees inside a nativized network; the 3-channel image is padded to four channels inside the
   timed call, as the runner does); stock = F.conv2d(x, w, bias) + F.relu on NCHW tensors.  Both are warmed -- MIOpen's
   algorithm search is outside the timed window --; the timed rounds alternate between the two (device events around `reps` calls,
   the median of `rounds` rounds and their spread = max - min);
3. the example loop: `examples/train_ddp.py`'s SmallVgg under the plain Trainer, batch 64, once with native_layers + native_biased
   and once on the stock layers, each in a FRESH process with an empty MIOpen user database (the native run first): the time of the
   first update (host clock, synchronised: the cold start) and the mean of the following `steps` updates.
The last line is the same as JSON."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ghn3_amd import target_ops as T  # noqa: E402

VGG16 = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 512)]
# N, C_in, C_out, H: the distinct 3 x 3 / stride 1 / pad 1 convolutions of VGG-16 and the map each one sees
SHAPES = {32: [(32, ci, co, 32 >> (k // 2 if k < 8 else 4)) for k, (ci, co) in enumerate(VGG16)],
          224: [(32, ci, co, 224 >> (k // 2 if k < 8 else 4)) for k, (ci, co) in enumerate(VGG16)]}


def rounds_of(fns, reps, rounds):
    """Per function the times (ms per call) of `rounds` rounds of `reps` calls; the functions alternate within a round."""
    for fn in fns:
        for _ in range(3):
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


def slice_error(got, ref, axes_list):
    """Worst per-slice error: for every axis set the L2 error of a slice (over all other axes) over the reference's RMS slice norm."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    worst = 0.0
    for axes in axes_list:
        others = [a for a in range(r.dim()) if a not in axes]
        err = ((g - r) ** 2).sum(others).sqrt() if others else (g - r).abs()
        worst = max(worst, float(err.max() / (r.norm() / err.numel() ** 0.5)))
    return worst


def inputs(N, Ci, Co, H, dev='cuda'):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, Ci, H, H, generator=g)
    w = torch.randn(Co, Ci, 3, 3, generator=g) * (2.0 / (Ci * 9)) ** 0.5
    b = 0.5 * torch.randn(Co, generator=g)
    up = torch.randn(N, Co, H, H, generator=g)
    return [t.to(dev) for t in (x, w, b, up)]


def native_call(x, w, b, up):
    xin, win = T._image_pad(x, w)
    out = T.conv_bias_act(xin, win, b, None, 1, 1, 1, True, False)
    return [out] + list(torch.autograd.grad(out, [x, w, b], up))


def stock_call(x, w, b, up):
    out = F.relu(F.conv2d(x, w, b, 1, 1))
    return [out] + list(torch.autograd.grad(out, [x, w, b], up))


def accuracy():
    print('%-22s %9s %9s %9s %9s' % ('fp64: N C_in C_out HxW', 'out', 'dx', 'dw', 'dbias'))
    rows = []
    act, wg, vec = [(1,), (2, 3), (0,)], [(0,), (1,), (2, 3)], [(0,)]
    for (N, Ci, Co, H) in SHAPES[32]:
        x, w, b, up = inputs(N, Ci, Co, H, 'cpu')
        x64, w64, b64 = [t.double().requires_grad_(True) for t in (x, w, b)]
        y = F.conv2d(x64, w64, b64, 1, 1)
        up = torch.where(y.detach().abs() < 2e-3, torch.zeros_like(up), up)         # (the ReLU's kink: a sign flip is no error)
        ref = [F.relu(y)] + list(torch.autograd.grad(F.relu(y), [x64, w64, b64], up.double()))
        xn = x.cuda().contiguous(memory_format=torch.channels_last if Ci > 3 else torch.contiguous_format).requires_grad_(True)
        wn, bn = w.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
        got = native_call(xn, wn, bn, up.cuda())
        errs = [slice_error(a, r, ax) for a, r, ax in zip(got, ref, (act, act, wg, vec))]
        rows.append(dict(N=N, C_in=Ci, C_out=Co, H=H, out=errs[0], dx=errs[1], dw=errs[2], dbias=errs[3]))
        print('%-22s %9.2e %9.2e %9.2e %9.2e' % ('%d %d %d %dx%d' % (N, Ci, Co, H, H), *errs))
    return rows


def timing(reps, rounds):
    print('%-22s %10s %8s %10s %8s %7s' % ('N C_in C_out HxW', 'native ms', 'spread', 'stock ms', 'spread', 'ratio'))
    rows = []
    for size, shapes in SHAPES.items():
        for (N, Ci, Co, H) in shapes:
            x, w, b, up = inputs(N, Ci, Co, H)
            cl = torch.channels_last
            xs, ws, bs = [t.clone().requires_grad_(True) for t in (x, w, b)]
            xn = (x.contiguous(memory_format=cl) if Ci > 3 else x.clone()).requires_grad_(True)
            wn, bn = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
            upn = up.contiguous(memory_format=cl)
            assert T.ConvBiasAct.applicable(*T._image_pad(xn, wn), bn, None, 1, 1, 1)
            r = reps if H <= 56 else max(2, reps // 5)
            tn, ts = rounds_of([lambda: native_call(xn, wn, bn, upn), lambda: stock_call(xs, ws, bs, up)], r, rounds)
            row = dict(input=size, N=N, C_in=Ci, C_out=Co, H=H, reps=r, native_ms=round(statistics.median(tn), 4),
                       stock_ms=round(statistics.median(ts), 4), native_spread_ms=round(max(tn) - min(tn), 4),
                       stock_spread_ms=round(max(ts) - min(ts), 4))
            rows.append(row)
            print('%-22s %10.3f %8.3f %10.3f %8.3f %7.2f' % ('%d %d %d %dx%d' % (N, Ci, Co, H, H), row['native_ms'],
                                                             row['native_spread_ms'], row['stock_ms'], row['stock_spread_ms'],
                                                             row['native_ms'] / row['stock_ms']))
            del x, w, b, up, xs, ws, bs, xn, wn, bn, upn
            torch.cuda.empty_cache()
    return rows


def loop_child(native, steps):
    """One fresh process: SmallVgg under the plain Trainer; the first update alone, then `steps` more."""
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import train_ddp as E
    from ghn3_amd import Trainer
    torch.manual_seed(0)
    model = E.SmallVgg(10)
    tr = Trainer(model, opt='sgd', opt_args={'lr': 0.025, 'weight_decay': 3e-5, 'momentum': 0.9}, scheduler='cosine',
                 n_batches=steps + 1, grad_clip=5, device='cuda', log_interval=10 ** 6, label_smoothing=0.1, epochs=1,
                 native_layers=native, native_biased=native)
    g = torch.Generator().manual_seed(1)
    images, targets = torch.randn(64, 3, 32, 32, generator=g).cuda(), torch.randint(0, 10, (64,), generator=g).cuda()
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
    step = (time.perf_counter() - t0) / steps
    rep = tr._forward_model.report() if native else None
    print(json.dumps(dict(native=native, first_update_s=round(first, 4), step_ms=round(1e3 * step, 4), steps=steps,
                          loss=float(tr.metrics.avg()['loss']), stock_convs=None if rep is None else len(rep['stock_convs']),
                          windows=None if rep is None else rep['windows'])))


def loop(steps):
    rows = []
    for native in (True, False):                                   # (the native run first: it leaves nothing MIOpen could reuse)
        with tempfile.TemporaryDirectory() as db:
            env = dict(os.environ, MIOPEN_USER_DB_PATH=db, MIOPEN_CUSTOM_CACHE_DIR=db)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', 'native' if native else 'stock',
                                  '--steps', str(steps)], env=env, capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            raise SystemExit('the %s loop ended with %d:\n%s' % ('native' if native else 'stock', out.returncode, out.stderr[-2000:]))
        rows.append(json.loads(out.stdout.strip().splitlines()[-1]))
        print('example loop, %-22s first update %.3f s, then %.3f ms per update (%d updates)'
              % ('native_biased:' if native else 'stock layers:', rows[-1]['first_update_s'], rows[-1]['step_ms'], steps))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--skip-loop', action='store_true')
    ap.add_argument('--child', choices=('native', 'stock'), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tnet_bias_bench measures on an MI355X: no GPU here, nothing measured')
    if args.child:
        return loop_child(args.child == 'native', args.steps)
    # (the loops first: this process has not opened the GPU's convolution library yet, and they run one at a time)
    loops = [] if args.skip_loop else loop(args.steps)
    acc = accuracy()
    rows = timing(args.reps, args.rounds)
    print(json.dumps({'tool': 'tnet_bias_bench', 'reps': args.reps, 'rounds': args.rounds, 'accuracy': acc, 'shapes': rows,
                      'loop': loops}))


if __name__ == '__main__':
    main()
