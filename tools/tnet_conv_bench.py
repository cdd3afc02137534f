"""Micro-benchmark of the dense-convolution op (ghn3_conv_bn_fwd / _bwd) on the shapes the training loop's architecture stream
produces (batch 64, 32 x 32 images): microseconds per forward / backward, and the same for the stock MIOpen layers.
--wide: six blocks of a WIDE network instead (1024 .. 4096 channels at 4 x 4 and 2 x 2, batch 64; torch.nn-flavour modules taking
and returning NCHW tensors, so the native setting pays its layout copies): forward + backward of the same call with
GHN3_NATIVE_OPS=1 (above 512 channels: Depthwise + the dense-convolution family) and =0 (the stock ATen / MIOpen layers, WARM: their
find step is paid before the timing), alternated round by round, median of ROUNDS=5 rounds of REPS calls with max - min."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch
import torch.nn.functional as F
from ghn3_amd import target_ops as T

SHAPES = [  # C_in, C_out, H, (kh, kw), stride, pad
    (32, 32, 16, (3, 3), 1, 1), (64, 64, 8, (3, 3), 1, 1), (128, 128, 4, (3, 3), 1, 1), (256, 256, 4, (3, 3), 1, 1),
    (64, 64, 16, (5, 5), 1, 2), (128, 128, 8, (5, 5), 1, 2), (64, 64, 8, (1, 7), 1, (0, 3)), (128, 128, 8, (7, 1), 1, (3, 0)),
    (48, 48, 32, (3, 3), 2, 1), (96, 96, 16, (7, 7), 1, 3), (256, 256, 8, (3, 3), 1, 1), (64, 128, 16, (2, 2), 2, 0),
]
REPS = int(os.environ.get('REPS', '30'))


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


WIDE = [  # constructor, arguments, H = W
    ('ReLUConvBN', (1024, 1024, 3, 1, 1), 4), ('ReLUConvBN', (2048, 2048, 1), 2), ('ReLUConvBN', (4096, 1024, 1), 4),
    ('DilConv', (1024, 1024, 3, 1, 2, 2), 4), ('SepConv', (2048, 2048, 3, 1, 1), 2), ('SepConv', (1024, 1024, 5, 1, 2), 4),
]


def wide():
    from ghn3_amd import ops
    rounds = int(os.environ.get('ROUNDS', '5'))
    print('%-44s %22s %22s %8s' % ('block (batch 64)', 'native fwd+bwd us', 'stock fwd+bwd us', 'ratio'))
    for kind, args, hw in WIDE:
        torch.manual_seed(1)
        m = getattr(ops, kind)(*args, norm='bn').cuda().train()
        x = torch.randn(64, args[0], hw, hw, device='cuda', requires_grad=True)
        up = None
        res = {'1': [], '0': []}

        def step():
            m(x).backward(up)

        for setting in ('1', '0'):                             # warm-up of both settings (the stock layers' find step)
            os.environ['GHN3_NATIVE_OPS'] = setting
            up = torch.randn_like(m(x)) if up is None else up
            step()
        for _ in range(rounds):
            for setting in ('1', '0'):
                os.environ['GHN3_NATIVE_OPS'] = setting
                res[setting].append(timed(step))
        med = {k: statistics.median(v) for k, v in res.items()}
        print('%-44s %12.1f +- %-7.1f %12.1f +- %-7.1f %8.2f' % (
            '%s%s %dx%d' % (kind, args, hw, hw), med['1'], max(res['1']) - min(res['1']), med['0'], max(res['0']) - min(res['0']),
            med['0'] / med['1']))
    os.environ['GHN3_NATIVE_OPS'] = '1'


if '--wide' in sys.argv[1:]:
    wide()
    sys.exit(0)

print('%-34s %10s %10s %10s %10s   %s' % ('shape', 'fwd us', 'bwd us', 'stock fwd', 'stock bwd', 'GFLOP fwd'))
tot = [0.0, 0.0, 0.0, 0.0]
for ci, co, hw, ks, st, pad in SHAPES:
    x = torch.randn(64, ci, hw, hw, device='cuda').contiguous(memory_format=torch.channels_last).requires_grad_(True)
    w = (torch.randn(co, ci, *ks, device='cuda') / (ci * ks[0] * ks[1]) ** 0.5).requires_grad_(True)
    g, b = torch.ones(co, device='cuda', requires_grad=True), torch.zeros(co, device='cuda', requires_grad=True)
    out, _ = T.conv_bn(x, w, g, b, st, pad, 1, True)
    up = torch.randn_like(out)
    xs = x.detach().contiguous(memory_format=torch.contiguous_format).requires_grad_(True)

    def fwd():
        with torch.no_grad():
            T.conv_bn(x, w, g, b, st, pad, 1, True)

    def fwdbwd():
        o, _ = T.conv_bn(x, w, g, b, st, pad, 1, True)
        o.backward(up)

    def sfwd():
        with torch.no_grad():
            F.batch_norm(F.conv2d(F.relu(xs), w, None, st, pad), None, None, g, b, True, 0.1, 1e-5)

    ups = up.contiguous(memory_format=torch.contiguous_format)

    def sfwdbwd():
        o = F.batch_norm(F.conv2d(F.relu(xs), w, None, st, pad), None, None, g, b, True, 0.1, 1e-5)
        o.backward(ups)

    tf, tfb, sf, sfb = timed(fwd), timed(fwdbwd), timed(sfwd), timed(sfwdbwd)
    gf = 2.0 * out.numel() * ci * ks[0] * ks[1] / 1e9
    for k, v in enumerate((tf, tfb - tf, sf, sfb - sf)):
        tot[k] += v
    print('%-34s %10.1f %10.1f %10.1f %10.1f   %.2f' % ('%d->%d %dx%d k%s s%s' % (ci, co, hw, hw, ks, st), tf, tfb - tf, sf, sfb - sf, gf))
print('%-34s %10.1f %10.1f %10.1f %10.1f' % ('sum', *tot))
