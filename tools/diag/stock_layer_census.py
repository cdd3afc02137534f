"""Diagnostic: which layers of the training loop's target networks still run on stock ATen / MIOpen kernels?
Runs Trainer.update on the architecture stream of examples/train_ghn_ddp.py and counts, per step, the stock Conv2d / BatchNorm2d /
Linear / pooling calls and F.cross_entropy calls by configuration and by the module class that issued them.
--bn-free-prob P: the share of the stream drawn without norm layers (norm=None), as in examples/train_ghn_ddp.py.
--width-mult M: multiplies the drawn width C of every architecture (4: the widths of the `wide` evaluation split).
--large-images: the ImageNet-sized stream of examples/train_ghn_ddp.py --imagenet (SampledNets(large_images=True), 224 x 224 inputs,
1000 classes, max_shape 16 x 16); --batch B: images per step (default 64; a small one keeps the large-image census short)."""
import argparse
import collections
import inspect
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
import torch
from ghn3_amd import GHN3, Trainer, light_ops
from ghn3_amd.deepnets1m import SampledNets
from ghn3_amd.graph import GraphBatch

STEPS = int(os.environ.get('CENSUS_STEPS', '12'))
_ap = argparse.ArgumentParser()
_ap.add_argument('--bn-free-prob', type=float, default=0.0)
_ap.add_argument('--width-mult', type=int, default=1)
_ap.add_argument('--large-images', action='store_true')
_ap.add_argument('--batch', type=int, default=64)
BN_FREE_PROB, WIDTH_MULT = _ap.parse_args().bn_free_prob, _ap.parse_args().width_mult
LARGE, BATCH = _ap.parse_args().large_images, _ap.parse_args().batch
SIDE, CLASSES, MAX_K = (224, 1000, 16) if LARGE else (32, 10, 11)
counts = collections.Counter()
host = collections.Counter()


def caller():
    for fr in inspect.stack()[2:8]:
        slf = fr.frame.f_locals.get('self')
        if slf is not None and type(slf).__module__.endswith('ops') and not type(slf).__name__.startswith(('Sequential', 'Conv2d')):
            return type(slf).__name__
    return '?'


def wrap(cls, describe):
    orig = cls.forward

    def fwd(self, x):
        key = (cls.__name__, caller(), describe(self, x))
        t0 = time.perf_counter()
        y = orig(self, x)
        host[key] += time.perf_counter() - t0
        counts[key] += 1
        return y
    cls.forward = fwd


wrap(light_ops.Conv2d, lambda m, x: 'w%s s%s p%s d%s g%d x%s' % (tuple(m.weight.shape), m.stride, m.padding, m.dilation, m.groups,
                                                                 tuple(x.shape[1:])))
wrap(light_ops.BatchNorm2d, lambda m, x: 'x%s' % (tuple(x.shape[1:]),))
wrap(light_ops.Linear, lambda m, x: 'w%s x%s' % (tuple(m.weight.shape), tuple(x.shape)))
wrap(light_ops.AvgPool2d, lambda m, x: '')
wrap(light_ops.MaxPool2d, lambda m, x: '')
wrap(light_ops.AdaptiveAvgPool2d, lambda m, x: '')
_cross_entropy = torch.nn.functional.cross_entropy


def counted_cross_entropy(*args, **kwargs):
    counts[('cross_entropy', 'F', '')] += 1
    return _cross_entropy(*args, **kwargs)


torch.nn.functional.cross_entropy = counted_cross_entropy

hid, layers, heads = 64, 3, 8
config = {'max_shape': (hid, hid, MAX_K, MAX_K), 'num_classes': CLASSES, 'weight_norm': True, 've': True, 'layernorm': True, 'hid': hid,
          'layers': layers, 'heads': heads}
torch.manual_seed(0)
ghn = GHN3(**config, compute='f16')
trainer = Trainer(ghn, opt='adamw', opt_args={'lr': 4e-4, 'weight_decay': 1e-2}, scheduler='cosine', n_batches=STEPS, grad_clip=5,
                  device='cuda', log_interval=100, amp=False, predparam_wd=3e-5, verbose=False)
gen = torch.Generator().manual_seed(1)
images = torch.randn(BATCH, 3, SIDE, SIDE, generator=gen).cuda()
targets = torch.randint(0, CLASSES, (BATCH,), generator=gen).cuda()
nets = SampledNets(large_images=LARGE, seed=0, max_nodes=400, bn_free_prob=BN_FREE_PROB, width_mult=WIDTH_MULT)
print('architecture stream: seed 0, max_nodes 400, bn_free_prob %g, width_mult %d, %d steps of 8 networks%s' % (
    BN_FREE_PROB, WIDTH_MULT, STEPS, ', large images (%d x %d x %d, %d classes)' % (BATCH, SIDE, SIDE, CLASSES) if LARGE else ''))
for step in range(STEPS):
    gb = GraphBatch([nets[step * 8 + k] for k in range(8)], dense=True)
    trainer.update(images, targets, graphs=gb)
torch.cuda.synchronize()
by_kind = collections.Counter()
for (kind, who, cfg), n in counts.items():
    by_kind[(kind, who)] += n
print('stock calls per step: Linear %.1f, AdaptiveAvgPool2d %.1f, F.cross_entropy %.1f' % tuple(
    sum(n for (k, _), n in by_kind.items() if k == kind) / STEPS for kind in ('Linear', 'AdaptiveAvgPool2d', 'cross_entropy')))
print('stock layer calls per step, by (layer, issuing class):')
for (kind, who), n in by_kind.most_common():
    t = sum(v for (k2, w2, _), v in host.items() if (k2, w2) == (kind, who))
    print('  %-20s %-24s %7.1f calls/step  %7.2f ms host/step (forward only)' % (kind, who, n / STEPS, 1e3 * t / STEPS))
print('stock Conv2d calls in all: %d, stock BatchNorm2d calls in all: %d' % (
    sum(n for (k, _), n in by_kind.items() if k == 'Conv2d'), sum(n for (k, _), n in by_kind.items() if k == 'BatchNorm2d')))
print('top Conv2d configurations:')
for (kind, who, cfg), n in counts.most_common(400):
    if kind == 'Conv2d':
        print('  %6.2f /step  %-18s %s' % (n / STEPS, who, cfg))
