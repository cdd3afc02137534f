"""A/B of one environment switch in the training loop, in ONE process (the protocol of profiles/r07b_train_loop_ab.txt):
Trainer.update on the architecture stream of examples/train_ghn_ddp.py (ghn3tm8, meta-batch 8, 64 images of 32 x 32), the two
settings alternated round by round on the SAME architectures, wall time per step with a device sync around each step.

    python3 tools/diag/train_loop_switch_ab.py GHN3_NATIVE_JOIN          (AB_ROUNDS=3 AB_STEPS=8)

Prints median / min / max per setting and every round's median: the spread between the rounds of one setting is what a
difference between the settings has to be read against."""
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..')
sys.path.insert(0, ROOT)
import torch
from ghn3_amd import GHN3, Trainer
from ghn3_amd.deepnets1m import SampledNets
from ghn3_amd.graph import GraphBatch

SWITCH = sys.argv[1]
ROUNDS, STEPS = int(os.environ.get('AB_ROUNDS', '3')), int(os.environ.get('AB_STEPS', '8'))

hid, layers, heads = 64, 3, 8
config = {'max_shape': (hid, hid, 11, 11), 'num_classes': 10, 'weight_norm': True, 've': True, 'layernorm': True, 'hid': hid,
          'layers': layers, 'heads': heads}
torch.manual_seed(0)
ghn = GHN3(**config, compute='f16')
trainer = Trainer(ghn, opt='adamw', opt_args={'lr': 4e-4, 'weight_decay': 1e-2}, scheduler='cosine',
                  n_batches=2 * (ROUNDS + 1) * STEPS, grad_clip=5, device='cuda', log_interval=10 ** 6, amp=False, predparam_wd=3e-5,
                  verbose=False)
gen = torch.Generator().manual_seed(1)
images = torch.randn(64, 3, 32, 32, generator=gen).cuda()
targets = torch.randint(0, 10, (64,), generator=gen).cuda()
nets = SampledNets(large_images=False, seed=0, max_nodes=400)

times = {'0': [], '1': []}
for rnd in range(ROUNDS + 1):                      # (round 0 warms both settings up on the first architectures: not timed)
    for setting in (('0', '1') if rnd % 2 else ('1', '0')):
        os.environ[SWITCH] = setting
        row = []
        for step in range(STEPS):
            gb = GraphBatch([nets[(rnd * STEPS + step) * 8 + k] for k in range(8)], dense=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.update(images, targets, graphs=gb)
            torch.cuda.synchronize()
            row.append(1e3 * (time.perf_counter() - t0))
        if rnd:
            times[setting].append(row)
for setting in ('0', '1'):
    flat = [v for row in times[setting] for v in row]
    print('%s=%s: median %.1f ms per step, min %.1f, max %.1f (%d steps); medians of the rounds: %s' % (
        SWITCH, setting, statistics.median(flat), min(flat), max(flat), len(flat),
        ', '.join('%.1f' % statistics.median(row) for row in times[setting])))
