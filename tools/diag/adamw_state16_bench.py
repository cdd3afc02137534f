"""Micro-benchmark (GPU box): GHN3_OP_SUMSQ + GHN3_OP_ADAMW over ghn3xlm16's 654 M parameters with fp32 moments against
GHN3_OP_SUMSQ + GHN3_OP_ADAMW_S16 with bf16 moments (stochastic rounding), timed with HIP events.  The two settings alternate
inside one process, `--rounds` times, so that a drift of the box shows as spread within a setting and not as a difference
between them.  Bytes per parameter: SUMSQ reads 4; the update moves 28 (fp32 state) or 20 (bf16 state).

    python tools/diag/adamw_state16_bench.py [--state fp32|bf16|both] [--rounds 5] [--reps 10] [--n 654365312]
"""
import argparse
import numpy as np
import torch
import _paths  # noqa: F401  (repository root, tests/, tests/golden/ on sys.path)
from ghn3_amd import _lib as L
from ghn3_amd.optim import _dbits

ap = argparse.ArgumentParser()
ap.add_argument('--state', choices=('fp32', 'bf16', 'both'), default='both')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--n', type=int, default=654365312, help='parameters (default: the flat buffer of ghn3xlm16)')
args = ap.parse_args()
n, dev = args.n, 'cuda'
p = torch.randn(n, device=dev)
g = torch.randn(n, device=dev) * 1e-3
moments = {'fp32': [torch.zeros(n, device=dev) for _ in range(2)],
           'bf16': [torch.zeros(n, dtype=torch.bfloat16, device=dev) for _ in range(2)]}
scal = torch.zeros(64, device=dev)
parts = torch.zeros(1 << 16, device=dev)
ctx = L.context(0)
st = torch.cuda.current_stream().cuda_stream
none = np.zeros(0, dtype=L.PROBLEM_DT)
BYTES = {'fp32': 28, 'bf16': 20}


def run(state, with_sumsq, reps, step0):
    ops = np.zeros(3, dtype=L.OP_DT)
    ops['r']['buf'][:] = -1
    ops[0]['kind'] = L.OP_MEMSET0
    ops[0]['r']['buf'][0] = 4
    ops[0]['i'][0] = 4
    ops[1]['kind'] = L.OP_SUMSQ if with_sumsq else L.OP_NOP
    ops[1]['r']['buf'][:3] = (4, 1, 5)
    ops[1]['i'][0] = n
    ops[2]['kind'] = L.OP_ADAMW if state == 'fp32' else L.OP_ADAMW_S16
    ops[2]['r']['buf'][:5] = (0, 1, 2, 3, 4 if with_sumsq else -1)
    ops[2]['i'][0] = n
    ops[2]['f'][0] = 5.0 if with_sumsq else 0.0
    ops[2]['f'][1] = 1.0
    bufs = np.asarray([p.data_ptr(), g.data_ptr()] + [t.data_ptr() for t in moments[state]] +
                      [scal.data_ptr(), parts.data_ptr()], dtype=np.uint64)

    def once(t):
        for k, h in enumerate((1e-6, 0.9, 0.999, 1e-8, 1e-2, 1.0 - 0.9 ** t, 1.0 - 0.999 ** t)):
            ops[2]['i'][1 + k] = _dbits(h)
        ops[2]['f'][2] = float(t)                         # (step and seed of the bf16-state kind; unused by GHN3_OP_ADAMW)
        ctx.run(ops, none, bufs, st)
    for t in range(2):
        once(step0 + t)
    a, b = L.Event(), L.Event()
    a.record(st)
    for t in range(reps):
        once(step0 + 2 + t)
    b.record(st)
    torch.cuda.synchronize()
    return a.elapsed_ms(b) / reps


states = ('fp32', 'bf16') if args.state == 'both' else (args.state,)
times = {(s, w): [] for s in states for w in (True, False)}
for r in range(args.rounds):
    for s in states:
        for w in (True, False):
            times[(s, w)].append(run(s, w, args.reps, 1 + r * (args.reps + 2)))
for (s, w), ts in times.items():
    med = float(np.median(ts))
    nbytes = BYTES[s] + (4 if w else 0)
    print('%s state, %-13s median %.3f ms  min %.3f  max %.3f  (%.2f TB/s over %d B/param)  rounds: %s' % (
        s, 'sumsq + adamw' if w else 'adamw alone', med, min(ts), max(ts), nbytes * n / med / 1e9, nbytes,
        ' '.join('%.3f' % t for t in ts)))
if len(states) == 2:
    for w in (True, False):
        a, b = np.median(times[('fp32', w)]), np.median(times[('bf16', w)])
        print('%-13s bf16 state / fp32 state = %.3f   (byte counts: %.3f)' % (
            'sumsq + adamw' if w else 'adamw alone', b / a, (20 + (4 if w else 0)) / (28 + (4 if w else 0))))
