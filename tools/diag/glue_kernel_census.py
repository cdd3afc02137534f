"""Per-step launch counts of the glue kernels in a rocprofv3 kernel trace (rocpd sqlite) of tools/diag/stock_layer_census.py:
all kernels, ATen copies, ATen adds, ATen concatenations, and the project's own join kernels.

    python3 tools/diag/glue_kernel_census.py <results.db> <steps> [label]"""
import collections
import sqlite3
import sys

CLASSES = (('ATen cat', ('CatArrayBatchedCopy',)),
           ('ATen add', ('CUDAFunctor_add', 'AddFunctor', 'add_kernel')),
           ('ATen copy', ('direct_copy_kernel', 'copy_kernel', 'copy_device_to_device')),
           ('runtime copyBuffer', ('__amd_rocclr_copyBuffer',)),
           ('tnet_join', ('tnet_join_', 'tnet_posenc_')))


def main():
    db, steps = sys.argv[1], int(sys.argv[2])
    label = sys.argv[3] if len(sys.argv) > 3 else db
    cur = sqlite3.connect(db).cursor()
    n, us = collections.Counter(), collections.Counter()
    total = 0
    for name, calls, dur in cur.execute('select name,total_calls,total_duration from top_kernels'):
        total += calls
        for cls, keys in CLASSES:
            if any(k in name for k in keys):
                n[cls] += calls
                us[cls] += dur
                break
    print('%s: %d kernels in %d steps (+ setup), %.0f per step' % (label, total, steps, total / steps))
    for cls, _ in CLASSES:
        print('    %-20s %8.1f launches per step  %8.1f us per step' % (cls, n[cls] / steps, us[cls] / steps))


if __name__ == '__main__':
    main()
