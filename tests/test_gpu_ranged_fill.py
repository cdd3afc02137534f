"""
ghn3_run turns a run of consecutive GHN3_OP_MEMSET0 ops bound for one stream into ranged-fill launches (fill_ranges_kernel,
elementwise.hip; the range table lives with the run's cached device tables).  Programs of MEMSET0 ops go through `ctx.run` on
device buffers pre-filled with 0xab and every byte is held against a numpy image built from the documented meaning of the op
alone -- (buffer, offset, byte count); an absent buffer or a zero count does nothing -- so the bytes on both sides of every
range are guards.
"""

import numpy as np
import pytest
import torch

from ghn3_amd import _lib as L

pytestmark = pytest.mark.gpu

FILL = 0xab


@pytest.fixture(scope='module')
def ctx():
    return L.context(0)


def _ops(items):
    """items: ('fill', buf or None, offset, bytes[, side]) | ('nop',) | ('add', buf, dst offset, src offset, floats)."""
    ops = np.zeros(len(items), dtype=L.OP_DT)
    ops['r']['buf'][:] = -1
    for o, it in zip(ops, items):
        if it[0] == 'fill':
            o['kind'] = L.OP_MEMSET0
            if it[1] is not None:
                o['r'][0]['buf'], o['r'][0]['off'] = it[1], it[2]
            o['i'][0] = it[3]
            o['flags'] = L.OPFLAG_SIDE if (len(it) > 4 and it[4]) else 0
        elif it[0] == 'nop':
            o['kind'] = L.OP_NOP
        else:
            o['kind'] = L.OP_ADD
            o['r'][0]['buf'], o['r'][0]['off'] = it[1], it[2]
            o['r'][1]['buf'], o['r'][1]['off'] = it[1], it[3]
            o['i'][0] = it[4]
    return ops


def _image(items, bufs):
    """What the documented ops leave in host copies of the buffers, in program order."""
    img = [b.copy() for b in bufs]
    for it in items:
        if it[0] == 'fill' and it[1] is not None and it[3] > 0:
            img[it[1]][it[2]:it[2] + it[3]] = 0
        elif it[0] == 'add':
            d = img[it[1]][it[2]:it[2] + 4 * it[4]].view(np.float32)
            d += img[it[1]][it[3]:it[3] + 4 * it[4]].view(np.float32)
    return img


def _check(ctx, items, bufs, runs=1):
    ops = _ops(items)
    dev = [torch.from_numpy(b.copy()).cuda() for b in bufs]
    ptrs = np.asarray([d.data_ptr() for d in dev], dtype=np.uint64)
    stream = torch.cuda.current_stream().cuda_stream
    want = _image(items, bufs)
    for n in range(runs):
        if n:
            for d, b in zip(dev, bufs):                  # (same pointers: the second run finds its tables on the device)
                d.copy_(torch.from_numpy(b))
        hits = ctx.cache_stats()[0]
        ctx.run(ops, np.zeros(0, dtype=L.PROBLEM_DT), ptrs, stream)
        torch.cuda.synchronize()
        if n:
            assert ctx.cache_stats()[0] == hits + 1
        for k, (d, w) in enumerate(zip(dev, want)):
            got = d.cpu().numpy()
            bad = np.nonzero(got != w)[0]
            assert bad.size == 0, 'run %d buffer %d: %d bytes differ, first at %d' % (n, k, bad.size, int(bad[0]))


def _buf(n):
    return np.full(n, FILL, dtype=np.uint8)


ODD = [(16, 1), (35, 3), (64, 5), (101, 1026), (3000, 7)]


def test_odd_offsets_and_byte_counts_with_empty_ops_inside_the_run(ctx):
    items = [('fill', 0, off, n) for off, n in ODD]
    items[2:2] = [('fill', 0, 2000, 0), ('fill', None, 0, 8)]    # a zero count and an absent buffer in the middle
    _check(ctx, items, [_buf(4096)])


def test_ranges_longer_than_a_work_block_from_unaligned_addresses(ctx):
    # (a work block is 64 KB of the 16-byte grid: first and last blocks partial, blocks inside the range on the unchecked path)
    items = [('fill', 0, 5, 2 * 65536 + 11), ('fill', 0, 300001, 65535), ('fill', 1, 15, 65536 + 2), ('fill', 1, 200000, 16),
             ('fill', 1, 200033, 15), ('fill', 1, 262144, 65536)]
    _check(ctx, items, [_buf(1 << 19), _buf(1 << 19)])


def test_ranges_that_touch_and_ranges_that_overlap(ctx):
    items = [('fill', 0, 1200, 300), ('fill', 0, 100, 50), ('fill', 0, 150, 70), ('fill', 0, 1000, 300), ('fill', 0, 1100, 20)]
    _check(ctx, items, [_buf(4096)])


def test_a_run_longer_than_the_range_table_is_split_not_truncated(ctx):
    items = [('fill', k % 2, 64 + 97 * k, 1 + (7 * k) % 61) for k in range(300)]
    _check(ctx, items, [_buf(64 + 97 * 300 + 64)] * 2)


def test_runs_broken_by_a_nop_and_by_a_kernel_keep_memory_order(ctx):
    b = _buf(8192)
    b[1024:2048].view(np.float32)[:] = 1.5               # x: the kernel's destination
    b[4096:5120].view(np.float32)[:] = np.arange(256, dtype=np.float32) + 1.0      # y: its source
    items = [('fill', 0, 1024, 512), ('fill', 0, 3000, 9),               # a fill in front of the kernel: x[:128] = 0 + y
             ('nop',),
             ('fill', 0, 3100, 3), ('fill', 0, 3200, 33),
             ('add', 0, 1024, 4096, 256),                                 # x += y
             ('fill', 0, 1536, 512), ('fill', 0, 6001, 31)]               # a fill behind it still zeroes x[128:]
    want = _image(items, [b])[0][1024:2048].view(np.float32)
    assert np.array_equal(want[:128], np.arange(128) + 1.0) and not want[128:].any()
    _check(ctx, items, [b])


def test_main_and_side_fills_alternating(ctx):
    single = [('fill', 0, 100 + 300 * k, 1 + 37 * k, k % 2 == 1) for k in range(6)]        # runs of one op each
    pairs = [('fill', 1, 64 + 500 * k, 3 + 101 * (k % 3), (k // 2) % 2 == 1) for k in range(8)]    # runs of two per stream
    _check(ctx, single + pairs, [_buf(4096), _buf(8192)])


def test_a_replayed_program_takes_its_cached_table(ctx):
    items = [('fill', 0, off, n) for off, n in ODD] + [('fill', 1, 7, 70001)]
    _check(ctx, items, [_buf(4096), _buf(1 << 17)], runs=3)


def test_one_64_mb_range(ctx):
    n, guard = 64 << 20, 4096
    dev = torch.full((n + 2 * guard,), FILL, dtype=torch.uint8, device='cuda')
    small = torch.full((256,), FILL, dtype=torch.uint8, device='cuda')
    ops = _ops([('fill', 0, guard + 3, n), ('fill', 1, 9, 100)])
    ptrs = np.asarray([dev.data_ptr(), small.data_ptr()], dtype=np.uint64)
    ctx.run(ops, np.zeros(0, dtype=L.PROBLEM_DT), ptrs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((dev[guard + 3:guard + 3 + n] == 0).all())
    assert bool((dev[:guard + 3] == FILL).all()) and bool((dev[guard + 3 + n:] == FILL).all())
    s = small.cpu().numpy()
    assert not s[9:109].any() and (s[:9] == FILL).all() and (s[109:] == FILL).all()
