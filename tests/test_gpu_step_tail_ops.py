"""
The end of the training step, one short op list at a time: every case of tests/step_tail_cases.py (GHN3_OP_SUMSQ, the four AdamW
kinds, GHN3_OP_WIRE_PACK, GHN3_OP_RANK_REDUCE, GHN3_OP_TRANSPOSE32, GHN3_OP_GRAPH_PROLOGUE, GHN3_OP_MEMSET0) runs through `ctx.run`
on device copies of its buffers and is held against the case's independent image.

  * Every byte outside a case's loose regions equals the image: slack in front of and behind every range, gaps between
    descriptors, padding, inputs -- and every result that is exact by design: bf16 moments and parameters of the bf16-state
    kinds (the second restatement of the rule), wire codes, rank-order sums, transposes, the graph prologue, memset.
  * fp32 AdamW results and sums: per 1024-element span (sums: per entry) within max(8 x float32 floor, 1e-6), never above 2e-5.
  * NaNs stay NaNs with their sign (wire) / come out (rank reduce); a non-finite gradient norm leaves everything untouched.
  * A second run from the same state gives equal bits, every buffer compared whole (no case here uses float atomics).
  * What the host functions refuse (misaligned buffers of the cast forms, step / seed outside the op's float fields, a bad
    skipped range or slot table of GHN3_OP_SUMSQ, n_pad < n) raises and writes nothing.
  * AdamW routes: aligned, all four buffers 4 bytes off, exp_avg alone, the gradient alone -- equal bits on the same data.
  * AdamW over a descriptor table: parameters and moments bit-equal to the flat op over the same buffers; every 16-bit copy
    equal to the cast of the run's own updated parameters by the case module's cast reference AND to what a fresh
    GHN3_OP_CAST16 with the same table writes, whole destination buffers compared (padding zeros, gaps, sentinels).
  * bf16 state: one launch, two partitions into three launches and the route with exp_avg 2 bytes off give equal bits; the
    flat form over the source range of a descriptor table agrees with the table form on the table's elements; seed and step
    change the stored moments and do not commute; p equals the fp32-state op's bits from the widened state.
  * GHN3_ADAMW_NT=0 in a fresh child process: the same digests for all four kinds.
  * Six looping cases (a lane takes a second trip through its grid-stride loop, a tail follows): adamw and adamw_s16 at
    n = 16384 * 1024 + 1027, sumsq at 4096 * 1024 + 1029 and with more than 4032 * 1024 floats above a skipped range,
    wire_pack at 8192 * 2048 + 2051 (both directions), rank_reduce at per = 8192 * 1024 + 1003, W = 2.

A flat index at or above 2^32 (bf16 state) needs an 8 GB state buffer and stays untested.

Every check prints a `MEASURED family case tensor ratio floor bound` line under pytest -s.

Measured on an MI355X (154 tests, 11 s, of which the six looping cases 5.4 s and the child process 2.7 s; 163 whole-image and
copy comparisons with equal bits; per family and tensor the case with the largest ratio / bound):

  family    tensor ratio    floor    bound    ratio / floor  case
  adamw     p      1.0e-07  1.1e-07  1.0e-06  0.95           adamw-n14000-ss0
  adamw     m      1.2e-08  5.1e-08  1.0e-06  0.24           adamw-n14000-lr0-f0neg
  adamw     v      9.1e-08  9.1e-08  1.0e-06  1.00           adamw-range-off1001
  cast      p      6.9e-08  6.9e-08  1.0e-06  1.00           cast-tight-130x64
  cast      m      1.6e-08  4.1e-08  1.0e-06  0.38           cast-ragged-ld136
  cast      v      9.1e-08  9.1e-08  1.0e-06  1.00           cast-w2-f16-bf16T
  sumsq     sumsq  1.1e-07  1.1e-07  1.0e-06  1.00           sumsq-skip-mid-e4
  reduce    out    5.5e-07  5.5e-07  4.4e-06  1.00           reduce-W8-per3-mis

Every ratio is at or below the float32 floor of its own span; no bound is widened.  s16, cast-s16, wire, reduce (bf16 outputs
and the rank-order column), transpose, prologue and memset have no float tensor: they are exact.  Looping cases: adamw-loop p
1.0e-07 / m 9.0e-09 / v 8.8e-08, sumsq-loop-plain 0 (floor 7.7e-08), sumsq-loop-skip 8.1e-08 (floor 3.3e-07), the others equal bits.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    for p_ in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
        if p_ not in sys.path:
            sys.path.insert(0, p_)

import torch  # noqa: E402

import step_tail_cases as S  # noqa: E402
from ghn3_amd import _lib as L  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return L.context(0)


def run_gpu(ctx, case, ops=None):
    dev = [torch.from_numpy(b).cuda() for b in S.host_bytes(case)]
    assert all(t.data_ptr() % 16 == 0 for t in dev)
    ptrs = np.asarray([t.data_ptr() + case.shift.get(k, 0) for k, t in enumerate(dev)], dtype=np.uint64)
    ctx.run(case.ops if ops is None else ops, case.problems, ptrs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev]


def same_bytes(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def check_copies(case, got):
    b = case.meta.bufs
    want = S.copy_image(case, S.typed(case, got, b[0]))
    for k, what in ((b[5], 'fused copies'), (b[6], 'fresh GHN3_OP_CAST16')):
        d = np.nonzero(S.typed(case, got, k) != want)[0]
        assert d.size == 0, (case.name, what, '%d codes differ from the cast of the updated parameters, first at %d' % (d.size, d[0]))
    assert np.array_equal(got[b[5]], got[b[6]])
    print('MEASURED %s %s copies equal bits' % (case.family, case.name))


def check_case(ctx, case, rerun=None):
    got = run_gpu(ctx, case)
    bad = S.mismatches(case, got)
    assert not bad, (case.name, 'differs from the image outside the loose regions (buffer, count, first element, got, want)', bad)
    print('MEASURED %s %s image equal bits' % (case.family, case.name))
    for name, v, fl, bd, ok in S.measure(case, got):
        assert bd <= S.FWD_CAP
        assert ok, (case.name, name, v, fl, bd)
    if case.family.startswith('cast') and not case.meta.skipped:
        check_copies(case, got)
    if case.rerun if rerun is None else rerun:
        assert same_bytes(got, run_gpu(ctx, case)), (case.name, 'two runs differ')
    return got


def region(case, got, k, a, n):
    return S.typed(case, got, k)[a:a + n]


# ---- fp32 state -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.cases('adamw'), ids=lambda c: c.name)
def test_adamw(ctx, case):
    check_case(ctx, case)


def test_adamw_routes_give_equal_bits(ctx):
    res = {}
    for nm in S.SAME_DATA:
        c = S.case_named(nm)
        got = run_gpu(ctx, c)
        res[nm] = [region(c, got, k, c.meta.starts[k], c.meta.n).view(np.uint32) for k in (0, 2, 3)]
    for nm in S.SAME_DATA[1:]:
        for a, b, t in zip(res[S.SAME_DATA[0]], res[nm], 'pmv'):
            assert np.array_equal(a, b), (nm, t, int((a != b).sum()), 'elements differ from the aligned route')


@pytest.mark.parametrize('case', S.cases('cast'), ids=lambda c: c.name)
def test_adamw_cast16(ctx, case):
    got = check_case(ctx, case)
    # the flat op over the whole source range, same buffers: equal bits on the descriptors' elements
    m = case.meta
    twin = run_gpu(ctx, case, S.flat_twin(case))
    for k, t in zip(m.bufs[:4], 'pgmv'):
        a, b = S.typed(case, got, k)[m.lo0 + m.el].view(np.uint32), S.typed(case, twin, k)[m.lo0 + m.el].view(np.uint32)
        assert np.array_equal(a, b), (case.name, t, int((a != b).sum()), 'elements differ from GHN3_OP_ADAMW')


# ---- bf16 state -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.cases('s16'), ids=lambda c: c.name)
def test_adamw_s16(ctx, case):
    got = check_case(ctx, case)
    m = case.meta
    if S.clip_of(m.cfg, np.float32) is None:
        return
    # p: the fp32-state op from the widened state gives the same bits
    twin = S.adamw_case('twin', m.n, m.cfg, data=(m.arrs[0], m.arrs[1], S.widen(m.mb), S.widen(m.vb)))
    tw = run_gpu(ctx, twin)
    a, b = region(case, got, m.bufs[0], m.lo, m.n).view(np.uint32), region(twin, tw, 0, 0, m.n).view(np.uint32)
    assert np.array_equal(a, b), (case.name, int((a != b).sum()), 'parameters differ from the fp32-state op on the widened state')


def test_adamw_s16_partitions_and_routes_give_equal_bits(ctx):
    res = {}
    for nm in S.S16_SAME:
        c = S.case_named(nm)
        got = run_gpu(ctx, c)
        m = c.meta
        res[nm] = [region(c, got, m.bufs[0], m.lo, m.n).view(np.uint32), region(c, got, m.bufs[2], m.lo + m.m_shift, m.n),
                   region(c, got, m.bufs[3], m.lo, m.n)]
    for nm in S.S16_SAME[1:]:
        for a, b, t in zip(res[S.S16_SAME[0]], res[nm], 'pmv'):
            assert np.array_equal(a, b), (nm, t, int((a != b).sum()))


def test_adamw_s16_seed_and_step_change_the_stored_moments(ctx):
    """(more than 90 % is impossible for the stored codes -- tests/test_step_tail_cases_cpu.py; the rounding bits are checked
    there, and every code here is equal to the restatement's)"""
    def moments(nm):
        c = S.case_named(nm)
        got = run_gpu(ctx, c)
        assert not S.mismatches(c, got)
        return [region(c, got, c.meta.bufs[k], 0, c.meta.n) for k in (2, 3)]
    one, six, a, b = moments('s16-one'), moments('s16-seed6'), moments('s16-step5-seed1'), moments('s16-step1-seed5')
    for k in (0, 1):
        assert (one[k] != six[k]).mean() > 0.25 and (a[k] != b[k]).mean() > 0.25


@pytest.mark.parametrize('case', S.cases('cast-s16'), ids=lambda c: c.name)
def test_adamw_s16_cast16(ctx, case):
    """also pins the flat index r2 offset / 2 + src_off + row * ld_src + column: the flat form over the same elements agrees"""
    got = check_case(ctx, case)
    m = case.meta
    twin = run_gpu(ctx, case, S.flat_twin(case))
    for k, t in zip(m.bufs[:4], 'pgmv'):
        a, b = S.typed(case, got, k)[m.lo0 + m.el], S.typed(case, twin, k)[m.lo0 + m.el]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (case.name, t, 'elements differ from GHN3_OP_ADAMW_S16')


# ---- the cache policy ---------------------------------------------------------------------------------------------------------------
NT_CASES = ('adamw-aligned', 's16-one', 'cast-ragged-ld136', 'cs16-ragged-ld136')


def digests(ctx):
    out = {}
    for nm in NT_CASES:
        c = S.case_named(nm)
        h = hashlib.sha256()
        for b in run_gpu(ctx, c):
            h.update(b.tobytes())
        out[nm] = h.hexdigest()
    return out


def test_the_cache_policy_changes_no_bit(ctx):
    """GHN3_ADAMW_NT=0 (read once per process) in a fresh child: p, m, v and the copies of all four kinds have the digests of
    this process, which runs the non-temporal default"""
    assert os.environ.get('GHN3_ADAMW_NT', '1') != '0'
    here = digests(ctx)
    run = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GHN3_ADAMW_NT='0'), capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    there = json.loads(run.stdout.strip().splitlines()[-1])
    assert there['nt'] == '0' and there['digests'] == here


# ---- sums, exchange, utilities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.cases('sumsq'), ids=lambda c: c.name)
def test_sumsq_ranges_and_slot_tables(ctx, case):
    check_case(ctx, case)


@pytest.mark.parametrize('case', S.cases('wire'), ids=lambda c: c.name)
def test_wire_pack(ctx, case):
    if case.refused:
        with pytest.raises(L.Ghn3Error, match='padded length'):
            run_gpu(ctx, case)
        return
    check_case(ctx, case)


@pytest.mark.parametrize('case', S.cases('reduce'), ids=lambda c: c.name)
def test_rank_reduce(ctx, case):
    check_case(ctx, case)


@pytest.mark.parametrize('case', S.cases('transpose'), ids=lambda c: c.name)
def test_transpose32(ctx, case):
    check_case(ctx, case)


@pytest.mark.parametrize('case', S.cases('prologue'), ids=lambda c: c.name)
def test_graph_prologue(ctx, case):
    check_case(ctx, case)


@pytest.mark.parametrize('case', S.cases('memset'), ids=lambda c: c.name)
def test_memset0(ctx, case):
    check_case(ctx, case)


# ---- what the host functions refuse ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [r[0] for r in S.refusals()])
def test_refused_arguments_write_nothing(ctx, name):
    _, case, ops, what = next(r for r in S.refusals() if r[0] == name)
    dev = [torch.from_numpy(b).cuda() for b in S.host_bytes(case)]
    ptrs = np.asarray([t.data_ptr() + case.shift.get(k, 0) for k, t in enumerate(dev)], dtype=np.uint64)
    with pytest.raises(L.Ghn3Error, match=what):
        ctx.run(ops, case.problems, ptrs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert same_bytes([t.cpu().numpy() for t in dev], S.host_bytes(case)), (name, 'a refused op wrote')


# ---- a second trip through the grid-stride loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(S.BIG))
def test_looping_sizes(ctx, name):
    case = S.BIG[name]()                                   # (built here: nothing large exists at collection time)
    check_case(ctx, case, rerun=name.startswith('sumsq'))


if __name__ == '__main__':
    print(json.dumps({'nt': os.environ.get('GHN3_ADAMW_NT'), 'digests': digests(L.context(0))}))
