"""
The 16-bit GEMM pipeline, one short op list at a time: every case of tests/gemm_pipeline_cases.py (GHN3_OP_CAST16 feeding
GHN3_GEMM_OP16 problems with scaled operands, `lim` tables, GHN3_GEMM_SUMSQ slot tables and GHN3_OP_SUMSQ; the fp32 kernels'
b_gather / a_q / bias_q / split-K fields; the cast variants) runs through `ctx.run` on device copies of its buffers and is
compared with the case's independent float64 reference (operands rounded on the CPU as the cast kernel rounds them).

  * 16-bit copies: bit-equal to the reference, zero padding included.
  * Float results: the error per 32 x 32 output tile and per row (util_parity.slice_errors on a blocked view; slot sums and
    GHN3_OP_SUMSQ results per entry) is at most max(8 x the case's float32 floor, 1e-6) and never above 2e-5.  With lim_kind 1
    only the columns below each row's own extent are compared.
  * Untouched memory: every byte outside the places a case names keeps its bits -- padding columns and slack of C, rows the row
    map of C skips, column tiles beyond a row tile's extent (lim_kind 1), the span [round8(rows), round64(rows)) of a TIGHT
    transposed copy, part slots of no row tile, slots of tile ids that name no tile, the other plane's buffers, all inputs.
  * Reruns: a second run gives the same bits for every result without split-K and without atomic column sums, the
    GHN3_GEMM_SUMSQ slots and the COLSUM_PARTS slots included.
  * K = 1: one product per output -- C is bit-equal to the reference, subnormal f16 copies included.
  * GHN3_GEMM_SUMSQ: besides the per-tile sums, the sum of all written slots equals the float64 sum of squares of the fp32
    values the same run stored in C.

Every check prints a `MEASURED family case tensor ratio floor bound` line under pytest -s.

Measured on an MI355X (67 cases, 3 s; every sixteen-bit copy with equal bits; per family and tensor the case with the largest
ratio / bound, and the largest ratio / floor of the family):

  family   tensor             ratio    floor    bound    ratio / floor   case
  scaled   C                  1.3e-07  9.1e-08  1.0e-06  1.41            scaled-t24-bf16-zero-K200 (the 18 cases with normal copies)
  scaled   C (subnormal f16)  1.9e-05  2.3e-08  2.0e-05  834             scaled-t25-f16-1e4-K456 (five cases: 147 .. 834, below)
  lim      C                  1.4e-07  1.2e-07  1.0e-06  1.26            lim2-t28-bf16-ks1
  sqgemm   C                  2.2e-07  1.1e-07  1.0e-06  2.00            sq-t29-xcd-groups (K = 1024)
  sqgemm   sq (per tile)      1.2e-07  1.1e-07  1.0e-06  1.05            sq-t30-cmap-cap
  sqgemm   slots - stored C   1.0e-08  7.9e-08  1.0e-06  0.13            sq-t29-ragged
  sqgemm   sumsq (op, range)  7.5e-08  0        1.0e-06  -               sq-t30-ragged
  sumsq    sumsq              2.2e-07  0        1.0e-06  -               sumsq-scratch-n70001
  f32      C                  3.5e-07  2.0e-07  1.6e-06  1.71            f32-ksplit2-t128
  cast     parts              1.3e-07  1.1e-07  1.0e-06  1.22            cast-parts-bf16-2desc
  cast     colsum             2.1e-07  1.5e-07  1.2e-06  1.33            cast-scaled-colsum-bf16

The f16 cases with a pow2 / below-pow2 amax on tile codes 20, 24, 25, 29 and 30 stay at or below their floors (0.6 .. 0.9 x).
The factor 8 is widened for five cases with K > 1 (and, without effect, two exact K = 1 cases: equal bits), all f16 with a scale <= 1 (amax 0, 1e-35, 1e4) on 1e-7 sources, whose operand
copies are SUBNORMAL: scaled-t20-f16-zero 1.08e-5, -t24-f16-1e-35 1.03e-5, -t25-f16-1e4 1.95e-5, -t29-f16-zero 1.01e-5,
-t30-f16-1e-35 1.09e-5 per tile (147 .. 834 x their floors), the same on every kernel.  A single product is exact; sums of
two and more products of one MFMA lie on a grid of 2^-39 at results of ~1e-7, and the same data scaled by 2^14 or 2^32, or in
bf16, is back at 1e-7: the matrix cores align the products at the nominal exponent of a subnormal, 2^-14, and lose the leading
zeros of its ten fraction bits.  Bound for these: 8 x 2^10 x floor, cut by the 2e-5 cap (gemm_pipeline_cases.SUBNORMAL_F16_FACTOR).
"""
import numpy as np
import pytest
import torch

import gemm_pipeline_cases as G
from ghn3_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return L.context(0)


def run_gpu(ctx, case):
    dev = [torch.from_numpy(b).cuda() for b in G.host_bytes(case)]
    ptrs = np.asarray([t.data_ptr() for t in dev], dtype=np.uint64)
    assert all(int(p) % 16 == 0 for p in ptrs)
    ctx.run(case.ops, case.problems, ptrs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_case(ctx, case):
    gpu = run_gpu(ctx, case)
    got, raw, ref = G.extract(case, gpu), G.extract_raw(case, gpu), G.reference(case)
    # what the ops must not touch
    w, before = G.written(case), G.host_bytes(case)
    for k, b in enumerate(case.bufs):
        keep = np.repeat(~w[k], b.dtype.itemsize)
        bad = np.nonzero(gpu[k][keep] != before[k][keep])[0]
        assert bad.size == 0, (case.name, 'buffer %d: %d bytes changed outside the written region' % (k, bad.size))
    for o in case.outs:
        g, r = got[o.name], ref[o.name]
        if o.kind == 'bits':
            diff = np.argwhere(g != r)
            assert diff.size == 0, (case.name, o.name, '%d codes differ, first at %s: %#x != %#x' % (
                len(diff), tuple(diff[0]), int(g[tuple(diff[0])]), int(r[tuple(diff[0])])))
            print('MEASURED %s %s %s equal bits' % (case.family, case.name, o.name))
            continue
        g = G.masked(case, o.name, g, r)
        v, where = G.measure(case, o.name, g, r)
        fl, bd = G.floors(case)[o.name], G.bound(case, o.name)
        print('MEASURED %s %s %s ratio %.3e floor %.3e bound %.3e' % (case.family, case.name, o.name, v, fl, bd))
        assert bd <= G.FWD_CAP
        assert np.isfinite(g).all(), (case.name, o.name, 'NaN or infinity where the op must write')
        assert v <= bd, (case.name, o.name, v, bd, where)
    # a second run: equal bits wherever the design promises them
    again = G.extract_raw(case, run_gpu(ctx, case))
    for o in case.outs:
        if o.rerun:
            assert same_bits(raw[o.name], again[o.name]), (case.name, o.name, 'two runs differ')
    return gpu, got, raw


@pytest.mark.parametrize('case', G.cases('scaled'), ids=lambda c: c.name)
def test_scaled_operands(ctx, case):
    gpu, got, raw = check_case(ctx, case)
    if case.meta.K == 1:
        # one product per output, exact in float32 whatever the copies hold -- subnormal f16 codes included
        assert same_bits(got['C'], G.reference(case)['C']), (case.name, 'a single product differs from the exact one')


@pytest.mark.parametrize('case', G.cases('lim'), ids=lambda c: c.name)
def test_lim_tables(ctx, case):
    check_case(ctx, case)


@pytest.mark.parametrize('case', G.cases('sqgemm'), ids=lambda c: c.name)
def test_gemm_sumsq(ctx, case):
    gpu, got, raw = check_case(ctx, case)
    m = case.meta
    for tag in ('', '1'):
        if 'sq' + tag not in raw:
            continue
        o = G.out_of(case, 'C' + tag)
        stored = G._typed(case, gpu, o.buf)[o.idx].astype(np.float64)
        want = float((stored * stored).sum())
        slots = raw['sq' + tag].astype(np.float64)
        assert np.isfinite(slots).all(), (case.name, 'a slot of a tile was not written')
        err = abs(float(slots.sum()) - want) / want
        bd = max(G.bound(case, 'sq' + tag), G.MIN_BOUND)
        print('MEASURED %s %s slots%s-vs-stored-C ratio %.3e floor %.3e bound %.3e' % (case.family, case.name, tag, err,
                                                                                     G.floors(case)['sq' + tag], bd))
        assert err <= bd, (case.name, tag, err, bd)
    table = G._typed(case, gpu, m.b_slots)
    unnamed = np.ones(table.size, bool)
    unnamed[G.out_of(case, 'sq').idx.reshape(-1)] = False
    assert unnamed[:8 * m.n_ids].any() and np.isnan(table[unnamed]).all(), 'slots of ids that name no tile keep the sentinel'


@pytest.mark.parametrize('case', G.cases('sumsq'), ids=lambda c: c.name)
def test_sumsq_op(ctx, case):
    check_case(ctx, case)


@pytest.mark.parametrize('case', G.cases('f32'), ids=lambda c: c.name)
def test_fp32_kernel_fields(ctx, case):
    check_case(ctx, case)


@pytest.mark.parametrize('case', G.cases('cast'), ids=lambda c: c.name)
def test_cast_variants(ctx, case):
    gpu, got, raw = check_case(ctx, case)
    if 'cast:paths' in case.regimes:
        assert same_bits(got['d0.st'], got['d1.st']) and same_bits(got['d0.st'], got['d2.st']), 'the two straight paths differ'
