"""
The decoder tail -- the kernels between the decoder GEMMs and the predicted parameters (ghn3_amd/csrc/elementwise.hip:
GHN3_OP_TILE_FWD / _BWD, GHN3_OP_PARAM_NORM_FWD / _BWD / _FIN, GHN3_OP_RELU_FIX, GHN3_OP_ROWSET_COLSUM, GHN3_OP_ADD), one op
record (or the short chain of training) at a time: every case of tests/decoder_tail_cases.py runs through `ctx.run` on device
copies of its buffers and through the float64 interpreter (tests/program_interp.py) on host copies.

Bit-equal: the mode-0 tile forward (a single fp32 multiply), the zeros the tile backward writes outside the consumed box,
GHN3_OP_ADD, the ReLU of every element GHN3_OP_RELU_FIX does not recompute, and everything an op must not touch -- sentinels,
slack and guard floats, inputs, the amax slot when no descriptor of source buffer 0 runs, fp32 regions of descriptors that went
to 16 bits and 16-bit regions of those that did not; amax = norms[-1] * |g| on the 16-bit route; the deterministic reductions
(GHN3_OP_PARAM_NORM_FWD with first_seg, GHN3_OP_PARAM_NORM_FIN, GHN3_OP_ROWSET_COLSUM, the sq_parts of the tile forward) run
twice for equal bits.

Rounded results are compared per slice (util_parity.slice_errors: per o row and per 16-channel group of i for tile outputs and
source gradients, per output row and 64-column block for the row-set sums, per row and 1024-column block for RELU_FIX) or per
entry (per-segment norms, per-block sums of squares; dflat per segment).  Bound = 8 x the float32 floor of the case (the formula
in plain float32 against float64), at least 1e-6, never above the published 2e-5 (forward) / 2e-4 (gradient).

16-bit tile gradients: each decoded element lies within half a unit in the last place of the 16-bit format at the reference
value plus the fp32 bound x |reference| of reference x pow2_scale(bound); every element is finite and at most 4096 in magnitude;
and the float64 reference gradient of source buffer 0 stays below the a-priori bound -- the property the route rests on.

Modes 1 and 2 go through __expf / tanhf: measured at most 1.04 x the float32 floor of the plain formula (out, below), so no
tensor needed a factor of its own (their source gradients: 1.23 x, tileb-elem-both d1).  GHN3_OP_RELU_FIX compares |x| < tau strictly: two cases put every |x| exactly on tau (0.5,
tau_rel = 1: the rms is exact in float32 and in float64) and hand the kernel a NaN weight matrix.

Measured on an MI355X (every check prints a `MEASURED family case tensor ratio floor bound` line under pytest -s; per family and
tensor the case with the largest ratio / bound; `d1`: descriptor 1 of the case; 52 cases, 2.9 s, all within their bounds; no
factor widened).  h16: ratio = worst |decoded - reference x scale| / (half a 16-bit unit + fp32 bound x |reference x scale|).

  family   tensor         ratio    floor    bound    case
  tilef    out            6.1e-08  6.1e-08  1.0e-06  tilef-elem-blocks d1 (mode 1)
  tilef    sq             1.1e-07  1.1e-07  1.0e-06  tilef-row-mix
  tilef    bp             0.0e+00  0.0e+00  1.0e-06  (every case: equal bits)
  tileb    out            3.8e-08  3.8e-08  1.0e-06  tileb-elem-norm d1
  tileb    dsrc           3.6e-07  3.0e-07  2.4e-06  tileb-elem-both d1 (mode 1)
  tileb    sq             1.1e-07  1.1e-07  1.0e-06  tileb-elem-norm
  tileb    norms          9.2e-08  9.2e-08  1.0e-06  tileb-row-both
  tileb    loss           7.1e-08  7.1e-08  1.0e-06  tileb-row-norm
  tileb    ratio          8.5e-08  9.3e-08  1.0e-06  tileb-row-norm
  tileb    bound          0.0e+00  0.0e+00  1.0e-06  (every case: equal bits)
  tileb16  dsrc (fp32)    4.0e-07  4.0e-07  3.2e-06  tileb16-bf16-h2 d5
  tileb16  sq             1.1e-07  9.1e-08  1.0e-06  tileb16-bf16-h2
  tileb16  norms          1.0e-07  1.1e-07  1.0e-06  tileb16-f16-h2
  tileb16  loss           1.2e-07  1.2e-07  1.0e-06  tileb16-bf16-h2
  tileb16  ratio          8.7e-08  8.7e-08  1.0e-06  tileb16-f16-h2
  tileb16  bound          7.5e-08  7.5e-08  1.0e-06  tileb16-bf16-h2
  tileb16  h16            0.999    -        1        tileb16-bf16-h0 d1
  pnorm    norms          1.0e-07  0.0e+00  1.0e-06  pnorm-gap (the atomic form: the same)
  pnorm    loss           3.2e-07  1.1e-07  1.0e-06  pnorm-261seg (the atomic form: the same)
  pnorm    dflat          1.9e-07  9.2e-08  1.0e-06  pnorm-gap
  pfin     norms          1.2e-07  1.2e-07  1.0e-06  pfin-261
  pfin     ratio          1.3e-07  1.3e-07  1.0e-06  pfin-261
  pfin     loss, bound    0.0e+00  9.3e-08  1.0e-06  pfin-bparts
  rfix     X              3.1e-07  1.5e-07  1.2e-06  rfix-r70-c5-K252-tau0.005-map1-bias0
  rfix     X(candidates)  5.8e-07  1.5e-07  1.2e-06  rfix-r70-c5-K252-tau0.005-map1-bias0
  rset     out            7.2e-08  1.3e-07  1.0e-06  rset-bias0
  add      dst            equal bits
"""
import numpy as np
import pytest
import torch

import decoder_tail_cases as G
from ghn3_amd import _lib as L
from program_interp import Interp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return L.context(0)


def run_gpu(ctx, case):
    dev = [torch.from_numpy(b).cuda() for b in G.host_bytes(case)]
    ptrs = np.asarray([t.data_ptr() for t in dev], dtype=np.uint64)
    assert all(int(p) % 16 == 0 for p in ptrs)                  # (the regimes of the CPU test count on aligned allocations)
    ctx.run(case.ops, np.zeros(0, dtype=L.PROBLEM_DT), ptrs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check(case, name, got, ref):
    v, where = G.measure(case, name, got, ref)
    fl, bd = G.floors(case)[name], G.bound(case, name)
    print('MEASURED %s %s %s ratio %.3e floor %.3e bound %.3e' % (case.family, case.name, name, v, fl, bd))
    assert np.isfinite(np.asarray(got)).all(), (case.name, name, 'NaN or infinity in a region the op must write')
    assert v <= bd, (case.name, name, v, bd, where)


def both(ctx, case):
    gpu = run_gpu(ctx, case)
    ref = G.run_interp(case)
    return gpu, ref, G.extract(case, gpu), G.extract(case, ref)


def untouched(case, gpu, k, written=None):
    """buffer k keeps its bits (outside the float mask `written`)"""
    a, b = gpu[k].view(np.uint8), G.host_bytes(case)[k]
    if written is None:
        assert np.array_equal(a, b), (case.name, 'buffer %d changed' % k)
        return
    n = written.size
    keep = ~written
    assert np.array_equal(a[:4 * n].view(np.uint32)[keep], b[:4 * n].view(np.uint32)[keep]) and np.array_equal(a[4 * n:], b[4 * n:]), \
        (case.name, 'buffer %d changed where the op must not write' % k)


# ---- tile ops ---------------------------------------------------------------------------------------------------------------
def ulp16(v, bf16):
    e = np.floor(np.log2(np.maximum(np.abs(v), 1e-300)))
    return np.where(v == 0, 0.0, 2.0 ** (e - 7) if bf16 else np.maximum(2.0 ** (e - 10), 2.0 ** -24))


def tile_checks(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    hi = G.reference(case)
    written, written16 = G.tile_written(case)
    for k in range(len(case.bufs)):
        if k in written:
            untouched(case, gpu, k, written[k])
        else:
            untouched(case, gpu, k)                   # sources, tables, g, dflat, first
    if m.bf16 is not None:                            # 16-bit elements between the copies
        a16, b16 = gpu[G.B_DSRC].view(np.uint8).view(np.uint16), G.host_bytes(case)[G.B_DSRC].view(np.uint16)
        assert np.array_equal(a16[~written16], b16[~written16]), '16-bit elements outside the copies changed'
    top = 0.0
    for k, d in enumerate(m.descs):
        name = 'out.d%d' % k
        if name in g:
            if d.mode == 0:
                assert same_bits(g[name], r[name]), (case.name, name, 'mode 0 is a single fp32 multiply')
            else:
                check(case, name, g[name], r[name])
        name = 'dsrc.d%d' % k
        if name in g:
            check(case, name, g[name], r[name])
            box = np.zeros(d.R, bool)
            box[:d.E[0], :d.E[1], :d.E[2], :d.E[3]] = True
            assert same_bits(g[name][~box], np.zeros(int((~box).sum()), np.float32)), (case.name, name, 'exact zeros outside the consumed box')
            if d.buf == 0 and g[name].size:
                top = max(top, float(np.abs(g[name]).max()))
    for name in ('sq', 'bp', 'norms', 'loss', 'ratio', 'bound'):
        if name in g:
            check(case, name, g[name], r[name])
    if m.bwd:
        am = float(g['amax'][0])
        if m.bf16 is not None:
            assert same_bits(g['amax'], np.float32(g['bound'][0]) * np.float32(abs(np.float32(m.g))).reshape(1)), 'amax = norms[-1] * |g|'
        elif any(d.buf == 0 for d in m.descs):
            want = max(top, m.amax0)
            assert abs(am - want) <= 1e-6 * want, (am, want)
    return gpu, g, hi


@pytest.mark.parametrize('case', G.cases('tilef'), ids=lambda c: c.name)
def test_tile_fwd(ctx, case):
    gpu, g, hi = tile_checks(ctx, case)
    if case.meta.sq:
        again = G.extract(case, run_gpu(ctx, case))
        assert same_bits(g['sq'], again['sq']), 'sq_parts: two runs differ'


@pytest.mark.parametrize('case', G.cases('tileb'), ids=lambda c: c.name)
def test_tile_bwd(ctx, case):
    gpu, g, hi = tile_checks(ctx, case)
    if case.meta.fin:
        again = G.extract(case, run_gpu(ctx, case))
        for name in ('sq', 'norms', 'loss', 'ratio', 'bound'):
            assert same_bits(g[name], again[name]), (name, 'two runs differ')


@pytest.mark.parametrize('case', G.cases('tileb16'), ids=lambda c: c.name)
def test_tile_bwd_16bit(ctx, case):
    m = case.meta
    gpu, g, hi = tile_checks(ctx, case)
    bnd = float(g['amax'][0])
    hsc = Interp.pow2_scale(bnd)
    for k, d in enumerate(m.descs):
        exact = hi['dsrc.d%d' % k].astype(np.float64)
        if d.buf == 0:
            assert float(np.abs(exact).max()) <= bnd, (case.name, k, 'the a-priori bound does not hold')
        if d.h is None:
            continue
        got = Interp.from16(g['h16.d%d' % k].reshape(-1), bool(m.bf16)).reshape(d.R).astype(np.float64)
        assert np.isfinite(got).all() and float(np.abs(got).max()) <= 4096.0, (case.name, k)
        want = exact * hsc
        fp32 = G.bound(case, 'dsrc.d%d' % k)
        tol = 0.5 * ulp16(want, m.bf16) + fp32 * np.abs(want)
        err = np.abs(got - want)
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = float(np.nanmax(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))))
        print('MEASURED %s %s h16.d%d ratio %.3e floor %.3e bound %.3e' % (case.family, case.name, k, ratio, 0.0, 1.0))     # (error / tolerance)
        assert (err <= tol).all(), (case.name, k, ratio)
        box = np.zeros(d.R, bool)
        box[:d.E[0], :d.E[1], :d.E[2], :d.E[3]] = True
        assert (g['h16.d%d' % k][~box] == 0).all(), 'zero codes outside the consumed box'
    again = G.extract(case, run_gpu(ctx, case))
    for name in g:                                    # no atomics on this route: every result twice for equal bits
        assert same_bits(g[name], again[name]), (name, 'two runs differ')


# ---- norms ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.cases('pnorm'), ids=lambda c: c.name)
def test_param_norm(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    again = run_gpu(ctx, case)
    for name in r:
        check(case, name, np.where(np.isnan(r[name]), 0, g[name]), np.where(np.isnan(r[name]), 0, r[name]))
    for k in (0, 3, 5, 6):                           # the deterministic form and what follows from it: equal bits
        assert same_bits(gpu[k], again[k]), (case.name, 'buffer %d: two runs differ' % k)
    inside = np.zeros(case.bufs[6].size, bool)
    for s0, s1 in m.seg:
        inside[s0:s1] = True
    untouched(case, gpu, 6, inside)
    first_n = lambda size, n: np.arange(size) < n
    untouched(case, gpu, 3, first_n(case.bufs[3].size, m.n))
    untouched(case, gpu, 7, first_n(case.bufs[7].size, m.n))
    untouched(case, gpu, 0, first_n(4, 1))
    untouched(case, gpu, 8, first_n(4, 1))
    slots = np.zeros(case.bufs[5].size, bool)
    slots[:m.n_chunks + m.n] = True
    untouched(case, gpu, 5, slots)
    for k in (1, 2, 4):
        untouched(case, gpu, k)
    zero = np.asarray([not case.bufs[1][s0:s1].any() for s0, s1 in m.seg])
    assert (g['norms'][zero] == 0).all() and (g['norms_atomic'][zero] == 0).all()
    for (s0, s1), z in zip(m.seg, zero):
        if z:
            assert same_bits(g['dflat'][s0:s1], np.zeros(s1 - s0, np.float32)), 'a zero segment: gradient 0, not NaN'


@pytest.mark.parametrize('case', G.cases('pfin'), ids=lambda c: c.name)
def test_param_norm_fin(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    again = G.extract(case, run_gpu(ctx, case))
    for name in r:
        check(case, name, g[name], r[name])
        assert same_bits(g[name], again[name]), (name, 'two runs differ')
    if m.bp:
        assert float(g['bound'][0]) == float(g['ratio'].max())
    w = np.zeros(case.bufs[1].size, bool)
    w[G.NORMS_AT:G.NORMS_AT + m.n] = True
    w[G.NORMS_AT - 1] = m.bp
    untouched(case, gpu, 1, w)
    untouched(case, gpu, 0, np.arange(4) < 1)
    untouched(case, gpu, 5, (np.arange(case.bufs[5].size) < m.n) & bool(m.bp))
    for k in (2, 3, 4):
        untouched(case, gpu, k)


# ---- RELU_FIX, ROWSET_COLSUM, ADD -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.cases('rfix'), ids=lambda c: c.name)
def test_relu_fix(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    x0 = case.bufs[0][:m.rows * m.ld].reshape(m.rows, m.ld)[:, :m.cols]
    cand = G.rfix_candidates(case)
    assert same_bits(g['X'][~cand], np.maximum(x0, 0)[~cand]), 'ReLU of the elements that are not recomputed'
    assert not np.isnan(g['X']).any() and (g['X'] >= 0).all()
    check(case, 'X', g['X'], r['X'])
    if cand.any():                                    # the recomputed elements alone (not diluted by the copies)
        v, where = G.measure(case, 'X', np.where(cand, g['X'], 0), np.where(cand, r['X'], 0))
        print('MEASURED rfix %s X(candidates) ratio %.3e floor %.3e bound %.3e' % (case.name, v, G.floors(case)['X'], G.bound(case, 'X')))
        assert v <= G.bound(case, 'X'), (case.name, v, where)
    w = np.zeros(case.bufs[0].size, bool)
    w[:m.rows * m.ld].reshape(m.rows, m.ld)[:, :m.cols] = True
    untouched(case, gpu, 0, w)
    for k in (1, 2, 3):
        untouched(case, gpu, k)


@pytest.mark.parametrize('case', G.cases('rset'), ids=lambda c: c.name)
def test_rowset_colsum(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    again = G.extract(case, run_gpu(ctx, case))
    check(case, 'out', g['out'], r['out'])
    assert same_bits(g['out'], again['out']), 'two runs differ'
    named = np.zeros((m.O, m.I), bool)
    for rows, o, i, ld, i0 in m.sets:
        named[:o, i0:i0 + i] = True
    assert not named.all() and (g['out'][~named] == G.SENT).all(), 'outputs no set names changed'
    untouched(case, gpu, 0, np.arange(case.bufs[0].size) < m.O * m.I)
    untouched(case, gpu, 1)
    untouched(case, gpu, 2)


@pytest.mark.parametrize('case', G.cases('add'), ids=lambda c: c.name)
def test_add(ctx, case):
    gpu, ref, g, r = both(ctx, case)
    assert same_bits(g['dst'], r['dst']), 'dst += src in float32; the slack keeps its bits'
    print('MEASURED add %s dst ratio %.3e floor %.3e bound %.3e' % (case.name, 0.0, 0.0, 0.0))
    untouched(case, gpu, 1)
