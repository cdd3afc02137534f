"""
The Graphormer's attention, LayerNorm and gather / scatter kernels (ghn3_amd/csrc/attention.hip, elementwise.hip), one op record
at a time: every case of tests/graphormer_op_cases.py runs through `ctx.run` on device copies of its buffers and through the
float64 interpreter (tests/program_interp.py) on host copies, and the results are compared PER SLICE
(util_parity.slice_errors): per graph, head, 16- and 32-row query block, 32-key block and q / k / v third for attention, per row
and 64-channel group for LayerNorm, per output row / column block for the reductions.  An error confined to one tile is not
divided by the norm of everything else, as the whole-model parity tests do.

Bound of a tensor = 8 x the float32 floor of its case (the op's formula in plain numpy float32 against float64, graphormer_op_cases.formula;
the factor covers another summation order), at least 1e-6, never more than the published fp32 limits (2e-5 forward, 2e-4
gradients).  GHN3_OP_BIAS_HIST adds its fixed-point resolution, 2^-31 max|dBias| per term of a bin.  Pure index / copy results
(GHN3_OP_BIAS_GATHER, padded rows of GHN3_OP_EMBED_NODES, the masked dhid, sentinels of everything an op must not touch, the
in-place plane sums of LayerNorm) are bit-equal; the deterministic reductions run twice for equal bits.

What the kernels do with padded nodes (read from the code, asserted here): the forward writes `out` and P for every query row
below N -- a padded query has every score masked to -32768, so its P row is exactly 1 / N and its output the mean of all N value
rows, as in the reference; the backward writes every dqkv row below N: dQ and dK of padded nodes are exact zeros, dV is P^T dO
over ALL queries (the uniform rows of padded queries included); dBias outside the valid square keeps its value.

Measured on an MI355X (every check prints a `MEASURED family case tensor ratio floor bound` line under pytest -s; per tensor or
family the case with the largest ratio / bound; 137 cases, 5 s, all within their bounds):

  family  tensor ratio    floor    bound    case
  attn    out    1.9e-06  1.3e-06  1.0e-05  attn-N300-H2-C16-bound-nodbias-general
  attn    P      3.9e-06  5.0e-06  2.0e-05  attn-N1056-H2-C48-full-general
  attn    dqkv   1.8e-06  1.3e-06  1.0e-05  attn-N33-H1-C32-bound1
  attn    dBias  7.5e-07  4.8e-07  3.9e-06  attn-N17-H2-C48-bound-general
  ln      y      2.9e-07  2.3e-07  1.8e-06  ln-r257-C513-planesNone
  ln      dx     1.3e-06  1.2e-06  9.4e-06  ln-r257-C513-planesNone
  ln      mean   6.9e-08  0.0e+00  1.0e-06  ln-r1-C65-planes7-nores
  ln      rstd   1.5e-08  1.5e-08  1.0e-06  ln-r257-C65-planesNone
  lnpg    all    1.8e-07  1.9e-07  1.5e-06  lnpg-r16-C17-accum0
  hist    dT     5.9e-08  2.3e-07  1.8e-06  hist-V9-amax1
  edge    all    1.1e-07  8.3e-08  1.0e-06  edge-V9-C65
  embed   all    3.2e-07  1.5e-07  1.2e-06  embed-C8-onerow
  rowseg  out    3.8e-07  1.1e-06  9.2e-06  rowseg-C4-ldx7-ldo4-accum0
  colsum  out    1.2e-07  3.0e-07  2.4e-06  colsum-M256-N65-qNone-stride3-gather1
  dact    X      1.2e-07  1.2e-07  1.0e-06  dact-kind2-M70-N24-ld24-parts0-amax1

With one node P = 1 and O = V, so dS = P (dO . V - dO . O) is exactly 0 in exact arithmetic, but the two dot products are summed
in different orders (by the kernel: matrix core against a lane sum; by the float32 evaluation of the formula: matmul against
a pairwise sum) and differ in the last bit of a sum of ~4: the floor of that case's dBias is 1.9e-6, and the kernel gives the same.
"""
import numpy as np
import pytest
import torch

import graphormer_op_cases as G
from ghn3_amd import _lib as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    return L.context(0)


def run_gpu(ctx, case):
    """The case on device copies of its buffers -> the buffers as byte arrays (like graphormer_op_cases.run_interp)."""
    dev = [torch.from_numpy(b).cuda() for b in G.host_bytes(case)]
    ptrs = np.asarray([t.data_ptr() for t in dev], dtype=np.uint64)
    assert all(int(p) % 16 == 0 for p in ptrs)                  # (the regimes of the CPU test count on aligned allocations)
    ctx.run(case.ops, np.zeros(0, dtype=L.PROBLEM_DT), ptrs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in dev]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


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


def untouched(case, gpu, k):
    assert same_bits(gpu[k], G.host_bytes(case)[k]), (case.name, 'buffer %d changed' % k)


# ---- attention ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.cases('attn'), ids=lambda c: c.name)
def test_attention(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    for name in r:
        check(case, name, g[name], r[name])
    nn, N = np.asarray(m.nn), m.N
    valid = np.arange(N)[None, :] < nn[:, None]
    if m.save_p:                                      # rows of padded queries: exactly uniform over all N keys
        assert (g['P'][~valid[:, None, :, None] & np.ones((1, m.H, 1, N), bool)] == np.float32(1.0) / np.float32(N)).all()
    else:
        untouched(case, gpu, 3)
    if m.bwd:
        pad = ~valid
        assert (g['dqkv'][:, :, :2][pad] == 0).all(), 'dQ / dK of padded nodes are exact zeros'
        if m.dbias:
            sq = valid[:, None, :, None] & valid[:, None, None, :]
            assert (g['dBias'][~np.broadcast_to(sq, g['dBias'].shape)] == G.SENT).all(), 'dBias outside the valid square changed'
            am = float(G.f32(gpu, 8)[0])
            if m.amax:
                top = float(np.abs(g['dBias']).max())
                assert abs(am - top) <= 1e-6 * top, (am, top)
            else:
                assert am == 0.0
        else:
            untouched(case, gpu, 7)
            untouched(case, gpu, 8)
    else:
        untouched(case, gpu, 5)
        untouched(case, gpu, 7)
    for k in (1, 2, 4, 6):                            # inputs (and the float in front of a misaligned base)
        untouched(case, gpu, k)
    if m.misalign:
        assert all(float(G.f32(gpu, k)[0]) == 7.0 for k in (0, 3, 5, 7))


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.cases('ln'), ids=lambda c: c.name)
def test_layernorm(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    for name in r:
        check(case, name, g[name], r[name])
    xs, dys = G._ln_sums(case)
    # the in-place sums: a sequential float32 sum in plane order (include/ghn3_hip.h), bit for bit
    assert same_bits(G.f32(gpu, 1)[:xs.size], xs.reshape(-1)), 'x + planes written back'
    assert same_bits(G.f32(gpu, 8)[:dys.size], dys.reshape(-1)), 'dy + planes written back'
    if not m.stats:
        untouched(case, gpu, 4)
        untouched(case, gpu, 5)
    for k in (2, 3, 6, 9, 10, 11, 12):
        untouched(case, gpu, k)


@pytest.mark.parametrize('case', G.cases('lnpg'), ids=lambda c: c.name)
def test_ln_param_grad(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    again = G.extract(case, run_gpu(ctx, case))
    for name in r:
        check(case, name, g[name], r[name])
        assert same_bits(g[name], again[name]), (name, 'two runs differ')
    if m.batch:                                       # the batch on zeroed gradients = the single op with accum = 0 per item
        assert same_bits(g['dgamma'].reshape(-1), G.f32(gpu, 3)) and same_bits(g['dbeta'].reshape(-1), G.f32(gpu, 4))
        keep = np.ones(case.bufs[0].size, bool)
        for t in m.table:
            keep[t[0]:t[0] + m.C] = keep[t[1]:t[1] + m.C] = False
        assert (G.f32(gpu, 0)[keep] == 0).all(), 'gradient floats between the items changed'
    for k in range(2, len(case.bufs)):
        if not (m.batch and k in (3, 4)):
            untouched(case, gpu, k)


# ---- gather / scatter ops ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', G.cases('gather'), ids=lambda c: c.name)
def test_bias_gather(ctx, case):
    gpu, ref, g, r = both(ctx, case)
    assert same_bits(g['bias'], r['bias'])
    untouched(case, gpu, 1)
    untouched(case, gpu, 2)


@pytest.mark.parametrize('case', G.cases('hist'), ids=lambda c: c.name)
def test_bias_hist(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    again = G.extract(case, run_gpu(ctx, case))
    assert same_bits(g['dT'], again['dT']), 'two runs differ'
    got, exp = g['dT'].astype(np.float64), r['dT'].astype(np.float64)
    assert np.isfinite(got).all()
    assert (g['dT'][:, m.H:] == G.SENT).all(), 'padding columns of the table gradient changed'
    assert (g['dT'][m.counts == 0] == G.SENT).all(), 'rows of pair ids nobody has changed'
    err = np.sqrt(((got - exp) ** 2).sum(1))                      # per table row (pair id)
    den = np.linalg.norm(exp) / np.sqrt(len(exp))
    bd, fl = G.bound(case, 'dT'), G.floors(case)['dT']
    fixed = m.counts * 2.0 ** -31 * m.amax * np.sqrt(m.H)        # 2^-31 max|dBias| per term of the bin
    k = int(np.argmax(err - fixed))
    print('MEASURED hist %s dT ratio %.3e floor %.3e bound %.3e (+ fixed point %.3e)' %
          (case.name, max(err[k] - fixed[k], 0) / den, fl, bd, fixed[k] / den))
    assert (err <= bd * den + fixed).all(), (case.name, k, err[k] / den, bd, fixed[k] / den)
    untouched(case, gpu, 1)
    untouched(case, gpu, 2)


@pytest.mark.parametrize('case', G.cases('edge'), ids=lambda c: c.name)
def test_edge_hidden(ctx, case):
    gpu, ref, g, r = both(ctx, case)
    assert same_bits(g['dhid'], r['dhid']), 'the masked gradient is a copy'
    for name in ('hid', 'dPfw', 'dPbw'):
        check(case, name, g[name], r[name])
    assert ((g['hid'] == 0) == (r['hid'] == 0)).all(), 'ReLU of a pre-activation that is exactly 0'
    for k in (1, 2, 6):
        untouched(case, gpu, k)


@pytest.mark.parametrize('case', G.cases('embed'), ids=lambda c: c.name)
def test_embed(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    again = G.extract(case, run_gpu(ctx, case))
    padded = (np.arange(m.N)[None, :] >= m.nn[:, None]).reshape(-1)
    assert padded.any() and same_bits(g['x'][padded], np.zeros_like(g['x'][padded])), 'padded rows are exact zeros'
    check(case, 'x', g['x'], r['x'])
    for t, used in enumerate(G._embed_indexed(case)):
        name = 'dE%d' % t
        assert not used.all()
        assert (g[name][~used] == G.SENT).all(), (name, 'rows nobody indexes changed')
        check(case, name, g[name], r[name])
        assert same_bits(g[name], again[name]), (name, 'two runs differ')
    for k in range(1, 15):
        untouched(case, gpu, k)


@pytest.mark.parametrize('case', G.cases('rowseg'), ids=lambda c: c.name)
def test_rowseg_sum(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    again = G.extract(case, run_gpu(ctx, case))
    assert same_bits(g['out'][:, m.C:], case.bufs[0][:, m.C:]), 'columns between C and ldo changed'
    check(case, 'out', g['out'][:, :m.C], r['out'][:, :m.C])
    empty = np.asarray(m.lens) == 0
    assert (g['out'][empty, :m.C] == (G.SENT if m.accum else 0)).all(), 'empty segments'
    assert same_bits(g['out'], again['out']), 'two runs differ'


@pytest.mark.parametrize('case', G.cases('colsum'), ids=lambda c: c.name)
def test_colsum(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    keep = np.ones(g['out'].size, bool)
    keep[m.omap] = False
    assert (g['out'][keep] == G.SENT).all(), 'outputs the map does not name changed'
    check(case, 'out', g['out'], r['out'])
    untouched(case, gpu, 1)


@pytest.mark.parametrize('case', G.cases('dact'), ids=lambda c: c.name)
def test_dact(ctx, case):
    m = case.meta
    gpu, ref, g, r = both(ctx, case)
    assert same_bits(g['X'][:, m.N:], case.bufs[0][:, m.N:]), 'columns between N and ld changed'
    check(case, 'X', g['X'][:, :m.N], r['X'][:, :m.N])
    z = case.bufs[1][:, :m.N]
    if m.kind == L.DACT_RELU:
        assert (g['X'][:, :m.N][z == 0] == 0).all(), 'pre-activations that are exactly 0'
    elif m.kind == L.DACT_GELU and not m.n_parts:
        assert same_bits(g['X'][:, :m.N][z == 0], (case.bufs[0][:, :m.N] * np.float32(0.5))[z == 0]), 'gelu\'(0) = 1 / 2 exactly'
    am = float(G.f32(gpu, 2)[0])
    if m.amax:
        top = max(float(np.abs(g['X'][:, :m.N]).max()), float(case.bufs[2][0]))
        assert abs(am - top) <= 1e-6 * top, (am, top)
    else:
        untouched(case, gpu, 2)
    untouched(case, gpu, 1)
    untouched(case, gpu, 3)
