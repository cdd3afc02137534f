"""
The case table of tests/graphormer_op_cases.py, checked without a GPU:

  * the reference is honest: for every case the float64 interpreter (tests/program_interp.py, the reference of
    tests/test_gpu_graphormer_ops.py) agrees with an independent evaluation to float32 output rounding, <= 2e-7 per slice --
    torch float64 on the CPU for attention (softmax(Q K^T d^-1/2 + bias) with the key mask) and LayerNorm (F.layer_norm) with
    their autograd gradients, a few lines of numpy float64 for the other ops; sentinels of regions an op must not touch included;
  * the table reaches every regime of the launchers' dispatch (ghn3_attn_fwd / ghn3_attn_bwd in attention.hip, the launchers
    of elementwise.hip), re-derived here in Python: whoever edits the table cannot silently shrink the coverage;
  * the float32 floor of every case (the op's own formula in plain numpy float32 against float64, same slices) is finite and printed:
    the GPU tolerance is 8 x that floor, at least 1e-6, at most the project's published fp32 limits.
"""
import numpy as np
import pytest

import graphormer_op_cases as G
from ghn3_amd import _lib as L

CPU_TOL = 2e-7
ALL = G.all_cases()


def _same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_interpreter_agrees_with_an_independent_evaluation(case):
    got = G.extract(case, G.run_interp(case))
    ref = G.reference(case, np.float64)
    assert set(ref) <= set(got)
    worst = {}
    for name, r in ref.items():
        g = got[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        assert _same_nan(g, r), (name, 'sentinels differ')
        fin = np.isfinite(r)
        g, r = np.where(fin, g, 0), np.where(fin, r, 0)
        if case.family == 'attn':
            # on the valid rows, graph by graph: the all-zero slices of padded nodes would only shrink the RMS slice norm
            # the errors are divided by (rows of padded nodes: the sentinel pattern above, and the GPU test)
            parts = [G.measure(case, name, G.attn_valid(case, name, g, b), G.attn_valid(case, name, r, b)) for b in range(case.meta.B)]
            v, where = max(parts, key=lambda t: t[0])
        else:
            v, where = G.measure(case, name, g, r)
        worst[name] = v
        assert v <= CPU_TOL, (case.name, name, v, where)
    fl = G.floors(case)
    assert all(np.isfinite(v) for v in fl.values()), fl
    print(case.name, 'interp vs independent:', ', '.join('%s %.1e' % kv for kv in worst.items()),
          '| float32 floor:', ', '.join('%s %.1e' % kv for kv in fl.items()),
          '| bound:', ', '.join('%s %.1e' % (k, G.bound(case, k)) for k in fl))


# ---- the dispatch of the launchers, restated ----------------------------------------------------------------------------------
def _ks(d):
    return 2 if d <= 4 else 4 if d <= 8 else 8 if d <= 16 else 12 if d <= 24 else 16


def attn_regimes(c):
    """ghn3_attn_fwd / ghn3_attn_bwd (device allocations are 16-byte aligned: a base is aligned iff its byte offset is)."""
    m = c.meta
    nb = (m.N + 31) // 32
    tpw = (nb + 3) // 4
    vec = int(m.C % 4 == 0 and m.off % 16 == 0)
    vq = int(vec and m.d % 4 == 0)
    pvec = int(vec and m.N % 4 == 0)
    r = {'fwd:' + ('staged16' if tpw <= 2 else 'reg32' if tpw <= 8 else 'stream'), 'KS%d' % _ks(m.d), 'vec%d' % vec, 'vq%d' % vq,
         'pvec%d' % pvec, 'fwd:bias%d' % m.bias, 'fwd:P%d' % m.save_p, 'partial-k-step%d' % int(m.d % 2 == 1 or m.d < 2 * _ks(m.d) - 1)}
    if m.bwd:
        nw = 8 if m.N <= 256 else 4
        staged = nw == 8 and vec and m.d % 4 == 0 and not m.general
        r |= {'bwd:NW%d' % nw, 'bwd:' + ('staged' if staged else 'general'), 'bwd:dbias%d' % m.dbias, 'bwd:amax%d' % m.amax,
              'bwd:general-flag%d' % m.general}
        if nw == 8 and vec and m.d % 4 == 0 and m.general:
            r.add('bwd:general-where-staged-would-run')
    nn = np.asarray(m.nn)
    for edge in (16, 32):
        if (nn == edge).any() and m.N > edge:
            r.add('graph-ends-on-%d' % edge)
        if (nn == edge + 1).any() and m.N > edge + 1:
            r.add('graph-ends-past-%d' % edge)
    if (nn == m.N).all():
        r.add('all-full')
    if len(nn) == 3 and list(nn) == [m.N, m.N - 1, 1]:
        r.add('N,N-1,1')
    if m.misalign:
        r.add('misaligned')
    return r


def ln_regimes(c):
    m = c.meta
    r = {'ln:' + ('registers' if m.C <= 8 * 64 else 'loop'), 'ln:stats%d' % m.stats, 'ln:residual%d' % m.residual}
    r.add('ln:planes-' + ('absent' if m.planes is None else 'i2=0' if m.planes == 0 else '<=7' if m.n_pl <= 7 else '>7'))
    r.add(('ln:registers' if m.C <= 512 else 'ln:loop') + ('+planes' if m.n_pl else ''))
    if m.C <= 512 and m.n_pl > 7:
        r.add('ln:registers+planes>7')
    r |= {'ln:row-' + k for k in m.special}
    return r


def other_regimes(c):
    m, f = c.meta, c.family
    if f == 'lnpg':
        return {'lnpg:batch'} if m.batch else {'lnpg:accum%d' % m.accum, 'lnpg:rows' + ('<=16' if m.rows <= 16 else '<=128' if m.rows <= 128 else '>128'),
                                              'lnpg:col-blocks' + ('1' if m.C <= 16 else '>1')}
    if f == 'gather':
        return {'gather:' + ('lds' if m.ldT <= 64 else 'direct'), 'gather:key-blocks' + ('1' if m.N <= 256 else '>1')}
    if f == 'hist':
        return {'hist:' + ('lds' if 8 * m.V * m.V <= 64 * 1024 else 'global'), 'hist:amax%d' % m.have_amax}
    if f == 'edge':
        return {'edge:col-blocks' + ('1' if m.C <= 64 else '>1'), 'edge:V' + ('<4' if m.V < 4 else '>=4')}
    if f == 'embed':
        return {'embed:C' + ('<=256' if m.C <= 256 else '>256'), 'embed:one-row%d' % m.one_row}
    if f == 'rowseg':
        vec = m.C % 4 == 0 and m.ldx % 4 == 0
        return {'rowseg:' + ('vec' if vec else 'scalar'), 'rowseg:accum%d' % m.accum, 'rowseg:ldo' + ('>C' if m.ldo > m.C else '=C')}
    if f == 'colsum':
        return {'colsum:row-blocks' + ('1' if m.M <= 256 else '>1'), 'colsum:map%d' % int(m.q > 0), 'colsum:stride' + ('1' if m.stride == 1 else '>1'),
                'colsum:gather%d' % m.gather, 'colsum:col-blocks' + ('1' if m.N <= 64 else '>1')}
    if f == 'dact':
        vec = m.N == m.ld and m.N % 4 == 0
        return {'dact:kind%d' % m.kind, 'dact:' + ('vec' if vec else 'scalar'), 'dact:amax%d' % m.amax,
                'dact:planes' + ('0' if not m.n_parts else '<=8' if m.n_parts <= 8 else '>8')}
    raise KeyError(f)


REQUIRED = {
    'attn': {'fwd:staged16', 'fwd:reg32', 'fwd:stream', 'KS2', 'KS4', 'KS8', 'KS12', 'KS16', 'vec0', 'vec1', 'vq0', 'vq1', 'pvec0', 'pvec1',
             'partial-k-step0', 'partial-k-step1', 'fwd:bias0', 'fwd:bias1', 'fwd:P0', 'fwd:P1', 'bwd:NW8', 'bwd:NW4', 'bwd:staged',
             'bwd:general', 'bwd:general-where-staged-would-run', 'bwd:dbias0', 'bwd:dbias1', 'bwd:amax0', 'bwd:amax1',
             'bwd:general-flag0', 'bwd:general-flag1', 'graph-ends-on-16', 'graph-ends-on-32', 'graph-ends-past-16',
             'graph-ends-past-32', 'all-full', 'N,N-1,1', 'misaligned'},
    'ln': {'ln:registers', 'ln:loop', 'ln:registers+planes', 'ln:loop+planes', 'ln:registers+planes>7', 'ln:planes-absent', 'ln:planes-i2=0',
           'ln:planes-<=7', 'ln:planes->7', 'ln:stats0', 'ln:stats1', 'ln:residual0', 'ln:residual1', 'ln:row-big', 'ln:row-const'},
    'lnpg': {'lnpg:batch', 'lnpg:accum0', 'lnpg:accum1', 'lnpg:rows<=16', 'lnpg:rows<=128', 'lnpg:rows>128', 'lnpg:col-blocks1',
             'lnpg:col-blocks>1'},
    'gather': {'gather:lds', 'gather:direct', 'gather:key-blocks1', 'gather:key-blocks>1'},
    'hist': {'hist:lds', 'hist:global', 'hist:amax0', 'hist:amax1'},
    'edge': {'edge:col-blocks1', 'edge:col-blocks>1', 'edge:V<4', 'edge:V>=4'},
    'embed': {'embed:C<=256', 'embed:C>256', 'embed:one-row0', 'embed:one-row1'},
    'rowseg': {'rowseg:vec', 'rowseg:scalar', 'rowseg:accum0', 'rowseg:accum1', 'rowseg:ldo>C', 'rowseg:ldo=C'},
    'colsum': {'colsum:row-blocks1', 'colsum:row-blocks>1', 'colsum:map0', 'colsum:map1', 'colsum:stride1', 'colsum:stride>1',
               'colsum:gather0', 'colsum:gather1', 'colsum:col-blocks1', 'colsum:col-blocks>1'},
    'dact': {'dact:kind0', 'dact:kind1', 'dact:kind2', 'dact:vec', 'dact:scalar', 'dact:amax0', 'dact:amax1', 'dact:planes0',
             'dact:planes<=8', 'dact:planes>8'},
}


def regimes(c):
    return attn_regimes(c) if c.family == 'attn' else ln_regimes(c) if c.family == 'ln' else other_regimes(c)


@pytest.mark.parametrize('family', sorted(REQUIRED))
def test_the_table_reaches_every_regime(family):
    reached = {}
    for c in G.cases(family):
        for r in regimes(c):
            reached.setdefault(r, []).append(c.name)
    for r in sorted(reached):
        print('%-40s %d case(s), e.g. %s' % (r, len(reached[r]), reached[r][0]))
    missing = REQUIRED[family] - set(reached)
    assert not missing, missing


def test_the_attention_rows_cross_node_counts_and_head_dims_as_stated():
    """Every N with d = 8 and d = 24, every d with N = 33 and N = 257, the boundaries of both forward thresholds, and the
    combinations a single flag cannot show: the staged backward at every KS bucket, the 4-wave backward with and without vq."""
    cs = [c.meta for c in G.cases('attn') if c.meta.bwd]
    have = {(m.N, m.d) for m in cs}
    for N in G.ATTN_N:
        assert (N, 8) in have and (N, 24) in have, N
    for d in G.ATTN_HC:
        assert (33, d) in have and (257, d) in have, d
    assert {256, 257, 1056} <= set(G.ATTN_N) and max(n for n in G.ATTN_N if n <= 1024) >= 257
    staged = {_ks(m.d) for m in cs if m.N <= 256 and m.C % 4 == 0 and m.d % 4 == 0 and not m.general and not m.misalign}
    assert staged == {2, 4, 8, 12, 16}, staged
    assert {(m.d % 4 == 0) for m in cs if m.N > 256} == {True, False}
    assert any(m.H == 16 and m.C == 384 and m.N == 33 for m in cs)


def test_names_are_unique():
    names = [c.name for c in ALL]
    assert len(names) == len(set(names))
