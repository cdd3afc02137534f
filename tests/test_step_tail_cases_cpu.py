"""
The case table of tests/step_tail_cases.py, checked without a GPU:

  * the images are honest: for every case the interpreter (tests/program_interp.py) leaves what the independent image says --
    every byte outside the loose regions equal, float results equal to 1e-12 (both evaluate in float64 and round to the float32
    buffers), NaNs where NaNs belong, the 16-bit copies of the AdamW-cast kinds equal to the cast of the interpreter's own
    parameters (twice: the fused op and a fresh GHN3_OP_CAST16).  For the bf16-state kinds the interpreter runs the package's
    own restatement (ghn3_amd.optim.adamw_state16_reference_): the case module's second restatement agrees with it bit for
    bit on every case, parameters included;
  * the table reaches every regime the issue behind it lists, re-derived from the cases' data;
  * no float32 intermediate of an AdamW case is subnormal, every floor is finite, and no bound is cut by the 2e-5 cap;
  * every op kind but nop / join / detach occurs in one of the four op-level case tables, and the interpreter has an op for
    every kind.

What the comparison found in the interpreter: op_adamw took the hyper-parameters as doubles where the op rounds them to float
(with beta2 = 0.999 the float 1 - beta2 is 1.3e-5 away from 0.001: exp_avg_sq differed by that much); op_memset0 with an absent
buffer zeroed the LAST buffer of the table (a negative index).  op_adamw_cast16, op_adamw_s16, op_adamw_s16_cast16,
op_wire_pack and op_rank_reduce are new.

"Changing the seed or the step changes more than 90 % of the stored moments" cannot hold for the stored codes: a moment whose
discarded half is f / 2^16 goes up with probability f under either seed, so two seeds disagree with probability 2 f (1 - f)
<= 1 / 2.  It is asserted here for the 16 rounding bits of each moment (which decide the codes), and the codes themselves are
held bit for bit against the restatement for every seed and step; they must differ between seeds for more than 25 %.
"""
import numpy as np
import pytest

import step_tail_cases as S
from ghn3_amd import _lib as L

CPU_TOL = 1e-12
ALL = S.all_cases()


def check_against_image(case, got):
    bad = S.mismatches(case, got)
    assert not bad, (case.name, bad)
    for name, buf, idx, ref, floor, err in S.float_checks(case):
        e = err(S.typed(case, got, buf)[idx], ref)
        # (results that are pinned bit for bit are float32 evaluations: they meet the float64 reference within its bound)
        exact = any(name == a[0] for a in case.also_float)
        assert (e <= (S.bounds_of(floor) if exact else CPU_TOL)).all(), (case.name, name, float(e.max()))
    if case.family.startswith('cast') and not case.meta.skipped:
        b = case.meta.bufs
        want = S.copy_image(case, S.typed(case, got, b[0]))
        for k in (b[5], b[6]):
            d = np.nonzero(S.typed(case, got, k) != want)[0]
            assert d.size == 0, (case.name, 'destination %d: %d codes differ, first at %d' % (k, d.size, d[0]))


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_interpreter_agrees_with_the_independent_image(case):
    if case.refused:
        with pytest.raises(AssertionError):
            S.run_interp(case)
        return
    check_against_image(case, S.run_interp(case))


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_floors_are_finite_and_bounds_below_the_cap(case):
    for name, buf, idx, ref, floor, err in S.float_checks(case):
        assert np.isfinite(floor).all() and np.isfinite(ref).all(), (case.name, name)
        raw = np.maximum(S.FLOOR_FACTOR * floor, S.MIN_BOUND)
        assert raw.max() <= S.FWD_CAP, (case.name, name, float(floor.max()), 'the input of this case asks for a bound above the cap')
        print(case.name, name, 'floor %.2e bound %.2e' % (floor.max(), S.bounds_of(floor).max()))


TINY = float(np.finfo(np.float32).tiny)


def _adamw_inputs(case):
    """(g, m, v as floats, cfg) of the elements an AdamW case updates"""
    m = case.meta
    if case.family in ('adamw',):
        return m.arrs[1], m.arrs[2], m.arrs[3], m.cfg
    if case.family == 's16':
        return m.arrs[1], S.widen(m.mb), S.widen(m.vb), m.cfg
    g = m.arrs[1][m.el]
    if m.s16:
        mb, vb = S.s16_state(m.arrs)
        return g, S.widen(mb[m.el]), S.widen(vb[m.el]), m.cfg
    return g, m.arrs[2][m.el], m.arrs[3][m.el], m.cfg


ADAMW_LIKE = [c for c in ALL if c.family in ('adamw', 's16', 'cast', 'cast-s16')]


@pytest.mark.parametrize('case', ADAMW_LIKE, ids=lambda c: c.name)
def test_no_float32_intermediate_is_subnormal(case):
    g, m, v, cfg = _adamw_inputs(case)
    clip = S.clip_of(cfg, np.float32)
    if clip is None:
        return
    f = np.float32
    b1, b2 = f(S.BETAS[0]), f(S.BETAS[1])
    gi = g * clip
    normal = lambda x: bool(((x == 0) | (np.abs(x) >= TINY)).all())
    assert ((gi == 0) | (np.abs(gi) >= 1e-15)).all(), case.name
    t1, t2 = (f(1) - b1) * gi, (f(1) - b2) * gi
    m2 = b1 * m + t1
    v2 = b2 * v + t2 * gi
    for x in (gi, t1, t2, t2 * gi, b1 * m, b2 * v, m2, v2, np.sqrt(v2), m, v):
        assert normal(x), case.name
    assert ((v == 0) | (v >= TINY)).all()


def test_every_named_regime_is_reached():
    adamw = [c for c in ALL if c.family == 'adamw']
    cfgs = {k for c in adamw for k, v in S.CFG.items() if v is c.meta.cfg}
    assert cfgs == set(S.CFG), set(S.CFG) - cfgs
    assert {c.meta.n for c in adamw} >= {1, 3, 4, 1023, 1024, 1025, 5156}
    C = S.CFG
    assert C['step1-clip']['step'] == 1 and abs(S.hyper(C['step1-clip'])[5] - 0.1) < 1e-12 and abs(S.hyper(C['step1-clip'])[6] - 1e-3) < 1e-12
    assert C['step1e4-nor4']['step'] == 10000 and C['step1e4-nor4']['ss'] is None and C['step1e4-nor4']['wd'] == 0
    assert C['lr0-f0neg']['lr'] == 0 and C['lr0-f0neg']['ss'] is not None and C['lr0-f0neg']['f0'] <= 0
    assert S.clip_of(C['step1-clip'], np.float64) < 0.51 and C['step1-clip']['wd'] > 0                       # clipping active
    assert S.clip_of(C['noclip'], np.float64) == 1.0 and S.clip_of(C['noclip'], np.float32) == 1.0           # norm below max_norm
    assert C['ss0']['ss'] == 0.0 and S.clip_of(C['ss0'], np.float32) == 1.0
    assert C['scale1024']['f1'] == 1.0 / 1024 and C['step1-clip']['f1'] == 0.0
    assert S.clip_of(C['inf'], np.float32) is None and S.clip_of(C['nan'], np.float32) is None
    # 1e-6 matters at 1e-4 in one clipped configuration (a kernel without it is 1e-4 off)
    c = C['tiny-norm']
    assert abs(S.clip_of(c, np.float64) / (c['f0'] / np.sqrt(c['ss'])) - 1) > 5e-5
    # per-element regimes, on the data of the 14000-element cases: every span kind occurs
    big = S.case_named('adamw-n14000-step1-clip')
    p, g, m, v = big.meta.arrs
    span = lambda x: x.reshape(-1)[:13 * 1024].reshape(13, 1024)
    assert any((span(g)[s] == 0).all() and (span(m)[s] == 0).all() and (span(v)[s] == 0).all() for s in range(13))      # the all-zero span
    assert any((span(g)[s] == 0).all() and (span(v)[s] == 0).all() and (span(m)[s] != 0).all() for s in range(13))      # eps alone
    assert ((g * m) < 0).any() and ((g * m) > 0).any() and (v == 0).any() and v.max() > 5e3 and np.abs(p).max() > 5e2
    mags = np.abs(g[g != 0])
    assert mags.min() < 2e-12 and mags.max() > 5e2
    img = big.image(np.float64)
    assert ((img[3][:14000] == 0) & (img[2][:14000] != 0)).any()                                                          # v' = 0, m' != 0
    by = {c.name: c for c in adamw}
    assert by['adamw-range-off1001'].meta.starts == [1001] * 4 and by['adamw-m-off4'].meta.starts == [0, 0, 1, 0]
    assert by['adamw-g-off4'].meta.starts == [0, 1, 0, 0]
    for nm in S.SAME_DATA:
        assert all(np.array_equal(a, b) for a, b in zip(by[nm].meta.arrs, by['adamw-aligned'].meta.arrs))
    # bf16 state
    s16 = {c.name: c for c in ALL if c.family == 's16'}
    assert (s16['s16-one'].meta.mb >> 15).any() and not (s16['s16-one'].meta.mb >> 15).all()                             # negative exp_avg
    assert s16['s16-m-off2'].shift == {2: 2} and s16['s16-n1025-scale1024'].meta.lo == 1001
    assert len(s16['s16-three-parts'].ops) == 3 and int(s16['s16-three-parts'].ops[1]['r']['off'][2]) == 2 * 1001
    for nm in S.S16_SAME:
        assert np.array_equal(s16[nm].meta.mb, s16['s16-one'].meta.mb)
    # the cast forms: descriptor counts, shapes, flags
    for fam in ('cast', 'cast-s16'):
        cs = [c for c in ALL if c.family == fam]
        assert {len(c.meta.descs) for c in cs} >= {1, 2, 3, 5}
        fl = [int(d['flags']) for c in cs for d in c.meta.descs]
        for want in (L.CAST_STRAIGHT, L.CAST_TRANSPOSED, L.CAST_STRAIGHT | L.CAST_TRANSPOSED):
            assert any(f & 3 == want for f in fl)
        for bit in (L.CAST_TIGHT, L.CAST_SPLIT, L.CAST_SPLIT_F16, L.CAST_FRAG, L.CAST_STRAIGHT_BF16, L.CAST_TRANSPOSED_BF16):
            assert any(f & bit for f in fl), bit
        assert any(f & L.CAST_TRANSPOSED_BF16 and not f & L.CAST_STRAIGHT_BF16 and f & L.CAST_STRAIGHT for f in fl)    # types per copy
        shapes = {(int(d['rows']), int(d['cols']), int(d['ld_src'])) for c in cs for d in c.meta.descs}
        assert {(64, 64, 64), (70, 132, 136), (1, 4, 4), (130, 64, 64)} <= shapes
        assert all(int(d['src_off']) > 0 and int(d['src_off']) % 4 == 0 for c in cs for d in c.meta.descs)
        assert any(c.meta.lo0 > 0 for c in cs) and any(c.meta.skipped for c in cs)
        sp = [c for c in cs if c.name.endswith('special-f16')][0]
        assert (np.abs(sp.meta.arrs[0][sp.meta.el]) > 65504).any() and sp.meta.cfg['lr'] == 0
        sb = [c for c in cs if c.name.endswith('special-bf16')][0]
        assert ((sb.meta.arrs[0][sb.meta.el].view(np.uint32) & 0xffff) == 0x8000).any()                                 # bf16 ties
    reached = set().union(*(c.regimes for c in ALL))
    need = ['sumsq:skip-at-0', 'sumsq:skip-to-n', 'sumsq:extra1', 'sumsq:extra3', 'sumsq:extra4', 'sumsq:extra261', 'wire:refused',
            'transpose:batch-both-routes', 'memset:absent'] + ['wire:n%d' % n for n in (1, 7, 8, 9, 2051)] + \
           ['reduce:W%d' % w for w in (1, 2, 5, 8)] + ['reduce:per%d' % p_ for p_ in (1, 3, 4, 5, 1003, 1024)] + \
           ['transpose:r%d' % r for r in (1, 63, 64, 65, 130)] + ['prologue:N%d' % n for n in (1, 2, 255, 256, 257, 1024, 33)]
    assert not [r for r in need if r not in reached]
    assert len({c.name for c in ALL}) == len(ALL)
    assert set(S.BIG) == {'adamw-loop', 's16-loop', 'sumsq-loop-plain', 'sumsq-loop-skip', 'wire-loop', 'reduce-loop'}
    print('%d cases' % len(ALL))


def test_the_prologue_cases_hold_what_the_clamps_must_see():
    for c in S.cases('prologue'):
        A, N, V = c.meta.A, c.meta.N, c.meta.V
        if N < 33:
            continue
        assert (A < 0).any() and (A == V).any() and (A > (1 << 32)).any() and (A < -(1 << 32)).any()
        assert not np.array_equal(A, np.swapaxes(A, 1, 2))
        assert {1000, 1001, -7} <= set(A[0, 0, 1:6].tolist())
        if N >= 255:
            one = (A == 1)
            want = {99, 100, 101} | ({300} if N >= 1024 else set())
            assert want <= set(one.sum(1).reshape(-1).tolist()) and want <= set(one.sum(2).reshape(-1).tolist()), c.name


def test_the_wire_reference_rounds_as_the_header_says():
    got = S.bf16_rne(S.WIRE_SPECIAL.view(np.float32))
    for u, want in S.WIRE_WANT.items():
        assert int(got[list(S.WIRE_SPECIAL).index(u)]) == want, hex(u)
    x = S.wire_values(2051, 0, ('t',))
    assert np.isnan(x).sum() >= 3 and np.isinf(x).any() and (x.view(np.uint32) == 0x80000000).any()
    lowonly = np.isnan(x) & ((x.view(np.uint32) & 0x007f0000) == 0)
    assert lowonly.sum() >= 2 and len({bool(s) for s in np.signbit(x[lowonly])}) == 2


def test_the_rank_order_columns_tell_a_tree_from_a_sequence():
    f = np.float32
    for W in (5, 8):
        v = [f(x) for x in S.ORDER[:W]]
        seq = f(0)
        for x in v:
            seq = f(seq + x)
        back = f(0)
        for x in reversed(v):
            back = f(back + x)
        tree = v
        while len(tree) > 1:
            tree = [f(tree[i] + tree[i + 1]) if i + 1 < len(tree) else tree[i] for i in range(0, len(tree), 2)]
        assert seq != back and seq != tree[0] and float(seq) != float(np.sum(np.asarray(v, np.float64)))


def test_the_second_restatement_agrees_with_the_packages_own():
    """s16_bits against optim.state16_random_bits, s16_eval against optim.adamw_state16_reference_ with a base, a seed and a
    step of its own (the interpreter test above covers every case of the table)"""
    import torch
    from ghn3_amd import optim
    for seed, step, base in ((0, 1, 0), (5, 10000, 1001), ((1 << 24) - 1, (1 << 24) - 1, (1 << 32) - 7)):
        assert np.array_equal(S.s16_bits(seed, step, base + np.arange(4096)), optim.state16_random_bits(seed, step, base, 4096).astype(np.uint64))
    cfg = dict(S.CFG['tiny-norm'], step=77)
    arrs = S.adamw_data(9000, ('restate',), 0)
    mb, vb = S.s16_state(arrs)
    p2, m2, v2 = S.s16_eval(arrs[0], arrs[1], mb, vb, cfg, 123, 555 + np.arange(9000))
    tp, tg = torch.from_numpy(arrs[0].copy()), torch.from_numpy(arrs[1].copy())
    tm = torch.from_numpy(mb.copy().view(np.int16)).view(torch.bfloat16)
    tv = torch.from_numpy(vb.copy().view(np.int16)).view(torch.bfloat16)
    optim.adamw_state16_reference_(tp, tg, tm, tv, cfg['ss'], 77, cfg['lr'], S.BETAS, S.EPS, cfg['wd'], cfg['f0'], cfg['f1'], seed=123, base=555)
    assert np.array_equal(tp.numpy().view(np.uint32), p2.view(np.uint32))
    assert np.array_equal(tm.view(torch.int16).numpy().view(np.uint16), m2) and np.array_equal(tv.view(torch.int16).numpy().view(np.uint16), v2)


def test_seed_and_step_change_the_rounding_bits_and_do_not_commute():
    idx = np.arange(14000)
    h = S.s16_bits(5, 1, idx)
    for other in (S.s16_bits(6, 1, idx), S.s16_bits(5, 2, idx), S.s16_bits(1, 5, idx)):
        assert ((h & 0xffff) != (other & 0xffff)).mean() > 0.9 and ((h >> 16) != (other >> 16)).mean() > 0.9
    a, b = S.case_named('s16-step5-seed1'), S.case_named('s16-step1-seed5')
    ia, ib = a.image(), b.image()
    for k in (2, 3):
        assert (ia[k] != ib[k]).mean() > 0.25
    one, six = S.case_named('s16-one').image(), S.case_named('s16-seed6').image()
    for k in (2, 3):
        assert (one[k] != six[k]).mean() > 0.25


def test_every_op_kind_has_an_op_level_case_and_an_interpreter_op():
    import decoder_tail_cases as D
    import gemm_pipeline_cases as G
    import graphormer_op_cases as O
    from program_interp import Interp
    used = set(S.kinds_used())
    for mod in (D, G, O):
        for c in mod.all_cases():
            used |= {int(k) for k in np.atleast_1d(c.ops['kind'])}
    missing = [L.OP_NAMES[k] for k in range(len(L.OP_NAMES)) if k not in used and L.OP_NAMES[k] not in ('nop', 'join', 'detach')]
    assert not missing, missing
    assert not [n for n in L.OP_NAMES if not hasattr(Interp, 'op_' + n)]
