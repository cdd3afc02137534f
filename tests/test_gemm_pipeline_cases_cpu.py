"""
The case table of tests/gemm_pipeline_cases.py, checked without a GPU:

  * the reference is honest: for every case the float64 interpreter (tests/program_interp.py) agrees with the independent
    evaluation `reference`, which never reads the op records -- 16-bit copies bit for bit, float results to 1e-12 relative per
    tensor (both round to the float32 buffers), and nothing outside the places a case names is written;
  * the table reaches every regime the issue behind it lists (scaled operands per tile code / type / amax kind, `lim` tables of
    both kinds per tile code, GHN3_GEMM_SUMSQ and the GHN3_OP_SUMSQ forms, the fp32 kernels' fields, the cast variants), the
    cast cases take the straight-copy path they are meant to take, and the table stays small;
  * every case's float32 floor is finite and printed, and its bound -- 8 x the floor, at least 1e-6 -- is below the project's
    2e-5 without being cut: an ill-chosen input cannot ask for a wide bound.

What the comparison found in the interpreter: Interp.to16 rounded |x| > 65504 to an f16 infinity where cast_f16 saturates
(cast-paths cases, 65520 and 1e5); GHN3_OP_SUMSQ ignored the excluded range [i1, i2), the slot table r3 and added in float32;
GHN3_GEMM_SUMSQ added every problem into slot 0 of its table (a NaN sentinel there poisons the sum): tile codes 29 / 30 now
write each tile's sum to the slots of its id in the launch.
"""
import numpy as np
import pytest

import gemm_pipeline_cases as G
from ghn3_amd import _lib as L

CPU_TOL = 1e-12
ALL = G.all_cases()


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_interpreter_agrees_with_an_independent_evaluation(case):
    host = G.run_interp(case)
    got = G.extract(case, host)
    ref = G.reference(case, np.float64)
    worst = {}
    for o in case.outs:
        g, r = got[o.name], ref[o.name]
        assert g.shape == r.shape, (o.name, g.shape, r.shape)
        if o.kind == 'bits':
            assert np.array_equal(g, r), (case.name, o.name, '16-bit codes differ', int((g != r).sum()))
            continue
        g = G.masked(case, o.name, g, r)
        assert np.isfinite(r).all() and np.isfinite(g).all(), (case.name, o.name)
        worst[o.name] = rel(g, r)
        assert worst[o.name] <= CPU_TOL, (case.name, o.name, worst[o.name])
    # everything else keeps its bits (the interpreter writes nothing into don't-care regions but scratch)
    w = G.written(case)
    before = G.host_bytes(case)
    for k, b in enumerate(case.bufs):
        item = b.dtype.itemsize
        keep = np.repeat(~w[k], item)
        assert np.array_equal(host[k][keep], before[k][keep]), (case.name, 'buffer %d written outside the named places' % k)
    print(case.name, 'worst %.1e' % max(worst.values(), default=0.0))


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_floors_are_finite_and_bounds_below_the_cap(case):
    fl = G.floors(case)
    for name, v in fl.items():
        assert np.isfinite(v), (case.name, name, v)
        assert G.raw_bound(case, name) <= G.FWD_CAP, (case.name, name, v, 'the input of this case asks for a bound above the cap')
        assert G.MIN_BOUND <= G.bound(case, name) <= G.FWD_CAP
    print(case.name, ', '.join('%s floor %.2e bound %.2e' % (k, v, G.bound(case, k)) for k, v in fl.items()))


WIDENED = {'scaled-t20-f16-zero-K456-alpha', 'scaled-t24-f16-1e-35-K456', 'scaled-t25-f16-1e4-K456', 'scaled-t29-f16-zero-K456',
           'scaled-t30-f16-1e-35-K456-alpha', 'scaled-t24-f16-zero-K1', 'scaled-t30-f16-zero-K1-alpha'}


def test_only_the_cases_with_subnormal_f16_copies_have_a_wider_factor():
    """the factor 8 is widened for exactly the f16 cases whose scale (<= 1) leaves subnormal operand copies -- the reason and the
    measured ratios stand beside SUBNORMAL_F16_FACTOR in tests/gemm_pipeline_cases.py and in docs/HISTORY.md"""
    assert {c.name for c in ALL if G.widened(c)} == WIDENED
    for c in ALL:
        if G.widened(c):
            assert not c.meta.bf and c.meta.sc <= 1.0 and c.family == 'scaled'


REQUIRED = (
    ['scaled:tile%s' % t for t in (0, 16, 20, 24, 25, 28, '28m', 29, 30)] + ['scaled:f16', 'scaled:bf16'] +
    ['scaled:amax-' + k for k in G.AMAX] + ['scaled:shared-slot', 'scaled:alpha', 'scaled:subnormal-K1'] +
    ['scaled:ring-wrap-tile%d' % t for t in (16, 20, 24, 25, 28, 29, 30)] +
    ['lim:kind%d-tile%d' % (k, t) for k in (1, 2) for t in (0, 16, 20, 24, 28)] +
    ['lim:two-entries', 'lim:kind2-kmap', 'lim:kind2-ksplit', 'lim:kind2-amax'] +
    ['sumsq:' + n for n in ('tile29', 'tile30', 'ragged', 'cmap', 'grid-cap', 'tiles-per-wg', 'op-range', 'two-problems', 'walk', 'xcd-groups', 'plain-scratch', 'plain-atomic')] +
    ['f32:' + n for n in ('b_gather', 'a_qs', 'bias_qs', 'ksplit2-t64', 'ksplit3-t64', 'ksplit2-t128', 'ksplit3-t128')] +
    ['cast:' + n for n in ('parts', 'tight', 'src-map', 'scaled-colsum', 'grid-cap', 'search', 'paths', 'special', 'tail1', 'tail4', 'tail7')])


def test_every_named_regime_is_reached_and_the_table_stays_small():
    reached = set().union(*(c.regimes for c in ALL))
    missing = [r for r in REQUIRED if r not in reached]
    assert not missing, missing
    assert len(ALL) <= G.MAX_CASES, len(ALL)
    assert len({c.name for c in ALL}) == len(ALL)
    print('%d cases' % len(ALL))


def test_the_regime_labels_follow_from_the_cases():
    """the labels a case carries are re-derived from its op records and problem table"""
    for c in ALL:
        for r in c.regimes:
            fam, what = r.split(':')
            gemms = [o for o in c.ops if int(o['kind']) == L.OP_GEMM]
            if fam in ('scaled', 'lim') or r in ('sumsq:tile29', 'sumsq:tile30'):
                p = c.problems[0]
                assert int(p['flags']) & L.GEMM_OP16
            if fam == 'scaled':
                assert int(c.problems[0]['alpha_amax']['buf']) >= 0
                if what.startswith('tile'):
                    assert int(gemms[0]['i'][2]) == int(what[4:6].rstrip('m')) and (what.endswith('m')) == (int(c.problems[0]['mtiles']['buf']) >= 0)
                if what == 'alpha':
                    assert float(c.problems[0]['alpha']) != 1.0
            if fam == 'lim' and what.startswith('kind') and '-tile' in what:
                p = c.problems[0]
                assert int(p['lim']['buf']) >= 0 and int(p['mtiles']['buf']) < 0 and int(p['lim_kind']) == int(what[4])
                assert int(gemms[0]['i'][2]) == int(what.split('tile')[1])
                assert 3 <= (int(p['M']) + 127) // 128 <= 5
            if r == 'lim:kind2-kmap':
                assert int(c.problems[0]['b_kq']) > 0
            if r == 'lim:kind2-ksplit':
                assert int(c.problems[0]['ksplit']) > 1
            if r in ('sumsq:tile29', 'sumsq:tile30'):
                assert int(c.problems[0]['flags']) & L.GEMM_SUMSQ and int(gemms[0]['i'][2]) == int(what[4:])
                assert c.bufs[c.meta.b_slots].size > 8 * c.meta.n_ids and len(c.meta.ids) < c.meta.n_ids      # ids that name no tile exist
            if r == 'sumsq:two-problems':
                assert int(gemms[0]['i'][1]) == 2 and len(gemms) == 1 and int(c.problems[1]['aux_out']['buf']) != int(c.problems[0]['aux_out']['buf'])
            if r == 'sumsq:xcd-groups':
                assert int(c.problems[0]['N']) * int(c.problems[0]['K']) * 2 > G.XCD_B_BYTES
                assert {t % 8 for (mt, nt), t in c.meta.ids.items() if mt == 0} == {0, 1}        # row tile 0 on two XCDs: G = 2
            if r == 'sumsq:walk':                     # fewer workgroups than tile ids, no bound on the tiles of a workgroup
                cap = int(gemms[0]['i'][3])
                assert 0 < cap < c.meta.n_ids and cap >> 16 == 0 and len(c.meta.ids) > cap // 2
            if r == 'scaled:subnormal-K1':
                assert G.widened(c) and c.meta.K == 1 and c.meta.sc == 1.0
            if r == 'sumsq:op-range':
                o = [o for o in c.ops if int(o['kind']) == L.OP_SUMSQ][0]
                assert int(o['i'][1]) < int(o['i'][2]) and int(o['i'][3]) > 0
            if r == 'f32:b_gather':
                p = c.problems[0]
                assert all(int(p[n]['buf']) >= 0 for n in ('a_gather', 'b_gather', 'c_gather')) and int(p['flags']) & L.GEMM_ACCUM
                assert int(p['a_mode']) == L.MODE_COL and int(p['b_mode']) == L.MODE_COL
            if r.startswith('f32:ksplit'):
                assert int(c.problems[0]['ksplit']) == int(what[6]) and int(gemms[0]['i'][2]) == int(what.split('-t')[1])
            if fam == 'cast':
                D = c.meta.descs
                fl = [int(d['flags']) for d in D]
                if what == 'parts':
                    assert any(f & L.CAST_COLSUM_PARTS for f in fl) and any(int(d['rows']) % 64 and int(d['cols']) % 64 for d in D)
                if what == 'tight':
                    assert any(f & L.CAST_TIGHT and int(d['rows']) % 8 for f, d in zip(fl, D))
                if what == 'src-map':
                    assert any(int(d['src_q']) > 0 for d in D)
                if what == 'scaled-colsum':
                    assert any((f & L.CAST_SCALED) and (f & L.CAST_COLSUM) and not f & L.CAST_COLSUM_PARTS for f in fl)
                if what == 'grid-cap':
                    assert 0 < c.meta.grid_cap < c.meta.blocks
                if what == 'search':
                    assert len(D) >= 3 and len({int(d['rows']) * int(d['cols']) for d in D}) >= 3
                if what == 'paths':
                    assert [G.straight_path(d) for d in D] == ['fast', 'general', 'general']
                    assert int(D[1]['dst_off']) % 8 and int(D[2]['lo_off']) % 8
                    ref = G.reference(c)
                    assert np.array_equal(ref['d0.st'], ref['d1.st']) and np.array_equal(ref['d0.st'], ref['d2.st'])
                if what.startswith('tail'):
                    assert int(D[0]['cols']) % 8 == int(what[4:])


def test_every_place_that_applies_the_inverse_scale_sees_a_scale_that_is_not_one():
    """gemm.hip and gemm_p8.hip undo the scale of the copies in six places: the row epilogue of tile codes 16 / 20 / 24, their
    split-K epilogue, and the kernels of tile codes 25, 28, 29 and 30.  With amax 0 or 1e-35 the inverse scale is 1 and a wrong
    exponent would not show: every tile code and split-K need a case with another scale, and for every tile code one
    of them is f16 and not among the cases with the wider factor."""
    def scaled_ops(c):
        if not len(c.problems):
            return None
        p = c.problems[0]
        if not (int(p['flags']) & L.GEMM_OP16 and int(p['alpha_amax']['buf']) >= 0 and c.meta.sc != 1.0):
            return None
        tile = int([o for o in c.ops if int(o['kind']) == L.OP_GEMM][0]['i'][2])
        return (16 if tile == 0 else tile), int(p['ksplit']) > 1
    seen = {}
    for c in ALL:
        t = scaled_ops(c)
        if t is not None:
            seen.setdefault(t, []).append(c)
    for tile in (16, 20, 24, 25, 28, 29, 30):
        cs = seen.get((tile, False), [])
        assert cs, ('no unsplit case with a scale != 1 on tile code', tile)
        assert any(not c.meta.bf and not G.widened(c) for c in cs), ('no f16 case at the factor-8 bound on tile code', tile)
    assert any(split for (_, split) in seen), 'no split-K case with a scale != 1'
    assert any(c.meta.sc < 1.0 for cs in seen.values() for c in cs) and any(c.meta.sc > 1.0 for cs in seen.values() for c in cs)


def test_the_special_values_round_as_the_kernels_round():
    f16 = G.back16(G.to16(G.SPECIAL, False), False)
    assert list(f16[:7]) == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, 65504.0, -65504.0]      # saturation, no infinity
    assert f16[7] == np.float32(2.0 ** -24) and f16[9] == 0.0 and np.signbit(f16[13]) and f16[15] == 65504.0
    bf = G.back16(G.to16(G.SPECIAL, True), True)
    assert bf[10] == 1.0 and bf[11] == np.float32(1.015625) and bf[12] == -1.0 and np.signbit(bf[13])  # ties to even
    for amax, want in ((2.0 ** -21, 2.0 ** 32), (np.nextafter(np.float32(2.0 ** -21), np.float32(0)), 2.0 ** 33), (0.0, 1.0), (1e-35, 1.0),
                       (1e4, 2.0 ** -2)):
        assert G.pow2_scale(amax) == want, (amax, G.pow2_scale(amax), want)
