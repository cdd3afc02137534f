"""
The case table of tests/decoder_tail_cases.py, checked without a GPU:

  * the reference is honest: for every case the float64 interpreter (tests/program_interp.py, the reference of
    tests/test_gpu_decoder_tail_ops.py) agrees with the independent float64 evaluation `reference` to 1e-12 relative per tensor
    (both round their results to the float32 buffers; NaN sentinels in the same places; 16-bit codes equal);
  * the table reaches every regime of the kernels' run-time dispatch (tile_fwd_kernel, tile_bwd_kernel, param_sq_kernel, ... in
    ghn3_amd/csrc/elementwise.hip), re-derived here from the descriptors and the work-block tables: whoever edits the table
    cannot silently shrink the coverage;
  * the float32 floor of every tensor is finite and below the published limit of its kind;
  * the work-block tables of ghn3_amd.program.tile_work_tables: every target element of a descriptor is written by exactly one
    forward block and every region element by exactly one backward block.
"""
import numpy as np
import pytest

import decoder_tail_cases as G

CPU_TOL = 1e-12
ALL = G.all_cases()


def rel(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_interpreter_agrees_with_an_independent_evaluation(case):
    got = G.extract(case, G.run_interp(case))
    ref = G.reference(case, np.float64)
    assert set(got) <= set(ref), set(got) - set(ref)
    worst = {}
    for name, g in got.items():
        r = ref[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if name.startswith('h16.'):
            assert np.array_equal(g, r), (case.name, name, '16-bit codes differ')
            continue
        assert np.array_equal(np.isnan(g), np.isnan(r)), (name, 'sentinels differ')
        fin = np.isfinite(r)
        worst[name] = rel(np.where(fin, g, 0), np.where(fin, r, 0))
        assert worst[name] <= CPU_TOL, (case.name, name, worst[name])
    print(case.name, 'worst %.1e' % max(worst.values()))


@pytest.mark.parametrize('case', ALL, ids=lambda c: c.name)
def test_floors_are_finite_and_below_the_cap(case):
    fl = G.floors(case)
    for name, v in fl.items():
        assert np.isfinite(v) and v < G.cap(case, name), (case.name, name, v)
        assert G.MIN_BOUND <= G.bound(case, name) <= G.cap(case, name)
    print(case.name, ', '.join('%s %.1e' % kv for kv in fl.items()))


# ---- the block tables ---------------------------------------------------------------------------------------------------------
TILE = [c for c in ALL if c.family in ('tilef', 'tileb', 'tileb16')]


@pytest.mark.parametrize('case', TILE, ids=lambda c: c.name)
def test_every_element_belongs_to_exactly_one_work_block(case):
    m = case.meta
    for table, shape_of in ((m.fb, lambda d: d.T), (m.bb, lambda d: d.R)):
        hits = [np.zeros(int(np.prod(shape_of(d))), np.int32) for d in m.descs]
        last = -1
        for k in range(len(table)):
            di, lo, hi, row = G.block_range(case, table, k, shape_of)
            assert di >= last and 0 <= lo <= hi <= len(hits[di])
            last = di
            if row is not None:
                d = m.descs[di]
                ich = int(m.desc_arr['_pad'][di])
                assert d.mode == 0 and d.S[1] == 1 and d.T[2:] == d.E[2:] == d.R[2:] and 1 < d.T[2] * d.T[3] <= 1024     # the host's promises
                assert (ich % 16 == 0 or ich == max(d.T[1], d.R[1])) and (row[1] % ich == 0) and row[0] < shape_of(d)[0]
            hits[di][lo:hi] += 1
        for di, h in enumerate(hits):
            assert (h == 1).all(), (case.name, di)
    assert m.lds[0] <= 128 * 1024


# ---- the kernels' branches, restated --------------------------------------------------------------------------------------------
def tile_regimes(c):
    m = c.meta
    r = set()
    A = m.desc_arr
    if m.fwd:
        r |= {'f:sq%d' % m.sq, 'f:bp%d' % m.bp}
        if m.lds[0] > 48 * 1024:
            r.add('f:lds>48K')
        for k in range(len(m.fb)):
            di, lo, hi, row = G.block_range(c, m.fb, k, lambda d: d.T)
            d = m.descs[di]
            T, E, S = d.T, d.E, d.S
            if row is None:
                r |= {'fe:mode%d' % d.mode, 'fe:buf%d' % d.buf}
                wrap = [E[j] != T[j] for j in range(4)]
                if sum(wrap) == 1:
                    r.add('fe:wrap%d-alone' % wrap.index(True))
                if all(wrap):
                    r.add('fe:wrap-all')
                if d.numel < 256:
                    r.add('fe:numel<256')
                if d.numel % 256:
                    r.add('fe:numel%256')
                if d.numel % 2048 and d.numel > 2048:
                    r.add('fe:numel%2048')
                if d.numel > 2 * G.CHUNK:
                    r.add('fe:several-blocks')
                # Odo::step: the digits of 256 in radices T; a carry runs through three digits when all radices below are small
                s3, q = 256 % T[3], 256 // T[3]
                s2, q = q % T[2], q // T[2]
                s1 = q % T[1]
                if (T[3] < 256 and T[2] * T[3] < 256 and s3 and s2) or (T[2] == T[3] == 1 and T[1] > 256):
                    r.add('fe:odo-carry')
                if lo > 0 and lo // (T[1] * T[2] * T[3]) > 0:
                    r.add('fe:start-top-digit')
                if 0 in S:
                    r.add('fe:stride0')
                if d.src_off:
                    r.add('fe:src_off')
                if d.scale != 1.0 and d.mode == 0:
                    r.add('fe:scale')
            else:
                a0, i0 = row
                hw = T[2] * T[3]
                ni = min(int(A['_pad'][di]), T[1] - i0)
                n = ni * hw
                r.add('fr:hw%d' % hw)
                base = d.src_off + (a0 % E[0]) * S[0] + i0
                why = []
                if E[1] != T[1]:
                    why.append('E1')
                if ni % 4:
                    why.append('ni')
                if S[2] % 4 or S[3] % 4:
                    why.append('S23')
                if base % 4:
                    why.append('base')
                r.add('fr:vec' if not why else 'fr:scalar')
                if len(why) == 1:
                    r.add('fr:scalar-only-' + why[0])
                if i0 > 0 and ni < int(A['_pad'][di]):
                    r.add('fr:short-last-chunk')
                if T[1] < 16:
                    r.add('fr:T1<16')
                if E[0] < T[0] and a0 >= E[0]:
                    r.add('fr:a0%E0')
                if n % 4:
                    r.add('fr:n%4')
                if (d.dst_off + (a0 * T[1] + i0) * hw) % 4:
                    r.add('fr:row-start%4')
                if d.scale != 1.0:
                    r.add('fr:scale')
                if d.fill == 'zero':
                    r.add('fr:norm0')
    if m.bwd:
        r |= {'b:src-' + m.bwd, 'b:amax0-' + ('zero' if m.amax0 == 0 else 'set')}
        ref = G.reference(c)
        if m.bf16 is None and any(d.buf == 0 for d in m.descs):
            top = max(float(np.abs(ref['dsrc.d%d' % k]).max()) for k, d in enumerate(m.descs) if d.buf == 0)
            if m.amax0 > 0:
                r.add('b:amax0-above' if m.amax0 > top else 'b:amax0-below')
        if all(d.buf != 0 for d in m.descs):
            r.add('b:no-buf0')
        if m.bf16 is not None:
            r.add('h:bf16' if m.bf16 else 'h:f16')
        for k in range(len(m.bb)):
            di, lo, hi, row = G.block_range(c, m.bb, k, lambda d: d.R)
            d = m.descs[di]
            T, E, S, R = d.T, d.E, d.S, d.R
            reps = [(T[j] + E[j] - 1) // E[j] for j in range(4)]
            to16 = m.bf16 is not None and d.h is not None
            if m.bf16 is not None:
                r.add('h:' + ('16bit' if to16 else 'keeps-fp32-h-min' if d.buf == 0 else 'keeps-fp32-buf%d' % d.buf) + ('-elem' if row is None else '-row'))
            if to16:
                hoff, rel0, ld32, ld16 = d.h
                assert ld16 != ld32
            if row is None:
                r |= {'be:mode%d' % d.mode, 'be:R1=%d' % R[1]}
                for j in range(4):
                    if R[j] > E[j]:
                        r.add('be:R%d>E%d' % (j, j))
                big = [reps[j] > 1 for j in range(4)]
                part = [T[j] % E[j] != 0 for j in range(4)]
                if sum(big) == 1 and any(part):
                    r.add('be:replicas-one-dim-partial')
                if all(big) and any(part):
                    r.add('be:replicas-all-dims-partial')
                if d.fill == 'zero' and m.norm_term:
                    r.add('be:norm0')
                if len([kk for kk in range(len(m.bb)) if m.bb[kk, 0] == di]) > 1:
                    r.add('be:several-blocks')
            else:
                a0, i0 = row
                hw = T[2] * T[3]
                ni = min(int(A['_pad'][di]), R[1] - i0)
                nl = max(0, min(ni, E[1] - i0))
                live = a0 < E[0] and nl > 0
                r.add('br:live' if live else 'br:a0>=E0' if a0 >= E[0] else 'br:nl=0')
                if live and nl < ni:
                    r.add('br:nl<ni')
                if nl == 0 and i0 > 0:
                    r.add('br:nl=0-later-chunk')
                if live:
                    if reps[0] > 1 and a0 + E[0] < T[0]:
                        r.add('br:replicas-o')
                    if reps[1] > 1:
                        r.add('br:replicas-i')
                        for r0 in range(0, T[1], E[1]):
                            if r0 + i0 < T[1] and T[1] - r0 - i0 < nl:
                                r.add('br:partial-last-replica')
                    if (nl * hw) % 4:
                        r.add('br:n%4')
                    if nl * hw > 4096:
                        r.add('br:batch-loop-twice')
                vec = ni % 4 == 0 and S[2] % 4 == 0 and S[3] % 4 == 0 and (d.src_off + a0 * S[0] + i0) % 4 == 0
                r.add('br:store-vec' if vec else 'br:store-scalar')
                if to16:
                    r.add('h:row-vec' if vec else 'h:row-scalar')
                    if vec:
                        r.add('h:8-byte-aligned' if d.h_at % 4 == 0 else 'h:four-scalar-stores')
                if d.fill == 'zero' and m.norm_term:
                    r.add('br:norm0')
            if to16 and d.fill == 'big':
                r.add('h:big-tensor')
    return r


def other_regimes(c):
    m, f = c.meta, c.family
    r = set()
    if f == 'pnorm':
        r.add('pn:n_seg=%d' % m.n if m.n in (1, 5, 261) else 'pn:n_seg-other')
        in_chunk = {}
        for k, (s0, s1) in enumerate(m.seg):
            in_chunk[s0 // G.NORM_CHUNK] = in_chunk.get(s0 // G.NORM_CHUNK, 0) + int((s1 - 1) // G.NORM_CHUNK <= s0 // G.NORM_CHUNK)
            if s1 == s0:
                r.add('pn:empty')
                continue
            if s0 % 4:
                r.add('pn:start%4')
            if s1 % 4:
                r.add('pn:end%4')
            if s1 - s0 < 4:
                r.add('pn:shorter-than-4')
            b0, b1 = s0 // G.NORM_CHUNK, (s1 - 1) // G.NORM_CHUNK
            if b1 > b0:
                r.add('pn:straddles')
            if s1 % G.NORM_CHUNK == 0:
                r.add('pn:ends-on-boundary')
            if b1 - b0 + 1 > 64:
                r.add('pn:lane-stride-loop')
            if k and s0 // G.NORM_CHUNK > (m.seg[k - 1, 1] - 1) // G.NORM_CHUNK + 1:
                r.add('pn:gap>chunk')
            for b in range(b0, b1 + 1):
                c0, c1 = max(s0, b * G.NORM_CHUNK), min(s1, (b + 1) * G.NORM_CHUNK)
                a0, a1 = (c0 + 3) // 4 * 4, c1 // 4 * 4
                r.add('pn:interior' if a0 < a1 else 'pn:no-interior')
                if a0 < a1 and c0 < a0:
                    r.add('pn:head')
                if a0 < a1 and a1 < c1:
                    r.add('pn:tail')
            if not c.bufs[1][s0:s1].any():
                r.add('pn:zero-segment')
        if max(in_chunk.values()) >= 5:
            r.add('pn:five-in-a-chunk')
    elif f == 'pfin':
        r |= {'pf:blocks=%d' % n for n in m.counts if n in (0, 1, 63, 64, 65, 200)}
        r |= {'pf:bp%d' % m.bp, 'pf:n_seg>256' if m.n > 256 else 'pf:n_seg<=256'}
        ref = G.reference(c)
        if (ref['norms'][np.asarray(m.counts) > 0] == 0).any():
            r.add('pf:norm0')
    elif f == 'rfix':
        r |= {'rf:cols=%d' % m.cols, 'rf:K=%d' % m.K, 'rf:map%d' % int(m.q > 0), 'rf:bias%d' % m.bias,
              'rf:tau=' + ('0' if m.tau_rel == 0 else 'default' if m.tau_rel == 5e-3 else 'all' if m.tau_rel == 10.0 else 'fence')}
        assert m.ld > m.cols
        cand = G.rfix_candidates(c)
        if m.tau_rel == 10.0:
            assert cand.all()
            if m.cols >= 1024:
                r.add('rf:1024-list-entries')
        if m.tau_rel == 5e-3 and cand.any() and not cand.all():
            r.add('rf:some-candidates')
        if m.tau_rel == 0 or m.fence:
            assert np.isnan(c.bufs[2][:-G.SLACK]).all() and not cand.any()
        if m.fence:                                  # |x| == tau exactly, in float32 as in float64: `<` is strict
            x = c.bufs[0][:m.rows * m.ld].reshape(m.rows, m.ld)[:, :m.cols]
            assert (np.abs(x) == 0.5).all() and np.float32(m.tau_rel) * np.sqrt(np.float32((x * x).sum(1) / np.float32(min(m.cols, 1024)))).max() == 0.5
            r.add('rf:on-the-fence-exactly')
    elif f == 'rset':
        r |= {'rs:rows=%d' % s[0] for s in m.sets} | {'rs:n_sets=%d' % len(m.sets)}
        if m.I % 64:
            r.add('rs:I%64')
        for rows, o, i, ld, i0 in m.sets:
            if o == 1 and len(m.sets) == 1:
                r.add('rs:o=1-alone')
            if o < m.O:
                r.add('rs:o<O')
            if i0 % 64:
                r.add('rs:i0%64')
            if ld > o * i:
                r.add('rs:ld>o*i')
            nb = (i0 + i - 1) // 64 - i0 // 64 + 1
            r.add('rs:inside-one-block' if nb == 1 else 'rs:spans-%d-blocks' % nb)
            if (m.I + 63) // 64 > nb:
                r.add('rs:uniform-skip')
        cols = [set(range(s[4], s[4] + s[2])) for s in m.sets]
        if any(cols[a] & cols[b] for a in range(len(cols)) for b in range(a)):
            r.add('rs:overlap')
    elif f == 'add':
        r.add('add:n=%d' % m.n)
        if (m.n + 255) // 256 > 4096:
            r.add('add:grid-capped')
    return r


REQUIRED = {
    'tilef': {'f:sq0', 'f:sq1', 'f:bp0', 'f:bp1', 'f:lds>48K', 'fe:mode0', 'fe:mode1', 'fe:mode2', 'fe:wrap0-alone', 'fe:wrap1-alone',
              'fe:wrap2-alone', 'fe:wrap3-alone', 'fe:wrap-all', 'fe:numel<256', 'fe:numel%256', 'fe:numel%2048', 'fe:several-blocks',
              'fe:odo-carry', 'fe:start-top-digit', 'fe:stride0', 'fe:src_off', 'fe:scale', 'fe:buf0', 'fe:buf1', 'fe:buf2', 'fe:buf3',
              'fe:buf4', 'fr:hw4', 'fr:hw9', 'fr:hw49', 'fr:hw784', 'fr:vec', 'fr:scalar', 'fr:scalar-only-E1', 'fr:scalar-only-ni',
              'fr:scalar-only-S23', 'fr:scalar-only-base', 'fr:short-last-chunk', 'fr:T1<16', 'fr:a0%E0', 'fr:n%4', 'fr:row-start%4',
              'fr:scale', 'fr:norm0'},
    'tileb': {'b:src-dflat', 'b:src-norm', 'b:src-both', 'b:amax0-above', 'b:amax0-below', 'b:no-buf0', 'be:mode0', 'be:mode1', 'be:mode2',
              'be:R1=1', 'be:R1=3', 'be:R1=300', 'be:R0>E0', 'be:R1>E1', 'be:R2>E2', 'be:R3>E3', 'be:replicas-one-dim-partial',
              'be:replicas-all-dims-partial', 'be:norm0', 'be:several-blocks', 'br:live', 'br:a0>=E0', 'br:nl<ni', 'br:nl=0-later-chunk',
              'br:replicas-o', 'br:replicas-i', 'br:partial-last-replica', 'br:n%4', 'br:batch-loop-twice', 'br:store-vec',
              'br:store-scalar', 'br:norm0'},
    'tileb16': {'h:f16', 'h:bf16', 'h:16bit-elem', 'h:16bit-row', 'h:keeps-fp32-h-min-row', 'h:keeps-fp32-buf2-elem', 'h:row-vec',
                'h:row-scalar', 'h:8-byte-aligned', 'h:four-scalar-stores', 'h:big-tensor', 'br:live', 'br:a0>=E0', 'br:replicas-o'},
    'pnorm': {'pn:n_seg=1', 'pn:n_seg=5', 'pn:n_seg=261', 'pn:empty', 'pn:start%4', 'pn:end%4', 'pn:shorter-than-4', 'pn:straddles',
              'pn:ends-on-boundary', 'pn:lane-stride-loop', 'pn:gap>chunk', 'pn:interior', 'pn:no-interior', 'pn:head', 'pn:tail',
              'pn:zero-segment', 'pn:five-in-a-chunk'},
    'pfin': {'pf:blocks=0', 'pf:blocks=1', 'pf:blocks=63', 'pf:blocks=64', 'pf:blocks=65', 'pf:blocks=200', 'pf:bp0', 'pf:bp1', 'pf:norm0',
             'pf:n_seg>256', 'pf:n_seg<=256'},
    'rfix': {'rf:cols=5', 'rf:cols=1024', 'rf:cols=1030', 'rf:cols=2049', 'rf:K=4', 'rf:K=252', 'rf:K=260', 'rf:map0', 'rf:map1', 'rf:bias0',
             'rf:bias1', 'rf:tau=0', 'rf:tau=default', 'rf:tau=all', 'rf:1024-list-entries', 'rf:some-candidates', 'rf:on-the-fence-exactly'},
    'rset': {'rs:rows=1', 'rs:rows=3', 'rs:rows=33', 'rs:rows=70', 'rs:n_sets=1', 'rs:n_sets=4', 'rs:I%64', 'rs:o=1-alone', 'rs:o<O', 'rs:i0%64',
             'rs:ld>o*i', 'rs:inside-one-block', 'rs:spans-3-blocks', 'rs:uniform-skip', 'rs:overlap'},
    'add': {'add:n=1', 'add:n=255', 'add:n=%d' % (4096 * 256 + 5), 'add:grid-capped'},
}


def regimes(c):
    return tile_regimes(c) if c.family.startswith('tile') else other_regimes(c)


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


def test_the_16_bit_cases_keep_the_promises_of_the_host_table():
    for c in G.cases('tileb16'):
        for d in c.meta.descs:
            if d.h is not None:
                assert d.h[1] % 4 == 0 and d.h[2] != d.h[3] and d.buf == 0 and d.mode == 0
        assert any(d.h is None and d.buf == 0 for d in c.meta.descs) and any(d.buf == 2 for d in c.meta.descs)
        big = [k for k, d in enumerate(c.meta.descs) if d.fill == 'big']
        assert len(big) == 1 and int(np.argmax(G.reference(c)['ratio'])) == c.meta.descs[big[0]].seg, 'the 1e4 x tensor decides the bound'


def test_names_are_unique_and_cases_stay_small():
    names = [c.name for c in ALL]
    assert len(names) == len(set(names))
    for c in ALL:
        n = sum(b.size for b in c.bufs)
        assert n < 200_000 or c.name in ('pnorm-600k', 'add-n%d' % (4096 * 256 + 5)), (c.name, n)
