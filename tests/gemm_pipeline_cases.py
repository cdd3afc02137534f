"""Adversarial op-level cases for the 16-bit GEMM pipeline (ghn3_amd/csrc/gemm.hip, gemm_p8.hip, gemm_small.hip and the operand
copies of GHN3_OP_CAST16 in elementwise.hip) -- the features of the training step that tests/gemm_cases.py never sets:
power-of-two scaled operand copies with `alpha_amax`, per-128-row `lim` tables of both kinds, GHN3_GEMM_SUMSQ slot tables and
the GHN3_OP_SUMSQ forms that consume them, the fp32 kernels' b_gather / a_q / bias_q / split-K fields and the cast variants
(COLSUM_PARTS, TIGHT, source column map, SCALED | COLSUM, grid cap, descriptor search, both straight paths, special values).

Same layout as tests/graphormer_op_cases.py and tests/decoder_tail_cases.py, whose plumbing is imported: a case is a list of
`ghn3_op` records (CAST16, GEMM, SUMSQ) plus a problem table over numpy buffers.  Every output and every 16-bit destination is
pre-filled with a sentinel: NaN bit patterns, 0.25 where the op accumulates; only what include/ghn3_hip.h makes the caller's
duty is zeroed (C of a split-K problem, B rows behind what the cast writes when a k-map reads there, a slot table that
GHN3_OP_SUMSQ adds).  Source padding holds NaN (cast sources) or 1e4 (fp32 GEMM operands).

Shared by tests/test_gemm_pipeline_cases_cpu.py (the float64 interpreter against `reference`, regime coverage, floors and caps)
and tests/test_gpu_gemm_pipeline_ops.py (`ctx.run` against `reference`).  No GPU is touched here.

`reference(case, float64)` shares no code with tests/program_interp.py and does not read the op records: every case keeps
its logical matrices and the places where its results must appear (`case.outs`: buffer, element indices, expected values).
Operands are rounded on the CPU as cast_f16 / cast_bf16 round (round-to-nearest-even, f16 saturating at +-65504), products
and sums are float64.  `reference(case, float32)` is the op's formula in numpy float32 with the reduction accumulated
sequentially in 64-wide k-tiles: the float32 floor of the case (`floors`).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

from ghn3_amd import _lib as L
from graphormer_op_cases import NAN, SENT, FWD_CAP, FLOOR_FACTOR, MIN_BOUND, make_op, host_bytes, _seed, blocked  # noqa: F401
from util_parity import slice_errors

SLACK = 16
NAN16 = {False: 0x7e00, True: 0x7fc0}                 # a NaN of f16 / of bf16
POISON = np.float32(1e4)                              # padding of fp32 GEMM operands
XCD_B_BYTES = 5 << 19
# rows x columns of a tile per tile code (0 = auto: the shapes of this table are too small for anything but 128 x 128)
TILE_GEO = {0: (128, 128), 16: (128, 128), 20: (256, 128), 24: (256, 256), 25: (256, 256), 28: (256, 256), 29: (256, 256),
            30: (256, 128)}
MAX_CASES = 72
# f16 operand copies that hold SUBNORMAL codes (scale <= 1 on ~1e-7 sources: amax 0, 1e-35, 1e4).  The matrix cores align the
# products of one MFMA at their nominal exponents, and a subnormal f16 carries exponent 2^-14 whatever the leading zeros of its
# 10 fraction bits: up to 10 bits of the window hold zeros instead of data.  One product is still exact (K = 1: equal bits); from
# two terms per MFMA on the sums sit on a grid of 2^-39 at results of ~1e-7 (measured: errors of 1, 3 x 2^-39 at K = 2; every
# 16-bit-operand kernel alike -- tile codes 16, 20, 24, 25, 29, 30 -- and gone with the same data scaled by 2^14 or in bf16).
# The K = 1 cases scaled-t24-f16-zero-K1 / scaled-t30-f16-zero-K1-alpha pin the exact single product, the f16 cases with a
# pow2 / below-pow2 amax on the same tile codes the factor-8 bound on normal copies of the same kind of data.
# That is the reason GHN3_CAST_SCALED exists; with a scale <= 1 the kernels cannot do better.  Their bound: the factor 8 times
# 2^10 for the 10 bits, which the cap of 2e-5 cuts for every case of today.  Measured ratio to the float32 floor (MI355X):
# scaled-t20-f16-zero 190, -t24-f16-1e-35 242, -t25-f16-1e4 834, -t29-f16-zero 150, -t30-f16-1e-35 147 (1.0e-5 .. 1.95e-5).
SUBNORMAL_F16_FACTOR = 2.0 ** 10

r64 = lambda v: (v + 63) // 64 * 64
r8 = lambda v: (v + 7) // 8 * 8
pad4 = lambda v: (v + 3) // 4 * 4


# ---- number formats -------------------------------------------------------------------------------------------------------------
def to16(x, bf):
    """float32 -> 16-bit codes as cast_f16 / cast_bf16 (elementwise.hip): nearest even; f16 saturates at +-65504."""
    x = np.ascontiguousarray(x, np.float32)
    if not bf:
        with np.errstate(invalid='ignore', over='ignore'):
            sat = np.where(np.abs(x) > np.float32(65504.0), np.copysign(np.float32(65504.0), x), x)
            return sat.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    up, low = u >> 16, u & 0xffff
    inc = (low > 0x8000) | ((low == 0x8000) & ((up & 1) == 1))
    return (up + inc).astype(np.uint16)


def back16(h, bf):
    h = np.ascontiguousarray(h, np.uint16)
    if not bf:
        return h.view(np.float16).astype(np.float32)
    return (h.astype(np.uint32) << 16).view(np.float32)


def pow2_scale(amax):
    """ghn3_pow2_scale (ghn3_internal.h): 2^(11 - e) for amax = m 2^e, 1 <= m < 2; 1 for amax <= 0 or e < -100."""
    amax = float(np.float32(amax))
    if not amax > 0:
        return 1.0
    e = math.frexp(amax)[1] - 1
    return 1.0 if e < -100 else math.ldexp(1.0, 11 - e)


AMAX = {'pow2': np.float32(2.0 ** -21), 'below-pow2': np.nextafter(np.float32(2.0 ** -21), np.float32(0)), 'zero': np.float32(0),
        '1e-35': np.float32(1e-35), '1e4': np.float32(1e4)}


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
def new_problem(**kw):
    p = np.zeros(1, dtype=L.PROBLEM_DT)
    for n in L._REF_NAMES + ('lim', 'alpha_amax', 'B2', 'mtiles'):
        p[n]['buf'] = -1
    p['ln_p']['buf'] = -1
    p['alpha'], p['ksplit'] = 1.0, 1
    for k, v in kw.items():
        if p.dtype[k] == L.REF_DT:
            p[k]['buf'], p[k]['off'] = v if isinstance(v, tuple) else (v, 0)
        else:
            p[k] = v
    return p


class Pipe:
    def __init__(self, family, name, regimes=()):
        self.family, self.name, self.regimes = family, name, set(regimes)
        self.bufs, self.ops, self.probs, self.outs, self.free = [], [], [], [], []

    def add(self, arr):
        self.bufs.append(np.ascontiguousarray(arr))
        return len(self.bufs) - 1

    def out(self, name, buf, idx, ref, kind, valid=None, rerun=True, post=None):
        """idx: element indices (in elements of the buffer's dtype) where the result appears; ref(dtype) -> expected values
        (codes for kind 'bits'); valid: mask of what is compared; post: reduction applied to the gathered values."""
        self.outs.append(SimpleNamespace(name=name, buf=buf, idx=np.asarray(idx, np.int64), ref=ref, kind=kind, valid=valid,
                                         rerun=rerun, post=post))

    def dontcare(self, buf, idx):
        self.free.append((buf, np.asarray(idx, np.int64).reshape(-1)))

    def problem(self, **kw):
        self.probs.append(new_problem(**kw))
        return len(self.probs) - 1

    def op(self, kind, refs, i=(), f=(), flags=0):
        o = make_op(kind, refs, i, f)
        o['flags'] = flags
        self.ops.append(o)

    def done(self, **meta):
        probs = np.concatenate(self.probs) if self.probs else np.zeros(0, dtype=L.PROBLEM_DT)
        return SimpleNamespace(family=self.family, name=self.name, ops=np.concatenate(self.ops), problems=probs, bufs=self.bufs,
                               outs=self.outs, free=self.free, regimes=self.regimes, meta=SimpleNamespace(**meta))


def run_interp(case):
    """The case through the float64 interpreter on host copies -> the buffers as byte arrays."""
    from program_interp import Interp
    host = host_bytes(case)
    Interp(host).run(case.ops, case.problems)
    return host


def _typed(case, bufs, k):
    return bufs[k].reshape(-1).view(np.uint8).view(case.bufs[k].dtype)


def extract_raw(case, bufs):
    return {o.name: _typed(case, bufs, o.buf)[o.idx] for o in case.outs}


def extract(case, bufs):
    """name -> the case's results in `bufs` (byte arrays as run_interp returns them, device copies, or the case's own)."""
    raw = extract_raw(case, bufs)
    return {o.name: (o.post(raw[o.name]) if o.post else raw[o.name]) for o in case.outs}


def written(case):
    """buffer -> boolean mask over its elements of what the case's ops may write; everything else keeps its bits"""
    w = {k: np.zeros(b.size, bool) for k, b in enumerate(case.bufs)}
    for o in case.outs:
        w[o.buf][o.idx.reshape(-1)] = True
    for k, idx in case.free:
        w[k][idx] = True
    return w


# ---- the GEMM formula -------------------------------------------------------------------------------------------------------------
def matmul_t(A, B, dt):
    """A [M][K] times B[N][K]^T with products and sums in dt; float32: sequentially over 64-wide k-tiles"""
    if dt == np.float64:
        return A.astype(np.float64) @ B.astype(np.float64).T
    acc = np.zeros((A.shape[0], B.shape[0]), np.float32)
    for k0 in range(0, A.shape[1], 64):
        acc = acc + A[:, k0:k0 + 64].astype(np.float32) @ B[:, k0:k0 + 64].astype(np.float32).T
    return acc


def tile_views(a):
    """per 32 x 32 output tile and per row"""
    if a.ndim == 2:
        return [(blocked(blocked(a, 1, 32), 0, 32), [(0, 2)]), (a, [(0,)])]
    return [(a.reshape(-1), [(0,)])]


def persistent_ids(M, N, K, bn):
    """tile ids of a tile code 29 / 30 problem that comes first in its launch: (row tile, column tile) -> id, ids in all.  The
    runtime numbers them XCD-blocked (workgroup b runs on XCD b % 8): the columns are cut into G groups -- G doubles while a
    group's share of B exceeds the per-XCD budget and there are two column tiles per group left -- XCD x takes column group
    x % G and every (8 / G)-th row tile from x / G, and walks the column tiles of its group for one row tile, then the next."""
    tm, tn = (M + 255) // 256, (N + bn - 1) // bn
    G = 1
    while G < 8 and N * K * 2 // G > XCD_B_BYTES and tn >= 2 * G:
        G *= 2
    per_group, stride = -(-tn // G), 8 // G
    ids = {}
    for mt in range(tm):
        for nt in range(tn):
            xcd = (mt % stride) * G + nt // per_group
            step = (mt // stride) * per_group + nt % per_group
            ids[(mt, nt)] = 8 * step + xcd
    return ids, 8 * per_group * -(-tm // stride)


# ---- CAST16 + GHN3_GEMM_OP16 ------------------------------------------------------------------------------------------------------
# buffers: 0 fp32 sources 1 16-bit copies 2 descriptors 3 amax 4 C 5 lim / mtiles 6 slot table
#          (chain) 7 C of the second launch 8 its zeroed slot table 9 sum 10 x 11 scratch
def op16_case(family, name, M, N, K, bf, tile, regimes=(), amax=None, share=False, alpha=1.0, lim=None, lim_kind=0, mtiles=None,
              kmap=None, ksplit=1, grid_cap=0, cmap=None, sumsq=False, accum=False, chain=False):
    rs = np.random.RandomState(_seed((family, name)))
    P = Pipe(family, name, regimes)
    scaled = amax is not None
    sc = pow2_scale(amax) if scaled else 1.0
    A = (rs.standard_normal((M, K)) * (1e-7 if scaled else 1.0)).astype(np.float32)
    A[::7, ::5] = 0.0
    ext_row = None
    if lim is not None:
        assert len(lim) == (M + 127) // 128 and all(a > b for a, b in zip(lim, lim[1:]))
        ext_row = np.repeat(np.asarray(lim), 128)[:M]
        if lim_kind == 2:
            A[np.arange(K)[None, :] >= ext_row[:, None]] = 0.0
    kq, ks = kmap or (0, 0)
    Kp = ((K + kq - 1) // kq) * ks if kmap else K
    kk = np.arange(K)
    kphys = (kk // kq) * ks + kk % kq if kmap else kk
    Bp = (rs.standard_normal((N, Kp)) * (1e-7 if share else 1.0)).astype(np.float32)
    # fp32 sources, NaN in the padding of every row
    ld_sa, ld_sb = pad4(K) + 4, pad4(Kp) + 8
    SA, SB = np.full((M, ld_sa), NAN, np.float32), np.full((N, ld_sb), NAN, np.float32)
    SA[:, :K], SB[:, :Kp] = A, Bp
    b_src = P.add(np.concatenate([SA.reshape(-1), SB.reshape(-1), np.full(SLACK, NAN, np.float32)]))
    # 16-bit copies
    lda = r64(K) + 8
    ldb = r64(Kp) + (64 + 8 if kmap else 8)
    offB = r64(M * lda) + 64
    d16 = np.full(offB + N * ldb + 64, NAN16[bf], np.uint16)
    if kmap:                                             # the k-map reads behind what the cast writes: the caller's zeros
        kpad = np.arange(r64(K))
        assert int(((kpad // kq) * ks + kpad % kq).max()) < ldb
        d16[offB:offB + N * ldb].reshape(N, ldb)[:, r64(Kp):] = 0
    b_16 = P.add(d16)
    descs = np.zeros(2, dtype=L.CAST_DT)
    st = L.CAST_STRAIGHT | (L.CAST_STRAIGHT_BF16 if bf else 0)
    descs[0]['src_off'], descs[0]['rows'], descs[0]['cols'], descs[0]['ld_src'] = 0, M, K, ld_sa
    descs[0]['dst_off'], descs[0]['ld_dst'], descs[0]['flags'] = 0, lda, st | (L.CAST_SCALED if scaled else 0)
    descs[1]['src_off'], descs[1]['rows'], descs[1]['cols'], descs[1]['ld_src'] = SA.size, N, Kp, ld_sb
    descs[1]['dst_off'], descs[1]['ld_dst'], descs[1]['flags'] = offB, ldb, st | (L.CAST_SCALED if share else 0)
    descs[1]['block_start'] = ((M + 63) // 64) * ((K + 63) // 64)
    blocks = int(descs[1]['block_start']) + ((N + 63) // 64) * ((Kp + 63) // 64)
    b_desc = P.add(descs.view(np.uint8).reshape(-1))
    b_amax = P.add(np.asarray([amax if scaled else NAN, NAN, NAN, NAN], np.float32))
    P.op(L.OP_CAST16, [b_src, b_16, b_desc, None, b_amax if scaled else None], (2, blocks))
    A16 = np.zeros((M, r64(K)), np.uint16)
    A16[:, :K] = to16(A * np.float32(sc), bf)
    B16 = np.zeros((N, r64(Kp)), np.uint16)
    B16[:, :Kp] = to16(Bp * np.float32(sc if share else 1.0), bf)
    P.out('A16', b_16, np.arange(M)[:, None] * lda + np.arange(r64(K))[None, :], lambda dt: A16, 'bits')
    P.out('B16', b_16, offB + np.arange(N)[:, None] * ldb + np.arange(r64(Kp))[None, :], lambda dt: B16, 'bits')
    # C
    ldc = pad4(N) + 4
    cq, cs = cmap or (0, 0)
    m = np.arange(M)
    c_idx = (m // cq) * cs + m % cq if cmap else m
    c_rows = int(c_idx.max()) + 2
    ci = c_idx[:, None] * ldc + np.arange(N)[None, :]
    init = SENT if accum else np.float32(0) if ksplit > 1 else None

    def new_c():
        C0 = np.full(c_rows * ldc + SLACK, NAN, np.float32)
        if init is not None:
            C0[ci] = init
        return C0
    b_c = P.add(new_c())
    b_lim = None
    if lim is not None:
        b_lim = P.add(np.asarray(list(lim) + [1 << 30] * 2, np.int32))
    if mtiles is not None:
        b_lim = P.add(np.asarray([(m_[0], m_[1], 1 << 30) for m_ in mtiles], np.int32).reshape(-1))
    bm, bn = TILE_GEO[tile]
    ids, n_ids = persistent_ids(M, N, K, bn) if sumsq else ({}, 0)
    b_slots = P.add(np.full(8 * n_ids + 24, NAN, np.float32)) if sumsq else None
    Ad, Bd = back16(A16[:, :K], bf), back16(B16[:, :Kp], bf)[:, kphys]
    al32 = np.float32(alpha) * np.float32(1.0 / sc if scaled else 1.0)          # (a power of two: exact unless it leaves the range)

    def c_ref(dt):
        v = matmul_t(Ad, Bd, dt) * dt(al32)
        if init is not None:
            v = v + dt(init)
        return v.astype(np.float32)

    def problem(c_buf, slots_buf):
        kw = dict(A=(b_16, 0), B=(b_16, 2 * offB), C=c_buf, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, c_q=cq, c_s=cs,
                  flags=L.GEMM_OP16 | (L.GEMM_ACCUM if accum else 0) | (L.GEMM_SUMSQ if sumsq else 0), alpha=alpha, ksplit=ksplit,
                  b_kq=kq, b_ks=ks, bias_stride=1)
        if scaled:
            kw['alpha_amax'] = b_amax
        if lim is not None:
            kw['lim'], kw['lim_kind'] = b_lim, lim_kind
        if mtiles is not None:
            kw['mtiles'], kw['n_mtiles'] = b_lim, len(mtiles)
        if sumsq:
            kw['aux_out'] = slots_buf
        return P.problem(**kw)

    def outputs(tag, c_buf, slots_buf, id0=0):
        valid = None
        if lim_kind == 1:
            valid = np.arange(N)[None, :] < ext_row[:, None]
            # a tile whose first column lies beyond the extents of all its rows is skipped; the others are written full width
            t_ext = np.asarray([max(lim[(m0 >> 7):(m0 >> 7) + (2 if (bm > 128 and m0 + 128 < M) else 1)]) for m0 in range(0, M, bm)])
            wcols = np.minimum(N, (np.repeat(t_ext, bm)[:M] + bn - 1) // bn * bn)
            free = (np.arange(N)[None, :] < wcols[:, None]) & ~valid
            P.dontcare(c_buf, ci[free])
        P.out('C' + tag, c_buf, ci, c_ref, 'float', valid=valid, rerun=ksplit <= 1)
        if sumsq:
            keys = sorted(ids)
            sidx = np.asarray([[8 * (id0 + ids[k_]) + w for w in range(8)] for k_ in keys])

            def sq_ref(dt):
                c = c_ref(np.float64).astype(dt)
                return np.asarray([(c[mt * 256:(mt + 1) * 256, nt * bn:(nt + 1) * bn] ** 2).sum(dtype=dt) for mt, nt in keys]).astype(np.float32)
            P.out('sq' + tag, slots_buf, sidx, sq_ref, 'entries', post=lambda a: a.astype(np.float64).sum(-1).astype(np.float32))

    q0 = problem(b_c, b_slots)
    ct = L.CT_BF16 if bf else L.CT_F16
    n_extra = 8 * n_ids
    if chain:
        # the same product into a second plane with a ZEROED slot table (the header's contract), then GHN3_OP_SUMSQ over a
        # buffer whose range [i1, i2) holds 1e30 -- read, the sum would be infinite -- with the slots added in its place.
        # chain 'op': a launch of its own.  chain 'problem': the second problem of the SAME launch, whose tile ids -- and so
        # its slots, in its own table -- continue behind those of the first problem.
        assert sumsq and chain in ('op', 'problem')
        id0 = n_ids if chain == 'problem' else 0
        n_extra = 8 * (id0 + n_ids)
        b_c1 = P.add(new_c())
        b_s1 = P.add(np.concatenate([np.zeros(n_extra, np.float32), np.full(24, NAN, np.float32)]))
        q1 = problem(b_c1, b_s1)
    P.op(L.OP_GEMM, [], (q0, 2 if chain == 'problem' else 1, tile, grid_cap), flags=1 + ct)
    outputs('', b_c, b_slots)
    if chain:
        if chain == 'op':
            P.op(L.OP_GEMM, [], (q1, 1, tile, grid_cap), flags=1 + ct)
        outputs('1', b_c1, b_s1, id0)
        n, i1, i2 = 5003, 1000, 3048
        x = rs.standard_normal(n + SLACK).astype(np.float32)
        x[i1:i2] = np.float32(1e30)
        x[n:] = NAN
        b_sum, b_x, b_scr = P.add(np.asarray([SENT, NAN, NAN, NAN], np.float32)), P.add(x), P.add(np.full(8192 + SLACK, NAN, np.float32))
        P.op(L.OP_SUMSQ, [b_sum, b_x, b_scr, b_s1], (n, i1, i2, n_extra))
        P.dontcare(b_scr, np.arange(8192))

        def sum_ref(dt):
            keep = np.concatenate([x[:i1], x[i2:n]]).astype(dt)
            slots = out_of_list(P.outs, 'sq1').ref(dt).astype(dt)                 # (the float32 slots as stored)
            return np.asarray([dt(SENT) + (keep * keep).sum(dtype=dt) + slots.sum(dtype=dt)], np.float32)
        P.out('sumsq', b_sum, [0], sum_ref, 'entries')
    # (a stray subnormal among normal codes does not count: most of the nonzero codes of an operand are subnormal)
    frac = lambda H: float((((H & 0x7c00) == 0) & ((H & 0x3ff) != 0)).sum()) / max(1, int(((H & 0x7fff) != 0).sum()))
    subn = (not bf) and max(frac(A16), frac(B16)) > 0.5
    return P.done(M=M, N=N, K=K, bf=bf, tile=tile, ksplit=ksplit, sc=sc, ids=ids, n_ids=n_ids, bn=bn, b_slots=b_slots, b_c=b_c,
                  f16_subnormal=subn)


def _scaled_cases():
    out = []
    shapes = {0: (130, 129), 16: (130, 132), 20: (260, 132), 24: (260, 260), 25: (260, 260), 28: (260, 260), '28m': (330, 260),
              29: (260, 264), 30: (260, 132)}
    Ks = (200, 1, 2, 64 * 7 + 8)                        # a few k-tiles and a tail, 1, 2, and one ring wrap-around per kernel
    kinds = list(AMAX)
    n = 0
    for bf in (False, True):
        for t, (M, N) in shapes.items():
            tile = 28 if t == '28m' else t
            kind = kinds[n % 5]
            K = Ks[3] if not bf else Ks[n % 3]
            share, alpha = n % 4 == 1, (-0.375 if n % 3 == 2 else 1.0)
            reg = {'scaled:tile%s' % t, 'scaled:%s' % ('bf16' if bf else 'f16'), 'scaled:amax-' + kind}
            reg |= {'scaled:shared-slot'} if share else set()
            reg |= {'scaled:alpha'} if alpha != 1.0 else set()
            reg |= {'scaled:ring-wrap-tile%s' % tile} if K > 400 else set()
            out.append(op16_case('scaled', 'scaled-t%s-%s-%s-K%d%s%s' % (t, 'bf16' if bf else 'f16', kind, K, '-shared' if share else '',
                                                                        '-alpha' if alpha != 1.0 else ''),
                                 M, N, K, bf, tile, reg, amax=AMAX[kind], share=share, alpha=alpha,
                                 mtiles=[(0, 6), (192, 6)] if t == '28m' else None))
            n += 1
    # every tile code, and so every one of the six places where the inverse scale is applied, also with a scale that is not 1
    # in f16 (the rotation above leaves tile codes 20, 24, 25, 29, 30 with subnormal f16 copies), at the factor-8 bound; tile
    # code 24 with K = 1; and one product per output from SUBNORMAL copies, which the matrix cores form exactly (K = 1)
    for t, kind, K, alpha in ((20, 'below-pow2', 200, 1.0), (24, 'pow2', 1, 1.0), (25, 'below-pow2', 2, 1.0), (29, 'pow2', 200, 1.0),
                              (30, 'below-pow2', 200, -0.375), (24, 'zero', 1, 1.0), (30, 'zero', 1, -0.375)):
        M, N = shapes[t]
        reg = {'scaled:tile%s' % t, 'scaled:f16', 'scaled:amax-' + kind} | ({'scaled:alpha'} if alpha != 1.0 else set())
        reg |= {'scaled:subnormal-K1'} if (kind == 'zero' and K == 1) else set()
        out.append(op16_case('scaled', 'scaled-t%s-f16-%s-K%d%s' % (t, kind, K, '-alpha' if alpha != 1.0 else ''), M, N, K, False, t, reg,
                             amax=AMAX[kind], alpha=alpha))
    return out


def _lim_cases():
    out = []
    n = 0
    for kind in (1, 2):
        for tile in (0, 16, 20, 24, 28):
            bm, bn = TILE_GEO[tile]
            bf = n % 2 == 1
            reg = {'lim:kind%d-tile%d' % (kind, tile)} | ({'lim:two-entries'} if bm == 256 else set())
            if kind == 1:
                # extents of the five 128-row blocks: one past a column-tile edge, exactly on it, on the next one, one short, < 64
                lim = [2 * bn + 1, 2 * bn, bn, bn - 1, 40] if n % 2 == 0 else [2 * bn, bn + 1, bn - 1, 40]
                M = 128 * (len(lim) - 1) + 5
                out.append(op16_case('lim', 'lim1-t%d-%s' % (tile, 'bf16' if bf else 'f16'), M, 2 * bn + 8, 200, bf, tile, reg,
                                     lim=lim, lim_kind=1))
            else:
                # reduction extents: one past a k-tile edge, on it, one short of the one below, < 64; with the k-map of B,
                # split-K (not on tile 28, which takes none) and alpha_amax, as the dgrad of the decoder
                lim = [193, 192, 127, 40] if n % 2 == 0 else [200, 129, 128, 64, 33]
                M = 128 * (len(lim) - 1) + 5
                ksplit = 1 if tile == 28 else 2 + n % 2
                reg |= {'lim:kind2-kmap', 'lim:kind2-amax'} | ({'lim:kind2-ksplit'} if ksplit > 1 else set())
                out.append(op16_case('lim', 'lim2-t%d-%s-ks%d' % (tile, 'bf16' if bf else 'f16', ksplit), M, 136, 200, bf, tile, reg,
                                     lim=lim, lim_kind=2, kmap=(64, 96) if tile == 28 else (40, 56), ksplit=ksplit,
                                     amax=AMAX['below-pow2']))
            n += 1
    return out


def _sumsq_gemm_cases():
    R = lambda *names: {'sumsq:' + n_ for n_ in names}
    return [
        op16_case('sqgemm', 'sq-t29-ragged', 260, 264, 200, False, 29, R('tile29', 'ragged', 'op-range'), sumsq=True, chain='op'),
        op16_case('sqgemm', 'sq-t29-cmap-cap', 520, 260, 72, True, 29, R('tile29', 'cmap', 'grid-cap', 'tiles-per-wg'), sumsq=True,
                  cmap=(100, 130), grid_cap=8 | (1 << 16), amax=AMAX['pow2']),
        op16_case('sqgemm', 'sq-t30-ragged', 260, 132, 200, True, 30, R('tile30', 'ragged', 'op-range', 'two-problems'), sumsq=True, chain='problem'),
        # 8 workgroups walk 16 ids, 6 of them tiles: a tile's C and slots leave during the workgroup's next tile
        # B above the per-XCD budget: two column groups in the tile order (the ids of the slots follow it)
        op16_case('sqgemm', 'sq-t29-xcd-groups', 520, 1304, 1024, True, 29, R('tile29', 'xcd-groups'), sumsq=True),
        op16_case('sqgemm', 'sq-t29-walk', 520, 260, 200, False, 29, R('tile29', 'grid-cap', 'walk'), sumsq=True, grid_cap=8,
                  amax=AMAX['below-pow2']),
        op16_case('sqgemm', 'sq-t30-cmap-cap', 520, 260, 72, False, 30, R('tile30', 'cmap', 'grid-cap'), sumsq=True, cmap=(100, 130),
                  grid_cap=8),
    ]


# ---- GHN3_OP_SUMSQ alone ----------------------------------------------------------------------------------------------------------
def sumsq_case(name, n, scratch):
    rs = np.random.RandomState(_seed(('sumsq', name)))
    P = Pipe('sumsq', name, {'sumsq:plain-scratch' if scratch else 'sumsq:plain-atomic'})
    x = rs.standard_normal(n + SLACK).astype(np.float32)
    x[n:] = NAN
    b_sum, b_x = P.add(np.asarray([SENT, NAN, NAN, NAN], np.float32)), P.add(x)
    b_scr = P.add(np.full(4096 + SLACK, NAN, np.float32)) if scratch else None
    P.op(L.OP_SUMSQ, [b_sum, b_x, b_scr], (n,))
    if scratch:
        P.dontcare(b_scr, np.arange(4096))
    xs = x[:n]
    P.out('sumsq', b_sum, [0], lambda dt: np.asarray([dt(SENT) + (xs.astype(dt) ** 2).sum(dtype=dt)], np.float32), 'entries',
          rerun=scratch)
    return P.done(n=n)


def _sumsq_cases():
    return [sumsq_case('sumsq-atomic-n1027', 1027, False), sumsq_case('sumsq-scratch-n1027', 1027, True),
            sumsq_case('sumsq-scratch-n3', 3, True), sumsq_case('sumsq-scratch-n70001', 70001, True)]


# ---- fp32 kernels -----------------------------------------------------------------------------------------------------------------
# buffers: 0 XA 1 XB 2 C 3 bias 4 a_gather 5 b_gather 6 c_gather
def f32_case(name, M, N, K, a_mode, b_mode, tile, regimes, gather=False, a_qs=None, bias=None, ksplit=1, accum=False):
    rs = np.random.RandomState(_seed(('f32', name)))
    P = Pipe('f32', name, regimes)
    a_rows, a_cols = (M, K) if a_mode == L.MODE_ROW else (K, M)
    b_rows, b_cols = (N, K) if b_mode == L.MODE_ROW else (K, N)
    extra = 5 if gather else 0
    aq, as_ = a_qs or (0, 0)
    ga = rs.permutation(a_rows + extra)[:a_rows].astype(np.int32) if gather else None
    gb = rs.permutation(b_rows + extra)[:b_rows].astype(np.int32) if gather else None
    gc = rs.permutation(M + extra)[:M].astype(np.int32) if gather else None
    ra = ga.astype(np.int64) if gather else np.arange(a_rows)
    if aq:
        ra = (ra // aq) * as_ + ra % aq
    rb = gb.astype(np.int64) if gather else np.arange(b_rows)
    rc = gc.astype(np.int64) if gather else np.arange(M)
    lda, ldb, ldc = pad4(a_cols) + 4, pad4(b_cols) + 8, pad4(N) + 4
    XA = np.full((int(ra.max()) + 1 + extra, lda), POISON, np.float32)
    XB = np.full((int(rb.max()) + 1 + extra, ldb), POISON, np.float32)
    XA[:, :a_cols] = rs.standard_normal((XA.shape[0], a_cols))
    XB[:, :b_cols] = rs.standard_normal((XB.shape[0], b_cols))
    Al = XA[ra][:, :a_cols]
    Al = Al if a_mode == L.MODE_ROW else Al.T                     # [M][K]
    Bl = XB[rb][:, :b_cols]
    Bl = Bl if b_mode == L.MODE_ROW else Bl.T                     # [N][K]
    ci = rc[:, None] * ldc + np.arange(N)[None, :]
    init = SENT if accum else np.float32(0) if ksplit > 1 else None
    C0 = np.full((M + extra + 1) * ldc + SLACK, NAN, np.float32)
    if init is not None:
        C0[ci] = init
    bvec = bidx = None
    bq, bs, bstride = bias or (0, 0, 1)
    if bias:
        nn = np.arange(N)
        bidx = ((nn // bq) * bs + nn % bq) * bstride
        bvec = rs.standard_normal(int(bidx.max()) + 1 + SLACK).astype(np.float32)
    bufs = [P.add(XA.reshape(-1)), P.add(XB.reshape(-1)), P.add(C0), P.add(bvec if bias else np.zeros(4, np.float32))]
    for g in (ga, gb, gc):
        bufs.append(P.add(g if gather else np.zeros(4, np.int32)))
    kw = dict(A=0, B=1, C=2, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, a_mode=a_mode, b_mode=b_mode, a_q=aq, a_s=as_,
              flags=L.GEMM_ACCUM if accum else 0, alpha=0.75, ksplit=ksplit, bias_stride=bstride, bias_q=bq, bias_s=bs)
    if gather:
        kw.update(a_gather=4, b_gather=5, c_gather=6)
    if bias:
        kw['bias'] = 3
    q = P.problem(**kw)
    P.op(L.OP_GEMM, [], (q, 1, tile), flags=1 + L.CT_F32)

    def c_ref(dt):
        v = matmul_t(Al, Bl, dt) * dt(0.75)
        if bias:
            v = v + bvec[bidx].astype(dt)[None, :]
        if init is not None:
            v = v + dt(init)
        return v.astype(np.float32)
    P.out('C', 2, ci, c_ref, 'float', rerun=ksplit <= 1)
    return P.done(M=M, N=N, K=K, tile=tile, ksplit=ksplit)


def _f32_cases():
    ROW, COL = L.MODE_ROW, L.MODE_COL
    return [
        f32_case('f32-gathers-colcol-t0', 70, 50, 37, COL, COL, 0, {'f32:b_gather'}, gather=True, accum=True),
        f32_case('f32-gathers-colcol-t64', 70, 133, 200, COL, COL, 64, {'f32:b_gather'}, gather=True, accum=True),
        f32_case('f32-aqs-t64', 130, 70, 200, ROW, ROW, 64, {'f32:a_qs'}, a_qs=(40, 56)),
        f32_case('f32-aqs-t0', 33, 65, 19, ROW, COL, 0, {'f32:a_qs'}, a_qs=(8, 9)),
        f32_case('f32-biasqs-t128', 130, 136, 72, ROW, ROW, 128, {'f32:bias_qs'}, bias=(24, 40, 3)),
        f32_case('f32-biasqs-t64', 65, 70, 1, ROW, COL, 64, {'f32:bias_qs'}, bias=(7, 9, 2)),
        f32_case('f32-ksplit2-t64', 130, 70, 200, ROW, ROW, 64, {'f32:ksplit2-t64'}, ksplit=2),
        f32_case('f32-ksplit3-t64', 65, 129, 456, COL, ROW, 64, {'f32:ksplit3-t64'}, ksplit=3),
        f32_case('f32-ksplit2-t128', 130, 136, 456, ROW, COL, 128, {'f32:ksplit2-t128'}, ksplit=2),
        f32_case('f32-ksplit3-t128', 260, 129, 200, ROW, ROW, 128, {'f32:ksplit3-t128'}, ksplit=3),
    ]


# ---- cast variants ------------------------------------------------------------------------------------------------------------------
# buffers: 0 fp32 sources 1 16-bit copies 2 descriptors 3 dbias / parts 4 amax
SPECIAL = np.asarray([65504.0, -65504.0, 65520.0, -65520.0, 65505.0, 1e5, -1e5, 6e-8, -6e-8, 2.98e-8, 1.00390625, 1.01171875,
                      -1.00390625, -0.0, 0.0, 3.0e38], np.float32)


def cast_case(name, specs, bf, regimes, grid_cap=0, amax=None):
    """specs: dicts with rows, cols and optionally st / tr (copies), tight, colsum ('atomic' / 'parts'), scaled, src_map (q, s),
    dst_mis (16-bit elements added to the straight copy's offset), lo_off, bias_map (q, s, off), special, same_src (index of an
    earlier descriptor whose source is used again)."""
    rs = np.random.RandomState(_seed(('cast', name)))
    P = Pipe('cast', name, regimes)
    sc = pow2_scale(amax) if amax is not None else 1.0
    srcs, src_at, cur = [], [], 0
    for s_ in specs:
        if s_.get('same_src') is not None:
            src_at.append(src_at[s_['same_src']])
            continue
        rows, cols = s_['rows'], s_['cols']
        q, sd = s_.get('src_map', (0, 0))
        cc = np.arange(cols)
        cphys = (cc // q) * sd + cc % q if q else cc
        ld = pad4(int(cphys.max()) + 1) + 4
        S = np.full((rows, ld), NAN, np.float32)
        body = rs.standard_normal((rows, int(cphys.max()) + 1)) * (1e-7 if s_.get('scaled') else 1.0)
        S[:, :body.shape[1]] = body
        S[::3, 1::4] = 0.0
        if s_.get('special'):
            n_sp = min(cols, len(SPECIAL))
            S[0, cphys[:n_sp]] = SPECIAL[:n_sp]
            S[rows - 1, cphys[cols - n_sp:]] = SPECIAL[:n_sp]
        src_at.append((cur, ld, S, cphys))
        srcs.append(S.reshape(-1))
        cur += S.size + 4
        srcs.append(np.full(4, NAN, np.float32))
    b_src = P.add(np.concatenate(srcs + [np.full(SLACK, NAN, np.float32)]))
    descs = np.zeros(len(specs), dtype=L.CAST_DT)
    at16, atf, blocks = 64, 8, 0
    plan = []
    for k, s_ in enumerate(specs):
        rows, cols = s_['rows'], s_['cols']
        off, ld, S, cphys = src_at[k]
        D = descs[k]
        D['src_off'], D['rows'], D['cols'], D['ld_src'] = off, rows, cols, ld
        D['src_q'], D['src_s'] = s_.get('src_map', (0, 0))
        D['lo_off'] = s_.get('lo_off', 0)
        fl = 0
        pl = dict(X=S[:, cphys])
        if s_.get('st'):
            fl |= L.CAST_STRAIGHT | (L.CAST_STRAIGHT_BF16 if bf else 0)
            D['dst_off'], D['ld_dst'] = at16 + s_.get('dst_mis', 0), r64(cols) + 8
            pl['st'] = int(D['dst_off'])
            at16 = r64(at16 + rows * (r64(cols) + 8) + 8) + 64
        if s_.get('tr'):
            fl |= L.CAST_TRANSPOSED | (L.CAST_TRANSPOSED_BF16 if bf else 0) | (L.CAST_TIGHT if s_.get('tight') else 0)
            D['dstT_off'], D['ld_dstT'] = at16, r64(rows) + 8
            pl['tr'] = at16
            at16 = r64(at16 + cols * (r64(rows) + 8)) + 64
        if s_.get('scaled'):
            fl |= L.CAST_SCALED
        if s_.get('colsum') == 'parts':
            fl |= L.CAST_COLSUM | L.CAST_COLSUM_PARTS
            D['part_off'] = atf
            pl['parts'] = atf
            atf += ((rows + 63) // 64) * cols + 5
        elif s_.get('colsum') == 'atomic':
            fl |= L.CAST_COLSUM
            q, sd, boff = s_.get('bias_map', (0, 0, 0))
            D['bias_q'], D['bias_s'], D['bias_off'] = q, sd, atf + boff
            cc = np.arange(cols)
            pl['colsum'] = atf + boff + ((cc // q) * sd + cc % q if q else cc)
            atf = int(pl['colsum'].max()) + 6
        D['flags'], D['block_start'] = fl, blocks
        blocks += ((rows + 63) // 64) * ((cols + 63) // 64)
        plan.append(pl)
    b_16 = P.add(np.full(at16 + 64, NAN16[bf], np.uint16))
    b_desc = P.add(descs.view(np.uint8).reshape(-1))
    dbias = np.full(atf + SLACK, NAN, np.float32)
    for s_, pl in zip(specs, plan):
        if 'colsum' in pl:                               # accumulated: a sentinel of the magnitude of the sums
            pl['init'] = np.float32(SENT * (1e-6 if s_.get('scaled') else 1.0))
            dbias[pl['colsum']] = pl['init']
    b_db = P.add(dbias)
    b_amax = P.add(np.asarray([amax if amax is not None else NAN, NAN, NAN, NAN], np.float32))
    any_sum = any('colsum' in pl or 'parts' in pl for pl in plan)
    P.op(L.OP_CAST16, [b_src, b_16, b_desc, b_db if any_sum else None, b_amax if amax is not None else None],
         (len(specs), blocks, grid_cap))
    for k, (s_, pl) in enumerate(zip(specs, plan)):
        rows, cols = s_['rows'], s_['cols']
        X = pl['X']
        H = to16(X * np.float32(sc if s_.get('scaled') else 1.0), bf)
        if 'st' in pl:
            Z = np.zeros((rows, r64(cols)), np.uint16)
            Z[:, :cols] = H
            P.out('d%d.st' % k, b_16, pl['st'] + np.arange(rows)[:, None] * (r64(cols) + 8) + np.arange(r64(cols))[None, :],
                  lambda dt, Z=Z: Z, 'bits')
        if 'tr' in pl:
            rw = r8(rows) if s_.get('tight') else r64(rows)
            Z = np.zeros((cols, rw), np.uint16)
            Z[:, :rows] = H.T
            P.out('d%d.tr' % k, b_16, pl['tr'] + np.arange(cols)[:, None] * (r64(rows) + 8) + np.arange(rw)[None, :],
                  lambda dt, Z=Z: Z, 'bits')
        if 'parts' in pl:
            nt = (rows + 63) // 64
            P.out('d%d.parts' % k, b_db, pl['parts'] + np.arange(nt)[:, None] * cols + np.arange(cols)[None, :],
                  lambda dt, X=X, nt=nt: np.stack([X[t * 64:(t + 1) * 64].astype(dt).sum(0, dtype=dt) for t in range(nt)]).astype(np.float32),
                  'float')
        if 'colsum' in pl:
            P.out('d%d.colsum' % k, b_db, pl['colsum'],
                  lambda dt, X=X, i0=pl.get('init'): (dt(i0) + X.astype(dt).sum(0, dtype=dt)).astype(np.float32), 'float', rerun=False)
    return P.done(specs=specs, bf=bf, descs=descs, blocks=blocks, grid_cap=grid_cap)


def _cast_cases():
    R = lambda *names: {'cast:' + n_ for n_ in names}
    out = [
        cast_case('cast-parts-f16', [dict(rows=130, cols=70, tr=True, colsum='parts')], False, R('parts')),
        cast_case('cast-parts-bf16-2desc', [dict(rows=65, cols=129, tr=True, colsum='parts'), dict(rows=3, cols=5, tr=True, st=True, colsum='parts')],
                  True, R('parts')),
        cast_case('cast-tight-r77', [dict(rows=77, cols=70, tr=True, tight=True, special=True)], False, R('tight', 'special')),
        cast_case('cast-tight-r13-bf16', [dict(rows=13, cols=130, tr=True, tight=True, colsum='parts')], True, R('tight')),
        cast_case('cast-srcmap', [dict(rows=70, cols=40, st=True, tr=True, src_map=(8, 12)), dict(rows=5, cols=72, tr=True, src_map=(24, 40), colsum='parts')],
                  False, R('src-map')),
        cast_case('cast-scaled-colsum', [dict(rows=60, cols=70, tr=True, scaled=True, colsum='atomic', bias_map=(24, 40, 3))], False,
                  R('scaled-colsum'), amax=AMAX['below-pow2']),
        cast_case('cast-scaled-colsum-bf16', [dict(rows=130, cols=33, tr=True, st=True, scaled=True, colsum='atomic')], True,
                  R('scaled-colsum'), amax=AMAX['pow2']),
        cast_case('cast-gridcap', [dict(rows=130, cols=200, st=True), dict(rows=130, cols=70, tr=True, st=True)], False, R('grid-cap'),
                  grid_cap=3),
        cast_case('cast-5desc', [dict(rows=130, cols=70, st=True), dict(rows=5, cols=200, tr=True), dict(rows=64, cols=64, st=True, tr=True),
                                 dict(rows=1, cols=1, st=True, dst_mis=4), dict(rows=70, cols=5, tr=True, tight=True)], True, R('search')),
    ]
    for cols, bf in ((65, False), (68, True), (71, False)):
        out.append(cast_case('cast-paths-c%d-%s' % (cols, 'bf16' if bf else 'f16'),
                             [dict(rows=70, cols=cols, st=True, special=True),                         # 16-byte path
                              dict(rows=70, cols=cols, st=True, dst_mis=4, same_src=0),                # general: dst_off % 8
                              dict(rows=70, cols=cols, st=True, lo_off=4, same_src=0)],                # general: lo_off % 8
                             bf, R('paths', 'special', 'tail%d' % (cols % 8))))
    return out


def straight_path(D):
    """which of cast16_body's two straight-copy paths descriptor D takes"""
    fl = int(D['flags'])
    fast = (fl & L.CAST_STRAIGHT) and not fl & (L.CAST_TRANSPOSED | L.CAST_FRAG | L.CAST_COLSUM | L.CAST_SRC16) and int(D['src_q']) == 0 \
        and int(D['ld_dst']) % 8 == 0 and int(D['dst_off']) % 8 == 0 and int(D['lo_off']) % 8 == 0
    return 'fast' if fast else 'general' if fl & L.CAST_STRAIGHT else None


# ---- the table ----------------------------------------------------------------------------------------------------------------------
_FAMILIES = {'scaled': _scaled_cases, 'lim': _lim_cases, 'sqgemm': _sumsq_gemm_cases, 'sumsq': _sumsq_cases, 'f32': _f32_cases,
             'cast': _cast_cases}


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(_FAMILIES[family]())


def all_cases():
    return [c for fam in _FAMILIES for c in cases(fam)]


def reference(case, dtype=np.float64):
    """The independent evaluation of the case in `dtype`, results rounded to float32 as every buffer is (16-bit codes for the
    copies).  Computed once per case: do not modify."""
    cache = case.__dict__.setdefault('_ref', {})
    if dtype not in cache:
        cache[dtype] = {o.name: o.ref(dtype) for o in case.outs}
    return cache[dtype]


def out_of_list(outs, name):
    return next(o for o in outs if o.name == name)


def out_of(case, name):
    return out_of_list(case.outs, name)


def masked(case, name, got, ref):
    """got with the don't-care elements of the output replaced by the reference's"""
    o = out_of(case, name)
    return got if o.valid is None else np.where(o.valid, got, ref)


def measure(case, name, got, ref):
    """'float' outputs: worst error per 32 x 32 tile and per row (util_parity.slice_errors); 'entries': every entry against its
    own value."""
    o = out_of(case, name)
    got, ref = np.asarray(got), np.asarray(ref)
    if o.kind == 'entries':
        g64, r64_ = got.astype(np.float64), ref.astype(np.float64)
        with np.errstate(invalid='ignore', divide='ignore'):
            e = np.where(r64_ != 0, np.abs(g64 - r64_) / np.abs(r64_), np.abs(g64 - r64_))
        e = np.where(np.isfinite(e), e, np.inf)
        k = int(np.argmax(e))
        return float(e.reshape(-1)[k]), ('entry', k)
    got = masked(case, name, got, ref)
    worst, where = 0.0, None
    for (g_, axes), (r_, _) in zip(tile_views(got), tile_views(ref)):
        v, w = slice_errors(g_, r_, axes)
        if where is None or v > worst:
            worst, where = v, (g_.shape, w)
    return worst, where


def float_names(case):
    return [o.name for o in case.outs if o.kind != 'bits']


_FLOORS = {}


def floors(case):
    """name -> float32 floor: the formulas in float32 (k-tiles of 64 added in order) against the same in float64"""
    if case.name not in _FLOORS:
        lo, hi = reference(case, np.float32), reference(case, np.float64)
        _FLOORS[case.name] = {k: measure(case, k, lo[k], hi[k])[0] for k in float_names(case)}
    return _FLOORS[case.name]


def raw_bound(case, name):
    """the bound before the cap, with the project's factor 8 alone"""
    return max(FLOOR_FACTOR * floors(case)[name], MIN_BOUND)


def widened(case):
    """cases whose f16 operand copies hold subnormal codes (SUBNORMAL_F16_FACTOR above)"""
    return bool(getattr(case.meta, 'f16_subnormal', False))


def bound(case, name):
    """8 x the float32 floor of the case, at least 1e-6, never above the project's per-tensor fp32 forward limit 2e-5; the GEMM
    results of the cases with subnormal f16 copies: 8 x 2^10 x the floor under the same cap (SUBNORMAL_F16_FACTOR)"""
    f = SUBNORMAL_F16_FACTOR if (widened(case) and name.startswith('C')) else 1.0
    return min(max(f * FLOOR_FACTOR * floors(case)[name], MIN_BOUND), FWD_CAP)
