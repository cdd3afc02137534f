"""Adversarial single-op cases for the decoder tail -- the kernels between the decoder GEMMs and the predicted parameters
(ghn3_amd/csrc/elementwise.hip): GHN3_OP_TILE_FWD / _BWD, GHN3_OP_PARAM_NORM_FWD / _BWD / _FIN, GHN3_OP_RELU_FIX,
GHN3_OP_ROWSET_COLSUM and GHN3_OP_ADD.  Same layout as tests/graphormer_op_cases.py, whose plumbing is imported: a case is one
or more `ghn3_op` records over a list of numpy buffers, every output region pre-filled with NaN (SENT where the op accumulates),
every buffer with slack floats behind its last used element.  The work-block tables of the tile ops come from the host code
itself (ghn3_amd.program.tile_work_tables), so the host's promises about row blocks are part of what is tested.

Shared by tests/test_decoder_tail_cases_cpu.py (the float64 interpreter against `reference`, regime coverage, floors, the
block tables cover every element once) and tests/test_gpu_decoder_tail_ops.py (`ctx.run` against the interpreter).
No GPU is touched here.

`reference(case, dtype)` shares no code with tests/program_interp.py.  A chain of ops is evaluated op by op; an op consumes what
the previous one STORED (float32), as on the device.  Tile forward: out[t] = norm(src[sum_k (t_k mod E_k) S_k]), the digits of
t by divmod; tile backward: torch autograd through that gather of  sum dflat . out + g sum_t ||p_t||  (the norm term with the
stored float32 norm as its denominator: g p_t . p_t / n_t with one factor detached, gradient g p_t / n_t).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from ghn3_amd import _lib as L
from ghn3_amd.program import tile_work_tables
from graphormer_op_cases import (NAN, SENT, FWD_CAP, GRAD_CAP, FLOOR_FACTOR, MIN_BOUND, make_op, _case, host_bytes, run_interp,  # noqa: F401
                                 f32, _seed, blocked)
from util_parity import slice_errors

I64_MIN = np.iinfo(np.int64).min
CHUNK, NORM_CHUNK = 2048, 8192
SLACK = 8

# ---- tile ops ---------------------------------------------------------------------------------------------------------------
# buffers: 0 flat  1..5 sources  6 descriptors + block tables + descriptor -> tensor + 16-bit table  7 sq_parts  8 b_parts
#          9..13 source gradients  14 amax  15 [.. bound at float 63 | norms from float 64]  16 g  17 dflat  18 loss
#          19 first forward block of every tensor  20 ratio scratch
B_FLAT, B_SRC, B_DESC, B_SQ, B_BP, B_DSRC, B_AMAX, B_NORMS, B_G, B_DFLAT, B_LOSS, B_FIRST, B_RATIO = 0, 1, 6, 7, 8, 9, 14, 15, 16, 17, 18, 19, 20
NORMS_AT = 64


def conv_S(R, i_pad=0, ld_pad=0):
    """decoder tile layout of a (o, i, kh, kw) region: one [o][i_ld] matrix per kernel position, row stride ld"""
    i_ld = R[1] + i_pad
    ld = R[0] * i_ld + ld_pad
    return (i_ld, 1, R[3] * ld, ld)


def dense_S(R):
    return (R[1] * R[2] * R[3], R[2] * R[3], R[3], 1)


def D(T, E=None, R=None, S=None, buf=0, mode=0, scale=1.0, seg=None, fill='normal', soff=0, h=None):
    E = tuple(E or T)
    R = tuple(R or E)
    return SimpleNamespace(T=tuple(T), E=E, R=R, S=tuple(S or dense_S(R)), buf=buf, mode=mode, scale=scale, seg=seg, fill=fill,
                           soff=soff, h=h)


def _region(d):
    r = np.indices(d.R).reshape(4, -1)
    return (r * np.asarray(d.S, np.int64)[:, None]).sum(0)


def _fill(rs, kind, n):
    v = rs.standard_normal(n)
    if kind == 'zero':
        return np.zeros(n, np.float32)
    if kind == 'wide':                                   # up to +-20 in front of the sigmoid / tanh
        v = rs.uniform(-20.0, 20.0, n)
        if n >= 4:
            v[:4] = (20.0, -20.0, 0.0, -0.0)
    elif kind == 'big':
        v = v * 1e4
    v = v.astype(np.float32)
    v[5::7] = 0.0                                        # exact zeros
    return v


def tile_case(name, descs, sq=True, bp=True, bwd=None, g=0.75, amax0=0.0, bf16=None):
    """bwd: None, 'dflat', 'norm' or 'both' (the gradient sources); bf16: None = fp32 output, 0 / 1 = the direct 16-bit route
    (descriptors with .h = (offset in 16-bit elements behind the fp32 regions, rel0, ld32, ld16))."""
    rs = np.random.RandomState(_seed(('tile', name)))
    norm_term = bwd in ('norm', 'both')
    assert not norm_term or sq
    cur_src, cur_dst, rows = [5] * 5, 0, []
    for k, d in enumerate(descs):
        d.seg = k if d.seg is None else d.seg
        d.src_off = (cur_src[d.buf] + 3) // 4 * 4 + d.soff
        reg = _region(d)
        assert len(np.unique(reg)) == len(reg) or bwd is None
        cur_src[d.buf] = d.src_off + int(reg.max()) + 1 + 3
        d.dst_off, d.numel = cur_dst, int(np.prod(d.T))
        cur_dst = (cur_dst + d.numel + 15) // 16 * 16
        rows.append((d.dst_off, d.src_off, d.S, d.T, d.E, d.R, d.buf, d.mode, d.scale))
    desc_arr, fb, bb, fwd_first, lds = tile_work_tables(rows)
    nd = len(descs)
    dseg = np.asarray([d.seg for d in descs], np.int32)
    n_seg = int(dseg.max()) + 1
    assert (np.diff(dseg) >= 0).all() and len(np.unique(dseg)) == n_seg
    first = np.asarray([fwd_first[int(np.nonzero(dseg == t)[0][0])] for t in range(n_seg)] + [len(fb)], np.int32)
    # 16-bit table: the copies lie behind every fp32 region of source-gradient buffer 0
    h_tab = np.zeros((nd, 3), np.int64)
    h_tab[:, 0] = I64_MIN
    halfs0 = 2 * ((cur_src[0] + 3) // 4 * 4)
    halfs = halfs0
    for k, d in enumerate(descs):
        if d.h is not None:
            hoff, rel0, ld32, ld16 = d.h
            assert bf16 is not None and d.buf == 0 and d.mode == 0 and rel0 % 4 == 0 and d.src_off % 4 == 0 and ld32 % 4 == 0
            d.h_at = (halfs + 3) // 4 * 4 + hoff
            h_tab[k] = (d.h_at, rel0, ld32 | (ld16 << 32))
            halfs = d.h_at + ((rel0 + int(_region(d).max())) // ld32 + 1) * ld16 + 3
    raw = np.concatenate([a.view(np.uint8).reshape(-1) for a in (desc_arr, fb, bb, dseg, np.zeros((-len(dseg) * 4) % 8, np.uint8), h_tab)])
    off_fb = desc_arr.nbytes
    off_bb = off_fb + fb.nbytes
    off_seg = off_bb + bb.nbytes
    off_h = off_seg + dseg.nbytes + (-len(dseg) * 4) % 8
    srcs = []
    for b in range(5):
        s = rs.standard_normal(cur_src[b] + SLACK).astype(np.float32)
        for d in descs:
            if d.buf == b:
                reg = _region(d)
                s[d.src_off + reg] = _fill(rs, d.fill, len(reg))
        srcs.append(s)
    dsrcs = [np.full(len(s), NAN, np.float32) for s in srcs]
    if halfs > halfs0:
        dsrcs[0] = np.full((halfs + 1) // 2 + SLACK, NAN, np.float32)
    flat = np.full(cur_dst + SLACK, NAN, np.float32)
    dflat = (rs.standard_normal(cur_dst + SLACK) * (1.0 + (np.arange(cur_dst + SLACK) % 5 == 0))).astype(np.float32)
    bufs = [flat] + srcs + [raw, np.full(len(fb) + SLACK, NAN, np.float32), np.full(len(fb) + SLACK, NAN, np.float32)] + dsrcs + \
        [np.asarray([amax0, 0, 0, 0], np.float32), np.full(NORMS_AT + n_seg + SLACK, NAN, np.float32), np.asarray([g, 0, 0, 0], np.float32),
         dflat, np.full(4, SENT, np.float32), first, np.full(n_seg + SLACK, NAN, np.float32)]
    ops = []
    fwd = bwd is None or norm_term
    if fwd:
        ops.append(make_op(L.OP_TILE_FWD, [B_FLAT] + [B_SRC + b for b in range(5)] + [None, B_DESC, B_SQ if sq else None,
                                                                                  B_BP if (sq and bp) else None],
                           (nd, len(fb), off_fb, lds[0])))
    fin = norm_term
    if fin:
        have_b = bool(sq and bp)
        ops.append(make_op(L.OP_PARAM_NORM_FIN, [B_LOSS, (B_NORMS, 4 * NORMS_AT), B_SQ, B_FIRST, B_BP if have_b else None,
                                                 B_RATIO if have_b else None, (B_NORMS, 4 * NORMS_AT - 4) if have_b else None], (n_seg,)))
    if bwd:
        assert bf16 is None or (bwd == 'norm' and sq and bp)
        refs = [B_DFLAT if bwd in ('dflat', 'both') else None] + [B_SRC + b for b in range(5)] + [B_G if norm_term else None, B_DESC] + \
            [B_DSRC + b for b in range(5)] + [B_AMAX, (B_NORMS, 4 * NORMS_AT) if norm_term else None, B_FLAT if norm_term else None]
        ops.append(make_op(L.OP_TILE_BWD, refs, (nd, len(bb), off_bb, lds[1], off_seg, off_h if bf16 is not None else 0, bf16 or 0)))
    fam = 'tilef' if bwd is None else 'tileb16' if bf16 is not None else 'tileb'
    return _case(fam, name, ops, bufs, descs=descs, desc_arr=desc_arr, fb=fb, bb=bb, lds=lds, dseg=dseg, n_seg=n_seg, first=first,
                 sq=sq, bp=bool(sq and bp), bwd=bwd, fwd=fwd, fin=fin, norm_term=norm_term, g=g, amax0=amax0, bf16=bf16, h_tab=h_tab,
                 n_flat=cur_dst)


def _tilef_cases():
    out = []
    # element blocks
    for mode in (0, 1, 2):
        out.append(tile_case('tilef-elem-mode%d' % mode, [D((5, 7, 3, 3), mode=mode, scale=1.5 if mode == 0 else 1.0, fill='wide' if mode else 'normal'),
                                                         D((3, 5, 2, 2), mode=mode, fill='wide' if mode else 'normal')],
                             sq=mode != 1, bp=mode == 0))
    wraps = {'w0': ((6, 5, 3, 2), (4, 5, 3, 2)), 'w1': ((3, 9, 3, 2), (3, 4, 3, 2)), 'w2': ((3, 5, 5, 2), (3, 5, 3, 2)),
             'w3': ((3, 5, 2, 7), (3, 5, 2, 3)), 'wall': ((5, 7, 3, 3), (2, 3, 2, 2))}
    out.append(tile_case('tilef-elem-wrap', [D(T, E, mode=k % 3, fill='wide' if k % 3 else 'normal') for k, (T, E) in enumerate(wraps.values())]))
    out.append(tile_case('tilef-elem-blocks', [D((20, 300, 1, 1), (20, 300, 1, 1), S=(304, 1, 0, 0), scale=0.75),      # hw = 1: element blocks
                                              D((9, 300, 1, 1), (4, 300, 1, 1), mode=1, fill='wide'),
                                              D((3, 300, 1, 1), mode=2, fill='wide')]))
    # broadcast strides (3-D targets: positional encoding rows) and all five source buffers at non-zero offsets
    out.append(tile_case('tilef-elem-sources', [D((1, 6, 10, 1), (1, 6, 8, 1), S=(0, 12, 1, 0), buf=0, soff=1),
                                               D((4, 6, 1, 1), (3, 6, 1, 1), S=(1, 8, 0, 0), buf=1, soff=2),
                                               D((1, 37, 1, 1), (1, 20, 1, 1), S=(0, 1, 0, 0), buf=2, mode=1, fill='wide'),
                                               D((1, 9, 1, 1), (1, 5, 1, 1), S=(0, 1, 0, 0), buf=3, soff=3, seg=3),
                                               D((1, 1, 11, 1), (1, 1, 7, 1), S=(0, 0, 1, 0), buf=4, mode=2, fill='wide', seg=3)], bp=False))
    out.append(tile_case('tilef-elem-noparts', [D((5, 7, 3, 3), (2, 3, 2, 2)), D((3, 300, 1, 1), mode=2, fill='wide')], sq=False))
    # row blocks
    rowd = [
        D((3, 16, 3, 3), S=conv_S((3, 16, 3, 3), 0, 16)),                                   # 16-byte source path
        D((2, 24, 3, 3), (2, 16, 3, 3), S=conv_S((2, 16, 3, 3))),                           # E1 != T1: si % E1
        D((2, 18, 3, 3), S=conv_S((2, 18, 3, 3), 2, 0), scale=-2.0),                        # ni % 4 != 0
        D((2, 16, 3, 3), S=conv_S((2, 16, 3, 3), 0, 2)),                                    # S3 % 4 != 0
        D((2, 16, 3, 3), S=conv_S((2, 16, 3, 3)), soff=1),                                  # src + i0 misaligned
        D((5, 16, 2, 2), (2, 16, 2, 2), S=conv_S((2, 16, 2, 2)), scale=0.75),               # E0 < T0: a0 % E0
        D((3, 5, 3, 3), S=conv_S((3, 5, 3, 3), 3, 0)),                                      # T1 < 16; rows start at 45 t: n % 4 != 0
        D((2, 100, 7, 7), S=conv_S((2, 100, 7, 7))),                                        # hw = 49: chunks of 80 and 20
        D((2, 16, 3, 3), S=conv_S((2, 16, 3, 3)), fill='zero'),                             # a tensor of norm 0
    ]
    out.append(tile_case('tilef-row-mix', rowd))
    out.append(tile_case('tilef-row-hw4', [D((2, 1030, 2, 2), S=conv_S((2, 1030, 2, 2), 2, 0)), D((2, 20, 2, 2), S=conv_S((2, 20, 2, 2)))], bp=False))
    out.append(tile_case('tilef-row-hw9', [D((2, 452, 3, 3), S=conv_S((2, 452, 3, 3)), scale=1.5)], sq=False))
    out.append(tile_case('tilef-row-hw784', [D((2, 18, 28, 28), S=conv_S((2, 18, 28, 28), 2, 0)), D((1, 16, 28, 28), S=conv_S((1, 16, 28, 28)))]))
    return out


def _tileb_cases():
    out = []
    k = 0
    for src in ('dflat', 'norm', 'both'):
        # element blocks: R larger than E in each dimension, replica sums with partial last replicas, R1 in {1, 3, 300}
        ds = [D((5, 7, 3, 3), (2, 3, 2, 2), (3, 3, 3, 3), mode=0, scale=1.5),
              D((5, 7, 3, 3), (2, 3, 2, 2), (2, 4, 2, 2), mode=1, fill='wide'),
              D((4, 3, 2, 2), (3, 3, 2, 2), (4, 3, 2, 2), mode=2, fill='wide'),
              D((2, 7, 1, 1), (2, 1, 1, 1), (2, 1, 1, 1), S=(1, 0, 0, 0), buf=2),            # R1 = 1 (3-D target from the 1-D decoder)
              D((9, 700, 1, 1), (8, 300, 1, 1), (8, 300, 1, 1), S=(304, 1, 0, 0), buf=1, scale=0.75),     # R1 = 300, two blocks
              D((3, 5, 2, 2), fill='zero', buf=0),                                            # norm 0: kn = 0
              D((1, 9, 1, 1), (1, 5, 1, 1), (1, 6, 1, 1), S=(0, 1, 0, 0), buf=3)]
        out.append(tile_case('tileb-elem-%s' % src, ds, bwd=src, amax0=(1e-3, 50.0, 0.0)[k], g=(0.75, -1.25, 2.0)[k]))
        k += 1
    out.append(tile_case('tileb-elem-buf1-only', [D((4, 6, 1, 1), (3, 6, 1, 1), S=(1, 8, 0, 0), buf=1)], bwd='dflat', amax0=0.125))
    for src, am in (('dflat', 0.0), ('norm', 40.0), ('both', 1e-3)):
        ds = [D((5, 16, 3, 3), (2, 16, 3, 3), (3, 16, 3, 3), S=conv_S((3, 16, 3, 3), 0, 16)),            # rows a0 >= E0, replicas along o
              D((2, 40, 3, 3), (2, 16, 3, 3), (2, 16, 3, 3), S=conv_S((2, 16, 3, 3))),                   # replicas along i, partial last
              D((2, 24, 3, 3), (2, 20, 3, 3), (2, 24, 3, 3), S=conv_S((2, 24, 3, 3))),                   # nl < ni, 16-byte store
              D((2, 100, 7, 7), (2, 50, 7, 7), (2, 100, 7, 7), S=conv_S((2, 100, 7, 7))),                # nl < ni in chunk 0, nl = 0 in chunk 1
              D((2, 250, 7, 7), (2, 100, 7, 7), (2, 120, 7, 7), S=conv_S((2, 120, 7, 7)), buf=1),        # partial last replica in chunk 0
              D((3, 7, 3, 3), (2, 5, 3, 3), (2, 5, 3, 3), S=conv_S((2, 5, 3, 3), 3, 0), scale=-2.0),     # n % 4 != 0, scalar store
              D((2, 18, 3, 3), S=conv_S((2, 18, 3, 3), 2, 2), soff=1),                                   # scalar store: strides + base
              D((2, 452, 3, 3), (1, 452, 3, 3), (1, 452, 3, 3), S=conv_S((1, 452, 3, 3)), buf=1),        # chunks of 448 and 4 channels
              D((2, 16, 3, 3), S=conv_S((2, 16, 3, 3)), fill='zero')]
        out.append(tile_case('tileb-row-%s' % src, ds, bwd=src, amax0=am, g=1.5))
    # more than 4096 elements in one row block (hw > 256: 16 channels per chunk whatever hw is): the U = 4 batch loop runs twice
    out.append(tile_case('tileb-row-batch2', [D((3, 16, 17, 17), (2, 16, 17, 17), S=conv_S((2, 16, 17, 17)))], bwd='both', g=0.5))
    return out


def _tileb16_cases():
    out = []
    for bf16 in (0, 1):
        for mis in (0, 2):
            R1, R2 = (3, 16, 3, 3), (2, 20, 3, 3)
            S1, S2 = conv_S(R1, 0, 16), conv_S(R2, 0, 4)
            ds = [D((5, 16, 3, 3), (2, 16, 3, 3), R1, S=S1, h=(mis, 8, S1[3], S1[3] + 8)),                # row blocks, 16-byte store
                  D((2, 24, 3, 3), (2, 20, 3, 3), R2, S=S2, h=(mis, 4, S2[3], S2[3] + 8)),                # replicas along i, nl < ni
                  D((3, 7, 3, 3), (2, 5, 3, 3), (2, 5, 3, 3), S=conv_S((2, 5, 3, 3), 3, 0), h=(0, 0, 16, 24), fill='big'),   # scalar row-block store; 1e4 x the rest, decides the bound
                  D((9, 40, 1, 1), (8, 30, 1, 1), (8, 32, 1, 1), S=(32, 1, 0, 0), scale=0.75, h=(1, 12, 32, 40)),   # element blocks
                  D((2, 16, 3, 3), S=conv_S((2, 16, 3, 3))),                                               # h = INT64_MIN: keeps fp32
                  D((1, 37, 1, 1), (1, 20, 1, 1), S=(0, 1, 0, 0), buf=2, mode=1, fill='wide')]             # source buffer 2: fp32
            out.append(tile_case('tileb16-%s-h%d' % ('bf16' if bf16 else 'f16', mis), ds, bwd='norm', bf16=bf16, g=(-0.75, 3.0)[bf16]))
    return out


def _digits(n, radices):
    """all elements 0 .. n - 1 as digits of the mixed radix `radices` (last fastest), by divmod"""
    q = np.arange(n, dtype=np.int64)
    out = []
    for r in reversed(radices):
        out.append(q % r)
        q = q // r
    return out[::-1]


def _src_index(d):
    t = _digits(d.numel, d.T)
    return d.src_off + sum((t[k] % d.E[k]) * d.S[k] for k in range(4))


def block_range(case, table, k, shape_of):
    """(descriptor, lo, hi, (a0, i0) or None): block k of `table` handles elements lo .. hi of its descriptor in the order of the
    pass (forward: target order; backward row blocks: i0 .. i0 + ni of source row a0, all kernel positions)."""
    di, word = int(table[k, 0]), int(table[k, 1])
    if di >= 0:
        n = int(np.prod(shape_of(case.meta.descs[di])))
        return di, word, min(word + CHUNK, n), None
    di = ~di
    d = case.meta.descs[di]
    a0, i0 = word & 0xffffff, word >> 24
    n1 = shape_of(d)[1]
    ni = min(int(case.meta.desc_arr['_pad'][di]), n1 - i0)
    hw = d.T[2] * d.T[3]
    return di, (a0 * n1 + i0) * hw, (a0 * n1 + i0 + ni) * hw, (a0, i0)


def _norm_np(v, mode, scale, dt):
    v = v.astype(dt)
    if mode == 0:
        return v * dt(scale)
    if mode == 1:
        return dt(2) / (dt(1) + np.exp(dt(-0.5) * v))
    return np.tanh(dt(0.2) * v)


def _norm_t(v, mode, scale):
    if mode == 0:
        return v * scale
    if mode == 1:
        return 2.0 * torch.sigmoid(0.5 * v)
    return torch.tanh(0.2 * v)


def _pow2_scale(amax):
    amax = float(amax)
    if not amax > 0:
        return 1.0
    e = math.frexp(amax)[1] - 1
    return 1.0 if e < -100 else math.ldexp(1.0, 11 - e)


def _to16(x, bf16):
    x = np.ascontiguousarray(x, np.float32)
    if not bf16:
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _tile_reference(case, dt):
    m = case.meta
    tdt = torch.float64 if dt == np.float64 else torch.float32
    b = case.bufs
    res = {}
    outs = []
    for k, d in enumerate(m.descs):
        o = _norm_np(b[B_SRC + d.buf][_src_index(d)], d.mode, d.scale, dt).astype(np.float32)
        outs.append(o)
        if m.fwd:
            res['out.d%d' % k] = o.reshape(d.T)
    if m.fwd and m.sq:
        sqv, bpv = np.zeros(len(m.fb), np.float32), np.zeros(len(m.fb), np.float32)
        for kb in range(len(m.fb)):
            di, lo, hi, _ = block_range(case, m.fb, kb, lambda d_: d_.T)
            d = m.descs[di]
            w = outs[di][lo:hi].astype(dt)
            sqv[kb] = (w * w).sum(dtype=dt)
            if d.buf == 0 and d.mode == 0 and hi > lo:
                reps = np.prod([(d.T[j] + d.E[j] - 1) // d.E[j] for j in range(4)])
                bpv[kb] = dt(np.abs(outs[di][lo:hi]).max()) * dt(abs(d.scale) * reps)
        res['sq'] = sqv
        if m.bp:
            res['bp'] = bpv
    if m.fin:
        norms = np.asarray([np.sqrt(res['sq'][m.first[t]:m.first[t + 1]].astype(dt).sum(dtype=dt)) for t in range(m.n_seg)]).astype(np.float32)
        res['norms'] = norms
        res['loss'] = np.asarray([norms.astype(dt).sum(dtype=dt)], np.float32)
        if m.bp:
            ratio = np.asarray([(res['bp'][m.first[t]:m.first[t + 1]].max() / norms[t]) if norms[t] > 0 and m.first[t + 1] > m.first[t] else 0.0
                                for t in range(m.n_seg)], np.float32)
            res['ratio'], res['bound'] = ratio, np.asarray([ratio.max()], np.float32)
    if m.bwd:
        g = np.float32(m.g)
        srcs = [torch.from_numpy(b[B_SRC + j].copy()).to(tdt).requires_grad_(True) for j in range(5)]
        loss = torch.zeros((), dtype=tdt)
        for k, d in enumerate(m.descs):
            o = _norm_t(srcs[d.buf][torch.from_numpy(_src_index(d))], d.mode, float(np.float32(d.scale)))
            if m.bwd in ('dflat', 'both'):
                loss = loss + (o * torch.from_numpy(b[B_DFLAT][d.dst_off:d.dst_off + d.numel].copy()).to(tdt)).sum()
            if m.norm_term and res['norms'][d.seg] > 0:
                saved = torch.from_numpy(outs[k].copy()).to(tdt)                 # the stored float32 predicted values
                loss = loss + (float(g) / float(res['norms'][d.seg])) * (o * saved).sum()
        loss.backward()
        top = 0.0
        if m.bf16 is not None:
            bnd = np.float32(res['bound'][0]) * np.float32(abs(g))
            hsc = np.float32(_pow2_scale(bnd))
            res['amax'] = np.asarray([bnd], np.float32)
        for k, d in enumerate(m.descs):
            reg = d.src_off + _region(d)
            gr = srcs[d.buf].grad.numpy()[reg].astype(np.float32)
            res['dsrc.d%d' % k] = gr.reshape(d.R)
            if m.bf16 is not None and d.h is not None:
                res['h16.d%d' % k] = _to16(gr * hsc, m.bf16).reshape(d.R)
            if d.buf == 0 and gr.size:
                top = max(top, float(np.abs(gr).max()))
        if m.bf16 is None:
            res['amax'] = np.asarray([max(top, m.amax0)], np.float32)
    return res


def h16_addr(d):
    """positions (16-bit elements behind source-gradient buffer 0) of the region of descriptor d, in region order"""
    hoff, rel0, ld32, ld16 = d.h
    rel = rel0 + _region(d)
    return d.h_at + (rel // ld32) * ld16 + rel % ld32


def _tile_extract(case, bufs):
    m = case.meta
    res = {}
    flat = f32(bufs, B_FLAT)
    for k, d in enumerate(m.descs):
        if m.fwd:
            res['out.d%d' % k] = flat[d.dst_off:d.dst_off + d.numel].reshape(d.T)
        if m.bwd:
            if m.bf16 is not None and d.h is not None:
                res['h16.d%d' % k] = bufs[B_DSRC].view(np.uint8).view(np.uint16)[h16_addr(d)].reshape(d.R)
            else:
                res['dsrc.d%d' % k] = f32(bufs, B_DSRC + d.buf)[d.src_off + _region(d)].reshape(d.R)
    if m.fwd and m.sq:
        res['sq'] = f32(bufs, B_SQ)[:len(m.fb)]
        if m.bp:
            res['bp'] = f32(bufs, B_BP)[:len(m.fb)]
    if m.fin:
        res['norms'], res['loss'] = f32(bufs, B_NORMS)[NORMS_AT:NORMS_AT + m.n_seg], f32(bufs, B_LOSS)[:1]
        if m.bp:
            res['ratio'], res['bound'] = f32(bufs, B_RATIO)[:m.n_seg], f32(bufs, B_NORMS)[NORMS_AT - 1:NORMS_AT]
    if m.bwd:
        res['amax'] = f32(bufs, B_AMAX)[:1]
    return res


def tile_written(case):
    """(buffer -> boolean mask over its floats of what the case's ops write, the same for source-gradient buffer 0 viewed as
    16-bit elements); everything else keeps its bits"""
    m = case.meta
    w = {k: np.zeros(case.bufs[k].size, bool) for k in (B_FLAT, B_SQ, B_BP, B_AMAX, B_NORMS, B_LOSS, B_RATIO)}
    w.update({B_DSRC + j: np.zeros(case.bufs[B_DSRC + j].size, bool) for j in range(5)})
    h = np.zeros(2 * case.bufs[B_DSRC].size, bool)
    for d in m.descs:
        if m.fwd:
            w[B_FLAT][d.dst_off:d.dst_off + d.numel] = True
        if m.bwd:
            if m.bf16 is not None and d.h is not None:
                h[h16_addr(d)] = True
            else:
                w[B_DSRC + d.buf][d.src_off + _region(d)] = True
    if m.fwd and m.sq:
        w[B_SQ][:len(m.fb)] = True
        w[B_BP][:len(m.fb)] = m.bp
    if m.fin:
        w[B_NORMS][NORMS_AT:NORMS_AT + m.n_seg] = True
        w[B_LOSS][0] = True
        if m.bp:
            w[B_RATIO][:m.n_seg] = True
            w[B_NORMS][NORMS_AT - 1] = True
    if m.bwd and (m.bf16 is not None or any(d.buf == 0 for d in m.descs)):
        w[B_AMAX][0] = True
    h16 = h | np.repeat(w[B_DSRC], 2)                   # (16-bit view of source-gradient buffer 0: the copies and the fp32 regions)
    w[B_DSRC] = w[B_DSRC] | h.reshape(-1, 2).any(1)
    return w, h16


def _tile_views(case, name, a):
    if a.ndim == 4:                                   # per o row and per 16-channel group of i
        return [(blocked(a, 1, 16), [(0,), (1,), (0, 1)])]
    return [(a, [tuple(range(a.ndim))])]


# ---- PARAM_NORM_FWD (both forms) + PARAM_NORM_BWD ---------------------------------------------------------------------------
# buffers: 0 loss 1 flat 2 segments 3 norms 4 first_seg 5 parts 6 dflat 7 norms (atomic form) 8 loss (atomic form)
def pnorm_case(name, segs, fills=None, g=0.75):
    rs = np.random.RandomState(_seed(('pnorm', name)))
    seg = np.asarray(segs, np.int64).reshape(-1, 2)
    n, numel = len(seg), int(seg[-1, 1])
    flat = rs.standard_normal(numel + SLACK).astype(np.float32)
    flat[3::11] = 0.0
    for k, kind in (fills or {}).items():
        s0, s1 = seg[k]
        flat[s0:s1] = 0.0 if kind == 'zero' else flat[s0:s1] * np.float32(1e4)
    n_chunks = (numel + NORM_CHUNK - 1) // NORM_CHUNK
    first = np.searchsorted(seg[:, 1], np.arange(0, max(numel, 1), NORM_CHUNK), side='right').astype(np.int32)
    bufs = [np.full(4, SENT, np.float32), flat, seg.reshape(-1), np.full(n + SLACK, NAN, np.float32), first,
            np.full(n_chunks + n + SLACK, NAN, np.float32), np.full(numel + SLACK, NAN, np.float32), np.full(n + SLACK, NAN, np.float32),
            np.full(4, SENT, np.float32)]
    ops = [make_op(L.OP_PARAM_NORM_FWD, [0, 1, 2, 3, 4, 5], (n, numel)),
           make_op(L.OP_PARAM_NORM_FWD, [8, 1, 2, 7], (n, numel)),
           make_op(L.OP_PARAM_NORM_BWD, [6, 1, 2, 3, 4], (n, numel), (g,))]
    return _case('pnorm', name, ops, bufs, seg=seg, n=n, numel=numel, g=g, first=first, n_chunks=n_chunks)


def _pnorm_cases():
    out = [pnorm_case('pnorm-1seg', [(3, 8190)]),
           # five segments inside chunk 0 (unaligned ends, shorter than 4, empty), a gap of more than one chunk, one that straddles
           # a boundary and one that ends exactly on the next
           pnorm_case('pnorm-5seg', [(1, 6), (6, 9), (9, 9), (13, 8000), (8001, 8003)], {3: 'big'}),
           pnorm_case('pnorm-gap', [(2, 100), (100, 103), (3 * 8192 + 5, 4 * 8192 + 7), (4 * 8192 + 16, 5 * 8192), (5 * 8192, 5 * 8192 + 3)],
                      {1: 'zero'})]
    rs = np.random.RandomState(5)
    lens = rs.randint(0, 90, 261)
    lens[::17] = 0
    starts = np.cumsum(np.concatenate([[2], lens[:-1] + rs.randint(0, 3, 260)]))
    out.append(pnorm_case('pnorm-261seg', np.stack([starts, starts + lens], 1), {7: 'zero', 100: 'big'}))
    out.append(pnorm_case('pnorm-600k', [(5, 600005), (600016, 600020)]))
    return out


def _pnorm_reference(case, dt):
    m, b = case.meta, case.bufs
    norms = np.asarray([np.sqrt((b[1][s0:s1].astype(dt) ** 2).sum(dtype=dt)) for s0, s1 in m.seg]).astype(np.float32)
    dflat = b[6].copy()
    for (s0, s1), nrm in zip(m.seg, norms):
        dflat[s0:s1] = (b[1][s0:s1].astype(dt) * (dt(np.float32(m.g)) / dt(nrm) if nrm > 0 else dt(0))).astype(np.float32)
    loss = np.asarray([dt(SENT) + norms.astype(dt).sum(dtype=dt)], np.float32)
    return {'norms': norms, 'norms_atomic': norms, 'loss': loss, 'loss_atomic': loss, 'dflat': dflat[:m.numel + SLACK]}


def _pnorm_extract(case, bufs):
    m = case.meta
    return {'norms': f32(bufs, 3)[:m.n], 'norms_atomic': f32(bufs, 7)[:m.n], 'loss': f32(bufs, 0)[:1], 'loss_atomic': f32(bufs, 8)[:1],
            'dflat': f32(bufs, 6)[:m.numel + SLACK]}


def seg_split(case, a):
    """a flat-sized array cut into the case's segments (finite parts only)"""
    return [a[s0:s1] for s0, s1 in case.meta.seg]


# ---- PARAM_NORM_FIN alone ---------------------------------------------------------------------------------------------------
# buffers: 0 loss 1 [.. bound | norms] 2 parts 3 first 4 b_parts 5 ratio
def pfin_case(name, counts, bp, zero=()):
    rs = np.random.RandomState(_seed(('pfin', name)))
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    nb, n = int(first[-1]), len(counts)
    parts = (rs.standard_normal(nb + SLACK) ** 2).astype(np.float32)
    bparts = np.abs(rs.standard_normal(nb + SLACK)).astype(np.float32)
    for t in zero:
        parts[first[t]:first[t + 1]] = 0.0
    parts[nb:] = NAN
    bparts[nb:] = NAN
    bufs = [np.full(4, SENT, np.float32), np.full(NORMS_AT + n + SLACK, NAN, np.float32), parts, first, bparts, np.full(n + SLACK, NAN, np.float32)]
    ops = [make_op(L.OP_PARAM_NORM_FIN, [0, (1, 4 * NORMS_AT), 2, 3, 4 if bp else None, 5 if bp else None, (1, 4 * NORMS_AT - 4) if bp else None], (n,))]
    return _case('pfin', name, ops, bufs, first=first, n=n, bp=bp, counts=list(counts))


def _pfin_cases():
    counts = [0, 1, 63, 64, 65, 200, 3]
    return [pfin_case('pfin-bparts', counts, True, zero=(6,)), pfin_case('pfin-plain', counts, False, zero=(6,)),
            pfin_case('pfin-261', [1 + k % 3 for k in range(261)], True)]


def _pfin_reference(case, dt):
    m, b = case.meta, case.bufs
    norms = np.asarray([np.sqrt(b[2][m.first[t]:m.first[t + 1]].astype(dt).sum(dtype=dt)) for t in range(m.n)]).astype(np.float32)
    res = {'norms': norms, 'loss': np.asarray([norms.astype(dt).sum(dtype=dt)], np.float32)}
    if m.bp:
        ratio = np.asarray([b[4][m.first[t]:m.first[t + 1]].max() / norms[t] if (m.counts[t] and norms[t] > 0) else 0.0 for t in range(m.n)], np.float32)
        res['ratio'], res['bound'] = ratio, np.asarray([ratio.max()], np.float32)
    return res


def _pfin_extract(case, bufs):
    m = case.meta
    res = {'norms': f32(bufs, 1)[NORMS_AT:NORMS_AT + m.n], 'loss': f32(bufs, 0)[:1]}
    if m.bp:
        res['ratio'], res['bound'] = f32(bufs, 5)[:m.n], f32(bufs, 1)[NORMS_AT - 1:NORMS_AT]
    return res


# ---- RELU_FIX -----------------------------------------------------------------------------------------------------------------
# buffers: 0 X 1 U 2 W 3 bias
def rfix_case(rows, cols, K, tau_rel, rowmap, bias, fence=False):
    """fence: every |x| = 0.5 and tau_rel = 1, so tau = rms = 0.5 exactly in float32 and in float64 -- no coin toss: `<` is strict, nobody
    is a candidate and W (NaN) is not read."""
    ld = (cols + 7) // 4 * 4
    q, sdim = (5, 7) if rowmap else (0, 0)
    c = np.arange(cols)
    wrow = (c // q) * sdim + c % q if q else c
    n_w = int(wrow.max()) + 1
    name = 'rfix-r%d-c%d-K%d-tau%g-map%d-bias%d%s' % (rows, cols, K, tau_rel, rowmap, bias, '-fence' if fence else '')
    for attempt in range(64):
        rs = np.random.RandomState(_seed(('rfix', name, attempt)))
        U = rs.standard_normal((rows, K)).astype(np.float32)
        W = (rs.standard_normal((n_w, K)) / math.sqrt(K)).astype(np.float32)
        bv = (0.3 * rs.standard_normal(n_w)).astype(np.float32)
        exact = U.astype(np.float64) @ W.astype(np.float64)[wrow].T + (bv.astype(np.float64)[wrow] if bias else 0.0)
        x = (exact * (1.0 + 1e-3 * rs.standard_normal(exact.shape))).astype(np.float32)         # as a 16-bit GEMM leaves it
        x[:, ::9] = 0.0
        if fence:
            x = np.where(rs.random_sample(x.shape) < 0.5, -0.5, 0.5).astype(np.float32)
        X = np.full((rows, ld), NAN, np.float32)
        X[:, :cols] = x
        ok = True
        if tau_rel > 0 and not fence:
            for c0 in range(0, cols, 1024):
                blk = x[:, c0:c0 + 1024].astype(np.float64)
                tau = tau_rel * np.sqrt((blk ** 2).mean(1, keepdims=True))
                ok &= bool((np.abs(np.abs(blk) - tau) > 1e-4 * tau).all())       # nobody on the fence of the fp32 / fp64 tau
        if ok:
            break
    assert ok, name
    if tau_rel == 0 or fence:
        W = np.full_like(W, NAN)                                                 # plain ReLU: W is not read
    bufs = [np.concatenate([X.reshape(-1), np.full(SLACK, NAN, np.float32)]), np.concatenate([U.reshape(-1), np.zeros(SLACK, np.float32)]),
            np.concatenate([W.reshape(-1), np.zeros(SLACK, np.float32)]), np.concatenate([bv, np.zeros(SLACK, np.float32)])]
    ops = [make_op(L.OP_RELU_FIX, [0, 1, 2, 3 if bias else None], (rows, cols, ld, K, q, sdim), (tau_rel,))]
    return _case('rfix', name, ops, bufs, rows=rows, cols=cols, ld=ld, K=K, tau_rel=tau_rel, q=q, sdim=sdim, wrow=wrow, bias=bias, fence=fence)


def _rfix_cases():
    out, k = [], 0
    for cols in (5, 1024, 1030, 2049):                    # (K = 252 and 260 on the narrow matrix: W has cols x K floats)
        for tau in (0.0, 5e-3, 10.0):
            if tau == 10.0 and cols not in (5, 1030):
                continue
            out.append(rfix_case(3, cols, (252, 260, 260)[k % 3] if cols == 5 else 4, tau, k % 2 == 1, k % 4 < 2))
            k += 1
    out.append(rfix_case(70, 5, 252, 5e-3, True, False))
    out.append(rfix_case(70, 5, 260, 5e-3, False, True))
    out.append(rfix_case(2, 1030, 4, 5e-3, False, False))
    out.append(rfix_case(2, 5, 4, 1.0, False, True, fence=True))
    out.append(rfix_case(2, 1024, 4, 1.0, True, False, fence=True))
    return out


def rfix_candidates(case):
    """boolean [rows][cols]: |x| below tau_rel x the rms of its 1024-column block (float64)"""
    m = case.meta
    x = case.bufs[0][:m.rows * m.ld].reshape(m.rows, m.ld)[:, :m.cols].astype(np.float64)
    cand = np.zeros(x.shape, bool)
    if m.tau_rel > 0:
        for c0 in range(0, m.cols, 1024):
            blk = x[:, c0:c0 + 1024]
            cand[:, c0:c0 + 1024] = np.abs(blk) < m.tau_rel * np.sqrt((blk ** 2).mean(1, keepdims=True))
    return cand


def _rfix_reference(case, dt):
    m, b = case.meta, case.bufs
    X = b[0][:m.rows * m.ld].reshape(m.rows, m.ld).copy()
    cand = rfix_candidates(case)
    if cand.any():
        U, W = b[1][:m.rows * m.K].reshape(m.rows, m.K).astype(dt), b[2][:-SLACK].reshape(-1, m.K).astype(dt)
        full = U @ W[m.wrow].T + (b[3][m.wrow].astype(dt) if m.bias else dt(0))
        X[:, :m.cols] = np.where(cand, full.astype(np.float32), X[:, :m.cols])
    return {'X': np.maximum(X[:, :m.cols], 0)}


def _rfix_extract(case, bufs):
    m = case.meta
    return {'X': f32(bufs, 0)[:m.rows * m.ld].reshape(m.rows, m.ld)[:, :m.cols]}


# ---- ROWSET_COLSUM ------------------------------------------------------------------------------------------------------------
# buffers: 0 out 1 X 2 sets
def rset_case(name, O, I, sets):
    """sets: (rows, o, i, ld, i0)"""
    rs = np.random.RandomState(_seed(('rset', name)))
    tab = np.zeros(len(sets), L.ROWSET_DT)
    off = 3
    for k, (rows, o, i, ld, i0) in enumerate(sets):
        assert ld >= o * i and i0 + i <= I and o <= O
        tab[k] = (off, rows, o, i, ld, i0, 0)
        off += rows * ld + 5
    X = (rs.standard_normal(off + 8 * SLACK) + 0.5).astype(np.float32)
    X[2::13] = 0.0
    return _case('rset', name, [make_op(L.OP_ROWSET_COLSUM, [0, 1, 2], (len(sets), O, I))],
                 [np.full(O * I + SLACK, SENT, np.float32), X, tab.view(np.uint8).reshape(-1)], O=O, I=I, sets=sets, tab=tab)


def _rset_cases():
    return [rset_case('rset-bias0', 1, 70, [(33, 1, 66, 72, 0)]),
            rset_case('rset-4sets', 5, 150, [(1, 3, 40, 125, 10), (3, 4, 30, 121, 20), (33, 2, 100, 203, 45), (70, 1, 7, 9, 70)]),
            rset_case('rset-spans', 3, 200, [(3, 3, 140, 425, 50), (70, 2, 9, 19, 130), (1, 1, 64, 64, 64)])]


def _rset_reference(case, dt):
    m, b = case.meta, case.bufs
    out = np.zeros((m.O, m.I), dt)
    for S in m.tab:
        for op in range(int(S['o'])):
            for r in range(int(S['rows'])):
                a = int(S['off']) + r * int(S['ld']) + op * int(S['i'])
                out[op, int(S['i0']):int(S['i0']) + int(S['i'])] += b[1][a:a + int(S['i'])].astype(dt)
    return {'out': b[0][:m.O * m.I].reshape(m.O, m.I) + out.astype(np.float32)}          # a float32 sum added to the float32 buffer


def _rset_extract(case, bufs):
    m = case.meta
    return {'out': f32(bufs, 0)[:m.O * m.I].reshape(m.O, m.I)}


# ---- ADD ----------------------------------------------------------------------------------------------------------------------
def add_case(n):
    rs = np.random.RandomState(_seed(('add', n)))
    a, b_ = rs.standard_normal(n + SLACK).astype(np.float32), rs.standard_normal(n + SLACK).astype(np.float32)
    return _case('add', 'add-n%d' % n, [make_op(L.OP_ADD, [0, 1], (n,))], [a, b_], n=n)


def _add_cases():
    return [add_case(n) for n in (1, 255, 4096 * 256 + 5)]


def _add_reference(case, dt):
    m, b = case.meta, case.bufs
    out = b[0].copy()
    out[:m.n] = (b[0][:m.n].astype(dt) + b[1][:m.n].astype(dt)).astype(np.float32)
    return {'dst': out}


def _add_extract(case, bufs):
    return {'dst': f32(bufs, 0)[:case.meta.n + SLACK]}


def _flat_views(case, name, a):
    if a.ndim == 2:                                  # rset: per output row and 64-column block; rfix: per row and 1024-column block
        size = 64 if case.family == 'rset' else 1024
        return [(blocked(a, 1, size), [(0,), (1,), (0, 1)])]
    return [(a, [tuple(range(a.ndim))])]


# ---- the table ------------------------------------------------------------------------------------------------------------------
_FWD_NAMES = ('out', 'sq', 'bp', 'norms', 'loss', 'ratio', 'bound', 'X', 'dst', 'norms_atomic', 'loss_atomic')
_FAMILIES = {
    'tilef': (_tilef_cases, _tile_extract, _tile_reference, _tile_views),
    'tileb': (_tileb_cases, _tile_extract, _tile_reference, _tile_views),
    'tileb16': (_tileb16_cases, _tile_extract, _tile_reference, _tile_views),
    'pnorm': (_pnorm_cases, _pnorm_extract, _pnorm_reference, _flat_views),
    'pfin': (_pfin_cases, _pfin_extract, _pfin_reference, _flat_views),
    'rfix': (_rfix_cases, _rfix_extract, _rfix_reference, _flat_views),
    'rset': (_rset_cases, _rset_extract, _rset_reference, _flat_views),
    'add': (_add_cases, _add_extract, _add_reference, _flat_views),
}


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(_FAMILIES[family][0]())


def all_cases():
    return [c for fam in _FAMILIES for c in cases(fam)]


def extract(case, bufs):
    """name -> array view of the case's results in `bufs` (byte arrays as run_interp returns, or the case's own buffers)."""
    return _FAMILIES[case.family][1](case, bufs)


@functools.lru_cache(maxsize=None)
def _reference(case_name, dtype):
    case = next(c for c in all_cases() if c.name == case_name)
    return _FAMILIES[case.family][2](case, dtype)


def reference(case, dtype=np.float64):
    """The independent evaluation of the case in `dtype`, results rounded to float32 as every buffer is (computed once per case:
    do not modify)."""
    return _reference(case.name, dtype)


def formula(case, dtype):
    """The ops' own formulas with every intermediate in `dtype`: the restatements above."""
    return reference(case, dtype)


def measure(case, name, got, ref):
    """Worst per-slice error (util_parity.slice_errors) over the axes where this op's kernels can fail locally."""
    worst, where = 0.0, None
    got, ref = np.asarray(got), np.asarray(ref)
    if case.family == 'pnorm' and name == 'dflat':                     # per segment
        den = np.sqrt(sum(float((r.astype(np.float64) ** 2).sum()) for r in seg_split(case, ref)) / max(case.meta.n, 1))
        for k, (g_, r_) in enumerate(zip(seg_split(case, got), seg_split(case, ref))):
            e = float(np.linalg.norm(g_.astype(np.float64) - r_.astype(np.float64)))
            e = e if np.isfinite(e) else np.inf
            v = e / den if den > 0 else e
            if where is None or v > worst:
                worst, where = v, ('segment', k)
        return worst, where
    if name in ('sq', 'bp', 'norms', 'norms_atomic', 'ratio'):          # per block / per segment: every entry against its own value
        g64, r64 = got.astype(np.float64), ref.astype(np.float64)
        with np.errstate(invalid='ignore', divide='ignore'):
            e = np.where(r64 != 0, np.abs(g64 - r64) / np.abs(r64), np.abs(g64 - r64))
        e = np.where(np.isfinite(e), e, np.inf)
        k = int(np.argmax(e)) if e.size else 0
        return (float(e[k]) if e.size else 0.0), ('entry', k)
    views = _FAMILIES[case.family][3]
    for (g_, axes), (r_, _) in zip(views(case, name, got), views(case, name, ref)):
        v, w = slice_errors(g_, r_, axes)
        if where is None or v > worst:
            worst, where = v, (g_.shape, w)
    return worst, where


def rounded_names(case):
    """the float results of a case that are compared within a bound (16-bit codes are compared element-wise by the GPU test)"""
    return [k for k in reference(case) if not k.startswith('h16.')]


_FLOORS = {}


def floors(case):
    """name -> float32 floor of the case: the formulas in float32 against the same in float64, per slice."""
    if case.name not in _FLOORS:
        lo, hi = formula(case, np.float32), formula(case, np.float64)
        _FLOORS[case.name] = {k: measure(case, k, lo[k], hi[k])[0] for k in rounded_names(case)}
    return _FLOORS[case.name]


def cap(case, name):
    return FWD_CAP if name.split('.')[0] in _FWD_NAMES else GRAD_CAP


def bound(case, name):
    """8 x the float32 floor (another summation order), at least 1e-6, never looser than the published fp32 limit of the kind."""
    return min(max(FLOOR_FACTOR * floors(case)[name], MIN_BOUND), cap(case, name))
