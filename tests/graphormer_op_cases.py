"""Adversarial single-op cases for the Graphormer's attention, LayerNorm and gather / scatter ops (ghn3_amd/csrc/attention.hip,
elementwise.hip): the smallest shapes that still reach every branch of the launchers' dispatch, with inputs that are not
i.i.d.-only (scores up to ~ +-30 and one head with 8 x larger q.k, a LayerNorm row of mean 1000, a constant row, exact zeros in
front of ReLU / dact) and every output pre-filled with a sentinel (NaN; 0.25 where the op accumulates).

A case is one or more `ghn3_op` records over a list of numpy buffers.  It is shared by
  * tests/test_graphormer_op_cases_cpu.py: the float64 interpreter (tests/program_interp.py) against an independent evaluation
    (`reference(case, float64)`), the regime coverage of the table, and the float32 floor of every case (`floors`: the op's
    own formula, `formula`, in plain numpy float32 against float64);
  * tests/test_gpu_graphormer_ops.py: `ctx.run` on device copies against the interpreter on host copies, per slice (`measure`).
No GPU is touched here.

LayerNorm cases use eps = 2^-16 (1.53e-5): the constant row's rstd is then exactly 256 and the comparison of two float64
evaluations is not blurred by the float32 rounding of a saved statistic.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
from scipy.special import erf

from ghn3_amd import _lib as L
from util_parity import slice_errors

NAN = np.float32('nan')
SENT = np.float32(0.25)               # sentinel of accumulated buffers
LN_EPS = 2.0 ** -16
FWD_CAP, GRAD_CAP = 2e-5, 2e-4        # the project's published per-tensor fp32 limits (tests/test_gpu_parity.py), here per slice
FLOOR_FACTOR, MIN_BOUND = 8.0, 1e-6


# ---- plumbing -----------------------------------------------------------------------------------------------------------
def make_op(kind, refs, i=(), f=()):
    """One ghn3_op; refs: buffer index, (buffer index, byte offset) or None."""
    op = np.zeros(1, dtype=L.OP_DT)
    op['r']['buf'][:] = -1
    op['kind'] = kind
    for j, r in enumerate(refs):
        if r is None:
            continue
        buf, off = r if isinstance(r, tuple) else (r, 0)
        op['r']['buf'][0][j], op['r']['off'][0][j] = buf, off
    op['i'][0][:len(i)] = i
    op['f'][0][:len(f)] = f
    return op


def _case(family, name, ops, bufs, **meta):
    return SimpleNamespace(family=family, name=name, ops=np.concatenate(ops), bufs=[np.ascontiguousarray(b) for b in bufs],
                           meta=SimpleNamespace(**meta))


def host_bytes(case):
    return [b.copy().reshape(-1).view(np.uint8) for b in case.bufs]


def run_interp(case):
    """The case through the float64 interpreter on host copies -> the buffers as byte arrays."""
    from program_interp import Interp
    host = host_bytes(case)
    Interp(host).run(case.ops, None)
    return host


def f32(bufs, k, off=0):
    return bufs[k].view(np.uint8)[off:].view(np.float32) if bufs[k].dtype == np.uint8 else bufs[k].reshape(-1).view(np.float32)[off // 4:]


def _seed(key):
    s = 17
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def blocked(a, axis, size):
    """`axis` of a cut into blocks of `size` (zero padded): (..., n_blocks, size, ...)."""
    n = a.shape[axis]
    nb = (n + size - 1) // size
    if nb * size != n:
        pad = [(0, 0)] * a.ndim
        pad[axis] = (0, nb * size - n)
        a = np.pad(a, pad)
    return a.reshape(a.shape[:axis] + (nb, size) + a.shape[axis + 1:])


# ---- attention ----------------------------------------------------------------------------------------------------------
# buffers: 0 out 1 qkv 2 bias 3 P 4 n_nodes 5 dqkv 6 dO 7 dBias 8 amax
ATTN_N = [1, 16, 17, 31, 32, 33, 97, 255, 256, 257, 300, 1056]
ATTN_HC = {3: (4, 12), 1: (2, 2), 4: (4, 16), 8: (2, 16), 12: (2, 24), 20: (2, 40), 24: (2, 48), 32: (1, 32)}


def _nn_pattern(N, B, pat):
    if B == 1:
        return [N - 1 if pat == 'mixed' and N > 1 else N]
    if pat == 'full':
        return [N] * B
    if pat == 'mixed':
        return [N, max(N - 1, 1), 1]
    if pat == 'bound':                           # ends exactly on a 16-row and on a 32-row boundary
        return [min(N, 16), min(N, 32), N]
    return [min(N, 17), min(N, 33), N]           # 'bound1': one past each


def attn_case(N, H, C, pat='full', bias=True, save_p=True, bwd=True, dbias=True, amax=True, general=0, misalign=False, B=None):
    d = C // H
    B = B or (1 if N > 1024 else 3)
    nn = _nn_pattern(N, B, pat)
    rs = np.random.RandomState(_seed(('attn', N, H, C, pat, general, misalign)))
    qkv = rs.standard_normal((B, N, 3, H, d)).astype(np.float32)
    qkv += (0.3 * np.sin(np.arange(N)))[None, :, None, None, None].astype(np.float32)          # not i.i.d.: a trend along the nodes
    qkv[:, :, :2, 0] *= np.float32(math.sqrt(8.0))                                              # one head with 8 x larger q.k
    bia = (3.0 * rs.standard_normal((B, H, N, N))).astype(np.float32)
    hot = rs.random_sample(bia.shape) < 0.02
    bia[hot] = np.where(rs.random_sample(int(hot.sum())) < 0.5, -30.0, 30.0).astype(np.float32)
    dO = (rs.standard_normal((B, N, H, d)) * (1.0 + np.arange(H))[None, None, :, None]).astype(np.float32)
    p = 1 if misalign else 0                      # one float in front of every float buffer: bases 4 bytes off 16

    def fb(a):
        return np.concatenate([np.full(p, 7.0, np.float32), np.asarray(a, np.float32).reshape(-1)])
    o4 = 4 * p
    bufs = [fb(np.full(B * N * C, NAN)), fb(qkv), fb(bia), fb(np.full(B * H * N * N, NAN)), np.asarray(nn, np.int32),
            fb(np.full(B * N * 3 * C, NAN)), fb(dO), fb(np.full(B * H * N * N, SENT)), np.zeros(4, np.float32)]
    ops = [make_op(L.OP_ATTN_FWD, [(0, o4), (1, o4), (2, o4) if bias else None, (3, o4) if save_p else None, 4], (B, N, C, H))]
    if bwd:
        assert save_p
        ops.append(make_op(L.OP_ATTN_BWD, [(5, o4), (6, o4), (1, o4), (3, o4), (0, o4), 8 if (dbias and amax) else None,
                                           (7, o4) if dbias else None, 4], (B, N, C, H, general)))
    name = 'attn-N%d-H%d-C%d-%s%s%s%s%s%s%s' % (N, H, C, pat, '' if bias else '-nobias', '' if save_p else '-noP',
                                               '' if bwd else '-fwdonly', '' if dbias else '-nodbias',
                                               '-general' if general else '', '-misaligned' if misalign else '')
    return _case('attn', name, ops, bufs, B=B, N=N, C=C, H=H, d=d, nn=nn, bias=bias, save_p=save_p, bwd=bwd, dbias=dbias and bwd,
                 amax=dbias and amax and bwd, general=general, misalign=misalign, off=o4)


def _attn_cases():
    pats = ['mixed', 'bound', 'bound1', 'full']
    out, k = [], 0
    for N in ATTN_N:                                              # every N at d = 8 and d = 24
        for dd in (8, 24):
            H, C = ATTN_HC[dd]
            out.append(attn_case(N, H, C, pats[k % 4], general=(k // 4) % 2))
            k += 1
    for dd in (3, 1, 4, 12, 20, 32):                              # every other d at N = 33 and N = 257
        for N in (33, 257):
            H, C = ATTN_HC[dd]
            out.append(attn_case(N, H, C, pats[k % 4], general=k % 2))
            k += 1
    out.append(attn_case(33, 16, 384, 'bound1'))                 # the released XL shape, once
    # variants
    out.append(attn_case(33, 2, 16, 'mixed', bias=False, save_p=False, bwd=False))
    out.append(attn_case(257, 2, 48, 'mixed', bias=False, save_p=False, bwd=False))
    out.append(attn_case(1056, 2, 16, 'mixed', bias=False, save_p=False, bwd=False))
    out.append(attn_case(97, 2, 48, 'mixed', dbias=False))
    out.append(attn_case(300, 2, 16, 'bound', dbias=False, general=1))
    out.append(attn_case(97, 2, 16, 'bound1', amax=False))
    out.append(attn_case(256, 2, 48, 'mixed', general=1))        # the general kernel where the staged one would run
    out.append(attn_case(64, 2, 48, 'mixed', misalign=True))     # vec = 0 at a head dim that is otherwise vectorised
    out.append(attn_case(300, 2, 16, 'mixed', misalign=True))
    return out


def _attn_extract(case, bufs):
    m = case.meta
    B, N, C, H, d, o = m.B, m.N, m.C, m.H, m.d, m.off
    res = {'out': f32(bufs, 0, o)[:B * N * C].reshape(B, N, H, d)}
    if m.save_p:
        res['P'] = f32(bufs, 3, o)[:B * H * N * N].reshape(B, H, N, N)
    if m.bwd:
        res['dqkv'] = f32(bufs, 5, o)[:B * N * 3 * C].reshape(B, N, 3, H, d)
        if m.dbias:
            res['dBias'] = f32(bufs, 7, o)[:B * H * N * N].reshape(B, H, N, N)
    return res


def _attn_reference(case, dtype):
    """softmax(Q K^T d^-1/2 + bias) V with the key mask and its autograd gradients, torch on the CPU in `dtype`."""
    m = case.meta
    B, N, C, H, d, o = m.B, m.N, m.C, m.H, m.d, m.off
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    qkv = torch.from_numpy(f32(case.bufs, 1, o)[:B * N * 3 * C].reshape(B, N, 3, H, d).copy()).to(tdt).requires_grad_(True)
    bia = torch.from_numpy(f32(case.bufs, 2, o)[:B * H * N * N].reshape(B, H, N, N).copy()).to(tdt).requires_grad_(True)
    nn = torch.tensor(m.nn)
    valid = torch.arange(N)[None, :] < nn[:, None]
    mask = (valid[:, :, None] & valid[:, None, :])[:, None]
    q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
    s = (q @ k.transpose(-1, -2)) * d ** -0.5
    if m.bias:
        s = s + bia
    s = s.masked_fill(~mask, -32768.0)
    p = torch.softmax(s, -1)
    out = (p @ v).permute(0, 2, 1, 3)
    res = {'out': out.detach().numpy().astype(np.float32)}
    if m.save_p:
        res['P'] = p.detach().numpy().astype(np.float32)
    if m.bwd:
        # the backward op consumes the SAVED float32 probabilities and outputs (r3, r4): autograd through out = P V from that
        # leaf gives dP and dV, dS = P (dP - rowsum(dO O)) inside the mask, autograd through the scores gives dQ and dK
        dO = torch.from_numpy(f32(case.bufs, 6, o)[:B * N * C].reshape(B, N, H, d).copy()).to(tdt)
        ps = p.detach().float().to(tdt).requires_grad_(True)
        ((ps @ v).permute(0, 2, 1, 3) * dO).sum().backward(retain_graph=True)
        dv = qkv.grad.clone()
        qkv.grad = None
        delta = (dO * out.detach().float().to(tdt)).sum(-1).permute(0, 2, 1)[..., None]
        dS = (ps.detach() * (ps.grad - delta)).masked_fill(~mask, 0.0)
        ((q @ k.transpose(-1, -2)) * d ** -0.5).backward(dS)
        res['dqkv'] = (qkv.grad + dv).numpy().astype(np.float32)
        if m.dbias:
            res['dBias'] = (dS + float(SENT)).numpy().astype(np.float32)
    return res


def attn_valid(case, name, a, b):
    """graph b of an attention result cut to its valid nodes (a leading axis of length 1 is kept)"""
    n = case.meta.nn[b]
    return a[b:b + 1, :n] if name in ('out', 'dqkv') else a[b:b + 1, :, :n, :n]


def _attn_views(case, name, a):
    """Per graph, per head, per 16- and per 32-row query block, per 32-key block, per q / k / v third."""
    v = []
    for qb in (16, 32):
        if name == 'out':                                     # (B, N, H, d)
            v.append((blocked(a, 1, qb), [(0,), (3,), (0, 1, 3)]))
        elif name == 'dqkv':                                  # (B, N, 3, H, d)
            v.append((blocked(a, 1, qb), [(0,), (3,), (4,), (0, 1, 3, 4)]))
        else:                                                 # P, dBias (B, H, N, N)
            v.append((blocked(blocked(a, 3, 32), 2, qb), [(0,), (1,), (0, 1, 2, 4)]))
    return v


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------
# buffers: 0 y 1 x 2 gamma 3 beta 4 mean 5 rstd 6 planes(fwd) 7 dx 8 dy 9 mean_in 10 rstd_in 11 residual 12 planes(bwd)
def seq_sum(x, planes, n, stride, rows, C):
    """x + planes in plane order, float32 throughout (what the header promises for the in-place sums)."""
    acc = x.astype(np.float32).copy()
    for p in range(n):
        acc = (acc + planes[p * stride:p * stride + rows * C].reshape(rows, C)).astype(np.float32)
    return acc


def ln_case(rows, C, planes=None, stats=True, residual=True):
    """planes: None = absent, 0 = present with i2 = 0 (meaning 1), else their number."""
    rs = np.random.RandomState(_seed(('ln', rows, C, planes, stats, residual)))
    n_pl = 0 if planes is None else max(1, planes)
    stride = rows * C + 5
    target = (rs.standard_normal((rows, C)) * (0.5 + rs.random_sample((rows, 1))) + rs.standard_normal((rows, 1))).astype(np.float32)
    grid = lambda a: (np.round(np.asarray(a) * 64) / 64).astype(np.float32)
    special = {}
    if rows > 1 and C > 1:                        # mean exactly 1000, unit spread, everything on a 2^-6 grid
        u = grid(rs.standard_normal(C))
        u[-1] = -u[:-1].sum()
        target[1] = 1000.0 + u
        special['big'] = 1
    if rows > 2:
        target[2] = 0.75                          # constant row: variance 0
        special['const'] = 2
    pl = rs.standard_normal((max(n_pl, 1), stride)).astype(np.float32) * 0.5
    x0 = target.copy()
    if n_pl:
        for r in special.values():               # special rows: planes on the grid, x0 = target - sum (all exact in fp32)
            for p in range(n_pl):
                pl[p, r * C:(r + 1) * C] = grid(pl[p, r * C:(r + 1) * C])
            x0[r] = target[r] - sum(pl[p, r * C:(r + 1) * C].astype(np.float64) for p in range(n_pl))
    xs = seq_sum(x0, pl.reshape(-1), n_pl, stride, rows, C)
    for r in special.values():
        assert (xs[r] == target[r]).all()
    gamma = (1.0 + 0.3 * rs.standard_normal(C)).astype(np.float32)
    beta = (0.2 * rs.standard_normal(C)).astype(np.float32)
    x64 = xs.astype(np.float64)
    mean_in = x64.mean(1).astype(np.float32)
    rstd_in = (1.0 / np.sqrt(x64.var(1) + LN_EPS)).astype(np.float32)
    dy = (rs.standard_normal((rows, C)) * (1.0 + (np.arange(C) % 7 == 0))).astype(np.float32)
    pl2 = rs.standard_normal((max(n_pl, 1), stride)).astype(np.float32) * 0.5
    res = rs.standard_normal((rows, C)).astype(np.float32)
    bufs = [np.full(rows * C, NAN), x0, gamma, beta, np.full(rows, NAN), np.full(rows, NAN), pl.reshape(-1),
            np.full(rows * C, NAN), dy, mean_in, rstd_in, res, pl2.reshape(-1)]
    i = (rows, C, 0 if planes is None else planes, stride)
    ops = [make_op(L.OP_LAYERNORM_FWD, [0, 1, 2, 3, 4 if stats else None, 5 if stats else None, None if planes is None else 6],
                   i, (LN_EPS,)),
           make_op(L.OP_LAYERNORM_BWD, [7, 8, 1, 2, 9, 10, 11 if residual else None, None if planes is None else 12], i)]
    name = 'ln-r%d-C%d-planes%s%s%s' % (rows, C, planes, '' if stats else '-nostats', '' if residual else '-nores')
    return _case('ln', name, ops, [np.asarray(b, np.float32) for b in bufs], rows=rows, C=C, planes=planes, n_pl=n_pl,
                 stride=stride, stats=stats, residual=residual, special=special)


def _ln_cases():
    out, k = [], 0
    pls = [None, 0, 1, 7, 8, 9]
    for C in (4, 63, 64, 65, 384, 512, 513, 772):
        for rows in ((5,) if C not in (65, 513) else (1, 3, 5, 257)):
            out.append(ln_case(rows, C, pls[k % 6], stats=k % 3 != 2, residual=k % 2 == 0))
            k += 1
    for C in (65, 384, 772):                                      # every plane count on a register-resident and on a loop row
        for pl in pls:
            if not any(c.meta.C == C and c.meta.planes == pl and c.meta.rows == 5 for c in out):
                out.append(ln_case(5, C, pl, stats=k % 3 != 2, residual=k % 2 == 0))
                k += 1
    return out


def _ln_sums(case):
    m = case.meta
    x = seq_sum(case.bufs[1].reshape(m.rows, m.C), case.bufs[6], m.n_pl, m.stride, m.rows, m.C)
    dy = seq_sum(case.bufs[8].reshape(m.rows, m.C), case.bufs[12], m.n_pl, m.stride, m.rows, m.C)
    return x, dy


def _ln_extract(case, bufs):
    m = case.meta
    r = {'y': f32(bufs, 0)[:m.rows * m.C].reshape(m.rows, m.C), 'dx': f32(bufs, 7)[:m.rows * m.C].reshape(m.rows, m.C)}
    if m.stats:
        r['mean'], r['rstd'] = f32(bufs, 4)[:m.rows], f32(bufs, 5)[:m.rows]
    return r


def _ln_reference(case, dtype):
    """F.layer_norm and its autograd gradient (+ residual), torch on the CPU in `dtype`, on the sequentially summed rows."""
    m = case.meta
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    xs, dys = _ln_sums(case)
    x = torch.from_numpy(xs).to(tdt).requires_grad_(True)
    g, b = (torch.from_numpy(case.bufs[k]).to(tdt) for k in (2, 3))
    y = torch.nn.functional.layer_norm(x, (m.C,), g, b, LN_EPS)
    (y * torch.from_numpy(dys).to(tdt)).sum().backward()
    dx = x.grad
    if m.residual:
        dx = dx + torch.from_numpy(case.bufs[11].reshape(m.rows, m.C)).to(tdt)
    r = {'y': y.detach().numpy().astype(np.float32), 'dx': dx.numpy().astype(np.float32)}
    if m.stats:
        xd = x.detach()
        mu = xd.mean(1)
        r['mean'] = mu.numpy().astype(np.float32)
        r['rstd'] = (1.0 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(1) + LN_EPS)).numpy().astype(np.float32)
    return r


def _ln_views(case, name, a):
    if a.ndim == 1:
        return [(a, [(0,)])]
    return [(blocked(a, 1, 64), [(0,), (1,), (0, 1)])]       # per row, per 64-channel group, per (row, group)


# ---- LayerNorm parameter gradients ------------------------------------------------------------------------------------------
# single: 0 dgamma 1 dbeta 2 dy 3 x 4 mean 5 rstd.   batch: 0 gradients 1 activations 2 table; + one single op per item behind
def _lnpg_data(rs, rows, C):
    x = (rs.standard_normal((rows, C)) * 1.5 + rs.standard_normal((rows, 1))).astype(np.float32)
    dy = (rs.standard_normal((rows, C)) + 0.5).astype(np.float32)          # (a common sign: sums that grow)
    x64 = x.astype(np.float64)
    return dy, x, x64.mean(1).astype(np.float32), (1.0 / np.sqrt(x64.var(1) + LN_EPS)).astype(np.float32)


def lnpg_case(rows, C, accum):
    rs = np.random.RandomState(_seed(('lnpg', rows, C, accum)))
    dy, x, mu, rstd = _lnpg_data(rs, rows, C)
    fill = SENT if accum else NAN
    bufs = [np.full(C, fill, np.float32), np.full(C, fill, np.float32), dy, x, mu, rstd]
    return _case('lnpg', 'lnpg-r%d-C%d-accum%d' % (rows, C, accum), [make_op(L.OP_LN_PARAM_GRAD, [0, 1, 2, 3, 4, 5], (rows, C, accum))],
                 bufs, rows=rows, C=C, accum=accum, batch=0)


def lnpg_batch_case(rows=37, C=40, n=3):
    """GHN3_OP_LN_PARAM_GRAD_BATCH on zeroed gradients, items at scattered non-monotone offsets; behind it one single op with
    accum = 0 per item into buffers 3 (dgamma) and 4 (dbeta): the two must agree bit for bit."""
    rs = np.random.RandomState(_seed(('lnpgb', rows, C, n)))
    per = 2 * rows * C + 2 * rows + 3
    order = [2, 0, 1][:n]
    act = np.zeros(n * per + 8, np.float32)
    grads = np.zeros(2 * n * C + 11, np.float32)
    table = np.zeros((n, 6), np.int64)
    singles = []
    for t in range(n):
        dy, x, mu, rstd = _lnpg_data(rs, rows, C)
        a0 = order[t] * per + 1                     # (odd float offsets: nothing is 16-byte aligned)
        offs = [a0, a0 + rows * C, a0 + 2 * rows * C, a0 + 2 * rows * C + rows]
        for o_, v in zip(offs, (dy, x, mu, rstd)):
            act[o_:o_ + v.size] = v.reshape(-1)
        g0 = (n - 1 - order[t]) * 2 * C + 3
        table[t] = (g0 + C, g0, *offs)              # dgamma behind dbeta
        singles.append(make_op(L.OP_LN_PARAM_GRAD, [(3, 4 * t * C), (4, 4 * t * C)] + [(1, 4 * o_) for o_ in offs], (rows, C, 0)))
    bufs = [grads, act, table.reshape(-1), np.full(n * C, NAN, np.float32), np.full(n * C, NAN, np.float32)]
    ops = [make_op(L.OP_LN_PARAM_GRAD_BATCH, [0, 1, 2], (n, rows, C))] + singles
    return _case('lnpg', 'lnpg-batch-r%d-C%d-n%d' % (rows, C, n), ops, bufs, rows=rows, C=C, accum=1, batch=n, table=table)


def _lnpg_cases():
    out = []
    for k, rows in enumerate((1, 15, 16, 17, 128, 129, 300)):
        out.append(lnpg_case(rows, 17, k % 2))
    for k, C in enumerate((1, 15, 16, 384)):
        out.append(lnpg_case(129, C, (k + 1) % 2))
    out.append(lnpg_case(300, 384, 1))
    out.append(lnpg_batch_case())
    return out


def _lnpg_extract(case, bufs):
    m = case.meta
    if not m.batch:
        return {'dgamma': f32(bufs, 0)[:m.C], 'dbeta': f32(bufs, 1)[:m.C]}
    g = f32(bufs, 0)
    return {'dgamma': np.stack([g[t[0]:t[0] + m.C] for t in m.table]), 'dbeta': np.stack([g[t[1]:t[1] + m.C] for t in m.table])}


def _lnpg_reference(case, dtype):
    m = case.meta

    def one(dy, x, mu, rstd, base):
        dy, x, mu, rstd = (np.asarray(a, dtype) for a in (dy, x, mu, rstd))
        xh = (x - mu[:, None]) * rstd[:, None]
        return ((dtype(base) + (dy * xh).sum(0, dtype=dtype)).astype(np.float32), (dtype(base) + dy.sum(0, dtype=dtype)).astype(np.float32))
    if not m.batch:
        dg, db = one(case.bufs[2], case.bufs[3], case.bufs[4], case.bufs[5], SENT if m.accum else 0.0)
        return {'dgamma': dg, 'dbeta': db}
    act, r, C = case.bufs[1], m.rows, m.C
    res = [one(act[t[2]:t[2] + r * C].reshape(r, C), act[t[3]:t[3] + r * C].reshape(r, C), act[t[4]:t[4] + r], act[t[5]:t[5] + r], 0.0)
           for t in m.table]
    return {'dgamma': np.stack([a for a, _ in res]), 'dbeta': np.stack([b for _, b in res])}


def _cols16_views(case, name, a):
    return [(blocked(a, a.ndim - 1, 16), [tuple(range(a.ndim))])]     # per 16-column block (per item)


# ---- gather / scatter ops ---------------------------------------------------------------------------------------------------
def gather_case(B, N, H, V=9):
    """GHN3_OP_BIAS_GATHER: 0 bias 1 T 2 pair"""
    rs = np.random.RandomState(_seed(('gather', B, N, H)))
    ldT = (H + 3) // 4 * 4
    T = rs.standard_normal((V * V, ldT)).astype(np.float32)
    pair = rs.randint(0, V * V, (B, N, N)).astype(np.int32)
    pair[:, :, -1] = V * V - 1                                       # the last table row, in the last column
    bufs = [np.full(B * H * N * N, NAN, np.float32), T, pair]
    return _case('gather', 'gather-B%d-N%d-H%d' % (B, N, H), [make_op(L.OP_BIAS_GATHER, [0, 1, 2], (B, N, H))], bufs,
                 B=B, N=N, H=H, ldT=ldT)


def _gather_cases():
    return [gather_case(2, 257, H) for H in (1, 3, 4, 16)] + [gather_case(1, 257, H) for H in (64, 65)] + \
        [gather_case(2, N, 3) for N in (1, 255, 256)] + [gather_case(2, 33, 65)]


def hist_case(V, have_amax, B=2, N=40, H=3):
    """GHN3_OP_BIAS_HIST: 0 dT 1 dBias 2 pair 3 scratch (int64 [V V H] + the amax float, zeroed)"""
    rs = np.random.RandomState(_seed(('hist', V, have_amax)))
    ldT = (H + 3) // 4 * 4
    ids = rs.choice(V * V, size=min(V * V, 12), replace=False)      # one id takes ~90 %, eleven share the rest, the others none
    pair = np.where(rs.random_sample((B, N, N)) < 0.9, ids[0], ids[rs.randint(1, len(ids), (B, N, N))] if len(ids) > 1 else ids[0])
    dB = (rs.standard_normal((B, H, N, N)) * 1e-3 * (1 + np.arange(H))[None, :, None, None]).astype(np.float32)
    dB[0, 0, 0, :8] = 0.0
    scratch = np.zeros(8 * V * V * H + 16, np.uint8)
    if have_amax:
        scratch[8 * V * V * H:8 * V * V * H + 4] = np.asarray([np.abs(dB).max()], np.float32).view(np.uint8)
    bufs = [np.full(V * V * ldT, SENT, np.float32), dB, pair.astype(np.int32), scratch]
    return _case('hist', 'hist-V%d-amax%d' % (V, have_amax), [make_op(L.OP_BIAS_HIST, [0, 1, 2, 3], (B, N, H, V, have_amax))], bufs,
                 B=B, N=N, H=H, V=V, ldT=ldT, have_amax=have_amax, amax=float(np.abs(dB).max()),
                 counts=np.bincount(pair.reshape(-1), minlength=V * V))


def _hist_cases():
    return [hist_case(V, a) for V in (9, 90, 91) for a in (0, 1)]


def edge_case(V, C):
    """0 hid 1 Pfw 2 Pbw (GHN3_OP_EDGE_HIDDEN); 3 dPfw 4 dPbw 5 dhid 6 hid_in (GHN3_OP_EDGE_HIDDEN_BWD)"""
    rs = np.random.RandomState(_seed(('edge', V, C)))
    Pfw = rs.standard_normal((V, C)).astype(np.float32)
    Pbw = rs.standard_normal((V, C)).astype(np.float32)
    Pbw[0, ::3] = -Pfw[0, ::3]                   # pre-activations exactly 0 (and exactly 0 + 0)
    Pfw[V - 1, 1::5] = 0.0
    Pbw[V - 1, 1::5] = 0.0
    hid = np.maximum(Pfw[:, None, :] + Pbw[None, :, :], 0).astype(np.float32)
    dhid = rs.standard_normal((V, V, C)).astype(np.float32)
    bufs = [np.full(V * V * C, NAN, np.float32), Pfw, Pbw, np.full(V * C, NAN, np.float32), np.full(V * C, NAN, np.float32), dhid, hid]
    ops = [make_op(L.OP_EDGE_HIDDEN, [0, 1, 2], (V, C)), make_op(L.OP_EDGE_HIDDEN_BWD, [3, 4, 5, 6], (V, C))]
    return _case('edge', 'edge-V%d-C%d' % (V, C), ops, bufs, V=V, C=C)


def _edge_cases():
    return [edge_case(V, 65) for V in (1, 5, 9)] + [edge_case(5, C) for C in (4, 63, 64, 384)]


EMB_ROWS = (6, 5, 4, 101, 101, 1001)              # rows of E_type, E_ch, E_sp, E_in, E_out, E_dist


def embed_case(C, one_row=False, B=3, N=12):
    """0 x 1 node_type 2 shape_idx 3 n_nodes 4 node_off 5..10 tables 11 deg_in 12 deg_out 13 dist0 (GHN3_OP_EMBED_NODES);
    14 dx, 15..20 table gradients (GHN3_OP_EMBED_BWD, sentinel 0.25)"""
    rs = np.random.RandomState(_seed(('embed', C, one_row)))
    nn = np.asarray([N, 7, 1], np.int32)[:B]
    total, cq = int(nn.sum()), C // 4
    noff = np.concatenate([[0], np.cumsum(nn)[:-1]]).astype(np.int32)
    if one_row:
        types, shp = np.full(total, 2, np.int32), np.full((total, 4), 1, np.int32)
        deg_in, deg_out, dist = (np.full(B * N, v, np.int32) for v in (100, 0, 1000))
    else:
        types = rs.randint(0, EMB_ROWS[0] - 1, total).astype(np.int32)          # (the last type row: nobody)
        shp = np.stack([rs.randint(0, EMB_ROWS[1] - 1, total), rs.randint(0, EMB_ROWS[1] - 1, total),
                        rs.randint(0, EMB_ROWS[2] - 1, total), rs.randint(0, EMB_ROWS[2] - 1, total)], 1).astype(np.int32)
        shp[0] = (3, 3, 2, 2)                                                    # both halves of a node on one row
        deg_in = rs.choice([0, 1, 2, 100], B * N).astype(np.int32)
        deg_out = rs.choice([0, 1, 3, 100], B * N).astype(np.int32)
        dist = rs.choice([0, 1, 5, 1000], B * N).astype(np.int32)
    widths = (C, cq, cq, C, C, C)
    tabs = [rs.standard_normal((r, w)).astype(np.float32) for r, w in zip(EMB_ROWS, widths)]
    dx = rs.standard_normal((B * N, C)).astype(np.float32)
    bufs = [np.full(B * N * C, NAN, np.float32), types, shp, nn, noff] + tabs + [deg_in, deg_out, dist, dx] + \
        [np.full((r, w), SENT, np.float32) for r, w in zip(EMB_ROWS, widths)]
    ops = [make_op(L.OP_EMBED_NODES, list(range(14)), (B, N, C)),
           make_op(L.OP_EMBED_BWD, [14, 1, 2, 3, 4, 15, 16, 17, 18, 19, 20, 11, 12, 13], (B, N, C) + EMB_ROWS[:3])]
    return _case('embed', 'embed-C%d%s' % (C, '-onerow' if one_row else ''), ops, bufs, B=B, N=N, C=C, nn=nn, noff=noff, widths=widths,
                 one_row=one_row)


def _embed_cases():
    return [embed_case(8), embed_case(260), embed_case(8, one_row=True), embed_case(512, one_row=True)]


def _embed_indexed(case):
    """per table: boolean [rows], which rows some valid node indexes"""
    m, b = case.meta, case.bufs
    idx = [[] for _ in range(6)]
    for g in range(m.B):
        for i in range(int(m.nn[g])):
            s, row = int(m.noff[g]) + i, g * m.N + i
            idx[0].append(b[1][s]); idx[1] += [b[2][s, 0], b[2][s, 1]]; idx[2] += [b[2][s, 2], b[2][s, 3]]
            idx[3].append(b[11][row]); idx[4].append(b[12][row]); idx[5].append(b[13][row])
    return [np.isin(np.arange(r), np.asarray(ix)) for r, ix in zip(EMB_ROWS, idx)]


def rowseg_case(C, ldx, ldo, accum):
    """GHN3_OP_ROWSEG_SUM: 0 out 1 X 2 seg_ptr 3 idx"""
    rs = np.random.RandomState(_seed(('rowseg', C, ldx, ldo, accum)))
    lens = [0, 1, 4, 5, 1000, 0, 3, 2]
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n_src = 300
    idx = rs.randint(0, n_src, int(seg[-1])).astype(np.int32)
    X = (rs.standard_normal((n_src, ldx)) + 0.25).astype(np.float32)
    out = np.full((len(lens), ldo), SENT if accum else NAN, np.float32)
    return _case('rowseg', 'rowseg-C%d-ldx%d-ldo%d-accum%d' % (C, ldx, ldo, accum),
                 [make_op(L.OP_ROWSEG_SUM, [0, 1, 2, 3], (len(lens), C, ldx, ldo, accum))], [out, X, seg, idx],
                 rows=len(lens), C=C, ldx=ldx, ldo=ldo, accum=accum, lens=lens)


def _rowseg_cases():
    return [rowseg_case(3, 5, 3, 0), rowseg_case(4, 8, 6, 1), rowseg_case(4, 7, 4, 0), rowseg_case(384, 388, 385, 1),
            rowseg_case(384, 384, 384, 0)]


def colsum_case(M, N, qs=None, stride=1, gather=False):
    """GHN3_OP_COLSUM: 0 out 1 X 2 row gather"""
    rs = np.random.RandomState(_seed(('colsum', M, N, qs, stride, gather)))
    ld, n_src = N + 3, M + 9
    X = (rs.standard_normal((n_src, ld)) + 0.5).astype(np.float32)
    g = rs.randint(0, n_src, M).astype(np.int32)
    g[M // 2] = g[0]                                # duplicates
    q, s = qs or (0, 0)
    n = np.arange(N)
    omap = (((n // q) * s + n % q) if q > 0 else n) * stride
    out = np.full(int(omap.max()) + 3, SENT, np.float32)
    return _case('colsum', 'colsum-M%d-N%d-q%s-stride%d-gather%d' % (M, N, qs, stride, gather),
                 [make_op(L.OP_COLSUM, [0, 1, 2 if gather else None], (M, N, ld, q, s, stride, 1))], [out, X, g],
                 M=M, N=N, ld=ld, q=q, s=s, stride=stride, gather=gather, omap=omap)


def _colsum_cases():
    out = []
    for k, M in enumerate((1, 255, 256, 257, 600)):
        out.append(colsum_case(M, 65, (5, 7) if k % 2 else None, 1 + k % 3, gather=k % 2 == 0))
    for k, N in enumerate((1, 63, 64)):
        out.append(colsum_case(257, N, (1, 2) if k % 2 == 0 else None, 2 - k % 2, gather=k % 2 == 1))
    return out


def dact_case(kind, M, N, ld, n_parts=0, rows_parts=0, amax=False):
    """GHN3_OP_DACT: 0 X 1 aux 2 amax 3 partial planes"""
    rs = np.random.RandomState(_seed(('dact', kind, M, N, ld, n_parts, amax)))
    X = rs.standard_normal((M, ld)).astype(np.float32)
    aux = (1.5 * rs.standard_normal((M, ld))).astype(np.float32)
    aux[:, ::3] = 0.0                               # pre-activations exactly 0
    aux[0, 1] = -0.0
    stride = M * N + 8
    parts = rs.standard_normal(max(n_parts, 1) * stride).astype(np.float32)
    ops = [make_op(L.OP_DACT, [0, 1, 2 if amax else None, 3 if n_parts else None], (M, N, ld, kind, n_parts, stride, rows_parts))]
    return _case('dact', 'dact-kind%d-M%d-N%d-ld%d-parts%d-amax%d' % (kind, M, N, ld, n_parts, amax), ops,
                 [X, aux, np.asarray([1e-3, 0, 0, 0], np.float32), parts], kind=kind, M=M, N=N, ld=ld, n_parts=n_parts,
                 rows_parts=rows_parts, stride=stride, amax=amax)


def _dact_cases():
    out = []
    for kind in (L.DACT_NONE, L.DACT_RELU, L.DACT_GELU):
        out.append(dact_case(kind, 70, 24, 24, amax=kind != L.DACT_NONE))        # vector layout, two workgroups
        out.append(dact_case(kind, 37, 23, 29, amax=kind == L.DACT_GELU))        # N != ld, N % 4 != 0: scalar
    out.append(dact_case(L.DACT_RELU, 37, 24, 28))                               # N % 4 == 0 but N != ld: scalar
    out.append(dact_case(L.DACT_RELU, 70, 24, 24, n_parts=3, rows_parts=41, amax=True))
    out.append(dact_case(L.DACT_GELU, 70, 24, 24, n_parts=9, rows_parts=69, amax=True))     # more planes than one batch of loads
    return out


# ---- numpy restatements of the gather / scatter ops ------------------------------------------------------------------------
def _gelu_grad(z):
    return 0.5 * (1 + erf(z / math.sqrt(2))) + z * np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def _simple_extract(case, bufs):
    m, fam = case.meta, case.family
    if fam == 'gather':
        return {'bias': f32(bufs, 0).reshape(m.B, m.H, m.N, m.N)}
    if fam == 'hist':
        return {'dT': f32(bufs, 0).reshape(m.V * m.V, m.ldT)}
    if fam == 'edge':
        return {'hid': f32(bufs, 0).reshape(m.V * m.V, m.C), 'dhid': f32(bufs, 5).reshape(m.V * m.V, m.C),
                'dPfw': f32(bufs, 3).reshape(m.V, m.C), 'dPbw': f32(bufs, 4).reshape(m.V, m.C)}
    if fam == 'embed':
        r = {'x': f32(bufs, 0).reshape(m.B * m.N, m.C)}
        for t in range(6):
            r['dE%d' % t] = f32(bufs, 15 + t).reshape(EMB_ROWS[t], m.widths[t])
        return r
    if fam == 'rowseg':
        return {'out': f32(bufs, 0).reshape(m.rows, m.ldo)}
    if fam == 'colsum':
        return {'out': f32(bufs, 0)}
    if fam == 'dact':
        return {'X': f32(bufs, 0).reshape(m.M, m.ld)}
    raise KeyError(fam)


def _simple_reference(case, dt):
    m, fam, b = case.meta, case.family, case.bufs
    A = lambda a: np.asarray(a, dt)
    if fam == 'gather':
        return {'bias': np.moveaxis(b[1][b[2]][..., :m.H], -1, 1).copy()}
    if fam == 'hist':
        dT = A(b[0]).reshape(-1, m.ldT).copy()
        acc = np.zeros((m.V * m.V, m.H), dt)
        for h in range(m.H):
            np.add.at(acc[:, h], b[2].reshape(-1), A(b[1])[:, h].reshape(m.B, -1).reshape(-1))
        dT[:, :m.H] += acc
        return {'dT': dT.astype(np.float32)}
    if fam == 'edge':
        hid = np.maximum(A(b[1])[:, None, :] + A(b[2])[None, :, :], 0)
        dh = np.where(b[6].reshape(m.V, m.V, m.C) > 0, A(b[5]).reshape(m.V, m.V, m.C), 0)
        return {'hid': hid.reshape(-1, m.C).astype(np.float32), 'dhid': dh.reshape(-1, m.C).astype(np.float32),
                'dPfw': dh.sum(1, dtype=dt).astype(np.float32), 'dPbw': dh.sum(0, dtype=dt).astype(np.float32)}
    if fam == 'embed':
        cq = m.C // 4
        x = np.zeros((m.B * m.N, m.C), dt)
        dE = [A(b[15 + t]).copy() for t in range(6)]
        T = [A(b[5 + t]) for t in range(6)]
        for g in range(m.B):
            for i in range(int(m.nn[g])):
                s, row = int(m.noff[g]) + i, g * m.N + i
                sh = b[2][s]
                x[row] = T[0][b[1][s]] + np.concatenate([T[1][sh[0]], T[1][sh[1]], T[2][sh[2]], T[2][sh[3]]]) + \
                    T[3][b[11][row]] + T[4][b[12][row]] + T[5][b[13][row]]
                gr = A(b[14][row])
                dE[0][b[1][s]] += gr
                for j in range(4):
                    dE[1 if j < 2 else 2][sh[j]] += gr[j * cq:(j + 1) * cq]
                dE[3][b[11][row]] += gr; dE[4][b[12][row]] += gr; dE[5][b[13][row]] += gr
        r = {'x': x.astype(np.float32)}
        r.update({'dE%d' % t: dE[t].astype(np.float32) for t in range(6)})
        return r
    if fam == 'rowseg':
        out = A(b[0]).copy()
        for r in range(m.rows):
            s = A(b[1])[b[3][b[2][r]:b[2][r + 1]], :m.C].sum(0, dtype=dt)
            out[r, :m.C] = s + (out[r, :m.C] if m.accum else 0)
        return {'out': out.astype(np.float32)}
    if fam == 'colsum':
        out = A(b[0]).copy()
        rows = b[2][:m.M] if m.gather else np.arange(m.M)
        out[m.omap] += A(b[1])[rows, :m.N].sum(0, dtype=dt)
        return {'out': out.astype(np.float32)}
    if fam == 'dact':
        X = b[0].copy()
        if m.n_parts:                                # plane order, float32 (deterministic by contract)
            for p in range(m.n_parts):
                X[:m.rows_parts] = X[:m.rows_parts] + b[3][p * m.stride:p * m.stride + m.rows_parts * m.N].reshape(m.rows_parts, m.N)
        v, z = A(X[:, :m.N]), A(b[1][:, :m.N])
        v = np.where(z > 0, v, 0) if m.kind == L.DACT_RELU else v * _gelu_grad(z) if m.kind == L.DACT_GELU else v
        X[:, :m.N] = v
        return {'X': X}
    raise KeyError(fam)


def _simple_views(case, name, a):
    fam = case.family
    if fam in ('gather',):
        return [(a, [(0,), (1,)])]
    if name in ('out',) and fam == 'colsum':
        return [(blocked(a, 0, 16), [(0,)])]
    if a.ndim == 2:                                  # per output row and per 64-column block
        return [(blocked(a, 1, 64), [(0,), (1,), (0, 1)])]
    return [(a, [tuple(range(a.ndim))])]


# ---- the table ------------------------------------------------------------------------------------------------------------------
_FAMILIES = {
    'attn': (_attn_cases, _attn_extract, _attn_reference, _attn_views, {'out': FWD_CAP, 'P': FWD_CAP}),
    'ln': (_ln_cases, _ln_extract, _ln_reference, _ln_views, {'y': FWD_CAP, 'mean': FWD_CAP, 'rstd': FWD_CAP}),
    'lnpg': (_lnpg_cases, _lnpg_extract, _lnpg_reference, _cols16_views, {}),
    'gather': (_gather_cases, _simple_extract, _simple_reference, _simple_views, {'bias': FWD_CAP}),
    'hist': (_hist_cases, _simple_extract, _simple_reference, _simple_views, {}),
    'edge': (_edge_cases, _simple_extract, _simple_reference, _simple_views, {'hid': FWD_CAP}),
    'embed': (_embed_cases, _simple_extract, _simple_reference, _simple_views, {'x': FWD_CAP}),
    'rowseg': (_rowseg_cases, _simple_extract, _simple_reference, _simple_views, {}),
    'colsum': (_colsum_cases, _simple_extract, _simple_reference, _simple_views, {}),
    'dact': (_dact_cases, _simple_extract, _simple_reference, _simple_views, {}),
}


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(_FAMILIES[family][0]())


def all_cases():
    return [c for fam in _FAMILIES for c in cases(fam)]


def extract(case, bufs):
    """name -> array view of the case's results in `bufs` (byte arrays as run_interp returns, or the case's own buffers)."""
    return _FAMILIES[case.family][1](case, bufs)


def reference(case, dtype):
    """The independent evaluation of the case in `dtype` (float64: the check of the interpreter; torch autograd for attention and
    LayerNorm), results rounded to float32 as every buffer is."""
    return _FAMILIES[case.family][2](case, dtype)


def measure(case, name, got, ref):
    """Worst per-slice error (util_parity.slice_errors) over the axes where this op's kernels can fail locally."""
    worst, where = 0.0, None
    got, ref = np.asarray(got), np.asarray(ref)
    for (g, axes), (r, _) in zip(_FAMILIES[case.family][3](case, name, got), _FAMILIES[case.family][3](case, name, ref)):
        v, w = slice_errors(g, r, axes)
        if where is None or v > worst:
            worst, where = v, (g.shape, w)
    return worst, where


# ---- the ops' own formulas in plain numpy, in `dtype`: the float32 floor ------------------------------------------------------
def _attn_formula(case, dtype):
    """GHN3_OP_ATTN_FWD / _BWD as include/ghn3_hip.h and the interpreter state them, every intermediate in `dtype`: the backward
    consumes the saved float32 P and O, delta = rowsum(dO * O), dS = P (dO V^T - delta) inside the mask."""
    m = case.meta
    B, N, C, H, d, o = m.B, m.N, m.C, m.H, m.d, m.off
    scale = dtype(d ** -0.5)
    qkv = f32(case.bufs, 1, o)[:B * N * 3 * C].reshape(B, N, 3, H, d).astype(dtype)
    q, k, v = (qkv[:, :, j].transpose(0, 2, 1, 3) for j in range(3))
    nn = np.asarray(m.nn)
    valid = np.arange(N)[None, :] < nn[:, None]
    mask = (valid[:, :, None] & valid[:, None, :])[:, None]
    s = np.matmul(q, k.transpose(0, 1, 3, 2)) * scale
    if m.bias:
        s = s + f32(case.bufs, 2, o)[:B * H * N * N].reshape(B, H, N, N).astype(dtype)
    s = np.where(mask, s, dtype(-32768.0))
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True, dtype=dtype)
    out = np.matmul(p, v)
    assert p.dtype == dtype and out.dtype == dtype
    res = {'out': out.transpose(0, 2, 1, 3).astype(np.float32)}
    if m.save_p:
        res['P'] = p.astype(np.float32)
    if m.bwd:
        P, O = p.astype(np.float32).astype(dtype), out.astype(np.float32).astype(dtype)
        dO = f32(case.bufs, 6, o)[:B * N * C].reshape(B, N, H, d).astype(dtype).transpose(0, 2, 1, 3)
        dV = np.matmul(P.transpose(0, 1, 3, 2), dO)
        dP = np.matmul(dO, v.transpose(0, 1, 3, 2))
        delta = (dO * O).sum(-1, keepdims=True, dtype=dtype)
        dS = np.where(mask, P * (dP - delta), dtype(0))
        dQ = np.matmul(dS, k) * scale
        dK = np.matmul(dS.transpose(0, 1, 3, 2), q) * scale
        assert dS.dtype == dtype and dQ.dtype == dtype
        res['dqkv'] = np.stack([dQ, dK, dV], 0).transpose(1, 3, 0, 2, 4).astype(np.float32)
        if m.dbias:
            res['dBias'] = (dtype(SENT) + dS).astype(np.float32)
    return res


def _ln_formula(case, dtype):
    """GHN3_OP_LAYERNORM_FWD / _BWD as the interpreter states them (the backward from the given mean / rstd), in `dtype`."""
    m = case.meta
    xs, dys = _ln_sums(case)
    x, dy = xs.astype(dtype), dys.astype(dtype)
    g, b = case.bufs[2].astype(dtype), case.bufs[3].astype(dtype)
    mu = x.mean(1, dtype=dtype)
    rs = dtype(1) / np.sqrt(((x - mu[:, None]) ** 2).mean(1, dtype=dtype) + dtype(LN_EPS))
    y = (x - mu[:, None]) * rs[:, None] * g + b
    mu_in, rs_in = case.bufs[9].astype(dtype)[:, None], case.bufs[10].astype(dtype)[:, None]
    xh = (x - mu_in) * rs_in
    dg = dy * g
    dx = rs_in * (dg - dg.mean(1, keepdims=True, dtype=dtype) - xh * (dg * xh).mean(1, keepdims=True, dtype=dtype))
    if m.residual:
        dx = dx + case.bufs[11].reshape(m.rows, m.C).astype(dtype)
    assert y.dtype == dtype and dx.dtype == dtype
    r = {'y': y.astype(np.float32), 'dx': dx.astype(np.float32)}
    if m.stats:
        r['mean'], r['rstd'] = mu.astype(np.float32), rs.astype(np.float32)
    return r


def formula(case, dtype):
    """The op's own formula in plain numpy with every intermediate in `dtype` (attention and LayerNorm: restated above; the other
    ops: their numpy restatement)."""
    fn = {'attn': _attn_formula, 'ln': _ln_formula}.get(case.family)
    return fn(case, dtype) if fn else reference(case, dtype)


_FLOORS = {}


def floors(case):
    """name -> float32 floor of the case: the op's formula in plain numpy float32 against the same in float64, per slice."""
    if case.name not in _FLOORS:
        lo, hi = formula(case, np.float32), formula(case, np.float64)
        _FLOORS[case.name] = {k: measure(case, k, lo[k], hi[k])[0] for k in hi}
    return _FLOORS[case.name]


def cap(case, name):
    return _FAMILIES[case.family][4].get(name, GRAD_CAP)


def bound(case, name):
    """8 x the float32 floor (another summation order: MFMA k-groups, wave and LDS reduction trees), at least 1e-6 (exactly
    representable cases do not demand bit equality), never looser than the published fp32 limit of the tensor's kind."""
    return min(max(FLOOR_FACTOR * floors(case)[name], MIN_BOUND), cap(case, name))
