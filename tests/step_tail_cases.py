"""Adversarial op-level cases for the end of the training step (ghn3_amd/csrc/elementwise.hip): GHN3_OP_SUMSQ at sizes that make
a lane go round its grid-stride loop twice, the four AdamW kinds (fp32 / bf16 state, flat / over a cast-descriptor table), the
two local passes of the gradient exchange (GHN3_OP_WIRE_PACK, GHN3_OP_RANK_REDUCE) and the utilities GHN3_OP_TRANSPOSE32,
GHN3_OP_GRAPH_PROLOGUE and GHN3_OP_MEMSET0.

A case is a list of `ghn3_op` records over numpy buffers plus an IMAGE: what every buffer must hold afterwards, written from
the text of include/ghn3_hip.h alone (`Case.image(dtype)`; it never reads the op records and imports nothing from
ghn3_amd.optim or tests/program_interp.py).  Everything outside a case's `loose` regions must equal the image bit for bit --
slack in front of and behind every range, gaps between descriptors, padding columns, whole input buffers; in-place outputs
are surrounded by the value 7, pure outputs are pre-filled with NaN patterns, accumulated ones with 0.25.  Loose regions:

  'float'  fp32 results compared per 1024-element span with the float64 image: ||got - ref|| / ||ref|| of the span (absolute
           for an all-zero span) <= max(8 x the span's float32 floor, 1e-6), never above 2e-5; the floor is `image(float32)`,
           the op's formula in plain numpy float32, against `image(float64)`;
  'entry'  single floats (sums) against their own value, same bound;
  'nan'    elements that must hold a NaN (with the given sign where one is given), whatever its payload;
  'free'   scratch, and 16-bit copies that are compared with the cast of the run's OWN updated parameters (`copy_image`).

The hyper-parameters of the AdamW kinds travel as doubles and are rounded to float on entry; 1 - beta is formed from the
rounded beta (include/ghn3_hip.h).  The float64 image does the same: with beta2 = 0.999 the float 1 - beta2 differs from
0.001 by 1.3e-5, which is a property of the op's interface and not an error of its arithmetic.

bf16-state kinds: `s16_eval` is a second restatement of the rule in the header (widen, the fp32 update with one rounding per
operation and fused multiply-adds for the two moment updates, mix32 hash, (bits + r16) >> 16), exact to the bit.  The CPU test
holds it against ghn3_amd.optim.adamw_state16_reference_ / state16_random_bits, so that the two restatements check each other.
A flat index at or above 2^32 needs an 8 GB state buffer and stays untested.

No input makes a float32 intermediate subnormal (|g * clip| >= 1e-15 wherever it is not 0, v either 0 or normal).

Large cases (`BIG`) are built inside their test from a short pattern, tiled and scaled by position; nothing large exists at
import or collection time.  No GPU is touched here.
"""
import functools
from types import SimpleNamespace

import numpy as np

from ghn3_amd import _lib as L
from graphormer_op_cases import SENT, FWD_CAP, FLOOR_FACTOR, MIN_BOUND, make_op, _seed

SLACK = 16
KEEP = np.float32(7.0)                                # slack around in-place buffers
NANBITS = 0x7fc00123                                  # sentinel of fp32 outputs (a NaN)
SENT16 = 0xabcd                                       # sentinel of 16-bit outputs (not a value any case produces)
SPAN = 1024
BETAS, EPS = (0.9, 0.999), 1e-8
f32 = np.float32

r64 = lambda v: (v + 63) // 64 * 64
r8 = lambda v: (v + 7) // 8 * 8


def dbits(x):
    return int(np.float64(x).view(np.int64))


def nan_f32(n):
    return np.full(n, NANBITS, np.uint32).view(np.float32)


# ---- the case -----------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, family, name, regimes=()):
        self.family, self.name, self.regimes = family, name, set(regimes)
        self.bufs, self._ops, self.loose, self.shift, self._writers, self._img = [], [], [], {}, [], {}
        self.also_float = []                              # (name, buf, idx, ref(dt)): bit-exact results also held against float64
        self.rerun, self.refused = True, False
        self.meta = SimpleNamespace()
        self.problems = np.zeros(0, dtype=L.PROBLEM_DT)

    def add(self, arr, shift=0):
        """a buffer; shift: the op sees it `shift` bytes behind its (16-byte aligned) start"""
        self.bufs.append(np.ascontiguousarray(arr))
        if shift:
            self.shift[len(self.bufs) - 1] = shift
        return len(self.bufs) - 1

    def op(self, kind, refs, i=(), f=()):
        self._ops.append(make_op(kind, refs, i, f))

    def writer(self, fn):
        self._writers.append(fn)

    def region(self, kind, name, buf, idx, **kw):
        self.loose.append(SimpleNamespace(kind=kind, name=name, buf=buf, idx=np.asarray(idx, np.int64).reshape(-1), **kw))

    @property
    def ops(self):
        return np.concatenate(self._ops)

    def image(self, dt=np.float64):
        """what every buffer holds after the ops, evaluated in `dt` and rounded to the buffers' types.  Do not modify."""
        if dt not in self._img:
            img = [b.copy() for b in self.bufs]
            for w in self._writers:
                w(img, dt)
            self._img[dt] = img
        return self._img[dt]


def host_bytes(case):
    return [b.copy().reshape(-1).view(np.uint8) for b in case.bufs]


def op_views(case, host):
    """the buffers as the ops see them (pointer shifts applied), sharing memory with `host`"""
    return [h[case.shift.get(k, 0):] for k, h in enumerate(host)]


def run_interp(case):
    from program_interp import Interp
    host = host_bytes(case)
    Interp(op_views(case, host)).run(case.ops, case.problems)
    return host


def typed(case, bufs, k):
    return bufs[k].reshape(-1).view(np.uint8).view(case.bufs[k].dtype)


def strict_mask(case, k):
    m = np.ones(case.bufs[k].size, bool)
    for r in case.loose:
        if r.buf == k:
            m[r.idx] = False
    return m


def span_errors(got, ref):
    """per 1024-element span: ||got - ref|| / ||ref|| (absolute where the reference span is all zero); inf for a NaN"""
    g, r = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    nb = (g.size + SPAN - 1) // SPAN
    pad = nb * SPAN - g.size
    if pad:
        g, r = np.concatenate([g, np.zeros(pad)]), np.concatenate([r, np.zeros(pad)])
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.sqrt(((g - r) ** 2).reshape(nb, SPAN).sum(1))
        d = np.sqrt((r * r).reshape(nb, SPAN).sum(1))
        rel = np.where(d > 0, e / np.where(d > 0, d, 1.0), e)
    return np.where(np.isfinite(rel), rel, np.inf)


def entry_errors(got, ref):
    g, r = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.where(r != 0, np.abs(g - r) / np.abs(r), np.abs(g - r))
    return np.where(np.isfinite(e), e, np.inf)


def bounds_of(floor):
    return np.minimum(np.maximum(FLOOR_FACTOR * np.asarray(floor), MIN_BOUND), FWD_CAP)


def float_checks(case):
    """(name, buf, idx, float64 reference, float32 floor per span / entry, error function) of every result held against float64"""
    out = []
    lo, hi = case.image(np.float32), case.image(np.float64)
    for r in case.loose:
        if r.kind in ('float', 'entry'):
            err = span_errors if r.kind == 'float' else entry_errors
            out.append((r.name, r.buf, r.idx, hi[r.buf].reshape(-1)[r.idx], err(lo[r.buf].reshape(-1)[r.idx], hi[r.buf].reshape(-1)[r.idx]), err))
    for name, buf, idx, ref in case.also_float:
        out.append((name, buf, idx, ref(np.float64), span_errors(ref(np.float32), ref(np.float64)), span_errors))
    return out


def measure(case, got_bufs, report=print):
    """every float check of the case on `got_bufs`: prints MEASURED lines, returns [(name, worst ratio, its floor, its bound, ok)]"""
    res = []
    for name, buf, idx, ref, floor, err in float_checks(case):
        e = err(typed(case, got_bufs, buf)[idx], ref)
        bd = bounds_of(floor)
        k = int(np.argmax(e / bd))
        report('MEASURED %s %s %s ratio %.3e floor %.3e bound %.3e' % (case.family, case.name, name, e[k], floor[k], bd[k]))
        res.append((name, float(e[k]), float(floor[k]), float(bd[k]), bool((e <= bd).all())))
    return res


def mismatches(case, got_bufs, ref_bufs=None):
    """[(buffer, number of differing bytes, first element)] outside the loose regions, against the image (or `ref_bufs`) -- and
    the 'nan' regions that hold something else"""
    img = ref_bufs if ref_bufs is not None else case.image()
    bad = []
    for k, b in enumerate(case.bufs):
        keep = strict_mask(case, k)
        g, r = typed(case, got_bufs, k), typed(case, img, k)
        ub = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[b.dtype.itemsize]
        d = np.nonzero((g.view(ub) != r.view(ub)) & keep)[0]
        if d.size:
            bad.append((k, int(d.size), int(d[0]), g[d[0]], r[d[0]]))
    for r in case.loose:
        if r.kind == 'nan':
            g = typed(case, got_bufs, r.buf)[r.idx]
            if g.dtype == np.uint16:
                isn = ((g & 0x7f80) == 0x7f80) & ((g & 0x7f) != 0)
                sign = (g >> 15).astype(bool)
            else:
                isn, sign = np.isnan(g), np.signbit(g)
            ok = isn if getattr(r, 'sign', None) is None else isn & (sign == np.asarray(r.sign, bool))
            if not ok.all():
                bad.append((r.buf, int((~ok).sum()), int(r.idx[np.nonzero(~ok)[0][0]]), 'not the NaN', r.name))
    return bad


# ---- number formats -------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> bf16 codes, round to nearest even (finite and infinite values; a NaN needs the caller's care)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    up, low = u >> 16, u & 0xffff
    return (up + ((low > 0x8000) | ((low == 0x8000) & ((up & 1) == 1)))).astype(np.uint16)


def f16_sat(x):
    """float32 -> f16 codes, nearest even, saturating at +-65504 (the operand copies never gain an infinity)"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(np.abs(x) > f32(65504.0), np.copysign(f32(65504.0), x), x).astype(np.float16).view(np.uint16)


def widen(h):
    return (np.ascontiguousarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)


def unf16(h):
    return np.ascontiguousarray(h, np.uint16).view(np.float16).astype(np.float32)


# ---- AdamW: the rule of the header -----------------------------------------------------------------------------------------------
CFG = {
    'step1-clip': dict(step=1, lr=1e-3, wd=1e-2, ss=4.0, f0=1.0, f1=0.0),                 # coefficient 1 / (2 + 1e-6)
    'step1e4-nor4': dict(step=10000, lr=1e-3, wd=0.0, ss=None, f0=1.0, f1=0.0),
    'lr0-f0neg': dict(step=1, lr=0.0, wd=1e-2, ss=4.0, f0=-1.0, f1=0.0),
    'noclip': dict(step=7, lr=3e-4, wd=1e-2, ss=0.25, f0=1.0, f1=0.0),                    # norm 0.5 below max_norm 1
    'ss0': dict(step=1, lr=1e-3, wd=0.0, ss=0.0, f0=1.0, f1=0.0),
    'scale1024': dict(step=10000, lr=1e-3, wd=1e-2, ss=4.0 * 1024 ** 2, f0=1.0, f1=1.0 / 1024, gscale=1024.0),
    'tiny-norm': dict(step=3, lr=1e-3, wd=1e-2, ss=1e-4, f0=5e-3, f1=0.0),                # 1e-6 is 1e-4 of the norm
    'inf': dict(step=1, lr=1e-3, wd=1e-2, ss=float('inf'), f0=1.0, f1=0.0),
    'nan': dict(step=1, lr=1e-3, wd=1e-2, ss=float('nan'), f0=0.0, f1=0.0),
}


def hyper(cfg):
    s = cfg['step']
    return (cfg['lr'], BETAS[0], BETAS[1], EPS, cfg['wd'], 1.0 - BETAS[0] ** s, 1.0 - BETAS[1] ** s)


def clip_of(cfg, dt):
    """the factor on the gradient: 1 / loss scale times clip_grad_norm_'s coefficient; None: the NaN guard skips the update"""
    ss, f0, f1 = cfg['ss'], cfg['f0'], cfg['f1']
    if ss is not None and not np.isfinite(f32(ss)):
        return None
    inv = dt(f32(f1)) if f1 > 0 else dt(1)
    clip = inv
    if ss is not None and f0 > 0:
        norm = dt(np.sqrt(dt(f32(ss))) * inv)
        clip = dt(inv * min(dt(1), dt(dt(f32(f0)) / dt(norm + dt(f32(1e-6))))))
    return clip


def adamw_eval(p, g, m, v, cfg, dt):
    """torch.optim.AdamW with the gradient scaled by clip_of, in `dt`, results rounded to float32"""
    clip = clip_of(cfg, dt)
    if clip is None:
        return p.copy(), m.copy(), v.copy()
    lr, b1, b2, eps, wd, bc1, bc2 = (dt(f32(x)) for x in hyper(cfg))
    gi = g.astype(dt) * clip
    m2 = b1 * m.astype(dt) + (dt(1) - b1) * gi
    v2 = b2 * v.astype(dt) + (dt(1) - b2) * gi * gi
    den = np.sqrt(v2) / np.sqrt(bc2) + eps
    p2 = p.astype(dt) * (dt(1) - lr * wd) - (lr / bc1) * m2 / den
    return p2.astype(np.float32), m2.astype(np.float32), v2.astype(np.float32)


def _fma32(a, x, y):
    """float32(a * x + y) with ONE rounding: the product of two floats is exact in float64; the float64 sum is made
    round-to-odd (TwoSum), which the final rounding to float32 cannot tell from the exact sum"""
    prod = np.float64(a) * x.astype(np.float64)
    y = y.astype(np.float64)
    s = prod + y
    bb = s - prod
    err = (prod - (s - bb)) + (y - bb)
    bits = s.view(np.int64).copy()
    inexact = (err != 0) & np.isfinite(s)
    away = inexact & ((err > 0) == (s > 0))               # the exact sum lies beyond s: truncation gives s itself
    toward = inexact & ~away                               # ... inside: the neighbour towards zero
    bits = np.where(toward, bits - 1, bits)
    bits = np.where(inexact, bits | 1, bits)
    return bits.view(np.float64).astype(np.float32)


def mix32(x):
    x = np.asarray(x, np.uint64) & 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def s16_bits(seed, step, flat_idx):
    key = mix32(np.asarray([(int(seed) * 0x9e3779b9 + int(step)) & 0xffffffff]))[0]
    return mix32((np.asarray(flat_idx, np.int64).astype(np.uint64) & 0xffffffff) ^ key)


def s16_eval(p, g, mb, vb, cfg, seed, flat_idx):
    """one bf16-state update of the elements with flat indices `flat_idx` -> (p, exp_avg codes, exp_avg_sq codes), exact"""
    clip = clip_of(cfg, np.float32)
    if clip is None:
        return p.copy(), mb.copy(), vb.copy()
    lr, b1, b2, eps, wd, bc1, bc2 = (f32(x) for x in hyper(cfg))
    stepsz, decay, bc2s = f32(lr / bc1), f32(f32(1) - f32(lr * wd)), np.sqrt(bc2)
    mf, vf = widen(mb), widen(vb)
    with np.errstate(under='ignore'):
        gi = g * clip
        mi = _fma32(b1, mf, (f32(1) - b1) * gi)
        vi = _fma32(b2, vf, ((f32(1) - b2) * gi) * gi)
        den = np.sqrt(vi) / bc2s + eps
        pn = p * decay - (stepsz * mi) / den
    h = s16_bits(seed, cfg['step'], flat_idx)
    st = lambda x, r: (((x.view(np.uint32).astype(np.uint64) + r) & 0xffffffff) >> 16).astype(np.uint16)
    return pn.astype(np.float32), st(mi, h & 0xffff), st(vi, h >> 16)


# ---- AdamW inputs: not i.i.d. ----------------------------------------------------------------------------------------------------
GMAG = (1e-12, 1e-3, 1.0, 1e3, 0.0, 1e-6, 1e-9, 30.0)       # gradient magnitude per 1024-element span
VMAG = (0.0, 1e-8, 1.0, 1e4, 1e-4)
PMAG = (1e-3, 1.0, 1e3)
MSIGN = (1, -1, -1, 1, 1, -1, 1)                             # exp_avg against the gradient on some spans


def adamw_data(n, key, phase=0, gscale=1.0):
    """p, g, m, v for n elements; span s = phase + i / 1024 picks the magnitudes.  A span with GMAG 0 has g = 0 and v = 0:
    m = 0 as well where (s / 8) is even (the all-zero span), m ~ 1e-3 where it is odd (eps alone in the denominator)"""
    rs = np.random.RandomState(_seed(('adamw-data',) + tuple(key)))
    s = phase + np.arange(n) // SPAN
    u = lambda: rs.uniform(0.5, 2.0, n)
    sg = np.where(rs.random_sample(n) < 0.5, -1.0, 1.0)
    gm = np.asarray(GMAG)[s % 8]
    g = sg * gm * u() * gscale
    m = np.asarray(MSIGN)[s % 7] * sg * gm * u() * 3.0
    v = np.asarray(VMAG)[s % 5] * u()
    zero = gm == 0.0
    v[zero] = 0.0
    m[zero] = np.where((s[zero] // 8) % 2 == 1, 1e-3 * u()[zero] * sg[zero], 0.0)
    p = np.where(rs.random_sample(n) < 0.5, -1.0, 1.0) * np.asarray(PMAG)[s % 3] * u()
    return p.astype(np.float32), g.astype(np.float32), m.astype(np.float32), v.astype(np.float32)


def _framed(x, front, fill=KEEP):
    return np.concatenate([np.full(front, fill, x.dtype), x, np.full(SLACK, fill, x.dtype)])


def _adamw_op(C, kind, refs, n_field, cfg, seed=None):
    f = [cfg['f0'], cfg['f1']] + ([float(cfg['step']), float(seed)] if seed is not None else [])
    C.op(kind, refs, [n_field] + [dbits(h) for h in hyper(cfg)], f)


def adamw_case(name, n, cfgname, phase=0, off=0, mis=None, regimes=(), data=None):
    """GHN3_OP_ADAMW on n elements that start `off` floats into their buffers; mis: the one buffer (0 p 1 g 2 m 3 v) that
    starts one float later -- 4 bytes off 16 while the others are aligned"""
    cfg = CFG[cfgname] if isinstance(cfgname, str) else cfgname
    C = Case('adamw', name, set(regimes) | ({'adamw:' + cfgname} if isinstance(cfgname, str) else set()))
    arrs = data if data is not None else adamw_data(n, (n, cfgname, phase), phase, cfg.get('gscale', 1.0))
    starts = [off + (1 if mis == k else 0) for k in range(4)]
    for k in range(4):
        C.add(_framed(arrs[k], starts[k]))
    ss = cfg['ss']
    b_ss = C.add(np.asarray([ss if ss is not None else 0.0, 7, 7, 7], np.float32))
    _adamw_op(C, L.OP_ADAMW, [(k, 4 * starts[k]) for k in range(4)] + [b_ss if ss is not None else None], n, cfg)

    def write(img, dt):
        p2, m2, v2 = adamw_eval(*arrs, cfg, dt)
        for k, a in ((0, p2), (2, m2), (3, v2)):
            img[k][starts[k]:starts[k] + n] = a
    C.writer(write)
    if clip_of(cfg, np.float64) is not None:
        for k, nm in ((0, 'p'), (2, 'm'), (3, 'v')):
            C.region('float', nm, k, starts[k] + np.arange(n))
    C.meta = SimpleNamespace(n=n, cfg=cfg, starts=starts, arrs=arrs, datakey=(n, cfgname, phase))
    return C


def _adamw_cases():
    out = []
    rot = ['step1-clip', 'step1e4-nor4', 'lr0-f0neg', 'noclip', 'ss0', 'scale1024', 'tiny-norm']
    for k, n in enumerate((1, 3, 4, 1023, 1024, 1025, 5156)):
        out.append(adamw_case('adamw-n%d-%s' % (n, rot[k]), n, rot[k], phase=(0, 4, 12, 1, 2, 3, 0)[k]))
    # every configuration once more where every span kind occurs (14 spans from phase 0: the all-zero span 4, the eps span 12)
    for cn in rot:
        out.append(adamw_case('adamw-n14000-%s' % cn, 14000, cn))
    out.append(adamw_case('adamw-range-off1001', 5156, 'step1-clip', off=1001, regimes={'adamw:all-misaligned'}))
    out.append(adamw_case('adamw-m-off4', 5156, 'step1-clip', mis=2, regimes={'adamw:m-misaligned'}))
    out.append(adamw_case('adamw-g-off4', 5156, 'step1-clip', mis=1, regimes={'adamw:g-misaligned'}))
    out.append(adamw_case('adamw-aligned', 5156, 'step1-clip', regimes={'adamw:aligned-twin'}))
    out.append(adamw_case('adamw-sumsq-inf', 5156, 'inf'))
    out.append(adamw_case('adamw-sumsq-nan', 1025, 'nan', mis=3))
    return out


SAME_DATA = ('adamw-aligned', 'adamw-range-off1001', 'adamw-m-off4', 'adamw-g-off4')     # one data set, four routes


# ---- bf16 state, flat ---------------------------------------------------------------------------------------------------------------
def s16_state(arrs):
    """the fp32 moments of adamw_data as bf16 codes (truncated: any representable state will do)"""
    return (arrs[2].view(np.uint32) >> 16).astype(np.uint16), (arrs[3].view(np.uint32) >> 16).astype(np.uint16)


def s16_case(name, n, cfgname, seed=5, lo=0, parts=None, m_shift=0, regimes=(), phase=0, datakey=None, step=None):
    """GHN3_OP_ADAMW_S16 on the elements [lo, lo + n) of flat buffers (r0 / r1 4 * lo bytes in, r2 / r3 2 * lo); parts: the
    split points of several ops over the same range; m_shift = 1: exp_avg reaches the op 2 bytes off its 16-byte boundary"""
    cfg = dict(CFG[cfgname])
    if step is not None:
        cfg['step'] = step
    C = Case('s16', name, set(regimes) | {'s16:' + cfgname})
    arrs = adamw_data(n, datakey or (n, cfgname, phase), phase, cfg.get('gscale', 1.0))
    mb, vb = s16_state(arrs)
    bp, bg = C.add(_framed(arrs[0], lo)), C.add(_framed(arrs[1], lo))
    bm = C.add(_framed(mb, lo + m_shift, np.uint16(0x40e0)), shift=2 * m_shift)
    bv = C.add(_framed(vb, lo, np.uint16(0x40e0)))
    ss = cfg['ss']
    b_ss = C.add(np.asarray([ss if ss is not None else 0.0, 7, 7, 7], np.float32))
    cuts = [0] + list(parts or []) + [n]
    for a, b in zip(cuts, cuts[1:]):
        _adamw_op(C, L.OP_ADAMW_S16, [(bp, 4 * (lo + a)), (bg, 4 * (lo + a)), (bm, 2 * (lo + a)), (bv, 2 * (lo + a)),
                                      b_ss if ss is not None else None], b - a, cfg, seed)

    def write(img, dt):
        p2, m2, v2 = s16_eval(arrs[0], arrs[1], mb, vb, cfg, seed, lo + np.arange(n))
        img[bp][lo:lo + n], img[bm][lo + m_shift:lo + m_shift + n], img[bv][lo:lo + n] = p2, m2, v2
    C.writer(write)
    C.meta = SimpleNamespace(n=n, cfg=cfg, lo=lo, arrs=arrs, mb=mb, vb=vb, seed=seed, m_shift=m_shift, bufs=(bp, bg, bm, bv, b_ss))
    return C


def _s16_cases():
    out = []
    rot = ['step1-clip', 'step1e4-nor4', 'lr0-f0neg', 'noclip', 'scale1024', 'tiny-norm']
    for k, n in enumerate((1, 3, 4, 1023, 1025, 5156)):
        out.append(s16_case('s16-n%d-%s' % (n, rot[k]), n, rot[k], phase=(0, 4, 12, 1, 2, 0)[k], lo=(0, 4, 0, 8, 1001, 0)[k]))
    key = (14000, 's16-shared')
    out.append(s16_case('s16-one', 14000, 'step1-clip', datakey=key, regimes={'s16:negative-m', 's16:one-launch'}))
    out.append(s16_case('s16-three-parts', 14000, 'step1-clip', datakey=key, parts=(1001, 9000), regimes={'s16:partition'}))
    out.append(s16_case('s16-three-parts-b', 14000, 'step1-clip', datakey=key, parts=(4, 4100), regimes={'s16:partition'}))
    out.append(s16_case('s16-m-off2', 14000, 'step1-clip', datakey=key, m_shift=1, regimes={'s16:m-misaligned'}))
    out.append(s16_case('s16-seed6', 14000, 'step1-clip', datakey=key, seed=6, regimes={'s16:other-seed'}))
    out.append(s16_case('s16-step5-seed1', 14000, 'noclip', datakey=key, seed=1, step=5, regimes={'s16:swap'}))
    out.append(s16_case('s16-step1-seed5', 14000, 'noclip', datakey=key, seed=5, step=1, regimes={'s16:swap'}))
    out.append(s16_case('s16-sumsq-nan', 1025, 'nan', lo=4))
    return out


S16_SAME = ('s16-one', 's16-three-parts', 's16-three-parts-b', 's16-m-off2')


# ---- AdamW over a cast-descriptor table -----------------------------------------------------------------------------------------------
# 65504 / 65520 / 1e5 saturate in f16; 1.00390625, 1.01171875 and their negatives are bf16 ties (down / up to even)
SPECIAL_P = np.asarray([65504.0, -65504.0, 65520.0, -65520.0, 65505.0, 1e5, -1e5, 7e4, 1.00390625, 1.01171875, -1.00390625,
                        -1.01171875, -0.0, 0.0, 3.0e38, 6e-8], np.float32)


def frag_index(n, k, K):
    return ((n // 16) * (K // 32) + k // 32) * 512 + ((k % 32) // 8 * 16 + n % 16) * 8 + k % 8


def cast_case(name, specs, cfgname, bf, s16=False, lo0=0, regimes=(), special=False, seed=9):
    """GHN3_OP_ADAMW_CAST16 / _S16_CAST16 over `specs` (dicts: rows, cols, ld, st, tr, tight, split, f16s, frag, tr_bf) whose
    sources lie behind one another with gaps of 8 floats in flat buffers that the op sees from element lo0 on, followed by a
    GHN3_OP_CAST16 with the same table into a second destination"""
    cfg = CFG[cfgname]
    C = Case('cast-s16' if s16 else 'cast', name, set(regimes) | {'cast:' + cfgname})
    descs = np.zeros(len(specs), dtype=L.CAST_DT)
    cur, at16, blocks, plan = 4, 64, 0, []
    for D, s_ in zip(descs, specs):
        rows, cols, ld = s_['rows'], s_['cols'], s_.get('ld', s_['cols'])
        assert cols % 4 == 0 and ld % 4 == 0 and cur % 4 == 0 and ld >= cols
        D['src_off'], D['rows'], D['cols'], D['ld_src'] = cur, rows, cols, ld
        split, frag = bool(s_.get('split')), bool(s_.get('frag'))
        fl = (L.CAST_SPLIT if split else 0) | (L.CAST_FRAG if frag else 0) | (L.CAST_SPLIT_F16 if s_.get('f16s') else 0)
        pl = dict(src=cur, rows=rows, cols=cols, ld=ld, split=split, frag=frag, f16s=bool(s_.get('f16s')))
        if s_.get('st'):
            fl |= L.CAST_STRAIGHT | (L.CAST_STRAIGHT_BF16 if bf else 0)
            ldd = r64(cols) + 8
            size = rows * ldd
            D['dst_off'], D['ld_dst'] = at16, ldd
            pl['st'], pl['st_bf'] = (at16, ldd), (bf or split) and not s_.get('f16s')
            if split:
                D['lo_off'] = r64(size) + 64
            at16 = r64(at16 + (2 * (r64(size) + 64) if split else size) + 8) + 64
        if s_.get('tr'):
            tbf = s_.get('tr_bf', bf)
            fl |= L.CAST_TRANSPOSED | (L.CAST_TRANSPOSED_BF16 if tbf else 0) | (L.CAST_TIGHT if s_.get('tight') else 0)
            ldd = r64(rows) + 8
            size = cols * ldd
            if split and not s_.get('st'):
                D['lo_off'] = r64(size) + 64
            lo_off = int(D['lo_off'])
            assert not split or lo_off >= size
            D['dstT_off'], D['ld_dstT'] = at16, ldd
            pl['tr'], pl['tr_bf'], pl['tight'] = (at16, ldd), tbf or split, bool(s_.get('tight'))
            at16 = r64(at16 + (lo_off + size if split else size) + 8) + 64
        pl['lo_off'] = int(D['lo_off'])
        D['flags'], D['block_start'] = fl, blocks
        blocks += ((rows + 63) // 64) * ((cols + 63) // 64)
        cur += rows * ld + 8
        plan.append(pl)
    total = cur
    arrs = list(adamw_data(total, (name,), 0, cfg.get('gscale', 1.0)))
    if special:
        arrs[0] = np.resize(SPECIAL_P, total).astype(np.float32) * np.where(np.arange(total) % 34 < 17, f32(1), f32(0.5))
    el = np.concatenate([e.reshape(-1) for e in [pl['src'] + np.arange(pl['rows'])[:, None] * pl['ld'] + np.arange(pl['cols'])[None, :]
                                                  for pl in plan]])
    assert len(np.unique(el)) == len(el)
    if s16:
        mb, vb = s16_state(arrs)
        state = [_framed(mb, lo0, np.uint16(0x40e0)), _framed(vb, lo0, np.uint16(0x40e0))]
    else:
        mb = vb = None
        state = [_framed(arrs[2], lo0), _framed(arrs[3], lo0)]
    bp, bg = C.add(_framed(arrs[0], lo0)), C.add(_framed(arrs[1], lo0))
    bm, bv = C.add(state[0]), C.add(state[1])
    ss = cfg['ss']
    b_ss = C.add(np.asarray([ss if ss is not None else 0.0, 7, 7, 7], np.float32))
    b_dst, b_dst2 = C.add(np.full(at16 + 64, SENT16, np.uint16)), C.add(np.full(at16 + 64, SENT16, np.uint16))
    b_desc = C.add(descs.view(np.uint8).reshape(-1).copy())
    it = 2 if s16 else 4
    refs = [(bp, 4 * lo0), (bg, 4 * lo0), (bm, it * lo0), (bv, it * lo0), b_ss if ss is not None else None, b_dst, b_desc]
    _adamw_op(C, L.OP_ADAMW_S16_CAST16 if s16 else L.OP_ADAMW_CAST16, refs, len(specs) + (blocks << 32), cfg, seed if s16 else None)
    skipped = clip_of(cfg, np.float64) is None
    if not skipped:
        C.op(L.OP_CAST16, [(bp, 4 * lo0), b_dst2, b_desc], (len(specs), blocks, 0))

    def write(img, dt):
        if s16:
            p2, m2, v2 = s16_eval(arrs[0][el], arrs[1][el], mb[el], vb[el], cfg, seed, lo0 + el)
        else:
            p2, m2, v2 = adamw_eval(arrs[0][el], arrs[1][el], arrs[2][el], arrs[3][el], cfg, dt)
        img[bp][lo0 + el], img[bm][lo0 + el], img[bv][lo0 + el] = p2, m2, v2
    C.writer(write)
    if not skipped:
        if not s16:
            for k, nm in ((bp, 'p'), (bm, 'm'), (bv, 'v')):
                C.region('float', nm, k, lo0 + el)
        C.region('free', 'copies', b_dst, np.arange(at16 + 64))
        C.region('free', 'copies2', b_dst2, np.arange(at16 + 64))
    C.meta = SimpleNamespace(cfg=cfg, lo0=lo0, total=total, el=el, plan=plan, descs=descs, blocks=blocks, bf=bf, s16=s16, arrs=arrs,
                             seed=seed, bufs=(bp, bg, bm, bv, b_ss, b_dst, b_dst2, b_desc), skipped=skipped, size16=at16 + 64)
    return C


def copy_image(case, p_now):
    """the destination buffer a cast of the parameters `p_now` (the typed parameter buffer of a run) by the case's table must
    give: copies, zero padding, sentinel everywhere else"""
    m = case.meta
    out = np.full(m.size16, SENT16, np.uint16)
    cv = lambda x, bf_: bf16_rne(x) if bf_ else f16_sat(x)
    for pl in m.plan:
        rows, cols = pl['rows'], pl['cols']
        X = np.ascontiguousarray(p_now[m.lo0 + pl['src'] + np.arange(rows)[:, None] * pl['ld'] + np.arange(cols)[None, :]], np.float32)
        with np.errstate(over='ignore', invalid='ignore'):
            hi_b = bf16_rne(X)
            lo_b = bf16_rne(X - widen(hi_b))
            Xs = X * f32(2.0 ** L.X3F16_WSHIFT)
            hi_h = f16_sat(Xs)
            lo_h = f16_sat(Xs - unf16(hi_h))
        if 'st' in pl:
            at, ldd = pl['st']
            H, Lo = (hi_h, lo_h) if pl['f16s'] else (hi_b, lo_b) if pl['split'] else (cv(X, pl['st_bf']), None)
            if pl['frag']:
                ii = at + frag_index(np.arange(rows)[:, None], np.arange(cols)[None, :], cols)
                out[ii], out[ii + pl['lo_off']] = H, Lo
            else:
                Z = np.zeros((rows, r64(cols)), np.uint16)
                ii = at + np.arange(rows)[:, None] * ldd + np.arange(r64(cols))[None, :]
                Z[:, :cols] = H
                out[ii] = Z
                if pl['split']:
                    Z[:, :cols] = Lo
                    out[ii + pl['lo_off']] = Z
        if 'tr' in pl:
            at, ldd = pl['tr']
            H, Lo = (hi_b, lo_b) if pl['split'] else (cv(X, pl['tr_bf']), None)
            if pl['frag']:
                ii = at + frag_index(np.arange(cols)[:, None], np.arange(rows)[None, :], rows)
                out[ii], out[ii + pl['lo_off']] = H.T, Lo.T
            else:
                rw = r8(rows) if pl['tight'] else r64(rows)
                Z = np.zeros((cols, rw), np.uint16)
                ii = at + np.arange(cols)[:, None] * ldd + np.arange(rw)[None, :]
                Z[:, :rows] = H.T
                out[ii] = Z
                if pl['split']:
                    Z[:, :rows] = Lo.T
                    out[ii + pl['lo_off']] = Z
    return out


def flat_twin(case):
    """the flat op (GHN3_OP_ADAMW / _S16) over the whole source range of a cast case, on the same buffers: the descriptors'
    elements must come out of both with the same bits"""
    o = case.ops[:1].copy()
    o['kind'] = L.OP_ADAMW_S16 if case.meta.s16 else L.OP_ADAMW
    o['i'][0][0] = case.meta.total
    o['r']['buf'][0][5:7] = -1
    return o


def _cast_specs():
    return [
        ('c64', [dict(rows=64, cols=64, st=True, tr=True)], 'step1-clip', False, {}),
        ('ragged-ld136', [dict(rows=70, cols=132, ld=136, st=True, tr=True)], 'step1e4-nor4', True, {}),
        ('r1c4', [dict(rows=1, cols=4, st=True, tr=True)], 'noclip', False, {}),
        ('tight-130x64', [dict(rows=130, cols=64, tr=True, tight=True)], 'tiny-norm', True, {}),
        ('desc2-st', [dict(rows=70, cols=68, ld=72, st=True), dict(rows=5, cols=200, st=True)], 'scale1024', False, dict(lo0=1000)),
        ('desc3-tr', [dict(rows=70, cols=68, tr=True), dict(rows=64, cols=64, tr=True, tight=True), dict(rows=3, cols=8, ld=12, tr=True)],
         'step1-clip', True, dict(lo0=8)),
        ('desc5-mixed', [dict(rows=130, cols=72, ld=76, st=True), dict(rows=5, cols=200, tr=True), dict(rows=64, cols=64, st=True, tr=True),
                         dict(rows=1, cols=4, st=True), dict(rows=70, cols=8, tr=True, tight=True)], 'noclip', False, dict(lo0=2048)),
        ('w2-f16-bf16T', [dict(rows=130, cols=64, st=True, tr=True, tr_bf=True)], 'step1-clip', False, {}),      # production: types per copy
        ('split', [dict(rows=70, cols=68, st=True, tr=True, split=True)], 'step1e4-nor4', True, {}),
        ('split-f16', [dict(rows=70, cols=68, st=True, tr=True, split=True, f16s=True)], 'noclip', True, {}),
        ('frag', [dict(rows=64, cols=96, st=True, tr=True, split=True, frag=True)], 'step1-clip', True, {}),
        ('special-f16', [dict(rows=70, cols=68, ld=72, st=True, tr=True)], 'lr0-f0neg', False, dict(special=True)),
        ('special-bf16', [dict(rows=70, cols=68, ld=72, st=True, tr=True)], 'lr0-f0neg', True, dict(special=True)),
        ('sumsq-inf', [dict(rows=70, cols=68, st=True, tr=True)], 'inf', False, {}),
        ('sumsq-nan', [dict(rows=70, cols=68, st=True, tr=True)], 'nan', True, dict(lo0=8)),
    ]


def _cast_cases(s16):
    return [cast_case(('cs16-' if s16 else 'cast-') + nm, specs, cn, bf, s16=s16, **kw) for nm, specs, cn, bf, kw in _cast_specs()]


# ---- GHN3_OP_SUMSQ ---------------------------------------------------------------------------------------------------------------------
def sumsq_case(name, x, skip=None, extra=None, scratch=True, regimes=()):
    """r0[0] += sum x^2, without the floats [skip) and with the `extra` partial sums added"""
    C = Case('sumsq', name, regimes)
    n = x.size
    b_out = C.add(np.asarray([SENT, 7, 7, 7], np.float32))
    b_x = C.add(np.concatenate([x, nan_f32(SLACK)]))
    scr = 8192 if (skip or extra is not None) else 4096
    b_scr = C.add(nan_f32(scr + SLACK)) if scratch else None
    b_ex = C.add(np.concatenate([extra, nan_f32(SLACK)])) if extra is not None else None
    lo, hi = skip or (0, 0)
    C.op(L.OP_SUMSQ, [b_out, b_x, b_scr, b_ex], (n, lo, hi, extra.size if extra is not None else 0))

    def write(img, dt):
        keep = np.concatenate([x[:lo], x[hi:]]).astype(dt)
        tot = dt(SENT) + (keep * keep).sum(dtype=dt)
        if extra is not None:
            tot = tot + extra.astype(dt).sum(dtype=dt)
        img[b_out][0] = f32(tot)
    C.writer(write)
    C.region('entry', 'sumsq', b_out, [0])
    if scratch:
        C.region('free', 'scratch', b_scr, np.arange(scr))
    C.rerun = scratch
    C.meta = SimpleNamespace(n=n, skip=skip)
    return C


def sum_pattern(n, key, tail=50.0):
    """values whose sum of squares notices a skipped, repeated or misplaced stretch: a short pattern tiled, scaled by the
    position (2^(i / 2^18 mod 4) / 2 and a slow ramp), and `tail` in the last n % 4 elements"""
    rs = np.random.RandomState(_seed(('sum',) + tuple(key)))
    base = rs.standard_normal(4099).astype(np.float32)
    i = np.arange(n)
    x = np.resize(base, n) * (2.0 ** ((i >> 18) % 4 - 1)).astype(np.float32) * (f32(1) + (i % 8191).astype(np.float32) / f32(8191))
    if n % 4:
        x[-(n % 4):] = tail
    return x.astype(np.float32)


def _sumsq_cases():
    rs = np.random.RandomState(3)
    ex = lambda k: (rs.standard_normal(k) ** 2).astype(np.float32)
    return [
        sumsq_case('sumsq-skip-from0-e1', sum_pattern(3001, 'a'), skip=(0, 1024), extra=ex(1), regimes={'sumsq:skip-at-0', 'sumsq:extra1'}),
        sumsq_case('sumsq-skip-to-n-e3', sum_pattern(3000, 'b'), skip=(1000, 3000), extra=ex(3), regimes={'sumsq:skip-to-n', 'sumsq:extra3'}),
        sumsq_case('sumsq-skip-mid-e4', sum_pattern(5003, 'c'), skip=(1000, 3048), extra=ex(4), regimes={'sumsq:extra4'}),
        sumsq_case('sumsq-noskip-e261', sum_pattern(1027, 'd'), extra=ex(261), regimes={'sumsq:extra261', 'sumsq:extra-alone'}),
    ]


def big_sumsq_plain():
    return sumsq_case('sumsq-loop-plain', sum_pattern(4096 * 1024 + 1029, 'big'), regimes={'sumsq:loop'})


def big_sumsq_skip():
    lo, gap = 1028, 2048
    n = lo + gap + 4032 * 1024 + 1029
    x = sum_pattern(n, 'bigskip')
    x[lo:lo + gap] = f32(1e30)                            # read, the sum would be infinite
    ex = (np.random.RandomState(4).standard_normal(261) ** 2).astype(np.float32)
    return sumsq_case('sumsq-loop-skip', x, skip=(lo, lo + gap), extra=ex, regimes={'sumsq:loop-above-gap'})


# ---- GHN3_OP_WIRE_PACK -------------------------------------------------------------------------------------------------------------------
# +-0, +-inf, the two ties (down to 0x3f80, up to 0x3f82), the largest float (-> inf), the largest that stays finite, the tie
# above it (-> inf), NaNs whose payload lies in the low half only (either sign), a quiet NaN, a negative tie, one bit above a tie
WIRE_SPECIAL = np.asarray([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x3f808000, 0x3f818000, 0x7f7fffff, 0x7f7f7fff,
                           0x7f7f8000, 0x7f800001, 0xff80ffff, 0x7fc00000, 0xbf808000, 0x3f808001, 0xff7f7fff, 0x00800000], np.uint32)
WIRE_WANT = {0x3f808000: 0x3f80, 0x3f818000: 0x3f82, 0x7f7fffff: 0x7f80, 0x7f7f7fff: 0x7f7f, 0x7f7f8000: 0x7f80, 0x80000000: 0x8000,
             0xbf808000: 0xbf80, 0x3f808001: 0x3f81, 0xff7f7fff: 0xff7f}


def wire_values(n, rot, key):
    rs = np.random.RandomState(_seed(('wire',) + tuple(key)))
    i = np.arange(n)
    x = (rs.standard_normal(n) * 2.0 ** ((i % 61) - 30)).astype(np.float32)
    k = np.arange(min(n, 2 * len(WIRE_SPECIAL)))
    x.view(np.uint32)[k] = WIRE_SPECIAL[(k + rot) % len(WIRE_SPECIAL)]
    return x


def _wire_forward(C, tag, x, n_pad, dmis, smis):
    n = x.size
    isn = np.isnan(x)
    b_src = C.add(np.concatenate([nan_f32(4 + smis), x, nan_f32(SLACK)]))
    b_dst = C.add(np.full(8 + dmis + n_pad + SLACK, SENT16, np.uint16))
    C.op(L.OP_WIRE_PACK, [(b_dst, 2 * (8 + dmis)), (b_src, 4 * (4 + smis))], (n, n_pad, 0))
    codes = bf16_rne(x)

    def write(img, dt):
        img[b_dst][8 + dmis:8 + dmis + n] = codes
        img[b_dst][8 + dmis + n:8 + dmis + n_pad] = 0
    C.writer(write)
    if isn.any():
        C.region('nan', tag, b_dst, 8 + dmis + np.nonzero(isn)[0], sign=np.signbit(x[isn]))
    return codes


def _wire_reverse(C, tag, codes, dmis, smis):
    n = codes.size
    b_src = C.add(np.concatenate([np.full(8 + smis, SENT16, np.uint16), codes, np.full(SLACK, SENT16, np.uint16)]))
    b_dst = C.add(nan_f32(4 + dmis + n + SLACK))
    C.op(L.OP_WIRE_PACK, [(b_dst, 4 * (4 + dmis)), (b_src, 2 * (8 + smis))], (n, n, 1))

    def write(img, dt):
        img[b_dst].view(np.uint32)[4 + dmis:4 + dmis + n] = codes.astype(np.uint32) << 16
    C.writer(write)


def wire_case(n):
    C = Case('wire', 'wire-n%d' % n, {'wire:n%d' % n})
    k = 0
    for n_pad in (n, n + 13):
        for dmis, smis in ((0, 0), (1, 0), (0, 1), (1, 1)):
            x = wire_values(n, 5 * k, (n, k))
            codes = _wire_forward(C, 'fw%d' % k, x, n_pad, dmis, smis)
            if n_pad == n:
                codes = np.where(np.isnan(x), np.where(np.signbit(x), 0xffc1, 0x7fc1), codes).astype(np.uint16)
                _wire_reverse(C, 'rv%d' % k, codes, smis, dmis)
            k += 1
    return C


def wire_refused():
    """n_pad < n: GHN3_E_ARG, nothing written"""
    C = Case('wire', 'wire-npad-below-n', {'wire:refused'})
    b_src, b_dst = C.add(wire_values(64, 0, ('ref',))), C.add(np.full(64 + SLACK, SENT16, np.uint16))
    C.op(L.OP_WIRE_PACK, [b_dst, b_src], (64, 63, 0))
    C.refused = True
    return C


def big_wire():
    n = 8192 * 2048 + 2051
    C = Case('wire', 'wire-loop', {'wire:loop'})
    x = np.resize(wire_values(4099, 3, ('big',)), n)
    with np.errstate(over='ignore', invalid='ignore'):       # (powers of two: the special values stay special)
        x = (x * (2.0 ** ((np.arange(n) >> 20) % 5)).astype(np.float32)).astype(np.float32)
    codes = _wire_forward(C, 'fw', x, n + 13, 0, 0)
    isn = np.isnan(x)
    codes = np.where(isn, np.where(np.signbit(x), 0xffc1, 0x7fc1), codes).astype(np.uint16)
    _wire_reverse(C, 'rv', codes, 0, 0)
    return C


# ---- GHN3_OP_RANK_REDUCE -------------------------------------------------------------------------------------------------------------------
ORDER = (2.0 ** 27, 1.0, -(2.0 ** 27), 1.0, 3.0, -(2.0 ** 27), 2.0 ** 27, 0.5)     # by rank: only the rank-order sum is right


def reduce_case(W, per, mis, big=False):
    """all four type combinations, f0 = 1 / W and 1: eight ops over their own buffers.  Column 0 holds ORDER by rank (exact in
    bf16; excluded from the float64 comparison: its float32 rank-order sum is by construction not the exact sum), column 2 a NaN
    in one rank"""
    C = Case('reduce', 'reduce-W%d-per%d%s' % (W, per, '-mis' if mis else ''), {'reduce:W%d' % W, 'reduce:per%d' % per})
    rs = np.random.RandomState(_seed(('reduce', W, per)))
    e = np.arange(per)
    for k, (in16, out16, scale) in enumerate([(a, b, s) for a in (0, 1) for b in (0, 1) for s in ((1.0 / W, 1.0) if not big else (1.0 / W,))]):
        if big and (in16, out16) not in ((1, 1), (0, 0)):
            continue
        base = rs.standard_normal((W, min(per, 4099))).astype(np.float32)
        X = np.stack([np.resize(base[w], per) for w in range(W)]) * (2.0 ** ((e % 37) - 18)).astype(np.float32)[None, :]
        X = X.astype(np.float32)
        X[:, 0] = np.asarray(ORDER[:W], np.float32)
        if per > 2:
            X[W // 2, 2] = np.float32('nan')
        if in16:
            X = widen((X.view(np.uint32) >> 16).astype(np.uint16))
        fi, fo = (8 if in16 else 4) + (mis if mis else 0), (8 if out16 else 4) + (mis if mis else 0)
        flat = X.reshape(-1)
        src = np.concatenate([np.full(fi, SENT16, np.uint16), (flat.view(np.uint32) >> 16).astype(np.uint16), np.full(SLACK, SENT16, np.uint16)]) \
            if in16 else np.concatenate([nan_f32(fi), flat, nan_f32(SLACK)])
        b_in = C.add(src)
        b_out = C.add(np.full(fo + per + SLACK, SENT16, np.uint16) if out16 else nan_f32(fo + per + SLACK))
        C.op(L.OP_RANK_REDUCE, [(b_out, (2 if out16 else 4) * fo), (b_in, (2 if in16 else 4) * fi)], (per, W, in16, out16), (scale,))
        with np.errstate(invalid='ignore', over='ignore'):
            acc = np.zeros(per, np.float32)
            for w in range(W):
                acc = acc + X[w]
            res = acc * f32(scale)
        isn = np.isnan(res)

        def write(img, dt, b_out=b_out, fo=fo, res=res, out16=out16):
            if out16:
                img[b_out][fo:fo + per] = bf16_rne(res)
            else:
                img[b_out][fo:fo + per] = res
        C.writer(write)
        if isn.any():
            C.region('nan', 'nan%d' % k, b_out, fo + np.nonzero(isn)[0])
        if not out16:
            ok = np.nonzero(~isn & (e != 0))[0]
            if ok.size:
                def ref(dt, X=X, ok=ok, scale=scale, res=res):
                    if dt == np.float32:
                        return res[ok]
                    return (X[:, ok].astype(np.float64).sum(0) * np.float64(f32(scale))).astype(np.float32)
                C.also_float.append(('out%d' % k, b_out, fo + ok, ref))
    return C


def _reduce_cases():
    out, k = [], 0
    for W in (1, 2, 5, 8):
        for per in (1, 3, 4, 5, 1003, 1024):
            out.append(reduce_case(W, per, k % 2))
            k += 1
    return out


def big_reduce():
    return reduce_case(2, 8192 * 1024 + 1003, 0, big=True)


# ---- GHN3_OP_TRANSPOSE32 --------------------------------------------------------------------------------------------------------------------
def _transpose_op(C, rows, cols, ld_s, ld_d, front, batch=1, sb=0, db=0, key=0):
    rs = np.random.RandomState(_seed(('tr', rows, cols, ld_s, ld_d, front, batch, key)))
    sb, db = sb or rows * ld_s, db or cols * ld_d
    n_s, n_d = (batch - 1) * sb + rows * ld_s, (batch - 1) * db + cols * ld_d
    src = rs.standard_normal(front + n_s + SLACK).astype(np.float32)
    b_src, b_dst = C.add(src), C.add(nan_f32(front + n_d + SLACK))
    C.op(L.OP_TRANSPOSE32, [(b_dst, 4 * front), (b_src, 4 * front)], (rows, cols, ld_s, ld_d, batch, sb, db))

    def write(img, dt):
        for b in range(batch):
            S = src[front + b * sb + np.arange(rows)[:, None] * ld_s + np.arange(cols)[None, :]]
            img[b_dst][front + b * db + np.arange(cols)[:, None] * ld_d + np.arange(rows)[None, :]] = S.T
    C.writer(write)


def transpose_case(rows, cols):
    C = Case('transpose', 'transpose-%dx%d' % (rows, cols), {'transpose:r%d' % rows, 'transpose:c%d' % cols})
    p4 = lambda v: (v + 3) // 4 * 4
    _transpose_op(C, rows, cols, p4(cols) + 4, p4(rows) + 4, 4)                # 16-byte route
    _transpose_op(C, rows, cols, p4(cols) + 3, p4(rows) + 5, 4)                # ld not a multiple of 4
    _transpose_op(C, rows, cols, p4(cols) + 4, p4(rows) + 4, 5)                # bases 4 bytes off
    _transpose_op(C, rows, cols, cols, rows, 4)                                # tight
    return C


def transpose_batched():
    C = Case('transpose', 'transpose-batch3', {'transpose:batch-both-routes'})
    # batch strides that are no multiples of 4: batch 0 takes the 16-byte route, batches 1 and 2 the scalar one
    _transpose_op(C, 65, 130, 132, 68, 4, batch=3, sb=65 * 132 + 1, db=130 * 68 + 3)
    _transpose_op(C, 130, 63, 64, 132, 4, batch=3, sb=130 * 64 + 2, db=63 * 132 + 4)
    return C


def _transpose_cases():
    return [transpose_case(r, c) for r in (1, 63, 64, 65, 130) for c in (1, 63, 64, 65, 130)] + [transpose_batched()]


# ---- GHN3_OP_GRAPH_PROLOGUE --------------------------------------------------------------------------------------------------------------------
MAX_DEGREE, MAX_INPUT_DIST = 100, 1000


def prologue_case(N, B, V=7):
    """A: asymmetric, shortest-path-like values in [0, V) with entries below 0, at and above V and far above the int32 range;
    a row and a column each with 99, 100, 101 and (N permitting) 300 ones; A[0, i] of 1000, 1001 and negative.  The image restates
    the reference model's graph code: degrees are the clipped row / column counts of A == 1, the input distance the clipped first
    row, the pair index the (forward, backward) entry clamped into the V x V table"""
    C = Case('prologue', 'prologue-N%d-B%d' % (N, B), {'prologue:N%d' % N})
    rs = np.random.RandomState(_seed(('prologue', N, B)))
    A = rs.randint(0, V, size=(B, N, N)).astype(np.int64)
    A[rs.random_sample(A.shape) < 0.6] = 0
    odd = rs.random_sample(A.shape)
    A[odd < 0.01] = -3
    A[(odd >= 0.01) & (odd < 0.02)] = V
    A[(odd >= 0.02) & (odd < 0.03)] = V + 5
    A[(odd >= 0.03) & (odd < 0.035)] = (1 << 40) + 1
    A[(odd >= 0.035) & (odd < 0.04)] = -(1 << 40)
    counts = [c for c in (99, 100, 101, 300) if c <= N]
    for b in range(B):
        for k, c in enumerate(counts):
            r = (3 + 5 * k + b) % N
            A[b, r, :] = np.where(A[b, r, :] == 1, 0, A[b, r, :])
            A[b, r, rs.permutation(N)[:c]] = 1
        for k, c in enumerate(counts):
            col = (N - 2 - 7 * k - b) % N
            keep = A[b, [(3 + 5 * j + b) % N for j in range(len(counts))], col].copy()
            A[b, :, col] = np.where(A[b, :, col] == 1, 0, A[b, :, col])
            rows = [r for r in rs.permutation(N) if r not in [(3 + 5 * j + b) % N for j in range(len(counts))]][:c - int((keep == 1).sum())]
            A[b, rows, col] = 1
            A[b, [(3 + 5 * j + b) % N for j in range(len(counts))], col] = keep
        for i, val in enumerate((1000, 1001, -7, (1 << 33) + 5, 999)):
            if 1 + i < N:
                A[b, 0, 1 + i] = val
    b_A = C.add(A.reshape(-1))
    outs = [C.add(np.full(B * N + SLACK, -77, np.int32)) for _ in range(3)] + [C.add(np.full(B * N * N + SLACK, -77, np.int32))]
    C.op(L.OP_GRAPH_PROLOGUE, [b_A] + outs, (B, N, V))

    def write(img, dt):
        one = (A == 1)
        img[outs[0]][:B * N] = np.clip(one.sum(1), 0, MAX_DEGREE).reshape(-1)          # in-degree: column sums
        img[outs[1]][:B * N] = np.clip(one.sum(2), 0, MAX_DEGREE).reshape(-1)
        img[outs[2]][:B * N] = np.clip(A[:, 0, :], 0, MAX_INPUT_DIST).reshape(-1)
        fw = np.clip(A, 0, V - 1)
        img[outs[3]][:B * N * N] = (fw * V + np.swapaxes(fw, 1, 2)).reshape(-1)
    C.writer(write)
    C.meta = SimpleNamespace(A=A, N=N, B=B, V=V)
    return C


def _prologue_cases():
    return [prologue_case(N, 1) for N in (1, 2, 255, 256, 257, 1024)] + [prologue_case(33, 3)]


# ---- GHN3_OP_MEMSET0 --------------------------------------------------------------------------------------------------------------------
def memset_case():
    C = Case('memset', 'memset0', {'memset:odd-bytes', 'memset:zero-count', 'memset:absent'})
    b = C.add(np.full(4096, 0xab, np.uint8))
    spans = [(16, 1), (35, 3), (64, 5), (101, 1026), (2000, 0), (3000, 7)]
    for off, cnt in spans:
        C.op(L.OP_MEMSET0, [(b, off)], (cnt,))
    C.op(L.OP_MEMSET0, [None], (8,))                       # an absent buffer: nothing happens

    def write(img, dt):
        for off, cnt in spans:
            img[b][off:off + cnt] = 0
    C.writer(write)
    return C


# ---- the table -----------------------------------------------------------------------------------------------------------------------------
_FAMILIES = {
    'adamw': _adamw_cases, 's16': _s16_cases, 'cast': lambda: _cast_cases(False), 'cast-s16': lambda: _cast_cases(True),
    'sumsq': _sumsq_cases, 'wire': lambda: [wire_case(n) for n in (1, 7, 8, 9, 2051)] + [wire_refused()],
    'reduce': _reduce_cases, 'transpose': _transpose_cases, 'prologue': _prologue_cases, 'memset': lambda: [memset_case()],
}


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(_FAMILIES[family]())


def all_cases():
    return [c for fam in _FAMILIES for c in cases(fam)]


def case_named(name):
    return next(c for c in all_cases() if c.name == name)


def big_adamw(s16=False):
    """n = 16384 * 1024 + 1027: the smallest size at which a lane of the 16384-workgroup grid takes a second trip and the
    scalar tail follows.  Eight spans of adamw_data tiled; p and g scaled by powers of two that change with the position."""
    n = 16384 * 1024 + 1027
    base = adamw_data(8 * SPAN, ('big', s16), 0)
    i = np.arange(n)
    sp = (2.0 ** ((i >> 21) % 3)).astype(np.float32)
    sg = (2.0 ** ((i >> 16) % 4 - 1)).astype(np.float32)
    arrs = (np.resize(base[0], n) * sp, np.resize(base[1], n) * sg, np.resize(base[2], n) * sg, np.resize(base[3], n))
    if not s16:
        C = adamw_case('adamw-loop', n, 'step1-clip', data=arrs, regimes={'adamw:loop'})
        return C
    C = Case('s16', 's16-loop', {'s16:loop'})
    cfg, seed = CFG['step1-clip'], 11
    mb, vb = s16_state(arrs)
    bufs = [C.add(_framed(a, 0, a.dtype.type(7) if a.dtype == np.float32 else np.uint16(0x40e0))) for a in (arrs[0], arrs[1], mb, vb)]
    b_ss = C.add(np.asarray([cfg['ss'], 7, 7, 7], np.float32))
    _adamw_op(C, L.OP_ADAMW_S16, bufs + [b_ss], n, cfg, seed)

    def write(img, dt):
        img[bufs[0]][:n], img[bufs[2]][:n], img[bufs[3]][:n] = s16_eval(arrs[0], arrs[1], mb, vb, cfg, seed, np.arange(n))
    C.writer(write)
    return C


BIG = {'adamw-loop': lambda: big_adamw(False), 's16-loop': lambda: big_adamw(True), 'sumsq-loop-plain': big_sumsq_plain,
       'sumsq-loop-skip': big_sumsq_skip, 'wire-loop': big_wire, 'reduce-loop': big_reduce}


def kinds_used():
    """every op kind that occurs in a case of this table"""
    return {int(k) for c in all_cases() for k in c.ops['kind']}


def refusals():
    """(name, case, ops, what the error names): arguments the host functions refuse with GHN3_E_ARG / GHN3_E_LIMIT before any
    launch (each refusal read in elementwise.hip: ghn3_adamw_cast16, ghn3_adamw_s16_cast16, adamw_rng_of, ghn3_sumsq,
    ghn3_wire_pack).  Nothing may be written.  The rules of the descriptor TABLE of the cast forms (src_off % 4, ld_src % 4,
    cols % 4) live in device memory, which a host function cannot read without a synchronisation: they are asserted where the
    table is built (Program.pack_cast_descs), and no case here breaks them."""
    out = []

    def variant(name, base, what, change):
        c = case_named(base)
        ops = c.ops[:1].copy()
        change(ops)
        out.append((name, c, ops, what))

    def shift_ref(k, by):
        def f(ops):
            ops['r']['off'][0][k] += by
        return f

    def set_f(k, v):
        def f(ops):
            ops['f'][0][k] = v
        return f

    def set_i(k, v):
        def f(ops):
            ops['i'][0][k] = v
        return f
    variant('cast-p-4-bytes-off', 'cast-c64', '16-byte aligned', shift_ref(0, 4))
    variant('cast-m-4-bytes-off', 'cast-c64', '16-byte aligned', shift_ref(2, 4))
    variant('cs16-g-4-bytes-off', 'cs16-c64', '16-byte', shift_ref(1, 4))
    variant('cs16-m-2-bytes-off', 'cs16-c64', '8-byte aligned', shift_ref(2, 2))
    variant('s16-step-2^24', 's16-one', 'not exact', set_f(2, float(1 << 24)))
    variant('s16-seed-2^24', 's16-one', 'not exact', set_f(3, float(1 << 24)))
    variant('s16-step-fraction', 's16-one', 'non-negative integers', set_f(2, 1.5))
    variant('s16-seed-negative', 'cs16-c64', 'non-negative integers', set_f(3, -1.0))
    variant('sumsq-x-4-bytes-off', 'sumsq-skip-mid-e4', '16-byte aligned', shift_ref(1, 4))
    variant('sumsq-skip-lo-not-x4', 'sumsq-skip-mid-e4', 'skipped range', set_i(1, 1002))
    variant('sumsq-skip-beyond-n', 'sumsq-skip-mid-e4', 'skipped range', set_i(2, 5004))
    variant('sumsq-slots-4-bytes-off', 'sumsq-skip-mid-e4', 'slot table', shift_ref(3, 4))
    return out
