"""
The target-network HIP ops (ghn3_amd/csrc/target_ops.hip: dense convolution with and without a norm, depthwise + pointwise +
norm, squeeze-and-excitation, pooling) at the edge shapes of tests/target_edge_cases.py -- half-vector channel tails, fewer
pixels than one tile or one reduction step, 1 x 1 images, stride with dilation, column counts just over a group boundary, the
widest channel counts, tied maxima -- against the stock torch layers in fp64, forward and every gradient.

The measure is tests/util_parity.slice_errors: per channel, per position and per sample for activations, per C_out, per C_in
and per tap for convolution weight gradients, per element for per-channel vectors, each divided by the reference's RMS slice
norm.  An error confined to one tail group, one border ring or one tap is not divided by the norm of everything else
(tests/test_target_edges_cpu.py shows the difference to the whole-tensor ratio).  The tolerances are the ones the project
states for these ops: 2e-4 outputs and statistics, 3e-4 gradients (split-bf16 products, ~1e-5 with two terms); 1e-5 / 2e-5
squeeze-and-excitation; 1e-6 / exact pooling.

Each row also runs with every buffer the op allocates pre-filled with NaN (a tail column, a partial tile or a partial-chunk row
the kernels leave unwritten would surface), twice for equal bits (forward and the gradients: fixed-order reductions), and after
asserting `applicable(...)`, so that no row tests the stock fallback.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import target_edge_cases as E
from util_gpu import _graph_nodes, buffers                  # noqa: F401 (buffers: a fixture, asked for by name)
from util_parity import slice_errors

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = 2e-4, 3e-4
SE_TOL, SE_PARAM_TOL = 1e-5, 2e-5
POOL_TOL = 1e-6


def _measure(label, name, got, ref, axes, tol, worst):
    assert got.shape == ref.shape, (label, name, got.shape, ref.shape)
    v, where = slice_errors(got, ref, axes)
    worst[name] = max(worst.get(name, 0.0), v)
    assert v <= tol, (label, name, v, where)


def _report(label, row, worst):
    print('%s %s worst per-slice error: %s' % (label, row, ', '.join('%s %.2e' % kv for kv in worst.items())))


def _leaves(tensors, dt=None):
    return [None if t is None else (t.clone().double() if dt else t.cuda()).requires_grad_(True) for t in tensors]


# ---- dense convolution ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _conv_reference(row, norm, dead=None):
    """Inputs and the fp64 results of a CONV row: (inputs, out, gradients, pre-norm result)."""
    from ghn3_amd import target_ops as T
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    x, w, gamma, beta, up = E.conv_inputs(row, 0 if norm else E.CONV_ONLY_SEED)
    if dead is not None:
        w[dead] = 0.0
    ref_in = _leaves((x, w, gamma, beta) if norm else (x, w), torch.float64)
    z = F.conv2d(F.relu(ref_in[0]) if relu else ref_in[0], ref_in[1], None, st, pad, dil)     # (the pre-norm result: statistics)
    ref = T.conv_reference(*ref_in, stride=st, padding=pad, dilation=dil, relu=relu) if norm else z
    (ref * up.double()).sum().backward()
    return (x, w, gamma, beta, up), ref.detach(), [t.grad for t in ref_in], z.detach()


def _run_conv(row, norm, dead=None):
    from ghn3_amd import target_ops as T
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    (x, w, gamma, beta, up), ref, ref_grads, z = _conv_reference(row, norm, dead)
    label = 'conv_bn' if norm else 'conv_only'
    var = z.var((0, 2, 3), unbiased=False) if z.numel() > Co else None
    keep = torch.arange(Co) != (-1 if dead is None else dead)
    if norm:
        assert float(var[keep].min()) >= E.VAR_FLOOR, float(var[keep].min())
    runs = []
    for _ in range(2):
        dev_in = _leaves((x, w, gamma, beta) if norm else (x, w))
        if norm:
            assert T.ConvBn.applicable(*dev_in)
            out, stats = T.conv_bn(dev_in[0], dev_in[1], dev_in[2], dev_in[3], stride=st, padding=pad, dilation=dil, relu=relu)
        else:
            assert T.ConvOnly.applicable(*dev_in)
            out, stats = T.conv_only(dev_in[0], dev_in[1], stride=st, padding=pad, dilation=dil, relu=relu), None
        assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
        (out * up.cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().cpu(), None if stats is None else stats.cpu(), [t.grad.cpu() for t in dev_in]))
    (out, stats, grads), (out2, stats2, grads2) = runs
    assert torch.equal(out2, out)                                   # deterministic: the same bits again,
    for name, a, b in zip(('dx', 'dw', 'dgamma', 'dbeta'), grads, grads2):
        assert torch.equal(a, b), name                              # ... the fixed-order reductions of the gradients included
    worst = {}
    _measure(label, 'out', out[:, keep], ref[:, keep], E.ACT_AXES, OUT_TOL, worst)
    if norm:
        _measure(label, 'mean', stats[:Co][keep], z.mean((0, 2, 3))[keep], E.VEC_AXES, OUT_TOL, worst)
        _measure(label, 'var', stats[2 * Co:][keep], var[keep], E.VEC_AXES, OUT_TOL, worst)
    _measure(label, 'dx', grads[0], ref_grads[0], E.ACT_AXES, GRAD_TOL, worst)
    _measure(label, 'dw', grads[1][keep], ref_grads[1][keep], E.WGRAD_AXES, GRAD_TOL, worst)
    if norm:
        _measure(label, 'dgamma', grads[2][keep], ref_grads[2][keep], E.VEC_AXES, GRAD_TOL, worst)
        _measure(label, 'dbeta', grads[3][keep], ref_grads[3][keep], E.VEC_AXES, GRAD_TOL, worst)
    if st[0] > dil * (k[0] - 1) + 1 and st[1] > dil * (k[1] - 1) + 1 and pad == (0, 0):
        # a stride larger than the kernel: the input pixels between two windows reach no output
        read = torch.zeros(H, W, dtype=torch.bool)
        for kh in range(k[0]):
            for kw in range(k[1]):
                read[kh * dil:kh * dil + st[0] * ref.shape[2]:st[0], kw * dil:kw * dil + st[1] * ref.shape[3]:st[1]] = True
        assert not read.all() and torch.equal(grads[0][:, :, ~read], torch.zeros_like(grads[0][:, :, ~read]))
    if dead is not None:
        assert all(torch.isfinite(t).all() for t in [out] + grads)
        assert torch.equal(out[:, dead], beta[dead].expand_as(out[:, dead]))       # pre-norm result exactly 0: out = beta, bit for bit
        assert float(stats[dead]) == 0.0 and float(stats[2 * Co + dead]) == 0.0
        assert float(grads[2][dead]) == 0.0                                        # dgamma = sum dout . xhat, xhat = 0
    _report(label, row, worst)


@pytest.mark.parametrize('row', E.CONV_ROWS, ids=str)
def test_conv_bn_edge_rows(row, buffers):
    _run_conv(row, True)


@pytest.mark.parametrize('row', E.CONV_ONLY_ROWS, ids=str)
def test_conv_only_edge_rows(row, buffers):
    _run_conv(row, False)


def test_conv_bn_with_a_dead_output_channel(buffers):
    _run_conv(E.CONV_DEAD[0], True, dead=E.CONV_DEAD[1])


# ---- ReLU -> depthwise -> pointwise -> norm, and the pointwise-only form -------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dwpw_reference(row, depthwise, dead=None):
    from ghn3_amd import target_ops as T
    if depthwise:
        N, Ci, Co, H, W, ks, st, pad, dil, gain = row
        x, w_dw, w_pw, gamma, beta, up = E.dwpw_inputs(row)
    else:
        (N, Ci, Co, H, W, st), ks, pad, dil = row, 1, 0, 1
        x, w_pw, gamma, beta, up = E.pw_inputs(row)
        w_dw = None
    if dead is not None:
        w_pw[dead] = 0.0
    ref_in = _leaves((x, w_dw, w_pw, gamma, beta), torch.float64)
    if depthwise:
        y = F.conv2d(F.relu(ref_in[0]), ref_in[1], None, st, pad, dil, groups=Ci)
        z = F.conv2d(y, ref_in[2])
        ref = T.reference(*ref_in, stride=st, padding=pad, dilation=dil)
    else:
        z = F.conv2d(F.relu(ref_in[0]), ref_in[2], None, st)
        ref = F.batch_norm(z, None, None, ref_in[3], ref_in[4], True, 0.1, 1e-5)
    (ref * up.double()).sum().backward()
    return (x, w_dw, w_pw, gamma, beta, up), (ks, st, pad, dil), ref.detach(), [None if t is None else t.grad for t in ref_in], z.detach()


def _run_dwpw(row, depthwise, dead=None):
    from ghn3_amd import target_ops as T
    (x, w_dw, w_pw, gamma, beta, up), (ks, st, pad, dil), ref, ref_grads, z = _dwpw_reference(row, depthwise, dead)
    label = 'dwpw_bn' if depthwise else 'pointwise'
    Co = w_pw.shape[0]
    var = z.var((0, 2, 3), unbiased=False)
    keep = torch.arange(Co) != (-1 if dead is None else dead)
    assert float(var[keep].min()) >= E.VAR_FLOOR, float(var[keep].min())
    runs = []
    for _ in range(2):
        dev_in = _leaves((x, w_dw, w_pw, gamma, beta))
        assert T.DwPwBn.applicable(dev_in[0], dev_in[1], dev_in[2], dev_in[3], dev_in[4], ks)
        out, stats = T.dwpw_bn(dev_in[0], dev_in[1], dev_in[2], dev_in[3], dev_in[4], stride=st, padding=pad, dilation=dil)
        assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
        (out * up.cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().cpu(), stats.cpu(), [None if t is None else t.grad.cpu() for t in dev_in]))
    (out, stats, grads), (out2, stats2, grads2) = runs
    names = ('dx', 'dw_dw', 'dw_pw', 'dgamma', 'dbeta')
    assert torch.equal(out2, out)
    for name, a, b in zip(names, grads, grads2):
        assert a is None or torch.equal(a, b), name
    worst = {}
    _measure(label, 'out', out[:, keep], ref[:, keep], E.ACT_AXES, OUT_TOL, worst)
    _measure(label, 'mean', stats[:Co][keep], z.mean((0, 2, 3))[keep], E.VEC_AXES, OUT_TOL, worst)
    _measure(label, 'var', stats[2 * Co:][keep], var[keep], E.VEC_AXES, OUT_TOL, worst)
    _measure(label, 'dx', grads[0], ref_grads[0], E.ACT_AXES, GRAD_TOL, worst)
    if depthwise:
        _measure(label, 'dw_dw', grads[1], ref_grads[1], E.WGRAD_AXES, GRAD_TOL, worst)
    _measure(label, 'dw_pw', grads[2][keep], ref_grads[2][keep], E.WGRAD_AXES, GRAD_TOL, worst)
    _measure(label, 'dgamma', grads[3][keep], ref_grads[3][keep], E.VEC_AXES, GRAD_TOL, worst)
    _measure(label, 'dbeta', grads[4][keep], ref_grads[4][keep], E.VEC_AXES, GRAD_TOL, worst)
    if dead is not None:
        assert all(torch.isfinite(t).all() for t in [out] + [t for t in grads if t is not None])
        assert torch.equal(out[:, dead], beta[dead].expand_as(out[:, dead]))
        assert float(stats[dead]) == 0.0 and float(stats[2 * Co + dead]) == 0.0
        assert float(grads[3][dead]) == 0.0
    _report(label, row, worst)


@pytest.mark.parametrize('row', E.DWPW_ROWS, ids=str)
def test_dwpw_bn_edge_rows(row, buffers):
    _run_dwpw(row, True)


@pytest.mark.parametrize('row', E.PW_ROWS, ids=str)
def test_pointwise_bn_edge_rows(row, buffers):
    _run_dwpw(row, False)


def test_dwpw_bn_with_a_dead_output_channel(buffers):
    _run_dwpw(E.DWPW_DEAD[0], True, dead=E.DWPW_DEAD[1])


# ---- squeeze-and-excitation through its module ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _se_reference(row):
    from ghn3_amd import ops
    N, C, H, W, stride = row
    x, up = E.se_inputs(row)
    torch.manual_seed(C + H)
    m = ops.ChannelSELayer(C, stride=stride)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(3.0)
    ref_m = ops.ChannelSELayer(C, stride=stride).double()
    ref_m.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    xr = x.double().requires_grad_(True)
    ref = ref_m(xr)
    (ref * up.double()).sum().backward()
    return x, up, m.state_dict(), ref.detach(), xr.grad, [(n, p.grad) for n, p in ref_m.named_parameters()]


@pytest.mark.parametrize('row', E.SE_ROWS, ids=str)
def test_squeeze_excitation_edge_rows(row, buffers):
    from ghn3_amd import ops, target_ops as T
    N, C, H, W, stride = row
    x, up, state, ref, ref_dx, ref_params = _se_reference(row)
    runs = []
    for _ in range(2):
        m = ops.ChannelSELayer(C, stride=stride)
        m.load_state_dict(state)
        m = m.cuda()
        xd = x.cuda().requires_grad_(True)
        assert T.SqueezeExcite.applicable(xd, m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias)
        assert m.fc1.weight.shape[0] == C // 2
        out = m(xd)
        assert 'SqueezeExcite' in _graph_nodes(out), _graph_nodes(out)       # (behind the stride slicing / a layout copy)
        (out * up.cuda()).sum().backward()
        torch.cuda.synchronize()
        runs.append((out.detach().cpu(), xd.grad.cpu(), [p.grad.cpu() for p in m.parameters()]))
    (out, dx, params), (out2, dx2, params2) = runs
    assert torch.equal(out2, out) and torch.equal(dx2, dx) and all(torch.equal(a, b) for a, b in zip(params, params2))
    worst = {}
    _measure('se', 'out', out, ref, E.ACT_AXES, SE_TOL, worst)
    _measure('se', 'dx', dx, ref_dx, E.ACT_AXES, SE_TOL, worst)
    for a, (name, b) in zip(params, ref_params):
        _measure('se', name, a, b, E.MAT_AXES if b.dim() == 2 else E.VEC_AXES, SE_PARAM_TOL, worst)
    _report('se', row, worst)


# ---- pooling through the light modules, tied maxima --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pool_reference(row, mode):
    N, C, H, W, k, s, pad = row
    x, up = E.pool_inputs(row, mode)
    xr = x.double().requires_grad_(True)
    ref = F.max_pool2d(xr, k, s, pad) if mode else F.avg_pool2d(xr, k, s, pad, count_include_pad=False)
    (ref * up.double()).sum().backward()
    return x, up, ref.detach(), xr.grad


@pytest.mark.parametrize('mode', [0, 1], ids=['avg', 'max'])
@pytest.mark.parametrize('row', E.POOL_ROWS, ids=str)
def test_pooling_edge_rows_with_ties(row, mode, buffers):
    from ghn3_amd import light_ops, target_ops as T
    N, C, H, W, k, s, pad = row
    x, up, ref, ref_dx = _pool_reference(row, mode)
    assert float((x == 0).float().mean()) >= 0.4                      # behind a ReLU: most windows hold several equal zeros
    m = light_ops.MaxPool2d(k, stride=s, padding=pad) if mode else light_ops.AvgPool2d(k, stride=s, padding=pad, count_include_pad=False)
    xd = x.cuda().requires_grad_(True)
    assert T.Pool2d.applicable(xd, k, s, pad)
    out = m(xd)
    assert 'Pool2d' in type(out.grad_fn).__name__, type(out.grad_fn).__name__
    assert out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
    (out * up.cuda()).sum().backward()
    torch.cuda.synchronize()
    out, dx = out.detach().cpu(), xd.grad.cpu()
    xd2 = x.cuda().requires_grad_(True)                                  # deterministic: the same bits again, both directions
    out2 = m(xd2)
    (out2 * up.cuda()).sum().backward()
    assert torch.equal(out2.detach().cpu(), out) and torch.equal(xd2.grad.cpu(), dx)
    worst = {}
    if mode:
        assert torch.equal(out.double(), ref)                           # bit-exact
        assert torch.equal(dx != 0, ref_dx != 0)                        # the FIRST maximum in scan order wins a tie, as in torch
    else:
        _measure('pool', 'out', out, ref, E.ACT_AXES, POOL_TOL, worst)
    _measure('pool', 'dx', dx, ref_dx, E.ACT_AXES, POOL_TOL, worst)
    _report('max_pool' if mode else 'avg_pool', row, worst)


# ---- the backward's reduced (sum dout, sum dout xhat) pair when dgamma does not follow dbeta -------------------------------------
# target_ops.py always lays dgamma directly behind dbeta, where the C side reduces the pair in place; any other caller gets it
# reduced into the scratch's s12 area and copied out.  Both ways must give the same bits: same kernels, same order.
APART_SHAPES = [(2, 9, 7, 2), (3, 9, 9, 1)]        # (N, H, W, stride), 8 -> 12 channels, 3 x 3, pad 1: P = 40 (one partial
#                                                     tile) and 243 (four tiles, the last partial)


@pytest.mark.parametrize('shape', APART_SHAPES, ids=str)
@pytest.mark.parametrize('fn', ['ghn3_dwpw_bn_bwd', 'ghn3_dwpw_frozen_bwd', 'ghn3_conv_bn_bwd', 'ghn3_conv_frozen_bwd'])
def test_backward_with_dgamma_apart_from_dbeta(fn, shape):
    import ctypes
    from ghn3_amd import _lib as L, target_ops as T
    (N, H, W, st), Ci, Co, ks, pad = shape, 8, 12, 3, 1
    Ho, Wo = (H + 2 * pad - ks) // st + 1, (W + 2 * pad - ks) // st + 1
    P = N * Ho * Wo
    dwpw, frozen = fn.startswith('ghn3_dwpw'), '_frozen_' in fn
    lib = L.load()
    if dwpw:
        d = T._Desc(N, H, W, Ci, Co, ks, st, pad, 1, Ho, Wo, 1e-5)
    else:
        d = T._ConvDesc(N, H, W, Ci, Co, ks, ks, st, st, pad, pad, 1, Ho, Wo, 1, 1e-5)
    size = getattr(lib, fn.replace('_bn_bwd', '_scratch_floats').replace('_bwd', '_scratch_floats'))
    n_scratch = int(size(ctypes.byref(d), 1))
    assert n_scratch > 0
    g = torch.Generator().manual_seed(P)
    rnd = lambda *s: torch.randn(*s, generator=g).cuda()
    dout, x, z, gamma = rnd(P, Co), rnd(N, H, W, Ci), rnd(P, Co), rnd(Co)
    weights = [rnd(Ci, ks, ks), rnd(Co, Ci)] if dwpw else [rnd(Co, Ci, ks, ks)]
    mean, var = z.mean(0), z.var(0, unbiased=False)
    stats = torch.cat([mean, (var + 1e-5).rsqrt(), var])
    norm_in = [mean, var] if frozen else []
    runs = []
    for apart in (False, True):
        nan = lambda *s: torch.full(s, float('nan'), device='cuda')
        dx, grads, scratch = nan(N, H, W, Ci), [nan(*w.shape) for w in weights], nan(n_scratch)
        if apart:
            dgamma, dbeta = nan(Co), nan(Co)
        else:
            pair = nan(2 * Co)
            dbeta, dgamma = pair[:Co], pair[Co:]
        assert (dgamma.data_ptr() == dbeta.data_ptr() + 4 * Co) != apart
        if frozen:
            args = [dout, x, z] + weights + [gamma] + norm_in
        else:
            args = [dout, x, z, stats] + weights + [gamma]
        args += [dx] + grads + [dgamma, dbeta, scratch]
        L._check(getattr(lib, fn)(ctypes.byref(d), *[t.data_ptr() for t in args], T._stream()), fn)
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in [dx] + grads + [dgamma, dbeta]])
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, b)
