"""Host-only checks of the wide target-network layers (tests/wide_cases.py; the kernels are tested in
tests/test_gpu_target_wide.py):

  * the stand-alone depthwise op's entry points are declared and exported; the ABI version stays (symbols only, as for the
    earlier slices: tests/test_nonorm_cpu.py, test_evalbn_cpu.py, test_head_cpu.py, test_msa_lean_cpu.py and
    test_adamw_state16_cpu.py pin it at 21);
  * ghn3_conv_scratch_floats and ghn3_dw_scratch_floats answer the layout include/ghn3_hip.h documents up to C_out = 4096,
    C_in = 16384 and a depthwise C = 16384, and GHN3_E_LIMIT (-2) beyond or for a channel count that is no multiple of four;
  * `width_mult` of the architecture sampler scales C and nothing else, makes no random draw, and is 1 by default;
  * `applicable` follows the lifted limits and GHN3_NATIVE_WIDE; on CPU tensors every runner returns what the stock layers do;
  * every row with batch statistics keeps the project's variance floor in the fp64 reference (why the rows carry a gain).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import target_edge_cases as E
import wide_cases as Wd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('ghn3_dw_scratch_floats', 'ghn3_dw_fwd', 'ghn3_dw_bwd')
E_LIMIT = -2


def _lib():
    from ghn3_amd import _lib as L
    return L.load()


def test_the_depthwise_entry_points_are_declared_and_exported():
    from ghn3_amd import _lib as L
    header = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    lib = _lib()
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in L.EXPORTS and hasattr(lib, name), name
    assert lib.ghn3_abi_version() == L.ABI_VERSION
    assert re.search(r'#define\s+GHN3_ABI_VERSION\s+%d\b' % L.ABI_VERSION, header)


# ---- scratch sizes ---------------------------------------------------------------------------------------------------------
def _cdesc(N, Ci, Co, H, W, k, st, pad):
    from ghn3_amd import target_ops as T
    Ho, Wo = E.conv_out_hw(H, W, (k, k), (st, st), (pad, pad), 1)
    return T._ConvDesc(N, H, W, Ci, Co, k, k, st, st, pad, pad, 1, Ho, Wo, 1, 1e-5)


def _ceil(a, b):
    return -(-a // b)


def _conv_layout(d, backward):
    """The size include/ghn3_hip.h documents for ghn3_conv_scratch_floats."""
    P, taps = d.N * d.Ho * d.Wo, d.kh * d.kw
    tiles = _ceil(P, 64)
    pack = lambda rows, k: _ceil(_ceil(3 * taps * rows * (_ceil(k, 32) * 32), 2), 4) * 4
    if not backward:
        return 2 * tiles * d.C_out + pack(d.C_out, d.C_in) + 64
    n = max(1, min(_ceil(768, _ceil(d.C_out, 64) * _ceil(d.C_in, 64) * taps), _ceil(P, 32)))
    chunks = _ceil(P, 32 * _ceil(_ceil(P, n), 32))
    return 2 * tiles * d.C_out + 2 * d.C_out + pack(d.C_in, d.C_out) + chunks * taps * d.C_out * d.C_in + P * d.C_out + 256


WIDE_CONV = [(2, 12, 516, 3, 3, 3, 1, 1), (2, 8, 1028, 2, 2, 1, 1, 0), (1, 16, 4096, 4, 4, 3, 2, 1), (1, 16384, 8, 1, 2, 1, 1, 0),
             (2, 1028, 1028, 2, 2, 1, 1, 0), (70, 516, 520, 3, 3, 3, 1, 1)]


@pytest.mark.parametrize('shape', WIDE_CONV, ids=str)
def test_conv_scratch_sizes_follow_the_documented_layout(shape):
    lib = _lib()
    d = _cdesc(*shape)
    for backward in (0, 1):
        n = int(lib.ghn3_conv_scratch_floats(ctypes.byref(d), backward))
        assert n > 0 and n == _conv_layout(d, backward), (backward, n, _conv_layout(d, backward))


def test_conv_scratch_refuses_beyond_the_limits():
    lib = _lib()
    for shape in [(2, 12, 4100, 3, 3, 3, 1, 1), (1, 16388, 8, 1, 2, 1, 1, 0), (2, 12, 518, 3, 3, 3, 1, 1), (2, 10, 516, 3, 3, 3, 1, 1),
                  (1, 16384, 4096, 4, 4, 4, 1, 0)]:                       # (the last: 2^30 weights)
        d = _cdesc(*shape)
        for fn in (lib.ghn3_conv_scratch_floats, lib.ghn3_conv_frozen_scratch_floats):
            assert [int(fn(ctypes.byref(d), b)) for b in (0, 1)] == [E_LIMIT, E_LIMIT], shape
    assert b'4096' in lib.ghn3_last_error() or b'2^30' in lib.ghn3_last_error()
    d = _cdesc(2, 12, 516, 3, 3, 3, 1, 1)
    d.Ho += 1
    assert int(lib.ghn3_conv_scratch_floats(ctypes.byref(d), 0)) == -1     # GHN3_E_ARG: not a limit


def _dwdesc(N, C, H, W, ks, st, pad, dil):
    from ghn3_amd import target_ops as T
    Ho, Wo = E.conv_out_hw(H, W, (ks, ks), (st, st), (pad, pad), dil)
    return T._Desc(N, H, W, C, C, ks, st, pad, dil, Ho, Wo, 0.0)


@pytest.mark.parametrize('row', Wd.DW_ROWS + [(40, 1028, 9, 9, 3, 1, 1, 1)], ids=str)
def test_depthwise_scratch_sizes_follow_the_documented_layout(row):
    lib = _lib()
    d = _dwdesc(*row)
    P = d.N * d.Ho * d.Wo
    px = max(16, min(128, _ceil(_ceil(P, 256), 16) * 16))
    assert int(lib.ghn3_dw_scratch_floats(ctypes.byref(d), 0)) == 0
    n = int(lib.ghn3_dw_scratch_floats(ctypes.byref(d), 1))
    assert n > 0 and n == _ceil(P, px) * d.ks * d.ks * d.C_in + 256, n


def test_depthwise_scratch_refuses_beyond_the_limits():
    lib = _lib()
    for row in [(1, 16388, 2, 2, 5, 2, 2, 1), (2, 18, 3, 3, 3, 1, 1, 1), (1, 8, 16, 16, 9, 1, 4, 1)]:
        d = _dwdesc(*row)
        assert [int(lib.ghn3_dw_scratch_floats(ctypes.byref(d), b)) for b in (0, 1)] == [E_LIMIT, E_LIMIT], row
    d = _dwdesc(2, 16, 3, 3, 3, 1, 1, 1)
    d.C_out = 20
    assert int(lib.ghn3_dw_scratch_floats(ctypes.byref(d), 1)) == -1        # GHN3_E_ARG: the op keeps the channel count
    d = _dwdesc(2, 16384, 256, 256, 3, 1, 1, 1)                              # 2^31 activations
    assert int(lib.ghn3_dw_scratch_floats(ctypes.byref(d), 1)) == E_LIMIT


def test_the_se_entry_points_refuse_beyond_4096_channels():
    lib = _lib()
    one = ctypes.c_void_p(64)                                                # (never dereferenced: the size check comes first)
    assert lib.ghn3_se_fwd(1, 1, 4100, 8, one, one, one, one, one, one, one, None) == E_LIMIT
    assert lib.ghn3_se_fwd(1, 1, 8, 4097, one, one, one, one, one, one, one, None) == E_LIMIT
    assert lib.ghn3_se_fwd(1, 1, 1030, 8, one, one, one, one, one, one, one, None) == E_LIMIT   # C % 4


# ---- the architecture sampler ----------------------------------------------------------------------------------------------
def _plain(args):
    a = dict(args)
    g = a.pop('genotype')
    return a, (list(g.normal), list(g.normal_concat), list(g.reduce), list(g.reduce_concat))


def test_width_mult_scales_c_alone_and_draws_nothing():
    from ghn3_amd.deepnets1m import SampledNets, sample_net_args
    for seed in range(200):
        for large in (False, True):
            rngs = [np.random.RandomState(seed) for _ in range(3)]
            base = sample_net_args(rngs[0], large)
            one = sample_net_args(rngs[1], large, width_mult=1)
            wide = sample_net_args(rngs[2], large, width_mult=4)
            assert _plain(base) == _plain(one)
            assert wide['C'] == 4 * base['C']
            assert _plain(dict(wide, C=base['C'])) == _plain(base)
            assert rngs[0].rand() == rngs[1].rand() == rngs[2].rand()      # the generators stand where they stood
    a, b = SampledNets(seed=0, max_nodes=400)[2], SampledNets(seed=0, max_nodes=400, width_mult=4)[2]
    assert b.net_args['C'] == 4 * a.net_args['C'] and _plain(dict(b.net_args, C=a.net_args['C'])) == _plain(a.net_args)
    assert max(e['sz'][0] for cell in b.net._layered_modules for e in cell.values()) > 512


# ---- applicable, the switch, CPU tensors -------------------------------------------------------------------------------------
class _Cuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: what `applicable` decides is a matter of shapes and types."""
    is_cuda = True


def _c(*shape):
    return torch.empty(1).expand(*shape).as_subclass(_Cuda)      # (one element, whatever the shape)


def test_applicable_follows_the_lifted_limits_and_the_switch(monkeypatch):
    from ghn3_amd import target_ops as T
    monkeypatch.delenv('GHN3_NATIVE_WIDE', raising=False)
    assert T.CONV_MAX_IN == 16384 and T.CONV_MAX_OUT == 4096 and T.DW_MAX == 16384 and T.SE_MAX == 4096
    narrow = (_c(1, 8, 2, 2), _c(512, 8, 1, 1))
    wide_out, wide_in = (_c(1, 8, 2, 2), _c(516, 8, 1, 1)), (_c(1, 4100, 1, 1), _c(8, 4100, 1, 1))
    widest = (_c(1, 16384, 1, 1), _c(4096, 16384, 1, 1))
    for x, w in (narrow, wide_out, wide_in, widest):
        assert T.ConvOnly.applicable(x, w) and T.ConvBn.applicable(x, w, _c(w.shape[0]), _c(w.shape[0]))
    assert not T.ConvOnly.applicable(_c(1, 8, 2, 2), _c(4100, 8, 1, 1))
    assert not T.ConvOnly.applicable(_c(1, 16388, 1, 1), _c(8, 16388, 1, 1))
    assert not T.ConvOnly.applicable(_c(1, 16384, 4, 4), _c(4096, 16384, 4, 4))          # 2^30 weights
    assert T.Depthwise.applicable(_c(1, 16384, 2, 2), _c(16384, 1, 5, 5), 2, 2, 1)
    assert not T.Depthwise.applicable(_c(1, 16388, 2, 2), _c(16388, 1, 5, 5), 2, 2, 1)
    assert not T.Depthwise.applicable(_c(1, 18, 2, 2), _c(18, 1, 3, 3), 1, 1, 1)
    assert not T.Depthwise.applicable(_c(1, 16, 2, 2), _c(16, 1, 3, 3), 1, 0, 1)          # no output pixel
    assert not T.Depthwise.applicable(_c(1, 16, 2, 2), _c(16, 2, 3, 3), 1, 1, 1)          # not a depthwise weight
    se = lambda C, J: T.SqueezeExcite.applicable(_c(1, C, 1, 1), _c(J, C), _c(J), _c(C, J), _c(C))
    assert se(1024, 512) and se(1028, 514) and se(4096, 4096) and not se(4100, 8) and not se(8, 4097)
    # the fused depthwise + pointwise members keep their width: wider chains take the two-node form
    assert not T.DwPw.applicable(_c(1, 516, 2, 2), _c(516, 1, 3, 3), _c(516, 516), 3)
    monkeypatch.setenv('GHN3_NATIVE_WIDE', '0')
    assert T.ConvOnly.applicable(*narrow) and se(1024, 512)
    assert T.ConvOnly.applicable(_c(1, 4096, 1, 1), _c(8, 4096, 1, 1))                    # (the parent took such inputs)
    for x, w in (wide_out, wide_in, widest):
        assert not T.ConvOnly.applicable(x, w) and not T.ConvBn.applicable(x, w, _c(w.shape[0]), _c(w.shape[0]))
    assert not se(1028, 514)


@pytest.mark.parametrize('norm', ['bn-track', None])
@pytest.mark.parametrize('name', list(Wd.MODULES))
def test_on_cpu_tensors_the_runners_return_what_the_stock_layers_return(name, norm):
    from ghn3_amd import ops, target_ops as T
    kind, args, C_in = Wd.MODULES[name]
    torch.manual_seed(3)
    m = getattr(ops, kind)(*args, norm=norm)
    x = torch.randn(2, C_in, 4, 4)
    layers = list(m.op)
    for train in (True, False):
        m.train(train)
        want = m.op(x)
        if kind == 'SepConv':
            got = T.run_block(layers[4:], T.run_block(layers[:4], x, keep_layout=True))
        else:
            got = (T.run_block if kind == 'DilConv' else T.run_pointwise_block)(layers, x)
        assert got.grad_fn is not None and 'Depthwise' not in type(got.grad_fn).__name__
        assert torch.equal(got, want) and torch.equal(m(x), want)
    with pytest.raises(Exception):
        T.depthwise_relu(x, torch.randn(C_in, 1, 3, 3), padding=1)          # no CPU implementation
    se = ops.ChannelSELayer(1028)
    xs = torch.randn(2, 1028, 1, 1)
    assert T.run_se_layer(se.fc1, se.fc2, xs) is None and se(xs).shape == xs.shape


# ---- conditioning of the GPU rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', Wd.CONV_ROWS, ids=str)
def test_norm_rows_keep_the_variance_floor(row):
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    x, w, gamma, beta, up, rm, rv = Wd.conv_inputs(row, 'norm')
    z = F.conv2d(F.relu(x.double()) if relu else x.double(), w.double(), None, st, pad, dil)
    assert z.shape[1] == Co and z.numel() // Co >= 2
    var = z.var((0, 2, 3), unbiased=False)
    print(row, 'smallest batch variance %.3f of %d channels over %d pixels' % (float(var.min()), Co, z.numel() // Co))
    assert float(var.min()) >= E.VAR_FLOOR, float(var.min())
    # the frozen member normalises with drawn statistics: their variances are at least 0.5
    assert float(Wd.conv_inputs(row, 'frozen')[6].min()) >= 0.5 > E.VAR_FLOOR
