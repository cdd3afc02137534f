"""Host-only checks of the patch-embedding op (tests/patch_cases.py; the kernels are tested in tests/test_gpu_target_patch.py):

  * the three entry points are declared, exported and listed in _lib.EXPORTS; the ABI version stays 21 (symbols only);
  * ghn3_patch_scratch_floats answers the layout include/ghn3_hip.h documents, GHN3_E_LIMIT (-2) beyond each limit and GHN3_E_ARG
    (-1) for an output size that does not follow from the arithmetic;
  * `PatchEmbed.applicable` refuses the same rows on stand-in tensors and takes the rows the C side takes;
  * on CPU tensors `run_conv_layer` returns what the stock layer returns, bit for bit.
"""
import ctypes
import os
import re

import pytest
import torch

import patch_cases as Pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('ghn3_patch_scratch_floats', 'ghn3_patch_fwd', 'ghn3_patch_bwd')
E_ARG, E_LIMIT = -1, -2


def _lib():
    from ghn3_amd import _lib as L
    return L.load()


def test_the_patch_entry_points_are_declared_and_exported():
    from ghn3_amd import _lib as L
    header = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    lib = _lib()
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in L.EXPORTS and hasattr(lib, name), name


def test_the_abi_version_is_still_21():
    from ghn3_amd import _lib as L
    header = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    assert _lib().ghn3_abi_version() == L.ABI_VERSION == 21
    assert re.search(r'#define\s+GHN3_ABI_VERSION\s+21\b', header)


def _desc(N, Ci, H, W, k, st, Co, nhwc=0):
    from ghn3_amd import target_ops as T
    Ho, Wo = Pc.out_hw(H, W, k, st)
    return T._PatchDesc(N, H, W, Ci, Co, k[0], k[1], st[0], st[1], Ho, Wo, nhwc)


def _ceil(a, b):
    return -(-a // b)


def _layout(d):
    """The backward size include/ghn3_hip.h documents for ghn3_patch_scratch_floats."""
    K, P = d.C_in * d.kh * d.kw, d.N * d.Ho * d.Wo
    tiles = _ceil(d.C_out, 32) * _ceil(K, 32)
    n = max(1, min(_ceil(1024, tiles), _ceil(P, 64)))
    px = _ceil(_ceil(P, n), 16) * 16
    chunks = _ceil(P, px)
    return _ceil(chunks * d.C_out * K, 64) * 64 if chunks > 1 else 0


WORKLOAD = [(64, 3, 224, 224, (16, 16), (16, 16), C) for C in (32, 64, 128)]


@pytest.mark.parametrize('row', [r[:7] for r in Pc.ROWS] + Pc.TAKEN + WORKLOAD, ids=str)
def test_scratch_sizes_follow_the_documented_layout(row):
    lib = _lib()
    for nhwc in (0, 1):
        d = _desc(*row, nhwc=nhwc)
        assert int(lib.ghn3_patch_scratch_floats(ctypes.byref(d), 0)) == 0
        n = int(lib.ghn3_patch_scratch_floats(ctypes.byref(d), 1))
        assert n == _layout(d), (n, _layout(d))
    # (both branches of the layout are among the rows: one chunk -> no partials, several -> chunks C_out K)


def test_the_rows_cover_both_branches_of_the_layout():
    sizes = [_layout(_desc(*r[:7])) for r in Pc.ROWS]
    assert 0 in sizes and any(s > 0 for s in sizes)


@pytest.mark.parametrize('name', list(Pc.REFUSED))
def test_scratch_refuses_beyond_the_limits(name):
    lib = _lib()
    d = _desc(*Pc.REFUSED[name])
    assert [int(lib.ghn3_patch_scratch_floats(ctypes.byref(d), b)) for b in (0, 1)] == [E_LIMIT, E_LIMIT], name
    assert lib.ghn3_last_error()


def test_scratch_answers_e_arg_for_an_inconsistent_output_size():
    lib = _lib()
    d = _desc(*Pc.ROWS[0][:7])
    assert int(lib.ghn3_patch_scratch_floats(ctypes.byref(d), 0)) == 0
    d.Ho += 1
    assert int(lib.ghn3_patch_scratch_floats(ctypes.byref(d), 0)) == E_ARG
    d = _desc(*Pc.ROWS[0][:7])
    d.nhwc = 2
    assert int(lib.ghn3_patch_scratch_floats(ctypes.byref(d), 1)) == E_ARG
    d = _desc(1, 3, 8, 32, (16, 16), (16, 16), 8)                         # an image smaller than the kernel: no output pixel
    assert int(lib.ghn3_patch_scratch_floats(ctypes.byref(d), 0)) == E_ARG


# ---- applicable ------------------------------------------------------------------------------------------------------------
class _Cuda(torch.Tensor):
    """A CPU tensor that says it lives on the GPU: what `applicable` decides is a matter of shapes and types."""
    is_cuda = True


def _c(*shape, dtype=torch.float32):
    return torch.empty(1, dtype=dtype).expand(*shape).as_subclass(_Cuda)      # (one element, whatever the shape)


def _standins(N, Ci, H, W, k, st, Co):
    return _c(N, Ci, H, W), _c(Co, Ci, *k)


def test_applicable_agrees_with_the_c_side(monkeypatch):
    from ghn3_amd import target_ops as T
    for var in ('GHN3_NATIVE_OPS', 'GHN3_NATIVE_CONV', 'GHN3_NATIVE_AMP'):
        monkeypatch.delenv(var, raising=False)
    lib = _lib()
    for name, row in Pc.REFUSED.items():
        x, w = _standins(*row)
        assert not T.PatchEmbed.applicable(x, w, row[5], 0, 1), name
    for row in [r[:7] for r in Pc.ROWS] + Pc.TAKEN + WORKLOAD:
        x, w = _standins(*row)
        assert T.PatchEmbed.applicable(x, w, row[5], 0, 1), row
        assert int(lib.ghn3_patch_scratch_floats(ctypes.byref(_desc(*row)), 1)) >= 0, row
    row = Pc.ROWS[0][:7]
    x, w = _standins(*row)
    assert not T.PatchEmbed.applicable(x, w, row[5], 1, 1)                   # padding
    assert not T.PatchEmbed.applicable(x, w, row[5], 0, 2)                   # dilation
    assert not T.PatchEmbed.applicable(x, w, row[5], 'same', 1)
    assert not T.PatchEmbed.applicable(_c(1, 3, 8, 32), w, row[5], 0, 1)     # no output pixel
    assert not T.PatchEmbed.applicable(_c(2, 4, 32, 32), w, row[5], 0, 1)    # the weight has three input channels
    assert not T.PatchEmbed.applicable(_c(2, 3, 32, 32, dtype=torch.float16), w, row[5], 0, 1)
    assert not T.PatchEmbed.applicable(torch.empty(2, 3, 32, 32), torch.empty(8, 3, 16, 16), row[5], 0, 1)   # CPU tensors
    # what the dense-convolution op takes stays there: the CIFAR patch embedding
    assert not T.PatchEmbed.applicable(_c(2, 3, 32, 32), _c(32, 3, 3, 3), 3, 1, 1)
    for var in ('GHN3_NATIVE_OPS', 'GHN3_NATIVE_CONV'):
        monkeypatch.setenv(var, '0')
        assert not T.PatchEmbed.applicable(x, w, row[5], 0, 1), var
        monkeypatch.delenv(var)
    assert T.PatchEmbed.applicable(x, w, row[5], 0, 1)


@pytest.mark.parametrize('light', [False, True], ids=['torch', 'light'])
@pytest.mark.parametrize('shape', [(3, 32, 16, 16, 0, 32), (3, 32, 3, 3, 1, 32), (3, 8, 9, 9, 0, 27)], ids=str)
def test_on_cpu_tensors_run_conv_layer_returns_what_the_stock_layer_returns(shape, light):
    from ghn3_amd import light_ops, target_ops as T
    Ci, Co, k, st, pad, side = shape
    torch.manual_seed(5)
    if light:
        conv = light_ops.Conv2d(Ci, Co, k, stride=st, padding=pad, bias=False)
        conv.weight = (torch.randn(Co, Ci, k, k) / k).requires_grad_(True)
    else:
        conv = torch.nn.Conv2d(Ci, Co, k, stride=st, padding=pad, bias=False)
    x = torch.randn(2, Ci, side, side)
    got, want = T.run_conv_layer(conv, x), conv(x)
    assert type(got.grad_fn).__name__ == type(want.grad_fn).__name__ and 'PatchEmbed' not in type(got.grad_fn).__name__
    assert torch.equal(got, want)
    with pytest.raises(Exception):
        T.patch_embed(x, conv.weight, st)                                    # no CPU implementation
