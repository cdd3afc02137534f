"""CPU checks of the wide msa path (include/ghn3_hip.h ghn3_attn_wide_*, ghn3_msa_wide_*; target_ops.MsaWideLayer): the
exports, the host-side limits of ghn3_msa_wide_scratch_floats next to the unchanged refusals of the two older functions, and
`MsaWideLayer.applicable` under GHN3_NATIVE_MSA_WIDE unset, 0 and 1."""
import ctypes
import os
import re

import pytest
import torch

import msa_wide_cases as M
from ghn3_amd import _lib as L
from ghn3_amd import target_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['ghn3_attn_wide_fwd', 'ghn3_attn_wide_bwd', 'ghn3_msa_wide_scratch_floats', 'ghn3_msa_wide_fwd',
               'ghn3_msa_wide_bwd']


def _lib():
    if not os.path.exists(L.LIB_PATH):
        from ghn3_amd import build
        build.build(verbose=False)
    return L.load()


def _desc(B, C, H, W, stride=1, heads=8, hidden=None, layout=0):
    return T._MsaDesc(B, H, W, C, heads, C if hidden is None else hidden, stride, (H - 1) // stride + 1, (W - 1) // stride + 1,
                      layout, 1e-5, 0)


def test_exports_and_abi_version():
    lib = _lib()
    text = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    declared = set(re.findall(r'\b(ghn3_[a-z0-9_]+)\s*\(', text))
    h = ctypes.CDLL(L.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.EXPORTS and hasattr(h, s), s
    assert lib.ghn3_abi_version() == L.ABI_VERSION == 21
    from ghn3_amd import build
    assert 'tnet_msa_wide.hip' in build.SOURCES


@pytest.mark.parametrize('case', M.LAYER_CASES)
def test_scratch_size_accepts_the_layer_cases(case):
    B, C, heads, H, W, s, cl, ratio, qb = case
    lib = _lib()
    hidden = C * ratio
    d = _desc(B, C, H, W, s, heads=heads, hidden=hidden, layout=int(cl))
    fwd, bwd = lib.ghn3_msa_wide_scratch_floats(ctypes.byref(d), 0), lib.ghn3_msa_wide_scratch_floats(ctypes.byref(d), 1)
    R, K = B * H * W, B * d.Ho * d.Wo
    assert fwd >= R * 4 * C + K * (C + hidden) + B * heads * H * W, fwd      # qkv, O, y1, pre-GELU values, lse
    assert bwd >= R * 3 * C + 2 * R * C + K * hidden, bwd                    # dqkv, dO, dy1, dh


@pytest.mark.parametrize('bad', M.REFUSED)
def test_scratch_size_refuses_what_is_outside_the_wide_limits(bad):
    lib = _lib()
    for backward in (0, 1):
        assert lib.ghn3_msa_wide_scratch_floats(ctypes.byref(_desc(**bad)), backward) == -2, bad      # GHN3_E_LIMIT
        assert b'msa wide' in lib.ghn3_last_error()


def test_mismatched_output_grid_is_an_argument_error():
    lib = _lib()
    d = _desc(2, 512, 8, 8, 2)
    d.Ho = 3
    assert lib.ghn3_msa_wide_scratch_floats(ctypes.byref(d), 0) == -1


def test_the_older_entry_points_still_refuse_their_four_descriptors():
    lib = _lib()
    for bad in [dict(B=2, C=512, H=4, W=4), dict(B=1, C=64, H=65, W=64), dict(B=2, C=60, H=4, W=4),
                dict(B=2, C=64, H=4, W=4, hidden=2048)]:
        for fn in (lib.ghn3_msa_lean_scratch_floats, lib.ghn3_msa_scratch_floats):
            for backward in (0, 1):
                assert fn(ctypes.byref(_desc(**bad)), backward) == -2, bad
                assert lib.ghn3_last_error()


# ---- MsaWideLayer.applicable ----------------------------------------------------------------------------------------------
# (C, heads, mlp_ratio, input shape B H W)
NARROW = [(64, 8, 1, (2, 4, 4)), (256, 8, 4, (2, 3, 3)), (32, 1, 1, (1, 1, 1)), (128, 4, 8, (2, 2, 2))]
WIDE = [(C, heads, ratio, (B, H, W)) for B, C, heads, H, W, s, cl, ratio, qb in M.LAYER_CASES]
OUTSIDE = [
    (1088, 17, 1, (1, 2, 2)),        # C above 1024 at head dim 64
    (520, 8, 1, (1, 2, 2)),          # head dim 65
    (100, 4, 41, (1, 2, 2)),         # hidden 4100
    (40, 1, 1, (1, 65, 64)),         # 4160 tokens
    (40, 1, 1, (65536, 1, 1)),       # more than 65535 sequences
]


@pytest.fixture
def on_cpu(monkeypatch):
    """CPU tensors pass for CUDA ones: `_f32_cuda` (which `_native_input` asks too) looks at the dtype alone."""
    monkeypatch.setattr(T, '_f32_cuda', lambda *ts: all(torch.is_tensor(t) and t.dtype == torch.float32 for t in ts))
    for name in ('OPS', 'MSA', 'AMP', 'MSA_WIDE'):
        monkeypatch.delenv('GHN3_NATIVE_' + name, raising=False)
    monkeypatch.delenv('GHN3_MSA_LEAN', raising=False)


def _stand_in(C, heads, ratio, bhw):
    from ghn3_amd import ops
    layer = ops.TransformerLayer(C, num_heads=heads, mlp_ratio=ratio)
    return layer, torch.zeros(bhw[0], C, bhw[1], bhw[2])


def test_applicable_follows_the_switch_and_the_limits(on_cpu, monkeypatch):
    narrow, wide, outside = ([_stand_in(*c) for c in cs] for cs in (NARROW, WIDE, OUTSIDE))
    assert all(T.MsaLayer.applicable(l, x) for l, x in narrow)
    assert not any(T.MsaLayer.applicable(l, x) for l, x in wide + outside)
    for setting in (None, '0', '1'):
        if setting is not None:
            monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', setting)
        assert not any(T.MsaWideLayer.applicable(l, x) for l, x in narrow + outside), setting
        got = [T.MsaWideLayer.applicable(l, x) for l, x in wide]
        assert got == [setting == '1'] * len(wide), (setting, got)
        assert all(T.MsaLayer.applicable(l, x) for l, x in narrow), setting           # (the narrow routing does not move)
    # whatever `applicable` lets through, the C check takes: no GHN3_E_LIMIT in the middle of a network
    lib = _lib()
    for (l, x), (C, heads, ratio, (B, H, W)) in zip(wide, WIDE):
        d = _desc(B, C, H, W, heads=heads, hidden=C * ratio)
        assert lib.ghn3_msa_wide_scratch_floats(ctypes.byref(d), 0) > 0 and lib.ghn3_msa_wide_scratch_floats(ctypes.byref(d), 1) > 0
    for C, heads, ratio, (B, H, W) in OUTSIDE:
        assert lib.ghn3_msa_wide_scratch_floats(ctypes.byref(_desc(B, C, H, W, heads=heads, hidden=C * ratio)), 0) == -2


def test_the_other_conditions_of_the_narrow_op_hold_for_the_wide_one(on_cpu, monkeypatch):
    monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', '1')
    layer, x = _stand_in(512, 8, 1, (2, 4, 4))
    assert T.MsaWideLayer.applicable(layer, x)
    for name in ('GHN3_NATIVE_MSA', 'GHN3_NATIVE_OPS'):
        monkeypatch.setenv(name, '0')
        assert not T.MsaWideLayer.applicable(layer, x), name
        monkeypatch.delenv(name)
    with monkeypatch.context() as m:
        m.setenv('GHN3_NATIVE_AMP', '0')
        m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
        assert not T.MsaWideLayer.applicable(layer, x)
    assert T.MsaWideLayer.applicable(layer, x)
    assert not T.MsaWideLayer.applicable(layer, x.double()) and not T.MsaWideLayer.applicable(layer, x[0])
    layer.train()
    layer.ff.net[2] = torch.nn.Dropout(0.3)
    assert not T.MsaWideLayer.applicable(layer, x)                                   # an active dropout
    layer.eval()
    assert T.MsaWideLayer.applicable(layer, x)
    layer.ff.net[1] = torch.nn.GELU(approximate='tanh')
    assert not T.MsaWideLayer.applicable(layer, x)
    layer.ff.net[1] = torch.nn.GELU()
    layer.ln2.eps = 1e-6
    assert not T.MsaWideLayer.applicable(layer, x)                                   # two different eps


def test_run_msa_layer_tries_the_narrow_op_then_the_wide_one(on_cpu, monkeypatch):
    seen = []
    monkeypatch.setattr(T.MsaLayer, 'apply', lambda x, cfg, *p: (seen.append('narrow'), torch.zeros(1, 1, 1, 1))[1])
    monkeypatch.setattr(T.MsaWideLayer, 'apply', lambda x, cfg, *p: (seen.append('wide'), torch.zeros(1, 1, 1, 1))[1])
    monkeypatch.setattr(T, '_hand_on', lambda y, *a: y)
    narrow, wide = _stand_in(64, 8, 1, (2, 4, 4)), _stand_in(512, 8, 1, (2, 4, 4))
    assert T.run_msa_layer(*narrow) is not None and T.run_msa_layer(*wide) is None
    monkeypatch.setenv('GHN3_NATIVE_MSA_WIDE', '1')
    assert T.run_msa_layer(*narrow) is not None and T.run_msa_layer(*wide) is not None
    assert seen == ['narrow', 'narrow', 'wide']
