"""CPU checks of the lean attention of the msa layers (include/ghn3_hip.h ghn3_attn_lean_*, ghn3_msa_lean_*;
target_ops.msa_lean): the exports and the host-side limits, the selection rule under its three settings, and the float64
reference of msa_lean_cases.py against torch float64 autograd."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import msa_lean_cases as M
from ghn3_amd import _lib as L
from ghn3_amd import target_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['ghn3_attn_lean_fwd', 'ghn3_attn_lean_bwd', 'ghn3_msa_lean_scratch_floats', 'ghn3_msa_lean_fwd',
               'ghn3_msa_lean_bwd']


def _lib():
    if not os.path.exists(L.LIB_PATH):
        from ghn3_amd import build
        build.build(verbose=False)
    return L.load()


def _desc(B, C, H, W, stride=1, heads=M.HEADS, hidden=None, layout=0):
    return T._MsaDesc(B, H, W, C, heads, C if hidden is None else hidden, stride, (H - 1) // stride + 1, (W - 1) // stride + 1,
                      layout, 1e-5, 0)


def test_exports_and_limits():
    lib = _lib()
    text = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    declared = set(re.findall(r'\b(ghn3_[a-z0-9_]+)\s*\(', text))
    h = ctypes.CDLL(L.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in L.EXPORTS and hasattr(h, s), s
    assert lib.ghn3_abi_version() == L.ABI_VERSION == 21
    # the shapes the saved-P path refuses (B heads N^2 >= 2^31): the GHN-3 recipe's 56 x 56 maps, and 64 x 64 maps
    for B, C, H, W in [(128, 64, 56, 56), (16, 32, 64, 64)]:
        d = _desc(B, C, H, W)
        assert B * M.HEADS * (H * W) ** 2 >= 2 ** 31
        assert lib.ghn3_msa_scratch_floats(ctypes.byref(d), 0) == -2 and lib.ghn3_msa_scratch_floats(ctypes.byref(d), 1) == -2
        fwd, bwd = lib.ghn3_msa_lean_scratch_floats(ctypes.byref(d), 0), lib.ghn3_msa_lean_scratch_floats(ctypes.byref(d), 1)
        R = B * H * W
        assert fwd >= R * 4 * C + R * (C + C) + B * M.HEADS * H * W and bwd >= R * 6 * C + R * (C + 2 * C), (fwd, bwd)
    # what neither path takes (the four descriptors of test_msa_cpu.py)
    for bad in [dict(B=2, C=512, H=4, W=4), dict(B=1, C=64, H=65, W=64), dict(B=2, C=60, H=4, W=4),
                dict(B=2, C=64, H=4, W=4, hidden=2048)]:
        for fn in (lib.ghn3_msa_lean_scratch_floats, lib.ghn3_msa_scratch_floats):
            for backward in (0, 1):
                assert fn(ctypes.byref(_desc(**bad)), backward) == -2, bad
                assert lib.ghn3_last_error()
    d = _desc(2, 64, 8, 8, 2)
    d.Ho = 3
    assert lib.ghn3_msa_lean_scratch_floats(ctypes.byref(d), 0) == -1
    # sizes where both paths apply: the lean state holds lse on top of the saved-P scratch and is smaller than that scratch
    # plus P (at a single token P and lse are the same B heads floats: equal)
    for (B, C, H, W, s), hidden in zip(M.LAYER_SHAPES, [32, 64, 128, 128, 256, 48, 64, 256, 32]):
        d = _desc(B, C, H, W, s, hidden=hidden)
        N, R, K = H * W, B * H * W, B * d.Ho * d.Wo
        lean, saved = lib.ghn3_msa_lean_scratch_floats(ctypes.byref(d), 0), lib.ghn3_msa_scratch_floats(ctypes.byref(d), 0)
        assert lean >= R * 4 * C + K * (C + hidden) + B * M.HEADS * N
        if N > 1:
            assert lean < saved + B * M.HEADS * N * N
        else:
            assert lean <= saved + B * M.HEADS * N * N
        assert lib.ghn3_msa_lean_scratch_floats(ctypes.byref(d), 1) == lib.ghn3_msa_scratch_floats(ctypes.byref(d), 1)


def test_selection_rule(monkeypatch):
    t = T.MSA_LEAN_THRESHOLD
    assert 2 ** 24 <= t <= 2 ** 31 and t & (t - 1) == 0
    shapes = [(B, M.HEADS, H * W) for B, C, H, W, s in M.LAYER_SHAPES]
    assert max(B * h * N * N for B, h, N in shapes) == 64 * 8 * 121 ** 2 < 2 ** 24
    new = [(16, M.HEADS, 4096), (128, M.HEADS, 56 * 56)]
    monkeypatch.delenv('GHN3_MSA_LEAN', raising=False)
    assert not any(T.msa_lean(*s) for s in shapes) and all(T.msa_lean(*s) for s in new)
    monkeypatch.setenv('GHN3_MSA_LEAN', 'auto')
    assert not any(T.msa_lean(*s) for s in shapes) and all(T.msa_lean(*s) for s in new)
    assert T.msa_lean(1, 1, 1) is False and T.msa_lean(t, 1, 1) is True
    monkeypatch.setenv('GHN3_MSA_LEAN', '0')
    assert not any(T.msa_lean(*s) for s in shapes + new)
    monkeypatch.setenv('GHN3_MSA_LEAN', '1')
    assert all(T.msa_lean(*s) for s in shapes + new)
    # the rule does not look at the grad mode
    monkeypatch.setenv('GHN3_MSA_LEAN', 'auto')
    with torch.no_grad():
        assert all(T.msa_lean(*s) for s in new) and not any(T.msa_lean(*s) for s in shapes)


def _torch_ref(q, k, v, g):
    q, k, v = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (q, k, v))
    S = (q @ k.T) / float(np.sqrt(q.shape[1]))
    out = torch.softmax(S, dim=1) @ v
    out.backward(torch.from_numpy(g.astype(np.float64)))
    return [out.detach().numpy(), torch.logsumexp(S, dim=1).detach().numpy(), q.grad.numpy(), k.grad.numpy(), v.grad.numpy()]


@pytest.mark.parametrize('case', M.OP_CASES[:-1])
def test_reference_matches_torch_float64_autograd(case):
    """The lse-form reference against autograd of softmax attention, both in float64, and -- printed, not asserted: it is the
    floor the tolerances stand on -- the same formula in numpy float32 against the reference."""
    q, k, v, g = M.inputs(case)
    ref = M.reference(case)
    names = ('out', 'lse', 'dq', 'dk', 'dv')
    theirs = {s: _torch_ref(q[s], k[s], v[s], g[s]) for s in M.ref_slices(case)}
    f32 = {s: M.attention_ref(q[s], k[s], v[s], g[s], dtype=np.float32) for s in M.ref_slices(case)}
    floors = []
    for i, n in enumerate(names):
        mine = [ref[s][i] for s in M.ref_slices(case)]
        err = np.sqrt(sum(float(((a - theirs[s][i]) ** 2).sum()) for a, s in zip(mine, M.ref_slices(case))))
        scale = np.sqrt(sum(float((theirs[s][i] ** 2).sum()) for s in M.ref_slices(case)))
        assert err <= 1e-12 * max(scale, 1.0), (n, err, scale)
        floors.append(M.rel_l2([f32[s][i] for s in M.ref_slices(case)], mine))
    S = max(float(np.abs(q[s].astype(np.float64) @ k[s].astype(np.float64).T).max()) / np.sqrt(case[3]) for s in M.ref_slices(case))
    print('case %s: max |scale S| %.1f, float32 floor %s' % (case, S, ' '.join('%s %.1e' % f for f in zip(names, floors))))
    if case[2] > 1:
        assert max(floors[:2]) < M.OUT_TOL / 4 and max(floors[2:]) < M.GRAD_TOL / 4, floors
    if case[4]:                              # a ramp case: the maximum of most rows lies beyond the first key tile
        moved = np.mean([(np.argmax(q[s].astype(np.float64) @ k[s].astype(np.float64).T, axis=1) >= 32).mean()
                         for s in M.ref_slices(case)])
        assert moved > 0.4 and S > 50, (moved, S)
