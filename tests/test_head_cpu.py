"""CPU checks of the classifier head's and the cross-entropy's C ABI (include/ghn3_hip.h ghn3_head_* / ghn3_xent_*): the ctypes
mirrors have the C layout, ghn3_head_scratch_floats (host only) refuses what the kernels do not take and sizes what they do, and
ClassifierHead's shape rule (the part of `applicable` that mirrors the C limits) agrees with it; the stock fallback of
meta_cross_entropy on CPU tensors."""
import ctypes
import itertools
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from ghn3_amd import _lib as L
from ghn3_amd import target_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(L.LIB_PATH):
        from ghn3_amd import build
        build.build(verbose=False)
    return L.load()


def test_head_structs_match_header_layout(tmp_path):
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "ghn3_hip.h"\nint main(){printf("%zu %zu %zu %zu %d %d\\n",'
                   'sizeof(ghn3_head_desc),sizeof(ghn3_head_params),sizeof(ghn3_head_grads),sizeof(ghn3_xent_desc),'
                   'GHN3_HEAD_MAX_LINEAR,GHN3_XENT_MAX_NETS);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(T._HeadDesc), ctypes.sizeof(T._HeadParams), ctypes.sizeof(T._HeadGrads),
                     ctypes.sizeof(T._XentDesc), T.HEAD_MAX_LINEAR, 32]


def test_abi_version_is_21():
    assert L.ABI_VERSION == 21 and _lib().ghn3_abi_version() == 21


def _desc(B, C, H, W, glob_avg, dims, layout=0):
    return T._head_desc(B, C, H, W, layout, glob_avg, dims)


@pytest.mark.parametrize('bad', [
    dict(B=4097, C=64, H=1, W=1, glob_avg=1, dims=[64, 10]),                     # batch above 4096
    dict(B=8, C=1024, H=6, W=6, glob_avg=0, dims=[1024 * 36, 10]),               # 36864 flattened features
    dict(B=8, C=64, H=4, W=4, glob_avg=1, dims=[64, 5000, 10]),                  # a hidden width above 4096
    dict(B=8, C=64, H=4, W=4, glob_avg=1, dims=[64, 10, 10, 10, 10, 10]),        # five linear layers
])
def test_scratch_size_refuses_what_the_kernels_do_not_take(bad):
    lib = _lib()
    for backward in (0, 1):
        n = lib.ghn3_head_scratch_floats(ctypes.byref(_desc(**bad)), backward)
        assert n == -2, n                         # GHN3_E_LIMIT
        assert lib.ghn3_last_error()


def test_mismatched_feature_size_is_an_argument_error():
    lib = _lib()
    assert lib.ghn3_head_scratch_floats(ctypes.byref(_desc(4, 64, 4, 4, 1, [65, 10])), 0) == -1
    assert lib.ghn3_head_scratch_floats(ctypes.byref(_desc(4, 64, 4, 4, 0, [64, 10])), 0) == -1


@pytest.mark.parametrize('case', [   # B, C, H, W, glob_avg, dims, layout
    (64, 256, 8, 8, 1, [256, 10], 1), (64, 512, 7, 7, 1, [512, 256, 1000], 1), (256, 1024, 4, 4, 1, [1024, 64, 10], 0),
    (4, 32, 4, 4, 0, [512, 64, 10], 0), (4, 32, 4, 4, 0, [512, 64, 10], 1), (3, 48, 1, 1, 1, [48, 512, 64, 10], 1),
    (300, 64, 2, 2, 1, [64, 128, 10], 0)])
def test_scratch_size_accepts_the_tested_shapes(case):
    B, C, H, W, g, dims, layout = case
    lib = _lib()
    d = _desc(B, C, H, W, g, dims, layout)
    fwd, bwd = lib.ghn3_head_scratch_floats(ctypes.byref(d), 0), lib.ghn3_head_scratch_floats(ctypes.byref(d), 1)
    hidden = sum(B * v for v in dims[1:-1])
    direct = not g and layout == 0
    assert fwd >= (0 if direct else B * dims[0]) + hidden          # f (unless x is f) and the hidden activations
    assert bwd >= hidden + (0 if B <= 256 else sum(2 * dims[j + 1] * (dims[j] + 1) for j in range(len(dims) - 1)))


def test_applicable_shape_rule_agrees_with_the_c_limits():
    lib = _lib()
    grid = itertools.product([1, 256, 4096, 4097], [(64, 1, 1), (512, 8, 8), (2048, 4, 4), (32768, 1, 1), (32769, 1, 1)],
                             [0, 1], [[10], [4096, 10], [4097, 1000], [64, 64, 64, 10], [8, 8, 8, 8, 8]])
    n_true = n_false = 0
    for B, (C, H, W), g, tail in grid:
        dims = [C if g else C * H * W] + tail
        ok = T.ClassifierHead.shape_ok(B, C, H, W, bool(g), dims)
        rc = lib.ghn3_head_scratch_floats(ctypes.byref(_desc(B, C, H, W, g, dims)), 0)
        assert ok == (rc >= 0), (B, C, H, W, g, dims, rc)
        n_true, n_false = n_true + ok, n_false + (not ok)
    assert n_true > 20 and n_false > 20


def test_applicable_is_false_on_cpu_and_for_other_heads():
    from ghn3_amd import ops
    x = torch.randn(2, 8, 3, 3)
    head = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Dropout(0.5), torch.nn.Linear(16, 10))
    assert T._head_modules(head) is not None
    assert not T.ClassifierHead.applicable(torch.nn.AdaptiveAvgPool2d(1), head, x)           # (a CPU tensor)
    assert T._head_modules(torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.GELU())) is None
    assert T._head_modules(torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.GELU(), torch.nn.Dropout(), torch.nn.Linear(16, 4))) is None
    assert T._is_global_pool(torch.nn.AdaptiveAvgPool2d(1)) and T._is_global_pool(torch.nn.AdaptiveAvgPool2d((1, 1)))
    assert not T._is_global_pool(torch.nn.AdaptiveAvgPool2d(2))
    import numpy as np
    from ghn3_amd.deepnets1m import sample_net_args
    args = sample_net_args(np.random.RandomState(0))
    args.update(fc_layers=2, fc_dim=16)
    net = ops.NetworkLight(**args)
    lin, drops = T._head_modules(net.classifier)
    assert len(lin) == 2 and len(drops) == 1


def test_meta_cross_entropy_falls_back_on_cpu():
    g = torch.Generator().manual_seed(0)
    logits = [torch.randn(6, 10, generator=g, requires_grad=True) for _ in range(3)]
    targets = torch.tensor([0, 3, 9, 2, 2, 7])
    ce, hits = T.meta_cross_entropy(logits, targets, 0.1)
    want = torch.stack([F.cross_entropy(y, targets, label_smoothing=0.1) for y in logits])
    assert torch.allclose(ce, want)
    lg = torch.stack([y.detach() for y in logits])
    top = lg.topk(5, dim=-1).indices == targets.view(1, -1, 1)
    assert hits.tolist() == [int(top[..., :1].any(-1).sum()), int(top.any(-1).sum())]
    ce.sum().backward()
    assert all(y.grad is not None for y in logits)
