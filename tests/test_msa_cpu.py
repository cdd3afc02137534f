"""CPU checks of the msa op's C ABI (include/ghn3_hip.h ghn3_msa_*): the ctypes mirror of the descriptor has the C layout, and
ghn3_msa_scratch_floats (host only) refuses what the kernels do not take and sizes what they do."""
import ctypes
import os
import subprocess

import pytest

from ghn3_amd import _lib as L
from ghn3_amd import target_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(L.LIB_PATH):
        from ghn3_amd import build
        build.build(verbose=False)
    return L.load()


def test_msa_structs_match_header_layout(tmp_path):
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "ghn3_hip.h"\nint main(){printf("%zu %zu %zu\\n",sizeof(ghn3_msa_desc),'
                   'sizeof(ghn3_msa_params),sizeof(ghn3_msa_grads));return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(T._MsaDesc), ctypes.sizeof(T._MsaPtrs), ctypes.sizeof(T._MsaPtrs)]


def _desc(B, C, H, W, stride=1, heads=8, hidden=None, layout=0):
    return T._MsaDesc(B, H, W, C, heads, C if hidden is None else hidden, stride, (H - 1) // stride + 1, (W - 1) // stride + 1,
                      layout, 1e-5, 0)


@pytest.mark.parametrize('bad', [
    dict(B=2, C=512, H=4, W=4),                 # head dim 64
    dict(B=1, C=64, H=65, W=64),                # 4160 tokens
    dict(B=2, C=60, H=4, W=4),                  # C % heads != 0
    dict(B=2, C=64, H=4, W=4, hidden=2048),     # hidden above 1024
])
def test_scratch_size_refuses_what_the_kernels_do_not_take(bad):
    lib = _lib()
    for backward in (0, 1):
        n = lib.ghn3_msa_scratch_floats(ctypes.byref(_desc(**bad)), backward)
        assert n == -2, n                         # GHN3_E_LIMIT
        assert lib.ghn3_last_error()


@pytest.mark.parametrize('case', [   # B, C, H, W, stride, hidden
    (64, 32, 11, 11, 1, 32), (64, 64, 11, 11, 1, 64), (64, 128, 11, 11, 1, 128), (8, 128, 14, 14, 1, 128),
    (4, 256, 7, 7, 2, 256), (3, 48, 5, 7, 2, 48), (2, 64, 1, 1, 1, 64), (6, 64, 8, 8, 1, 256), (16, 128, 14, 14, 1, 128),
    (16, 256, 14, 14, 1, 1024)])
def test_scratch_size_accepts_the_tested_shapes(case):
    B, C, H, W, s, hidden = case
    lib = _lib()
    d = _desc(B, C, H, W, s, hidden=hidden)
    fwd, bwd = lib.ghn3_msa_scratch_floats(ctypes.byref(d), 0), lib.ghn3_msa_scratch_floats(ctypes.byref(d), 1)
    R, K = B * H * W, B * d.Ho * d.Wo
    assert fwd >= R * 4 * C + K * (C + hidden)          # qkv, attention output, y1, pre-GELU values
    assert bwd >= R * 6 * C + K * (C + 2 * hidden)


def test_mismatched_output_grid_is_an_argument_error():
    lib = _lib()
    d = _desc(2, 64, 8, 8, 2)
    d.Ho = 3
    assert lib.ghn3_msa_scratch_floats(ctypes.byref(d), 0) == -1
