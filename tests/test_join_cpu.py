"""CPU checks of the target-network joins (ghn3_join_fwd / _bwd, ghn3_posenc_bwd; target_ops.pair_sum / cell_concat / pos_enc):
the C-ABI boundary, what `join_refusal` refuses, and that nothing moves on CPU tensors."""

import ctypes
import os
import re
import subprocess

import torch

from ghn3_amd import _lib as L
from ghn3_amd import ops
from ghn3_amd import target_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ghn3_join_fwd', 'ghn3_join_bwd', 'ghn3_posenc_bwd')


def test_header_symbols_are_the_exports_and_the_library_has_the_new_ones():
    text = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    declared = set(re.findall(r'\b(ghn3_[a-z0-9_]+)\s*\(', text))
    assert declared == set(L.EXPORTS)
    assert set(NEW) <= declared
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name), name


def test_join_structs_match_header_layout(tmp_path):
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "ghn3_hip.h"\nint main(){printf("%zu %zu %zu %d\\n",sizeof(ghn3_join_src),'
                   'sizeof(ghn3_join_slice),sizeof(ghn3_join_desc),GHN3_JOIN_MAX_SLICES);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(T._JoinSrc), ctypes.sizeof(T._JoinSlice), ctypes.sizeof(T._JoinDesc), T.JOIN_MAX_SLICES]


def test_the_c_entry_points_refuse_what_join_refusal_refuses():
    """The limits of the header straight through the ABI (the checks run on the host before any launch: no GPU needed)."""
    lib = L.load()
    buf = (ctypes.c_float * 64)()                       # (an address to pass the null checks; nothing is launched)
    p = ctypes.addressof(buf) // 16 * 16 + 16

    def desc(C, Hs=4, N=2, step=1):
        d = T._JoinDesc(N, -(-Hs // step), -(-Hs // step), C, 1, 1)
        d.s[0].a = T._JoinSrc(p, p, Hs, Hs, step, 1, 0, 0)
        d.s[0].c0, d.s[0].C = 0, C
        return d
    for fn in (lib.ghn3_join_fwd, lib.ghn3_join_bwd):
        assert fn(ctypes.byref(desc(6)), p, None) == -2                            # GHN3_E_LIMIT: C % 4
        assert fn(ctypes.byref(desc(4, Hs=2 ** 15, N=2 ** 7 + 1)), p, None) == -2  # 2^31 elements and more
        d = desc(8)
        d.n_slices = T.JOIN_MAX_SLICES + 1
        assert fn(ctypes.byref(d), p, None) == -2
        d = desc(8)
        d.H = 3                                                                    # (a 4 x 4 source is no 3 x 3 output map)
        assert fn(ctypes.byref(d), p, None) == -1                                  # GHN3_E_ARG
        assert b'map' in lib.ghn3_last_error()
    assert lib.ghn3_posenc_bwd(2, 6, 3, 3, 0, p, p, None) == -2
    assert lib.ghn3_posenc_bwd(2 ** 10, 2 ** 10, 2 ** 6, 2 ** 5, 0, p, p, None) == -2


def test_join_refusal_states_the_limits():
    x = torch.zeros(2, 8, 5, 5)
    ok = torch.zeros(2, 8, 5, 5)
    # (on CPU tensors that satisfy every shape rule the first rule to fail is the device's)
    assert T.join_refusal([(x, ok, 1, 1)]) == 'device'
    assert T.join_refusal([(x.contiguous(memory_format=torch.channels_last), ok, 1, 1)]) == 'device'
    assert T.join_refusal([(torch.zeros(2, 8, 9, 10), ok, 2, 1)]) == 'device'       # 9 x 10 at step 2 is a 5 x 5 map
    # C % 4 != 0
    assert T.join_refusal([(torch.zeros(2, 6, 5, 5), torch.zeros(2, 6, 5, 5), 1, 1)]) == 'channels'
    assert T.join_refusal([(x, None, 1, 1), (torch.zeros(2, 6, 5, 5), None, 1, 1)]) == 'channels'
    assert T.join_refusal([(x, torch.zeros(2, 12, 5, 5), 1, 1)]) == 'channels'
    # non-dense sources: a strided slice, a channel slice, a permuted view
    assert T.join_refusal([(torch.zeros(2, 8, 10, 10)[:, :, ::2, ::2], ok, 1, 1)]) == 'dense'
    assert T.join_refusal([(torch.zeros(2, 16, 5, 5)[:, :8], ok, 1, 1)]) == 'dense'
    assert T.join_refusal([(torch.zeros(2, 5, 8, 5).permute(0, 2, 1, 3), ok, 1, 1)]) == 'dense'
    # mismatched maps and batch sizes
    assert T.join_refusal([(x, torch.zeros(2, 8, 5, 6), 1, 1)]) == 'map'
    assert T.join_refusal([(x, torch.zeros(2, 8, 11, 11), 1, 2)]) == 'map'          # 11 x 11 at step 2 is 6 x 6
    assert T.join_refusal([(x, torch.zeros(3, 8, 5, 5), 1, 1)]) == 'map'
    assert T.join_refusal([(x, None, 1, 1), (torch.zeros(2, 4, 4, 4), None, 1, 1)]) == 'map'
    assert T.join_refusal([(x, torch.zeros(1, 8, 5, 5), 1, 1)]) == 'map'            # (broadcasting is pos_enc's alone)
    assert T.join_refusal([(x, torch.zeros(1, 8, 5, 5), 1, 1)], broadcast_b=True) == 'device'
    # tensors of 2^31 elements or more (meta tensors: no memory behind them)
    big = torch.empty((2, 4, 2 ** 14, 2 ** 14), device='meta')
    assert big.numel() == 2 ** 31
    assert T.join_refusal([(big, None, 1, 1)]) == 'size'
    half = torch.empty((2, 4, 2 ** 14, 2 ** 13), device='meta')
    assert T.join_refusal([(half, None, 1, 1), (half, None, 1, 1)]) == 'size'       # (the output is the tensor too large)
    assert T.join_refusal([(half, None, 1, 1)]) == 'device'
    # types, steps, slice counts
    assert T.join_refusal([(x.half(), ok.half(), 1, 1)]) == 'type'
    assert T.join_refusal([(x, ok, 3, 1)]) == 'type'
    assert T.join_refusal([(x[0], ok[0], 1, 1)]) == 'type'
    assert T.join_refusal([]) == 'slices'
    assert T.join_refusal([(x, None, 1, 1)] * (T.JOIN_MAX_SLICES + 1)) == 'slices'
    assert not T.join_applicable([(x, ok, 1, 1)])


def test_nothing_moves_on_cpu_tensors():
    a, b = torch.randn(2, 8, 5, 5), torch.randn(2, 8, 5, 5)
    assert T.pair_sum(a, b) is None and T.cell_concat([a, b]) is None
    assert T.pos_enc(a, torch.randn(1, 8, 5, 5)) is None
    pe = ops.PosEnc(8, 5)
    x = torch.randn(3, 8, 5, 5)
    assert torch.equal(pe(x), x + pe.weight)
    # a cell without preprocessing layers: state 2 = max_pool(s0) + s1, state 3 = s0 + state 2, output = cat(states 2, 3)
    geno = ops.Genotype(normal=[('max_pool_3x3', 0), ('skip_connect', 1), ('skip_connect', 0), ('skip_connect', 2)],
                        normal_concat=[2, 3], reduce=[('skip_connect', 0), ('skip_connect', 1)], reduce_concat=[2])
    cell = ops.Cell(geno, 8, 8, 8, 8, reduction=False, reduction_prev=False, preproc=False)
    s0, s1 = torch.randn(2, 8, 6, 6), torch.randn(2, 8, 6, 6)
    st2 = torch.nn.functional.max_pool2d(s0, 3, 1, 1) + s1
    assert torch.equal(cell(s0, s1), torch.cat([st2, s0 + st2], dim=1))
