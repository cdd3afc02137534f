"""CPU checks of the multi-tensor SGD step (ghn3_mt_sumsq / ghn3_mt_sgd; ghn3_amd.optim.FusedSGD, sgd_reference_): the C-ABI
boundary, the torch restatement against float64 clip_grad_norm_ + torch.optim.SGD, and the checkpoint layout."""

import ctypes
import os
import re
import subprocess

import pytest
import torch

from ghn3_amd import _lib as L
from ghn3_amd import optim as O
from ghn3_amd import FusedSGD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ghn3_mt_sumsq', 'ghn3_mt_sgd')
C = O.MT_CHUNK
SIZES = [1, 3, 4, 5, 255, 1024, 1025, C - 1, C, C + 1, 2 * C + 7, 0]
SHAPES = [(n,) for n in SIZES] + [(1,)] * 40 + [(64,), (16, 3, 3, 3), (10, 16)]


def test_header_declares_the_entry_points_and_the_library_exports_them():
    text = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    declared = set(re.findall(r'\b(ghn3_[a-z0-9_]+)\s*\(', text))
    assert declared == set(L.EXPORTS)
    assert set(NEW) <= declared
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.ghn3_abi_version() == L.ABI_VERSION == 21


def test_table_structs_match_header_layout(tmp_path):
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "ghn3_hip.h"\nint main(){printf("%zu %zu %zu %d\\n",sizeof(ghn3_mt_tensor),'
                   'sizeof(ghn3_mt_chunk),sizeof(ghn3_mt_sgd_args),GHN3_MT_CHUNK);return 0;}\n')
    exe = tmp_path / 'sz'
    subprocess.check_call(['gcc', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    sizes = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert sizes == [ctypes.sizeof(O._MtTensor), ctypes.sizeof(O._MtChunk), ctypes.sizeof(O._MtSgdArgs), O.MT_CHUNK]
    assert O._MT_TENSOR_DT.itemsize == sizes[0] and O._MT_CHUNK_DT.itemsize == sizes[1]
    assert O.MT_CHUNK % 1024 == 0


def test_the_c_entry_points_refuse_malformed_calls():
    """The host-side checks run before any launch: no GPU needed."""
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) // 16 * 16 + 16
    args = O._MtSgdArgs(0.1, 0.0, 0.0, 0.0, 1.0, 1)
    assert lib.ghn3_mt_sgd(p, p, p, 1, None, ctypes.byref(args), None) == -1           # nesterov without momentum
    assert b'nesterov' in lib.ghn3_last_error()
    args.nesterov = 0
    assert lib.ghn3_mt_sgd(None, p, p, 1, None, ctypes.byref(args), None) == -1        # null table
    assert lib.ghn3_mt_sgd(p, p + 4, p, 1, None, ctypes.byref(args), None) == -1       # misaligned table
    assert lib.ghn3_mt_sgd(p, p, p, 1, None, None, None) == -1
    assert lib.ghn3_mt_sgd(p, p, p, -1, None, ctypes.byref(args), None) == -1
    assert lib.ghn3_mt_sgd(p, p, p, 0, None, ctypes.byref(args), None) == 0            # nothing to do, nothing launched
    assert lib.ghn3_mt_sumsq(p, p, p, 1, p, None, None) == -1
    assert lib.ghn3_mt_sumsq(p, p, p, 1, None, p, None) == -1
    assert lib.ghn3_mt_sumsq(p, None, p, 1, p, p, None) == -1


def _tensors(seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=torch.float32).to(dtype) for s in SHAPES]


@pytest.mark.parametrize('momentum,nesterov', [(0.9, False), (0.9, True), (0.0, False)])
@pytest.mark.parametrize('max_norm', [5.0, 1e9, 0.0])
def test_reference_equals_float64_torch(momentum, nesterov, max_norm):
    """sgd_reference_ in float64 against float64 clip_grad_norm_ + torch.optim.SGD, 4 steps: 1e-12 relative.  The gradients
    are 3 randn (norm about 600): max_norm 5 clips, 1e9 does not, 0 switches clipping off."""
    f64 = torch.float64
    ps = _tensors(1, f64)
    qs = [p.clone().requires_grad_() for p in ps]
    bufs = [torch.zeros_like(p) for p in ps]
    opt = torch.optim.SGD(qs, lr=0.05, momentum=momentum, weight_decay=1e-4, nesterov=nesterov)
    for step in range(4):
        gs = [3 * g for g in _tensors(10 + step, f64)]
        for q, g in zip(qs, gs):
            q.grad = g.clone()
        ref_norm = torch.nn.utils.clip_grad_norm_(qs, max_norm if max_norm > 0 else float('inf'))
        opt.step()
        norm = O.sgd_reference_(ps, gs, bufs, 0.05, momentum, 1e-4, nesterov, max_norm)
        assert abs(float(norm) - float(ref_norm)) <= 1e-12 * float(ref_norm)
        if max_norm == 5.0:
            assert float(norm) > 100 * max_norm                          # (the clip is active)
    a, b = torch.cat([p.reshape(-1) for p in ps]), torch.cat([q.detach().reshape(-1) for q in qs])
    assert float((a - b).norm() / b.norm()) <= 1e-12
    if momentum:
        m = torch.cat([x.reshape(-1) for x in bufs])
        mr = torch.cat([opt.state[q]['momentum_buffer'].reshape(-1) for q in qs])
        assert float((m - mr).norm() / mr.norm()) <= 1e-12


def test_reference_with_loss_scale_and_non_finite_norm():
    f64 = torch.float64
    ps, qs = _tensors(2, f64), _tensors(2, f64)
    gs = [3 * g for g in _tensors(3, f64)]
    b1, b2 = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    n1 = O.sgd_reference_(ps, gs, b1, 0.05, 0.9, 1e-4, False, 5.0)
    n2 = O.sgd_reference_(qs, [g * 1024 for g in gs], b2, 0.05, 0.9, 1e-4, False, 5.0, inv_scale=1.0 / 1024)
    assert abs(float(n1) - float(n2)) <= 1e-12 * float(n1)
    for p, q in zip(ps, qs):
        assert torch.allclose(p, q, rtol=1e-12, atol=0)
    before = [p.clone() for p in ps]
    gs[5][0] = float('inf')
    assert not torch.isfinite(O.sgd_reference_(ps, gs, b1, 0.05, 0.9, 1e-4, False, 5.0))
    assert all(torch.equal(p, q) for p, q in zip(ps, before))


def _model_params(seed):
    return [p.requires_grad_() for p in _tensors(seed, torch.float32)[-4:]] + [torch.zeros(3, requires_grad=True)]


def test_fused_sgd_on_cpu_tensors_state_dict_round_trip():
    ps, qs = _model_params(4), _model_params(4)
    fused = FusedSGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True, max_grad_norm=5.0)
    stock = torch.optim.SGD(qs, lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)

    def grads(step):
        for k, (p, q) in enumerate(zip(ps[:-1], qs[:-1])):                # (the last parameter never has a gradient)
            g = 3 * torch.randn(p.shape, generator=torch.Generator().manual_seed(100 * step + k))
            p.grad, q.grad = g.clone(), g.clone()

    def both(step):
        grads(step)
        norm = fused.step()
        ref = torch.nn.utils.clip_grad_norm_(qs, 5.0)
        stock.step()
        assert torch.allclose(norm, ref, rtol=1e-6)
        for p, q in zip(ps, qs):
            assert torch.allclose(p, q, rtol=1e-6, atol=1e-7)

    both(0)
    both(1)
    sd, ref_sd = fused.state_dict(), stock.state_dict()
    assert set(sd['param_groups'][0]) == set(ref_sd['param_groups'][0]) == {
        'dampening', 'differentiable', 'foreach', 'fused', 'lr', 'maximize', 'momentum', 'nesterov', 'params', 'weight_decay'}
    assert sd['param_groups'][0] == ref_sd['param_groups'][0]
    assert set(sd['state']) == set(ref_sd['state']) == {0, 1, 2, 3}       # no entry for the parameter without a gradient
    for k in sd['state']:
        assert set(sd['state'][k]) == {'momentum_buffer'}
        assert sd['state'][k]['momentum_buffer'].shape == ps[k].shape
        assert sd['state'][k]['momentum_buffer'].data_ptr() == fused._buf(k).data_ptr()     # a view, not a copy
    # swap the states: each optimizer goes on from the other's checkpoint
    keep = {k: {'momentum_buffer': v['momentum_buffer'].clone()} for k, v in sd['state'].items()}
    fused.load_state_dict(ref_sd)
    stock.load_state_dict({'state': keep, 'param_groups': sd['param_groups']})
    both(2)
    both(3)
    fresh = FusedSGD(ps, lr=0.01, momentum=0.9)
    fresh.load_state_dict(fused.state_dict())
    assert fresh.lr == 0.05 and fresh.weight_decay == 1e-4 and fresh.nesterov
    assert torch.equal(fresh.momentum_buffer, fused.momentum_buffer)
    assert set(fresh.state_dict()['state']) == {0, 1, 2, 3}


def test_fused_sgd_without_momentum_keeps_no_state():
    ps = _model_params(5)
    opt = FusedSGD(ps, lr=0.1)
    ps[0].grad = torch.ones_like(ps[0])
    before = ps[0].detach().clone()
    assert opt.step() is not None
    assert torch.equal(ps[0].detach(), before - 0.1)
    assert opt.momentum_buffer is None and opt.state_dict()['state'] == {}
    assert opt.state_dict()['state'] == torch.optim.SGD(ps, lr=0.1).state_dict()['state']


def test_fused_sgd_refuses_what_it_does_not_implement():
    ps = _model_params(6)
    with pytest.raises(ValueError):
        FusedSGD(ps, lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError):
        FusedSGD(ps, lr=0.1, nesterov=True)
    with pytest.raises(ValueError):
        FusedSGD([], lr=0.1)
    with pytest.raises(ValueError):
        FusedSGD([torch.zeros(4, dtype=torch.float64, requires_grad=True)], lr=0.1)
    opt = FusedSGD(ps, lr=0.1, momentum=0.9)
    sd = opt.state_dict()
    sd['param_groups'][0]['dampening'] = 0.1
    with pytest.raises(ValueError):
        opt.load_state_dict(sd)
