"""CPU checks around the stand-alone BatchNorm [+ ReLU] (ghn3_bn_act_*) and nativize(windows='all') (no GPU):

 * the C-ABI boundary: header == EXPORTS, ABI 21, the descriptor's layout, every refusal of ghn3_bn_act_scratch_floats mirrored
   by target_ops.bn_act_refusal on meta tensors;
 * the cases of tests/bnact_cases.py are well conditioned (the 1 % cap of the zeroed upstream gradient, the variance floor) and
   the stock fp32 layers meet, against fp64, the tolerances tests/test_gpu_target_bnact.py asks of the kernels;
 * nativize(net) is today's report and nativize(net, windows='all') the expected one on three hand-written networks, and on the
   CPU -- where every window re-runs the call it replaced -- both are the original bit for bit, in train and eval mode;
 * the refused constructions of tests/resblock_cases.py under windows='all';
 * Trainer(native_layers='all') on the CPU equals native_layers=False.
"""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn

import bnact_cases as B
import resblock_cases as R
import target_edge_cases as E
from util_parity import slice_errors

import ghn3_amd
from ghn3_amd import _lib as L
from ghn3_amd import native_net, target_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ghn3_bn_act_scratch_floats', 'ghn3_bn_act_fwd', 'ghn3_bn_act_bwd', 'ghn3_bn_act_frozen_fwd', 'ghn3_bn_act_frozen_bwd')
OUT_TOL, GRAD_TOL = 2e-4, 3e-4
CASES = B.all_cases()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_symbols_are_the_exports_and_the_library_has_the_new_ones():
    text = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    declared = set(re.findall(r'\b(ghn3_[a-z0-9_]+)\s*\(', text))
    assert declared == set(L.EXPORTS) and len(L.EXPORTS) == len(set(L.EXPORTS))
    assert set(NEW) <= declared
    assert L.ABI_VERSION == 21 and re.search(r'#define\s+GHN3_ABI_VERSION\s+21\b', text)
    lib = L.load()
    assert lib.ghn3_abi_version() == 21
    for name in NEW:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    from ghn3_amd import build
    assert 'tnet_bnact.hip' in build.SOURCES
    m = re.search(r'typedef struct ghn3_bnact_desc \{ int32_t P, C, relu; float eps; \} ghn3_bnact_desc;', text)
    assert m and ctypes.sizeof(T._BnActDesc) == 16 and [f[0] for f in T._BnActDesc._fields_] == ['P', 'C', 'relu', 'eps']


def _desc(shape, relu=1):
    N, C, H, W = shape
    return T._BnActDesc(N * H * W, C, relu, 1e-5)


@pytest.mark.parametrize('name', sorted(B.LIMITS))
def test_every_refusal_of_the_size_function_is_mirrored_by_applicable(name):
    shape, frozen, rule = B.LIMITS[name]
    lib = L.load()
    for backward in (0, 1):
        assert lib.ghn3_bn_act_scratch_floats(ctypes.byref(_desc(shape)), backward | (2 if frozen else 0)) == -2, name   # GHN3_E_LIMIT
    assert lib.ghn3_last_error()
    x = torch.empty(shape, device='meta')
    p = torch.empty(shape[1], device='meta')
    assert T.bn_act_refusal(x, p, p, frozen, p, p) == rule
    xc = torch.empty(1, dtype=torch.float32).expand(shape)                      # a CPU tensor of that shape (one element of storage)
    pc = torch.empty(shape[1])
    assert T.bn_act_refusal(xc, pc, pc, frozen, pc, pc) == rule
    assert not T.BnAct.applicable(xc, pc, pc) and not T.BnActEval.applicable(xc, pc, pc, pc, pc)


@pytest.mark.parametrize('name', sorted(B.ACCEPTED))
def test_what_lies_just_inside_the_limits_is_taken_by_both_sides(name):
    shape, frozen = B.ACCEPTED[name]
    lib = L.load()
    mode = 2 if frozen else 0
    n_fwd, n_bwd = [lib.ghn3_bn_act_scratch_floats(ctypes.byref(_desc(shape)), mode | b) for b in (0, 1)]
    # [chunk][2][C] partials, rounded up to 64 floats; the frozen forward is one launch and takes none
    assert n_bwd >= 2 * shape[1] and n_bwd % 64 == 0 and (n_fwd == 0 if frozen else n_fwd == n_bwd), (n_fwd, n_bwd)
    x = torch.empty(shape, device='meta')
    p = torch.empty(shape[1], device='meta')
    assert T.bn_act_refusal(x, p, p, frozen, p, p) == 'device'                   # (every shape rule passed: the device's comes next)


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf) // 16 * 16 + 16
    d = _desc((2, 8, 2, 2))
    assert lib.ghn3_bn_act_fwd(ctypes.byref(d), p + 4, p, p, p, p, p, None) == -1           # GHN3_E_ARG: x not on 16 bytes
    assert b'16 bytes' in lib.ghn3_last_error()
    assert lib.ghn3_bn_act_fwd(ctypes.byref(d), p, p, p, None, p, p, None) == -1            # a null pointer
    assert lib.ghn3_bn_act_bwd(ctypes.byref(_desc((1, 8, 1, 1))), *([p] * 9), None) == -2   # P == 1 with batch statistics
    assert lib.ghn3_bn_act_frozen_bwd(ctypes.byref(_desc((2, 6, 1, 1))), *([p] * 10), None) == -2
    assert lib.ghn3_bn_act_frozen_fwd(ctypes.byref(_desc((2, 8, 1, 1), relu=2)), *([p] * 6), None) == -1
    assert lib.ghn3_bn_act_scratch_floats(ctypes.byref(d), 4) == -1


def test_runner_and_nodes_on_cpu_tensors_and_the_switch(monkeypatch):
    bn = nn.BatchNorm2d(8)
    x = torch.randn(2, 8, 5, 5)
    for relu in (True, False):
        assert T.run_bn_act(bn, x, relu) is None                                  # (a CPU tensor: the caller keeps its stock layer)
        assert T.run_bn_act(bn.eval(), x, relu) is None
        bn.train()
    assert T.bn_act_refusal(x, bn.weight, bn.bias) == 'device'
    assert not T.BnAct.applicable(x, bn.weight, bn.bias)
    assert not T.BnActEval.applicable(x, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    assert T.bn_act_refusal(x.double(), bn.weight, bn.bias) == 'type'
    assert T.bn_act_refusal(x, bn.weight[:4], bn.bias) == 'params'
    assert int(bn.num_batches_tracked) == 0                                        # (a refusal moves no statistics)
    with pytest.raises(L.Ghn3Error):
        T.bn_act(x, bn.weight, bn.bias)                                            # no CPU implementation, as for conv_bn
    assert T.bnact_enabled()
    monkeypatch.setenv('GHN3_NATIVE_BNACT', '0')
    assert not T.bnact_enabled()
    xm, pm = torch.empty(2, 8, 5, 5, device='meta'), torch.empty(8, device='meta')
    assert T.bn_act_refusal(xm, pm, pm) == 'device'                               # (the device rule is asked before the switch)
    assert T.run_bn_act(bn, x, True) is None


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_cases_are_well_conditioned_and_stock_fp32_meets_the_tolerances(case):
    label, name, relu, frozen = case
    c = B.case(name, relu, frozen)
    N, H, W, C = B.SHAPES[name]
    assert c['x'].shape == (N, C, H, W) and float(c['gamma'].abs().min()) >= 0.5
    assert c['share'] <= B.MASK_SHARE, c['share']                                  # the 1 % cap
    if relu:
        assert bool((c['up'][c['y'].abs() < B.MASK_BAND] == 0).all())
    keep = torch.ones(C, dtype=torch.bool)
    if name == 'special':
        keep[B.CONST_CH] = False
        sd = c['var'].sqrt()
        assert float(c['mean'][B.FAR_CH].abs() / sd[B.FAR_CH]) > 90                # mean = 100 sigma
        assert float(c['var'][B.CONST_CH]) == 0.0 and float(c['beta'][B.CONST_CH]) == pytest.approx(0.3)
        if relu:
            assert float(c['out'][:, B.MASKED_CH].abs().max()) == 0.0              # fully masked in the reference,
            assert bool((c['y'][:, B.OPEN_CH] > 0).all())                          # ... and never masked
    # (the two-row case lives at variances of a few eps on purpose: bnact_cases.inputs)
    floor = 2 * B.EPS if name == 'min' else E.VAR_FLOOR
    assert float(c['var'][keep].min()) >= floor, float(c['var'][keep].min())
    # stock fp32 against fp64
    leaves = [c[k].clone().requires_grad_(True) for k in ('x', 'gamma', 'beta')]
    out = T.bn_act_reference(*leaves, relu, B.EPS, *(c['running'] if frozen else (None, None)))
    (out * c['up']).sum().backward()
    worst = {}
    for key, got, axes, tol in (('out', out.detach(), E.ACT_AXES, OUT_TOL), ('dx', leaves[0].grad, E.ACT_AXES, GRAD_TOL),
                                ('dgamma', leaves[1].grad, E.VEC_AXES, GRAD_TOL), ('dbeta', leaves[2].grad, E.VEC_AXES, GRAD_TOL)):
        v, where = slice_errors(got, c[key], axes)
        worst[key] = v
        assert v <= tol, (label, key, v, where)
    print(label, 'zeroed share %.4f %%' % (100 * c['share']), ', '.join('%s %.1e' % kv for kv in worst.items()))


def test_the_case_list_has_what_the_kernels_need():
    text = open(os.path.join(ROOT, 'ghn3_amd', 'csrc', 'tnet_bnact.hip')).read()
    tile = int(re.search(r'constexpr int BA_TILE = (\d+);', text).group(1))
    cbw = int(re.search(r'constexpr int BA_CBW = (\d+);', text).group(1))
    gy = int(re.search(r'constexpr int BA_GRID_Y = (\d+);', text).group(1))
    rows = {n: B.rows_of(n) for n in B.SHAPES}
    assert rows['min'] == 2 and B.SHAPES['min'][3] == 4
    assert {rows['p63'], rows['p64'], rows['p65']} == {tile - 1, tile, tile + 1}
    assert rows['chunks'] == 4097 and rows['chunks'] % tile == 1 and rows['chunks'] // tile >= 64    # many chunks, a one-row tail
    assert cbw < B.SHAPES['blocks'][3] <= cbw * gy and B.SHAPES['blocks'][3] % cbw == 4               # several blocks, a one-quad tail
    assert B.SHAPES['wide'][3] > cbw * gy                                                             # the loop over channel blocks
    assert {(relu, frozen) for _, n, relu, frozen in CASES if n == 'special'} == {(a, b) for a in (True, False) for b in (True, False)}


# ---- nativize -----------------------------------------------------------------------------------------------------------------------
def _step(model, x, y, train=True):
    model.train(train)
    out = model(x)
    if train:
        nn.functional.cross_entropy(out, y).backward()
    return out.detach()


@pytest.mark.parametrize('cls', B.NETS + [R.BasicNet], ids=lambda c: c.__name__)
def test_nativize_reports_and_on_the_cpu_is_the_original_bit_for_bit(cls):
    plain = ghn3_amd.nativize(B.make_net(cls), strict=True).report()
    assert plain['windows'] == cls.windows and list(plain['windows']) == list(native_net.WINDOW_KINDS), str(plain)   # today's report
    assert len(plain['stock_convs']) == getattr(cls, 'stock_default', 0)
    assert native_net.WINDOW_KINDS == ('conv_bn_relu', 'conv_bn_add_relu', 'conv_bn', 'pool', 'head')
    net = B.make_net(cls)
    ref = copy.deepcopy(net)
    keys = list(net.state_dict())
    nat = ghn3_amd.nativize(net, strict=True, windows='all')
    rep = nat.report()
    assert rep['windows'] == B.windows_all(cls), str(rep)
    assert rep['stock_convs'] == {}, str(rep)
    assert all(k in str(rep) for k in native_net.EXTRA_KINDS)
    assert sorted(nat.state_dict()) == sorted(keys) and keys == list(net.state_dict())
    mine = dict(net.named_parameters())
    assert all(p is mine[k] for k, p in nat.named_parameters()) and len(list(nat.parameters())) == len(mine)
    mine = dict(net.named_buffers())
    assert all(b is mine[k] for k, b in nat.named_buffers()) and len(list(nat.buffers())) == len(mine)
    assert not any(isinstance(m, native_net._Window) for m in net.modules())
    x, y = B.net_batch(cls)
    out, out_ref = _step(nat, x, y), _step(ref, x, y)
    assert torch.equal(out, out_ref)
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
    for (k, b), c in zip(net.named_buffers(), ref.buffers()):               # running statistics and num_batches_tracked
        assert torch.equal(b, c), k
    assert any('num_batches_tracked' in k and int(b) == 1 for k, b in net.named_buffers())
    with torch.no_grad():
        assert torch.equal(_step(nat, x, y, train=False), _step(ref, x, y, train=False))
    for (k, b), c in zip(net.named_buffers(), ref.buffers()):               # eval mode moves nothing
        assert torch.equal(b, c), k
    assert not nat.training and not any(m.training for m in net.modules() if isinstance(m, nn.BatchNorm2d))
    with pytest.raises(ValueError):
        ghn3_amd.nativize(net, windows='dense')


@pytest.mark.parametrize('kind', sorted(R.REFUSALS))
def test_refused_constructions_under_all_windows(kind):
    """The convolutions the dense kernels refuse (biased, grouped, reflect-padded, 9 x 9) stay stock with the same reason under
    windows='all'; the BatchNorm behind them becomes a window of its own.  'two_users' and 'relu6' hold a convolution the
    kernels take, refused today only for what follows its norm layer: it becomes a 'conv' window and leaves the list, as the
    module text says.  Either way the results are the original's bit for bit."""
    torch.manual_seed(3)
    net = R.Refused(kind)
    ref = copy.deepcopy(net)
    today = ghn3_amd.nativize(net, strict=True).report()
    assert sum(today['windows'].values()) == 0 and R.REFUSALS[kind] in today['stock_convs']['conv']
    nat = ghn3_amd.nativize(net, strict=True, windows='all')
    rep = nat.report()
    w = rep['windows']
    assert all(w[k] == 0 for k in native_net.WINDOW_KINDS), str(rep)
    if native_net.conv_refusal(net.conv) is not None:
        assert kind in ('bias', 'groups', 'reflect', 'kernel')
        assert rep['stock_convs'] == today['stock_convs'] and R.REFUSALS[kind] in str(rep)
        assert (w['conv'], w['bn_relu'], w['bn']) == (0, 1, 0)
    else:
        assert kind in ('two_users', 'relu6') and rep['stock_convs'] == {}
        assert (w['conv'], w['bn_relu'], w['bn'], w['add']) == (1, 0, 1, 1 if kind == 'two_users' else 0)
    x = torch.randn(3, 4, 6, 6, generator=torch.Generator().manual_seed(4))
    for train in (True, False):
        nat.train(train)
        ref.train(train)
        assert torch.equal(nat(x), ref(x))
    assert torch.equal(net.bn.running_mean, ref.bn.running_mean) and int(net.bn.num_batches_tracked) == 1


def test_an_in_place_add_whose_operand_has_other_readers_stays_the_call_it_is():
    class Net(nn.Module):
        def forward(self, x):
            y = x * 2
            z = y.relu()
            y.add_(x)                                    # (the multiplication's result has other readers, which see the sum)
            return y + z
    nat = ghn3_amd.nativize(Net(), windows='all')
    assert nat.report()['windows']['add'] == 1
    x = torch.randn(2, 4, 3, 3)
    assert torch.equal(nat(x), Net()(x))


def test_trainer_native_layers_all_on_the_cpu_equals_the_default():
    from ghn3_amd import Trainer
    results = {}
    for native in (False, True, 'all'):
        net = B.make_net(B.PreActResNet)
        tr = Trainer(net, opt='sgd', opt_args={'lr': 0.05, 'momentum': 0.9}, scheduler='cosine', n_batches=4, device='cpu',
                     epochs=2, log_interval=1, native_layers=native)
        assert tr._model is net and tr._native_layers == native                   # (the value, not its truth)
        for k in range(2):
            tr.update(*B.net_batch(B.PreActResNet, seed=20 + k))
        results[native] = (tr.metrics.avg()['loss'], [p.detach().clone() for p in net.parameters()],
                           [b.detach().clone() for b in net.buffers()])
        assert (tr._forward_model is not None) == bool(native)
        if native:
            w = tr._forward_model.report()['windows']
            assert ('bn_relu' in w) == (native == 'all') and (native != 'all' or w == B.windows_all(B.PreActResNet))
    for native in (True, 'all'):
        assert results[native][0] == results[False][0]
        assert all(torch.equal(a, b) for a, b in zip(results[native][1], results[False][1]))
        assert all(torch.equal(a, b) for a, b in zip(results[native][2], results[False][2]))
    with pytest.raises(ValueError):
        Trainer(B.make_net(B.PreActResNet), opt='sgd', opt_args={'lr': 0.1}, scheduler='cosine', n_batches=4, device='cpu',
                native_layers='dense')
