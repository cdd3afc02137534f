"""CPU checks around the "bias" member of the dense-convolution family (ghn3_conv_bias_act_*) and nativize(biased=True) (no GPU):

 * the C-ABI boundary: the header declares the new symbols and the flag, the built library exports them, the size function
   answers in the terms of its neighbours and refuses what they refuse, and the neighbours ignore the new flag;
 * the cases of tests/bias_cases.py are well conditioned (the 1 % cap of the zeroed upstream gradient; the special channels; the
   variance floor in front of the networks' norm layers);
 * nativize(net) and nativize(net, windows='all') without `biased` are today's reports on both networks -- every biased
   convolution stock, with its reason --, with biased=True they are the expected ones and no convolution is stock, and on the CPU
   -- where every window re-runs the layers it replaced -- the module is the original bit for bit, in train and eval mode;
 * the switch, the runner and the op on CPU tensors; Trainer(native_biased=...) on the CPU.
"""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import bias_cases as B

import ghn3_amd
from ghn3_amd import _lib as L, native_net, target_ops as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ghn3_conv_bias_act_scratch_floats', 'ghn3_conv_bias_act_fwd', 'ghn3_conv_bias_act_bwd')
CASES = B.all_cases()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_new_symbols_and_the_library_exports_them():
    text = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    declared = set(re.findall(r'\b(ghn3_[a-z0-9_]+)\s*\(', text))
    assert set(NEW) <= declared and set(NEW) <= set(L.EXPORTS)
    assert re.search(r'#define\s+GHN3_CONV_ACT_OUT\s+4\b', text) and T.CONV_ACT_OUT == 4
    assert L.ABI_VERSION == 21 and re.search(r'#define\s+GHN3_ABI_VERSION\s+21\b', text)      # no version step
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name


def _desc(row, relu_bits):
    N, Ci, Co, H, W, k, st, pad, dil, relu_in, gain = row
    x = torch.empty(N, max(Ci, 4), H, W, device='meta')
    w = torch.empty(Co, max(Ci, 4), *k, device='meta')
    d = T._conv_desc(x, w, st, pad, dil, False, 0.0)
    d.relu = relu_bits
    return d


@pytest.mark.parametrize('row', B.ROWS, ids=['row%d' % i for i in B.ROW_IDS])
def test_the_size_function_and_the_flag(row):
    lib = L.load()
    for bits in (0, 1, T.CONV_ACT_OUT, 1 | T.CONV_ACT_OUT):
        d = _desc(row, bits)
        fwd, bwd = [int(lib.ghn3_conv_bias_act_scratch_floats(ctypes.byref(d), m)) for m in (0, 1)]
        # forward: the weight pack alone (the frozen member's forward); backward: the batch member's backward layout
        assert fwd == int(lib.ghn3_conv_frozen_scratch_floats(ctypes.byref(d), 0)) > 0
        assert bwd == int(lib.ghn3_conv_scratch_floats(ctypes.byref(d), 1)) > 0
        # every other size function answers as without the new bit
        plain = _desc(row, bits & 1)
        for fn in ('ghn3_conv_scratch_floats', 'ghn3_conv_frozen_scratch_floats', 'ghn3_conv_act_scratch_floats'):
            for m in (0, 1):
                assert int(getattr(lib, fn)(ctypes.byref(d), m)) == int(getattr(lib, fn)(ctypes.byref(plain), m)), (fn, m)
    d = _desc(row, T.CONV_NO_NORM | T.CONV_ACT_OUT)
    assert int(lib.ghn3_conv_bias_act_scratch_floats(ctypes.byref(d), 0)) < 0
    assert b'NO_NORM' in lib.ghn3_last_error()
    # and the null-pointer answer of the entry points comes before any launch
    d = _desc(row, T.CONV_ACT_OUT)
    assert lib.ghn3_conv_bias_act_fwd(ctypes.byref(d), None, None, None, None, None, None, None) < 0
    assert lib.ghn3_conv_bias_act_bwd(ctypes.byref(d), None, None, None, None, None, None, None, None, None, None) < 0


def test_the_limits_are_refused_by_the_c_side_and_by_applicable_alike():
    lib = L.load()
    bad = [(2, 6, 8, 4, 4, (3, 3), (1, 1), (1, 1), 1, False, 1.0),                 # C_in not a multiple of 4
           (2, 8, 8200, 4, 4, (1, 1), (1, 1), (0, 0), 1, False, 1.0),              # C_out > 4096
           (2 ** 15, 4, 4, 128, 128, (1, 1), (1, 1), (0, 0), 1, False, 1.0)]       # N H W C = 2^31
    for row in bad:
        d = _desc(row, T.CONV_ACT_OUT)
        assert int(lib.ghn3_conv_bias_act_scratch_floats(ctypes.byref(d), 1)) < 0, row
        assert int(lib.ghn3_conv_scratch_floats(ctypes.byref(d), 1)) < 0, row


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_cases_are_well_conditioned(case):
    name, row, with_res, relu, special = case
    c = B.bias_case(row, with_res, relu, special)
    print('%s: zeroed share %.4f, positive share %.3f' % (name, c['share'], c['positive']))
    assert c['share'] <= B.MASK_SHARE
    if not relu:
        assert c['share'] == 0.0
    assert all(torch.isfinite(c[k]).all() for k in ('out', 'dx', 'dw', 'dbias'))
    assert (c['dres'] is not None) == with_res
    if special:
        # channel 19 fully masked: exact zeros in the reference as well; channel 3 never masked
        assert float(c['out'][:, B.MASKED_CH].abs().max()) == 0.0 and bool((c['y'][:, B.MASKED_CH] < -B.MASK_BAND).all())
        assert float(c['dbias'][B.MASKED_CH]) == 0.0 and float(c['dw'][B.MASKED_CH].abs().max()) == 0.0
        assert bool((c['y'][:, B.OPEN_CH] > B.MASK_BAND).all())
    elif relu:
        assert 0.3 < c['positive'] < 0.8


def test_the_case_list_has_what_the_kernels_need():
    rows = B.ROWS
    assert len(CASES) == 4 * len(rows) + 2
    P = [r[0] * B.R.conv_out_hw(r[3], r[4], r[5], r[6], r[7], r[8])[0] * B.R.conv_out_hw(r[3], r[4], r[5], r[6], r[7], r[8])[1] for r in rows]
    assert any(p < 64 for p in P) and any(p > 64 and p % 64 for p in P)              # a partial tile; a full one and a rest
    assert any(r[2] // 4 > 256 for r in rows)                                        # the looping arm of the column-sum pass
    assert any(256 % (r[2] // 4) for r in rows if r[2] // 4 <= 256)                  # idle threads in its other arm
    assert any(r[1] == 3 for r in rows) and any(r[9] for r in rows) and any(r[6] == (2, 2) for r in rows)


@pytest.mark.parametrize('cls', B.NETS, ids=lambda c: c.__name__)
def test_the_networks_keep_the_variance_floor_in_front_of_their_norm_layers(cls):
    """What conv_inputs' rows keep (VAR_FLOOR), asked of the whole networks: no channel in front of a BatchNorm has a batch
    variance so small that 1 / sqrt(var) amplifies the rounding of either fp32 path into the comparison."""
    net = B.make_net(cls)
    net.train()
    seen = B.bn_input_variances(net, B.net_batch(cls)[0])
    print(cls.__name__, seen)
    assert len(seen) == sum(isinstance(m, nn.BatchNorm2d) for m in net.modules())
    assert all(v >= B.VAR_FLOOR for v in seen.values()), seen


# ---- nativize ---------------------------------------------------------------------------------------------------------------------------
def _step(model, x, y, train=True):
    model.train(train)
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(11)                                                            # (the Dropout draws)
    out = model(x)
    if train:
        F.cross_entropy(out, y).backward()
    return out.detach()


@pytest.mark.parametrize('windows', ['resnet', 'all'])
@pytest.mark.parametrize('cls', B.NETS, ids=lambda c: c.__name__)
def test_without_biased_the_report_is_todays(cls, windows):
    net = B.make_net(cls)
    rep = ghn3_amd.nativize(net, strict=True, windows=windows).report()
    assert rep['windows'] == B.expected_windows(cls, windows, False), str(rep)
    convs = [k for k, m in net.named_modules() if isinstance(m, nn.Conv2d)]
    assert sorted(rep['stock_convs']) == sorted(convs) and all('biased' in v for v in rep['stock_convs'].values())
    assert not set(native_net.BIAS_KINDS) & set(rep['windows'])
    assert native_net.conv_refusal(net.get_submodule(convs[0])) == 'biased convolution'
    assert native_net.conv_refusal(net.get_submodule(convs[0]), biased=True) is None


@pytest.mark.parametrize('windows', ['resnet', 'all'])
@pytest.mark.parametrize('cls', B.NETS, ids=lambda c: c.__name__)
def test_nativize_biased_on_the_cpu_is_the_original_bit_for_bit(cls, windows):
    net = B.make_net(cls)
    ref = copy.deepcopy(net)
    keys = list(net.state_dict())
    nat = ghn3_amd.nativize(net, strict=True, windows=windows, biased=True)
    rep = nat.report()
    assert rep['windows'] == B.expected_windows(cls, windows, True) and rep['stock_convs'] == {}, str(rep)
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
    for (k, b), c in zip(net.named_buffers(), ref.buffers()):
        assert torch.equal(b, c), k
    with torch.no_grad():
        assert torch.equal(_step(nat, x, y, train=False), _step(ref, x, y, train=False))
    # eval() on the nativized module reaches the shared layers (the leaves: the original's containers are not part of the graph)
    assert not nat.training and not any(m.training for m in net.modules() if not list(m.children()))


def test_windows_dense_still_raises_and_the_skip_add_window():
    with pytest.raises(ValueError):
        ghn3_amd.nativize(B.make_net(B.VggNet), windows='dense', biased=True)

    class Res(nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c = nn.Conv2d(4, 8, 3, 1, 1), nn.Conv2d(8, 8, 3, 1, 1), nn.Conv2d(4, 8, 1)

        def forward(self, x):
            y = F.relu(self.a(x))
            return F.relu(self.b(y) + self.c(x)) + y

    torch.manual_seed(2)
    net = Res()
    ref = copy.deepcopy(net)
    nat = ghn3_amd.nativize(net, strict=True, biased=True)
    rep = nat.report()
    # a (two users of its ReLU, one of the convolution) with its ReLU; b takes the add and the ReLU, c -- the other operand -- stands alone
    assert {k: v for k, v in rep['windows'].items() if v} == {'conv_bias_relu': 1, 'conv_bias_add_relu': 1, 'conv_bias': 1}, str(rep)
    assert rep['stock_convs'] == {}
    x = torch.randn(2, 4, 5, 5, generator=torch.Generator().manual_seed(4))
    assert torch.equal(nat(x), ref(x))
    # a biased convolution the kernels refuse for another reason keeps that reason
    net = nn.Sequential(nn.Conv2d(4, 8, 3, 1, 1, groups=2), nn.ReLU())
    rep = ghn3_amd.nativize(net, strict=True, biased=True).report()
    assert list(rep['stock_convs'].values()) == ['grouped convolution (groups=2)'] and rep['windows']['conv_bias_relu'] == 0


def test_the_same_size_pool_runs_the_stock_layer_on_another_size():
    pool = nn.AdaptiveAvgPool2d((2, 2))
    win = native_net.NativeSameSizePool(pool, (2, 2))
    x = torch.randn(2, 4, 2, 2)
    assert win(x) is x and torch.equal(pool(x), x)                                   # the mean of one element: exact
    x = torch.randn(2, 4, 6, 4)
    assert torch.equal(win(x), pool(x))


# ---- the op, its switch and the runner on CPU tensors -----------------------------------------------------------------------------------
def test_switch_and_runner_on_cpu_tensors(monkeypatch):
    conv = nn.Conv2d(4, 8, 3, 1, 1)
    x = torch.randn(2, 4, 5, 5)
    assert T.run_conv_bias_act(conv, x, True) is None                      # (a CPU tensor: the caller keeps its stock layers)
    assert not T.ConvBiasAct.applicable(x, conv.weight, conv.bias)
    assert T.bias_enabled()
    monkeypatch.setenv('GHN3_NATIVE_BIAS', '0')
    assert not T.bias_enabled() and T.run_conv_bias_act(conv, x, True) is None
    with pytest.raises(ghn3_amd._lib.Ghn3Error):
        T.conv_bias_act(x, conv.weight, conv.bias)                         # no CPU implementation, as for conv_bn_act
    ref = T.conv_bias_act_reference(x, conv.weight, conv.bias, x.new_ones(2, 8, 5, 5), 1, 1, 1, True, True)
    assert torch.equal(ref, F.relu(conv(F.relu(x)) + 1))


def test_the_switch_alone_turns_an_applicable_call_down(monkeypatch):
    """On meta tensors standing in for device tensors every other condition of `applicable` holds: the switch decides."""
    monkeypatch.setattr(T, '_f32_cuda', lambda *ts: all(torch.is_tensor(t) and t.dtype == torch.float32 for t in ts))
    x, w, b = torch.empty(2, 4, 5, 5, device='meta'), torch.empty(8, 4, 3, 3, device='meta'), torch.empty(8, device='meta')
    assert T.ConvBiasAct.applicable(x, w, b, None, 1, 1, 1)
    assert not T.ConvBiasAct.applicable(x, w, b, torch.empty(2, 8, 4, 4, device='meta'), 1, 1, 1)      # not the output's shape
    assert not T.ConvBiasAct.applicable(x, w, b[:4], None, 1, 1, 1)
    assert not T.ConvBiasAct.applicable(x, w, b, None, 1, 0, 3)                                          # no output pixel left
    big = torch.empty(2 ** 15, 4, 128, 64, device='meta')                                                # N H W C_out = 2^31
    assert not T.ConvBiasAct.applicable(big, torch.empty(8, 4, 1, 1, device='meta'), b, None, 1, 0, 1)
    for name in ('GHN3_NATIVE_BIAS', 'GHN3_NATIVE_CONV', 'GHN3_NATIVE_OPS'):
        monkeypatch.setenv(name, '0')
        assert not T.ConvBiasAct.applicable(x, w, b, None, 1, 1, 1), name
        monkeypatch.delenv(name)
    assert T.ConvBiasAct.applicable(x, w, b, None, 1, 1, 1)


def test_trainer_native_biased_on_the_cpu():
    from ghn3_amd import Trainer
    args = dict(opt='sgd', opt_args={'lr': 0.05, 'momentum': 0.9}, scheduler='cosine', n_batches=4, device='cpu', epochs=2, log_interval=1)
    losses = {}
    for native in (False, True):
        net = B.make_net(B.VggNet)
        tr = Trainer(net, native_layers=native, native_biased=native, **args)
        assert tr._model is net
        for k in range(2):
            torch.manual_seed(50 + k)                                                # (the Dropout draws)
            tr.update(*B.net_batch(B.VggNet, seed=20 + k))
        losses[native] = (tr.metrics.avg()['loss'], [p.detach().clone() for p in net.parameters()])
        assert (tr._forward_model is not None) == native
        if native:
            assert tr._forward_model.report()['windows']['conv_bias_relu'] == 3 and tr._forward_model.report()['stock_convs'] == {}
    assert losses[True][0] == losses[False][0]
    assert all(torch.equal(a, b) for a, b in zip(losses[True][1], losses[False][1]))
    with pytest.raises(ValueError):
        Trainer(B.make_net(B.VggNet), native_biased=True, **args)
    with pytest.raises(ValueError):
        Trainer(B.make_net(B.VggNet), native_layers='dense', native_biased=True, **args)
