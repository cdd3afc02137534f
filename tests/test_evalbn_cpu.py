"""Host side of the eval-mode BatchNorm members of the target-network op families (target_ops.conv_bn_eval / dwpw_bn_eval on
ghn3_conv_frozen_* / ghn3_dwpw_frozen_*), without a GPU: the C ABI declares and exports the new entry points at the same ABI
version, the `applicable` functions refuse what the kernels do not take, and on CPU tensors every runner returns what the stock
modules return for a block whose BatchNorm normalises with its running statistics."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['ghn3_dwpw_frozen_scratch_floats', 'ghn3_dwpw_frozen_fwd', 'ghn3_dwpw_frozen_bwd',
       'ghn3_conv_frozen_scratch_floats', 'ghn3_conv_frozen_fwd', 'ghn3_conv_frozen_bwd']


def test_new_entry_points_are_declared_and_listed_at_abi_21():
    from ghn3_amd import _lib as L
    with open(os.path.join(ROOT, 'include', 'ghn3_hip.h'), encoding='utf-8') as fh:
        header = fh.read()
    assert L.ABI_VERSION == 21 and re.search(r'#define\s+GHN3_ABI_VERSION\s+21\b', header)
    for name in NEW:
        assert re.search(r'\b(int|int64_t)\s+%s\(' % name, header), name
        assert name in L.EXPORTS, name
    if os.path.exists(L.LIB_PATH):                                 # (a built tree: the library exports them too)
        lib = L.load()
        assert all(hasattr(lib, name) for name in NEW) and lib.ghn3_abi_version() == 21


def test_applicable_refuses_what_the_kernels_do_not_take():
    from ghn3_amd import target_ops as T
    r = torch.randn
    x, w, wd, wp = r(2, 8, 6, 6), r(12, 8, 3, 3), r(8, 1, 3, 3), r(12, 8)
    g, b, rm, rv = r(12), r(12), r(12), r(12).abs()
    # CPU tensors, whatever else holds
    assert not T.ConvBnEval.applicable(x, w, g, b, rm, rv, 1, 1, 1)
    assert not T.DwPwBnEval.applicable(x, wd, wp, g, b, rm, rv, 3)
    # wrong dtypes, a missing statistic, one of another length, channel counts that are no multiple of 4
    assert not T.ConvBnEval.applicable(x.double(), w.double(), g.double(), b.double(), rm.double(), rv.double(), 1, 1, 1)
    assert not T.DwPwBnEval.applicable(x.half(), wd.half(), wp.half(), g.half(), b.half(), rm.half(), rv.half(), 3)
    assert not T.ConvBnEval.applicable(x, w, g, b, None, rv, 1, 1, 1)
    assert not T.DwPwBnEval.applicable(x, wd, wp, g, b, rm, None, 3)
    assert not T.ConvBnEval.applicable(r(2, 6, 6, 6), r(12, 6, 3, 3), g, b, rm, rv, 1, 1, 1)
    assert not T.DwPwBnEval.applicable(x, wd, r(10, 8), r(10), r(10), r(10), r(10), 3)
    assert not T.ConvBnEval.applicable(x, w, None, b, rm, rv, 1, 1, 1)
    # the statistics' own test, on tensors that only lack the device
    assert not T._frozen_stats_ok(rm, rv, 12) and not T._frozen_stats_ok(None, None, 12)
    for fn, args in ((T.conv_bn_eval, (x, w, g, b, rm, rv)), (T.dwpw_bn_eval, (x, wd, wp, g, b, rm, rv))):
        with pytest.raises(T.L.Ghn3Error):
            fn(*args)


def test_conv_desc_fits_mirrors_both_2_31_rules_of_check_cdesc():
    """check_cdesc refuses N H W max(C_in, C_out) >= 2^31 and N Ho Wo max(C_in, C_out) >= 2^31; x.numel() < 2^31 sees neither
    when C_out is the wider side."""
    from ghn3_amd import target_ops as T

    class Shape:
        def __init__(self, *shape):
            self.shape = shape

    def fits(x, w, stride, pad):
        return T.conv_desc_fits(T._conv_desc(Shape(*x), Shape(*w), stride, pad, 1, True, 1e-5))

    assert fits((2, 8, 6, 6), (12, 8, 3, 3), 1, 1)
    # input pixels x C_out: 256 x 224 x 224 x 256 = 2^31 x 1.53 although the padded image itself has 51 M elements
    assert not fits((256, 4, 224, 224), (256, 4, 3, 3), 2, 1)
    # output pixels x C_out exactly 2^31 (input pixels x C_out as well); one pixel row less on either side of the limit
    assert not fits((1, 4, 2048, 2048), (512, 4, 1, 1), 1, 0)
    assert fits((1, 4, 2047, 2048), (512, 4, 1, 1), 1, 0)
    # only the output side over the limit: padding grows the image (2046 + 2 x 1 - 0 = 2048 rows and columns of a 1 x 1 kernel)
    assert fits((1, 4, 2046, 2046), (512, 4, 1, 1), 1, 0) and not fits((1, 4, 2046, 2046), (512, 4, 1, 1), 1, 1)
    # no output at all
    assert not fits((1, 4, 2, 2), (8, 4, 3, 3), 1, 0)


def test_the_switch_is_read_per_call_and_only_for_frozen_statistics(monkeypatch):
    from ghn3_amd import target_ops as T
    monkeypatch.delenv('GHN3_NATIVE_EVALBN', raising=False)
    assert T._frozen_norm(False) and not T._frozen_norm(True)
    monkeypatch.setenv('GHN3_NATIVE_EVALBN', '0')
    assert not T._frozen_norm(False) and not T._frozen_norm(True)
    bn = torch.nn.BatchNorm2d(4)
    assert T._norm_inputs(bn)[3] and not T._norm_inputs(bn.eval())[3]
    assert T._norm_inputs(torch.nn.BatchNorm2d(4, track_running_stats=False).eval())[3]       # nothing to freeze


def _eval_block(m, seed):
    """A torch.nn-flavour block in eval mode with seeded running statistics."""
    g = torch.Generator().manual_seed(seed)
    for sub in m.modules():
        if isinstance(sub, torch.nn.BatchNorm2d):
            with torch.no_grad():
                sub.running_mean.copy_(0.5 * torch.randn(sub.num_features, generator=g))
                sub.running_var.copy_(0.5 + 1.5 * torch.rand(sub.num_features, generator=g))
                sub.weight.copy_(1 + 0.3 * torch.randn(sub.num_features, generator=g))
                sub.bias.copy_(0.2 * torch.randn(sub.num_features, generator=g))
    return m.eval()


def _seq(layers, x):
    for m in layers:
        x = m(x)
    return x


def test_every_runner_returns_the_stock_result_on_a_cpu_eval_mode_block():
    from ghn3_amd import ops, target_ops as T
    torch.manual_seed(5)
    x = torch.randn(2, 12, 8, 8)
    cases = [(T.run_block, ops.DilConv(12, 16, 3, 2, 2, 2, norm='bn-track')),
             (T.run_pointwise_block, ops.ReLUConvBN(12, 16, 1, 2, 0, norm='bn-track')),
             (T.run_conv_block, ops.ReLUConvBN(12, 16, 3, 1, 1, norm='bn-track')),
             (T.run_conv_pair_block, ops.ReLUConvBN(12, 12, 7, 2, 3, norm='bn-track', double=True))]
    for k, (runner, m) in enumerate(cases):
        m = _eval_block(m, 30 + k)
        layers = list(m.op)
        bn = layers[-1]
        before = [t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
        with torch.no_grad():
            want = _seq(layers, x)
            got = runner(layers, x)
            stock_bn = F.batch_norm(_seq(layers[:-1], x), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.1, bn.eps)
        assert torch.equal(got, want) and torch.equal(got, stock_bn), runner.__name__
        assert torch.equal(got, m(x))
        for a, b in zip(before, (bn.running_mean, bn.running_var, bn.num_batches_tracked)):
            assert torch.equal(a, b)
    # a stem: [Conv2d, BatchNorm2d, ReLU, Conv2d, BatchNorm2d] windows, a 3-channel image
    stem = _eval_block(torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, 1, 1, bias=False), torch.nn.BatchNorm2d(8),
                                           torch.nn.ReLU(inplace=False), torch.nn.Conv2d(8, 16, 3, 2, 1, bias=False),
                                           torch.nn.BatchNorm2d(16)), 40)
    img = torch.randn(2, 3, 8, 8)
    with torch.no_grad():
        assert torch.equal(T.run_layer_seq(stem, img), stem(img))
    # FactorizedReduce: the runner declines (None) and the module runs its stock layers
    fr = _eval_block(ops.FactorizedReduce(12, 16, norm='bn-track'), 41)
    with torch.no_grad():
        assert T.run_factorized_reduce(fr.relu, fr.conv_1, fr.conv_2, fr.bn, x) is None
        y = fr.relu(x)
        want = fr.bn(torch.cat([fr.conv_1(y), fr.conv_2(y[:, :, 1:, 1:])], dim=1))
        assert torch.equal(fr(x), want)
