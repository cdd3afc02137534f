"""
The edge-shape table of the target-network ops (tests/target_edge_cases.py) and the per-slice error measure
(tests/util_parity.slice_errors), checked without a GPU:

  * every row is well conditioned under the measure, independently of the kernels: the stock torch layers in fp32 against the
    same layers in fp64 stay within 1e-5 per slice, and every row with a norm layer keeps the smallest per-channel batch
    variance of its pre-norm result at or above VAR_FLOOR.  Measured: at most 1.5e-6, and 2.6e-6 on the two 128 x 128 rows;
  * the measure sees what the whole-tensor ratio of test_gpu_target_ops.py lets through: an error planted in one 4-channel
    tail group, in one border column, in one tap of a 7 x 7 weight gradient.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import target_edge_cases as E
from util_parity import rel_l2, slice_errors

CPU_TOL = 1e-5


def _conv_ref(x, w, gamma, beta, st, pad, dil, relu):
    """(pre-norm result, output) of [ReLU ->] convolution -> BatchNorm with batch statistics, stock layers; gamma None: no norm."""
    z = F.conv2d(F.relu(x) if relu else x, w, None, st, pad, dil)
    return z, (z if gamma is None else F.batch_norm(z, None, None, gamma, beta, True, 0.1, 1e-5))


def _dwpw_ref(x, w_dw, w_pw, gamma, beta, st, pad, dil):
    y = F.relu(x) if w_dw is None else F.conv2d(F.relu(x), w_dw, None, st, pad, dil, groups=x.shape[1])
    z = F.conv2d(y, w_pw, None, st if w_dw is None else 1)
    return z, F.batch_norm(z, None, None, gamma, beta, True, 0.1, 1e-5)


def _both_precisions(fn, tensors, up):
    """fn on fp32 and on fp64 leaves -> [(output, gradients...)] for the two precisions, and the fp64 pre-norm result."""
    res = []
    for dt in (torch.float32, torch.float64):
        leaves = [t.clone().to(dt).requires_grad_(True) for t in tensors]
        z, out = fn(*leaves)
        (out * up.to(dt)).sum().backward()
        res.append([out.detach()] + [t.grad for t in leaves])
    return res[0], res[1], z.detach()


def _check(got, ref, axes, names):
    worst = 0.0
    for name, a, b, ax in zip(names, got, ref, axes):
        v, where = slice_errors(a, b, ax)
        worst = max(worst, v)
        assert v <= CPU_TOL, (name, v, where)
    return worst


@pytest.mark.parametrize('row', E.CONV_ROWS, ids=str)
def test_conv_rows_are_well_conditioned(row):
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    x, w, gamma, beta, up = E.conv_inputs(row)
    got, ref, z = _both_precisions(lambda *t: _conv_ref(*t, st, pad, dil, relu), (x, w, gamma, beta), up)
    var = float(z.var((0, 2, 3), unbiased=False).min())
    print('conv_bn', row, 'min variance %.4f' % var)
    assert var >= E.VAR_FLOOR, var
    worst = _check(got, ref, [E.ACT_AXES, E.ACT_AXES, E.WGRAD_AXES, E.VEC_AXES, E.VEC_AXES], ('out', 'dx', 'dw', 'dgamma', 'dbeta'))
    print('  fp32 against fp64, worst slice: %.2e' % worst)


@pytest.mark.parametrize('row', E.CONV_ONLY_ROWS, ids=str)
def test_conv_only_rows_are_well_conditioned(row):
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    x, w, _, _, up = E.conv_inputs(row, seed_extra=E.CONV_ONLY_SEED)
    got, ref, _ = _both_precisions(lambda *t: _conv_ref(*t, None, None, st, pad, dil, relu), (x, w), up)
    worst = _check(got, ref, [E.ACT_AXES, E.ACT_AXES, E.WGRAD_AXES], ('out', 'dx', 'dw'))
    print('conv_only', row, 'fp32 against fp64, worst slice: %.2e' % worst)


@pytest.mark.parametrize('row', E.DWPW_ROWS, ids=str)
def test_dwpw_rows_are_well_conditioned(row):
    N, Ci, Co, H, W, ks, st, pad, dil, gain = row
    x, w_dw, w_pw, gamma, beta, up = E.dwpw_inputs(row)
    got, ref, z = _both_precisions(lambda *t: _dwpw_ref(*t, st, pad, dil), (x, w_dw, w_pw, gamma, beta), up)
    var = float(z.var((0, 2, 3), unbiased=False).min())
    print('dwpw_bn', row, 'min variance %.4f' % var)
    assert var >= E.VAR_FLOOR, var
    worst = _check(got, ref, [E.ACT_AXES, E.ACT_AXES, E.WGRAD_AXES, E.WGRAD_AXES, E.VEC_AXES, E.VEC_AXES],
                   ('out', 'dx', 'dw_dw', 'dw_pw', 'dgamma', 'dbeta'))
    print('  fp32 against fp64, worst slice: %.2e' % worst)


@pytest.mark.parametrize('row', E.PW_ROWS, ids=str)
def test_pointwise_rows_are_well_conditioned(row):
    N, Ci, Co, H, W, st = row
    x, w_pw, gamma, beta, up = E.pw_inputs(row)
    got, ref, z = _both_precisions(lambda a, b, c, d: _dwpw_ref(a, None, b, c, d, st, 0, 1), (x, w_pw, gamma, beta), up)
    var = float(z.var((0, 2, 3), unbiased=False).min())
    print('pointwise', row, 'min variance %.4f' % var)
    assert var >= E.VAR_FLOOR, var
    worst = _check(got, ref, [E.ACT_AXES, E.ACT_AXES, E.WGRAD_AXES, E.VEC_AXES, E.VEC_AXES], ('out', 'dx', 'dw_pw', 'dgamma', 'dbeta'))
    print('  fp32 against fp64, worst slice: %.2e' % worst)


@pytest.mark.parametrize('row', E.SE_ROWS, ids=str)
def test_se_rows_are_well_conditioned(row):
    from ghn3_amd import ops
    N, C, H, W, stride = row
    x, up = E.se_inputs(row)
    torch.manual_seed(C + H)
    m = ops.ChannelSELayer(C, stride=stride)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(3.0)
    res = []
    for dt in (torch.float32, torch.float64):
        mm = ops.ChannelSELayer(C, stride=stride).to(dt)
        mm.load_state_dict({k: v.to(dt) for k, v in m.state_dict().items()})
        xx = x.detach().clone().to(dt).requires_grad_(True)
        out = mm(xx)
        (out * up.to(dt)).sum().backward()
        res.append([out.detach(), xx.grad] + [p.grad for p in mm.parameters()])
    axes = [E.ACT_AXES, E.ACT_AXES] + [E.MAT_AXES if p.dim() == 2 else E.VEC_AXES for p in m.parameters()]
    worst = _check(res[0], res[1], axes, ['out', 'dx'] + [n for n, _ in m.named_parameters()])
    print('se', row, 'fp32 against fp64, worst slice: %.2e' % worst)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('row', E.POOL_ROWS, ids=str)
def test_pool_rows_hold_ties(row, mode):
    N, C, H, W, k, s, pad = row
    x, up = E.pool_inputs(row, mode)
    assert float((x == 0).float().mean()) >= 0.4
    res = []
    for dt in (torch.float32, torch.float64):
        xx = x.detach().clone().to(dt).requires_grad_(True)
        out = F.max_pool2d(xx, k, s, pad) if mode else F.avg_pool2d(xx, k, s, pad, count_include_pad=False)
        (out * up.to(dt)).sum().backward()
        res.append([out.detach(), xx.grad])
    _check(res[0], res[1], [E.ACT_AXES, E.ACT_AXES], ('out', 'dx'))


def test_dead_channel_rows_name_an_output_channel():
    for row, ch in (E.CONV_DEAD, E.DWPW_DEAD):
        assert 0 <= ch < row[2]


# ---- the measure itself ------------------------------------------------------------------------------------------------
OLD_TOL = 2e-4        # what the whole-tensor ratio of test_gpu_target_ops.py asks of an output


def _reference_tensors():
    """An fp64 output with 132 channels and an fp64 7 x 7 weight gradient, from rows of the table."""
    row = E.CONV_ROWS[2]
    x, w, gamma, beta, up = (t.double() for t in E.conv_inputs(row))
    out = _conv_ref(x, w, gamma, beta, row[6], row[7], row[8], row[9])[1]
    row7 = E.CONV_ROWS[6]
    x7, w7, g7, b7, up7 = (t.double() for t in E.conv_inputs(row7))
    w7.requires_grad_(True)
    (_conv_ref(x7, w7, g7, b7, row7[6], row7[7], row7[8], row7[9])[1] * up7).sum().backward()
    row4 = E.CONV_ROWS[3]
    x4, w4, g4, b4, _ = (t.double() for t in E.conv_inputs(row4))
    out4 = _conv_ref(x4, w4, g4, b4, row4[6], row4[7], row4[8], row4[9])[1]
    return out, w7.grad, out4


def test_slice_errors_is_zero_on_equal_tensors_and_reports_the_slice():
    out, dw, _ = _reference_tensors()
    assert slice_errors(out, out.clone(), E.ACT_AXES)[0] == 0.0
    bad = out.clone()
    bad[1, 7, 1, 0] += 1.0
    v, (axes, idx) = slice_errors(bad, out, [(1,)])
    assert axes == (1,) and idx == (7,)
    assert abs(v - 1.0 / (float(out.norm()) / out.shape[1] ** 0.5)) < 1e-12
    bad[0, 0, 0, 0] = float('nan')
    assert slice_errors(bad, out, E.ACT_AXES)[0] == float('inf')
    assert slice_errors(np.ones(4), np.zeros(4), E.VEC_AXES)[0] == 1.0       # (an all-zero reference: absolute)


def test_a_wrong_channel_tail_group_passes_the_whole_tensor_ratio_and_fails_the_slices():
    out, _, _ = _reference_tensors()
    bad = out.clone()
    bad[:, 128:132] *= 1 + 1e-3                    # 0.1 % in the last four of 132 channels
    assert rel_l2(bad, out) < OLD_TOL
    v, (axes, idx) = slice_errors(bad, out, E.ACT_AXES)
    assert v > OLD_TOL and axes == (1,) and idx[0] >= 128, (v, axes, idx)


def test_a_wrong_border_column_passes_the_whole_tensor_ratio_and_fails_the_slices():
    _, _, out = _reference_tensors()               # (3, 28, 5, 4)
    bad = out.clone()
    bad[:, :, :, -1] *= 1 + 3e-4
    assert rel_l2(bad, out) < OLD_TOL
    v, (axes, idx) = slice_errors(bad, out, E.ACT_AXES)
    assert v > OLD_TOL and axes == (2, 3) and idx[1] == out.shape[3] - 1, (v, axes, idx)


def test_a_wrong_tap_of_a_7x7_weight_gradient_passes_the_whole_tensor_ratio_and_fails_the_slices():
    _, dw, _ = _reference_tensors()
    bad = dw.clone()
    bad[:, :, 3, 3] *= 1 + 8e-4
    assert rel_l2(bad, dw) < OLD_TOL
    v, (axes, idx) = slice_errors(bad, dw, E.WGRAD_AXES)
    assert v > OLD_TOL and axes == (2, 3) and idx == (3, 3), (v, axes, idx)
