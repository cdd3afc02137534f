"""ghn3_amd.target_ops.run_conv_window without a GPU: on CPU tensors every row of its table (tests/conv_window_cases.py) and
every combination outside it answers None -- the caller keeps its stock layers --, in training and in eval mode, and the two
switches of its rows read as before."""
import pytest
import torch.nn as nn

import conv_window_cases as W
from ghn3_amd import native_net
from ghn3_amd import target_ops as T


@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('case', W.ROWS + W.OUTSIDE, ids=lambda c: c.name)
def test_every_combination_answers_none_on_cpu_tensors(case, train):
    conv, norm, x, res = W.build(case, train=train)
    before = None if norm is None or getattr(norm, 'running_mean', None) is None else norm.running_mean.clone()
    assert T.run_conv_window(conv, norm, x, case.relu, res) is None
    if before is not None:
        assert (norm.running_mean == before).all() and int(norm.num_batches_tracked) == 0
    # the window over the same layers computes what they compute, bit for bit
    win = native_net.NativeConvWindow(conv, norm, case.relu)
    y = conv(x) if norm is None else norm(conv(x))
    y = y if res is None else y + res
    assert (win(x, res) == (nn.functional.relu(y) if case.relu else y)).all()


def test_the_forwards_keep_their_none_answers():
    conv, bn, x, _ = W.build(W.ROWS[0])
    biased = nn.Conv2d(4, W.C_OUT, 3, 1, 1)
    assert T.run_conv_bn_act(conv, bn, x) is None and T.run_conv_bn_act(biased, None, x) is None
    assert T.run_conv_bias_act(biased, x, True) is None and T.run_conv_bias_act(conv, x, False) is None


def test_the_switches_read_as_before(monkeypatch):
    assert T.act_enabled() and T.bias_enabled()
    monkeypatch.setenv('GHN3_NATIVE_ACT', '0')
    assert not T.act_enabled() and T.bias_enabled()
    monkeypatch.delenv('GHN3_NATIVE_ACT')
    monkeypatch.setenv('GHN3_NATIVE_BIAS', '0')
    assert T.act_enabled() and not T.bias_enabled()
    monkeypatch.setenv('GHN3_NATIVE_BIAS', '1')
    assert T.bias_enabled()
