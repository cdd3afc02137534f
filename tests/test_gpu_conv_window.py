"""The routing of ghn3_amd.target_ops.run_conv_window on the GPU: WHICH member of the dense-convolution family runs for every row of
its table (tests/conv_window_cases.py), in training and in eval mode, which combinations it refuses, and what its switches turn
off.  The members' numerics are the subject of tests/test_gpu_target_resblock.py, _bnact.py, _bias.py and _edges.py."""
import pytest
import torch

import conv_window_cases as W
from util_gpu import _graph_nodes

pytestmark = pytest.mark.gpu


def _run(case, train=True):
    from ghn3_amd import target_ops as T
    conv, norm, x, res = W.build(case, 'cuda', train)
    return T.run_conv_window(conv, norm, x, case.relu, res), norm


# (a row without a norm layer has one mode)
ROW_MODES = [(c, t) for c in W.ROWS for t in ((True, False) if c.norm else (True,))]


@pytest.mark.parametrize('case,train', ROW_MODES, ids=['%s-%s' % (c.name, 'train' if t else 'eval') for c, t in ROW_MODES])
def test_every_row_runs_its_member(case, train):
    out, norm = _run(case, train)
    assert out is not None and tuple(out.shape) == (W.N, W.C_OUT, W.HW, W.HW)
    assert out.is_contiguous(memory_format=torch.channels_last)
    names = _graph_nodes(out).split()
    assert sorted(n for n in names if n in W.MEMBER_NODES) == [case.train if train else case.frozen], names
    assert not any(n.startswith('ConvolutionBackward') for n in names), names
    if norm is not None:
        # batch statistics: the running ones follow, as torch's would; eval mode: untouched
        moved = bool((norm.running_mean != 0).any())
        assert moved == train and int(norm.num_batches_tracked) == int(train)


@pytest.mark.parametrize('train', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('case', W.OUTSIDE, ids=lambda c: c.name)
def test_combinations_outside_the_table_answer_none(case, train):
    out, norm = _run(case, train)
    assert out is None
    if getattr(norm, 'num_batches_tracked', None) is not None:
        assert int(norm.num_batches_tracked) == 0


@pytest.mark.parametrize('switch', ['GHN3_NATIVE_ACT', 'GHN3_NATIVE_BIAS', 'GHN3_NATIVE_CONV'])
def test_a_switch_turns_off_its_rows_only(switch, monkeypatch):
    monkeypatch.setenv(switch, '0')
    for case, train in ROW_MODES:
        out, _ = _run(case, train)
        assert (out is None) == (switch in (case.switch, 'GHN3_NATIVE_CONV')), (case.name, train)
