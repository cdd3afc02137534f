"""The table of ghn3_amd.target_ops.run_conv_window as cases: every row with the autograd node of its member, and the
combinations outside the table, which answer None.  Sizes: N=2, 6 x 6 input, C_out=8, 3 x 3 kernel, padding 1 -- the smallest
that still reach every row --, C_in=4, and C_in=3 once so that `_image_pad` is on the path."""
import collections

import torch
import torch.nn as nn

N, HW, C_OUT = 2, 6, 8
MEMBER_NODES = ('ConvBnActBackward', 'ConvBnActEvalBackward', 'ConvBnBackward', 'ConvBnEvalBackward', 'ConvOnlyBackward',
                'ConvBiasActBackward')

# norm: a factory of the norm layer (None: no norm layer); switch: the row's own switch; train / frozen: the member's node with
# batch statistics / in eval mode
Case = collections.namedtuple('Case', 'name norm biased relu residual c_in switch train frozen')


def _row(name, norm, biased, relu, residual, switch, train, frozen=None, c_in=4):
    return Case(name, norm, biased, relu, residual, c_in, switch, train, frozen or train)


_BN = nn.BatchNorm2d
ROWS = (
    _row('bn-relu', _BN, False, True, False, 'GHN3_NATIVE_ACT', 'ConvBnActBackward', 'ConvBnActEvalBackward'),
    _row('bn-add-relu', _BN, False, True, True, 'GHN3_NATIVE_ACT', 'ConvBnActBackward', 'ConvBnActEvalBackward'),
    _row('bn-relu-image', _BN, False, True, False, 'GHN3_NATIVE_ACT', 'ConvBnActBackward', 'ConvBnActEvalBackward', c_in=3),
    _row('bn', _BN, False, False, False, None, 'ConvBnBackward', 'ConvBnEvalBackward'),
    _row('bias-relu', None, True, True, False, 'GHN3_NATIVE_BIAS', 'ConvBiasActBackward'),
    _row('bias-add-relu', None, True, True, True, 'GHN3_NATIVE_BIAS', 'ConvBiasActBackward'),
    _row('bias', None, True, False, False, 'GHN3_NATIVE_BIAS', 'ConvBiasActBackward'),
    _row('bias-add', None, True, False, True, 'GHN3_NATIVE_BIAS', 'ConvBiasActBackward'),
    _row('bare', None, False, False, False, None, 'ConvOnlyBackward'),
)

OUTSIDE = (
    _row('bias-bn-relu', _BN, True, True, False, None, None),
    _row('bias-bn', _BN, True, False, False, None, None),
    _row('bare-relu', None, False, True, False, None, None),
    _row('bare-add', None, False, False, True, None, None),
    _row('bare-add-relu', None, False, True, True, None, None),
    _row('bn-add', _BN, False, False, True, None, None),
    _row('groupnorm-relu', lambda c: nn.GroupNorm(2, c), False, True, False, None, None),
    _row('instancenorm', nn.InstanceNorm2d, False, False, False, None, None),
    _row('identity', lambda c: nn.Identity(), False, False, False, None, None),
)


def build(case, device='cpu', train=True):
    """(conv, norm layer or None, x, residual or None) of a case, seeded."""
    torch.manual_seed(7)
    conv = nn.Conv2d(case.c_in, C_OUT, 3, 1, 1, bias=case.biased)
    norm = case.norm(C_OUT) if case.norm else None
    layers = nn.ModuleList([conv] + ([norm] if norm is not None else [])).to(device).train(train)
    x = torch.randn(N, case.c_in, HW, HW, device=device)
    res = torch.randn(N, C_OUT, HW, HW, device=device) if case.residual else None
    return layers[0], norm, x, res
