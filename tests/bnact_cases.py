"""Cases of the stand-alone BatchNorm [+ ReLU] (ghn3_bn_act_*, ghn3_amd/csrc/tnet_bnact.hip) and of nativize(windows='all'), shared
by tests/test_bnact_cpu.py (the cases are well conditioned; nativize on the CPU) and tests/test_gpu_target_bnact.py (the kernels
against fp64; whole networks against the stock GPU path).

A case is (N, H, W, C) with P = N H W rows; every one runs with the ReLU on and off and with batch and frozen statistics.  The
shapes follow the kernels' geometry: 64-row chunks (P = 63, 64, 65; 4097 = 65 chunks, the last of one row), 64-channel blocks
(C = 260: five blocks, the last of one quad), the loop over channel blocks above 1024 channels (C = 1028), C = 4 and 8 (one and
two quads: 256 and 128 row lanes).

THE MASK (the convention of tests/resblock_cases.py).  An fp32 kernel and the fp64 reference may disagree on the sign of a
pre-activation within rounding of zero.  The upstream gradient is therefore 0 wherever the fp64 pre-activation has |y| <
MASK_BAND = 2e-3, and no more than MASK_SHARE = 1 % of a case's elements may be zeroed that way: with |gamma| >= 0.5 a standard
normal channel has at most 2 * 2e-3 / 0.5 * 0.399 = 0.32 % of its values in the band.  A condition on the cases, asserted by the
CPU test.
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import resblock_cases as R

MASK_BAND = R.MASK_BAND
MASK_SHARE = R.MASK_SHARE
EPS = 1e-5

# name -> (N, H, W, C)
SHAPES = {
    'min': (2, 1, 1, 4),
    'p63': (7, 3, 3, 20),
    'p64': (4, 4, 4, 20),
    'p65': (5, 13, 1, 20),
    'chunks': (17, 241, 1, 8),          # P = 4097
    'blocks': (2, 5, 13, 260),          # P = 130
    'wide': (2, 5, 7, 1028),            # P = 70
    'special': (4, 8, 8, 24),           # P = 256
}
# the special case: a channel whose mean lies 100 standard deviations from zero, a constant one (variance 0, beta = 0.3), one
# the ReLU masks everywhere (beta = -8) and one it never masks (beta = +8)
FAR_CH, CONST_CH, MASKED_CH, OPEN_CH = 5, 9, 14, 22
CONST_VALUE = 1.5


def rows_of(name):
    N, H, W, C = SHAPES[name]
    return N * H * W


def inputs(name):
    """(x (N, C, H, W), gamma, beta, up) in fp32, seeded: channels of different means and spreads, |gamma| in [0.5, 1.5]."""
    N, H, W, C = SHAPES[name]
    g = torch.Generator().manual_seed(100 + sum(ord(ch) for ch in name))
    spread = 0.5 + 1.5 * torch.rand(C, generator=g)
    centre = torch.randn(C, generator=g)
    x = torch.randn(N, C, H, W, generator=g) * spread.view(1, C, 1, 1) + centre.view(1, C, 1, 1)
    gamma = (0.5 + torch.rand(C, generator=g)) * (1 - 2 * (torch.rand(C, generator=g) < 0.3).float())
    beta = 0.3 * torch.randn(C, generator=g)
    up = torch.randn(N, C, H, W, generator=g)
    if name == 'min':
        # Two rows per channel at centre -+ s: the variance is s^2 and xhat = -+1 / sqrt(1 + eps / s^2), so the true dx is
        # -+ gamma rstd (g1 - g2) / 2 * eps / (s^2 + eps) -- it vanishes but for eps.  With s = 0.005 .. 0.02 (s^2 = 2.5 .. 40 eps)
        # that factor is 0.02 .. 0.3 and dx is conditioned; with s of order 1 it would be 1e-5 and dx the rounding of any fp32
        # implementation, torch's included.
        small = 0.01 * spread
        x = centre.view(1, C, 1, 1) + small.view(1, C, 1, 1) * torch.tensor([-1.0, 1.0]).view(2, 1, 1, 1)
    if name == 'special':
        x[:, FAR_CH] = 100.0 * spread[FAR_CH] + spread[FAR_CH] * torch.randn(N, H, W, generator=g)
        x[:, CONST_CH] = CONST_VALUE
        beta[CONST_CH], beta[MASKED_CH], beta[OPEN_CH] = 0.3, -8.0, 8.0
    return x.contiguous(), gamma, beta, up


def running_of(name, x):
    """Running statistics of the frozen cases: a mean near the batch's, a variance within a quarter of it (1 for the constant
    channel)."""
    C = x.shape[1]
    g = torch.Generator().manual_seed(300 + C + rows_of(name))
    var = x.double().var((0, 2, 3), unbiased=False).float()
    mean = x.double().mean((0, 2, 3)).float()
    var = torch.where(var > 0, var, torch.ones_like(var))
    return mean + 0.1 * var.sqrt() * torch.randn(C, generator=g), var * (0.75 + 0.5 * torch.rand(C, generator=g))


def reference(x, gamma, beta, relu, running=None):
    """(pre-activation y, out) of the stock layers on the given tensors (any dtype)."""
    if running is None:
        y = F.batch_norm(x, None, None, gamma, beta, True, 0.1, EPS)
    else:
        y = F.batch_norm(x, running[0], running[1], gamma, beta, False, 0.1, EPS)
    return y, (F.relu(y) if relu else y)


@functools.lru_cache(maxsize=None)
def case(name, relu, frozen):
    """A case, computed once and left unchanged: the fp32 CPU inputs (`up`: the conditioned upstream gradient; `running` for
    frozen cases), the fp64 reference results y, out, mean, var and the gradients dx, dgamma, dbeta, and `share`, the zeroed share
    of `up` (0 without the ReLU: there is no kink)."""
    x, gamma, beta, up = inputs(name)
    running = running_of(name, x) if frozen else None
    leaves = [t.double().requires_grad_(True) for t in (x, gamma, beta)]
    y, out = reference(*leaves, relu, None if running is None else [t.double() for t in running])
    near = (y.detach().abs() < MASK_BAND) if relu else torch.zeros_like(up, dtype=torch.bool)
    up = torch.where(near, torch.zeros_like(up), up)
    (out * up.double()).sum().backward()
    xd = x.double()
    return dict(x=x, gamma=gamma, beta=beta, up=up, running=running, y=y.detach(), out=out.detach(), mean=xd.mean((0, 2, 3)),
                var=xd.var((0, 2, 3), unbiased=False), dx=leaves[0].grad, dgamma=leaves[1].grad, dbeta=leaves[2].grad,
                share=float(near.float().mean()))


def all_cases():
    """(id, name, relu, frozen) of every case either test file runs."""
    return [('%s-%s-%s' % (name, 'relu' if relu else 'plain', 'frozen' if frozen else 'batch'), name, relu, frozen)
            for name in SHAPES for relu in (True, False) for frozen in (False, True)]


# what ghn3_bn_act_scratch_floats refuses with GHN3_E_LIMIT (-2), and bn_act_refusal with it: name -> (N, C, H, W), frozen, rule
LIMITS = {
    'C % 4': ((2, 6, 3, 3), False, 'channels'),
    'C > 16384': ((1, 16388, 1, 2), False, 'width'),
    'P C >= 2^31': ((2 ** 13, 1024, 2 ** 4, 2 ** 4), False, 'size'),
    'P == 1 batch': ((1, 8, 1, 1), False, 'rows'),
}
ACCEPTED = {
    'P == 1 frozen': ((1, 8, 1, 1), True),
    'C == 16384': ((1, 16384, 1, 2), False),
    'P C just below 2^31': ((2 ** 13 - 1, 1024, 2 ** 4, 2 ** 4), False),
}


# ---- two networks for nativize(windows='all') ---------------------------------------------------------------------------------------
class DenseLayer(nn.Module):
    def __init__(self, cin, growth, bn_size=4):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, bn_size * growth, 1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth)
        self.conv2 = nn.Conv2d(bn_size * growth, growth, 3, 1, 1, bias=False)

    def forward(self, x):
        y = self.conv1(F.relu(self.norm1(x)))
        y = self.conv2(F.relu(self.norm2(y)))
        return torch.cat([x, y], 1)


class Transition(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm = nn.BatchNorm2d(cin)
        self.relu = nn.ReLU(inplace=True)
        self.conv = nn.Conv2d(cin, cout, 1, bias=False)

    def forward(self, x):
        return F.avg_pool2d(self.conv(self.relu(self.norm(x))), 2)


class DenseNetBC(nn.Module):
    """DenseNet-BC in the CIFAR form: a bare 3 x 3 stem, two dense blocks of two bottleneck layers (growth 8), a transition that
    halves the channels, BatchNorm -> ReLU -> global pool -> Linear."""
    input_hw = 16
    # read off the definition.  default: conv1 -> norm2 -> ReLU of each of the four layers; the transition's pool; the head
    windows = {'conv_bn_relu': 4, 'conv_bn_add_relu': 0, 'conv_bn': 0, 'pool': 1, 'head': 1}
    # 'all': norm1 of four layers + the transition's + the last one; the stem, conv2 of four layers and the transition's
    # convolution; one concatenation per layer
    extra = {'bn_relu': 6, 'bn': 0, 'conv': 6, 'concat': 4, 'add': 0}
    stock_default = 6

    def __init__(self):
        super().__init__()
        self.conv0 = nn.Conv2d(3, 16, 3, 1, 1, bias=False)
        self.block1 = nn.Sequential(DenseLayer(16, 8), DenseLayer(24, 8))
        self.trans = Transition(32, 16)
        self.block2 = nn.Sequential(DenseLayer(16, 8), DenseLayer(24, 8))
        self.norm = nn.BatchNorm2d(32)
        self.fc = nn.Linear(32, 10)

    def forward(self, x):
        x = self.block2(self.trans(self.block1(self.conv0(x))))
        x = F.relu(self.norm(x))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


class PreActBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.shortcut = None
        if stride != 1 or cin != cout:
            self.shortcut = nn.Conv2d(cin, cout, 1, stride, bias=False)

    def forward(self, x):
        o = F.relu(self.bn1(x))
        skip = x if self.shortcut is None else self.shortcut(o)
        y = self.conv2(F.relu(self.bn2(self.conv1(o))))
        return y + skip


class PreActResNet(nn.Module):
    """Pre-activation (v2) ResNet: a bare stem, a block with an identity skip, one with a 1 x 1 stride-2 shortcut."""
    input_hw = 16
    windows = {'conv_bn_relu': 2, 'conv_bn_add_relu': 0, 'conv_bn': 0, 'pool': 0, 'head': 1}
    # bn1 of both blocks (its ReLU has two users in the second) and the last norm layer; the stem (two users), conv2 of both blocks
    # and the shortcut; one sum per block
    extra = {'bn_relu': 3, 'bn': 0, 'conv': 4, 'concat': 0, 'add': 2}
    stock_default = 4

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 3, 1, 1, bias=False)
        self.layer1 = PreActBlock(8, 8, 1)
        self.layer2 = PreActBlock(8, 16, 2)
        self.bn = nn.BatchNorm2d(16)
        self.fc = nn.Linear(16, 10)

    def forward(self, x):
        x = self.layer2(self.layer1(self.conv1(x)))
        x = torch.relu(self.bn(x))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


NETS = [DenseNetBC, PreActResNet]
make_net, net_batch = R.make_net, R.net_batch


def windows_all(cls):
    """The report of nativize(windows='all') for one of NETS, or for a network of resblock_cases (no extra window)."""
    return dict(cls.windows, **getattr(cls, 'extra', dict.fromkeys(('bn_relu', 'bn', 'conv', 'concat', 'add'), 0)))
