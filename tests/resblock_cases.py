"""Cases of the "act" member of the dense-convolution family (conv -> BatchNorm [-> + skip] -> ReLU: ghn3_conv_bn_act_*,
ghn3_conv_frozen_act_*) and of ghn3_amd.nativize, shared by tests/test_resblock_cpu.py (the cases are well conditioned; nativize on
the CPU) and tests/test_gpu_target_resblock.py (the kernels against fp64; whole networks against the stock GPU path).

Rows in the format of tests/target_edge_cases.CONV_ROWS -- N, C_in, C_out, H, W, (kh, kw), (sh, sw), (ph, pw), dil, relu_in, gain --
and the inputs of `conv_inputs`; every row runs with and without a skip tensor.  As there, the smallest per-channel batch variance
of the pre-norm result stays at or above VAR_FLOOR.

THE MASK.  An fp32 kernel and the fp64 reference may disagree on the sign of a pre-activation y within rounding of zero; such a
flip would test the row, not the kernel.  The upstream gradient is therefore set to 0 wherever the fp64 pre-activation has
|y| < MASK_BAND = 2e-3 -- with a 2e-4 per-slice output tolerance and slice RMS values of 1 to 1.5, about seven times the
admissible absolute error -- and no more than MASK_SHARE = 1 % of a row's elements may be zeroed that way.  This is a condition
on the cases, asserted by the CPU test for every row; it is not measured against the kernels.
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import target_edge_cases as E
from target_edge_cases import VAR_FLOOR, conv_inputs, conv_out_hw   # noqa: F401  (re-exported for the two test files)

F_ = False
MASK_BAND = 2e-3
MASK_SHARE = 0.01
# tnet_bn_act_apply_kernel and tnet_dz_act_kernel walk the activations in float4 quads, grid-stride, under this many workgroups
# of 256 threads (ACT_GRID_CAP, ghn3_amd/csrc/target_ops.hip)
ACT_GRID_CAP = 2048


def _no_relu_in(row):
    return row[:9] + (F_,) + row[10:]


ROWS = [
    _no_relu_in(E.CONV_ROWS[0]),                                   # channel counts 4 mod 8, one partial pixel tile (P = 50)
    (16, 36, 44, 1, 1, (3, 3), (1, 1), (1, 1), 1, F_, 3.0),       # 1 x 1 images, P = 16
    (6, 68, 132, 3, 3, (3, 3), (2, 2), (1, 1), 1, F_, 1.0),       # stride 2; the last column group holds 4 columns
    (33, 8, 12, 1, 2, (1, 1), (1, 1), (0, 0), 1, F_, 1.0),        # P = 66: a full tile and a 2-pixel tile
    (2, 12, 260, 4, 4, (3, 3), (1, 1), (1, 1), 1, F_, 1.0),       # just over 256 columns
    # more than 256 channel quads: the looping arm of the partial-sum kernel.  N = 8: with N = 2 (P = 8) the smallest batch
    # variance of the 1028 channels is 0.042, below VAR_FLOOR
    (8, 8, 1028, 2, 2, (1, 1), (1, 1), (0, 0), 1, F_, 1.0),
    # 589 824 quads > ACT_GRID_CAP x 256 = 524 288: the second trip of the two grid-stride kernels (2.36 M activations)
    (4, 4, 64, 96, 96, (1, 1), (1, 1), (0, 0), 1, F_, 1.0),
    # the stem: 7 x 7, stride 2, pad 3 on a 3-channel image (padded to four channels as target_ops._image_pad does); P = 128
    (2, 3, 16, 16, 16, (7, 7), (2, 2), (3, 3), 1, F_, 1.0),
    E.CONV_ROWS[0],                                                # the same with a ReLU on the input as well (relu_in)
]
GRID_ROW = ROWS[6]
assert GRID_ROW[0] * GRID_ROW[2] * GRID_ROW[3] * GRID_ROW[4] // 4 > ACT_GRID_CAP * 256
assert GRID_ROW[0] * GRID_ROW[2] * GRID_ROW[3] * GRID_ROW[4] < 5_000_000
# the rows of the frozen (eval mode) member
EVAL_ROWS = [ROWS[0], ROWS[2], ROWS[7]]
# special inputs, all on ROWS[0]: channel 19 (in the 4-channel tail group) fully masked, channel 3 never masked
SPECIAL_ROW, MASKED_CH, OPEN_CH = ROWS[0], 19, 3


def residual_of(row):
    """The skip tensor of a row: standard normal, of the output's shape."""
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    g = torch.Generator().manual_seed(1000 + N + Ci + Co + H + W + sum(k))
    return torch.randn(N, Co, *conv_out_hw(H, W, k, st, pad, dil), generator=g)


def image_pad(x, w):
    """A 3-channel image and its weight with a zero fourth channel (what target_ops._image_pad does, without autograd)."""
    if x.shape[1] == 3:
        return F.pad(x, (0, 0, 0, 0, 0, 1)), F.pad(w, (0, 0, 0, 0, 0, 1))
    return x, w


def reference(x, w, gamma, beta, res, row, running=None):
    """(pre-norm z, pre-activation y, out) of the stock layers on the given tensors (any dtype)."""
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    z = F.conv2d(F.relu(x) if relu else x, w, None, st, pad, dil)
    if running is None:
        y = F.batch_norm(z, None, None, gamma, beta, True, 0.1, 1e-5)
    else:
        y = F.batch_norm(z, running[0], running[1], gamma, beta, False, 0.1, 1e-5)
    if res is not None:
        y = y + res
    return z, y, F.relu(y)


def running_of(row):
    """Running statistics of the eval-mode cases: a mean near the batch's, a variance between 0.5 and 1.5."""
    Co = row[2]
    g = torch.Generator().manual_seed(2000 + Co)
    return 0.1 * torch.randn(Co, generator=g), 0.5 + torch.rand(Co, generator=g)


@functools.lru_cache(maxsize=None)
def act_case(row, with_res, special=False, frozen=False):
    """A case, computed once and left unchanged: dict with the fp32 CPU inputs (x and w padded to four channels for the stem
    row; `res` None without a skip tensor; `up` the conditioned upstream gradient; `running` for frozen cases), the fp64
    reference results z, y, out and the gradients dx, dw, dgamma, dbeta, dres, and `share`, the zeroed share of `up`."""
    x, w, gamma, beta, up = conv_inputs(row)
    x, w = image_pad(x, w)
    if special:
        beta = beta.clone()
        beta[MASKED_CH], beta[OPEN_CH] = -10.0, 10.0
    res = residual_of(row) if with_res else None
    running = running_of(row) if frozen else None
    leaves = [t.double().requires_grad_(True) for t in (x, w, gamma, beta)] + ([res.double().requires_grad_(True)] if with_res else [])
    z, y, out = reference(*leaves[:4], leaves[4] if with_res else None, row,
                          None if running is None else [t.double() for t in running])
    near = y.detach().abs() < MASK_BAND
    up = torch.where(near, torch.zeros_like(up), up)
    (out * up.double()).sum().backward()
    grads = [t.grad for t in leaves] + ([None] if not with_res else [])
    return dict(x=x, w=w, gamma=gamma, beta=beta, res=res, up=up, running=running, z=z.detach(), y=y.detach(), out=out.detach(),
                dx=grads[0], dw=grads[1], dgamma=grads[2], dbeta=grads[3], dres=grads[4], share=float(near.float().mean()))


def kept(key, t, keep):
    """The output channels `keep` (a bool mask over C_out) of the tensor named `key`; dx has none to leave out."""
    if key in ('out', 'dres'):
        return t[:, keep]
    return t if key == 'dx' else t[keep]


def all_cases():
    """(id, row, with_res, special, frozen) of every case either test file runs."""
    out = []
    for i, row in enumerate(ROWS):
        for with_res in (False, True):
            out.append(('row%d%s' % (i, '+res' if with_res else ''), row, with_res, False, False))
    out.append(('special', SPECIAL_ROW, False, True, False))
    out.append(('special+res', SPECIAL_ROW, True, True, False))
    for i, row in enumerate(EVAL_ROWS):
        out.append(('eval%d' % i, row, i != 1, False, True))
    return out


# ---- three plain networks for nativize ---------------------------------------------------------------------------------------------
class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        y = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))


class BasicNet(nn.Module):
    """BasicBlock-style, in the shape of the example's SmallResNet: 3 x 3 stem, functional ReLU, pooling and head."""
    input_hw = 16
    # read off the definition: the stem and conv1 of each block; conv2 of each block; one downsample branch
    windows = {'conv_bn_relu': 3, 'conv_bn_add_relu': 2, 'conv_bn': 1, 'pool': 1, 'head': 1}

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(8)
        self.layers = nn.Sequential(BasicBlock(8, 8, 1), BasicBlock(8, 16, 2))
        self.fc = nn.Linear(16, 10)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 2)
        x = self.layers(x)
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


class Bottleneck(nn.Module):
    def __init__(self, cin, mid, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, mid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)                          # one module, called three times
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out)).relu_()
        out = self.bn3(self.conv3(out))
        out += identity
        return self.relu(out)


class BottleneckNet(nn.Module):
    """Bottleneck-style with downsample branches: a shared in-place nn.ReLU, .relu_(), +=, torch.relu, module pooling and head."""
    input_hw = 16
    # the stem and two per block; conv3 of each block (the downsample result is the first operand's skip tensor); two
    # downsample branches
    windows = {'conv_bn_relu': 7, 'conv_bn_add_relu': 3, 'conv_bn': 2, 'pool': 1, 'head': 1}

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(16)
        self.layer1 = nn.Sequential(Bottleneck(16, 8, 32, 1), Bottleneck(32, 8, 32, 1))
        self.layer2 = Bottleneck(32, 16, 64, 2)
        self.pool = nn.AvgPool2d(2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.flatten = nn.Flatten()
        self.fc = nn.Linear(64, 10)

    def forward(self, x):
        x = torch.relu(self.bn1(self.conv1(x)))
        x = self.pool(self.layer2(self.layer1(x)))
        return self.fc(self.flatten(self.avgpool(x)))


class StemNet(nn.Module):
    """A 7 x 7 stem with MaxPool2d(3, 2, 1), in the shape of tests/golden/graph_nets.ResNetTiny; torch.add for the skip."""
    input_hw = 32
    windows = {'conv_bn_relu': 3, 'conv_bn_add_relu': 2, 'conv_bn': 1, 'pool': 1, 'head': 1}

    class Block(BasicBlock):
        def forward(self, x):
            y = F.relu(self.bn1(self.conv1(x)))
            y = self.bn2(self.conv2(y))
            return torch.add(y, x if self.downsample is None else self.downsample(x)).relu()

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 16, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(16)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = StemNet.Block(16, 16, 1)
        self.layer2 = StemNet.Block(16, 32, 2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(32, 10)

    def forward(self, x):
        x = self.maxpool(F.relu(self.bn1(self.conv1(x))))
        x = self.layer2(self.layer1(x))
        return self.fc(torch.flatten(self.avgpool(x), 1))


NETS = [BasicNet, BottleneckNet, StemNet]


def make_net(cls, seed=5):
    """A seeded instance whose BatchNorm layers have non-trivial affine pairs and running statistics."""
    torch.manual_seed(seed)
    net = cls()
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return net


def net_batch(cls, n=6, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, cls.input_hw, cls.input_hw, generator=g), torch.randint(0, 10, (n,), generator=g)


# ---- what nativize leaves on the stock layers: (constructor of conv -> norm -> activation, a word of the reason) -------------------
class Refused(nn.Module):
    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        kw = dict(bias=False)
        if kind == 'bias':
            kw = dict(bias=True)
        elif kind == 'groups':
            kw.update(groups=2)
        elif kind == 'reflect':
            kw.update(padding_mode='reflect')
        k = 9 if kind == 'kernel' else 3
        self.conv = nn.Conv2d(4, 8, k, 1, k // 2, **kw)
        self.bn = nn.BatchNorm2d(8)
        self.act = nn.ReLU6() if kind == 'relu6' else nn.ReLU()

    def forward(self, x):
        y = self.bn(self.conv(x))
        if self.kind == 'two_users':
            return self.act(y) + y
        return self.act(y)


REFUSALS = {'bias': 'biased', 'groups': 'grouped', 'reflect': 'reflect', 'two_users': '2 users', 'relu6': 'ReLU6', 'kernel': '9 x 9'}


class Branchy(nn.Module):
    """Data-dependent control flow: torch.fx cannot trace it."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(4, 8, 3, 1, 1, bias=False)
        self.bn = nn.BatchNorm2d(8)

    def forward(self, x):
        y = self.bn(self.conv(x))
        return F.relu(y) if y.sum() > 0 else y
