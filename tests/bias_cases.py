"""Cases of the "bias" member of the dense-convolution family (conv + bias [+ skip] [-> ReLU]: ghn3_conv_bias_act_*) and of
ghn3_amd.nativize(biased=True), shared by tests/test_bias_cpu.py (the cases are well conditioned; nativize on the CPU) and
tests/test_gpu_target_bias.py (the kernels against fp64; whole networks against the stock GPU path).

Rows in the format of tests/resblock_cases.ROWS, with its inputs (`conv_inputs`, `residual_of`, `image_pad`); the bias of a row
is 0.5 randn(C_out) from torch.Generator().manual_seed(3000 + C_out).  Every row runs with and without a skip tensor and with and
without the ReLU on the result.  The fp64 reference is F.conv2d(x, w, bias, ...) [+ res], then F.relu.

The mask / column-sum pass of the backward (tnet_bias_bwd_partial_kernel) runs one workgroup per 64-pixel tile: it is not
grid-stride under a workgroup cap, so the 2.36 M-activation row 6 of resblock_cases is left out.

THE MASK: resblock_cases' condition.  With the ReLU the upstream gradient is 0 wherever the fp64 pre-activation has
|y| < MASK_BAND, for at most MASK_SHARE of a row's elements; asserted by the CPU test, not measured against the kernels.
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

import resblock_cases as R
from resblock_cases import MASK_BAND, MASK_SHARE, VAR_FLOOR, conv_inputs, image_pad, residual_of, kept   # noqa: F401  (re-exported)

ROW_IDS = (0, 1, 2, 3, 4, 5, 7, 8)
ROWS = [R.ROWS[i] for i in ROW_IDS]
# special inputs, all on ROWS[0] with the ReLU: channel 19 (in the 4-channel tail group) fully masked, channel 3 never masked
SPECIAL_ROW, MASKED_CH, OPEN_CH = R.ROWS[0], 19, 3


def bias_of(row):
    Co = row[2]
    return 0.5 * torch.randn(Co, generator=torch.Generator().manual_seed(3000 + Co))


def reference(x, w, bias, res, row, relu):
    """(pre-activation y, out) of the stock layers on the given tensors (any dtype)."""
    N, Ci, Co, H, W, k, st, pad, dil, relu_in, gain = row
    y = F.conv2d(F.relu(x) if relu_in else x, w, bias, st, pad, dil)
    if res is not None:
        y = y + res
    return y, (F.relu(y) if relu else y)


@functools.lru_cache(maxsize=None)
def bias_case(row, with_res, relu, special=False):
    """A case, computed once and left unchanged: dict with the fp32 CPU inputs (x and w padded to four channels for the stem
    row; `res` None without a skip tensor; `up` the conditioned upstream gradient), the fp64 reference results y, out and the
    gradients dx, dw, dbias, dres, `share`, the zeroed share of `up`, and `positive`, the share of y > 0."""
    x, w, _gamma, _beta, up = conv_inputs(row)
    x, w = image_pad(x, w)
    bias = bias_of(row)
    if special:
        bias[MASKED_CH], bias[OPEN_CH] = -10.0, 10.0
    res = residual_of(row) if with_res else None
    leaves = [t.double().requires_grad_(True) for t in (x, w, bias)] + ([res.double().requires_grad_(True)] if with_res else [])
    y, out = reference(*leaves[:3], leaves[3] if with_res else None, row, relu)
    near = (y.detach().abs() < MASK_BAND) if relu else torch.zeros_like(y, dtype=torch.bool)
    up = torch.where(near, torch.zeros_like(up), up)
    (out * up.double()).sum().backward()
    grads = [t.grad for t in leaves] + ([None] if not with_res else [])
    return dict(x=x, w=w, bias=bias, res=res, up=up, y=y.detach(), out=out.detach(), dx=grads[0], dw=grads[1], dbias=grads[2],
                dres=grads[3], share=float(near.float().mean()), positive=float((y.detach() > 0).float().mean()))


def all_cases():
    """(id, row, with_res, relu, special) of every case either test file runs."""
    out = []
    for i, row in zip(ROW_IDS, ROWS):
        for with_res in (False, True):
            for relu in (True, False):
                out.append(('row%d%s%s' % (i, '+res' if with_res else '', '' if relu else '-norelu'), row, with_res, relu, False))
    out.append(('special', SPECIAL_ROW, False, True, True))
    out.append(('special+res', SPECIAL_ROW, True, True, True))
    return out


# ---- two networks for nativize(biased=True) ----------------------------------------------------------------------------------------
class VggNet(nn.Module):
    """VGG-shaped: three biased conv -> ReLU stages, two max pools, AdaptiveAvgPool2d((2, 2)) on a map that is 2 x 2 already,
    flatten, Linear-ReLU-Dropout x 2, Linear.  8 x 8 images, batch 8."""
    input_hw, batch = 8, 8
    # without biased=True (either `windows`): the two max pools, nothing else -- every convolution is refused for its bias
    plain_windows = {'conv_bn_relu': 0, 'conv_bn_add_relu': 0, 'conv_bn': 0, 'pool': 2, 'head': 0}
    plain_extra = {'bn_relu': 0, 'bn': 0, 'conv': 0, 'concat': 0, 'add': 0}
    biased = {'conv_bias_relu': 3, 'conv_bias_add_relu': 0, 'conv_bias': 0, 'mlp_head': 1, 'same_size_pool': 1}
    biased_extra = plain_extra                                     # windows='all' finds nothing more

    def __init__(self, p=0.5):
        super().__init__()
        self.features = nn.Sequential(
            nn.Conv2d(3, 8, 3, 1, 1), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2),
            nn.Conv2d(8, 16, 3, 1, 1), nn.ReLU(inplace=True), nn.MaxPool2d(2, 2),
            nn.Conv2d(16, 16, 3, 1, 1), nn.ReLU(inplace=True))
        self.avgpool = nn.AdaptiveAvgPool2d((2, 2))
        self.classifier = nn.Sequential(nn.Linear(64, 32), nn.ReLU(inplace=True), nn.Dropout(p),
                                        nn.Linear(32, 32), nn.ReLU(inplace=True), nn.Dropout(p), nn.Linear(32, 10))

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


class FireNet(nn.Module):
    """A SqueezeNet fire module -- a biased 1 x 1 squeeze + ReLU feeding a 1 x 1 and a 3 x 3 expand, each with a ReLU, then
    torch.cat(., 1) --, a biased convolution followed by BatchNorm + ReLU, and a global-pool head."""
    input_hw, batch = 8, 8
    plain_windows = {'conv_bn_relu': 0, 'conv_bn_add_relu': 0, 'conv_bn': 0, 'pool': 0, 'head': 1}
    # windows='all' without biased: the BatchNorm behind the (stock) biased convolution with its ReLU, and the concatenation
    plain_extra = {'bn_relu': 1, 'bn': 0, 'conv': 0, 'concat': 1, 'add': 0}
    # the stem, the squeeze and both expands with their ReLUs; the convolution in front of the BatchNorm alone (no folding)
    biased = {'conv_bias_relu': 4, 'conv_bias_add_relu': 0, 'conv_bias': 1, 'mlp_head': 0, 'same_size_pool': 0}
    biased_extra = plain_extra                                     # under 'resnet' that BatchNorm and the cat stay stock

    def __init__(self):
        super().__init__()
        self.stem = nn.Conv2d(3, 16, 3, 1, 1)
        self.squeeze = nn.Conv2d(16, 8, 1)
        self.expand1 = nn.Conv2d(8, 16, 1)
        self.expand3 = nn.Conv2d(8, 16, 3, 1, 1)
        self.conv = nn.Conv2d(32, 24, 3, 2, 1)
        self.bn = nn.BatchNorm2d(24)
        self.fc = nn.Linear(24, 10)

    def forward(self, x):
        x = F.relu(self.stem(x))
        s = F.relu(self.squeeze(x))
        x = torch.cat([F.relu(self.expand1(s)), F.relu(self.expand3(s))], 1)
        x = F.relu(self.bn(self.conv(x)))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


NETS = [VggNet, FireNet]


def expected_windows(cls, windows, biased):
    """report()['windows'] of nativize(cls(), windows=windows, biased=biased), read off the definitions above."""
    out = dict(cls.plain_windows)
    if windows == 'all':
        out.update(cls.biased_extra if biased else cls.plain_extra)
    if biased:
        out.update(cls.biased)
    return out


def make_net(cls, seed=5, **kw):
    """A seeded instance whose BatchNorm layers have non-trivial affine pairs and running statistics.  The convolutions are
    drawn as He normal (std sqrt(2 / fan_in), the scale that keeps activations of unit size through ReLUs) with biases
    0.1 randn: under nn.Conv2d's default initialisation the 8 x 8 images shrink layer by layer until a channel in front of the
    BatchNorm has a batch variance of 1.7e-4 -- rstd 77 --, far below the VAR_FLOOR every case of this suite keeps
    (target_edge_cases), and the comparison of two fp32 paths then measures that amplification.  bn_input_variances and the
    CPU test hold the networks to the floor."""
    torch.manual_seed(seed)
    net = cls(**kw)
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, nn.Conv2d):
            with torch.no_grad():
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
        if isinstance(m, nn.BatchNorm2d):
            with torch.no_grad():
                m.weight.copy_(1 + 0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    return net


def net_batch(cls, seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(cls.batch, 3, cls.input_hw, cls.input_hw, generator=g), torch.randint(0, 10, (cls.batch,), generator=g)


def bn_input_variances(net, x):
    """The smallest per-channel batch variance in front of each BatchNorm2d of `net` on the batch x: {module name: value}."""
    seen, hooks = {}, []
    for name, m in net.named_modules():
        if isinstance(m, nn.BatchNorm2d):
            hooks.append(m.register_forward_pre_hook(
                lambda mod, args, name=name: seen.__setitem__(name, float(args[0].double().var((0, 2, 3), unbiased=False).min()))))
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    return seen
