"""Wide shapes of the target-network HIP ops (ghn3_amd/csrc/target_ops.hip): layers above the widths the native layers took
before they ran the `wide` evaluation split of DeepNets-1M (512 channels for the convolution families, 1024 for
squeeze-and-excitation), the smallest inputs that reach the code paths such widths take.  Plain tuples plus the seeded inputs
made from them, shared by tests/test_wide_cpu.py (the rows are well conditioned) and tests/test_gpu_target_wide.py (the kernels
against fp64).  The row formats and the input builders are those of tests/target_edge_cases.py.

Every row that runs with batch statistics keeps the smallest per-channel batch variance of the pre-norm result at or above
target_edge_cases.VAR_FLOOR in the fp64 reference.  The wide rows have FEW pixels (a wide layer is a late one) and MANY channels,
so the smallest of thousands of sample variances over 2 .. 18 pixels is far below the typical one: the `gain` column scales the
weight until the floor holds (a BatchNorm's output does not depend on that scale, and every error is relative to the reference).
"""
import torch

import target_edge_cases as E

T, F = True, False

# ---- dense convolution (conv_bn, conv_only, conv_bn_eval): N, C_in, C_out, H, W, (kh, kw), (sh, sw), (ph, pw), dil, relu, gain
CONV_ROWS = [
    (2, 12, 516, 3, 3, (3, 3), (1, 1), (1, 1), 1, T, 2.0),        # the first column group beyond 512; 516 % 8 == 4; P = 18
    (2, 8, 1028, 2, 2, (1, 1), (1, 1), (0, 0), 1, T, 4.0),        # nq = 257 in the norm partials / dz; P = 8
    (2, 1028, 1028, 2, 2, (1, 1), (1, 1), (0, 0), 1, T, 8.0),     # both sides wide
    (1, 16, 4096, 4, 4, (3, 3), (2, 2), (1, 1), 1, T, 32.0),      # the widest output; P = 4
    (1, 16384, 8, 1, 2, (1, 1), (1, 1), (0, 0), 1, T, 16.0),      # the widest input; P = 2
]
# the seeds of the three members (added to the seed formula of target_edge_cases.conv_inputs)
CONV_SEED = {'norm': 0, 'none': E.CONV_ONLY_SEED, 'frozen': 5}



def conv_eps(row):
    """The norm layer's eps for a CONV row: 1e-5, except where the row has TWO output pixels.  There xhat = +-sqrt(var / (var +
    eps)) exactly, and the input gradient of a BatchNorm with batch statistics, gamma rstd (dout - mean(dout) - xhat mean(dout
    xhat)), collapses to gamma rstd (dout_1 - dout_2) / 2 . eps / (var + eps): with eps = 1e-5 every gradient in front of the norm
    is the difference of two numbers that agree to five digits or more, in any arithmetic (the stock fp32 layers included), and
    a relative bound on it judges the row, not the kernel.  An eps of the size of the typical batch variance of that row (the
    gain squared, times 0.25) keeps the factor between 0.2 and 1 in every channel."""
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    Ho, Wo = E.conv_out_hw(H, W, k, st, pad, dil)
    return 0.25 * gain * gain if N * Ho * Wo == 2 else 1e-5


# ---- the stand-alone depthwise op (depthwise_relu): N, C, H, W, ks, stride, pad, dil ---------------------------------------
DW_ROWS = [
    (3, 12, 9, 7, 3, 2, 2, 2),                    # narrow C (one partial channel slice), stride 2, dilation 2
    (2, 516, 3, 3, 3, 1, 1, 1),                   # nq = 129: five channel slices of the forward, one pixel lane of the weight gradient
    (2, 1028, 2, 2, 3, 1, 1, 1),                  # nq = 257: a second channel slice of the weight gradient, with one quad
    (1, 2052, 1, 1, 7, 1, 3, 1),                  # 1 x 1 images: 48 of 49 taps are padding; four tap groups
    (1, 16384, 2, 2, 5, 2, 2, 1),                 # the widest C; one output pixel
]

# ---- squeeze-and-excitation through `ChannelSELayer` (J = C // 2): N, C, H, W, stride -------------------------------------
SE_ROWS = [
    (2, 1028, 1, 1, 1),                           # nq = 257: the first width on the looping pixel sums
    (2, 2048, 2, 2, 1),
    (1, 4096, 1, 1, 2),                           # the widest layer; stride 2 slicing
]


def conv_inputs(row, member):
    """(x, w, gamma, beta, upstream gradient, running mean, running var) of a CONV row for the member 'norm' / 'none' /
    'frozen'; the running statistics (used by 'frozen' alone) are drawn after everything else."""
    x, w, gamma, beta, up = E.conv_inputs(row, CONV_SEED[member])
    g = torch.Generator().manual_seed(sum(row[:5]) + 77)
    Co = row[2]
    return x, w, gamma, beta, up, 0.5 * torch.randn(Co, generator=g), 0.5 + 1.5 * torch.rand(Co, generator=g)


def dw_inputs(row):
    """(x, w_dw, upstream gradient) of a DW row."""
    N, C, H, W, ks, st, pad, dil = row
    g = torch.Generator().manual_seed(sum(row))
    x = torch.randn(N, C, H, W, generator=g)
    w_dw = torch.randn(C, 1, ks, ks, generator=g) / ks
    up = torch.randn(N, C, *E.conv_out_hw(H, W, (ks, ks), (st, st), (pad, pad), dil), generator=g)
    return x, w_dw, up


# ---- module level: name -> (constructor, arguments, input channels) -- 2 x C x 4 x 4 inputs --------------------------------
MODULES = {
    'sep_conv_520': ('SepConv', (520, 520, 3, 1, 1), 520),
    'dil_conv_12_1028': ('DilConv', (12, 1028, 3, 2, 2, 2), 12),
    'conv_1x1_1028_516': ('ReLUConvBN', (1028, 516, 1), 1028),
}
