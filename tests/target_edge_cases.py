"""Edge shapes of the target-network HIP ops (ghn3_amd/csrc/target_ops.hip): the smallest inputs that still reach a branch the
training shapes of tests/test_gpu_target_ops.py leave untouched.  Plain tuples plus the seeded inputs made from them, shared by
tests/test_target_edges_cpu.py (the rows are well conditioned: stock fp32 against fp64) and tests/test_gpu_target_edges.py (the
kernels against fp64).

Every row with a norm layer keeps the smallest per-channel batch variance of the pre-norm result at or above VAR_FLOOR in the
fp64 reference: below it BatchNorm amplifies harmless rounding of the convolution result by |z| / sigma and the comparison would
judge the conditioning of the row, not the kernel.  The seeds follow the formulas of tests/test_gpu_target_ops.py; where the
floor did not hold, N was raised (written in the row).  That cannot help on a 1 x 1 image: every tap but the centre reads
padding, so a weight drawn at 1 / sqrt(fan-in) gives a result sqrt(taps) smaller than on a real image -- expected variance
0.34 / 9 = 0.038 for 3 x 3 taps behind a ReLU, below the floor for any N and seed.  The `gain` column multiplies the convolution
(depthwise) weight for that reason alone; gain = sqrt(taps) restores the usual scale, and is 1 everywhere else.

The rows stay below 0.6 M activations per tensor, with one exception: the last two dense rows (0.59 M and 1.1 M).  conv2_nt
leaves NT = 2 unless 64-pixel tiles x column groups reach 256, so NT = 4 needs 16 321 pixels and NT = 8 as many with more than
64 columns; 1 x 1 kernels keep these rows as cheap as the rest (tens of milliseconds each).
"""
import torch

VAR_FLOOR = 0.05
T, F = True, False

# ---- dense convolution (conv_bn, conv_only): N, C_in, C_out, H, W, (kh, kw), (sh, sw), (ph, pw), dil, relu, gain ------------
CONV_ROWS = [
    # both channel counts = 4 mod 8 (the half-vector arms of conv_in8, dz_in8 and both directions of tnet_conv2_kernel); one
    # partial K chunk; P = 50: a single, partial pixel tile
    (2, 12, 20, 5, 5, (3, 3), (1, 1), (1, 1), 1, T, 1.0),
    # 1 x 1 images: every tap but the centre is padding; P = 16 < 32 is less than one step of the weight gradient (w_chunks = 1)
    (16, 36, 44, 1, 1, (3, 3), (1, 1), (1, 1), 1, T, 3.0),
    # just over the 64 and the 128 column boundaries: the last blockIdx.y group of either direction holds 4 columns; P = 24
    (6, 68, 132, 3, 3, (3, 3), (2, 2), (1, 1), 1, T, 1.0),
    # stride 2 together with dilation 2
    (3, 20, 28, 9, 7, (3, 3), (2, 2), (2, 2), 2, T, 1.0),
    # dilation with kh != kw; more padding than the image edge needs (whole output rows / columns read padding only at some taps)
    (2, 16, 24, 6, 6, (3, 5), (1, 1), (3, 4), 2, F, 1.0),
    # a stride larger than the kernel: input pixels no output reads, dx exactly 0 there; P = 8
    (2, 8, 8, 4, 4, (1, 1), (3, 3), (0, 0), 1, T, 1.0),
    # the narrowest channels, 49 taps, no ReLU
    (2, 4, 4, 7, 7, (7, 7), (1, 1), (3, 3), 1, F, 1.0),
    # wide C_in (33 chunks, a 4-channel tail), 1 x 1; P = 8
    (2, 1028, 8, 2, 2, (1, 1), (1, 1), (0, 0), 1, T, 1.0),
    # wide C_in with k > 1
    (2, 516, 12, 3, 3, (3, 3), (1, 1), (1, 1), 1, T, 1.0),
    # P = 66: one full tile plus a 2-pixel tile (cnt = 2 in the per-tile mean / M2); a tile spans 32 samples
    (33, 8, 12, 1, 2, (1, 1), (1, 1), (0, 0), 1, T, 1.0),
    # just over the 256 column boundary: nine column groups, the last one with 4 columns; P = 32
    (2, 12, 260, 4, 4, (3, 3), (1, 1), (1, 1), 1, T, 1.0),
    # 256 pixel tiles: conv2_nt keeps 4 fragments per workgroup (every smaller image runs on 2), both directions
    (1, 36, 36, 128, 128, (1, 1), (1, 1), (0, 0), 1, T, 1.0),
    # ... and 8 fragments, the instantiation of the wide layers at training batch sizes (needs 256 tiles x more than 64 columns)
    (1, 68, 68, 128, 128, (1, 1), (1, 1), (0, 0), 1, T, 1.0),
]
# conv_only draws its inputs from another seed than conv_bn does (3 + ..., as test_conv_without_a_norm_layer)
CONV_ONLY_SEED = 3
# conv_only alone: one output pixel (F.batch_norm refuses P = 1 in training mode, so no norm row can have it)
CONV_ONLY_ROWS = CONV_ROWS + [
    (1, 12, 20, 3, 3, (3, 3), (1, 1), (0, 0), 1, T, 1.0),
]
# conv_bn with one output channel's weights set to zero: (row, channel) -- channel 19 sits in the 4-channel tail group
CONV_DEAD = (CONV_ROWS[0], 19)

# ---- ReLU -> depthwise -> pointwise -> norm (dwpw_bn): N, C_in, C_out, H, W, ks, stride, pad, dil, gain (on w_dw) -----------
DWPW_ROWS = [
    (2, 12, 20, 5, 5, 3, 1, 1, 1, 1.0),        # both channel counts = 4 mod 8 (dw_taps8 `second`, dz8's break); P = 50
    (16, 36, 44, 1, 1, 3, 1, 1, 1, 3.0),       # 1 x 1 images, 3 x 3 taps; P = 16 < 32
    (16, 20, 28, 1, 1, 5, 1, 2, 1, 5.0),       # 1 x 1 images, 5 x 5 taps
    (16, 12, 68, 1, 1, 7, 1, 3, 1, 7.0),       # 1 x 1 images, 7 x 7 taps; C_out just over 64 (nt_of -> 8)
    (3, 20, 132, 9, 7, 3, 2, 2, 2, 1.0),       # stride 2 with dilation 2; C_out just over 128 (nt_of -> 16); P = 60
    (2, 12, 260, 4, 4, 3, 1, 1, 1, 1.0),       # C_out just over 256: nt_of -> 32, the two-term products; P = 32
    (3, 36, 512, 3, 3, 3, 1, 1, 1, 1.0),       # the widest output, two-term products; P = 27
    (2, 68, 12, 3, 3, 3, 1, 1, 1, 1.0),        # C_in just over 64: nt_of(C_in) -> 8 in the data gradient, a second ci block
    (2, 132, 20, 3, 3, 3, 1, 1, 1, 1.0),       # C_in just over 128
    (2, 260, 12, 3, 3, 3, 1, 1, 1, 1.0),       # C_in just over 256: two-term products in the data gradient
]
# the same op without a depthwise stage (w_dw = None): N, C_in, C_out, H, W, stride
PW_ROWS = [
    (2, 12, 20, 5, 5, 1),                         # channel tails; P = 50
    (16, 36, 44, 1, 1, 1),                        # 1 x 1 images; P = 16 < 32
    (3, 20, 28, 5, 5, 2),                         # stride 2; P = 27
]
DWPW_DEAD = (DWPW_ROWS[0], 19)

# ---- squeeze-and-excitation through `ChannelSELayer` (J = C // 2): N, C, H, W, stride ----------------------------------------
SE_ROWS = [
    (2, 1024, 1, 1, 1),                           # the widest layer: nq = 256, one pixel lane in se_pixel_sum; HW = 1
    (3, 516, 3, 3, 2),                            # nq = 129: 127 idle threads beside one pixel lane; stride slicing
    (2, 1020, 2, 2, 1),                           # nq = 255: the last thread falls outside the only pixel lane
    (1, 4, 5, 5, 1),                              # one channel quad, 256 pixel lanes for 25 pixels; J = 2
]

# ---- pooling through light_ops on relu(randn) input (ties): N, C, H, W, k, stride, pad ---------------------------------------
POOL_ROWS = [
    (2, 4, 1, 1, 3, 1, 1),                        # H + 2 pad == k: a single output, eight of nine taps are padding; C = 4
    (2, 8, 2, 2, 4, 1, 1),                        # H + 2 pad == k with an even window
    (3, 12, 7, 5, 2, 2, 0),                       # k = 2, stride 2 on an odd-sized image: the last row / column is never read
    (2, 20, 6, 6, 3, 2, 1),                       # the stems' MaxPool2d(3, 2, 1) on an even image
    (1, 4, 9, 9, 3, 1, 1),                        # overlapping windows: a zero that wins several windows
]


def conv_out_hw(H, W, k, st, pad, dil):
    return (H + 2 * pad[0] - dil * (k[0] - 1) - 1) // st[0] + 1, (W + 2 * pad[1] - dil * (k[1] - 1) - 1) // st[1] + 1


def conv_inputs(row, seed_extra=0):
    """(x, w, gamma, beta, upstream gradient) of a CONV row, fp32 on the CPU; the seed formula of test_gpu_target_ops.py."""
    N, Ci, Co, H, W, k, st, pad, dil, relu, gain = row
    g = torch.Generator().manual_seed(N + Ci + Co + H + W + sum(k) + sum(st) + seed_extra)
    x = torch.randn(N, Ci, H, W, generator=g)
    w = gain * torch.randn(Co, Ci, k[0], k[1], generator=g) / (Ci * k[0] * k[1]) ** 0.5
    gamma = 1 + 0.3 * torch.randn(Co, generator=g)
    beta = 0.2 * torch.randn(Co, generator=g)
    up = torch.randn(N, Co, *conv_out_hw(H, W, k, st, pad, dil), generator=g)
    return x, w, gamma, beta, up


def dwpw_inputs(row):
    """(x, w_dw, w_pw, gamma, beta, upstream gradient) of a DWPW row."""
    N, Ci, Co, H, W, ks, st, pad, dil, gain = row
    g = torch.Generator().manual_seed(sum(row[:9]))
    x = torch.randn(N, Ci, H, W, generator=g)
    w_dw = gain * torch.randn(Ci, 1, ks, ks, generator=g) / ks
    w_pw = torch.randn(Co, Ci, 1, 1, generator=g) / Ci ** 0.5
    gamma = 1 + 0.3 * torch.randn(Co, generator=g)
    beta = 0.2 * torch.randn(Co, generator=g)
    up = torch.randn(N, Co, *conv_out_hw(H, W, (ks, ks), (st, st), (pad, pad), dil), generator=g)
    return x, w_dw, w_pw, gamma, beta, up


def pw_inputs(row):
    """(x, w_pw, gamma, beta, upstream gradient) of a PW row."""
    N, Ci, Co, H, W, st = row
    g = torch.Generator().manual_seed(sum(row))
    x = torch.randn(N, Ci, H, W, generator=g)
    w_pw = torch.randn(Co, Ci, 1, 1, generator=g) / Ci ** 0.5
    gamma = 1 + 0.3 * torch.randn(Co, generator=g)
    beta = 0.2 * torch.randn(Co, generator=g)
    up = torch.randn(N, Co, (H - 1) // st + 1, (W - 1) // st + 1, generator=g)
    return x, w_pw, gamma, beta, up


def se_inputs(row):
    """(x, upstream gradient) of an SE row; the module's own parameters come from torch.manual_seed(C + H), times 3 (gates on
    both sides of the hard-swish knees) as in test_gpu_target_ops.py."""
    N, C, H, W, stride = row
    g = torch.Generator().manual_seed(sum(row))
    x = torch.randn(N, C, H, W, generator=g) * 2
    up = torch.randn(N, C, (H - 1) // stride + 1, (W - 1) // stride + 1, generator=g)
    return x, up


def pool_inputs(row, mode):
    """(x, upstream gradient) of a POOL row: relu(randn), i.e. about half of the input exact zeros -- most max windows tie."""
    N, C, H, W, k, s, pad = row
    g = torch.Generator().manual_seed(sum(row) + mode)
    x = torch.relu(torch.randn(N, C, H, W, generator=g))
    up = torch.randn(N, C, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1, generator=g)
    return x, up


# the slicings of tests/util_parity.slice_errors
ACT_AXES = [(1,), (2, 3), (0,)]                   # activations and dx (N, C, H, W): per channel, per position, per sample
WGRAD_AXES = [(0,), (1,), (2, 3)]                 # convolution weight gradients: per C_out, per C_in, per tap
VEC_AXES = [(0,)]                                 # per-channel vectors: per element
MAT_AXES = [(0,), (1,)]                           # Linear weights: per row, per column
