"""Rows of the patch-embedding op (ghn3_patch_fwd / _bwd, target_ops.PatchEmbed), shared by tests/test_patch_cpu.py and
tests/test_gpu_target_patch.py: the smallest shapes at which the kernels can go wrong, and the descriptors the op refuses."""
import torch

# N, C_in, H, W, (kh, kw), (sh, sw), C_out, channels_last storage of x
ROWS = [
    (2, 3, 32, 32, (16, 16), (16, 16), 8, False),      # P = 8 output pixels: fewer than one MFMA row tile
    (65, 3, 16, 16, (16, 16), (16, 16), 12, False),    # P = 65: one pixel past a 64-pixel tile
    (1, 3, 48, 40, (16, 16), (16, 16), 68, False),     # eight trailing columns no window reaches; column tail of 4
    (2, 3, 27, 42, (9, 9), (9, 9), 132, False),        # K = 243, no multiple of 32; 9-float runs; W no multiple of 4
    (2, 4, 32, 48, (8, 16), (8, 16), 260, True),       # kh != kw; four channels in channels_last storage; 260 columns
    (1, 3, 64, 64, (32, 32), (32, 32), 16, False),     # K = 3072, the longest reduction
    (3, 3, 40, 40, (16, 16), (20, 20), 20, False),     # stride larger than the kernel: dx exactly 0 between windows
    (1, 1, 8, 8, (8, 8), (8, 8), 4, False),            # one pixel, one channel
]
# a row whose weight has a zero output channel (its index): z and that channel's dw are exactly 0 there
DEAD = ((2, 3, 32, 32, (16, 16), (16, 16), 8, False), 5)

# what the size query refuses with GHN3_E_LIMIT (-2), and PatchEmbed.applicable with it: name -> N, C_in, H, W, k, stride, C_out
REFUSED = {
    'kh = 33': (1, 3, 66, 64, (33, 16), (33, 16), 8),
    'max(kh, kw) = 7': (1, 3, 28, 28, (7, 7), (7, 7), 8),
    'C_in = 5': (1, 5, 32, 32, (16, 16), (16, 16), 8),
    'C_out = 6': (1, 3, 32, 32, (16, 16), (16, 16), 6),
    'C_out = 4100': (1, 3, 32, 32, (16, 16), (16, 16), 4100),
    'a stride below the kernel': (1, 3, 32, 32, (16, 16), (16, 8), 8),
    '2^31 elements': (2731, 3, 512, 512, (16, 16), (16, 16), 8),
}
# inside the limits, at their edges
TAKEN = [(1, 4, 32, 32, (32, 32), (32, 32), 4096), (1, 3, 9, 40, (1, 8), (9, 8), 4), (2730, 3, 512, 512, (16, 16), (16, 16), 8)]


def out_hw(H, W, k, st):
    return (H - k[0]) // st[0] + 1, (W - k[1]) // st[1] + 1


def covered(row):
    """(H, W) mask of the pixels some window reads."""
    N, Ci, H, W, k, st, Co = row[:7]
    Ho, Wo = out_hw(H, W, k, st)
    m = torch.zeros(H, W, dtype=torch.bool)
    for oh in range(Ho):
        for ow in range(Wo):
            m[oh * st[0]:oh * st[0] + k[0], ow * st[1]:ow * st[1] + k[1]] = True
    return m


def inputs(row, dead=None):
    """(x, w, up): randn images, randn / sqrt(K) weights, randn upstream gradient; seeded by the row."""
    N, Ci, H, W, k, st, Co, cl = row
    gen = torch.Generator().manual_seed(1000 + 7 * N + 13 * Co + H)
    x = torch.randn(N, Ci, H, W, generator=gen)
    w = torch.randn(Co, Ci, *k, generator=gen) / float(Ci * k[0] * k[1]) ** 0.5
    if dead is not None:
        w[dead] = 0
    up = torch.randn(N, Co, *out_hw(H, W, k, st), generator=gen)
    return x, w, up
