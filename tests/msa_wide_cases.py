"""
Cases of the wide msa path (ghn3_attn_wide_* / ghn3_msa_wide_*, ghn3_amd/csrc/tnet_msa_wide.hip; target_ops.WideAttention and
MsaWideLayer), shared by test_msa_wide_cpu.py and test_gpu_target_msa_wide.py.  The float64 attention reference, the packing of
qkv, the error measures and the tolerances are those of msa_lean_cases.py: the kernels are exact fp32 products with fp32
accumulation in another summation order than the reference's, as the lean ones.
"""
import functools

import numpy as np

from msa_lean_cases import GRAD_TOL, OUT_TOL, attention_ref, pack_heads, pack_qkv, rel_l2, worst_block  # noqa: F401

# (B, heads, N, d, ramp): head dims above 32; "ramp" as in msa_lean_cases (keys scaled by 0.25 + r j / (N - 1), q by 3)
OP_CASES = [
    (2, 2, 1, 64, 0),         # a single token
    (2, 4, 49, 33, 0),        # d % 4 != 0, one column into the second half; two key tiles
    (2, 2, 33, 40, 0),        # one key past a tile
    (1, 2, 129, 64, 6),       # the widest head; five key tiles on four waves: a second round
    (1, 2, 257, 48, 10),      # ramp over nine key tiles
    (1, 1, 1089, 36, 6),      # past 1024
    (2, 2, 4096, 64, 0),      # the longest sequence at the widest head
]
LARGEST = OP_CASES[-1]

# the lean kernels behind the wide entry points: (B, heads, N, d) at which both must agree bit for bit
LEAN_EQUAL = [(1, 8, 129, 6), (1, 8, 129, 32)]

# B, C, heads, H, W, stride, channels_last, mlp_ratio, qkv_bias
LAYER_CASES = [
    (2, 512, 8, 4, 4, 1, False, 1, False),
    (3, 264, 8, 5, 7, 2, True, 1, False),        # d = 33, odd grid, stride 2
    (2, 40, 1, 6, 6, 1, False, 1, False),        # one head of 40
    (2, 64, 1, 3, 3, 1, True, 36, False),        # hidden = 2304 on narrow rows
    (2, 1024, 16, 4, 4, 1, False, 4, True),      # the limits: C = 1024, d = 64, hidden = 4096; QKV bias
    (2, 512, 8, 1, 1, 1, False, 1, False),       # a single token
    (1, 768, 12, 14, 14, 1, True, 4, False),     # a ViT-B block
]

# descriptors ghn3_msa_wide_scratch_floats refuses with GHN3_E_LIMIT
REFUSED = [
    dict(B=2, C=1028, H=4, W=4, heads=4),        # C above 1024
    dict(B=2, C=520, H=4, W=4, heads=8),         # head dim 65
    dict(B=2, C=64, H=4, W=4, hidden=4100),      # hidden above 4096
    dict(B=1, C=64, H=65, W=64),                 # 4160 tokens
    dict(B=2, C=60, H=4, W=4, heads=8),          # C not a multiple of heads
]


def ref_slices(case):
    """The (b, head) slices a case is referenced on: all of them, except for the largest case (three: float64 of all four
    4096 x 4096 slices would take most of a minute on the host, and a slice depends on itself alone)."""
    B, H, N, d, r = case
    if case == LARGEST:
        return [(0, 0), (B // 2, H // 2), (B - 1, H - 1)]
    return [(b, h) for b in range(B) for h in range(H)]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """q, k, v, dO as float32 arrays (B, heads, N, d)."""
    B, H, N, d, r = case
    rng = np.random.default_rng(2000 + 7 * OP_CASES.index(case))
    q, k, v, g = (rng.standard_normal((B, H, N, d)).astype(np.float32) for _ in range(4))
    if r:
        ramp = (0.25 + r * np.arange(N, dtype=np.float64) / max(N - 1, 1)).astype(np.float32)
        k = (k * ramp[None, None, :, None]).astype(np.float32)
        q = (q * np.float32(3)).astype(np.float32)
    for a in (q, k, v, g):
        a.setflags(write=False)
    return q, k, v, g


@functools.lru_cache(maxsize=None)
def reference(case):
    """{(b, head): (out, lse, dq, dk, dv)} in float64 over ref_slices(case); computed once, never modified."""
    q, k, v, g = inputs(case)
    res = {}
    for (b, h) in ref_slices(case):
        t = attention_ref(q[b, h], k[b, h], v[b, h], g[b, h])
        for a in t:
            a.setflags(write=False)
        res[(b, h)] = t
    return res
