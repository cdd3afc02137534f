"""
Cases and the float64 reference of the lean attention of the target networks' msa layers (ghn3_attn_lean_fwd / _bwd,
ghn3_amd/csrc/tnet_attn.hip; target_ops.LeanAttention), shared by test_msa_lean_cpu.py and test_gpu_target_msa_lean.py.

Inputs: q, k, v and dO are seeded standard normals, rounded to float32 (the device gets exactly these values) and referenced
in float64.  "Ramp" cases (r > 0) also scale key j by 0.25 + r j / (N - 1) and q by 3: the row maximum then moves from key
tile to key tile for about half the rows and max |scale S| reaches ~ 80 - 140, so the forward's running-maximum rescale is
taken with factors far from 1 -- bounded random data never does that.

The reference is written in the form the kernels use (lse per query row, P = exp(scale S - lse), delta = rowsum(dO . O)),
in numpy float64; test_msa_lean_cpu.py holds it against torch float64 autograd of softmax attention.
"""
import functools

import numpy as np

# (B, heads, N, d, r)
OP_CASES = [
    (2, 8, 1, 8, 0),          # a single token
    (2, 8, 33, 6, 0),         # d % 4 != 0; one key past a tile
    (2, 8, 49, 8, 0),         # 49 tokens, two key tiles (49 = 32 + 17)
    (1, 8, 121, 16, 0),       # 121 tokens, four key tiles (121 = 3 x 32 + 25)
    (1, 8, 129, 8, 6),        # five key tiles on four waves: a second round
    (1, 8, 129, 32, 6),       # the widest head
    (1, 8, 257, 24, 10),      # ramp with 24-wide heads over nine key tiles
    (1, 8, 1024, 4, 4),       # the narrowest head, 32 tiles
    (1, 2, 1089, 8, 6),       # past 1024
    (16, 8, 4096, 4, 0),      # B heads N^2 = 2^31: the new ground
]
LARGEST = OP_CASES[-1]

OUT_TOL, GRAD_TOL = 2e-5, 1e-4           # relative L2: outputs (lse is one), gradients

# the shapes of the existing msa layer test (tests/test_gpu_target_msa.py CASES), restated: B, C, H, W, stride
LAYER_SHAPES = [(64, 32, 11, 11, 1), (64, 64, 11, 11, 1), (64, 128, 11, 11, 1), (8, 128, 14, 14, 1), (4, 256, 7, 7, 2),
                (3, 48, 5, 7, 2), (2, 64, 1, 1, 1), (6, 64, 8, 8, 1), (5, 32, 9, 9, 1)]
HEADS = 8                                # ops._TransformerLayer


def ref_slices(case):
    """The (b, head) slices a case is referenced on: all of them, except for the largest case (first, middle, last: all-slice
    float64 would take a minute on the host, and a slice's outputs and gradients depend on that slice alone)."""
    B, H, N, d, r = case
    if case == LARGEST:
        return [(0, 0), (B // 2, H // 2), (B - 1, H - 1)]
    return [(b, h) for b in range(B) for h in range(H)]


@functools.lru_cache(maxsize=None)
def inputs(case):
    """q, k, v, dO as float32 arrays (B, heads, N, d)."""
    B, H, N, d, r = case
    rng = np.random.default_rng(1000 + 7 * OP_CASES.index(case))
    q, k, v, g = (rng.standard_normal((B, H, N, d)).astype(np.float32) for _ in range(4))
    if r:
        ramp = (0.25 + r * np.arange(N, dtype=np.float64) / max(N - 1, 1)).astype(np.float32)
        k = (k * ramp[None, None, :, None]).astype(np.float32)
        q = (q * np.float32(3)).astype(np.float32)
    for a in (q, k, v, g):
        a.setflags(write=False)
    return q, k, v, g


def pack_qkv(q, k, v):
    """(B, heads, N, d) x 3 -> qkv (B, N, 3 C): columns q | k | v, head h at columns h d .. h d + d - 1 of each."""
    B, H, N, d = q.shape
    t = [a.transpose(0, 2, 1, 3).reshape(B, N, H * d) for a in (q, k, v)]
    return np.ascontiguousarray(np.concatenate(t, axis=2))


def pack_heads(a):
    """(B, heads, N, d) -> (B, N, C)"""
    B, H, N, d = a.shape
    return a.transpose(0, 2, 1, 3).reshape(B, N, H * d).copy()           # (a copy: the inputs are read-only)


def attention_ref(q, k, v, g, dtype=np.float64):
    """One (b, head) slice, (N, d) each, in `dtype`: out, lse, dq, dk, dv in the kernels' formulation."""
    q, k, v, g = (a.astype(dtype) for a in (q, k, v, g))
    scale = dtype(1.0) / np.sqrt(dtype(q.shape[1]))
    S = (q @ k.T) * scale
    m = S.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(S - m).sum(axis=1, keepdims=True, dtype=dtype))).astype(dtype)
    P = np.exp(S - lse)
    out = P @ v
    delta = (g * out).sum(axis=1, keepdims=True, dtype=dtype)
    dS = P * (g @ v.T - delta)
    return out, lse[:, 0], (dS @ k) * scale, (dS.T @ q) * scale, P.T @ g


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


def rel_l2(got, ref):
    """Relative L2 error over a list of (got, ref) slice pairs taken as one tensor."""
    num = sum(float(((np.asarray(a, dtype=np.float64) - b) ** 2).sum()) for a, b in zip(got, ref))
    den = sum(float((b ** 2).sum()) for b in ref)
    return float(np.sqrt(num / den)) if den > 0 else float(np.sqrt(num))


def worst_block(got, ref, block=32):
    """The largest error of a (b, head, 32-row block) slice, divided by the RMS of the whole (referenced) tensor times
    sqrt(slice size): a relative error per slice on the tensor's own scale, which one wrong tile cannot hide in."""
    den = sum(float((b ** 2).sum()) for b in ref)
    cnt = sum(b.size for b in ref)
    rms = np.sqrt(den / cnt) if den > 0 else 1.0
    worst = 0.0
    for a, b in zip(got, ref):
        a = np.asarray(a, dtype=np.float64)
        for i in range(0, b.shape[0], block):
            e = a[i:i + block] - b[i:i + block]
            worst = max(worst, float(np.sqrt((e ** 2).sum())) / (rms * np.sqrt(e.size)))
    return worst
