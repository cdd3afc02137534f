"""
bf16 optimizer state with stochastic rounding (FusedAdamW(state_dtype='bf16'), GHN3_OP_ADAMW_S16 / _S16_CAST16), checked
without a GPU on the host restatement of the rule, ghn3_amd.optim.adamw_state16_reference_ (the GPU tests compare the
kernels against it bit for bit):

  * the header declares the two op kinds with the loader's numbers, the kind count moved with them, the ABI version did not;
  * the rounding is unbiased: over 2^20 seeded normals the mean of (stored - exact) / ulp stays within 5 sigma =
    5 sqrt(1 / 6 / n) = 0.002 (a fraction f of an ulp goes up with probability f: variance f (1 - f), 1 / 6 on average), and
    every stored value is one of the two bf16 neighbours of the exact one;
  * round-to-nearest storage stalls exp_avg_sq (why it is not offered), stochastic storage does not: 4096 elements,
    gradients 1e-3 U(0.5, 1.5), beta2 = 0.999, 2000 steps.  Measured with the shipped hash: median ratio to the exact EMA
    0.9994, mean 0.9992, standard deviation 0.0236, worst element within 0.090 (bounds: 1 % and 0.15); RNE ends at a median
    of 0.30.  The spread is the rounding's own, not the hash's: with numpy's PCG64 as the source of the 16 bits the same
    recurrence gives a standard deviation of 0.0233 .. 0.0237 and a worst element of 0.083 .. 0.096 over six seeds (the hash:
    0.0231 .. 0.0237 and 0.081 .. 0.100) -- the worst of 4096 elements sits near 4 sigma, so no generator brings it under
    half the 0.15 cap (6.4 sigma), and the test also holds the standard deviation to the ideal generator's + 10 %;
  * the result does not depend on how the flat buffer is split into launches.
"""
import os
import re

import numpy as np
import pytest
import torch

from ghn3_amd import _lib as L
from ghn3_amd import optim as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=0.0, inv_scale=1.0)


def _bits(t):
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def test_the_two_kinds_are_declared_with_the_loaders_numbers():
    header = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    for name, num in (('GHN3_OP_ADAMW_S16', L.OP_ADAMW_S16), ('GHN3_OP_ADAMW_S16_CAST16', L.OP_ADAMW_S16_CAST16)):
        m = re.search(r'\b%s\s*=\s*(\d+)\s*,' % name, header)
        assert m and int(m.group(1)) == num, (name, num)
    assert (L.OP_ADAMW_S16, L.OP_ADAMW_S16_CAST16) == (L.OP_ADAMW_CAST16 + 1, L.OP_ADAMW_CAST16 + 2)
    assert re.search(r'GHN3_OP_ADAMW_S16_CAST16\s*=\s*\d+\s*,\s*GHN3_OP_KIND_COUNT\b', header)
    assert L.OP_KIND_COUNT == L.OP_ADAMW_S16_CAST16 + 1 == len(L.OP_NAMES)
    assert L.OP_NAMES[L.OP_ADAMW_S16] == 'adamw_s16' and L.OP_NAMES[L.OP_ADAMW_S16_CAST16] == 'adamw_s16_cast16'
    assert L.ABI_VERSION == 21 and re.search(r'#define\s+GHN3_ABI_VERSION\s+21\b', header)


def test_the_constructor_refuses_other_state_types_and_seeds():
    from ghn3_amd import FusedAdamW
    with pytest.raises(ValueError):
        FusedAdamW(None, state_dtype='fp16')
    with pytest.raises(ValueError):
        FusedAdamW(None, state_dtype='bf16', state_seed=1 << 24)


def test_the_rounding_is_unbiased_and_picks_a_neighbour():
    n = 1 << 20
    x = torch.from_numpy(np.random.default_rng(5).standard_normal(n).astype(np.float32))
    p = torch.zeros(n)
    m = torch.zeros(n, dtype=torch.bfloat16)
    v = torch.zeros(n, dtype=torch.bfloat16)
    # beta1 = beta2 = 0, no clipping: the new moments are exactly x and x * x
    O.adamw_state16_reference_(p, x.clone(), m, v, None, 1, 1e-3, (0.0, 0.0), 1e-8, 0.0, 0.0, 1.0, seed=3, base=12345)
    bound = 5.0 * (1.0 / 6.0 / n) ** 0.5
    assert bound < 0.002
    for exact, stored in ((x.numpy(), m), (x.numpy() * x.numpy(), v)):
        u = exact.view(np.uint32)
        lo = (u >> 16).astype(np.uint16)                  # the neighbour towards zero; the other one is one pattern up
        sb = _bits(stored)
        assert np.all((sb == lo) | (sb == lo + np.uint16(1)))
        ulp = np.ldexp(1.0, (((u >> 23) & 0xff).astype(np.int64) - 127 - 7))
        err = (stored.double().numpy() - exact.astype(np.float64)) / ulp
        assert np.abs(err).max() < 1.0
        assert abs(err.mean()) < bound, err.mean()
        assert abs((err * np.sign(exact)).mean()) < bound      # (in magnitude: neither sign is favoured)
        assert 0.3 < (sb != lo).mean() < 0.7                    # (both neighbours are taken)
        rep = (u & 0xffff) == 0
        assert np.array_equal(sb[rep], lo[rep])                 # (a representable value is stored as it is)


def _stall_case():
    rng = np.random.default_rng(11)
    g = (1e-3 * rng.uniform(0.5, 1.5, 4096)).astype(np.float32)
    exact = g.astype(np.float64) ** 2 * (1.0 - 0.999 ** 2000)
    return g, exact


def test_round_to_nearest_stalls_exp_avg_sq():
    g, exact = _stall_case()
    b2 = np.float32(0.999)
    add = ((np.float32(1) - b2) * g) * g
    v = torch.zeros(4096, dtype=torch.bfloat16)
    for _ in range(2000):
        v = torch.from_numpy(b2 * v.float().numpy() + add).to(torch.bfloat16)      # (round to nearest even)
    ratio = np.median(v.double().numpy() / exact)
    print('RNE: median v / exact = %.4f' % ratio)
    assert ratio < 0.5, ratio


def test_stochastic_storage_follows_the_exact_average():
    g, exact = _stall_case()
    gt = torch.from_numpy(g)
    p = torch.zeros(4096)
    m = torch.zeros(4096, dtype=torch.bfloat16)
    v = torch.zeros(4096, dtype=torch.bfloat16)
    for t in range(1, 2001):
        O.adamw_state16_reference_(p, gt, m, v, None, t, 0.0, (0.9, 0.999), 1e-8, 0.0, 0.0, 1.0, seed=0, base=0)
    ratio = v.double().numpy() / exact
    print('stochastic: median %.4f mean %.4f std %.4f worst %.4f' % (np.median(ratio), ratio.mean(), ratio.std(),
                                                                  np.abs(ratio - 1).max()))
    assert abs(np.median(ratio) - 1.0) < 0.01
    assert np.abs(ratio - 1.0).max() < 0.15
    assert ratio.std() < 0.026                                     # (an ideal generator: 0.0233 .. 0.0237, see above)
    assert np.abs(m.double().numpy() / g - 1.0).max() < 0.01      # (exp_avg of a constant gradient: within two bf16 ulps)


def test_the_result_does_not_depend_on_the_partition():
    n = 1000
    rng = np.random.default_rng(2)
    state = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)),
             torch.from_numpy((1e-2 * rng.standard_normal(n)).astype(np.float32)),
             torch.from_numpy((1e-2 * rng.standard_normal(n)).astype(np.float32)).to(torch.bfloat16),
             torch.from_numpy((1e-4 * rng.random(n)).astype(np.float32)).to(torch.bfloat16)]
    hyper = dict(HYPER, max_norm=0.05)
    sumsq = float((state[1].double() ** 2).sum())
    one = [t.clone() for t in state]
    O.adamw_state16_reference_(*one, sumsq, 7, seed=9, base=64, **hyper)
    three = [t.clone() for t in state]
    for lo, hi in ((0, 300), (300, 301), (301, n)):
        O.adamw_state16_reference_(*[t[lo:hi] for t in three], sumsq, 7, seed=9, base=64 + lo, **hyper)
    assert torch.equal(one[0], three[0]) and not torch.equal(one[0], state[0])
    assert np.array_equal(_bits(one[2]), _bits(three[2])) and np.array_equal(_bits(one[3]), _bits(three[3]))
    # other steps and seeds draw other bits
    for kw in (dict(step=8, seed=9), dict(step=7, seed=10)):
        other = [t.clone() for t in state]
        O.adamw_state16_reference_(*other, sumsq, kw['step'], seed=kw['seed'], base=64,
                                   **dict(hyper, betas=(0.9, 0.999)))
        assert not np.array_equal(_bits(other[3]), _bits(one[3]))
    # and the update is AdamW's: from the same (widened) state the fp32 restatement gives the same parameters
    ref = [state[0].clone(), state[1].clone(), state[2].float(), state[3].float()]
    O.adamw_reference_(*ref, sumsq, 7, **hyper)
    assert float((ref[0] - one[0]).abs().max()) < 1e-6
    err_m = (one[2].float() - ref[2]).abs() / ref[2].abs().clamp_min(1e-30)
    assert float(err_m.max()) < 2.0 ** -7                          # (one bf16 ulp)
    # a non-finite norm leaves everything as it was
    kept = [t.clone() for t in state]
    O.adamw_state16_reference_(*kept, float('nan'), 7, seed=9, base=64, **hyper)
    assert all(torch.equal(a.float(), b.float()) for a, b in zip(kept, state))
