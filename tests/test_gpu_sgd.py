"""GPU tests of the multi-tensor SGD step (csrc/tnet_sgd.hip through ghn3_amd.optim.FusedSGD) against float64
clip_grad_norm_ + torch.optim.SGD on the CPU.

The error metric is the relative L2 distance over the CONCATENATION of all parameters (and of all momentum buffers), not per
tensor: a one-element tensor whose updates cancel shows 4.5e-6 for stock fp32 torch against float64, which says nothing about a
kernel.  Two bounds, both asserted: 3e-6 (the gate of the fused AdamW, test_gpu_parity.py), and 4 x the error stock fp32
torch.optim.SGD + clip_grad_norm_ on the GPU shows against the same float64 run + 1e-7 (the 4 covers the fused multiply-add in
g coef + wd p and the other summation order of the norm, about one ulp each)."""

import functools

import pytest
import torch

from ghn3_amd import FusedSGD
from ghn3_amd import optim as O

pytestmark = pytest.mark.gpu

C = O.MT_CHUNK
SIZES = [1, 3, 4, 5, 255, 1024, 1025, C - 1, C, C + 1, 2 * C + 7, 0]
SHAPES = [(n,) for n in SIZES] + [(1,)] * 40 + [(64,), (16, 3, 3, 3), (10, 16)]
N_PVIEW, N_GVIEW, N_PAIR = 1029, 2051, C + 5
# after SHAPES: a parameter 4 bytes into a buffer, one whose gradient is such a view, the three tensors of the path test (same
# values: aligned / parameter view / gradient view), one that never has a gradient, one with requires_grad=False
EXTRA = [N_PVIEW, N_GVIEW, N_PAIR, N_PAIR, N_PAIR, 33, 17]
K_PVIEW, K_GVIEW, K_PAIR, K_NOGRAD, K_FROZEN = (len(SHAPES) + k for k in (0, 1, 2, 5, 6))
P_VIEWS, G_VIEWS = (K_PVIEW, K_PAIR + 1), (K_GVIEW, K_PAIR + 2)
STEPS = 4
CASES = {   # momentum, weight decay, nesterov, max_norm, grad_scale
    'momentum_wd_clip': (0.9, 1e-4, False, 5.0, 1.0),
    'plain': (0.0, 0.0, False, 0.0, 1.0),
    'nesterov': (0.9, 1e-4, True, 5.0, 1.0),
    'loss_scale': (0.9, 1e-4, False, 5.0, 1024.0),
}
LR = 0.05
assert sum(torch.Size(s).numel() for s in SHAPES) + sum(EXTRA) < 200000


def _values(seed):
    """fp32 CPU values for every tensor of the list; the three tensors of the path test share theirs."""
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(s, generator=g) for s in SHAPES] + [torch.randn(n, generator=g) for n in EXTRA]
    vals[K_PAIR + 1] = vals[K_PAIR].clone()
    vals[K_PAIR + 2] = vals[K_PAIR].clone()
    return vals


def _offset_view(v):
    """A CUDA copy of v that starts 4 bytes into a larger buffer."""
    buf = torch.zeros(v.numel() + 1, device='cuda')
    buf[1:].copy_(v.reshape(-1))
    t = buf[1:].view(v.shape)
    assert t.data_ptr() % 16 == 4
    return t


def _params(dtype=torch.float32, device='cuda'):
    ps = []
    for k, v in enumerate(_values(1)):
        if k in P_VIEWS and device == 'cuda':
            p = _offset_view(v).detach()
        else:
            p = v.to(device=device, dtype=dtype)
        ps.append(p.requires_grad_(k != K_FROZEN))
    return ps


def _set_grads(ps, step, scale=1.0, bad=None):
    """3 randn gradients (norm about 600, so max_norm 5 clips), the same values for every parameter list of one step."""
    for k, (p, v) in enumerate(zip(ps, _values(100 + step))):
        if k in (K_NOGRAD, K_FROZEN):
            continue
        g = 3 * v * scale
        if bad is not None and k == bad:
            g.view(-1)[g.numel() // 2] = float('inf')
        if k in G_VIEWS and p.is_cuda:
            p.grad = _offset_view(g)
        else:
            p.grad = g.to(device=p.device, dtype=p.dtype)


def _stock_step(ps, opt, max_norm):
    norm = torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], max_norm if max_norm > 0 else float('inf'))
    opt.step()
    return norm


def _stock_run(case, dtype, device, steps=range(STEPS)):
    mom, wd, nesterov, max_norm, _ = CASES[case]
    ps = _params(dtype, device)
    opt = torch.optim.SGD(ps, lr=LR, momentum=mom, weight_decay=wd, nesterov=nesterov)
    for step in steps:
        _set_grads(ps, step)
        _stock_step(ps, opt, max_norm)
    return ps, opt


def _cat(ts):
    return torch.cat([t.detach().reshape(-1).double().cpu() for t in ts])


def _stock_moms(ps, opt):
    return [opt.state[p]['momentum_buffer'] for p in ps if 'momentum_buffer' in opt.state.get(p, {})]


def _fused_moms(opt):
    return [v['momentum_buffer'] for _, v in sorted(opt.state_dict()['state'].items())]


@functools.lru_cache(maxsize=None)
def _reference(case, steps=tuple(range(STEPS))):
    """(parameters, momentum buffers) of the float64 CPU run, concatenated; and the errors stock fp32 on the GPU shows."""
    ps, opt = _stock_run(case, torch.float64, 'cpu', steps)
    ref_p, ref_m = _cat(ps), (_cat(_stock_moms(ps, opt)) if CASES[case][0] else None)
    qs, opt32 = _stock_run(case, torch.float32, 'cuda', steps)
    err_p = float((_cat(qs) - ref_p).norm() / ref_p.norm())
    err_m = float((_cat(_stock_moms(qs, opt32)) - ref_m).norm() / ref_m.norm()) if ref_m is not None else 0.0
    return ref_p, ref_m, err_p, err_m


def _check(case, ps, moms, what, steps=tuple(range(STEPS))):
    ref_p, ref_m, stock_p, stock_m = _reference(case, steps)
    err_p = float((_cat(ps) - ref_p).norm() / ref_p.norm())
    err_m = float((_cat(moms) - ref_m).norm() / ref_m.norm()) if ref_m is not None else 0.0
    print('sgd parity %-28s %-18s parameters %.3e (stock fp32 %.3e)  momentum %.3e (stock fp32 %.3e)'
          % (what, case, err_p, stock_p, err_m, stock_m))
    assert err_p <= 3e-6 and err_m <= 3e-6
    assert err_p <= 4 * stock_p + 1e-7
    assert err_m <= 4 * stock_m + 1e-7


def _fused(case, ps):
    mom, wd, nesterov, max_norm, _ = CASES[case]
    return FusedSGD(ps, lr=LR, momentum=mom, weight_decay=wd, nesterov=nesterov, max_grad_norm=max_norm)


def _fused_run(case, steps=range(STEPS)):
    scale = CASES[case][4]
    ps = _params()
    opt = _fused(case, ps)
    norms = []
    for step in steps:
        _set_grads(ps, step, scale)
        norms.append(opt.step(grad_scale=scale))
        opt.zero_grad()
    return ps, opt, norms


@pytest.mark.parametrize('case', list(CASES))
def test_four_steps_against_float64(case):
    ps, opt, norms = _fused_run(case)
    _check(case, ps, _fused_moms(opt), 'fused')
    # the returned norm is the unscaled one, as clip_grad_norm_ returns it
    qs = _params(torch.float64, 'cpu')
    _set_grads(qs, STEPS - 1)
    ref = float(_cat([q.grad for q in qs if q.grad is not None]).norm())
    assert abs(float(norms[-1]) - ref) <= 1e-6 * ref
    # untouched: the parameter without a gradient and the frozen one; no state entry for them either
    vals = _values(1)
    for k in (K_NOGRAD, K_FROZEN):
        assert torch.equal(ps[k].detach().cpu(), vals[k])
    sd = opt.state_dict()
    if CASES[case][0]:
        assert K_NOGRAD not in sd['state'] and K_FROZEN not in sd['state'] and len(sd['state']) == len(ps) - 2
    else:
        assert sd['state'] == {} and opt.momentum_buffer is None


def test_vector_and_scalar_paths_give_the_same_bits():
    """The same values in an aligned tensor, in a parameter 4 bytes into a buffer and under a gradient 4 bytes into a buffer."""
    ps, opt, _ = _fused_run('nesterov')
    assert ps[K_PAIR].data_ptr() % 16 == 0 and ps[K_PAIR + 1].data_ptr() % 16 == 4 and ps[K_PAIR + 2].data_ptr() % 16 == 0
    moms = opt.state_dict()['state']
    for k in (K_PAIR + 1, K_PAIR + 2):
        assert torch.equal(ps[k], ps[K_PAIR])
        assert torch.equal(moms[k]['momentum_buffer'], moms[K_PAIR]['momentum_buffer'])
    assert not torch.equal(ps[K_PAIR].detach().cpu(), _values(1)[K_PAIR])


def test_two_runs_give_the_same_bits():
    a, opt_a, norms_a = _fused_run('momentum_wd_clip')
    b, opt_b, norms_b = _fused_run('momentum_wd_clip')
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(opt_a.momentum_buffer, opt_b.momentum_buffer)
    assert all(torch.equal(x, y) for x, y in zip(norms_a, norms_b))


def test_a_non_finite_gradient_skips_the_step():
    case = 'momentum_wd_clip'
    ps = _params()
    opt = _fused(case, ps)
    _set_grads(ps, 0)
    opt.step()
    before, mom = [p.detach().clone() for p in ps], opt.momentum_buffer.clone()
    _set_grads(ps, 1, bad=len(SIZES) - 2)                               # one inf in the gradient of the 2 C + 7 tensor
    norm = opt.step()
    assert not bool(torch.isfinite(norm))
    assert all(torch.equal(p, q) for p, q in zip(ps, before))
    assert torch.equal(opt.momentum_buffer, mom)
    _set_grads(ps, 2)
    assert bool(torch.isfinite(opt.step()))
    _check(case, ps, _fused_moms(opt), 'fused, step 1 skipped', steps=(0, 2))    # a torch run that never saw the bad step


def _cloned(sd):
    return {'state': {k: {n: (v.clone() if torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd['state'].items()},
            'param_groups': sd['param_groups']}


def test_switch_to_the_stock_optimizer_and_back():
    case = 'momentum_wd_clip'
    mom, wd, nesterov, max_norm, _ = CASES[case]
    # two fused steps, then torch.optim.SGD from the fused state
    ps, opt, _ = _fused_run(case, steps=range(2))
    stock = torch.optim.SGD(ps, lr=LR, momentum=mom, weight_decay=wd, nesterov=nesterov)
    stock.load_state_dict(_cloned(opt.state_dict()))
    for step in (2, 3):
        _set_grads(ps, step)
        _stock_step(ps, stock, max_norm)
    _check(case, ps, _stock_moms(ps, stock), 'fused x 2, stock x 2')
    # two stock steps, then FusedSGD from torch's state
    ps, stock = _stock_run(case, torch.float32, 'cuda', steps=range(2))
    opt = _fused(case, ps)
    opt.load_state_dict(_cloned(stock.state_dict()))
    for step in (2, 3):
        _set_grads(ps, step)
        opt.step()
    _check(case, ps, _fused_moms(opt), 'stock x 2, fused x 2')
