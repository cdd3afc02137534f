"""
bf16 optimizer state with stochastic rounding on the MI355X (`pytest -m gpu`): GHN3_OP_ADAMW_S16 / GHN3_OP_ADAMW_S16_CAST16
and FusedAdamW(state_dtype='bf16').

  * one step on a bare flat buffer through ghn3_run, clipping and the loss scale on, from bf16-representable moments: the
    parameters equal the fp32-state GHN3_OP_ADAMW's bit for bit, the stored moments equal the host restatement's
    (ghn3_amd.optim.adamw_state16_reference_) bit for bit -- below one workgroup's span (1024 elements), over several spans
    with a ragged tail, split into launches at offsets, and on the scalar path (a count that is no multiple of 4, a
    misaligned range);
  * a non-finite squared norm leaves parameters and moments untouched; a step number of 2^24 is refused (GHN3_E_LIMIT);
  * a small GHN in f16 mode (hid 64, one 48-node graph): reruns are bit-identical, and the serial step, the overlapped
    step, the step that writes the W2 copies itself and the overlapped step without that fusion leave identical parameters
    and moments; the 16-bit W2 copies equal a fresh cast of the updated weight;
  * the stall case of tests/test_adamw_state16_cpu.py on the device, same bounds;
  * 30 training steps with bf16 state against the same steps with fp32 state (the parent's optimizer);
  * checkpoints: fp32 tensors torch.optim.AdamW loads; an fp32-state and a bf16-state optimizer resumed from one file take
    the same next step;
  * Trainer passes `state_dtype` through.
"""
import numpy as np
import pytest
import torch

from util_parity import make_models, synthetic_case

pytestmark = pytest.mark.gpu

CFG = dict(max_shape=(64, 64, 16, 16), num_classes=1000, hid=64, heads=8, layers=3, weight_norm=True, ve=True,
           layernorm=True)
HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
MAX_NORM, SCALE, STEP, SEED = 0.05, 1024.0, 7, 9


def _bits(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16).copy()


# ------------------------------------------------------------------------------------------- bare flat buffers
def _ops(kind, ranges, n, step=STEP, seed=SEED, guard=True):
    """[MEMSET0, SUMSQ over all n, one AdamW op per (lo, count)] over bufs = [p, g, m, v, scal, parts]."""
    from ghn3_amd import _lib as L
    from ghn3_amd.optim import _dbits
    s16 = kind == L.OP_ADAMW_S16
    ops = np.zeros(2 + len(ranges), dtype=L.OP_DT)
    ops['r']['buf'][:] = -1
    ops[0]['kind'] = L.OP_MEMSET0
    ops[0]['r']['buf'][0] = 4
    ops[0]['i'][0] = 4
    ops[1]['kind'] = L.OP_SUMSQ if guard else L.OP_NOP
    ops[1]['r']['buf'][:3] = (4, 1, 5)
    ops[1]['i'][0] = n
    hyper = (HYPER['lr'], HYPER['betas'][0], HYPER['betas'][1], HYPER['eps'], HYPER['weight_decay'],
             1.0 - HYPER['betas'][0] ** step, 1.0 - HYPER['betas'][1] ** step)
    for op, (lo, count) in zip(ops[2:], ranges):
        op['kind'] = kind
        op['r']['buf'][:5] = (0, 1, 2, 3, 4 if guard else -1)
        op['r']['off'][:4] = 4 * lo
        if s16:
            op['r']['off'][2:4] = 2 * lo
            op['f'][2], op['f'][3] = float(step), float(seed)
        op['i'][0] = count
        for k, h in enumerate(hyper):
            op['i'][1 + k] = _dbits(h)
        op['f'][0] = MAX_NORM if guard else 0.0
        op['f'][1] = 1.0 / SCALE
    return ops


def _run(ops, tensors):
    from ghn3_amd import _lib as L
    scal = torch.zeros(16, device='cuda')
    parts = torch.zeros(8192, device='cuda')
    bufs = np.asarray([t.data_ptr() for t in tensors] + [scal.data_ptr(), parts.data_ptr()], dtype=np.uint64)
    L.context(0).run(ops, np.zeros(0, dtype=L.PROBLEM_DT), bufs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return float(scal[0].item())


def _state(n, seed):
    rng = np.random.default_rng(seed)
    p = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
    g = torch.from_numpy((SCALE * 1e-2 * rng.standard_normal(n)).astype(np.float32))
    m = torch.from_numpy((1e-2 * rng.standard_normal(n)).astype(np.float32)).to(torch.bfloat16)
    v = torch.from_numpy((1e-4 * rng.random(n)).astype(np.float32)).to(torch.bfloat16)
    return p, g, m, v


_WANT = {}


def _want(n):
    """(initial state, parameters of the fp32-state op, sumsq, moments of the host restatement), once per size."""
    if n not in _WANT:
        from ghn3_amd import _lib as L
        from ghn3_amd.optim import adamw_state16_reference_
        state = _state(n, 100 + n)
        f32 = [state[0].cuda(), state[1].cuda(), state[2].float().cuda(), state[3].float().cuda()]
        sumsq = _run(_ops(L.OP_ADAMW, [(0, n)], n), f32)
        host = [t.clone() for t in state]
        adamw_state16_reference_(*host, sumsq, STEP, HYPER['lr'], HYPER['betas'], HYPER['eps'], HYPER['weight_decay'], MAX_NORM,
                                 1.0 / SCALE, seed=SEED, base=0)
        assert float((host[0] - f32[0].cpu()).abs().max()) < 1e-5          # (the same update; the bits are compared below)
        _WANT[n] = (state, f32[0].cpu(), sumsq, host)
    return _WANT[n]


@pytest.mark.parametrize('n,ranges', [
    (1000, [(0, 1000)]),                                   # below one workgroup's span (256 lanes x 4 elements)
    (5156, [(0, 5156)]),                                   # five spans and a ragged tail, a multiple of 4
    (5156, [(0, 1032), (1032, 4), (1036, 4120)]),          # the same buffer in three launches at offsets
    (5156, [(0, 1001), (1001, 4155)]),                     # scalar path: a tail of one element, then a misaligned range
])
def test_one_step_on_a_flat_buffer(n, ranges):
    from ghn3_amd import _lib as L
    state, p32, sumsq, host = _want(n)
    dev = [t.cuda() for t in state]
    got = _run(_ops(L.OP_ADAMW_S16, ranges, n), dev)
    assert got == sumsq
    clip = MAX_NORM / (sumsq ** 0.5 / SCALE + 1e-6)
    assert clip < 0.5, clip                                 # (the clipping is active)
    assert torch.equal(dev[0].cpu(), p32) and not torch.equal(p32, state[0])
    bm, bv = _bits(dev[2]), _bits(dev[3])
    wm, wv = _bits(host[2]), _bits(host[3])
    print('moments that differ from the host restatement: %d, %d of %d' % ((bm != wm).sum(), (bv != wv).sum(), n))
    assert np.array_equal(bm, wm) and np.array_equal(bv, wv)
    assert (bm != _bits(state[2])).mean() > 0.9


def test_a_non_finite_norm_leaves_everything_untouched_and_large_steps_are_refused():
    from ghn3_amd import _lib as L
    n = 5156
    state = _state(n, 3)
    state[1][n - 3] = float('nan')
    dev = [t.cuda() for t in state]
    got = _run(_ops(L.OP_ADAMW_S16, [(0, 1032), (1032, n - 1032)], n), dev)
    assert not np.isfinite(got)
    assert torch.equal(dev[0].cpu(), state[0])
    assert np.array_equal(_bits(dev[2]), _bits(state[2])) and np.array_equal(_bits(dev[3]), _bits(state[3]))
    with pytest.raises(L.Ghn3Error, match=r'\(-2\)'):        # GHN3_E_LIMIT
        _run(_ops(L.OP_ADAMW_S16, [(0, n)], n, step=1 << 24), dev)
    assert torch.equal(dev[0].cpu(), state[0])


def test_stochastic_storage_does_not_stall_on_the_device():
    """4096 elements, constant gradients 1e-3 U(0.5, 1.5), beta2 = 0.999, 2000 steps: the stored exp_avg_sq follows the exact
    average (median within 1 %, every element within 0.15, spread as an ideal generator's: see the CPU test's docstring)."""
    from ghn3_amd import _lib as L
    from ghn3_amd.optim import _dbits
    rng = np.random.default_rng(11)
    g = (1e-3 * rng.uniform(0.5, 1.5, 4096)).astype(np.float32)
    exact = g.astype(np.float64) ** 2 * (1.0 - 0.999 ** 2000)
    dev = [torch.zeros(4096, device='cuda'), torch.from_numpy(g).cuda(),
           torch.zeros(4096, dtype=torch.bfloat16, device='cuda'), torch.zeros(4096, dtype=torch.bfloat16, device='cuda')]
    bufs = np.asarray([t.data_ptr() for t in dev], dtype=np.uint64)
    ctx, stream = L.context(0), torch.cuda.current_stream().cuda_stream
    none = np.zeros(0, dtype=L.PROBLEM_DT)
    ops = np.zeros(1, dtype=L.OP_DT)
    ops['r']['buf'][:] = -1
    ops[0]['kind'] = L.OP_ADAMW_S16
    ops[0]['r']['buf'][:4] = (0, 1, 2, 3)
    ops[0]['i'][0] = 4096
    ops[0]['f'][1] = 1.0
    for t in range(1, 2001):
        for k, h in enumerate((0.0, 0.9, 0.999, 1e-8, 0.0, 1.0 - 0.9 ** t, 1.0 - 0.999 ** t)):
            ops[0]['i'][1 + k] = _dbits(h)
        ops[0]['f'][2] = float(t)
        ctx.run(ops, none, bufs, stream)
    torch.cuda.synchronize()
    ratio = dev[3].double().cpu().numpy() / exact
    print('device: median %.4f mean %.4f std %.4f worst %.4f' % (np.median(ratio), ratio.mean(), ratio.std(),
                                                              np.abs(ratio - 1).max()))
    assert abs(np.median(ratio) - 1.0) < 0.01
    assert np.abs(ratio - 1.0).max() < 0.15
    assert ratio.std() < 0.026
    assert torch.equal(dev[0], torch.zeros_like(dev[0]))      # (lr = 0, no weight decay)


# ------------------------------------------------------------------------------------------- FusedAdamW on a small GHN
_SD = {}


def _fresh():
    """The small GHN in f16 mode (the mode in which the optimizer writes the W2 copies), same seeded weights every time."""
    from ghn3_amd import GHN3
    if not _SD:
        hip, _ = make_models(CFG, 7, compute='f16')
        _SD.update({k: v.detach().cpu().clone() for k, v in hip.state_dict().items()})
        return hip.train()
    hip = GHN3(**CFG, compute='f16')
    hip.load_state_dict(_SD)
    return hip.to('cuda').train()


_CASE = []


def _case():
    if not _CASE:
        _CASE.extend(synthetic_case([48], 4800)[:2])
    return _CASE


def _steps(form, state_dtype='bf16', steps=3):
    from ghn3_amd import FusedAdamW
    nets, gb = _case()
    hip = _fresh()
    plan = hip.compile(nets, gb, training=True)
    assert plan.program.shadow_w2 is not None
    opt = FusedAdamW(hip, max_grad_norm=1.0, state_dtype=state_dtype, state_seed=5, **HYPER)
    torch.manual_seed(3)
    for k in range(steps):
        hip._run_forward(plan)
        hip._run_backward(plan, torch.randn(plan.program.out_numel, device='cuda') * 1e-3)
        if form == 'serial':
            opt.step(plan.gflat)
        else:
            opt.step(plan.gflat, plan=plan, overlap=form.startswith('overlap'))
            assert hip._ctx().side_pending() == form.startswith('overlap')
            assert (hip._shadow_w2_state is not None) == (not form.endswith('plain'))
    opt.wait()
    torch.cuda.synchronize()
    return hip, opt, plan


def test_every_form_of_the_step_and_a_rerun_give_the_same_bits(monkeypatch):
    runs = {form: _steps(form) for form in ('fused', 'serial', 'overlap')}
    runs['rerun'] = _steps('fused')
    monkeypatch.setenv('GHN3_ADAMW_CAST', '0')
    runs['overlap-plain'] = _steps('overlap-plain')
    monkeypatch.delenv('GHN3_ADAMW_CAST')
    hip, opt, plan = runs['fused']
    n = hip._flat.numel()
    assert opt.exp_avg.dtype == opt.exp_avg_sq.dtype == torch.bfloat16 and opt.exp_avg.numel() == opt.exp_avg_sq.numel() == n
    assert opt.steps == 3 and float(opt.exp_avg.float().abs().max()) > 0
    for form, (h, o, _) in runs.items():
        assert torch.equal(h._flat, hip._flat), form
        assert torch.equal(o.exp_avg, opt.exp_avg) and torch.equal(o.exp_avg_sq, opt.exp_avg_sq), form
    # the copies the fused step wrote: equal to a fresh cast of the updated weight (every copy re-cast from the parameters)
    hip._run_forward(plan)                                   # (refreshes the copies the optimizer does not write)
    torch.cuda.synchronize()
    assert hip._shadow_w2_state is not None
    mine = hip._shadow.clone()
    hip._shadow_w2_state = hip._shadow_state = None
    hip._run_forward(plan)
    torch.cuda.synchronize()
    assert torch.equal(mine, hip._shadow)


def _train(state_dtype, steps=30):
    from ghn3_amd import FusedAdamW
    nets, gb = _case()
    hip = _fresh()
    p0 = hip._flat.detach().clone()
    opt = FusedAdamW(hip, lr=1e-3, weight_decay=1e-2, max_grad_norm=5.0, state_dtype=state_dtype)
    for _ in range(steps):
        for p in hip.parameters():
            p.grad = None
        hip(nets, gb, keep_grads=True)
        hip.predicted_param_norm().backward()
        opt.step(hip.last_plan.gflat, plan=hip.last_plan, overlap=True)
    opt.wait()
    torch.cuda.synchronize()
    return (hip._flat.detach() - p0).double()


def test_a_short_trajectory_follows_the_fp32_state_optimizer():
    """30 steps on a fixed batch (one 48-node graph, loss = the predicted-parameter norm, lr 1e-3, clipping at 5), with bf16
    state and with fp32 state -- the parent's optimizer, which is the reference here.  Relative L2 distance of the parameter
    change p30 - p0 between the two, measured on the MI355X: 5.50e-2 (5.13e-2 with state_seed=1); the test allows twice that.
    The distance is the trajectory's own sensitivity, not an error of a step: it is 0 after step 1 (the parameters take the
    unrounded moments), 7.6e-4 after step 2, 6.6e-3 after 10, 2.1e-2 after 20 -- and the fp32-state trajectory moves by
    6.6e-2 after the same 30 steps when its learning rate changes by 0.1 % (1.3e-2 after 10, 3.1e-2 after 20)."""
    d32, d16 = _train('fp32'), _train('bf16')
    rel = float((d16 - d32).norm() / d32.norm())
    print('relative L2 of the parameter change, bf16 state against fp32 state: %.3e' % rel)
    assert float(d32.norm()) > 0
    assert rel < 2 * MEASURED_REL, rel


MEASURED_REL = 5.5e-2


def test_checkpoints_are_fp32_and_resume_in_either_optimizer(tmp_path):
    from ghn3_amd import FusedAdamW, save_checkpoint
    hip = _fresh()
    n = hip._flat.numel()
    with pytest.raises(ValueError):
        FusedAdamW(hip, state_dtype='fp16')
    gen = torch.Generator(device='cuda').manual_seed(1)
    mask = torch.zeros(n, device='cuda')                     # (a gradient buffer holds zeros between the parameters)
    for q in hip.parameters():
        o = (q.data_ptr() - hip._flat.data_ptr()) // 4
        mask[o:o + q.numel()] = 1.0

    def grad():
        return torch.randn(n, device='cuda', generator=gen) * 1e-3 * mask
    opt = FusedAdamW(hip, max_grad_norm=1.0, state_dtype='bf16', state_seed=5, **HYPER)
    for _ in range(2):
        opt.step(grad())
    path = save_checkpoint(str(tmp_path / 'ckpt.pt'), hip, opt, 0, 1)
    sd = torch.load(path, map_location='cpu')['optimizer']
    assert len(sd['state']) == len(list(hip.parameters()))
    for st in sd['state'].values():
        assert st['exp_avg'].dtype == st['exp_avg_sq'].dtype == torch.float32
    own = opt.state_dict()['state'][0]['exp_avg']
    assert own.dtype == torch.float32 and own.data_ptr() != opt.exp_avg.data_ptr()          # (a copy, not a view)
    # torch.optim.AdamW over a CPU copy of the parameters takes it as it is
    cpu_params = [p.detach().cpu().clone().requires_grad_() for p in hip.parameters()]
    stock = torch.optim.AdamW(cpu_params, lr=1e-3)
    stock.load_state_dict(sd)
    k, p = next((k, p) for k, p in enumerate(cpu_params) if p.numel() > 1000)
    assert stock.state[p]['exp_avg'].dtype == torch.float32
    assert torch.equal(stock.state[p]['exp_avg'], sd['state'][k]['exp_avg']) and float(stock.state[p]['step']) == 2.0
    # one further step from the file: fp32 state (exact load) and bf16 state move the parameters alike
    g = grad()
    after = {}
    for state_dtype in ('fp32', 'bf16'):
        other = _fresh()
        with torch.no_grad():
            other._flat.copy_(hip._flat)
        other.params_changed()
        o = FusedAdamW(other, max_grad_norm=1.0, state_dtype=state_dtype, state_seed=5, **HYPER)
        o.load_state_dict(sd)
        assert o.steps == 2
        assert torch.equal(o.exp_avg.float(), opt.exp_avg.float()) and torch.equal(o.exp_avg_sq.float(), opt.exp_avg_sq.float())
        o.step(g.clone())
        torch.cuda.synchronize()
        after[state_dtype] = other._flat.detach().clone()
    assert torch.equal(after['fp32'], after['bf16']) and not torch.equal(after['bf16'], hip._flat)


def test_trainer_passes_the_state_type_through():
    import recipe
    import graph_nets
    from ghn3_amd import Graph, GraphBatch, Trainer
    hip, _ = make_models(dict(recipe.TINY_CFG), recipe.TINY_SEED)
    tr = Trainer(hip, 'adamw', {'lr': 1e-3, 'state_dtype': 'bf16', 'state_seed': 3}, 'cosine', n_batches=10, grad_clip=5,
                 device='cuda', epochs=2, log_interval=1)
    opt = tr._optimizer
    assert opt.state_dtype == 'bf16' and opt.state_seed == 3
    assert opt.exp_avg.dtype == opt.exp_avg_sq.dtype == torch.bfloat16
    assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == hip._flat.numel()
    nets = [graph_nets.all_nets(graph_nets.local_bases())['resnet_tiny'].to('cuda')]
    gb = GraphBatch([Graph(net, ve_cutoff=50) for net in nets], dense=True)
    gb.nets = nets
    before = hip._flat.detach().clone()
    tr.update(torch.randn(2, 3, 32, 32), torch.tensor([1, 2]), gb)
    opt.wait()
    torch.cuda.synchronize()
    assert torch.isfinite(hip._flat).all() and not torch.equal(before, hip._flat)
    assert float(opt.exp_avg_sq.float().max()) > 0
