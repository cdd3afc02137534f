"""
GPU parity tests (run on the MI355X box with `pytest -m gpu`): every result comes from libghn3_hip.so
through its C ABI and is compared with the CPU oracle (oracle/) and the committed golden fixtures.

Tolerances (north star: 1e-3 relative fp32):
  * fp32 MFMA path      per-tensor relative L2 <= 2e-5 (forward), <= 2e-4 (gradients)
  * f16 operand path    per-tensor relative L2 <= 1e-3
  * integer / index work (degrees, distances, pair ids) bit-exact
"""

import os
import numpy as np
import pytest
import torch

import recipe
from util_parity import (rel_l2, make_models, tiny_case, synthetic_case, oracle_intermediates, ws_tensor,
                         predicted_dict_hip)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def ctx():
    from ghn3_amd import _lib as L
    return L.context(0)


def test_library_is_the_hip_build(ctx):
    from ghn3_amd import _lib as L
    assert L.load().ghn3_abi_version() == L.ABI_VERSION


@pytest.mark.parametrize('ctype,tol', [(0, 2e-6), (1, 2e-3), (2, 1.5e-2)])
def test_gemm_cases(ctx, ctype, tol):
    from gemm_cases import CASES, run_gemm_case
    for k, case in enumerate(CASES):
        got, exp, extra = run_gemm_case(ctx, ctype=ctype, seed=k, **case)
        err = rel_l2(got, exp)
        assert err < tol, (case, err)
        if extra is not None:
            assert rel_l2(extra[0], extra[1]) < tol, ('aux_out', case)


def test_split_bf16_weight_gradient_gemm_cases(ctx):
    """Tile code 48 (gemm_wg.hip): dW = dY^T X with both operands fp32 activations reduced over rows, as split-bf16 products;
    fused bias gradient and accumulate; tolerance = the dropped lo.lo term, as for the split-bf16 linears."""
    from gemm_cases import WG_CASES, run_gemm_case
    for k, case in enumerate(WG_CASES):
        got, exp, extra = run_gemm_case(ctx, ctype=0, seed=100 + k, **case)
        assert np.isfinite(got).all(), case
        err = rel_l2(got, exp)
        assert err < 3e-5, (case, err)
        if extra is not None:
            assert rel_l2(extra[0], extra[1]) < 2e-6, ('bias gradient', case, rel_l2(extra[0], extra[1]))


def test_layernorm_row_prologue_of_the_small_gemm(ctx):
    """ghn3_gemm_problem::ln_kind: LayerNorm forward / backward applied to the A rows while they are staged (exact
    fp32): products and by-products (normalised rows, mean, rstd) against fp64 numpy."""
    from gemm_cases import LN_CASES, run_ln_case
    for k, case in enumerate(LN_CASES):
        for j, (got, exp) in enumerate(run_ln_case(ctx, seed=k, **case)):
            assert np.isfinite(got).all(), (case, j)
            assert rel_l2(got, exp) < 3e-6, (case, j, rel_l2(got, exp))


def test_split_bf16_gemm_cases(ctx):
    """GHN3_GEMM_X3 + GHN3_CAST_SPLIT: split-bf16 products (hi.hi + hi.lo + lo.hi on v_mfma_f32_16x16x32_bf16) against fp64
    on the Graphormer shapes of the released models, every tile / slice variant and epilogue; tolerance = the dropped
    lo.lo term (2^-16 relative per product)."""
    from gemm_cases import X3_CASES, run_x3_case
    for k, case in enumerate(X3_CASES):
        for j, (got, exp) in enumerate(run_x3_case(ctx, seed=k, **case)):
            assert np.isfinite(got).all(), (case, j)
            err = rel_l2(got, exp)
            # (f16 pieces -- GHN3_GEMM_X3F16, the forward linears -- carry 11 + 11 bits: fp32-grade products)
            assert err < (2e-6 if case.get('f16') else 3e-5), (case, j, err)


def test_f16_piece_gemm_saturates_instead_of_overflowing(ctx):
    """GHN3_GEMM_X3F16 (the Graphormer's forward linears): an activation beyond the f16 range or a weight >= 1024 (x 2^6 in its
    copy) used to become inf in the hi piece and NaN in the lo piece (x - inf) where the bf16-piece / fp32 paths and the
    reference stay finite.  The pieces saturate now: finite everywhere, and every output that does not touch the out-of-range
    operands keeps the fp32-grade accuracy."""
    from gemm_cases import run_x3_case
    for case in (dict(M=256, N=384, K=384, tile=45, epilogue='bias_res', f16=True, big=True),
                 dict(M=70, N=192, K=64, tile=44, epilogue='bias_relu', f16=True, big=True)):
        (got, exp), = run_x3_case(ctx, seed=3, **case)
        assert np.isfinite(got).all(), case
        rows = np.r_[0, 2:case['M']]
        cols = np.r_[0:3, 4:case['N']]              # (W[3, :] holds the out-of-range weight: output column 3)
        assert rel_l2(got[np.ix_(rows, cols)], exp[np.ix_(rows, cols)]) < 2e-6, case


def _run_forward(hip, nets, gb, training=False):
    plan = hip.compile(nets, gb, training=training)
    with torch.no_grad():
        flat = hip._run_forward(plan)
    torch.cuda.synchronize()
    return plan, flat


@pytest.mark.parametrize('ctype', [1, 2])
def test_cast16_and_16bit_operand_gemm(ctx, ctype):
    """GHN3_OP_CAST16 + GHN3_GEMM_OP16: exact against fp64 products of the CPU-rounded operands (only the fp32
    accumulation order differs), incl. transposed copies, zero K padding, the B k-map, split-K and column sums."""
    from gemm_cases import OP16_CASES, run_op16_case
    for k, case in enumerate(OP16_CASES):
        for got, exp in run_op16_case(ctx, ctype=ctype, seed=k, **case):
            assert np.isfinite(got).all(), case
            err = rel_l2(got, exp)
            assert err < 3e-6, (case, err)


@pytest.mark.parametrize('case', ['b1', 'b2', 'b2r'])
def test_tiny_forward_matches_oracle_and_golden(case):
    hip, oracle = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
    nets_h, gb_h, nets_o, gb_o = tiny_case(case)
    plan, flat = _run_forward(hip, nets_h, gb_h)
    prog = plan.program
    # integer prologue: bit exact
    A = gb_o.edges
    deg_in = torch.clip((A == 1).long().sum(1), 0, 100).numpy().astype(np.int32)
    deg_out = torch.clip((A == 1).long().sum(2), 0, 100).numpy().astype(np.int32)
    off = prog._ws_names['deg_in']
    n = prog.B * prog.N
    got_in = plan.ws[off:off + 4 * n].view(torch.int32).cpu().numpy().reshape(prog.B, prog.N)
    off = prog._ws_names['deg_out']
    got_out = plan.ws[off:off + 4 * n].view(torch.int32).cpu().numpy().reshape(prog.B, prog.N)
    np.testing.assert_array_equal(got_in, deg_in)
    np.testing.assert_array_equal(got_out, deg_out)
    # stage-wise float parity
    inter = oracle_intermediates(oracle, nets_o, gb_o)
    B, N, C, H = prog.B, prog.N, prog.C, prog.H
    assert rel_l2(ws_tensor(plan, 'x0', (B, N, C)).cpu(), inter['x0']) < 1e-6
    assert rel_l2(ws_tensor(plan, 'bias', (B, H, N, N)).cpu(), inter['bias']) < 1e-5
    for l in range(1, prog.Lyr + 1):
        assert rel_l2(ws_tensor(plan, 'x%d' % l, (B, N, C)).cpu(), inter['x%d' % l]) < 2e-5, l
    assert rel_l2(hip.embeddings(plan).cpu(), inter['xe']) < 2e-5
    # predicted tensors vs oracle
    oracle.train()
    with torch.no_grad():
        _, pred_o = oracle(nets_o, gb_o, assign=False)
    pred_h = predicted_dict_hip(plan, flat)
    assert len(pred_o) == len(pred_h)
    for k, (ind, attr, m, t) in enumerate(pred_o):
        a, b = pred_h[k].cpu(), t
        assert tuple(a.shape) == tuple(b.shape), (k, a.shape, b.shape)
        if b.dim() == 3:
            a, b = a[:, 1:], b[:, 1:]            # Q3: random class-token row
        assert rel_l2(a, b) < 2e-5, (k, attr, tuple(b.shape), rel_l2(a, b))
    # and straight against the golden vectors produced by the reference
    g = np.load(os.path.join(GOLD, 'ghn3_tiny.npz'))
    hip.assign(plan, flat, keep_grads=False)
    for bi, net in enumerate(nets_h):
        for name, p in recipe.named_predicted(net):
            ref = g['%s/pred/%d/%s' % (case, bi, name)]
            got = p.detach().cpu().numpy()
            if ref.ndim == 3:
                got, ref = got[:, 1:], ref[:, 1:]
            assert rel_l2(got, ref) < 2e-5, (name, rel_l2(got, ref))
    assert rel_l2(hip.embeddings(plan).cpu(), g[case + '/emb']) < 2e-5


@pytest.mark.parametrize('case', ['b1', 'b2'])
def test_tiny_backward_matches_oracle_and_golden(case):
    hip, oracle = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
    nets_h, gb_h, nets_o, gb_o = tiny_case(case)
    hip.train()
    nets_h = hip(nets_h, gb_h, keep_grads=True)
    loss = 0
    for net in nets_h:
        for name, p in recipe.named_predicted(net):
            q = p[:, 1:] if p.dim() == 3 else p
            loss = loss + torch.norm(q, p='fro')
    loss.backward()
    torch.cuda.synchronize()
    oracle.train()
    nets_o, pred_o = oracle(nets_o, gb_o, keep_grads=True)
    loss_o = 0
    for (ind, attr, m, t) in pred_o:
        q = t[:, 1:] if t.dim() == 3 else t
        loss_o = loss_o + torch.norm(q, p='fro')
    loss_o.backward()
    assert abs(loss.item() - loss_o.item()) < 1e-4 * abs(loss_o.item())
    g = np.load(os.path.join(GOLD, 'ghn3_tiny.npz'))
    po = dict(oracle.named_parameters())
    worst = 0
    for k, p in hip.named_parameters():
        assert p.grad is not None, k
        go = po[k].grad
        err = float((p.grad.cpu().double() - go.double()).norm())
        e = err / (float(go.norm()) + 1e-12)
        worst = max(worst, err / (float(go.norm()) + 1e-3))
        # (proj_e.2.bias has an analytically zero gradient: softmax is shift invariant)
        assert err < 2e-4 * float(go.norm()) + 2e-6, (k, e, float(go.norm()))
        ref = g['%s/grad/%s' % (case, k)]
        assert abs(p.grad.norm().item() - ref[0]) < 2e-4 * max(1.0, ref[0]), (k, p.grad.norm().item(), ref[0])
    print('worst grad rel-L2', worst)


@pytest.mark.parametrize('case', sorted(recipe.EXTRA_CASES))
def test_extra_cases_forward_backward(case):
    """Kernels larger than the decoder grid (bilinear resize as a constant GEMM, nn.py:751-753) and the
    weight_norm=False / layernorm=False configurations: HIP path vs the oracle and vs the reference's goldens."""
    cfg = dict(recipe.TINY_CFG, **recipe.EXTRA_CASES[case][1])
    hip, oracle = make_models(cfg, recipe.TINY_SEED)
    nets_h, gb_h, nets_o, gb_o = tiny_case(case)
    hip.train()
    nets_h = hip(nets_h, gb_h, keep_grads=True)
    g = np.load(os.path.join(GOLD, 'ghn3_tiny_extra.npz'))
    loss = 0
    for bi, net in enumerate(nets_h):
        for name, p in recipe.named_predicted(net):
            ref = g['%s/pred/%d/%s' % (case, bi, name)]
            got = p.detach().cpu().numpy()
            assert got.shape == ref.shape, name
            if ref.ndim == 3:
                got, ref = got[:, 1:], ref[:, 1:]            # Q3: random class-token row
            assert rel_l2(got, ref) < 2e-5, (name, rel_l2(got, ref))
            loss = loss + torch.norm(p[:, 1:] if p.dim() == 3 else p, p='fro')
    assert rel_l2(hip.embeddings(hip.last_plan).cpu(), g[case + '/emb']) < 2e-5
    loss.backward()
    torch.cuda.synchronize()
    oracle.train()
    nets_o, pred_o = oracle(nets_o, gb_o, keep_grads=True)
    loss_o = sum(torch.norm(t[:, 1:] if t.dim() == 3 else t, p='fro') for (_, _, _, t) in pred_o)
    loss_o.backward()
    assert abs(loss.item() - loss_o.item()) < 1e-4 * abs(loss_o.item())
    po = dict(oracle.named_parameters())
    assert sorted(po) == sorted(k for k, _ in hip.named_parameters())
    for k, p in hip.named_parameters():
        go = po[k].grad
        err = float((p.grad.cpu().double() - go.double()).norm())
        assert err < 2e-4 * float(go.norm()) + 2e-6, (k, err, float(go.norm()))
        ref = g['%s/grad/%s' % (case, k)]
        assert abs(p.grad.norm().item() - ref[0]) < 2e-4 * max(1.0, ref[0]), (k, p.grad.norm().item(), ref[0])


@pytest.mark.parametrize('case', sorted(recipe.EDGE_CASES))
@pytest.mark.parametrize('compute', ['f32', 'f16'])
def test_degenerate_batches_forward_backward(case, compute):
    """Edge cases of the batch: a network without any 2-D / 4-D weight (zero decoder rows: every decoder GEMM, cast and
    tile launch of the family is empty), a single 1x1 convolution, three graphs of very different sizes (ragged masks), a
    weight-less network next to a normal one -- predicted tensors and every GHN gradient against the oracle; parameters
    the batch does not touch get an all-zero gradient."""
    hip, oracle = make_models(dict(recipe.TINY_CFG), recipe.TINY_SEED, compute=compute)
    nets_h, gb_h, nets_o, gb_o = tiny_case(case)
    hip.train()
    nets_h = hip(nets_h, gb_h, keep_grads=True)
    oracle.train()
    nets_o, pred_o = oracle(nets_o, gb_o, keep_grads=True)
    tol_f, tol_g = (2e-5, 2e-4) if compute == 'f32' else (1e-3, 2e-3)
    loss, loss_o, n_cmp = 0, 0, 0
    for net_h, net_o in zip(nets_h, nets_o):
        ref = dict(recipe.named_predicted(net_o))
        for name, p in recipe.named_predicted(net_h):
            t = ref[name]
            n_cmp += 1
            assert tuple(p.shape) == tuple(t.shape), name
            if p.dim() == 3:
                p, t = p[:, 1:], t[:, 1:]                    # Q3: random class-token row of positional encodings
            assert rel_l2(p.detach().cpu(), t.detach()) < tol_f, (name, rel_l2(p.detach().cpu(), t.detach()))
            loss = loss + torch.norm(p, p='fro')
            loss_o = loss_o + torch.norm(t, p='fro')
    assert n_cmp >= 1
    loss.backward()
    torch.cuda.synchronize()
    loss_o.backward()
    po = dict(oracle.named_parameters())
    for name, p in hip.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        go = po[name].grad if po[name].grad is not None else torch.zeros_like(po[name])
        err = float((p.grad.cpu().double() - go.double()).norm())
        assert err < tol_g * float(go.norm()) + 2e-6, (name, err, float(go.norm()))


@pytest.mark.parametrize('name', ['resnet_tiny', 'mobile_se', 'vit_tiny', 'attn_tiny'])
def test_ghn_model_without_a_graph(name):
    """examples/ghn_single_model.py call sequence: ``ghn(model)`` with graphs=None builds the graph from the module
    (ghn3_amd/graph_build.py, pinned against the reference in tests/test_host_api_cpu.py), predicts every
    parameter and assigns it; values checked against the oracle run on the same graph."""
    import graph_nets
    from ghn3_amd import Graph
    from oracle import ghn3_ref as R
    hip, oracle = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
    hip.eval()
    hip.debug_level = 1                                           # nn.py:354-403: the MATCHED! self-check
    net = graph_nets.all_nets(graph_nets.local_bases())[name].to('cuda')
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    with torch.no_grad():
        out = hip(net)                                            # graphs=None
    assert out is net
    info = hip.last_debug_info
    n_untouched = sum(v.numel() for k, v in before.items() if k.endswith('class_token'))
    assert info['n_params'] == sum(v.numel() for v in before.values())
    assert info['n_params_pred'] == info['n_params'] - n_untouched and info['matched'] == (n_untouched == 0)
    torch.cuda.synchronize()
    net_o = graph_nets.all_nets(graph_nets.local_bases())[name]
    g = Graph(net_o, ve_cutoff=50)
    gb_o = R.GraphBatchRef([R.GraphRef(g.node_feat, g.node_info, g._Adj)])
    oracle.eval()
    with torch.no_grad():
        oracle([net_o], gb_o, keep_grads=False)
    po = dict(net_o.named_parameters())
    changed = 0
    for k, p in net.named_parameters():
        assert isinstance(p, torch.nn.Parameter) and torch.isfinite(p).all(), k
        if k.endswith('class_token'):
            assert torch.equal(p, before[k])                       # not a graph node: left untouched
            continue
        a, b = p.detach().cpu(), po[k].detach()
        if a.dim() == 3:
            a, b = a[:, 1:], b[:, 1:]                              # Q3: random class-token row
        assert rel_l2(a, b) < 2e-5, (k, rel_l2(a, b))
        changed += int(not torch.equal(p, before[k]))
    assert changed == len(before) - int(any(k.endswith('class_token') for k in before))
    # the network runs with the predicted parameters
    y = net(torch.randn(2, 3, 32, 32, device='cuda'))
    assert y.shape == (2, 10) and torch.isfinite(y).all()


@pytest.mark.parametrize('name', ['resnet_tiny', 'mobile_se'])
def test_target_network_loss_trains_the_ghn(name):
    """The reference trainer's step (trainer.py:300-330): predict the parameters of a target network with gradients
    kept, run the network on an image batch, take the cross-entropy and back-propagate into the GHN.  The target
    network itself runs on stock torch ops (SURVEY 8(f) row 2 is not rebuilt); this checks that the predicted views
    of the flat buffer carry gradients from an arbitrary downstream loss back through the backward program."""
    import graph_nets
    import torch.nn.functional as F
    from ghn3_amd import Graph, GraphBatch
    from oracle import ghn3_ref as R
    hip, oracle = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
    hip.train()
    oracle.train()
    gen = torch.Generator().manual_seed(5)
    images = torch.randn(4, 3, 32, 32, generator=gen)
    labels = torch.tensor([1, 7, 3, 9])

    net = graph_nets.all_nets(graph_nets.local_bases())[name].to('cuda')
    g = Graph(net, ve_cutoff=50)
    net = hip(net, GraphBatch([g], dense=True).to_device('cuda'), keep_grads=True)
    loss = F.cross_entropy(net(images.cuda()), labels.cuda())
    loss.backward()
    torch.cuda.synchronize()

    net_o = graph_nets.all_nets(graph_nets.local_bases())[name]
    gb_o = R.GraphBatchRef([R.GraphRef(g.node_feat, g.node_info, g._Adj)])
    nets_o, _ = oracle([net_o], gb_o, keep_grads=True)
    loss_o = F.cross_entropy(nets_o[0](images), labels)
    loss_o.backward()

    assert abs(loss.item() - loss_o.item()) < 1e-4 * max(1.0, abs(loss_o.item())), (loss.item(), loss_o.item())
    po = dict(oracle.named_parameters())
    seen = 0
    for k, p in hip.named_parameters():
        go = po[k].grad
        if go is None or float(go.norm()) < 1e-7:
            continue
        assert p.grad is not None, k
        err = float((p.grad.cpu().double() - go.double()).norm())
        assert err < 2e-3 * float(go.norm()) + 1e-6, (k, err, float(go.norm()))
        seen += 1
    assert seen > 20


def test_training_steps_do_not_accumulate_memory():
    """A step's plan (workspace, flat gradients, index tables) must be released by reference counting once its
    backward has run: plan -> target modules -> predicted tensors -> autograd node -> plan was a cycle that leaked
    7 GB per step at ghn3xlm16 until Python's cycle collector ran."""
    import gc
    hip, _ = make_models(T_CFG, 7)
    hip.train()
    gc.collect()
    gc.disable()
    try:
        used = []
        for step in range(6):
            nets_h, gb_h, _, _ = synthetic_case([40], 4000 + step)
            nets_h = hip(nets_h, gb_h, keep_grads=True)
            loss = hip.predicted_param_norm() + sum(torch.norm(p) for p in list(nets_h[0].parameters())[:3])
            loss.backward()
            del nets_h, gb_h, loss
            torch.cuda.synchronize()
            used.append(torch.cuda.memory_allocated())
    finally:
        gc.enable()
    assert max(used[2:]) - min(used[2:]) < 0.25 * used[2], used


def test_repeated_runs_reuse_the_resolved_problem_tables():
    """ghn3_run keeps the resolved GEMM problem tables of its recent runs on the device (ghn3_ctx_cache_stats): the steps of a
    loop over one plan are served from that store -- and give the bits of the first step --, a different plan in between does
    not disturb it, and a run whose buffers moved (other output / gradient tensors at the same ops) resolves again instead of
    using a stale table."""
    from ghn3_amd import _lib as L
    hip, _ = make_models(T_CFG, 7)
    hip.train()
    ctx = L.context(0)
    nets_a, gb_a, _, _ = synthetic_case([40], 4100)
    nets_b, gb_b, _, _ = synthetic_case([33, 21], 4200)
    plan_a = hip.compile(nets_a, gb_a, training=True)
    plan_b = hip.compile(nets_b, gb_b, training=True)

    def step(plan, keep=None):
        torch.manual_seed(3)                                      # (the class-token rows of the positional encodings)
        out = hip._run_forward(plan)
        with torch.no_grad():                                     # (the predicted tensors: the gaps between them are not written)
            pred = torch.cat([out[p['offset']:p['offset'] + p['numel']] for p in plan.program.predicted])
        dout = torch.ones_like(out)
        grads = hip._run_backward(plan, dout)
        res = (pred, grads[0].clone(), plan.gflat.clone())
        if keep is not None:
            keep.append((out, plan.gflat))                        # (kept alive: the next step's tensors land elsewhere)
        return res

    first = step(plan_a)

    def same(got):
        assert torch.equal(first[0], got[0])
        for a, b in zip(first[1:], got[1:]):                      # (some gradient sums are accumulated with atomics)
            assert float((a - b).norm() / a.norm()) < 1e-6

    h0, m0 = ctx.cache_stats()
    for k in range(16):
        if k == 3:
            step(plan_b)
        same(step(plan_a))
    h1, m1 = ctx.cache_stats()
    assert h1 - h0 >= 2, (h0, m0, h1, m1)                         # (the allocator settles into a short period: misses, then hits -- typically 20+ of these 34 runs)
    keep = []
    for k in range(4):                                            # every step at new addresses: no stale table
        same(step(plan_a, keep))
    h2, m2 = ctx.cache_stats()
    assert m2 - m1 >= 4, (h1, m1, h2, m2)


def test_fused_predicted_param_norm_loss():
    """GHN3.predicted_param_norm (PARAM_NORM_FWD / BWD on the flat output, trainer.py:288-294) against the per-tensor
    torch.norm form: same value, same GHN gradients; scaled upstream gradient (predparam_wd) included."""
    hip, _ = make_models(T_CFG, 7)
    hip.train()
    grads = []
    for fused in (False, True):
        nets_h, gb_h, _, _ = synthetic_case([40], 4000)
        hip.zero_grad(set_to_none=True)
        nets_h = hip(nets_h, gb_h, keep_grads=True)
        if fused:
            loss = 3e-2 * hip.predicted_param_norm()
        else:
            loss = 3e-2 * sum(torch.norm(p, p='fro') for net in nets_h for p in net.parameters())
        loss.backward()
        torch.cuda.synchronize()
        grads.append((loss.item(), {k: p.grad.detach().clone() for k, p in hip.named_parameters()}))
    assert abs(grads[0][0] - grads[1][0]) < 1e-5 * abs(grads[0][0])
    for k in grads[0][1]:
        a, b = grads[1][1][k], grads[0][1][k]
        assert float((a - b).norm()) < 1e-5 * float(b.norm()) + 1e-7, k


def test_graph_with_more_than_1024_nodes():
    """N = 1100 (EfficientNet-B7-sized graphs exceed 1024 nodes): streamed two-pass attention forward, generic
    backward; head dim 24 like ghn3xlm16.  Forward and gradients vs the oracle."""
    cfg = dict(max_shape=(48, 48, 16, 16), num_classes=1000, hid=48, heads=2, layers=2, weight_norm=True, ve=True,
               layernorm=True)
    hip, oracle = make_models(cfg, 11)
    nets_h, gb_h, nets_o, gb_o = synthetic_case([1100], 1100000)
    hip.train()
    nets_h = hip(nets_h, gb_h, keep_grads=True)
    loss = sum(torch.norm(p, p='fro') for net in nets_h for p in net.parameters())
    loss.backward()
    torch.cuda.synchronize()
    assert hip.last_plan.program.N == 1100
    oracle.train()
    nets_o, pred_o = oracle(nets_o, gb_o, keep_grads=True)
    loss_o = sum(torch.norm(t, p='fro') for (_, _, _, t) in pred_o)
    loss_o.backward()
    pred_h = predicted_dict_hip(hip.last_plan, hip.last_plan.out)
    for k, (ind, attr, m, t) in enumerate(pred_o):
        e = rel_l2(pred_h[k].detach().cpu(), t.detach())
        assert e < 2e-5, (k, attr, tuple(t.shape), e)
    po = dict(oracle.named_parameters())
    for k, p in hip.named_parameters():
        go = po[k].grad
        err = float((p.grad.cpu().double() - go.double()).norm())
        # (gnn.0.attn.proj_e.2.bias has an analytically zero gradient -- softmax is shift invariant -- so both sides hold
        # rounding noise of ~1e-5 there: absolute floor)
        assert err < 3e-4 * float(go.norm()) + 5e-5, (k, err, float(go.norm()))


def test_index_mode_correct_matches_oracle():
    hip, oracle = make_models(recipe.TINY_CFG, recipe.TINY_SEED, index_mode='correct')
    nets_h, gb_h, nets_o, gb_o = tiny_case('b2')
    plan, flat = _run_forward(hip, nets_h, gb_h)
    with torch.no_grad():
        _, pred_o = oracle(nets_o, gb_o, assign=False)
    pred_h = predicted_dict_hip(plan, flat)
    for k, (ind, attr, m, t) in enumerate(pred_o):
        a, b = pred_h[k].cpu(), t
        if b.dim() == 3:
            a, b = a[:, 1:], b[:, 1:]
        assert rel_l2(a, b) < 2e-5, (k, attr)


T_CFG = dict(max_shape=(64, 64, 16, 16), num_classes=1000, hid=64, heads=8, layers=3, weight_norm=True, ve=True,
             layernorm=True)


@pytest.mark.parametrize('compute,tol_f,tol_g', [('f32', 2e-5, 3e-4), ('f16', 1e-3, 1e-3)])
def test_ghn3tm8_synthetic_forward_backward(compute, tol_f, tol_g):
    """BASELINE config 1/2 shape: ghn3tm8 on a seeded synthetic graph, forward + backward vs the oracle."""
    hip, oracle = make_models(T_CFG, 7, compute=compute)
    nets_h, gb_h, nets_o, gb_o = synthetic_case([48], 4800)
    hip.train()
    nets_h = hip(nets_h, gb_h, keep_grads=True)
    loss = sum(torch.norm(p, p='fro') for net in nets_h for p in net.parameters())
    loss.backward()
    torch.cuda.synchronize()
    oracle.train()
    nets_o, pred_o = oracle(nets_o, gb_o, keep_grads=True)
    loss_o = sum(torch.norm(t, p='fro') for (_, _, _, t) in pred_o)
    loss_o.backward()
    pred_h = predicted_dict_hip(hip.last_plan, hip.last_plan.out)
    for k, (ind, attr, m, t) in enumerate(pred_o):
        e = rel_l2(pred_h[k].detach().cpu(), t.detach())
        assert e < tol_f, (k, attr, tuple(t.shape), e)
    po = dict(oracle.named_parameters())
    for k, p in hip.named_parameters():
        go = po[k].grad
        err = float((p.grad.cpu().double() - go.double()).norm())
        assert err < tol_g * float(go.norm()) + 1e-5, (k, err, float(go.norm()))


def test_size_independent_properties_at_scale():
    """BASELINE config 3 per GPU at FULL size -- ghn3lm8 (hid 256, 12 layers, 16 heads, 214.7 M parameters), one synthetic
    200-node graph: properties that do not need the oracle at full size."""
    from ghn3_amd import GHN3
    from ghn3_amd.synthetic import synthetic_batch
    cfg = dict(max_shape=(256, 256, 16, 16), num_classes=1000, hid=256, heads=16, layers=12, weight_norm=True,
               ve=True, layernorm=True)
    torch.manual_seed(0)
    hip = GHN3(**cfg).to('cuda')
    gb, nets = synthetic_batch([200], 200000)
    plan = hip.compile(nets, gb, training=False)
    with torch.no_grad():
        flat1 = hip._run_forward(plan).clone()
        flat2 = hip._run_forward(plan)
    torch.cuda.synchronize()
    # idempotence / determinism of the forward (per predicted tensor: the alignment gaps of the flat buffer are
    # uninitialised memory)
    for p in plan.program.predicted:
        assert torch.equal(flat1[p['offset']:p['offset'] + p['numel']], flat2[p['offset']:p['offset'] + p['numel']])
    # every predicted element is finite and 1-D predictions respect their ranges (sigmoid / tanh, nn.py:587-590)
    for p in plan.program.predicted:
        t = flat2[p['offset']:p['offset'] + p['numel']]
        assert torch.isfinite(t).all()
        if len(p['tile_shape']) == 1:
            if p['is_w']:
                assert (t >= 0).all() and (t <= 2).all()
            else:
                assert (t >= -1).all() and (t <= 1).all()
    # tiling is periodic: a tensor wider than the tile repeats with period = tile extent (nn.py:466-485)
    for p, d in zip(plan.program.predicted, range(len(plan.program.predicted))):
        shp = p['tile_shape']
        if len(shp) == 4 and shp[0] > 256:
            t = flat2[p['offset']:p['offset'] + p['numel']].view(shp)
            assert torch.equal(t[:shp[0] - 256], t[256:])
            break
    n_pred = sum(p['numel'] for p in plan.program.predicted)
    assert n_pred == nets[0].num_params()
    assert sum(p.numel() for p in hip.parameters()) == 214668960          # ghn3lm8
    # forward + backward at full size: finite gradients for every parameter, bit-identical on a rerun (no float atomics)
    hip.train()
    plan_t = hip.compile(nets, gb, training=True)
    hip._run_forward(plan_t)
    dout = torch.randn(plan_t.program.out_numel, device='cuda') * 1e-3
    hip._run_backward(plan_t, dout)
    torch.cuda.synchronize()
    g1 = plan_t.gflat.clone()
    hip._run_forward(plan_t)
    hip._run_backward(plan_t, dout)
    torch.cuda.synchronize()
    assert torch.isfinite(g1).all() and float(g1.abs().sum()) > 0
    assert torch.equal(g1, plan_t.gflat)


@pytest.mark.parametrize('hid,heads,nodes', [(96, 4, [40]), (64, 4, [70, 33]), (48, 16, [30])])
def test_head_dims_of_released_models(hid, heads, nodes):
    """Head dims 24 (ghn3xlm16), 16 (ghn3lm8) and an odd one (3) through the specialised attention kernels and
    the small-GEMM kernel: forward + backward vs the oracle, B = 1 and a ragged B = 2 batch."""
    cfg = dict(max_shape=(hid, hid, 16, 16), num_classes=100, hid=hid, heads=heads, layers=2, weight_norm=True,
               ve=True, layernorm=True)
    hip, oracle = make_models(cfg, 11)
    nets_h, gb_h, nets_o, gb_o = synthetic_case(nodes, 9100)
    hip.train()
    nets_h = hip(nets_h, gb_h, keep_grads=True)
    loss = sum(torch.norm(p, p='fro') for net in nets_h for p in net.parameters())
    loss.backward()
    torch.cuda.synchronize()
    oracle.train()
    nets_o, pred_o = oracle(nets_o, gb_o, keep_grads=True)
    loss_o = sum(torch.norm(t, p='fro') for (_, _, _, t) in pred_o)
    loss_o.backward()
    pred_h = predicted_dict_hip(hip.last_plan, hip.last_plan.out)
    for k, (ind, attr, m, t) in enumerate(pred_o):
        e = rel_l2(pred_h[k].detach().cpu(), t.detach())
        assert e < 2e-5, (k, attr, tuple(t.shape), e)
    po = dict(oracle.named_parameters())
    for k, p in hip.named_parameters():
        go = po[k].grad
        err = float((p.grad.cpu().double() - go.double()).norm())
        assert err < 3e-4 * float(go.norm()) + 1e-5, (k, err, float(go.norm()))


def _resnet_fixture_check(depth, variant, compute, tol, n_expected=None):
    """HIP forward at a released GHN-3 size on the hand-written torchvision-shaped ResNet graph vs the golden
    produced by the REFERENCE GHN3 class on CPU (tests/golden/make_golden.py resnet): per predicted tensor the
    Frobenius norm and 2048 sampled elements."""
    from ghn3_amd import GHN3, Graph, GraphBatch
    tag = 'vit_b16' if depth == 'vit' else 'resnet%d' % depth
    gold = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', '%s_%s.npz' % (tag, variant)))
    hid, layers, heads = recipe.VARIANTS[variant]
    cfg = dict(max_shape=(hid, hid, 16, 16), num_classes=1000, hid=hid, heads=heads, layers=layers,
               weight_norm=True, ve=True, layernorm=True)
    hip = GHN3(**cfg, compute=compute)
    shapes = {k: tuple(v.shape) for k, v in hip.state_dict().items()}
    sd = recipe.seeded_state_dict(shapes, seed=recipe.RESNET_SEED)
    hip.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    del sd
    hip = hip.to('cuda').eval()
    spec = recipe.vit_b16_spec() if depth == 'vit' else recipe.resnet_spec(depth)
    net = recipe.build_torch_net(spec)
    nf, info, A = recipe.graph_arrays(spec)
    gb = GraphBatch([Graph(node_feat=nf, node_info=info, A=A)], dense=True)
    with torch.no_grad():
        net, emb = hip(net, gb, return_embeddings=True, bn_track_running_stats=True)
    torch.cuda.synchronize()
    assert rel_l2(emb.cpu().numpy(), gold['emb']) < (1e-4 if compute == 'f32' else tol)
    total, worst = 0, 0.0
    for name, p in recipe.named_predicted(net):
        total += p.numel()
        # (quirk Q3: row 0 of a predicted positional encoding is a random class-token row -> not compared)
        v = (p.detach()[:, 1:] if p.dim() == 3 else p.detach()).reshape(-1)
        idx = recipe.sample_indices(v.numel(), recipe.RESNET_SAMPLES, seed=len(name))
        got = v[torch.from_numpy(idx).to(v.device)].cpu().numpy()
        ref = gold['pred/%s/sample' % name]
        e = rel_l2(got, ref)
        worst = max(worst, e)
        assert e < tol, (name, tuple(p.shape), e)
        n_ref = float(gold['pred/%s/norm' % name][0])
        assert abs(float(v.double().norm()) - n_ref) < tol * n_ref, (name, float(v.norm()), n_ref)
    assert total == int(gold['meta/n_predicted'][0]) == {18: 11689512, 50: 25557032, 'vit': 86566888}[depth]
    if depth != 'vit':
        # eval_ghn.py:147-169 / nn.py:783-796: the total-norm known-answer check, executed against the norm of the
        # REFERENCE's own prediction for these seeded weights (the released checkpoints are not obtainable offline)
        from ghn3_amd import norm_check
        names = [n for n, _ in recipe.named_predicted(net)]
        ref_total = float(np.sqrt(sum(float(gold['pred/%s/norm' % n][0]) ** 2 for n in names)))
        total_norm, expected, ok = norm_check(net, arch=tag, ghn3_name='ghn3xlm16.pt', expected=ref_total)
        assert ok and abs(total_norm - ref_total) < 1e-2, (total_norm, ref_total)
    print('%s %s %s: worst sampled rel-L2 error %.2e' % (tag, variant, compute, worst))


@pytest.mark.parametrize('compute,tol', [('f32', 1e-4), ('f16', 1e-3)])
def test_resnet18_ghn3tm8_matches_reference_golden(compute, tol):
    """BASELINE config 1: ghn3tm8 forward on the torchvision.resnet18-shaped graph (53 nodes, 11,689,512 params)."""
    _resnet_fixture_check(18, 'ghn3tm8', compute, tol)


@pytest.mark.parametrize('compute,tol', [('f32', 1e-4), ('f16', 1e-3)])
def test_resnet50_ghn3xlm16_matches_reference_golden(compute, tol):
    """BASELINE config 4 / north star: ghn3xlm16 predicting the ResNet-50 weight tensors (127 nodes, 25,557,032
    params; output channels up to 2048 are tiled from the 384-wide decoder) within 1e-3 of the reference on CPU."""
    _resnet_fixture_check(50, 'ghn3xlm16', compute, tol)


@pytest.mark.parametrize('compute,tol', [('f32', 1e-4), ('f16', 1e-3)])
def test_vit_b16_ghn3xlm16_matches_reference_golden(compute, tol):
    """BASELINE config 4: ghn3xlm16 predicting the ViT-B/16 weight tensors (163 nodes, 86,566,888 parameters:
    16x16 patch embedding = 256 decoder rows, (1,197,768) positional encoding, MultiheadAttention in_proj / out_proj,
    768 / 3072-wide linears tiled from the 384-wide decoder) vs the reference on CPU."""
    _resnet_fixture_check('vit', 'ghn3xlm16', compute, tol)


def test_split_backward_with_overlapped_gradient_reduction():
    """The N > 1 execution path on one GPU: backward program run in three parts (GHN3_OP_DETACH), the W2 and the
    other decoder gradients all-reduced (1-rank RCCL group) from a communication stream that waits on the side stream while the
    Graphormer backward runs.  Gradients must equal the single-run path (fp32 exchange: bit-identical up to the
    atomics' order; bf16 on the wire: 2^-8)."""
    import socket
    import torch.distributed as dist
    from ghn3_amd.ddp_utils import FlatGradReducer
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        hip, _ = make_models(T_CFG, 7, compute='f16')
        nets_h, gb_h, _, _ = synthetic_case([48], 4800)
        hip.train()
        plan = hip.compile(nets_h, gb_h, training=True)
        hip._run_forward(plan)
        dout = torch.randn(plan.program.out_numel, device='cuda') * 1e-3
        hip._run_backward(plan, dout)
        torch.cuda.synchronize()
        ref = plan.gflat.clone()
        # both exchange algorithms; with force=True the mesh path really issues its all-to-all / all-gather in the 1-rank
        # RCCL group and runs its local passes as library ops (GHN3_OP_WIRE_PACK, GHN3_OP_RANK_REDUCE)
        for algo in ('allreduce', 'mesh', 'rsag'):
            for compress, tol in ((None, 2e-5), ('bf16', 1e-2)):
                hip._run_backward(plan, dout, reducer=FlatGradReducer(compress=compress, force=True, algo=algo))
                torch.cuda.synchronize()
                err = float((plan.gflat - ref).norm() / ref.norm())
                assert err < tol, (algo, compress, err)
            lo, hi = hip.decoder_grad_range(plan.program)
            assert 0 < lo < hi <= ref.numel() and (hi - lo) > 0.5 * ref.numel()
        # the sharded optimizer step on the same path (reduce-scatter only, update of the owned shard, all-gather of the
        # parameters; in a 1-rank group the shard is everything): the HIP ops over the shard ranges give the parameters and
        # moments of the plain fused step bit for bit (no clip: the two sum the squared norm in different orders)
        from ghn3_amd import FusedAdamW
        from ghn3_amd.optim import ShardedAdamW
        twin, _ = make_models(T_CFG, 7, compute='f16')
        twin.train()
        opt_s = ShardedAdamW(ghn=hip, lr=1e-2, weight_decay=0.05, max_grad_norm=0.0)
        opt_f = FusedAdamW(twin, lr=1e-2, weight_decay=0.05, max_grad_norm=0.0)
        for _ in range(2):
            red = FlatGradReducer(force=True, algo='rsag', gather=False, chunk_bytes=1 << 20)
            hip._run_backward(plan, dout, reducer=red)
            assert red.owned and sum(b - a for a, b in red.owned + red.replicated) == ref.numel()
            n_s = opt_s.step(plan.gflat, red)
            n_f = opt_f.step(plan.gflat.clone())
            torch.cuda.synchronize()
            assert abs(float(n_s) - float(n_f)) <= 1e-5 * float(n_f)
            assert torch.equal(hip._flat, twin._flat) and torch.equal(opt_s.exp_avg, opt_f.exp_avg) and \
                torch.equal(opt_s.exp_avg_sq, opt_f.exp_avg_sq)
            hip._run_forward(plan)                      # (the copies of the updated weights are re-cast here)
        # three parts: ... W2 gradient | rest of the decoder | Graphormer
        # (+ two DETACH records, + the MARK / WAIT pair in front of the weight gradient when it is issued first)
        assert len(plan.program.bwd_parts) == 3 and sum(len(o) for o, _ in plan.program.bwd_parts) == \
            len(plan.program.bwd_ops) + 2 + 2 * int(plan.program.ddp_wgrad_first)
        # the local passes alone, against torch: W-way fp32 sum of bf16 chunks in rank order, pack / unpack round trip
        from ghn3_amd.ddp_utils import _hip_ops
        from ghn3_amd import _lib as L
        W, per = 5, 1003
        x = torch.randn(W * per, device='cuda')
        xb = x.to(torch.bfloat16)
        out = torch.empty(per, dtype=torch.bfloat16, device='cuda')
        st = torch.cuda.current_stream().cuda_stream
        _hip_ops([(L.OP_RANK_REDUCE, (0, 1), (per, W, 1, 1), 1.0 / W)], [out.data_ptr(), xb.data_ptr()], st)
        want = (torch.sum(xb.view(W, per), dim=0, dtype=torch.float32) / W).to(torch.bfloat16)
        assert torch.equal(out, want)
        packed = torch.full((W * per + 13,), 7, dtype=torch.bfloat16, device='cuda')
        _hip_ops([(L.OP_WIRE_PACK, (0, 1), (W * per, W * per + 13, 0), 0.0)], [packed.data_ptr(), x.data_ptr()], st)
        assert torch.equal(packed[:W * per], xb) and float(packed[W * per:].abs().sum()) == 0.0
        back = torch.empty(W * per, device='cuda')
        _hip_ops([(L.OP_WIRE_PACK, (0, 1), (W * per, W * per, 1), 0.0)], [back.data_ptr(), packed.data_ptr()], st)
        assert torch.equal(back, xb.float())
        # GHN3_OP_TRANSPOSE32: batched fp32 transpose with leading dimensions and batch strides
        src = torch.randn(3, 37, 52, device='cuda')
        dst = torch.zeros(3, 50, 40, device='cuda')
        _hip_ops([(L.OP_TRANSPOSE32, (0, 1), (37, 50, 52, 40, 3, 37 * 52, 50 * 40), 0.0)], [dst.data_ptr(), src.data_ptr()], st)
        torch.cuda.synchronize()
        assert torch.equal(dst[:, :, :37], src[:, :, :50].transpose(1, 2)) and float(dst[:, :, 37:].abs().sum()) == 0.0
    finally:
        dist.destroy_process_group()


def test_distributed_data_parallel_wrapper_gives_the_same_gradients():
    """The reference wraps the GHN in DistributedDataParallel (trainer.py:136).  The flat-buffer model is an ordinary
    nn.Module whose parameters receive .grad through autograd, so the wrapper works on it (1-rank RCCL group; gloo cannot
    reduce device tensors): same predicted tensors and the same gradients as the bare model and as the model with the
    in-backward FlatGradReducer."""
    import socket
    import torch.distributed as dist
    from torch.nn.parallel import DistributedDataParallel
    from ghn3_amd.ddp_utils import FlatGradReducer
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        hip, _ = make_models(T_CFG, 7)
        hip.train()

        def step(model, reducer=None):
            hip.zero_grad(set_to_none=True)
            hip.grad_reducer = reducer
            nets_h, gb_h, _, _ = synthetic_case([40], 4000)
            nets_h = model(nets_h, gb_h, keep_grads=True)
            loss = sum(p.square().sum() for p in list(nets_h[0].parameters())[:12]) + hip.predicted_param_norm()
            loss.backward()
            torch.cuda.synchronize()
            return loss.item(), {k: p.grad.detach().clone() for k, p in hip.named_parameters() if p.grad is not None}

        loss0, g0 = step(hip)
        loss1, g1 = step(hip, FlatGradReducer(compress=None, force=True))
        ddp = DistributedDataParallel(hip, device_ids=[torch.cuda.current_device()])
        loss2, g2 = step(ddp)
        assert abs(loss0 - loss1) < 1e-6 * abs(loss0) and abs(loss0 - loss2) < 1e-6 * abs(loss0)
        assert set(g0) == set(g1) == set(g2) and len(g0) > 20
        for k in g0:                       # (fp32-mode split-K sums are atomic: equal up to the order of the additions)
            # (+ 1e-5: the bias in front of a softmax has a zero gradient in exact arithmetic, rounding noise here)
            bound = 1e-4 * float(g0[k].norm()) + 1e-5
            assert float((g0[k] - g1[k]).norm()) < bound, k
            assert float((g0[k] - g2[k]).norm()) < bound, k
    finally:
        hip.grad_reducer = None
        dist.destroy_process_group()


def test_fused_adamw_step_matches_torch():
    """clip_grad_norm_ + torch.optim.AdamW (trainer.py:356-381) as two kernels over the flat
    parameter / gradient buffers vs the PyTorch CPU implementation, 3 steps with clipping active."""
    from ghn3_amd import FusedAdamW
    hip, _ = make_models(T_CFG, 7)
    ref = [p.detach().cpu().clone().requires_grad_(True) for p in hip._slot_params()]
    opt_ref = torch.optim.AdamW(ref, lr=3e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05)
    opt = FusedAdamW(hip, lr=3e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.05, max_grad_norm=5.0)
    gen = torch.Generator().manual_seed(3)
    for step in range(3):
        gflat = torch.zeros_like(hip._flat)
        for p, r, off in zip(hip._slot_params(), ref, hip._offs):
            g = torch.randn(r.shape, generator=gen) * (0.5 + step)
            r.grad = g.clone()
            gflat[int(off):int(off) + g.numel()] = g.reshape(-1).cuda()
        norm_ref = torch.nn.utils.clip_grad_norm_(ref, 5.0)
        opt_ref.step()
        norm = opt.step(gflat)
        torch.cuda.synchronize()
        assert abs(float(norm) - float(norm_ref)) < 1e-4 * float(norm_ref)
        for p, r in zip(hip._slot_params(), ref):
            assert rel_l2(p.detach().cpu().numpy(), r.detach().numpy()) < 2e-6


def test_optimizer_state_interchanges_with_torch_adamw(tmp_path):
    """Checkpoint compatibility (trainer.py:413-432): a torch.optim.AdamW state over ghn.parameters() loads into
    FusedAdamW (and back) and training continues identically; save_checkpoint writes the reference trainer's file
    layout, which from_pretrained reads."""
    from ghn3_amd import FusedAdamW, from_pretrained, save_checkpoint
    hip, _ = make_models(T_CFG, 7)
    params = list(hip.parameters())
    ref = [p.detach().cpu().clone().requires_grad_(True) for p in params]
    kw = dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.02)
    opt_ref = torch.optim.AdamW(ref, **kw)
    gen = torch.Generator().manual_seed(5)

    def grads():
        gs = [torch.randn(r.shape, generator=gen) for r in ref]
        gflat = torch.zeros_like(hip._flat)
        slot_of = {id(p): k for k, p in enumerate(hip._slot_params())}
        for p, g in zip(params, gs):
            o = int(hip._offs[slot_of[id(p)]])
            gflat[o:o + g.numel()] = g.reshape(-1).cuda()
        for r, g in zip(ref, gs):
            r.grad = g.clone()
        return gflat

    for _ in range(2):                                   # two reference steps build up a state
        grads()
        opt_ref.step()
    with torch.no_grad():
        for p, r in zip(params, ref):
            p.copy_(r.cuda())
    opt = FusedAdamW(hip, lr=1.0)                        # (hyper-parameters come from the loaded state)
    opt.load_state_dict(opt_ref.state_dict())
    assert opt.steps == 2 and opt.lr == kw['lr'] and opt.betas == kw['betas']
    for _ in range(2):                                   # continue on both sides
        gflat = grads()
        opt_ref.step()
        opt.step(gflat)
    torch.cuda.synchronize()
    for p, r in zip(params, ref):
        assert rel_l2(p.detach().cpu().numpy(), r.detach().numpy()) < 3e-6
    sd = opt.state_dict()
    sd_ref = opt_ref.state_dict()
    assert sd['param_groups'][0]['params'] == sd_ref['param_groups'][0]['params']
    for i in sd_ref['state']:
        assert float(sd['state'][i]['step']) == float(sd_ref['state'][i]['step']) == 4.0
        assert rel_l2(sd['state'][i]['exp_avg'].cpu().numpy(), sd_ref['state'][i]['exp_avg'].numpy()) < 3e-6
        assert rel_l2(sd['state'][i]['exp_avg_sq'].cpu().numpy(), sd_ref['state'][i]['exp_avg_sq'].numpy()) < 3e-6
    opt_back = torch.optim.AdamW(ref, **kw)              # ... and back into torch
    opt_back.load_state_dict({'state': {i: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in st.items()}
                                        for i, st in sd['state'].items()}, 'param_groups': sd['param_groups']})
    path = save_checkpoint(str(tmp_path / 'checkpoint.pt'), hip, opt, epoch=3, step=17, config={'config': dict(T_CFG)})
    ck = torch.load(path, map_location='cpu')
    assert ck['epoch'] == 3 and ck['step'] == 17 and set(ck) >= {'state_dict', 'optimizer', 'config'}
    again = from_pretrained(path)
    for (k, a), (_, b) in zip(sorted(again.state_dict().items()), sorted(hip.state_dict().items())):
        assert torch.equal(a, b.cpu()), k


@pytest.mark.skipif(not os.environ.get('GHN3_CKPT'), reason='set GHN3_CKPT=/path/to/ghn3xlm16.pt (released checkpoint) '
                    'and GHN3_RESULTS_JSON to run the known-answer check of nn.py:783-861')
def test_released_checkpoint_known_answer():
    """With a released checkpoint at hand: from_pretrained -> predict the torchvision-shaped ResNet-50 -> total norm
    against the `ghn3-paramnorm` entry of ghn3_results.json (108.4530 for ghn3xlm16; nn.py:783-796).  This also pins the
    parts of the path only ppuda defines (shape vocabulary, primitive order), see DESIGN.md 5."""
    from ghn3_amd import from_pretrained, norm_check, Graph, GraphBatch
    ckpt = os.environ['GHN3_CKPT']
    ghn = from_pretrained(ckpt, compute='f32').to('cuda').eval()
    spec = recipe.resnet_spec(50)
    net = recipe.build_torch_net(spec)
    nf, info, A = recipe.graph_arrays(spec)
    with torch.no_grad():
        net = ghn(net, GraphBatch([Graph(node_feat=nf, node_info=info, A=A)], dense=True), bn_track_running_stats=True)
    path = os.environ.get('GHN3_RESULTS_JSON', os.path.join(GOLD, 'ghn3_results.json'))
    total, expected, ok = norm_check(net, arch='resnet50', ghn3_name=os.path.basename(ckpt), path=path)
    assert ok, (total, expected)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs 2 GPUs (the driver runs the multi-GPU bench itself)')
def test_two_rank_rccl_bench_line():
    """`python bench.py --gpus 2` starts its own ranks (fresh processes), exchanges the flat gradients over RCCL with the
    overlapped reducer and prints one JSON line for the whole job."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '1',
                          '--model', 'ghn3tm8', '--nodes', '64', '--no-cpu-baseline', '--no-extras'],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line['n_gpus'] == 2 and line['value'] > 0 and line['config']['parallelism'] == 'dp2'


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain `python bench.py` run prints the headline line alone (nothing behind --full) and, with --dump-outputs, writes
    what its last timed step computed: finite float arrays within 64 MB, the loss equal to the sum of the per-tensor norms it
    was formed from, those norms equal to the predicted tensors' own, and the same values again in a second run."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(d):
        out = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '1',
                              '--model', 'ghn3tm8', '--nodes', '64', '--dump-outputs', str(d)],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return json.loads(out.stdout.strip().splitlines()[-1]), {p.stem: np.load(p) for p in d.glob('*.npy')}
    line, a = run(tmp_path / 'a')
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line, k
    assert line['steps'] == 4 and line['warmup'] == 1 and line['ms_per_step'] > 0 and line['value'] > 0
    assert not {'roofline', 'cpu_baseline', 'forward', 'train_step', 'f32_mode'} & set(line)
    assert set(a) == {'loss', 'loss_terms', 'predicted_sample', 'predicted_norms', 'grad_sample', 'grad_norms'}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert abs(float(a['loss'][0]) - float(a['loss_terms'].astype(np.float64).sum())) <= 1e-5 * abs(float(a['loss'][0]))
    np.testing.assert_allclose(a['loss_terms'], a['predicted_norms'], rtol=1e-4)
    assert float(np.abs(a['grad_norms']).max()) > 0
    _, b = run(tmp_path / 'b')
    for k, v in a.items():
        np.testing.assert_allclose(b[k], v, rtol=1e-5, atol=1e-6 * float(np.abs(v).max()), err_msg=k)


def test_graft_entry_smoke():
    """The driver's smoke(): tiny forward + backward through the public API, checked against the oracle."""
    import __graft_entry__ as g
    g.smoke()


@pytest.mark.parametrize('bf16', [False, True])
def test_cast16_from_a_16bit_source_matches_the_interpreter(ctx, bf16):
    """GHN3_CAST_SRC16 (round 4): transposed band copies + column-sum slots re-laid out from a scaled 16-bit matrix (what
    GHN3_OP_TILE_BWD's direct route leaves) -- bit for bit what the numpy interpreter of tests/program_interp.py produces,
    incl. the source column map, tight row padding and ragged edges."""
    from ghn3_amd import _lib as L
    from program_interp import Interp
    rs = np.random.RandomState(3 + bf16)
    rows, ld_src, amax = 150, 1216, 0.0371
    sc = Interp.pow2_scale(amax)
    src32 = (rs.standard_normal((rows, ld_src)) * amax / 4).astype(np.float32)
    src16 = Interp.to16(src32 * np.float32(sc), bf16)
    n_src = rows * ld_src
    # descriptors: (first row, n rows, band i_lo, band width, o rows, i of the row layout)
    specs = [(0, 70, 0, 32, 9, 128), (70, 80, 32, 96, 5, 128), (3, 37, 128, 64, 4, 192), (100, 50, 0, 8, 20, 8)]
    descs = np.zeros(len(specs), dtype=L.CAST_DT)
    dst_off, part_off, blocks, ktot = (n_src + 63) // 64 * 64, 0, 0, 256
    for D, (r0, nr, i_lo, bw, o, i_) in zip(descs, specs):
        cols = o * bw
        D['src_off'], D['rows'], D['cols'], D['ld_src'] = r0 * ld_src + i_lo, nr, cols, ld_src
        D['src_q'], D['src_s'] = bw, i_
        D['dstT_off'], D['ld_dstT'] = dst_off, ktot
        D['part_off'] = part_off
        D['flags'] = (L.CAST_TRANSPOSED | (L.CAST_TRANSPOSED_BF16 if bf16 else 0) | L.CAST_COLSUM | L.CAST_COLSUM_PARTS |
                      L.CAST_SCALED | L.CAST_TIGHT | L.CAST_SRC16)
        D['block_start'] = blocks
        blocks += ((nr + 63) // 64) * ((cols + 63) // 64)
        dst_off += cols * ktot
        part_off += ((nr + 63) // 64) * cols
    buf16 = np.zeros(dst_off + 256, dtype=np.uint16)
    buf16[:n_src] = src16.reshape(-1)
    parts = np.zeros(part_off + 64, dtype=np.float32)
    am = np.asarray([amax] + [0] * 15, dtype=np.float32)
    op = np.zeros(1, dtype=L.OP_DT)
    op['r']['buf'][:] = -1
    op['kind'] = L.OP_CAST16
    for j, b in enumerate((0, 1, 2, 3, 4)):
        op['r']['buf'][0][j] = b
    op['i'][0][:3] = (len(specs), blocks, 0)
    # CPU
    host = [np.zeros(64, np.uint8), buf16.copy().view(np.uint8), descs.copy().view(np.uint8).reshape(-1),
            parts.copy().view(np.uint8), am.copy().view(np.uint8)]
    Interp(host).run(op, None)
    # GPU
    dev = [torch.zeros(64, dtype=torch.uint8, device='cuda')] + \
        [torch.from_numpy(a.copy().view(np.uint8).reshape(-1)).cuda() for a in (buf16, descs, parts, am)]
    ptrs = np.asarray([t.data_ptr() for t in dev], dtype=np.uint64)
    ctx.run(op, np.zeros(0, dtype=L.PROBLEM_DT), ptrs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got16 = dev[1].cpu().numpy().view(np.uint16)
    exp16 = host[1].view(np.uint16)
    assert (got16[:n_src] == src16.reshape(-1)).all()
    bad = np.nonzero(got16 != exp16)[0]
    assert bad.size == 0, (bad[:10], got16[bad[:10]], exp16[bad[:10]])
    gp, ep = dev[3].cpu().numpy().view(np.float32), host[3].view(np.float32)
    assert np.abs(gp - ep).max() <= 1e-6 * np.abs(ep).max()


@pytest.mark.parametrize('N,H,C,nn', [(256, 16, 384, [256]), (200, 16, 384, [200, 131]), (97, 8, 64, [97]), (33, 4, 128, [20, 33]),
                                      (64, 16, 48, [64])])
def test_staged_attention_backward_equals_the_general_kernel(ctx, N, H, C, nn):
    """attn_bwd_staged_kernel (operands through LDS, graphs of up to 256 nodes) against attn_bwd_kernel (operands straight
    from memory): same MFMAs in the same order -> the same bits, incl. padded graphs, the accumulated edge-bias gradient and
    the reported max |dBias|.  (C / H = 3 is not a multiple of 4: both calls take the general kernel there.)"""
    from ghn3_amd import _lib as L
    B = len(nn)
    g = torch.Generator(device='cuda').manual_seed(N * 7 + H)
    qkv = torch.randn(B * N, 3 * C, device='cuda', generator=g)
    bias = torch.randn(B, H, N, N, device='cuda', generator=g)
    dO = torch.randn(B * N, C, device='cuda', generator=g)
    P = torch.zeros(B, H, N, N, device='cuda')
    out = torch.zeros(B * N, C, device='cuda')
    n_nodes = torch.tensor(nn, dtype=torch.int32, device='cuda')
    res = []
    for general in (0, 1):
        dqkv = torch.full((B * N, 3 * C), float('nan'), device='cuda')
        dB = torch.full((B, H, N, N), 0.25, device='cuda')
        amax = torch.zeros(4, device='cuda')
        bufs = [out, qkv, bias, P, n_nodes, dqkv, dO, dB, amax]
        ptrs = np.asarray([t.data_ptr() for t in bufs], dtype=np.uint64)
        ops = np.zeros(2, dtype=L.OP_DT)
        ops['r']['buf'][:] = -1
        ops[0]['kind'] = L.OP_ATTN_FWD
        ops[0]['r']['buf'][:5] = (0, 1, 2, 3, 4)
        ops[0]['i'][:4] = (B, N, C, H)
        ops[1]['kind'] = L.OP_ATTN_BWD
        ops[1]['r']['buf'][:8] = (5, 6, 1, 3, 0, 8, 7, 4)
        ops[1]['i'][:5] = (B, N, C, H, general)
        ctx.run(ops, np.zeros(0, dtype=L.PROBLEM_DT), ptrs, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        res.append((dqkv.clone(), dB.clone(), float(amax[0])))
    (a, ab, am), (b, bb, bm) = res
    for k, n_ in enumerate(nn):                                  # rows of padded nodes are not written
        assert torch.isfinite(a[k * N:k * N + n_]).all()
    assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    assert torch.equal(ab, bb)
    assert am == bm and abs(am - float(ab.abs().max())) <= 1e-6 * am
