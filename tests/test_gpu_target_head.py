"""
The end of the target networks on the fused HIP op families of ghn3_amd/csrc/tnet_head.hip: the classifier head (global
average pool or flatten + `Linear (ReLU Dropout Linear)*`, target_ops.ClassifierHead) and the meta-batch cross-entropy with
its top-1 / top-5 hit counts (target_ops.meta_cross_entropy).  Each against float64 torch on the CPU, determinism, the cases
that keep the stock path, whole sampled networks against the stock path and one Trainer.update without any stock head or
loss operator.

Tolerances: every product is an exact fp32 product with fp32 accumulation (fp32 matrix cores), in another summation order
than torch's: 2e-5 of the output's scale, 1e-4 of a gradient's.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _ref_head(x, ws, bs, masks, ps, glob_avg):
    f = x.mean((2, 3)) if glob_avg else x.reshape(x.shape[0], -1)
    h = f @ ws[0].t() + bs[0]
    for j in range(1, len(ws)):
        a = torch.relu(h)
        if masks[j - 1] is not None:
            a = a * masks[j - 1].double() / (1.0 - ps[j - 1])
        h = a @ ws[j].t() + bs[j]
    return h


CASES = [   # B, C, H, W, channels_last, glob_avg, widths after the features, dropout masks
    (4, 64, 4, 4, False, True, [10], False),
    (64, 256, 8, 8, True, True, [64, 10], True),
    (64, 128, 7, 7, False, True, [512, 1000], False),
    (256, 512, 4, 4, True, True, [512, 64, 10], True),
    (64, 32, 4, 4, False, False, [64, 10], False),
    (64, 32, 4, 4, True, False, [256, 1000], True),
    (256, 64, 8, 8, False, True, [1000], False),
    (4, 48, 2, 2, True, False, [10], False),
    (300, 64, 2, 2, True, True, [128, 64, 10], True),
]


def _case_tensors(case, seed):
    B, C, H, W, cl, g, tail, masked = case
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen, dtype=torch.float64)
    dims = [C if g else C * H * W] + tail
    ws = [torch.randn(dims[j + 1], dims[j], generator=gen, dtype=torch.float64) / dims[j] ** 0.5 for j in range(len(tail))]
    bs = [0.1 * torch.randn(dims[j + 1], generator=gen, dtype=torch.float64) for j in range(len(tail))]
    masks = [(torch.rand(B, dims[j + 1], generator=gen) > 0.3).to(torch.uint8) if masked else None
             for j in range(len(tail) - 1)]
    ps = [0.3 if masked else 0.0] * (len(tail) - 1)
    G = torch.randn(B, dims[-1], generator=gen, dtype=torch.float64)
    return x, ws, bs, masks, ps, G


def _run_fused(case, x, ws, bs, masks, ps, G):
    from ghn3_amd import target_ops as T
    cl, g = case[4], case[5]
    xd = x.float().cuda()
    if cl:
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_(True)
    wd = [w.float().cuda().requires_grad_(True) for w in ws]
    bd = [b.float().cuda().requires_grad_(True) for b in bs]
    md = [None if m is None else m.cuda() for m in masks]
    y = T.classifier_head(xd, wd, bd, md, ps, glob_avg=g)
    assert type(y.grad_fn).__name__ == 'ClassifierHeadBackward'
    y.backward(G.float().cuda())
    torch.cuda.synchronize()
    return y.detach(), xd.grad, [w.grad for w in wd], [b.grad for b in bd]


@pytest.mark.parametrize('case', CASES)
def test_head_matches_float64(case):
    x, ws, bs, masks, ps, G = _case_tensors(case, seed=len(case[6]) * 100 + case[0])
    y, dx, dws, dbs = _run_fused(case, x, ws, bs, masks, ps, G)
    xr = x.clone().requires_grad_(True)
    wr = [w.clone().requires_grad_(True) for w in ws]
    br = [b.clone().requires_grad_(True) for b in bs]
    yr = _ref_head(xr, wr, br, masks, ps, case[5])
    yr.backward(G)
    assert _rel(y.cpu(), yr.detach()) < 2e-5, _rel(y.cpu(), yr.detach())
    if case[4]:
        assert dx.is_contiguous(memory_format=torch.channels_last)
    assert _rel(dx.cpu(), xr.grad) < 1e-4, _rel(dx.cpu(), xr.grad)
    for a, b in zip(dws + dbs, [w.grad for w in wr] + [b.grad for b in br]):
        assert a.shape == b.shape and _rel(a.cpu(), b) < 1e-4, _rel(a.cpu(), b)


def _ref_xent(logits, targets, eps):
    return torch.stack([F.cross_entropy(y, targets, label_smoothing=eps) for y in logits])


@pytest.mark.parametrize('n', [1, 8, 33])
@pytest.mark.parametrize('eps', [0.0, 0.1])
@pytest.mark.parametrize('B,K', [(64, 10), (32, 1000)])
def test_meta_cross_entropy_matches_float64(n, eps, B, K):
    from ghn3_amd import target_ops as T
    gen = torch.Generator().manual_seed(n * 7 + K)
    logits = [3 * torch.randn(B, K, generator=gen, dtype=torch.float64) for _ in range(n)]
    targets = torch.randint(0, K, (B,), generator=gen)
    gce = torch.rand(n, generator=gen, dtype=torch.float64) + 0.5
    ld = [y.float().cuda().requires_grad_(True) for y in logits]
    ce, hits = T.meta_cross_entropy(ld, targets.cuda(), eps)
    assert type(ce.grad_fn).__name__ == 'MetaCrossEntropyBackward'
    (ce * gce.float().cuda()).sum().backward()
    lr = [y.clone().requires_grad_(True) for y in logits]
    want = _ref_xent(lr, targets, eps)
    (want * gce).sum().backward()
    assert _rel(ce.detach().cpu(), want.detach()) < 2e-5
    for a, b in zip(ld, lr):
        assert _rel(a.grad.cpu(), b.grad) < 1e-4, _rel(a.grad.cpu(), b.grad)
    lg = torch.stack([y.float() for y in logits])                    # (continuous draws: no ties)
    top = lg.topk(min(5, K), dim=-1).indices == targets.view(1, -1, 1)
    assert hits.cpu().tolist() == [int(top[..., :1].any(-1).sum()), int(top.any(-1).sum())]


def test_meta_cross_entropy_out_of_range_target_gives_nan():
    from ghn3_amd import target_ops as T
    logits = [torch.randn(8, 10, device='cuda', requires_grad=True) for _ in range(3)]
    targets = torch.tensor([0, 1, 2, 3, 4, 5, 6, 10], device='cuda')
    ce, hits = T.meta_cross_entropy(logits, targets, 0.1)
    ce.sum().backward()
    torch.cuda.synchronize()
    assert torch.isnan(ce).all() and int(hits[0]) <= 21
    assert torch.isnan(logits[0].grad[7]).all() and torch.isfinite(logits[0].grad[:7]).all()
    targets[7] = -1
    ce, _ = T.meta_cross_entropy([y.detach() for y in logits], targets, 0.0)
    torch.cuda.synchronize()
    assert torch.isnan(ce).all()


def test_head_and_loss_are_deterministic():
    from ghn3_amd import target_ops as T
    case = CASES[3]
    x, ws, bs, masks, ps, G = _case_tensors(case, seed=9)
    r1, r2 = _run_fused(case, x, ws, bs, masks, ps, G), _run_fused(case, x, ws, bs, masks, ps, G)
    for a, b in zip([r1[0], r1[1]] + r1[2] + r1[3], [r2[0], r2[1]] + r2[2] + r2[3]):
        assert torch.equal(a, b)
    outs = []
    for _ in range(2):
        gen = torch.Generator().manual_seed(4)
        logits = [torch.randn(256, 1000, generator=gen).cuda().requires_grad_(True) for _ in range(5)]
        targets = torch.randint(0, 1000, (256,), generator=gen).cuda()
        ce, hits = T.meta_cross_entropy(logits, targets, 0.1)
        ce.sum().backward()
        outs.append([ce.detach(), hits] + [y.grad for y in logits])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def _stock_head(pool, classifier, x):
    out = pool(x) if pool is not None else x
    return classifier(out.float().reshape(out.size(0), -1))


def test_heads_outside_the_op_keep_the_stock_path(monkeypatch):
    from ghn3_amd import target_ops as T
    x = torch.randn(8, 64, 4, 4, device='cuda')
    pool = torch.nn.AdaptiveAvgPool2d(1)
    head = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU(), torch.nn.Dropout(0.5), torch.nn.Linear(32, 10)).cuda()
    assert T.run_classifier_head(pool, head, x) is not None
    for env in ('GHN3_NATIVE_HEAD', 'GHN3_NATIVE_OPS'):
        monkeypatch.setenv(env, '0')
        assert T.run_classifier_head(pool, head, x) is None
        ce, _ = T.meta_cross_entropy([torch.randn(8, 10, device='cuda', requires_grad=True)], torch.zeros(8, dtype=torch.long, device='cuda'))
        assert type(ce.grad_fn).__name__ != 'MetaCrossEntropyBackward'
        monkeypatch.delenv(env)
    assert T.run_classifier_head(pool, head.cpu(), x.cpu()) is None                       # CPU tensors
    head.cuda()
    assert T.run_classifier_head(pool, head, x.half()) is None                            # fp16 features
    gelu = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.GELU()).cuda()
    assert T.run_classifier_head(pool, gelu, x) is None                                    # not a classifier chain
    assert T.run_classifier_head(torch.nn.AdaptiveAvgPool2d(2), head, x) is None          # not a global pool
    ce, _ = T.meta_cross_entropy([torch.randn(8, 10, device='cuda').half().requires_grad_(True)],
                                 torch.zeros(8, dtype=torch.long, device='cuda'))         # fp16 logits
    assert type(ce.grad_fn).__name__ != 'MetaCrossEntropyBackward'
    # under no_grad nothing is kept: the logits are all that stays allocated
    head.eval()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        y = T.run_classifier_head(pool, head, x)
    torch.cuda.synchronize()
    assert y.grad_fn is None and torch.cuda.memory_allocated() - before <= 512 * ((y.numel() * 4 + 511) // 512)
    assert _rel(y.cpu(), _stock_head(pool, head, x).detach().cpu()) < 1e-5


def _light_params(net, seed):
    """Seeded tensors assigned as a GHN assigns its prediction: views of one flat buffer (the leaf)."""
    import recipe
    table = {}
    for cell in net._layered_modules:
        table.update(cell)
    shapes = [(n, tuple(e['sz'])) for n, e in table.items()]
    params = recipe.seeded_net_params(shapes, seed=seed)
    total = sum(int(np.prod(s)) for _, s in shapes)
    flat = torch.zeros(total, device='cuda')
    off = 0
    for n, s in shapes:
        k = int(np.prod(s))
        flat[off:off + k] = torch.from_numpy(params[n]).reshape(-1).cuda()
        off += k
    flat.requires_grad_(True)
    off = 0
    for n, e in table.items():
        k = int(np.prod(e['sz']))
        setattr(e['module'], 'weight' if e['is_w'] else 'bias', flat[off:off + k].view(tuple(e['sz'])))
        off += k
    return [flat]


def _no_head_dropout(net):
    for m in list(net.classifier):
        if type(m).__name__ == 'Dropout':
            m.p = 0.0


@pytest.mark.parametrize('light', [True, False])
@pytest.mark.parametrize('train', [False, True])
@pytest.mark.parametrize('k', [1, 4])
def test_sampled_networks_match_the_stock_path(light, train, k, monkeypatch):
    import recipe
    from ghn3_amd.deepnets1m import SampledNets
    x = torch.from_numpy(recipe.seeded_images((8, 3, 32, 32), seed=3)).cuda()
    res = {}
    for native in ('0', '1'):
        monkeypatch.setenv('GHN3_NATIVE_HEAD', native)
        net = SampledNets(large_images=False, seed=2, max_nodes=400, light=light)[k].net
        if light:
            leaves = _light_params(net, 50 + k)
        else:
            net = net.cuda()
            params = recipe.seeded_net_params([(n, tuple(p.shape)) for n, p in net.named_parameters()], seed=50 + k)
            with torch.no_grad():
                for n, p in net.named_parameters():
                    p.copy_(torch.from_numpy(params[n]))
            leaves = [p for _, p in net.named_parameters()]
        net.train(train)
        _no_head_dropout(net)
        torch.manual_seed(123)
        logits, _ = net(x)
        assert (type(logits.grad_fn).__name__ == 'ClassifierHeadBackward') == (native == '1'), type(logits.grad_fn).__name__
        logits.square().mean().backward()
        torch.cuda.synchronize()
        res[native] = (logits.detach().cpu(), [p.grad.detach().cpu() if p.grad is not None else None for p in leaves])
    (l0, g0), (l1, g1) = res['0'], res['1']
    assert _rel(l1, l0) < 2e-4, _rel(l1, l0)
    for a, b in zip(g1, g0):
        assert (a is None) == (b is None)
        if a is not None and float(b.norm()) > 0:
            assert _rel(a, b) < 5e-4, _rel(a, b)


STOCK_OPS = ('aten::addmm', 'aten::linear', 'aten::adaptive_avg_pool2d', 'aten::cross_entropy_loss', 'aten::_log_softmax',
             'aten::topk')


def test_trainer_update_runs_no_stock_head_or_loss(monkeypatch):
    import recipe
    from util_parity import make_models
    from ghn3_amd import Trainer
    from ghn3_amd.deepnets1m import SampledNets
    gen = torch.Generator().manual_seed(1)
    images = torch.randn(8, 3, 32, 32, generator=gen)
    targets = torch.tensor([1, 7, 3, 9, 0, 2, 5, 5])
    res = {}
    for native in ('0', '1'):
        monkeypatch.setenv('GHN3_NATIVE_HEAD', native)
        hip, _ = make_models(recipe.TINY_CFG, recipe.TINY_SEED)
        tr = Trainer(hip, 'adamw', {'lr': 1e-3}, 'cosine', n_batches=3, grad_clip=5, device='cuda', log_interval=1000,
                     epochs=1)
        graphs = next(SampledNets.loader(meta_batch_size=4, seed=9, max_nodes=120))
        for net in graphs.nets:
            _no_head_dropout(net)
        torch.manual_seed(5)
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            m = tr.update(images, targets, graphs=graphs)
            torch.cuda.synchronize()
        names = {e.key for e in prof.key_averages()}
        grads = {n: p.grad.detach().cpu().clone() for n, p in hip.named_parameters() if p.grad is not None}
        res[native] = (m.avg()['loss'], grads, names)
    (l0, g0, n0), (l1, g1, n1) = res['0'], res['1']
    assert 'aten::topk' in n0                                       # (the stock path does use them)
    assert not [op for op in STOCK_OPS if op in n1], [op for op in STOCK_OPS if op in n1]
    assert abs(l1 - l0) <= 1e-5 * abs(l0), (l1, l0)
    assert g0.keys() == g1.keys() and len(g1) > 0
    for n in g0:
        go = g0[n]
        if float(go.norm()) < 1e-7:
            continue
        assert float((g1[n] - go).norm()) < 2e-3 * float(go.norm()) + 1e-6, n
