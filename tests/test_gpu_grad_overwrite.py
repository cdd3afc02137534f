"""
The backward that overwrites single-writer weight gradients (Program(grad_layout=...), the default of GHN3) on the GPU: ghn3tm8
on a 12-node graph with a 3x3 and a 1x1 convolution, 1-D nodes and the classifier, and on a ragged batch of that graph and a
5-node one.  The flat gradient buffer is handed out poisoned (0x7f bytes instead of torch.empty), so a byte the backward neither
fills nor overwrites, or an overwrite that still adds its C operand, is a huge or non-finite gradient.  With the switch on and
off (GHN3_GRAD_OVERWRITE) the gradients must be finite, equal bit for bit, and within test_gpu_parity.py's tolerances for this
model (test_ghn3tm8_synthetic_forward_backward) of the oracle's.
"""

import pytest
import torch

import recipe
from oracle import ghn3_ref as R
from util_parity import make_models

pytestmark = pytest.mark.gpu

T_CFG = dict(max_shape=(64, 64, 16, 16), num_classes=1000, hid=64, heads=8, layers=3, weight_norm=True, ve=True,
             layernorm=True)
NET12 = dict(nodes=[('input', None, None),
                    ('conv', 'stem.weight', (32, 3, 3, 3)),
                    ('bn', 'bn1.weight', (32,)),
                    ('conv', 'c2.weight', (48, 32, 3, 3)),
                    ('bias', 'c2.bias', (48,)),
                    ('sum', None, None),
                    ('conv', 'c3.weight', (32, 48, 1, 1)),
                    ('bias', 'c3.bias', (32,)),
                    ('bn', 'bn2.weight', (32,)),
                    ('glob_avg', None, None),
                    ('conv', 'fc.weight', (1000, 32)),
                    ('bias', 'fc.bias', (1000,))],
             skips=[(1, 5)])
NET5 = dict(nodes=[('input', None, None),
                   ('conv', 'c.weight', (16, 3, 3, 3)),
                   ('bn', 'bn.weight', (16,)),
                   ('glob_avg', None, None),
                   ('conv', 'fc.weight', (1000, 16))])
BATCHES = {'one': [NET12], 'ragged': [NET12, NET5]}
TOL_G = {'f32': 3e-4, 'f16': 1e-3}
_ORACLE = {}


def _loss(nets):
    return sum(torch.norm(p, p='fro') for net in nets for p in net.parameters())


def _oracle_grads(oracle, batch):
    if batch not in _ORACLE:
        specs = BATCHES[batch]
        nets = [recipe.build_torch_net(s) for s in specs]
        graphs = []
        for s in specs:
            nf, info, A = recipe.graph_arrays(s)
            graphs.append(R.GraphRef(torch.from_numpy(nf), info, torch.from_numpy(A)))
        oracle.train()
        _, pred = oracle(nets, R.GraphBatchRef(graphs), keep_grads=True)
        sum(torch.norm(t, p='fro') for (_, _, _, t) in pred).backward()
        _ORACLE[batch] = {k: p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)
                          for k, p in oracle.named_parameters()}
    return _ORACLE[batch]


def _hip_grads(hip, batch):
    from ghn3_amd import Graph, GraphBatch
    specs = BATCHES[batch]
    nets = [recipe.build_torch_net(s) for s in specs]
    graphs = []
    for s in specs:
        nf, info, A = recipe.graph_arrays(s)
        graphs.append(Graph(node_feat=nf, node_info=info, A=A))
    for p in hip.parameters():
        p.grad = None
    torch.manual_seed(0)
    hip.train()
    nets = hip(nets, GraphBatch(graphs, dense=True), keep_grads=True)
    _loss(nets).backward()
    torch.cuda.synchronize()
    return {k: p.grad.detach().clone() for k, p in hip.named_parameters()}, hip.last_plan.program


@pytest.mark.parametrize('compute', ['f32', 'f16'])
@pytest.mark.parametrize('batch', sorted(BATCHES))
def test_poisoned_gradient_buffer_overwrite_on_and_off(batch, compute, monkeypatch):
    hip, oracle = make_models(T_CFG, 7, compute=compute)
    assert [len(s['nodes']) for s in BATCHES['ragged']] == [12, 5]

    def poisoned():
        g = torch.empty(hip._flat_numel, dtype=torch.float32, device=hip.device)
        g.view(torch.uint8).fill_(0x7f)
        return g
    monkeypatch.setattr(hip, '_new_grad_buffer', poisoned)
    grads = {}
    for sw in ('1', '0'):
        monkeypatch.setenv('GHN3_GRAD_OVERWRITE', sw)
        grads[sw], prog = _hip_grads(hip, batch)
        if sw == '1':
            assert prog.grad_fill_patch is not None and len(prog.grad_no_memset) >= 4 * hip.layers + 1
            assert all('gnn.%d.ff.net.0.weight' % l in prog.grad_no_memset for l in range(hip.layers))
        else:
            assert prog.grad_fill_patch is None and prog.grad_no_memset in ([], ['decoder.conv.2.weight'])
    ref = _oracle_grads(oracle, batch)
    assert set(grads['1']) == set(ref)
    for k, go in ref.items():
        on, off = grads['1'][k], grads['0'][k]
        assert bool(torch.isfinite(on).all()) and bool(torch.isfinite(off).all()), k
        assert torch.equal(on, off), (k, float((on - off).abs().max()))
        err = float((on.cpu().double() - go.double()).norm())
        assert err < TOL_G[compute] * float(go.norm()) + 1e-5, (k, err, float(go.norm()))
