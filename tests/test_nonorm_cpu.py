"""
The BN-free (norm=None) target networks on the native layers, checked without a GPU:

  * the three entry points of the no-norm depthwise + pointwise family are declared in the header and in the loader's export
    list, and the ABI version did not move (symbols only);
  * the default architecture stream is the one the commit before `bn_free_prob` drew (tests/golden/sampled_stream_parent.json,
    written by that commit: net_args of indices 0..31 of SampledNets(seed=0, max_nodes=400)); with bn_free_prob=1.0 every index
    is a norm=None network with a valid graph;
  * the op rows of tests/test_gpu_target_nonorm.py are well conditioned under tests/util_parity.slice_errors: the stock layers in
    fp32 against fp64 stay within a tenth of the GPU bounds (2e-5 output, 3e-5 gradients).
"""
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import nonorm_cases as C
import target_edge_cases as E
from util_parity import slice_errors

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SYMBOLS = ('ghn3_dwpw_plain_scratch_floats', 'ghn3_dwpw_plain_fwd', 'ghn3_dwpw_plain_bwd')


def test_the_plain_entry_points_are_declared_and_the_abi_version_stays():
    from ghn3_amd import _lib as L
    header = open(os.path.join(ROOT, 'include', 'ghn3_hip.h')).read()
    for name in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, header), name
        assert name in L.EXPORTS, name
    assert L.ABI_VERSION == 21
    assert re.search(r'#define\s+GHN3_ABI_VERSION\s+21\b', header)


def _plain(args):
    """net_args as the fixture stores them: the genotype as lists."""
    a = dict(args)
    g = a['genotype']
    a['genotype'] = {'normal': [[n, int(k)] for n, k in g.normal], 'normal_concat': [int(k) for k in g.normal_concat],
                     'reduce': [[n, int(k)] for n, k in g.reduce], 'reduce_concat': [int(k) for k in g.reduce_concat]}
    return a


def test_the_default_stream_is_the_parent_commits():
    from ghn3_amd.deepnets1m import SampledNets
    want = json.load(open(os.path.join(HERE, 'golden', 'sampled_stream_parent.json')))
    assert len(want) == 32
    nets = SampledNets(seed=0, max_nodes=400)
    for i, w in enumerate(want):
        got = json.loads(json.dumps(_plain(nets[i].net_args)))
        assert got == w, (i, got, w)
        assert got['norm'] == 'bn'
    # an explicit zero is the default
    assert _plain(SampledNets(seed=0, max_nodes=400, bn_free_prob=0.0)[3].net_args) == _plain(nets[3].net_args)


def test_bn_free_prob_one_draws_only_networks_without_norm_layers():
    from ghn3_amd.deepnets1m import SampledNets, sample_net_args
    import numpy as np
    nets = SampledNets(seed=0, max_nodes=400, bn_free_prob=1.0)
    for i in range(8):
        g = nets[i]
        assert g.net_args['norm'] is None, i
        # the completeness check of __getitem__: the graph's nodes name every tensor of the parameter tables, cell by cell
        tables = g.net._layered_modules
        assert len(g.node_info) == len(tables)
        for cell_nodes, table in zip(g.node_info, tables):
            in_graph = {n[1] for n in cell_nodes}
            assert all(k in in_graph or k.replace('.bias', '.weight') in in_graph for k in table)
        assert 0 < g.n_nodes <= 400
    # a share in between: both kinds appear, and the draw comes last (everything else is the default draw of that seed)
    drawn = [sample_net_args(np.random.RandomState(s), bn_free_prob=0.5) for s in range(40)]
    base = [sample_net_args(np.random.RandomState(s)) for s in range(40)]
    assert {a['norm'] for a in drawn} == {None, 'bn'}
    for a, b in zip(drawn, base):
        assert {k: v for k, v in _plain(a).items() if k != 'norm'} == {k: v for k, v in _plain(b).items() if k != 'norm'}


# ---- conditioning of the GPU rows -------------------------------------------------------------------------------------------
OUT_TOL, GRAD_TOL = 2e-5, 3e-5            # a tenth of the GPU bounds of tests/test_gpu_target_nonorm.py


@pytest.mark.parametrize('row', C.DWPW_ROWS, ids=str)
def test_dwpw_rows_are_well_conditioned_without_a_norm(row):
    x, w_dw, w_pw, up, (ks, st, pad, dil) = C.dwpw_case(row)
    res = []
    for dt in (torch.float32, torch.float64):
        leaves = [t.clone().to(dt).requires_grad_(True) for t in (x, w_dw, w_pw)]
        out = F.conv2d(F.conv2d(F.relu(leaves[0]), leaves[1], None, st, pad, dil, groups=x.shape[1]), leaves[2])
        (out * up.to(dt)).sum().backward()
        res.append([out.detach()] + [t.grad for t in leaves])
    worst = {}
    for name, a, b, ax, tol in zip(('out', 'dx', 'dw_dw', 'dw_pw'), res[0], res[1],
                                   (E.ACT_AXES, E.ACT_AXES, E.WGRAD_AXES, E.WGRAD_AXES), (OUT_TOL, GRAD_TOL, GRAD_TOL, GRAD_TOL)):
        v, where = slice_errors(a, b, ax)
        worst[name] = v
        assert v <= tol, (name, v, where)
    print('dwpw', row, ', '.join('%s %.2e' % kv for kv in worst.items()))


@pytest.mark.parametrize('row', C.PW_ROWS, ids=str)
def test_pointwise_rows_are_well_conditioned_without_a_norm(row):
    x, w_pw, up, st = C.pw_case(row)
    res = []
    for dt in (torch.float32, torch.float64):
        leaves = [t.clone().to(dt).requires_grad_(True) for t in (x, w_pw)]
        out = F.conv2d(F.relu(leaves[0]), leaves[1], None, st)
        (out * up.to(dt)).sum().backward()
        res.append([out.detach()] + [t.grad for t in leaves])
    worst = {}
    for name, a, b, ax, tol in zip(('out', 'dx', 'dw_pw'), res[0], res[1], (E.ACT_AXES, E.ACT_AXES, E.WGRAD_AXES),
                                   (OUT_TOL, GRAD_TOL, GRAD_TOL)):
        v, where = slice_errors(a, b, ax)
        worst[name] = v
        assert v <= tol, (name, v, where)
    print('pointwise', row, ', '.join('%s %.2e' % kv for kv in worst.items()))
