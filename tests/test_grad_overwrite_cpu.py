"""
Program(grad_layout=...) on the numpy interpreter: single-writer weight gradients overwrite and leave the zero-fill, and every
zero-fill of the backward stands at its head.  The flat gradient buffer is poisoned with 0x7f bytes (3.4e38: any byte that is
neither filled nor overwritten, and any overwrite that still reads its C operand, shows as a non-finite or a different value)
and the backward with the layout must leave the bits of the backward without it -- one graph, the ragged three-graph batch and
two equal graphs; the fp32 and the direct 16-bit route of the tile gradient; the single-run order and the three data-parallel
parts.  The structure checks hold the fill to the exact complement of the overwritten tensors.
"""

import numpy as np
import pytest

import recipe
from test_program_cpu import _build, _run_program, _tiny

from ghn3_amd import _lib as L

CASES = ['b1', 'ragged3', 'b2']
_MEMO = {}


def _backward(case, route, parts, overwrite):
    """Poisoned flat gradient buffer after the backward of `case`; route 'dout' (upstream gradient, fp32 tile gradient) or 'norm'
    (fused norm loss, direct 16-bit tiles); parts: the three data-parallel parts instead of the single-run order.  Computed once
    per combination."""
    key = (case, route, parts, overwrite)
    if key in _MEMO:
        return _MEMO[key]
    hip = _build(recipe.TINY_CFG, recipe.TINY_SEED, 'reference')[0]
    nets_h, gb_h = _tiny(case)[:2]
    prog, it, bufs, gflat = _run_program(hip, nets_h, gb_h, decoder_ctype=L.CT_F16, decoder_bwd_ctype=L.CT_F16,
                                         grad_layout=hip._grad_layout() if overwrite else None)
    assert (prog.grad_fill_patch is not None) == overwrite
    it.run(prog.norm_fin_ops(), prog.problems)
    bufs[prog.xbuf(prog.X_NORMG)] = np.asarray([0.37], dtype=np.float32).view(np.uint8)
    dout = (1e-3 * np.random.RandomState(4).standard_normal(prog.out_numel)).astype(np.float32)
    bufs[prog.xbuf(prog.X_DOUT)] = dout.view(np.uint8)
    it.bufs = bufs
    r = prog.bwd_ops[prog.tile_bwd_op]['r']
    for slot, (buf, off) in prog.tile_bwd_refs.items():
        on = (route == 'dout') if slot == 0 else (route == 'norm')
        r[slot]['buf'], r[slot]['off'] = (buf, off) if on else (-1, 0)
    patched = [prog.tile_bwd_op] + prog.set_tile_route(route == 'norm')
    gflat[:] = 0x7f
    hip._patch_grad_memsets(prog)
    if not parts:
        it.run(prog.bwd_ops, prog.problems)
    else:
        assert len(prog.bwd_parts) == 3
        k = prog.memset_grad_op                                  # (what GHN3._run_backward patches into part 1)
        prog.bwd_parts[0][0][k:k + 2] = prog.bwd_ops[k:k + 2]
        for k_ in patched:
            prog.bwd_parts[0][0][prog.ddp_index.get(k_, k_)] = prog.bwd_ops[k_]
        for ops, _ in prog.bwd_parts:
            it.run(ops, prog.problems)
    _MEMO[key] = (gflat.view(np.float32).copy(), prog, hip)
    return _MEMO[key]


@pytest.mark.parametrize('parts', [False, True], ids=['single', 'parts'])
@pytest.mark.parametrize('route', ['dout', 'norm'])
@pytest.mark.parametrize('case', CASES)
def test_overwriting_backward_leaves_the_bits_of_the_accumulating_one(case, route, parts):
    on = _backward(case, route, parts, True)[0]
    off = _backward(case, route, parts, False)[0]
    assert np.isfinite(on).all() and np.isfinite(off).all()
    assert np.array_equal(on, off)
    assert np.abs(on).max() > 0
    # (the parts write what the single run writes)
    assert np.array_equal(on, _backward(case, route, False, True)[0])


def _fill_ranges(prog, hip, ops):
    """[begin, end) bytes of the flat gradient buffer that the MEMSET0 ops of `ops` zero."""
    P, out = prog.P, []
    for o in ops:
        if int(o['kind']) != L.OP_MEMSET0:
            continue
        buf, off, n = int(o['r'][0]['buf']), int(o['r'][0]['off']), int(o['i'][0])
        if buf == prog.xbuf(prog.X_GRADFLAT):
            out.append((off, off + n))
        elif P <= buf < 2 * P:
            out.append((4 * int(hip._offs[buf - P]) + off, 4 * int(hip._offs[buf - P]) + off + n))
    return [(a, b) for a, b in out if b > a]


@pytest.mark.parametrize('case', CASES)
def test_the_fill_is_the_exact_complement_of_the_overwritten_tensors(case):
    _, prog, hip = _backward(case, 'dout', False, True)
    P = prog.P
    numel = {n: int(hip._split_sizes[2 * k]) for k, n in enumerate(prog.names)}
    # every Graphormer layer weight has one writer with K = B N, whatever the batch
    for l in range(prog.Lyr):
        for w in ('attn.to_qkv.weight', 'attn.to_out.0.weight', 'ff.net.0.weight', 'ff.net.3.weight'):
            assert 'gnn.%d.%s' % (l, w) in prog.grad_no_memset
    assert len(set(prog.grad_no_memset)) == len(prog.grad_no_memset)
    written = np.zeros(4 * hip._flat_numel, dtype=bool)
    for name in prog.grad_no_memset:
        slot = prog.slot[name]
        w = [p for p in prog.problems[prog.n_fwd_problems:] if int(p['C']['buf']) == P + slot]
        # exactly one problem, without GHN3_GEMM_ACCUM, that covers the tensor.  (dW2 had this status before: its band problems
        # write every row once, and the families on fp32 operands accumulate on top of them, later on the same stream.)
        over = [p for p in w if not int(p['flags']) & L.GEMM_ACCUM]
        assert len(w) == len(over) == 1 or name == 'decoder.conv.2.weight', name
        assert sum(int(p['M']) * int(p['N']) for p in over) == numel[name], name
        assert all(int(p['c_gather']['buf']) < 0 and int(p['ksplit']) <= 1 for p in w), name
        others = [p for p in prog.problems[prog.n_fwd_problems:]
                  if any(int(p[f]['buf']) == P + slot for f in ('bias', 'residual', 'aux_in', 'aux_out'))]
        assert not others, name
        written[4 * int(hip._offs[slot]):4 * (int(hip._offs[slot]) + numel[name])] = True
    filled = np.zeros(4 * hip._flat_numel, dtype=bool)
    for a, b in _fill_ranges(prog, hip, prog.bwd_ops):
        assert 0 <= a and b <= filled.size
        filled[a:b] = True
    assert not (filled & written).any()                  # no byte of an overwritten tensor is zeroed: the saving is real
    assert (filled | written).all()                      # every other byte is (alignment gaps included)
    # a tensor that keeps accumulating keeps its flag
    for p in prog.problems[prog.n_fwd_problems:]:
        b = int(p['C']['buf'])
        if P <= b < 2 * P and prog.names[b - P] not in prog.grad_no_memset:
            assert int(p['flags']) & L.GEMM_ACCUM, prog.names[b - P]


@pytest.mark.parametrize('case', CASES)
def test_every_zero_fill_stands_at_the_head_of_the_backward(case):
    _, prog, hip = _backward(case, 'dout', False, True)
    _, base, _ = _backward(case, 'dout', False, False)
    fills = [k for k, o in enumerate(prog.bwd_ops) if int(o['kind']) == L.OP_MEMSET0]
    k0 = prog.memset_grad_op
    assert fills == list(range(k0, k0 + len(fills))) and len(fills) > 2
    assert prog.tile_bwd_op == k0 + len(fills)
    # the workspace fills of the program without the layout are all there, at the same place of the workspace
    ws = prog.xbuf(prog.X_WS)
    key = lambda o: (int(o['r'][0]['off']), int(o['i'][0]))
    want = sorted(key(o) for o in base.bwd_ops if int(o['kind']) == L.OP_MEMSET0 and int(o['r'][0]['buf']) == ws)
    got = sorted(key(o) for o in prog.bwd_ops if int(o['kind']) == L.OP_MEMSET0 and int(o['r'][0]['buf']) == ws)
    assert got == want and prog.ws_bytes == base.ws_bytes
    # data-parallel parts: all of them in part 1
    n_part = [sum(int(o['kind']) == L.OP_MEMSET0 for o in ops) for ops, _ in prog.bwd_parts]
    assert n_part == [len(fills), 0, 0]
    if prog.grad_sumsq is not None:
        w_ops = [k for k, o in enumerate(prog.bwd_ops)
                 if int(o['kind']) == L.OP_GEMM and (int(o['flags']) >> 16) & 0xff == prog.TAG_D3_WGRAD]
        z = [k for k in fills if int(prog.bwd_ops[k]['r'][0]['off']) == prog.grad_sumsq['ws_off']]
        assert len(z) == 1 and z[0] < min(w_ops)
