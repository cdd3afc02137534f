"""The data-parallel plain-network branch of ghn3_amd.Trainer (data_parallel=True) on CPU tensors under gloo: opt-in and refusal,
two ranks against one process and a float64 oracle, bit-identical replicas, the skip of a non-finite gradient on every rank,
the start-up broadcast, resuming outside the group, and FusedSGD's contract under a reducer."""

import math
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import plain_ddp_cases as C
from ghn3_amd import FusedSGD
from ghn3_amd import optim as O
from ghn3_amd.ddp_utils import FlatGradReducer


def test_opt_in_and_refusal_in_a_real_one_rank_group():
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(C.free_port()))
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError, match='data_parallel=True'):
            C.make_trainer(C.bn_net())
        tr = C.make_trainer(C.bn_net(), data_parallel=True)
        assert isinstance(tr._optimizer, FusedSGD) and isinstance(tr._optimizer.reducer, FlatGradReducer)
        tr._optimizer.reducer = FlatGradReducer(force=True)      # (the collectives really run in the 1-rank group)
        for k in range(3):
            tr.update(*C.batch(k))
        tr.scheduler_step()
        got = C.state_of(tr)
    finally:
        dist.destroy_process_group()
    assert tr._optimizer.steps == 3 and math.isfinite(tr.metrics.avg()['loss'])
    # outside a group the option changes nothing: the same three updates, bit for bit (an average over one rank)
    alone = C.make_trainer(C.bn_net(), data_parallel=True)
    assert alone._optimizer.reducer is None
    for k in range(3):
        alone.update(*C.batch(k))
    want = C.state_of(alone)
    assert all(torch.equal(a, b) for a, b in zip(got[0] + got[1], want[0] + want[1]))


def test_the_stock_switch_takes_the_reducer_too(monkeypatch):
    monkeypatch.setenv('GHN3_FUSED_SGD', '0')
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(C.free_port()))
    dist.init_process_group('gloo', rank=0, world_size=1)
    try:
        tr = C.make_trainer(C.bn_net(), data_parallel=True)
        assert isinstance(tr._optimizer, O.StockSGD) and isinstance(tr._optimizer.reducer, FlatGradReducer)
        tr._optimizer.reducer = FlatGradReducer(force=True)
        for k in range(3):
            tr.update(*C.batch(k))
    finally:
        dist.destroy_process_group()
    alone = C.make_trainer(C.bn_net())                          # the same switch, no group: an average over one rank changes no bit
    assert isinstance(alone._optimizer, O.StockSGD) and alone._optimizer.reducer is None
    for k in range(3):
        alone.update(*C.batch(k))
    got, want = C.state_of_model(tr), C.state_of_model(alone)
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_two_ranks_on_half_batches_equal_one_process_on_the_whole_batch():
    """Errors against the float64 oracle, relative L2 over all parameters / all momentum buffers after three steps; measured
    here: one process 4.68e-8 / 2.01e-7, world 2 4.69e-8 / 1.90e-7 on both ranks."""
    ranks, _ = C.halves_run()
    one = C.make_trainer(C.norm_free_net())
    for k in range(3):
        one.update(*C.batch(k))
    p1, m1 = C.state_of(one)
    p64, m64 = C.oracle64(C.norm_free_net(), range(3))
    e1p, e1m = C.rel(p1, p64), C.rel(m1, m64)
    for r in (0, 1):
        p2, m2, avg = ranks[r]
        e2p, e2m = C.rel(p2, p64), C.rel(m2, m64)
        print('fp32 errors against float64: one process %.2e / %.2e, world 2 rank %d %.2e / %.2e' % (e1p, e1m, r, e2p, e2m))
        assert e2p <= C.MARGIN * e1p and e2m <= C.MARGIN * e1m, (e2p, e1p, e2m, e1m)
        assert avg['loss'] == pytest.approx(one.metrics.avg()['loss'], rel=1e-5)      # (metrics are averaged over the ranks)
    assert C.rel(p1, [p.detach() for p in C.norm_free_net().parameters()]) > 1e-2     # (the three steps did move them)


def test_a_world_2_checkpoint_resumes_in_one_process():
    """The checkpoint rank 0 wrote after two world-2 steps, resumed by a Trainer outside any group that then takes the WHOLE third
    batch, against the world-2 run's own third step: two fp32 runs, each within its bound of the oracle (the test above)."""
    ranks, save_dir = C.halves_run()
    resumed = C.make_trainer(C.norm_free_net(seed=99), save_dir=save_dir)
    assert (resumed.start_epoch, resumed.start_step) == (0, 2) and resumed._optimizer.reducer is None
    resumed.update(*C.batch(2))
    p, m = C.state_of(resumed)
    p64, m64 = C.oracle64(C.norm_free_net(), range(3))
    one = C.make_trainer(C.norm_free_net())
    for k in range(3):
        one.update(*C.batch(k))
    e1p, e1m = (C.rel(a, b) for a, b in zip(C.state_of(one), (p64, m64)))
    assert C.rel(p, p64) <= C.MARGIN * e1p and C.rel(m, m64) <= C.MARGIN * e1m
    assert C.rel(p, ranks[0][0]) <= (1 + C.MARGIN) * e1p and C.rel(m, ranks[0][1]) <= (1 + C.MARGIN) * e1m


@pytest.mark.parametrize('algo', ['rsag', 'mesh'])
def test_replicas_stay_bit_identical(algo):
    r0, r1 = (C.replica_run()[r][algo] for r in (0, 1))
    for k, ((p0, m0, n0), (p1, m1, n1)) in enumerate(zip(r0['steps'], r1['steps'])):
        assert all(torch.equal(a, b) for a, b in zip(p0 + m0, p1 + m1)), (algo, k)
        assert n0 == n1 and math.isfinite(n0), (algo, k)
    assert len(r0['steps']) == 4
    assert not all(torch.equal(a, b) for a, b in zip(r0['steps'][0][0], r0['steps'][3][0]))
    # the ranks saw different data: their BatchNorm statistics differ until scheduler_step() makes rank 0's the run's
    assert not all(torch.equal(a, b) for a, b in zip(r0['buffers_before'], r1['buffers_before']))
    assert all(torch.equal(a, b) for a, b in zip(r0['buffers_after'], r1['buffers_after']))
    assert all(torch.equal(a, b) for a, b in zip(r0['buffers_after'], r0['buffers_before']))


def test_start_up_makes_rank_0s_network_the_runs():
    run = C.replica_run()
    own = C.bn_net(seed=7).state_dict()                          # what rank 0 built; rank 1 came from another seed
    for r in (0, 1):
        start = run[r]['rsag']['start']
        assert list(start) == list(own)
        for k in own:
            assert torch.equal(start[k], own[k]), (r, k)
    assert int(run[1]['rsag']['start']['1.num_batches_tracked']) == 0     # (rank 1's own count was 1)
    assert not torch.equal(C.bn_net(seed=20).state_dict()['0.weight'], own['0.weight'])


def test_a_non_finite_gradient_on_one_rank_skips_the_update_on_both():
    run = C.spawn(C.poison_worker, 2)
    for r in (0, 1):
        before, after, skipped, counted = run[r]
        assert all(torch.equal(a, b) for a, b in zip(before[0] + before[1], after[0] + after[1])), r
        assert skipped == 1 and counted == 8          # (the skipped step is in neither the sums nor the counts)
    assert all(torch.equal(a, b) for a, b in zip(run[0][1][0], run[1][1][0]))


def test_fused_sgd_contract_under_a_reducer():
    torch.manual_seed(0)
    ps = [torch.randn(5, requires_grad=True), torch.randn(3, requires_grad=False), torch.randn(2, 3, requires_grad=True)]
    opt = FusedSGD(ps, lr=0.1, momentum=0.9, reducer=FlatGradReducer())
    assert opt._gflat.idx == [0, 2] and opt._gflat.offs.tolist() == [0, 8, 16] and opt._gflat.flat.numel() == 16
    ps[0].grad = torch.ones(5)
    with pytest.raises(RuntimeError, match='parameter 2 '):
        opt.step()
    ps[2].grad = torch.full((2, 3), 2.0)
    frozen = ps[1].clone()
    g0 = ps[0].grad.clone()
    ref = [p.detach().clone() for p in ps]
    norm = opt.step()
    assert float(norm) == pytest.approx(math.sqrt(5 + 24))
    assert torch.equal(ps[1], frozen) and torch.equal(ps[0].grad, g0)
    assert torch.allclose(ps[0].detach(), ref[0] - 0.1 * 1.0) and torch.allclose(ps[2].detach(), ref[2] - 0.1 * 2.0)
    assert float(opt._gflat.flat[5:8].abs().sum()) == 0 and float(opt._gflat.flat[14:].abs().sum()) == 0     # the pad floats
    # without a reducer nothing of this exists, and a missing gradient is torch's "does not take part"
    plain = FusedSGD(ps, lr=0.1, momentum=0.9)
    assert plain._gflat is None and plain.reducer is None
    ps[2].grad = None
    plain.step()


def test_the_layout_has_64_bit_offsets():
    sizes = [(1 << 30) + 1, 3, (1 << 30) + 5, 1 << 30, 7]
    offs = O.flat_layout(sizes)
    assert offs.dtype == np.int64 and len(offs) == len(sizes) + 1
    want, pos = [0], 0
    for n in sizes:
        pos += (n + 3) // 4 * 4
        want.append(pos)
    assert offs.tolist() == want and offs[-1] > (1 << 31) and all(o % 4 == 0 for o in want)
    assert 4 * int(offs[-1]) == 4 * want[-1] > (1 << 33)        # (byte offsets are formed in Python integers)
    assert O.flat_layout([]).tolist() == [0]
