"""GPU tests of the data-parallel plain-network path on one MI355X: ghn3_mt_pack / ghn3_mt_unpack against torch bit for bit,
FusedSGD under a reducer against FusedSGD without one (1-rank RCCL group, force=True), the Trainer with data_parallel=True
against a twin outside any group, sync_module_states' round trip, and -- with two GPUs -- the example under torchrun."""

import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

import plain_ddp_cases as C
from ghn3_amd import FusedSGD
from ghn3_amd import _lib as L
from ghn3_amd import optim as O
from ghn3_amd.ddp_utils import FlatGradReducer, sync_module_states

pytestmark = pytest.mark.gpu

CH = O.MT_CHUNK
SIZES = [1, 3, 4, 5, CH - 1, CH, CH + 1, 2 * CH + 7]   # partial quad, whole quad, exact chunk, one over, a multi-chunk tail
K_SRC_VIEW, K_DST_VIEW = 4, 6                          # tensors that start 4 bytes into their allocation
GUARD = 8                                              # floats on each side (32 bytes: keeps the 16-byte alignment)
SENTINEL = 0x7fc0dead                                  # a NaN payload no copy produces
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def group():
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(C.free_port()))
    dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        yield
    finally:
        dist.destroy_process_group()


def _bits(seed, n):
    """n random 32-bit patterns (so NaNs and infinities of every payload occur), the first ones fixed: -0.0, +-inf, quiet and
    signalling NaNs."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([-2 ** 31, 0x7f800000, 0xff800000 - 2 ** 32, 0x7fc00001, 0xffc12345 - 2 ** 32, 0x7f800001],
                           dtype=torch.int64).to(torch.int32)
    k = min(n, len(special))
    v[:k] = special[:k]
    return v


def _guarded(n, view):
    """(whole allocation as int32 filled with SENTINEL, the fp32 tensor of n elements inside it); view: 4 bytes off 16."""
    whole = torch.full((n + 2 * GUARD + 1,), SENTINEL, dtype=torch.int32, device='cuda')
    lo = GUARD + (1 if view else 0)
    t = whole[lo:lo + n].view(torch.float32)
    assert t.data_ptr() % 16 == (4 if view else 0)
    return whole, t


def _ptr_table(tensors):
    return torch.from_numpy(np.asarray([t.data_ptr() for t in tensors], dtype=np.int64)).cuda()


def test_mt_pack_and_unpack_equal_torch_bit_for_bit():
    lib = L.load()
    offs = O.flat_layout(SIZES)
    total = int(offs[-1])
    assert [int(o) % 4 for o in offs] == [0] * len(offs) and total > sum(SIZES)        # (there are pad floats)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    flat_whole = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.int32, device='cuda')
    flat = flat_whole[GUARD:GUARD + total].view(torch.float32)
    flat.zero_()
    assert flat.data_ptr() % 16 == 0
    rec, chunks, n_chunks = O._mt_tables(flat.data_ptr(), offs, SIZES, 'cuda')
    assert n_chunks == sum((n + CH - 1) // CH for n in SIZES)
    # ---- pack
    payload = [_bits(k, n) for k, n in enumerate(SIZES)]
    srcs = [_guarded(n, k == K_SRC_VIEW) for k, n in enumerate(SIZES)]
    for (_, t), v in zip(srcs, payload):
        t.view(torch.int32).copy_(v)
    src_tab = _ptr_table([t for _, t in srcs])
    want = torch.full((total + 2 * GUARD,), SENTINEL, dtype=torch.int32)
    want[GUARD:GUARD + total] = 0
    for o, v in zip(offs, payload):
        want[GUARD + int(o):GUARD + int(o) + v.numel()] = v
    runs = []
    for _ in range(2):
        flat.zero_()
        assert lib.ghn3_mt_pack(rec.data_ptr(), src_tab.data_ptr(), chunks.data_ptr(), n_chunks, stream) == 0
        runs.append(flat_whole.cpu())
    assert torch.equal(runs[0], want) and torch.equal(runs[1], runs[0])     # payloads, zero pads and both guards, as int32
    for (whole, t), v in zip(srcs, payload):                                # (the sources are read only)
        assert torch.equal(t.view(torch.int32).cpu(), v)
    # ---- unpack
    dsts = [_guarded(n, k == K_DST_VIEW) for k, n in enumerate(SIZES)]
    dst_tab = _ptr_table([t for _, t in dsts])
    runs = []
    for _ in range(2):
        for _, t in dsts:
            t.view(torch.int32).fill_(SENTINEL)
        assert lib.ghn3_mt_unpack(rec.data_ptr(), dst_tab.data_ptr(), chunks.data_ptr(), n_chunks, stream) == 0
        runs.append([whole.cpu() for whole, _ in dsts])
    for k, (n, v) in enumerate(zip(SIZES, payload)):
        lo = GUARD + (1 if k == K_DST_VIEW else 0)
        w = torch.full((n + 2 * GUARD + 1,), SENTINEL, dtype=torch.int32)
        w[lo:lo + n] = v
        assert torch.equal(runs[0][k], w), k                                # the tensor and the guards around it
        assert torch.equal(runs[1][k], runs[0][k]), k
    assert torch.equal(flat_whole.cpu(), want)                              # (unpack reads the flat buffer only)
    # ---- the optimizer-level wrappers give the same bytes
    flat2 = torch.zeros(total, device='cuda')
    O.mt_pack(flat2, offs, [t for _, t in srcs])
    assert torch.equal(flat2.view(torch.int32).cpu(), want[GUARD:GUARD + total])
    # ---- argument checks (check_tables)
    err = L.load().ghn3_last_error
    for fn in (lib.ghn3_mt_pack, lib.ghn3_mt_unpack):
        assert fn(None, None, None, 0, stream) == 0                         # no chunks: GHN3_OK without a launch
        assert fn(None, src_tab.data_ptr(), chunks.data_ptr(), n_chunks, stream) == -1 and b'null table' in err()
        assert fn(rec.data_ptr(), None, chunks.data_ptr(), n_chunks, stream) == -1
        assert fn(rec.data_ptr(), src_tab.data_ptr(), None, n_chunks, stream) == -1
        assert fn(rec.data_ptr() + 4, src_tab.data_ptr(), chunks.data_ptr(), n_chunks, stream) == -1 and b'8 bytes' in err()
        assert fn(rec.data_ptr(), src_tab.data_ptr(), chunks.data_ptr(), -1, stream) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# FusedSGD under a reducer
# ---------------------------------------------------------------------------------------------------------------------
STEPS = 4


def _offset_view(v):
    buf = torch.zeros(v.numel() + 1, device='cuda')
    buf[1:].copy_(v.reshape(-1))
    return buf[1:].view(v.shape)


def _params():
    g = torch.Generator().manual_seed(1)
    return [(_offset_view(torch.randn(n, generator=g)) if k == K_SRC_VIEW else torch.randn(n, generator=g).cuda())
            .requires_grad_(True) for k, n in enumerate(SIZES)]


def _set_grads(ps, step, wire=None):
    """3 randn gradients (their norm is above the clip of 5); the gradient of one tensor is a view 4 bytes into its allocation.
    wire: the gradients take a round trip through that type first (what a 16-bit exchange delivers)."""
    g = torch.Generator().manual_seed(100 + step)
    for k, p in enumerate(ps):
        v = 3 * torch.randn(p.shape, generator=g)
        if wire is not None:
            v = v.to(wire).float()
        p.grad = _offset_view(v) if k == K_DST_VIEW else v.cuda()


def _run(reducer, wire=None):
    ps = _params()
    opt = FusedSGD(ps, lr=0.05, momentum=0.9, weight_decay=1e-4, max_grad_norm=5.0, reducer=reducer)
    norms = []
    for step in range(STEPS):
        _set_grads(ps, step, wire)
        grads = [p.grad.clone() for p in ps]
        norms.append(opt.step())
        if reducer is not None:
            assert all(torch.equal(p.grad, g) for p, g in zip(ps, grads))   # p.grad is left as autograd wrote it
    torch.cuda.synchronize()
    return [p.detach() for p in ps], opt.momentum_buffer, torch.stack(norms)


@pytest.mark.parametrize('algo', ['rsag', 'allreduce'])
def test_the_reducer_path_equals_the_plain_step_bit_for_bit(group, algo):
    p0, m0, n0 = _run(None)
    p1, m1, n1 = _run(FlatGradReducer(force=True, algo=algo))
    assert all(torch.equal(a, b) for a, b in zip(p0, p1))
    assert torch.equal(m0, m1) and torch.equal(n0, n1)
    assert float(n0.min()) > 5.0                                             # (the clip took part)


def test_the_pack_switch_gives_the_same_bits(group, monkeypatch):
    monkeypatch.setenv('GHN3_MT_PACK', '0')                                  # torch._foreach_copy_ instead of ghn3_mt_pack
    p1, m1, n1 = _run(FlatGradReducer(force=True))
    monkeypatch.delenv('GHN3_MT_PACK')
    p0, m0, n0 = _run(None)
    assert all(torch.equal(a, b) for a, b in zip(p0, p1)) and torch.equal(m0, m1) and torch.equal(n0, n1)


def test_bf16_on_the_wire_equals_the_round_trip_of_the_packed_gradients(group):
    """compress='bf16' with the mesh exchange against the plain step on gradients rounded to bf16 and back; tolerance: the 1e-2
    of the 1-rank bf16 exchange in test_gpu_parity.py (relative L2)."""
    p0, m0, n0 = _run(None, wire=torch.bfloat16)
    p1, m1, n1 = _run(FlatGradReducer(force=True, algo='mesh', compress='bf16'))
    for name, a, b in (('parameters', p1, p0), ('momentum', [m1], [m0]), ('norm', [n1], [n0])):
        err = C.rel(a, b)
        print('bf16 wire, %s: %.3e' % (name, err))
        assert err < 1e-2, (name, err)


# ---------------------------------------------------------------------------------------------------------------------
# Trainer
# ---------------------------------------------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.down = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout)) if stride != 1 else None

    def forward(self, x):
        y = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
        return F.relu(y + (x if self.down is None else self.down(x)))


class _SmallResNet(nn.Module):
    def __init__(self, width=8):
        super().__init__()
        self.conv1 = nn.Conv2d(3, width, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.layers = nn.Sequential(_Block(width, width, 1), _Block(width, 2 * width, 2))
        self.fc = nn.Linear(2 * width, 10)

    def forward(self, x):
        x = self.layers(F.relu(self.bn1(self.conv1(x))))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


def _images(k):
    g = torch.Generator().manual_seed(70 + k)
    return torch.randn(8, 3, 16, 16, generator=g), torch.randint(0, 10, (8,), generator=g)


def _train(amp, data_parallel):
    torch.manual_seed(3)
    tr = C.make_trainer(_SmallResNet(), device='cuda', amp=amp, amp_init_scale=1024.0, data_parallel=data_parallel)
    if data_parallel:
        assert isinstance(tr._optimizer.reducer, FlatGradReducer)
        tr._optimizer.reducer = FlatGradReducer(force=True)
    else:
        assert tr._optimizer.reducer is None
    for k in range(4):
        tr.update(*_images(k))
    tr.scheduler_step()
    torch.cuda.synchronize()
    return tr


@pytest.mark.parametrize('amp', [False, True])
def test_the_trainer_in_a_one_rank_group_equals_its_twin_outside(amp):
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True          # (both runs: the convolutions' own run-to-run differences are not the subject)
    try:
        twin = _train(amp, False)
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(C.free_port()))
        dist.init_process_group('nccl', rank=0, world_size=1)
        try:
            tr = _train(amp, True)
        finally:
            dist.destroy_process_group()
    finally:
        torch.backends.cudnn.deterministic = det
    for (k, a), b in zip(tr._model.state_dict().items(), twin._model.state_dict().values()):
        assert torch.equal(a, b), k
    assert torch.equal(tr._optimizer.momentum_buffer, twin._optimizer.momentum_buffer)
    assert tr.metrics.avg() == twin.metrics.avg() and float(tr.metrics.cnt) == float(twin.metrics.cnt)
    assert tr.loss_scale == twin.loss_scale
    torch.manual_seed(3)
    start = _SmallResNet()
    assert not torch.equal(start.fc.weight, tr._model.fc.weight.cpu())       # (the four steps moved the parameters)


def test_sync_module_states_round_trip_leaves_every_bit(group):
    torch.manual_seed(5)
    net = _SmallResNet().cuda()
    # one buffer is a view 4 bytes into its allocation, one holds special bit patterns, the counters differ
    odd = torch.zeros(net.bn1.running_mean.numel() + 1, device='cuda')[1:]
    odd.copy_(torch.randn(odd.numel()))
    net.bn1.running_mean = odd
    assert net.bn1.running_mean.data_ptr() % 16 == 4
    net.bn1.running_var.view(torch.int32)[:4] = torch.tensor([-2 ** 31, 0x7f800000, 0x7fc00001, 0x7f800001], dtype=torch.int32).cuda()
    net.layers[0].bn1.num_batches_tracked.fill_(41)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    ptrs = [v.data_ptr() for v in net.state_dict().values()]
    sync_module_states(net, force=True)
    sync_module_states(net, force=True, parameters=False)
    torch.cuda.synchronize()
    after = net.state_dict()
    assert [v.data_ptr() for v in after.values()] == ptrs
    for k, v in before.items():
        a = after[k]
        assert a.dtype == v.dtype
        same = torch.equal(a.view(torch.int32), v.view(torch.int32)) if v.dtype == torch.float32 else torch.equal(a, v)
        assert same, k
    assert int(net.layers[0].bn1.num_batches_tracked) == 41


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs 2 GPUs')
def test_the_example_trains_under_torchrun_on_two_gpus():
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--standalone', '--nproc_per_node=2',
           os.path.join(ROOT, 'examples', 'train_ddp.py'), '--steps', '6', '--epochs', '1']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    m = re.search(r'final loss ([-+0-9.a-z]+) on 2 ranks; (\d+) updates skipped', out)
    assert m and np.isfinite(float(m.group(1))) and int(m.group(2)) == 0, out[-3000:]
