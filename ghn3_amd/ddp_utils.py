"""
Data-parallel helpers (one process per GPU, torch.distributed over RCCL/xGMI; gloo on CPU).

Mirrors /root/reference/ghn3/ddp_utils.py:21-93 (``setup_ddp, is_ddp, get_ddp_rank, clean_ddp,
avg_ddp_metric``) and adds ``all_reduce_flat_grads``: the GHN keeps every gradient in ONE flat fp32 buffer,
so the reference's bucketed DDP all-reduce (trainer.py:136, C1 in SURVEY 2.3) becomes a few large
collectives straight on that buffer -- no bucket copies -- issued largest-first so that RCCL can pipeline them.
"""

import os
from datetime import timedelta

import torch
import torch.distributed as dist


def setup_ddp():
    class Args:
        pass
    args = Args()
    args.ddp = False
    if 'RANK' in os.environ and 'WORLD_SIZE' in os.environ:
        args.world_size = int(os.environ['WORLD_SIZE'])
        args.gpu = int(os.environ.get('LOCAL_RANK', 0))
        args.device = 'cuda' if torch.cuda.is_available() else 'cpu'
        if args.device == 'cuda':
            args.device = 'cuda:%d' % args.gpu
            torch.cuda.set_device(args.gpu)
        args.ddp = True
        if not dist.is_initialized():
            dist.init_process_group(backend='nccl' if args.device.startswith('cuda') else 'gloo',
                                    timeout=timedelta(minutes=30), world_size=args.world_size,
                                    rank=int(os.environ['RANK']))
        args.rank = dist.get_rank()
    else:
        args.rank = 0
        args.world_size = 1
        args.device = 'cuda' if torch.cuda.is_available() else 'cpu'
    return args


def is_ddp():
    return dist.is_available() and dist.is_initialized()


def get_ddp_rank():
    return dist.get_rank() if is_ddp() else 0


def clean_ddp():
    if is_ddp():
        dist.barrier()
        dist.destroy_process_group()


def avg_ddp_metric(metric):
    """Mean of a scalar tensor over ranks: one all-reduce instead of the reference's all_gather + mean."""
    if not is_ddp():
        return metric
    m = metric.detach().clone()
    dist.all_reduce(m, op=dist.ReduceOp.SUM)
    return (m / dist.get_world_size()).view_as(metric)


def sync_parameters(ghn, src=0):
    """Broadcast rank `src`'s GHN parameters (the flat fp32 buffer) to every rank -- what wrapping the model in
    DistributedDataParallel does at construction (trainer.py:136).  Without it replicas stay consistent only if every
    rank seeds identically and loads the same checkpoint."""
    if not is_ddp() or dist.get_world_size() == 1:
        return ghn
    with torch.no_grad():
        dist.broadcast(ghn._flat, src=src)
    ghn.params_changed()
    return ghn


def sync_module_states(model, src=0, force=False, parameters=True):
    """Rank `src`'s parameters and buffers become every rank's -- what DistributedDataParallel's constructor does for a plain
    nn.Module.  The fp32 tensors (parameters and BatchNorm statistics) are gathered into ONE flat buffer (GPU: ghn3_mt_pack,
    one launch; CPU: torch copies), broadcast with one collective and scattered back (ghn3_mt_unpack); the rest
    (num_batches_tracked: int64) is stacked into one tensor per dtype and broadcast the same way.  parameters=False: the
    buffers alone (the Trainer's sync between epochs).  A 1-rank group returns at once unless `force` is set (tests of the code
    path)."""
    if not is_ddp() or (dist.get_world_size() == 1 and not force):
        return model
    from .optim import flat_layout, mt_pack, mt_unpack
    tensors = ([p.data for p in model.parameters()] if parameters else []) + [b for b in model.buffers() if b is not None]
    with torch.no_grad():
        f32 = [t for t in tensors if t.dtype == torch.float32 and t.numel() > 0 and t.is_contiguous()]
        if f32:
            offs = flat_layout([t.numel() for t in f32])
            flat = torch.zeros(int(offs[-1]), dtype=torch.float32, device=f32[0].device)
            if flat.is_cuda:
                mt_pack(flat, offs, f32)
            else:
                for o, t in zip(offs, f32):
                    flat[int(o):int(o) + t.numel()].copy_(t.reshape(-1))
            dist.broadcast(flat, src=src)
            if flat.is_cuda:
                mt_unpack(flat, offs, f32)
            else:
                for o, t in zip(offs, f32):
                    t.copy_(flat[int(o):int(o) + t.numel()].view(t.shape))
        done = set(id(t) for t in f32)
        rest = {}
        for t in tensors:
            if id(t) not in done and t.numel() > 0:
                rest.setdefault((t.dtype, t.device), []).append(t)
        for group in rest.values():                           # (the same sequence on every rank: module order)
            cat = torch.cat([t.reshape(-1) for t in group])
            dist.broadcast(cat, src=src)
            for t, piece in zip(group, cat.split([t.numel() for t in group])):
                t.copy_(piece.view(t.shape))
    return model


def all_reduce_flat_grads(flat, chunk_bytes=256 << 20, average=True):
    """
    In-place mean all-reduce of the flat gradient buffer in `chunk_bytes` pieces (async, then waited).
    xGMI is point-to-point (7 links x ~153 GB/s per GPU): a few large collectives keep every link busy,
    whereas the reference's 25 MB DDP buckets would issue >100 small ring steps for the 2.6 GB of ghn3xlm16.
    """
    if not is_ddp() or dist.get_world_size() == 1:
        return flat
    n = flat.numel()
    step = max(1, chunk_bytes // flat.element_size())
    works = []
    for s in range(0, n, step):
        works.append(dist.all_reduce(flat[s:s + step], op=dist.ReduceOp.SUM, async_op=True))
    for w in works:
        w.wait()
    if average:
        flat.div_(dist.get_world_size())
    return flat


def all_reduce_flat_grads_avg(flat, chunk_bytes=256 << 20):
    """Same as all_reduce_flat_grads(average=True) with the mean taken inside RCCL (ncclAvg): no extra pass."""
    if not is_ddp() or dist.get_world_size() == 1:
        return flat
    if not (flat.is_cuda and dist.get_backend() == 'nccl'):
        return all_reduce_flat_grads(flat, chunk_bytes, True)
    step = max(1, chunk_bytes // flat.element_size())
    works = [dist.all_reduce(flat[s:s + step], op=dist.ReduceOp.AVG, async_op=True)
             for s in range(0, flat.numel(), step)]
    for w in works:
        w.wait()
    return flat


def _hip_ops(records, ptrs, stream):
    """Run a few buffer-level ops of the library (GHN3_OP_WIRE_PACK / GHN3_OP_RANK_REDUCE) on `stream`."""
    import numpy as np
    from . import _lib as L
    ops = np.zeros(len(records), dtype=L.OP_DT)
    ops['r']['buf'][:] = -1
    for k, (kind, refs, ints, f0) in enumerate(records):
        ops[k]['kind'] = kind
        for e, r in enumerate(refs):
            ops[k]['r'][e]['buf'], ops[k]['r'][e]['off'] = r, 0
        ops[k]['i'][:len(ints)] = ints
        ops[k]['f'][0] = f0
    L.context(torch.cuda.current_device()).run(ops, np.zeros(0, dtype=L.PROBLEM_DT), np.asarray(ptrs, dtype=np.uint64), stream)


def mesh_all_reduce_avg(piece, wire_dtype=None, force=False):
    """
    Mean all-reduce of a 1-D tensor shaped for a fully connected xGMI mesh (7 links x ~153 GB/s per MI355X): the two-shot
    direct algorithm
        all-to-all:  rank r receives chunk r of every rank       (W - 1 links carry S / W each, concurrently)
        local sum :  fp32 accumulation of the W chunks, averaged, in rank order (every rank computes the same bits; no
                     16-bit accumulation error over the ranks)
        all-gather:  every rank receives every reduced chunk      (again all links, S / W each)
    `wire_dtype` (torch.bfloat16) is the type on the wire; the result is written back to `piece` in place.
    On the GPU the local passes are library ops on the current stream (GHN3_OP_WIRE_PACK: fp32 -> bf16 of the range and
    back, GHN3_OP_RANK_REDUCE: W-way sum + scale), 2-3 streaming passes instead of the five ATen ones of round 2; an
    fp32 exchange of a length divisible by W sends and gathers in place (one pass).  CPU tensors (gloo, the tests) take
    the equivalent torch expressions.  `force`: run the collectives even in a 1-rank group (GPU test of the code path).
    """
    W = dist.get_world_size()
    n = piece.numel()
    if W == 1 and not force:
        if wire_dtype is not None and wire_dtype != piece.dtype:
            piece.copy_(piece.to(wire_dtype))                     # (the rounding a real exchange would apply)
        return piece
    per = (n + W - 1) // W
    wd = wire_dtype or piece.dtype
    if piece.is_cuda and piece.dtype == torch.float32 and wd in (torch.float32, torch.bfloat16):
        from . import _lib as L
        stream = torch.cuda.current_stream(piece.device).cuda_stream
        b16 = wd == torch.bfloat16
        if not b16 and W * per == n:
            recv = torch.empty_like(piece)
            dist.all_to_all_single(recv, piece)
            red = torch.empty(per, dtype=torch.float32, device=piece.device)
            _hip_ops([(L.OP_RANK_REDUCE, (0, 1), (per, W, 0, 0), 1.0 / W)], [red.data_ptr(), recv.data_ptr()], stream)
            dist.all_gather_into_tensor(piece, red)
            return piece
        send = torch.empty(W * per, dtype=wd, device=piece.device)
        recv = torch.empty_like(send)
        red = torch.empty(per, dtype=wd, device=piece.device)
        if b16:
            _hip_ops([(L.OP_WIRE_PACK, (0, 1), (n, W * per, 0), 0.0)], [send.data_ptr(), piece.data_ptr()], stream)
        else:
            send[:n].copy_(piece)
            send[n:].zero_()
        dist.all_to_all_single(recv, send)
        _hip_ops([(L.OP_RANK_REDUCE, (0, 1), (per, W, int(b16), int(b16)), 1.0 / W)], [red.data_ptr(), recv.data_ptr()], stream)
        dist.all_gather_into_tensor(send, red)
        if b16:
            _hip_ops([(L.OP_WIRE_PACK, (0, 1), (n, n, 1), 0.0)], [piece.data_ptr(), send.data_ptr()], stream)
        else:
            piece.copy_(send[:n])
        return piece
    send = torch.empty(W * per, dtype=wd, device=piece.device)
    send[:n].copy_(piece)
    if W * per > n:
        send[n:].zero_()                                          # (fewer than W padding elements)
    recv = torch.empty_like(send)
    dist.all_to_all_single(recv, send)
    # (one pass: the W chunks are accumulated in fp32 on the fly, in rank order on every rank)
    red = torch.sum(recv.view(W, per), dim=0, dtype=torch.float32).mul_(1.0 / W).to(wd)
    dist.all_gather_into_tensor(send, red)
    piece.copy_(send[:n])
    return piece


def reduce_scatter_avg(piece, force=False):
    """Mean reduce-scatter of a 1-D fp32 tensor whose length is a multiple of the world size W: returns this rank's chunk
    (elements [r n / W, (r + 1) n / W) of the mean over ranks) as a new tensor.  RCCL: ncclReduceScatter with ncclAvg (one
    collective on the xGMI mesh; RCCL picks its direct / ring schedule).  gloo (the CPU tests; no reduce-scatter there):
    all-to-all + fp32 sum of the W chunks in rank order -- the same bits on every rank."""
    W = dist.get_world_size()
    n = piece.numel()
    assert n % W == 0, (n, W)
    per = n // W
    if W == 1 and not force:
        return piece.clone()
    if piece.is_cuda and dist.get_backend() == 'nccl':
        out = torch.empty(per, dtype=piece.dtype, device=piece.device)
        dist.reduce_scatter_tensor(out, piece, op=dist.ReduceOp.AVG)
        return out
    recv = torch.empty_like(piece)
    dist.all_to_all_single(recv, piece.contiguous())
    return torch.sum(recv.view(W, per), dim=0, dtype=torch.float32).mul_(1.0 / W).to(piece.dtype)


class FlatGradReducer:
    """
    Mean all-reduce of the flat gradient buffer, overlapped with the backward program:

        reducer.begin()
        reducer.start(flat, lo, hi, wait_for=ctx.side_wait)   # a range whose gradients are complete (W2: 69 %, ...)
        ... the rest of the backward runs on the current stream ...
        reducer.finish(flat)                                  # everything else, then wait

    The collectives are issued from a dedicated communication stream that waits for the producers (the current
    stream and, through `wait_for`, the context's side stream), so RCCL runs under the Graphormer backward.
    compress='bf16' sends bf16 copies (half the xGMI bytes); None keeps fp32.
    algo: 'allreduce' (default) = RCCL's own all-reduce (ncclAvg, sum accumulated in the wire type like torch's
    bf16_compress_hook); 'mesh' (GHN3_ALLREDUCE_ALGO=mesh) = all-to-all + fp32 local sum + all-gather
    (mesh_all_reduce_avg: the sum over ranks is accumulated in fp32 even with bf16 on the wire, replicas bit-identical).
    The mesh path has only ever run under gloo and in 1-rank RCCL groups (no multi-GPU box was available to the
    builder), so RCCL's tuned collective is the default until the two are timed side by side on real links.
    Works on CPU tensors (gloo).
    The sequence and sizes of the collectives depend on the GHN's parameter layout only (Program.bwd_parts), never on
    a rank's graph.
    """

    def __init__(self, compress=None, chunk_bytes=256 << 20, force=False, algo=None, gather=True):
        assert compress in (None, 'bf16')
        self.compress = compress
        self.chunk = max(1, chunk_bytes // 4)
        self.force = force                      # run the code path even for a 1-rank group (tests)
        # Round 5 default: 'rsag' = reduce-scatter + all-gather per chunk (RCCL's own two collectives on the mesh, fp32 on
        # the wire): the same bytes as an all-reduce, every element summed once on its owner -- identical bits on all ranks
        # -- and the two halves can be taken apart: with gather=False the exchange stops after the reduce-scatter and
        # `owned` lists the ranges of the flat buffer whose MEAN gradient this rank holds (optim.ShardedAdamW updates those
        # and all-gathers the updated PARAMETERS instead).  With bf16 on the wire 'rsag' runs the 'mesh' code (all-to-all of
        # bf16 chunks + fp32 local sum).  'allreduce' = RCCL's all-reduce, 'mesh' = all-to-all + local sum + all-gather.
        self.algo = algo or os.environ.get('GHN3_ALLREDUCE_ALGO', 'rsag')
        assert self.algo in ('mesh', 'allreduce', 'rsag')
        if self.algo == 'rsag' and compress == 'bf16':
            self.algo = 'mesh'
        self.gather = bool(gather)
        assert self.gather or self.algo == 'rsag', 'gather=False needs the fp32 reduce-scatter exchange'
        self._comm = None
        self._pending = []                      # (work, flat slice, staging buffer or None)
        self._done = []                         # ranges already started
        self.owned = []                         # (lo, hi) of this rank's shards after finish() (rsag)
        self.replicated = []                    # (lo, hi) reduced on every rank (the < 64 W elements a chunk leaves over)
        self.chunks = []                        # (start, length) of the chunks the shards were cut from

    def active(self):
        return is_ddp() and (dist.get_world_size() > 1 or self.force)

    def _issue(self, flat, lo, hi):
        if self.algo == 'rsag':
            W, r = dist.get_world_size(), dist.get_rank()
            for s in range(lo, hi, self.chunk):
                e = min(hi, s + self.chunk)
                main = (e - s) // (64 * W) * (64 * W)         # (shards start on 64-float boundaries, like the parameters)
                if main:
                    per = main // W
                    shard = reduce_scatter_avg(flat[s:s + main], force=self.force)
                    if self.gather:
                        dist.all_gather_into_tensor(flat[s:s + main], shard)
                    else:
                        flat[s + r * per:s + (r + 1) * per].copy_(shard)
                    self.owned.append((s + r * per, s + (r + 1) * per))
                    self.chunks.append((s, main))
                if s + main < e:                              # (fewer than 64 W elements: reduced everywhere)
                    tail = flat[s + main:e]
                    dist.all_reduce(tail, op=dist.ReduceOp.SUM)
                    tail.mul_(1.0 / W)
                    self.replicated.append((s + main, e))
            return
        if self.algo == 'mesh':
            wd = torch.bfloat16 if self.compress == 'bf16' else None
            for s in range(lo, hi, self.chunk):
                mesh_all_reduce_avg(flat[s:min(hi, s + self.chunk)], wd, force=self.force)   # (ordered on the comm stream)
            return
        # RCCL averages inside the collective (ncclAvg): no separate scaling pass over the 2.6 GB buffer
        self._avg = flat.is_cuda and dist.get_backend() == 'nccl'
        op = dist.ReduceOp.AVG if self._avg else dist.ReduceOp.SUM
        for s in range(lo, hi, self.chunk):
            piece = flat[s:min(hi, s + self.chunk)]
            if self.compress == 'bf16':
                buf = piece.to(torch.bfloat16)
                self._pending.append((dist.all_reduce(buf, op=op, async_op=True), piece, buf))
            else:
                self._pending.append((dist.all_reduce(piece, op=op, async_op=True), piece, None))

    def _drain(self):
        scale = 1.0 / dist.get_world_size()
        for work, piece, buf in self._pending:
            work.wait()
            if buf is not None:
                piece.copy_(buf)
            if not self._avg:
                piece.mul_(scale)
        self._pending = []

    def begin(self):
        """New backward: forget the ranges of the previous one."""
        self._done = []
        self.owned, self.replicated, self.chunks = [], [], []

    def start(self, flat, lo, hi, wait_for=None):
        """May be called several times per backward (one range each, begin() first)."""
        if not self.active():
            return
        self._done.append((lo, hi))
        if not flat.is_cuda:
            self._issue(flat, lo, hi)
            return
        if self._comm is None:
            self._comm = torch.cuda.Stream(device=flat.device)
        cur = torch.cuda.current_stream(flat.device)
        self._comm.wait_stream(cur)
        if wait_for is not None:
            wait_for(self._comm.cuda_stream)
        flat.record_stream(self._comm)
        with torch.cuda.stream(self._comm):
            self._issue(flat, lo, hi)

    def finish(self, flat):
        if not self.active():
            return flat
        n = flat.numel()
        rest, pos = [], 0
        for lo, hi in sorted(self._done):
            if lo > pos:
                rest.append((pos, lo))
            pos = max(pos, hi)
        if pos < n:
            rest.append((pos, n))
        if not flat.is_cuda:
            for lo, hi in rest:
                self._issue(flat, lo, hi)
            self._drain()
            return flat
        if self._comm is None:
            self._comm = torch.cuda.Stream(device=flat.device)
        cur = torch.cuda.current_stream(flat.device)
        self._comm.wait_stream(cur)
        flat.record_stream(self._comm)
        with torch.cuda.stream(self._comm):
            for lo, hi in rest:
                self._issue(flat, lo, hi)
            self._drain()
        cur.wait_stream(self._comm)
        self._done = []
        return flat
