"""
Fused trainer step on the GHN's flat buffers.

Replaces, for a ghn3_amd.GHN3 whose parameters and gradients live in one flat fp32 buffer each, the reference's
    nn.utils.clip_grad_norm_(parameters, grad_clip)      /root/reference/ghn3/trainer.py:356-360
    optimizer.step()   (torch.optim.AdamW)               /root/reference/ghn3/trainer.py:165-175,379
by two kernels over the flat buffers (GHN3_OP_SUMSQ + GHN3_OP_ADAMW) -- no per-tensor launches.

For a plain network (separate parameter tensors, the train_ddp.py recipe) FusedSGD does the same for clip_grad_norm_ +
torch.optim.SGD with a multi-tensor kernel pair (ghn3_mt_sumsq + ghn3_mt_sgd).
"""

import ctypes
import os

import numpy as np
import torch

from . import _lib as L
from .nn import pinned_ring


def _dbits(x):
    return int(np.asarray([x], dtype=np.float64).view(np.int64)[0])


class FusedAdamW:
    """AdamW + gradient-norm clipping for a ghn3_amd.GHN3 (same update rule and defaults as torch.optim.AdamW).

    state_dtype: 'fp32' (default: the moments are fp32, the update is torch.optim.AdamW's) or 'bf16': exp_avg and exp_avg_sq
    are kept in bf16 -- half the optimizer state, 20 instead of 28 bytes per parameter through the pass.  Parameters,
    gradients and the arithmetic of the update stay fp32; only what is carried to the next step is rounded, stochastically
    (GHN3_OP_ADAMW_S16; round-to-nearest would freeze exp_avg_sq).  The random bits are a function of `state_seed`, the step
    number and the element's index in the flat buffer: a rerun repeats them bit for bit, whatever form the step takes."""

    def __init__(self, ghn, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0,
                 nan_guard=True, state_dtype='fp32', state_seed=0):
        if state_dtype not in ('fp32', 'bf16'):
            raise ValueError("state_dtype must be 'fp32' or 'bf16', got %r" % (state_dtype,))
        if int(state_seed) != state_seed or not 0 <= state_seed < STATE16_LIMIT:
            raise ValueError('state_seed must be an integer in [0, 2^24), got %r' % (state_seed,))
        self.state_dtype, self.state_seed = state_dtype, int(state_seed)
        self.ghn = ghn
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.max_grad_norm = max_grad_norm
        # nan_guard: the squared gradient norm is always computed; when it is not finite (a NaN / inf anywhere in the
        # flat gradient -- after the data-parallel average every rank sees the same value) the kernel leaves parameters
        # and moments untouched: the reference trainer's skip-this-batch (trainer.py:240-257) without a host sync
        self.nan_guard = nan_guard
        flat = ghn._flat
        if not flat.is_cuda:
            raise L.Ghn3Error('FusedAdamW runs on an MI355X only (no CPU path)')
        mdt = torch.bfloat16 if state_dtype == 'bf16' else flat.dtype
        self.exp_avg = torch.zeros_like(flat, dtype=mdt)
        self.exp_avg_sq = torch.zeros_like(flat, dtype=mdt)
        self.scal = torch.zeros(16 + 8192, dtype=torch.float32, device=flat.device)   # [norm^2 ...| partial sums]
        self.steps = 0
        self._w2_descs = {}

    def _w2_fusion(self, plan):
        """(lo, hi, device descriptor table, work tiles, state key) when this step may write the 16-bit copies of
        decoder.conv.2.weight itself (GHN3_OP_ADAMW_CAST16), else None: the plan's program casts W2, the copies exist and were
        current for the parameters of the last forward."""
        ghn = self.ghn
        prog = plan.program if plan is not None else None
        w2 = prog.shadow_w2 if prog is not None else None
        if w2 is None or not prog.training or ghn._shadow is None or os.environ.get('GHN3_ADAMW_CAST', '1') == '0':
            return None
        # (the W2 copies must be current for the parameters as they are now -- written by the last forward's refresh or by
        # the previous fused step -- or a step the NaN guard skips would leave stale copies marked as current)
        ver = ghn._shadow_version()
        st, st2 = ghn._shadow_state, ghn._shadow_w2_state
        if not ((st is not None and st[0] == ver) or (st2 is not None and st2[0] == ver)):
            return None
        it = w2['item']
        if it['ld_src'] != it['cols'] or it['cols'] % 4:
            return None
        lo = int(ghn._offs[prog.slot[w2['name']]])
        key = (it['rows'], it['cols'], tuple(it.get('straight') or ()), tuple(it.get('transposed') or ()))
        if key not in self._w2_descs:
            descs, blocks = prog.pack_cast_descs([it])
            self._w2_descs[key] = (torch.from_numpy(descs.view(np.uint8).copy()).to(ghn._flat.device), blocks)
        d, blocks = self._w2_descs[key]
        types = (prog.decoder_ctype, prog.decoder_bwd_ctype, prog.x3, prog.uses_op16)
        return lo, lo + it['rows'] * it['cols'], d, blocks, types

    def wait(self):
        """Makes torch's current stream wait for an overlapped step's side-stream half (see step(overlap=True)): call before
        anything but a GHN3 forward reads the parameters or the moments (checkpoints, .cpu(), torch ops on them)."""
        if getattr(self, '_side_busy', False):
            self.ghn._ctx().side_wait(torch.cuda.current_stream().cuda_stream)
            self._side_busy = False

    def step(self, gflat, grad_scale=1.0, plan=None, local_grads=False, overlap=False):
        """gflat: the flat gradient buffer of the last backward (plan.gflat); grad_scale: the loss scale the gradients
        carry (AMP: they are divided by it inside the kernel, no separate unscale pass).  Returns the gradient norm
        (device scalar, like clip_grad_norm_) when clipping or the NaN guard is on; when it is not finite the kernel
        left parameters and moments untouched.
        plan: the plan of the step's forward / backward.  With it the update of decoder.conv.2.weight (69 % of the
        parameters at ghn3xlm16) also writes the weight's 16-bit operand copies (GHN3_OP_ADAMW_CAST16), so the next
        forward does not read the 1.8 GB again to re-cast them; same parameters bit for bit.
        local_grads: `gflat` is exactly what the plan's last backward wrote (NOT averaged over ranks afterwards).  The
        squared norm of the W2 gradient is then taken from the sums the weight-gradient kernel left per output tile
        (Program.grad_sumsq, GHN3_GEMM_SUMSQ) instead of from a pass over its 1.8 GB.
        overlap: the update of the DECODER parameters (93 % of them at ghn3xlm16: 3 ms of HBM-bound streaming) runs on the
        context's side stream and the call returns with it pending; the embeddings and the Graphormer (updated on the
        caller's stream first) are all the next forward needs for its first ~1 ms -- the latency-bound Graphormer chain --
        and its program joins the side stream in front of the decoders (Program._build_decoder_forward).  Same kernels, same
        order per element: parameters bit-identical to the serial step.  Until that forward (or wait()) nothing else may
        read the decoder parameters / moments; the gradient buffer is kept alive here until the next call."""
        ghn = self.ghn
        flat = ghn._flat
        assert gflat.numel() == flat.numel() and gflat.is_cuda
        # a previous overlapped step may still be reading `scal` and writing the decoder ranges on the side stream (two steps
        # without a GHN3 forward in between: gradient accumulation, a timing loop): order this step behind it
        self.wait()
        self.steps += 1
        n = flat.numel()
        clip = self.max_grad_norm and self.max_grad_norm > 0
        fuse = self._w2_fusion(plan)
        overlap = bool(overlap) and getattr(ghn, 'side_stream', True) and plan is not None and \
            plan.program.decoder_slots is not None and os.environ.get('GHN3_ADAMW_OVERLAP', '1') != '0'
        ops = np.zeros(9, dtype=L.OP_DT)
        ops['r']['buf'][:] = -1
        bufs = [flat.data_ptr(), gflat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                self.scal.data_ptr(), self.scal.data_ptr() + 64, 0, 0]
        ops[0]['kind'] = L.OP_MEMSET0
        ops[0]['r']['buf'][0] = 4
        ops[0]['i'][0] = 4
        guard = clip or self.nan_guard
        ops[1]['kind'] = L.OP_SUMSQ if guard else L.OP_NOP
        ops[1]['r']['buf'][:3] = (4, 1, 5)         # (r2: scratch for the fixed-order sum of the workgroup partials)
        ops[1]['i'][0] = n
        gs = plan.program.grad_sumsq if (plan is not None and local_grads and guard) else None
        if gs is not None and getattr(plan, 'gflat', None) is gflat and os.environ.get('GHN3_WGRAD_SUMSQ', '1') != '0':
            prog = plan.program
            k2 = prog.slot[gs['name']]
            lo2 = int(ghn._offs[k2])
            hi2 = int(ghn._offs[k2 + 1]) if k2 + 1 < len(ghn._offs) else n     # (the slot's padding holds zeros)
            bufs.append(int(plan.bufs[prog.xbuf(prog.X_WS)]) + gs['ws_off'])
            ops[1]['i'][1:4] = (lo2, hi2, gs['count'])
            ops[1]['r']['buf'][3] = len(bufs) - 1
        hyper = (self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                 1.0 - self.betas[0] ** self.steps, 1.0 - self.betas[1] ** self.steps)

        s16 = self.state_dtype == 'bf16'
        if s16 and self.steps >= STATE16_LIMIT:
            raise L.Ghn3Error('bf16 optimizer state: step %d does not fit the op (limit 2^24)' % self.steps)

        def adamw(op, kind, lo, count):
            op['kind'] = kind
            op['r']['buf'][:5] = (0, 1, 2, 3, 4 if guard else -1)
            op['r']['off'][:4] = 4 * lo
            if s16:
                # (bf16 moments: same element offset, 2 bytes each -- the kernel takes the flat index of its first element,
                # which the random bits of the rounding depend on, from this offset; step and seed ride in f2 / f3)
                op['kind'] = {L.OP_ADAMW: L.OP_ADAMW_S16, L.OP_ADAMW_CAST16: L.OP_ADAMW_S16_CAST16}[kind]
                op['r']['off'][2:4] = 2 * lo
                op['f'][2], op['f'][3] = float(self.steps), float(self.state_seed)
            op['i'][0] = count
            for k, h in enumerate(hyper):
                op['i'][1 + k] = _dbits(h)
            op['f'][0] = float(self.max_grad_norm or 0.0) if clip else 0.0
            op['f'][1] = 1.0 / float(grad_scale)

        if overlap:
            # [everything but the decoders] on the caller's stream, then the decoder ranges on the side stream, detached
            d_lo, d_hi = ghn.decoder_grad_range(plan.program)
            adamw(ops[2], L.OP_ADAMW, 0, d_lo)
            adamw(ops[3], L.OP_ADAMW, d_hi, n - d_hi)
            if fuse is None:
                adamw(ops[4], L.OP_ADAMW, d_lo, d_hi - d_lo)
            else:
                lo, hi, descs, blocks, types = fuse
                assert d_lo <= lo and hi <= d_hi
                bufs[6], bufs[7] = ghn._shadow.data_ptr(), descs.data_ptr()
                adamw(ops[4], L.OP_ADAMW, d_lo, lo - d_lo)
                adamw(ops[5], L.OP_ADAMW, hi, d_hi - hi)
                adamw(ops[6], L.OP_ADAMW_CAST16, lo, 1 + (blocks << 32))
                ops[6]['r']['buf'][5:7] = (6, 7)
            for k in (4, 5, 6):
                if int(ops[k]['kind']) != L.OP_NOP:
                    ops[k]['flags'] |= L.OPFLAG_SIDE
            # DETACH must END the run: the runtime ignores GHN3_OP_NOP padding behind it, but nothing else may follow
            # (round 6: it sat at ops[7] of 9 with a NOP behind it and the runtime re-armed the final join -- the
            # "overlapped" step of round 5 was serialised)
            ops[-1]['kind'] = L.OP_DETACH
            self._side_busy = True
            self._keep = gflat                   # (read by the side stream after this call returns)
        elif fuse is None:
            adamw(ops[2], L.OP_ADAMW, 0, n)
        else:
            lo, hi, descs, blocks, types = fuse
            bufs[6], bufs[7] = ghn._shadow.data_ptr(), descs.data_ptr()
            adamw(ops[2], L.OP_ADAMW, 0, lo)
            adamw(ops[3], L.OP_ADAMW, hi, n - hi)
            adamw(ops[4], L.OP_ADAMW_CAST16, lo, 1 + (blocks << 32))
            ops[4]['r']['buf'][5:7] = (6, 7)
        ghn._ctx().run(ops, np.zeros(0, dtype=L.PROBLEM_DT), np.asarray(bufs, dtype=np.uint64),
                       torch.cuda.current_stream().cuda_stream)
        ghn.params_changed()                     # (the kernel wrote the parameters through raw pointers)
        if fuse is not None:
            ghn._shadow_w2_state = (ghn._shadow_version(), True, fuse[4])
        return self.scal[0].sqrt() / float(grad_scale) if guard else None

    # ------------------------------------------------------------------ checkpoints (trainer.py:413-432)
    def state_dict(self):
        """State in the layout of ``torch.optim.AdamW.state_dict()`` over ``ghn.parameters()`` (the order the reference's
        trainer hands to its optimizer, trainer.py:165-175), so that ``{'state_dict', 'optimizer', 'epoch', 'step'}``
        checkpoints written by either trainer resume in the other.  With fp32 state the moment tensors are views of the flat
        buffers; with bf16 state they are fp32 COPIES (exact: every bf16 value is an fp32 value), so the file stays
        interchangeable with torch.optim.AdamW and with the fp32-state optimizer, which resumes from it exactly."""
        ghn = self.ghn
        self.wait()                               # (an overlapped step may still be writing the moments)
        slot_of = {id(p): k for k, p in enumerate(ghn._slot_params())}
        state, order = {}, []
        for i, p in enumerate(ghn.parameters()):
            k = slot_of[id(p)]
            o, n = int(ghn._offs[k]), p.numel()
            order.append(i)
            if self.steps > 0:
                state[i] = {'step': torch.tensor(float(self.steps)),
                            'exp_avg': self.exp_avg[o:o + n].view(p.shape).float(),
                            'exp_avg_sq': self.exp_avg_sq[o:o + n].view(p.shape).float()}
        group = {'lr': self.lr, 'betas': tuple(self.betas), 'eps': self.eps, 'weight_decay': self.weight_decay,
                 'amsgrad': False, 'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False,
                 'fused': None, 'params': order}
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        """Accepts a ``torch.optim.AdamW`` (or FusedAdamW, of either state type) state dict over ``ghn.parameters()``.  With
        bf16 state the fp32 moments of the file are rounded to nearest even (moments a bf16-state optimizer wrote are bf16
        values already: unchanged)."""
        ghn = self.ghn
        self.wait()
        groups = sd['param_groups']
        assert len(groups) == 1, 'one parameter group expected (trainer.py:175)'
        g = groups[0]
        self.lr, self.betas, self.eps = float(g['lr']), tuple(g['betas']), float(g['eps'])
        self.weight_decay = float(g['weight_decay'])
        assert not g.get('amsgrad', False), 'amsgrad is not supported'
        params = list(ghn.parameters())
        assert len(g['params']) == len(params), (len(g['params']), len(params))
        slot_of = {id(p): k for k, p in enumerate(ghn._slot_params())}
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        steps = 0
        for idx, p in zip(g['params'], params):
            st = sd['state'].get(idx)
            if st is None:
                continue
            k = slot_of[id(p)]
            o, n = int(ghn._offs[k]), p.numel()
            self.exp_avg[o:o + n].copy_(st['exp_avg'].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(st['exp_avg_sq'].reshape(-1))
            steps = max(steps, int(float(st['step'])))
        self.steps = steps


def adamw_reference_(p, g, m, v, sumsq, step, lr, betas, eps, weight_decay, max_norm, inv_scale):
    """torch restatement of one GHN3_OP_ADAMW launch on views of the flat buffers (host-side reference of the sharded step's
    CPU tests; the GPU path runs the HIP op): g / scale, clip coefficient from the GLOBAL squared norm `sumsq`, decoupled
    weight decay, bias-corrected moments -- torch.optim.AdamW's update.  A non-finite norm leaves everything untouched."""
    norm = float(sumsq) ** 0.5 * inv_scale
    if not np.isfinite(norm):
        return
    coef = inv_scale * (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0)
    gg = g * coef
    p.mul_(1.0 - lr * weight_decay)
    m.mul_(betas[0]).add_(gg, alpha=1.0 - betas[0])
    v.mul_(betas[1]).addcmul_(gg, gg, value=1.0 - betas[1])
    denom = (v / (1.0 - betas[1] ** step)).sqrt_().add_(eps)
    p.addcdiv_(m / (1.0 - betas[0] ** step), denom, value=-lr)


STATE16_LIMIT = 1 << 24        # step numbers and seeds of the bf16-state ops travel in floats: exact below 2^24


def _mix32(x):
    """The 32-bit integer hash of the bf16-state kernels (include/ghn3_hip.h, GHN3_OP_ADAMW_S16) on a uint32 array."""
    x = np.array(x, dtype=np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def state16_random_bits(seed, step, base, n):
    """One hash per element of the flat range [base, base + n): the low half rounds exp_avg, the high half exp_avg_sq.  A
    function of seed, step and flat index alone."""
    key = _mix32([(int(seed) * 0x9e3779b9 + int(step)) & 0xffffffff])[0]
    idx = ((np.arange(n, dtype=np.int64) + int(base)) & 0xffffffff).astype(np.uint32)
    return _mix32(idx ^ key)


def bf16_stochastic_round(x, r16):
    """bf16 bit patterns (uint16) of the fp32 array x: 16 random bits added to the low half of the pattern, then truncated."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) + r16.astype(np.uint32)
    return (u >> np.uint32(16)).astype(np.uint16)


def adamw_state16_reference_(p, g, m, v, sumsq, step, lr, betas, eps, weight_decay, max_norm, inv_scale, seed=0, base=0):
    """Host restatement of one GHN3_OP_ADAMW_S16 launch, operation for operation (numpy, in place): p, g are fp32 CPU tensors,
    m, v torch.bfloat16 ones, all views of flat buffers starting at flat element `base`.  The stored moments are widened
    (exact), the update runs in fp32 with the kernel's roundings (adamw_element: the two moment updates are fused
    multiply-adds, every other product is rounded on its own), p takes the unrounded moments, and each moment is stored by
    stochastic rounding with the bits of state16_random_bits.  A non-finite norm leaves everything untouched.  This is the
    rule the CPU tests check (unbiased, no stall, independent of the partition) and the GPU tests compare bits against."""
    f = np.float32
    if not 0 <= int(step) < STATE16_LIMIT:
        raise ValueError('step %r outside [0, 2^24)' % (step,))
    ss = f(float(sumsq)) if sumsq is not None else None
    if ss is not None and not np.isfinite(ss):
        return
    inv = f(inv_scale) if inv_scale > 0 else f(1)
    clip = inv
    if ss is not None and max_norm > 0:
        clip = f(inv * min(f(1), f(max_norm) / f(f(np.sqrt(ss) * inv) + f(1e-6))))
    b1, b2 = f(betas[0]), f(betas[1])
    bc1, bc2s = f(1.0 - betas[0] ** step), np.sqrt(f(1.0 - betas[1] ** step))
    stepsz = f(f(lr) / bc1)
    decay = f(f(1) - f(f(lr) * f(weight_decay)))
    pn, gn = p.numpy(), g.numpy()
    mb, vb = m.view(torch.int16).numpy().view(np.uint16), v.view(torch.int16).numpy().view(np.uint16)
    mf = (mb.astype(np.uint32) << np.uint32(16)).view(np.float32)
    vf = (vb.astype(np.uint32) << np.uint32(16)).view(np.float32)

    def fma(a, x, y):            # one rounding (the product of two fp32 values is exact in float64)
        return (np.float64(a) * x.astype(np.float64) + y.astype(np.float64)).astype(np.float32)
    gi = gn * clip
    mi = fma(b1, mf, (f(1) - b1) * gi)
    vi = fma(b2, vf, ((f(1) - b2) * gi) * gi)
    den = np.sqrt(vi) / bc2s + f(eps)
    pn[...] = pn * decay - (stepsz * mi) / den
    h = state16_random_bits(seed, step, base, pn.size).reshape(pn.shape)
    mb[...] = bf16_stochastic_round(mi, h & np.uint32(0xffff))
    vb[...] = bf16_stochastic_round(vi, h >> np.uint32(16))


class ShardedAdamW:
    """
    The optimizer step split over the data-parallel ranks (ZeRO-1 shape; round 5).

    The replicated trainer all-reduces 2.62 GB of gradients (ghn3xlm16) and then EVERY rank streams the same 18 GB through
    AdamW (3.7 ms).  Here the gradient exchange stops after its reduce-scatter half (FlatGradReducer(gather=False)): a rank
    holds the mean gradient of 1 / W of every chunk of the flat buffer, updates exactly those parameters (clip coefficient
    from the all-reduced squared norm: one scalar) and all-gathers the updated PARAMETERS -- the same bytes on the wire as
    the all-gather half of the gradient exchange it replaces, AdamW's HBM traffic divided by W (0.5 ms at W = 8).
    Parameters after a step are bit-identical to the replicated path with the same exchange (every element is reduced once,
    on its owner, in both).  The 16-bit copies of decoder.conv.2.weight are re-cast by the next forward (the fused
    GHN3_OP_ADAMW_CAST16 works on whole 64 x 64 tiles of the matrix, not on arbitrary shards): 1.2 ms, against 3.2 ms saved
    at W = 8.

    `update(lo, hi, sumsq, step)`: applies AdamW to the range of the flat buffers; default = the HIP op on the GHN's buffers,
    tests on CPU pass a torch restatement (adamw_reference_).
    """

    def __init__(self, ghn=None, flat=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0,
                 update=None, local_sumsq=None):
        self.ghn = ghn
        self.flat = ghn._flat if flat is None else flat
        self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm = lr, betas, eps, weight_decay, max_grad_norm
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.steps = 0
        self._update, self._local_sumsq = update, local_sumsq
        self.scal = torch.zeros(16 + 8192, dtype=torch.float32, device=self.flat.device)

    def _hip_ops(self, recs, bufs):
        ops = np.zeros(len(recs), dtype=L.OP_DT)
        ops['r']['buf'][:] = -1
        for k, fill in enumerate(recs):
            fill(ops[k])
        self.ghn._ctx().run(ops, np.zeros(0, dtype=L.PROBLEM_DT), np.asarray(bufs, dtype=np.uint64),
                            torch.cuda.current_stream().cuda_stream)

    def step(self, gflat, reducer, grad_scale=1.0):
        """gflat: the flat gradient buffer after a backward whose exchange was `reducer` = FlatGradReducer(gather=False) --
        reducer.owned / .replicated say which ranges hold the mean gradient here.  Returns the global gradient norm."""
        import torch.distributed as dist
        flat = self.flat
        W = dist.get_world_size() if dist.is_initialized() else 1
        rank = dist.get_rank() if dist.is_initialized() else 0
        self.steps += 1
        own, rep = sorted(reducer.owned), sorted(reducer.replicated)
        # reducer.gather (the exchange also all-gathered the GRADIENTS): the replicated update -- every rank updates every
        # element, nothing to gather afterwards; the squared norm is still summed shard-wise (1 / W of the buffer per rank +
        # one scalar all-reduce), so both modes clip with the same bits
        update_all = bool(getattr(reducer, 'gather', False))
        ranges = [(0, flat.numel())] if update_all else sorted(own + rep)
        norm_ranges = sorted(own + (rep if rank == 0 else []))             # (every element counted on exactly one rank)
        hip = self._update is None
        inv_scale = 1.0 / float(grad_scale)
        if hip:
            bufs = [flat.data_ptr(), gflat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                    self.scal.data_ptr(), self.scal.data_ptr() + 64]

            def memset(op):
                op['kind'], op['r']['buf'][0], op['i'][0] = L.OP_MEMSET0, 4, 4

            def sumsq(lo, hi):
                def f(op):
                    op['kind'] = L.OP_SUMSQ
                    op['r']['buf'][:3] = (4, 1, 5)
                    op['r']['off'][1] = 4 * lo
                    op['i'][0] = hi - lo
                return f
            self._hip_ops([memset] + [sumsq(lo, hi) for lo, hi in norm_ranges], bufs)
            total = self.scal[:1]
        else:
            total = torch.zeros(1, dtype=torch.float32, device=flat.device)
            for lo, hi in norm_ranges:
                total += (self._local_sumsq or (lambda t: (t.double() ** 2).sum().float()))(gflat[lo:hi])
        if W > 1:
            dist.all_reduce(total, op=dist.ReduceOp.SUM)
        if hip:
            hyper = (self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
                     1.0 - self.betas[0] ** self.steps, 1.0 - self.betas[1] ** self.steps)

            def adamw(lo, hi):
                def f(op):
                    op['kind'] = L.OP_ADAMW
                    op['r']['buf'][:5] = (0, 1, 2, 3, 4)
                    op['r']['off'][:4] = 4 * lo
                    op['i'][0] = hi - lo
                    for k, h in enumerate(hyper):
                        op['i'][1 + k] = _dbits(h)
                    op['f'][0] = float(self.max_grad_norm or 0.0)
                    op['f'][1] = inv_scale
                return f
            self._hip_ops([adamw(lo, hi) for lo, hi in ranges], bufs)
            self.ghn.params_changed()
        else:
            for lo, hi in ranges:
                self._update(flat[lo:hi], gflat[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi], total, self.steps,
                             self.lr, self.betas, self.eps, self.weight_decay, float(self.max_grad_norm or 0.0), inv_scale)
        # all-gather of the updated parameters: the geometry of the gradient chunks (replicated tails are identical already)
        if (W > 1 or reducer.force) and not update_all:
            for (s, main), (lo, hi) in zip(reducer.chunks, reducer.owned):
                dist.all_gather_into_tensor(flat[s:s + main], flat[lo:hi].clone())
        return total.sqrt() * inv_scale


# ---------------------------------------------------------------------------------------------------------------------
# Plain networks (train_ddp.py): clip_grad_norm_ + torch.optim.SGD over separate parameter tensors
# ---------------------------------------------------------------------------------------------------------------------
MT_CHUNK = 8192                       # include/ghn3_hip.h GHN3_MT_CHUNK


class _MtTensor(ctypes.Structure):
    _fields_ = [('p', ctypes.c_void_p), ('m', ctypes.c_void_p), ('n', ctypes.c_int64)]


class _MtChunk(ctypes.Structure):
    _fields_ = [('tensor', ctypes.c_int32), ('_pad', ctypes.c_int32), ('first', ctypes.c_int64)]


class _MtSgdArgs(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ('lr', 'momentum', 'weight_decay', 'max_norm', 'inv_scale')] + \
        [('nesterov', ctypes.c_int32)]


_MT_TENSOR_DT = np.dtype([('p', '<u8'), ('m', '<u8'), ('n', '<i8')])
_MT_CHUNK_DT = np.dtype([('tensor', '<i4'), ('_pad', '<i4'), ('first', '<i8')])
assert _MT_TENSOR_DT.itemsize == ctypes.sizeof(_MtTensor) == 24 and _MT_CHUNK_DT.itemsize == ctypes.sizeof(_MtChunk) == 16


def flat_layout(sizes):
    """Offsets (int64, in floats) of tensors of the element counts `sizes` inside one flat fp32 buffer: every segment is padded
    to 4 floats, so each starts on 16 bytes; the last entry is the buffer's length.  A function of the sizes alone."""
    offs = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum([(int(n) + 3) // 4 * 4 for n in sizes], dtype=np.int64, out=offs[1:])
    return offs


def _mt_tables(base, offs, sizes, device):
    """Device tables over the segments of a flat buffer at address `base` (layout `offs`) that hold tensors of `sizes` elements:
    the ghn3_mt_tensor records (p = the segment, m = 0), the chunk list, the number of chunks.  Empty tensors have no chunk."""
    rec = np.zeros(len(sizes), dtype=_MT_TENSOR_DT)
    chunks = []
    for k, n in enumerate(sizes):
        rec[k] = (base + 4 * int(offs[k]), 0, n)
        chunks += [(k, 0, first) for first in range(0, n, MT_CHUNK)]
    ch = np.array(chunks, dtype=_MT_CHUNK_DT)
    return torch.from_numpy(rec.view(np.uint8)).to(device), torch.from_numpy(ch.view(np.uint8)).to(device), len(ch)


def _mt_wire(name, flat, offs, tensors):
    """ghn3_mt_pack / ghn3_mt_unpack of a list of fp32 CUDA tensors and their segments of `flat`, tables built on the spot (the
    start-up paths; FusedSGD keeps its tables)."""
    dev = flat.device
    for t in tensors:
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise ValueError('%s takes contiguous fp32 tensors on the flat buffer\'s device' % name)
    sizes = [t.numel() for t in tensors]
    assert flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() >= int(offs[len(sizes)])
    lib = L.load()
    with torch.cuda.device(dev):
        rec, chunks, n_chunks = _mt_tables(flat.data_ptr(), offs, sizes, dev)
        ptrs = torch.from_numpy(np.asarray([t.data_ptr() for t in tensors], dtype=np.int64)).to(dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        L._check(getattr(lib, name)(rec.data_ptr(), ptrs.data_ptr(), chunks.data_ptr(), n_chunks, stream), name)


def mt_pack(flat, offs, tensors):
    """flat[offs[k] : offs[k] + n_k] = tensors[k], bit for bit, in one launch (ghn3_mt_pack); the pad floats are not written."""
    _mt_wire('ghn3_mt_pack', flat, offs, tensors)


def mt_unpack(flat, offs, tensors):
    """tensors[k] = flat[offs[k] : offs[k] + n_k], bit for bit, in one launch (ghn3_mt_unpack)."""
    _mt_wire('ghn3_mt_unpack', flat, offs, tensors)


class _FlatGrads:
    """The flat fp32 gradient buffer of an optimizer whose gradients go through a FlatGradReducer: one segment per parameter that
    had requires_grad when the optimizer was built, in flat_layout.  The layout depends on the parameter list alone -- the
    collectives of the exchange must have the same sequence and sizes on every rank -- so under a reducer every such parameter
    needs a gradient in every step (DistributedDataParallel with find_unused_parameters=False asks the same).  Allocated once
    with zeros: the pad floats are defined and an average of zeros is zero."""

    def __init__(self, params):
        self.idx = [i for i, p in enumerate(params) if p.requires_grad]
        self.sizes = [params[i].numel() for i in self.idx]
        self.offs = flat_layout(self.sizes)
        self.flat = torch.zeros(int(self.offs[-1]), dtype=torch.float32, device=params[0].device)
        self.params = params

    def grads(self):
        """The gradients of the layout's parameters as dense fp32 tensors on the device, or the RuntimeError."""
        out = []
        for i in self.idx:
            p = self.params[i]
            g = p.grad
            if g is None:
                raise RuntimeError('parameter %d (shape %s) has requires_grad but no gradient: under a gradient reducer every '
                                   'parameter of the layout takes part in every step (the exchange has the same sizes on every '
                                   'rank); freeze it before the optimizer is built' % (i, tuple(p.shape)))
            if g.dtype != torch.float32 or g.is_sparse or g.device != p.device or not g.is_contiguous():
                g = (g.to_dense() if g.is_sparse else g).to(device=p.device, dtype=torch.float32).contiguous()
            out.append(g)
        return out

    def view(self, k):
        o = int(self.offs[k])
        return self.flat[o:o + self.sizes[k]].view(self.params[self.idx[k]].shape)

    def exchange(self, reducer):
        reducer.begin()
        reducer.finish(self.flat)

    def gather_torch(self, reducer, grads):
        """Pack `grads` (self.grads()), exchange and return views of the averaged gradients, in torch expressions (CPU tensors,
        StockSGD)."""
        with torch.no_grad():
            for k, g in enumerate(grads):
                self.view(k).copy_(g)
            self.exchange(reducer)
        return [self.view(k) for k in range(len(self.idx))]


def sgd_reference_(params, grads, bufs, lr, momentum=0.0, weight_decay=0.0, nesterov=False, max_norm=0.0, inv_scale=1.0):
    """torch restatement of one FusedSGD step (ghn3_mt_sumsq + ghn3_mt_sgd), in place on lists of tensors of any float type:
    the gradients' global norm as clip_grad_norm_ takes it (the norm of the per-tensor norms), g / scale times the clip
    coefficient, then torch.optim.SGD's update with dampening 0 on momentum buffers that start at zero.  `grads` are not
    modified; bufs[i] is ignored when momentum == 0.  Returns the unscaled norm (0-d tensor); when it is not finite nothing was
    touched.  In float64 this is the oracle of the GPU tests; on fp32 CPU tensors it is FusedSGD's step, operation for
    operation what the stock pair computes."""
    if not grads:
        return torch.zeros(())
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads])) * inv_scale
    if not bool(torch.isfinite(norm)):
        return norm
    coef = inv_scale * (min(1.0, max_norm / (float(norm) + 1e-6)) if max_norm > 0 else 1.0)
    for p, g, m in zip(params, grads, bufs):
        d = g * coef if coef != 1.0 else g
        if weight_decay != 0:
            d = d.add(p, alpha=weight_decay)
        if momentum != 0:
            m.mul_(momentum).add_(d)
            d = d.add(m, alpha=momentum) if nesterov else m
        p.add_(d, alpha=-lr)
    return norm


class FusedSGD:
    """clip_grad_norm_ + torch.optim.SGD (same update rule, dampening 0) for a list of separate parameter tensors: two
    launches over a table of tensors (ghn3_mt_sumsq, ghn3_mt_sgd), whatever their number, instead of some ten foreach
    launches and five passes over the bytes.

    The momentum of all parameters lives in ONE buffer of the optimizer (segments padded to 4 floats, so each starts on 16
    bytes); state_dict() hands out views of it.  The buffers start at zero, which with dampening 0 is torch's first-step
    `buf = clone(d)` bit for bit.  The chunk table and the parameter / momentum pointers go to the device once per set of
    parameters that take part; the gradient pointers -- autograd allocates the gradients anew after zero_grad(set_to_none) --
    go up once per step through the pinned ring.  CPU parameters take sgd_reference_ (host logic can be tested anywhere).

    reducer (a ddp_utils.FlatGradReducer; None: nothing below applies): the data-parallel step.  The gradients are gathered into
    ONE flat buffer laid out like the momentum buffer (ghn3_mt_pack over the same chunk list and the gradient pointers the
    step uploads anyway), the reducer averages that buffer over the ranks, and norm + update read the averaged gradients from
    it through a static pointer table: p.grad stays what autograd wrote.  Every parameter that had requires_grad at construction
    is in the layout and must have a gradient in every step (_FlatGrads); the others are left out.  The returned norm is that of
    the averaged gradient, the same bits on every rank: a non-finite value on any rank skips the update on all of them."""

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=0.0,
                 nan_guard=True, reducer=None):
        if dampening != 0:
            raise ValueError('FusedSGD implements dampening = 0 only (momentum buffers start at zero and no first-step flag '
                             'exists on the device), got %r' % (dampening,))
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError('lr, momentum and weight_decay must not be negative')
        if nesterov and momentum <= 0:
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError('FusedSGD takes one parameter group')
            params = list(params[0]['params'])
        if not params:
            raise ValueError('FusedSGD got an empty parameter list')
        dev = params[0].device
        for p in params:
            if p.dtype != torch.float32 or p.device != dev or p.is_sparse or not p.is_contiguous():
                raise ValueError('FusedSGD takes dense contiguous fp32 parameters on one device')
        self.params, self.device = params, dev
        self.lr, self.momentum, self.weight_decay, self.nesterov = lr, momentum, weight_decay, bool(nesterov)
        self.max_grad_norm, self.nan_guard = max_grad_norm, nan_guard
        self._offs = flat_layout([p.numel() for p in params])
        self.momentum_buffer = torch.zeros(int(self._offs[-1]), dtype=torch.float32, device=dev) if momentum != 0 else None
        self._stepped = set()           # parameters that had a gradient in some step: the ones torch keeps a state entry for
        self._table = None
        self.steps = 0
        self.reducer = reducer
        self._gflat = _FlatGrads(params) if reducer is not None else None

    def _buf(self, i):
        if self.momentum_buffer is None:
            return None
        o = int(self._offs[i])
        return self.momentum_buffer[o:o + self.params[i].numel()].view(self.params[i].shape)

    def zero_grad(self, set_to_none=True):
        for p in self.params:
            if p.grad is not None:
                if set_to_none:
                    p.grad = None
                else:
                    p.grad.detach_().zero_()

    # ------------------------------------------------------------------ the step
    def _build_table(self, active, pptr):
        """Device tables for the parameters `active` (indices) at the addresses `pptr`: records, chunk list, scratch."""
        mbase = self.momentum_buffer.data_ptr() if self.momentum_buffer is not None else 0
        rec = np.zeros(len(active), dtype=_MT_TENSOR_DT)
        chunks = []
        for k, i in enumerate(active):
            n = self.params[i].numel()
            rec[k] = (pptr[k], mbase + 4 * int(self._offs[i]) if mbase else 0, n)
            chunks += [(k, 0, first) for first in range(0, n, MT_CHUNK)]
        ch = np.array(chunks, dtype=_MT_CHUNK_DT)
        dev = self.device
        tb = {'active': active, 'pptr': pptr, 'n_chunks': len(ch),
              'rec': torch.from_numpy(rec.view(np.uint8)).to(dev), 'chunks': torch.from_numpy(ch.view(np.uint8)).to(dev),
              'scal': torch.zeros(4 + len(ch), dtype=torch.float32, device=dev)}        # [norm^2, pad | one partial per chunk]
        if self._gflat is not None:
            # (reducer: the segments of the flat gradient buffer, as pack's records and as the step's gradient pointers: static)
            fl = self._gflat
            at = {i: k for k, i in enumerate(fl.idx)}
            seg = np.zeros(len(active), dtype=_MT_TENSOR_DT)
            for k, i in enumerate(active):
                seg[k] = (fl.flat.data_ptr() + 4 * int(fl.offs[at[i]]), 0, self.params[i].numel())
            tb['seg'] = torch.from_numpy(seg.view(np.uint8)).to(dev)
            tb['fptr'] = torch.from_numpy(seg['p'].astype(np.int64)).to(dev)
            tb['views'] = [fl.view(at[i]) for i in active]
        return tb

    def step(self, grad_scale=1.0):
        """One update from the parameters' .grad; grad_scale: the loss scale the gradients carry (they are divided by it inside
        the kernel).  Returns the gradient norm (device scalar, like clip_grad_norm_) when clipping or the NaN guard is on, else
        None; when it is not finite no parameter and no momentum buffer changed.  A parameter without a gradient or with
        requires_grad=False does not take part, as in torch.  With a reducer: see the class."""
        if self._gflat is not None:
            return self._step_reduced(grad_scale)
        active, grads = [], []
        for i, p in enumerate(self.params):
            g = p.grad
            if g is None or not p.requires_grad:
                continue
            self._stepped.add(i)
            if p.numel() == 0:                    # (torch keeps a state entry for it; there is nothing to update)
                continue
            if g.dtype != torch.float32 or g.is_sparse or g.device != p.device or not g.is_contiguous():
                g = (g.to_dense() if g.is_sparse else g).to(device=p.device, dtype=torch.float32).contiguous()
            active.append(i)
            grads.append(g)
        self.steps += 1
        guard = bool(self.max_grad_norm and self.max_grad_norm > 0) or self.nan_guard
        inv_scale = 1.0 / float(grad_scale)
        if self.device.type != 'cuda':
            with torch.no_grad():
                norm = sgd_reference_([self.params[i] for i in active], grads, [self._buf(i) for i in active], self.lr,
                                      self.momentum, self.weight_decay, self.nesterov,
                                      float(self.max_grad_norm or 0.0) if guard else 0.0, inv_scale)
            return norm if guard else None
        active = tuple(active)
        pptr = [self.params[i].data_ptr() for i in active]
        tb = self._table
        if tb is None or tb['active'] != active or tb['pptr'] != pptr:
            tb = self._table = self._build_table(active, pptr)
        if not active:
            return torch.zeros((), device=self.device) if guard else None
        lib = L.load()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            gptr = pinned_ring(self.device).upload(np.asarray([g.data_ptr() for g in grads], dtype=np.int64), self.device)
            scal = tb['scal']
            tables = (tb['rec'].data_ptr(), gptr.data_ptr(), tb['chunks'].data_ptr(), tb['n_chunks'])
            if guard:
                L._check(lib.ghn3_mt_sumsq(*tables, scal.data_ptr() + 16, scal.data_ptr(), stream), 'ghn3_mt_sumsq')
            args = _MtSgdArgs(self.lr, self.momentum, self.weight_decay, float(self.max_grad_norm or 0.0), inv_scale,
                              int(self.nesterov))
            L._check(lib.ghn3_mt_sgd(*tables, scal.data_ptr() if guard else None, ctypes.byref(args), stream), 'ghn3_mt_sgd')
        return scal[0].sqrt() * inv_scale if guard else None

    def _step_reduced(self, grad_scale):
        """The step under a reducer: pack, exchange, norm + update from the flat buffer."""
        fl = self._gflat
        grads = fl.grads()                        # (raises before anything is counted or written)
        self._stepped.update(fl.idx)
        self.steps += 1
        guard = bool(self.max_grad_norm and self.max_grad_norm > 0) or self.nan_guard
        inv_scale = 1.0 / float(grad_scale)
        max_norm = float(self.max_grad_norm or 0.0)
        if self.device.type != 'cuda':
            avg = fl.gather_torch(self.reducer, grads)
            with torch.no_grad():
                norm = sgd_reference_([self.params[i] for i in fl.idx], avg, [self._buf(i) for i in fl.idx], self.lr,
                                      self.momentum, self.weight_decay, self.nesterov, max_norm if guard else 0.0, inv_scale)
            return norm if guard else None
        keep = [k for k, n in enumerate(fl.sizes) if n > 0]          # (an empty tensor has no chunk and no record)
        active = tuple(fl.idx[k] for k in keep)
        pptr = [self.params[i].data_ptr() for i in active]
        tb = self._table
        if tb is None or tb['active'] != active or tb['pptr'] != pptr:
            tb = self._table = self._build_table(active, pptr)
        if not active:
            return torch.zeros((), device=self.device) if guard else None
        lib = L.load()
        with torch.cuda.device(self.device):
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            if os.environ.get('GHN3_MT_PACK', '1') != '0':
                gptr = pinned_ring(self.device).upload(np.asarray([grads[k].data_ptr() for k in keep], dtype=np.int64),
                                                       self.device)
                L._check(lib.ghn3_mt_pack(tb['seg'].data_ptr(), gptr.data_ptr(), tb['chunks'].data_ptr(), tb['n_chunks'], stream),
                         'ghn3_mt_pack')
            else:
                # the A/B switch: the same gather by torch's multi-tensor copy (the shorter one on a ResNet-18's 62 tensors, the
                # longer one on a ResNet-50's 161: profiles/r18a_plain_ddp_step.txt)
                torch._foreach_copy_(tb['views'], [grads[k] for k in keep])
            fl.exchange(self.reducer)
            scal = tb['scal']
            tables = (tb['rec'].data_ptr(), tb['fptr'].data_ptr(), tb['chunks'].data_ptr(), tb['n_chunks'])
            if guard:
                L._check(lib.ghn3_mt_sumsq(*tables, scal.data_ptr() + 16, scal.data_ptr(), stream), 'ghn3_mt_sumsq')
            args = _MtSgdArgs(self.lr, self.momentum, self.weight_decay, max_norm, inv_scale, int(self.nesterov))
            L._check(lib.ghn3_mt_sgd(*tables, scal.data_ptr() if guard else None, ctypes.byref(args), stream), 'ghn3_mt_sgd')
        return scal[0].sqrt() * inv_scale if guard else None

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """State in the layout of ``torch.optim.SGD.state_dict()`` over the same parameter list: a checkpoint written by
        either optimizer resumes in the other.  The momentum buffers are views of the optimizer's one buffer."""
        state = {}
        if self.momentum != 0:                    # (torch keeps no state entry at all without a momentum)
            for i in sorted(self._stepped):
                state[i] = {'momentum_buffer': self._buf(i)}
        group = {'lr': self.lr, 'momentum': self.momentum, 'dampening': 0, 'weight_decay': self.weight_decay,
                 'nesterov': self.nesterov, 'maximize': False, 'foreach': None, 'differentiable': False, 'fused': None,
                 'params': list(range(len(self.params)))}
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        """Accepts a ``torch.optim.SGD`` (or FusedSGD) state dict over the same parameter list."""
        groups = sd['param_groups']
        if len(groups) != 1 or len(groups[0]['params']) != len(self.params):
            raise ValueError('one parameter group over the same %d parameters expected' % len(self.params))
        g = groups[0]
        if g.get('dampening', 0) != 0 or g.get('maximize', False):
            raise ValueError('FusedSGD cannot resume a state with dampening or maximize')
        if (float(g['momentum']) != 0) != (self.momentum != 0):
            raise ValueError('momentum %r of the state does not fit an optimizer built with momentum %r'
                             % (g['momentum'], self.momentum))
        self.lr, self.momentum, self.weight_decay = float(g['lr']), float(g['momentum']), float(g['weight_decay'])
        self.nesterov = bool(g['nesterov'])
        if self.momentum_buffer is not None:
            self.momentum_buffer.zero_()
        self._stepped = set()
        for k, idx in enumerate(g['params']):
            st = sd['state'].get(idx)
            if st is None:
                continue
            self._stepped.add(k)
            buf = st.get('momentum_buffer')
            if buf is not None and self.momentum_buffer is not None:
                self._buf(k).copy_(buf)


class StockSGD:
    """nn.utils.clip_grad_norm_ + torch.optim.SGD (foreach) behind FusedSGD's interface: the other side of the Trainer's
    GHN3_FUSED_SGD switch.  Unscale, norm, clip and update are separate torch passes, and skipping a step whose norm is not
    finite costs one host read per step."""

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, max_grad_norm=0.0, reducer=None):
        self.params = list(params)
        # reducer: FusedSGD's data-parallel sequence in torch expressions -- the gradients are copied into the flat layout,
        # averaged by the reducer and copied back into p.grad (where DistributedDataParallel leaves them) for the stock pair
        self.reducer = reducer
        self._gflat = _FlatGrads(self.params) if reducer is not None else None
        self.opt = torch.optim.SGD(self.params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                   nesterov=nesterov)
        self.max_grad_norm = max_grad_norm
        self.steps = 0

    @property
    def lr(self):
        return self.opt.param_groups[0]['lr']

    @lr.setter
    def lr(self, value):
        self.opt.param_groups[0]['lr'] = value

    def zero_grad(self, set_to_none=True):
        self.opt.zero_grad(set_to_none=set_to_none)

    def step(self, grad_scale=1.0):
        if self._gflat is not None:
            avg = self._gflat.gather_torch(self.reducer, self._gflat.grads())
            with torch.no_grad():
                for i, a in zip(self._gflat.idx, avg):
                    self.params[i].grad.copy_(a)
        with_grad = [p for p in self.params if p.grad is not None]
        self.steps += 1
        if not with_grad:
            return torch.zeros((), device=self.params[0].device)
        if float(grad_scale) != 1.0:
            torch._foreach_mul_([p.grad for p in with_grad], 1.0 / float(grad_scale))
        clip = self.max_grad_norm and self.max_grad_norm > 0
        norm = torch.nn.utils.clip_grad_norm_(with_grad, self.max_grad_norm if clip else float('inf'))
        if bool(torch.isfinite(norm)):
            self.opt.step()
        return norm

    def state_dict(self):
        return self.opt.state_dict()

    def load_state_dict(self, sd):
        self.opt.load_state_dict(sd)


def save_checkpoint(path, ghn, optimizer, epoch, step, config=None):
    """Checkpoint in the reference trainer's format (trainer.py:413-426): {'state_dict', 'optimizer', 'epoch', 'step',
    **config}; `ghn3_amd.from_pretrained(path)` and the reference's resume code both read it."""
    ckpt = {'state_dict': {k: v.detach().cpu() for k, v in ghn.state_dict().items()},
            'optimizer': {'state': {i: {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in st.items()}
                                    for i, st in optimizer.state_dict()['state'].items()},
                          'param_groups': optimizer.state_dict()['param_groups']},
            'epoch': epoch, 'step': step}
    ckpt.update(config or {})
    torch.save(ckpt, path)
    return path
