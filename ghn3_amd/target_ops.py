"""
Native execution of target-network layers with GHN-predicted weights, first slice: the chain

    ReLU -> depthwise k x k convolution -> pointwise 1 x 1 convolution -> BatchNorm (batch statistics)

of ``DilConv`` and of each half of ``SepConv`` (/root/reference/ghn3/ops.py:198-240; run at trainer.py:308-319), forward and
backward, as ONE autograd node on the HIP op family ``ghn3_dwpw_bn_fwd / _bwd`` (include/ghn3_hip.h,
ghn3_amd/csrc/target_ops.hip) instead of four ATen / MIOpen modules per direction.

Activations are torch ``channels_last`` tensors (NHWC in memory, NCHW in shape) inside the op family: the kernels take such
storage as it is and return it, so consecutive fused blocks (the two halves of a SepConv) never convert.  At the boundary to
the stock layers the activations are converted (``_hand_on``): the stock ATen / MIOpen layers of this ROCm build return
wrong gradients for channels_last inputs, so the layout is not allowed to leak into them.  The weights are the views of the GHN's flat prediction buffer the GHN assigned to the
layers -- read in place, no copy; their gradients leave as dense tensors for autograd to route back into that buffer.

Two op families, three members each, one per state of the block's norm slot (``_norm_slot``, built once per call):

    norm slot                                          depthwise + pointwise            dense convolution
    BatchNorm2d with batch statistics ('batch')        DwPwBn / dwpw_bn                 ConvBn / conv_bn
    Identity: a network built with norm=None ('none')  DwPw / dwpw                      ConvOnly / conv_only
    BatchNorm2d with running statistics that is not    DwPwBnEval / dwpw_bn_eval        ConvBnEval / conv_bn_eval
    in training mode ('frozen')

(`bn_layer`, ops.py:91-96, puts an Identity in every norm slot of a norm=None network; ``net.eval()`` on a network built with the
default norm='bn-track' freezes the statistics: a per-channel affine map with constants known before the launch, read only --
no gradient, never written.)  GHN3_NATIVE_NONORM=0 / GHN3_NATIVE_EVALBN=0 keep the blocks of the second / third row on the stock
layers.  The three nodes of a family are thin ``autograd.Function`` classes over one forward and one backward
(``_dwpw_forward`` / ``_dwpw_backward``, ``_conv_forward`` / ``_conv_backward``); every runner (``run_block``,
``run_pointwise_block``, ``run_conv_block``, ``run_conv_pair_block``, ``run_factorized_reduce``, ``run_layer_seq``) checks its
layers' attributes, asks ONE dispatch per node (``_dwpw_dispatch`` / ``_conv_dispatch``: the slot's member, its ``applicable``,
the call, the running statistics of the batch member) and hands the result on or runs the stock layers.

WIDE networks (the `wide` evaluation split of DeepNets-1M: up to 2048 channels in the last stage, 8192 into a cell's 1 x 1
preprocessing layer): the fused depthwise + pointwise kernels keep all output columns of a pixel tile in one workgroup and stop at
512 channels, so a chain with max(C_in, C_out) > 512 runs as TWO nodes -- ``Depthwise`` / ``depthwise_relu`` (ghn3_dw_fwd / _bwd:
ReLU + depthwise taps alone, C <= 16384) and the 1 x 1 member of the dense-convolution family that fits the norm slot (``ConvBn``,
``ConvOnly``, ``ConvBnEval`` with relu=False), which takes C_out <= 4096 and C_in <= 16384; ``SqueezeExcite`` takes C, J <= 4096.
GHN3_NATIVE_WIDE=0 keeps every layer above the former limits (512 / 4096 -> 512 / 1024) on the stock layers.  The ``msa`` layers
of ``MsaLayer`` keep their limits (C <= 256, head dim <= 32, hidden <= 1024); above them, up to C <= 1024, head dim <= 64 and
hidden <= 4096, ``MsaWideLayer`` (ghn3_msa_wide_*, ghn3_amd/csrc/tnet_msa_wide.hip) takes the layer when GHN3_NATIVE_MSA_WIDE=1
-- opt-in: by default a wide ViT-style network still runs its msa layers on the stock path.

The patch embedding of the ViT-style networks (``run_conv_layer``): 3 x 3 / stride 3 on CIFAR-sized inputs runs on ``ConvOnly``;
16 x 16 / stride 16 on ImageNet-sized inputs -- a kernel the dense-convolution op refuses -- on ``PatchEmbed`` / ``patch_embed``
(ghn3_patch_fwd / _bwd, ghn3_amd/csrc/tnet_patch.hip): non-overlapping windows as a GEMM over the image as stored.
GHN3_NATIVE_STEM=0 keeps the layer stock.

Plain ``torch.nn`` networks (ResNet-shaped: ``conv -> BatchNorm -> ReLU``, and ``conv -> BatchNorm -> (+ skip) -> ReLU`` at the end of a
block -- the ReLU BEHIND the norm layer, which no member above has) run on the "act" members of the dense-convolution family,
``ConvBnAct`` / ``conv_bn_act`` (batch statistics) and ``ConvBnActEval`` / ``conv_bn_act_eval`` (running statistics), through the
runner ``run_conv_bn_act(conv, bn, x, residual=None)``; ``ghn3_amd.nativize`` (native_net.py) finds these windows in a traced
module.  GHN3_NATIVE_ACT=0 keeps them stock.  A BatchNorm2d [-> ReLU] that follows NO convolution (a DenseNet's dense layer, a
pre-activation residual block) has a node of its own, ``BnAct`` / ``bn_act`` and ``BnActEval`` / ``bn_act_eval`` (ghn3_bn_act_*,
csrc/tnet_bnact.hip), through ``run_bn_act(bn, x, relu)``; only ``nativize(windows='all')`` asks for it, and GHN3_NATIVE_BNACT=0
keeps it stock there too.  A convolution WITH a bias (``nn.Conv2d``'s default: VGG, AlexNet, SqueezeNet, networks without norm
layers) runs on the "bias" member, ``ConvBiasAct`` / ``conv_bias_act`` (ghn3_conv_bias_act_*: convolution + bias [+ skip]
[-> ReLU], nothing saved but x, w and the result), through ``run_conv_bias_act(conv, x, relu, residual=None)``; only
``nativize(biased=True)`` asks for it, and GHN3_NATIVE_BIAS=0 keeps it stock there too.

``DwPwBn.applicable`` states what the kernels take (fp32 CUDA tensors, batch statistics, C <= 512, ks <= 7); a layer
outside of it goes to the two-node form above or keeps the stock path.  There is no CPU implementation: on a CPU tensor the
stock path runs (the target networks themselves are torch modules), and ``dwpw_bn`` raises without the library.
"""

import collections
import ctypes
import math
import os

import torch
import torch.nn.functional as F

from . import _lib as L


class _Desc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C_in', 'C_out', 'ks', 'stride', 'pad', 'dil', 'Ho', 'Wo')] + \
        [('eps', ctypes.c_float)]


def _desc(x, C_out, ks, stride, pad, dil, eps):
    N, C, H, W = x.shape
    Ho = (H + 2 * pad - dil * (ks - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (ks - 1) - 1) // stride + 1
    return _Desc(N, H, W, C, C_out, ks, stride, pad, dil, Ho, Wo, float(eps))


def _ptr(t):
    """The address of t's storage (an int: ctypes converts it for the c_void_p parameters); None, a null pointer, for None."""
    return None if t is None else t.data_ptr()


def _ptrs(*tensors):
    """_ptr of every argument, in one call: a launch passes ten or more."""
    return [None if t is None else t.data_ptr() for t in tensors]


def _autocast_excludes():
    """Under torch.autocast the fused layers still run -- in fp32, on the fp32 tensors the GHN predicted and the fp32 activations the
    previous fused layer left (a precision at or above what the stock fp16 / bf16 autocast kernels would use; a 16-bit activation from
    a stock autocast layer makes the next fused layer inapplicable by its dtype check).  GHN3_NATIVE_AMP=0: leave every layer to the
    stock path while autocast is on (the behaviour until round 6)."""
    return torch.is_autocast_enabled() and os.environ.get('GHN3_NATIVE_AMP', '1') == '0'


def _stream():
    """The current HIP stream of the current device as an integer handle (torch.cuda.current_stream() builds a Stream object
    per call: 11 us; this is called twice per fused layer, ~700 times per training step)."""
    raw = getattr(torch._C, '_cuda_getCurrentRawStream', None)
    if raw is None:                                       # (a torch build without the raw accessor)
        return torch.cuda.current_stream().cuda_stream
    return raw(torch.cuda.current_device())


_SCRATCH = {}


def _scratch_floats(fn_name, d, backward):
    """What the C function `fn_name` (ghn3_*_scratch_floats) answers for the descriptor d (a ctypes structure), asked once per
    descriptor."""
    key = (fn_name, bytes(d), backward)
    n = _SCRATCH.get(key)
    if n is None:
        lib = L.load()
        n = int(getattr(lib, fn_name)(ctypes.byref(d), backward))
        if n < 0:
            raise L.Ghn3Error('%s: %s' % (fn_name, lib.ghn3_last_error().decode()))
        _SCRATCH[key] = n
    return n


def lazy_layout(*layers):
    """True when a fused block may hand its NHWC output on as it is: every layer of the block is of the light flavour (whose stock
    Conv2d / BatchNorm2d convert a channels_last input themselves, light_ops._stock_layout) and GHN3_NATIVE_LAZY_LAYOUT is not 0.
    torch.nn-flavour networks keep the conversion at the fused block's boundary."""
    if os.environ.get('GHN3_NATIVE_LAZY_LAYOUT', '1') == '0':
        return False
    return all(not isinstance(m, torch.nn.Module) for m in layers)


def _hand_on(out, keep_layout, *layers):
    """A fused block's NHWC output as the next layer takes it: as it is when the caller keeps the layout or the block's layers
    are of the light flavour (lazy_layout), else as a plain NCHW-contiguous tensor."""
    return out if (keep_layout or lazy_layout(*layers)) else out.contiguous(memory_format=torch.contiguous_format)


def _norm_inputs(bn):
    """(gamma, beta, has_run, batch_stats) of a BatchNorm-like module: its affine pair, whether it carries running statistics,
    and whether this call normalises with the batch's own."""
    has_run = getattr(bn, 'running_mean', None) is not None
    return getattr(bn, 'weight', None), getattr(bn, 'bias', None), has_run, getattr(bn, 'training', True) or not has_run


def enabled():
    """GHN3_NATIVE_OPS=0 keeps every target-network layer on the stock ATen / MIOpen path (A/B measurements)."""
    return os.environ.get('GHN3_NATIVE_OPS', '1') != '0'


def _f32_cuda(*tensors):
    """Every argument is an fp32 CUDA tensor (a plain loop: asked several times per fused layer, and a generator costs more
    than the tests)."""
    for t in tensors:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            return False
    return True


def _native_input(x, switch=None):
    """What every `applicable` asks first: x is a 4-d fp32 CUDA tensor, and neither GHN3_NATIVE_OPS=0, the op's own switch
    (`switch`=0, e.g. 'GHN3_NATIVE_CONV') nor autocast with GHN3_NATIVE_AMP=0 keeps the layer on the stock path."""
    return enabled() and (switch is None or os.environ.get(switch, '1') != '0') and _f32_cuda(x) and x.dim() == 4 and \
        not _autocast_excludes()


def _needs_gpu(name, x):
    if not x.is_cuda:
        raise L.Ghn3Error('%s runs on an MI355X only (no CPU implementation: use the stock torch layers)' % name)


def _no_norm(bn):
    """True for the norm slot of a network built with norm=None (`bn_layer`, ops.py:91-96: an Identity layer of either flavour):
    the block then runs on the no-norm members of the op families (DwPw, ConvOnly).  GHN3_NATIVE_NONORM=0 keeps such blocks on
    the stock layers (the behaviour before these members existed; A/B measurements)."""
    return _is_kind(bn, 'Identity') and os.environ.get('GHN3_NATIVE_NONORM', '1') != '0'


def _frozen_norm(batch_stats):
    """True for a norm layer that normalises with its running statistics in this call (`_norm_inputs`' batch_stats is False:
    the layer carries them and is not in training mode): the block then runs on the frozen-statistics members of the op families
    (DwPwBnEval, ConvBnEval).  GHN3_NATIVE_EVALBN=0 keeps such blocks on the stock layers (the behaviour before these members
    existed; A/B measurements)."""
    return not batch_stats and os.environ.get('GHN3_NATIVE_EVALBN', '1') != '0'


def _frozen_stats_ok(running_mean, running_var, C_out):
    return _f32_cuda(running_mean, running_var) and running_mean.numel() == C_out and running_var.numel() == C_out


def _wide():
    """Asked only for a layer wider than the limits the native layers had before they took wide networks: GHN3_NATIVE_WIDE=0
    keeps such a layer on the stock path (that behaviour, for A/B measurements)."""
    return os.environ.get('GHN3_NATIVE_WIDE', '1') != '0'


def _wants_grad(*tensors):
    """Whether a node's backward can ever run: grad mode is on and some input requires a gradient (asked BEFORE Function.apply,
    which switches grad mode off for its forward)."""
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in tensors)


def _is_kind(m, name):
    return type(m).__name__ == name


def _carve(like, n_scratch, *shapes, norm=0):
    """ONE allocation for a backward's parameter gradients and its scratch area (a call is launch- and host-bound for the small
    layers of a CIFAR network), on like's device: a gradient for every shape (None: no such parameter, None for its gradient),
    then -- norm = C_out of a node with a norm layer -- dbeta DIRECTLY FOLLOWED by dgamma (the kernels' own pair of sums:
    bn_param_grads, csrc/target_ops.hip, skips two device copies when dgamma == dbeta + C), then, a multiple of 64 floats from
    the start, the n_scratch floats the kernels asked for.  Returns ([gradient, ..., dbeta, dgamma], scratch)."""
    if norm:
        shapes += ((norm,), (norm,))
    sizes = [0 if s is None else math.prod(s) for s in shapes]
    start = (sum(sizes) + 63) // 64 * 64
    buf = torch.empty(start + n_scratch, dtype=torch.float32, device=like.device)
    grads, at = [], 0
    for s, n in zip(shapes, sizes):
        grads.append(None if s is None else buf[at:at + n].view(s))
        at += n
    return grads, buf[start:]


# ---- ReLU -> depthwise -> pointwise [-> norm]: one forward and one backward for the three members ----------------------------
# norm mode -> (forward, backward, scratch size) of the C side
_DWPW = {'batch': ('ghn3_dwpw_bn_fwd', 'ghn3_dwpw_bn_bwd', 'ghn3_dwpw_scratch_floats'),
         'none': ('ghn3_dwpw_plain_fwd', 'ghn3_dwpw_plain_bwd', 'ghn3_dwpw_plain_scratch_floats'),
         'frozen': ('ghn3_dwpw_frozen_fwd', 'ghn3_dwpw_frozen_bwd', 'ghn3_dwpw_frozen_scratch_floats')}


def _dwpw_applicable(x, w_dw, w_pw, ks, *norm):
    """What the three members ask of the input, the weights and the norm layer's tensors: fp32 CUDA tensors within the fused
    kernels' limits."""
    if not (_native_input(x) and (_f32_cuda(w_pw, *norm) if w_dw is None else _f32_cuda(w_dw, w_pw, *norm))):
        return False
    C_in, C_out = x.shape[1], w_pw.shape[0]
    return C_in % 4 == 0 and C_out % 4 == 0 and C_in <= DWPW_MAX and C_out <= DWPW_MAX and ks <= 7 and \
        x.numel() < 2 ** 31 and (w_dw is None or w_dw.shape[1] == 1) and w_pw.numel() == C_out * C_in


def _dwpw_forward(ctx, mode, x, w_dw, w_pw, norm, stride, pad, dil, eps, keep=True):
    """The forward of DwPwBn ('batch': norm = (gamma, beta)), DwPw ('none': ()) and DwPwBnEval ('frozen': (gamma, beta,
    running_mean, running_var)); w_dw None: no depthwise stage.  One launch; returns (out, stats -- None but for 'batch').  The
    pre-norm tensor z exists for 'batch', and for 'frozen' when `keep`; without `keep` nothing is saved on ctx."""
    lib = L.load()
    fwd, _, scratch_fn = _DWPW[mode]
    ks = 1 if w_dw is None else int(w_dw.shape[-1])
    C_out = int(w_pw.shape[0])
    xc = x.contiguous(memory_format=torch.channels_last)          # (a no-op inside a channels_last network)
    d = _desc(xc, C_out, ks, stride, pad, dil, eps)
    wd, wp = (None if w_dw is None else w_dw.contiguous()), w_pw.contiguous()
    norm = [t.contiguous() for t in norm]
    dev = x.device
    out = torch.empty((d.N, C_out, d.Ho, d.Wo), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
    z = torch.empty_like(out) if (mode == 'batch' or (mode == 'frozen' and keep)) else None
    stats = None
    if mode == 'batch':
        stats = torch.empty(3 * C_out, dtype=torch.float32, device=dev)
        scratch = torch.empty(_scratch_floats(scratch_fn, d, 0), dtype=torch.float32, device=dev)
        tail, saved = (z, out, stats, scratch), (z, stats, norm[0])
    elif mode == 'frozen':
        tail, saved = (z, out), (z, norm[0], norm[2], norm[3])
    else:
        tail, saved = (out,), ()
    L._check(getattr(lib, fwd)(ctypes.byref(d), *_ptrs(xc, wd, wp, *norm, *tail), _stream()), fwd)
    if keep:
        ctx.has_dw = wd is not None
        ctx.save_for_backward(xc, wp, wd if wd is not None else wp, *saved)     # (wp stands in for a missing depthwise weight)
        ctx.cfg = (stride, pad, dil, eps)
    return out, stats


def _dwpw_backward(ctx, mode, dout):
    """The backward of the three members: (dx, dw_dw or None, dw_pw), and (dgamma, dbeta) with a norm layer."""
    lib = L.load()
    _, bwd, scratch_fn = _DWPW[mode]
    xc, wp, wd, *saved = ctx.saved_tensors
    if not ctx.has_dw:
        wd = None
    stride, pad, dil, eps = ctx.cfg
    C_out, ks = int(wp.shape[0]), (1 if wd is None else int(wd.shape[-1]))
    d = _desc(xc, C_out, ks, stride, pad, dil, eps)
    do = dout.contiguous(memory_format=torch.channels_last)
    dx = torch.empty_like(xc)
    grads, scratch = _carve(xc, _scratch_floats(scratch_fn, d, 1), None if wd is None else wd.shape, wp.shape,
                            norm=0 if mode == 'none' else C_out)
    if mode == 'batch':
        (z, stats, g), (dwd, dwp, db, dg) = saved, grads
        args = (do, xc, z, stats, wd, wp, g, dx, dwd, dwp, dg, db, scratch)
    elif mode == 'frozen':
        (z, g, rm, rv), (dwd, dwp, db, dg) = saved, grads
        args = (do, xc, z, wd, wp, g, rm, rv, dx, dwd, dwp, dg, db, scratch)
    else:
        dwd, dwp = grads
        args = (do, xc, wd, wp, dx, dwd, dwp, scratch)
    L._check(getattr(lib, bwd)(ctypes.byref(d), *_ptrs(*args), _stream()), bwd)
    return (dx, dwd, dwp) if mode == 'none' else (dx, dwd, dwp, dg, db)


class DwPwBn(torch.autograd.Function):
    """ReLU -> depthwise k x k convolution -> pointwise 1 x 1 convolution -> BatchNorm with BATCH statistics as ONE autograd
    node on ghn3_dwpw_bn_fwd / _bwd; returns (out, stats), stats not differentiable."""

    @staticmethod
    def applicable(x, w_dw, w_pw, gamma, beta, ks, training_stats=True):
        return bool(training_stats) and _dwpw_applicable(x, w_dw, w_pw, ks, gamma, beta)

    @staticmethod
    def forward(ctx, x, w_dw, w_pw, gamma, beta, stride, pad, dil, eps):
        out, stats = _dwpw_forward(ctx, 'batch', x, w_dw, w_pw, (gamma, beta), stride, pad, dil, eps)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _dstats):
        return _dwpw_backward(ctx, 'batch', dout) + (None,) * 4


class DwPw(torch.autograd.Function):
    """ReLU -> depthwise k x k convolution -> pointwise 1 x 1 convolution WITHOUT a norm layer, as ONE autograd node on
    ghn3_dwpw_plain_fwd / _bwd: `DilConv`, each half of `SepConv` and the 1 x 1 `ReLUConvBN` of a network built with norm=None
    (ops.py:91-96).  Same conventions as DwPwBn (channels_last storage inside, weights read in place, w_dw None: no depthwise
    stage); one launch forward, no pre-norm tensor and no statistics: only x and the weights are saved."""

    applicable = staticmethod(_dwpw_applicable)

    @staticmethod
    def forward(ctx, x, w_dw, w_pw, stride, pad, dil):
        return _dwpw_forward(ctx, 'none', x, w_dw, w_pw, (), stride, pad, dil, 0.0)[0]

    @staticmethod
    def backward(ctx, dout):
        return _dwpw_backward(ctx, 'none', dout) + (None,) * 3


class DwPwBnEval(torch.autograd.Function):
    """ReLU -> depthwise k x k convolution -> pointwise 1 x 1 convolution -> BatchNorm with RUNNING statistics (eval mode) as ONE
    autograd node on ghn3_dwpw_frozen_fwd / _bwd.  Same conventions as DwPwBn.  One launch forward: the norm is applied to the
    product's accumulators; the pre-norm tensor z is allocated, written and saved only when `keep_z` (a backward can follow),
    which does not change the arithmetic of the output.  The statistics are constants: no gradient, never written."""

    @staticmethod
    def applicable(x, w_dw, w_pw, gamma, beta, running_mean, running_var, ks):
        return DwPwBn.applicable(x, w_dw, w_pw, gamma, beta, ks) and gamma.numel() == w_pw.shape[0] and \
            beta.numel() == w_pw.shape[0] and _frozen_stats_ok(running_mean, running_var, w_pw.shape[0])

    @staticmethod
    def forward(ctx, x, w_dw, w_pw, gamma, beta, running_mean, running_var, stride, pad, dil, eps, keep_z):
        return _dwpw_forward(ctx, 'frozen', x, w_dw, w_pw, (gamma, beta, running_mean, running_var), stride, pad, dil, eps,
                             keep_z)[0]

    @staticmethod
    def backward(ctx, dout):
        return _dwpw_backward(ctx, 'frozen', dout) + (None,) * 7


def dwpw_bn(x, w_dw, w_pw, gamma, beta, stride=1, padding=0, dilation=1, eps=1e-5):
    """out = batch_norm(conv1x1(depthwise_conv(relu(x)))) with batch statistics; returns (out, stats) with
    stats = [mean | 1 / sqrt(var + eps) | biased variance] per output channel.  x: (N, C, H, W) fp32 CUDA tensor
    (channels_last preferred), w_dw (C, 1, ks, ks), w_pw (C_out, C, 1, 1) or (C_out, C)."""
    _needs_gpu('dwpw_bn', x)
    return DwPwBn.apply(x, w_dw, w_pw.reshape(w_pw.shape[0], -1), gamma, beta, int(stride), int(padding), int(dilation),
                        float(eps))


def dwpw(x, w_dw, w_pw, stride=1, padding=0, dilation=1):
    """out = conv1x1(depthwise_conv(relu(x))), no norm layer; w_dw None: conv1x1(relu(x)) with the stride.  x: (N, C, H, W) fp32
    CUDA tensor (channels_last preferred), w_dw (C, 1, ks, ks), w_pw (C_out, C, 1, 1) or (C_out, C)."""
    _needs_gpu('dwpw', x)
    return DwPw.apply(x, w_dw, w_pw.reshape(w_pw.shape[0], -1), int(stride), int(padding), int(dilation))


def dwpw_bn_eval(x, w_dw, w_pw, gamma, beta, running_mean, running_var, stride=1, padding=0, dilation=1, eps=1e-5):
    """out = batch_norm(conv1x1(depthwise_conv(relu(x)))) with the given running statistics (a BatchNorm in eval mode); w_dw None:
    no depthwise stage.  Tensors as for dwpw_bn, running_mean / running_var (C_out) fp32.  Under torch.no_grad(), or when no
    input requires a gradient, nothing is saved and only the output is written."""
    _needs_gpu('dwpw_bn_eval', x)
    return DwPwBnEval.apply(x, w_dw, w_pw.reshape(w_pw.shape[0], -1), gamma, beta, running_mean, running_var, int(stride),
                            int(padding), int(dilation), float(eps), _wants_grad(x, w_dw, w_pw, gamma, beta))


def reference(x, w_dw, w_pw, gamma, beta, stride=1, padding=0, dilation=1, eps=1e-5):
    """The four stock layers the op replaces (ops.py:205-212), functional form -- the parity reference of the tests."""
    y = F.conv2d(F.relu(x), w_dw, None, stride, padding, dilation, groups=x.shape[1])
    zz = F.conv2d(y, w_pw.reshape(w_pw.shape[0], -1, 1, 1))
    return F.batch_norm(zz, None, None, gamma, beta, True, 0.1, eps)


class Depthwise(torch.autograd.Function):
    """y = depthwise_conv(relu(x)) as ONE autograd node on ghn3_dw_fwd / _bwd: the first node of a ReLU -> depthwise ->
    pointwise -> norm chain that is wider than DwPwBn / DwPw / DwPwBnEval take (the second one is a 1 x 1 member of the
    dense-convolution family).  Same conventions as DwPw: channels_last storage inside, w_dw (C, 1, ks, ks) read in place;
    only x (and the weight) is saved."""

    @staticmethod
    def applicable(x, w_dw, stride, pad, dil):
        if not (_native_input(x) and _f32_cuda(w_dw) and w_dw.dim() == 4):
            return False
        C, ks = x.shape[1], w_dw.shape[-1]
        if not (C % 4 == 0 and C <= DW_MAX and ks <= 7 and tuple(w_dw.shape) == (C, 1, ks, ks) and stride > 0 and dil > 0 and
                pad >= 0 and x.numel() < 2 ** 31):
            return False
        d = _desc(x, C, ks, stride, pad, dil, 0.0)
        return d.Ho > 0 and d.Wo > 0 and d.N * d.Ho * d.Wo * C < 2 ** 31

    @staticmethod
    def forward(ctx, x, w_dw, stride, pad, dil):
        lib = L.load()
        xc = x.contiguous(memory_format=torch.channels_last)
        wd = w_dw.contiguous()
        d = _desc(xc, int(xc.shape[1]), int(wd.shape[-1]), stride, pad, dil, 0.0)
        y = torch.empty((d.N, d.C_in, d.Ho, d.Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        L._check(lib.ghn3_dw_fwd(ctypes.byref(d), _ptr(xc), _ptr(wd), _ptr(y), _stream()), 'ghn3_dw_fwd')
        ctx.save_for_backward(xc, wd)
        ctx.cfg = (stride, pad, dil)
        return y

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        xc, wd = ctx.saved_tensors
        stride, pad, dil = ctx.cfg
        d = _desc(xc, int(xc.shape[1]), int(wd.shape[-1]), stride, pad, dil, 0.0)
        do = dout.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(xc)
        (dwd,), scratch = _carve(xc, _scratch_floats('ghn3_dw_scratch_floats', d, 1), wd.shape)
        L._check(lib.ghn3_dw_bwd(ctypes.byref(d), _ptr(do), _ptr(xc), _ptr(wd), _ptr(dx), _ptr(dwd), _ptr(scratch), _stream()),
                 'ghn3_dw_bwd')
        return dx, dwd, None, None, None


def depthwise_relu(x, w_dw, stride=1, padding=0, dilation=1):
    """depthwise_conv(relu(x)): x (N, C, H, W) fp32 CUDA tensor (channels_last preferred), w_dw (C, 1, ks, ks); the result is a
    channels_last tensor."""
    _needs_gpu('depthwise_relu', x)
    return Depthwise.apply(x, w_dw, int(stride), int(padding), int(dilation))


# ---- [ReLU ->] dense kh x kw convolution [-> norm]: one forward and one backward for the three members -----------------------
class _ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C_in', 'C_out', 'kh', 'kw', 'stride_h', 'stride_w', 'pad_h', 'pad_w',
                                              'dil', 'Ho', 'Wo', 'relu')] + [('eps', ctypes.c_float)]


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


CONV_NO_NORM = 2                  # include/ghn3_hip.h GHN3_CONV_NO_NORM
CONV_MAX_IN = 16384               # widest input of the dense-convolution op (the kernels walk C_in in chunks)
CONV_MAX_OUT = 4096               # widest output (the kernels split the columns over the grid)
CONV_NARROW = (4096, 512)         # (C_in, C_out) the op took before wide networks: beyond them GHN3_NATIVE_WIDE decides
DWPW_MAX = 512                    # widest side of the fused depthwise + pointwise kernels
DW_MAX = 16384                    # widest stand-alone depthwise op
SE_MAX, SE_NARROW = 4096, 1024    # squeeze-and-excitation: C and J

# norm mode -> (forward, backward, scratch size) of the C side: the no-norm member is ghn3_conv_bn_* with GHN3_CONV_NO_NORM
_CONV = {'batch': ('ghn3_conv_bn_fwd', 'ghn3_conv_bn_bwd', 'ghn3_conv_scratch_floats'),
         'none': ('ghn3_conv_bn_fwd', 'ghn3_conv_bn_bwd', 'ghn3_conv_scratch_floats'),
         'frozen': ('ghn3_conv_frozen_fwd', 'ghn3_conv_frozen_bwd', 'ghn3_conv_frozen_scratch_floats')}


def _conv_applicable(x, w):
    """What ConvBn and ConvOnly both ask of the input and the weight: fp32 CUDA tensors of four dimensions within the kernels'
    limits, and none of the switches that keep the layer on the stock path."""
    if not (_native_input(x, 'GHN3_NATIVE_CONV') and _f32_cuda(w) and w.dim() == 4):
        return False
    C_in, C_out = x.shape[1], w.shape[0]
    if not (C_in % 4 == 0 and C_out % 4 == 0 and C_in <= CONV_MAX_IN and C_out <= CONV_MAX_OUT and w.shape[1] == C_in and
            max(w.shape[2], w.shape[3]) <= 7 and x.numel() < 2 ** 31 and w.numel() < 2 ** 30):
        return False
    return (C_in <= CONV_NARROW[0] and C_out <= CONV_NARROW[1]) or _wide()


def _conv_desc(x, w, stride, pad, dil, relu, eps, no_norm=False):
    N, C, H, W = x.shape
    C_out, _, kh, kw = w.shape
    (sh, sw), (ph, pw) = _pair(stride), _pair(pad)
    Ho = (H + 2 * ph - dil * (kh - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dil * (kw - 1) - 1) // sw + 1
    return _ConvDesc(N, H, W, C, C_out, kh, kw, sh, sw, ph, pw, int(dil), Ho, Wo,
                     int(bool(relu)) | (CONV_NO_NORM if no_norm else 0), float(eps))


def conv_desc_fits(d):
    """The two 2^31 rules of the C side (check_cdesc: input pixels and output pixels, each times the wider channel count) on a
    _ConvDesc: a refusal there would come as an error in the middle of a network, not as a return to the stock layers."""
    widest = max(d.C_in, d.C_out)
    return d.Ho > 0 and d.Wo > 0 and d.N * d.H * d.W * widest < 2 ** 31 and d.N * d.Ho * d.Wo * widest < 2 ** 31


def _conv_geometry_fits(x, w, residual, stride, padding, dilation):
    """What the members that take a torch.nn network's convolution ask of its geometry: positive strides and dilation, padding
    that is not negative, the two 2^31 rules (`conv_desc_fits`), and a skip tensor that is an fp32 CUDA tensor of the output's
    shape (or None)."""
    (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
    if min(sh, sw) <= 0 or min(ph, pw) < 0 or int(dilation) <= 0:
        return False
    d = _conv_desc(x, w, stride, padding, dilation, False, 0.0)
    if not conv_desc_fits(d):
        return False
    return residual is None or (_f32_cuda(residual) and tuple(residual.shape) == (d.N, d.C_out, d.Ho, d.Wo))


def _conv_forward(ctx, mode, x, w, norm, stride, pad, dil, relu, eps, keep=True):
    """The forward of ConvBn ('batch': norm = (gamma, beta)), ConvOnly ('none': ()) and ConvBnEval ('frozen': (gamma, beta,
    running_mean, running_var)).  Returns (out, stats -- None but for 'batch').  z and `keep` as for _dwpw_forward; the no-norm
    member's result is written where the others write z."""
    lib = L.load()
    fwd, _, scratch_fn = _CONV[mode]
    xc = x.contiguous(memory_format=torch.channels_last)
    wc = w.contiguous()
    norm = [t.contiguous() for t in norm]
    d = _conv_desc(xc, wc, stride, pad, dil, relu, eps, no_norm=mode == 'none')
    dev, C_out = x.device, int(wc.shape[0])
    out = torch.empty((d.N, C_out, d.Ho, d.Wo), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
    z = torch.empty_like(out) if (mode == 'batch' or (mode == 'frozen' and keep)) else None
    stats = torch.empty(3 * C_out, dtype=torch.float32, device=dev) if mode == 'batch' else None
    scratch = torch.empty(_scratch_floats(scratch_fn, d, 0), dtype=torch.float32, device=dev)
    if mode == 'batch':
        tail, saved = (z, out, stats, scratch), (z, stats, norm[0])
    elif mode == 'frozen':
        tail, saved = (z, out, scratch), (z, norm[0], norm[2], norm[3])
    else:
        tail, saved = (None, None, out, None, None, scratch), ()
    L._check(getattr(lib, fwd)(ctypes.byref(d), *_ptrs(xc, wc, *norm, *tail), _stream()), fwd)
    if keep:
        ctx.save_for_backward(xc, wc, *saved)
        ctx.cfg = (stride, pad, dil, relu, eps)
    return out, stats


def _conv_backward(ctx, mode, dout):
    """The backward of the three members: (dx, dw), and (dgamma, dbeta) with a norm layer."""
    lib = L.load()
    _, bwd, scratch_fn = _CONV[mode]
    xc, wc, *saved = ctx.saved_tensors
    stride, pad, dil, relu, eps = ctx.cfg
    d = _conv_desc(xc, wc, stride, pad, dil, relu, eps, no_norm=mode == 'none')
    do = dout.contiguous(memory_format=torch.channels_last)
    dx = torch.empty_like(xc)
    grads, scratch = _carve(xc, _scratch_floats(scratch_fn, d, 1), wc.shape, norm=0 if mode == 'none' else int(wc.shape[0]))
    if mode == 'batch':
        (z, stats, g), (dw, db, dg) = saved, grads
        args = (do, xc, z, stats, wc, g, dx, dw, dg, db, scratch)
    elif mode == 'frozen':
        (z, g, rm, rv), (dw, db, dg) = saved, grads
        args = (do, xc, z, wc, g, rm, rv, dx, dw, dg, db, scratch)
    else:
        dw, = grads
        args = (do, xc, None, None, wc, None, dx, dw, None, None, scratch)
    L._check(getattr(lib, bwd)(ctypes.byref(d), *_ptrs(*args), _stream()), bwd)
    return (dx, dw) if mode == 'none' else (dx, dw, dg, db)


class ConvBn(torch.autograd.Function):
    """[ReLU ->] dense kh x kw convolution -> BatchNorm (batch statistics) as ONE autograd node on ghn3_conv_bn_fwd / _bwd
    (round 6: `ReLUConvBN` with a k x k kernel, ops.py:180-198).  Same conventions as DwPwBn: channels_last storage inside,
    the weight [C_out][C_in][kh][kw] read in place, its gradient written in the same order."""

    @staticmethod
    def applicable(x, w, gamma, beta, training_stats=True):
        return bool(training_stats) and _f32_cuda(gamma, beta) and _conv_applicable(x, w) and gamma.numel() == w.shape[0]

    @staticmethod
    def forward(ctx, x, w, gamma, beta, stride, pad, dil, relu, eps):
        out, stats = _conv_forward(ctx, 'batch', x, w, (gamma, beta), stride, pad, dil, relu, eps)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _dstats):
        return _conv_backward(ctx, 'batch', dout) + (None,) * 5


class ConvOnly(torch.autograd.Function):
    """[ReLU ->] dense kh x kw convolution WITHOUT a norm layer (ghn3_conv_bn_fwd / _bwd with GHN3_CONV_NO_NORM): the first half
    of the 1 x k / k x 1 pair of `ReLUConvBN(double=True)` (ops.py:186-190).  Same storage conventions as ConvBn."""

    applicable = staticmethod(_conv_applicable)

    @staticmethod
    def forward(ctx, x, w, stride, pad, dil, relu):
        return _conv_forward(ctx, 'none', x, w, (), stride, pad, dil, relu, 0.0)[0]

    @staticmethod
    def backward(ctx, dz):
        return _conv_backward(ctx, 'none', dz) + (None,) * 4


class ConvBnEval(torch.autograd.Function):
    """[ReLU ->] dense kh x kw convolution -> BatchNorm with RUNNING statistics (eval mode) as ONE autograd node on
    ghn3_conv_frozen_fwd / _bwd.  Same conventions as ConvBn; z and `keep_z` as for DwPwBnEval."""

    @staticmethod
    def applicable(x, w, gamma, beta, running_mean, running_var, stride=1, padding=0, dilation=1):
        if not (ConvBn.applicable(x, w, gamma, beta) and beta.numel() == w.shape[0] and
                _frozen_stats_ok(running_mean, running_var, w.shape[0])):
            return False
        return conv_desc_fits(_conv_desc(x, w, stride, padding, dilation, False, 0.0))

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, stride, pad, dil, relu, eps, keep_z):
        return _conv_forward(ctx, 'frozen', x, w, (gamma, beta, running_mean, running_var), stride, pad, dil, relu, eps, keep_z)[0]

    @staticmethod
    def backward(ctx, dout):
        return _conv_backward(ctx, 'frozen', dout) + (None,) * 8


def conv_bn(x, w, gamma, beta, stride=1, padding=0, dilation=1, relu=True, eps=1e-5):
    """out = batch_norm(conv2d(relu(x) if relu else x, w)) with batch statistics; returns (out, stats) as dwpw_bn does.
    x: (N, C, H, W) fp32 CUDA tensor (channels_last preferred), w (C_out, C, kh, kw)."""
    _needs_gpu('conv_bn', x)
    return ConvBn.apply(x, w, gamma, beta, _pair(stride), _pair(padding), int(dilation), bool(relu), float(eps))


def conv_only(x, w, stride=1, padding=0, dilation=1, relu=False):
    """conv2d(relu(x) if relu else x, w) on the dense-convolution kernels (no bias, groups = 1)."""
    _needs_gpu('conv_only', x)
    return ConvOnly.apply(x, w, _pair(stride), _pair(padding), int(dilation), bool(relu))


def conv_bn_eval(x, w, gamma, beta, running_mean, running_var, stride=1, padding=0, dilation=1, relu=True, eps=1e-5):
    """out = batch_norm(conv2d(relu(x) if relu else x, w)) with the given running statistics (a BatchNorm in eval mode).  Tensors
    as for conv_bn, running_mean / running_var (C_out) fp32.  Under torch.no_grad(), or when no input requires a gradient, nothing
    is saved and only the output is written."""
    _needs_gpu('conv_bn_eval', x)
    return ConvBnEval.apply(x, w, gamma, beta, running_mean, running_var, _pair(stride), _pair(padding), int(dilation), bool(relu),
                            float(eps), _wants_grad(x, w, gamma, beta))


def conv_reference(x, w, gamma, beta, stride=1, padding=0, dilation=1, relu=True, eps=1e-5):
    """The stock layers ConvBn replaces (ops.py:186-193), functional form -- the parity reference of the tests."""
    y = F.conv2d(F.relu(x) if relu else x, w, None, stride, padding, dilation)
    return F.batch_norm(y, None, None, gamma, beta, True, 0.1, eps)


# ---- the "act" member of the dense-convolution family: [ReLU ->] convolution -> norm [-> + skip] -> ReLU -----------------------
# The layer order of ResNet-shaped torch.nn networks (ghn3_amd.nativize puts them onto these nodes): the ReLU sits behind the norm
# layer, and at the end of a residual block the skip tensor is added between the two.  ghn3_conv_bn_act_* / ghn3_conv_frozen_act_*.
_ACT_SCRATCH = 'ghn3_conv_act_scratch_floats'         # (desc, mode): mode = backward | 2 frozen


def act_enabled():
    """GHN3_NATIVE_ACT=0 keeps every conv -> norm [-> add] -> ReLU window on the stock layers."""
    return os.environ.get('GHN3_NATIVE_ACT', '1') != '0'


def _conv_act_applicable(x, w, gamma, beta, residual, stride, padding, dilation):
    """Every limit of the C side (check_cdesc, the two 2^31 rules included) for the two members, and what they ask of the skip
    tensor: an fp32 CUDA tensor of the output's shape."""
    return act_enabled() and ConvBn.applicable(x, w, gamma, beta) and beta.numel() == w.shape[0] and \
        _conv_geometry_fits(x, w, residual, stride, padding, dilation)


def _conv_act_forward(ctx, frozen, x, w, norm, res, stride, pad, dil, relu, eps, keep=True):
    """The forward of ConvBnAct (norm = (gamma, beta)) and ConvBnActEval (norm = (gamma, beta, running_mean, running_var)); res:
    the skip tensor or None.  Returns (out, stats -- None when frozen).  With `keep`, x, w, z, out, gamma and the statistics are
    saved: out, which the next layer reads anyway, carries the ReLU mask."""
    lib = L.load()
    xc = x.contiguous(memory_format=torch.channels_last)
    wc = w.contiguous()
    norm = [t.contiguous() for t in norm]
    rc = None if res is None else res.contiguous(memory_format=torch.channels_last)
    d = _conv_desc(xc, wc, stride, pad, dil, relu, eps)
    dev, C_out = x.device, int(wc.shape[0])
    out = torch.empty((d.N, C_out, d.Ho, d.Wo), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
    z = torch.empty_like(out)
    scratch = torch.empty(_scratch_floats(_ACT_SCRATCH, d, 2 if frozen else 0), dtype=torch.float32, device=dev)
    if frozen:
        stats = None
        L._check(lib.ghn3_conv_frozen_act_fwd(ctypes.byref(d), *_ptrs(xc, wc, *norm, rc, z, out, scratch), _stream()),
                 'ghn3_conv_frozen_act_fwd')
        saved = (norm[0], norm[2], norm[3])
    else:
        stats = torch.empty(3 * C_out, dtype=torch.float32, device=dev)
        L._check(lib.ghn3_conv_bn_act_fwd(ctypes.byref(d), *_ptrs(xc, wc, *norm, rc, z, out, stats, scratch), _stream()),
                 'ghn3_conv_bn_act_fwd')
        saved = (norm[0], stats)
    if keep:
        ctx.save_for_backward(xc, wc, z, out, *saved)
        ctx.cfg = (stride, pad, dil, relu, eps)
        ctx.has_res = res is not None
    return out, stats


def _conv_act_backward(ctx, frozen, dout, want_dres):
    """The backward of both members: (dx, dw, dgamma, dbeta, dres).  The parameter gradients are tensors of their own, not views of
    one buffer with the scratch area (`_carve`): the parameters of a plain network are leaves, whose .grad would pin it."""
    lib = L.load()
    xc, wc, z, out, g, *st = ctx.saved_tensors
    stride, pad, dil, relu, eps = ctx.cfg
    d = _conv_desc(xc, wc, stride, pad, dil, relu, eps)
    do = dout.contiguous(memory_format=torch.channels_last)
    dx, dw = torch.empty_like(xc), torch.empty_like(wc)
    dg, db = torch.empty_like(g), torch.empty_like(g)
    dres = torch.empty_like(out) if (ctx.has_res and want_dres) else None
    scratch = torch.empty(_scratch_floats(_ACT_SCRATCH, d, 3 if frozen else 1), dtype=torch.float32, device=xc.device)
    if frozen:
        rm, rv = st
        L._check(lib.ghn3_conv_frozen_act_bwd(ctypes.byref(d), *_ptrs(do, out, xc, z, wc, g, rm, rv, dx, dw, dg, db, dres, scratch),
                                              _stream()), 'ghn3_conv_frozen_act_bwd')
    else:
        stats, = st
        L._check(lib.ghn3_conv_bn_act_bwd(ctypes.byref(d), *_ptrs(do, out, xc, z, stats, wc, g, dx, dw, dg, db, dres, scratch),
                                          _stream()), 'ghn3_conv_bn_act_bwd')
    return dx, dw, dg, db, dres


class ConvBnAct(torch.autograd.Function):
    """[ReLU ->] dense kh x kw convolution -> BatchNorm (batch statistics) [-> + residual] -> ReLU as ONE autograd node on
    ghn3_conv_bn_act_fwd / _bwd; returns (out, stats), stats not differentiable.  Conventions of ConvBn."""

    @staticmethod
    def applicable(x, w, gamma, beta, residual=None, stride=1, padding=0, dilation=1, training_stats=True):
        return bool(training_stats) and _conv_act_applicable(x, w, gamma, beta, residual, stride, padding, dilation)

    @staticmethod
    def forward(ctx, x, w, gamma, beta, residual, stride, pad, dil, relu, eps):
        out, stats = _conv_act_forward(ctx, False, x, w, (gamma, beta), residual, stride, pad, dil, relu, eps)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _dstats):
        return _conv_act_backward(ctx, False, dout, ctx.needs_input_grad[4]) + (None,) * 5


class ConvBnActEval(torch.autograd.Function):
    """The same behind a BatchNorm with RUNNING statistics (eval mode): ghn3_conv_frozen_act_fwd / _bwd.  Without `keep` (no
    backward can follow) nothing is saved."""

    @staticmethod
    def applicable(x, w, gamma, beta, running_mean, running_var, residual=None, stride=1, padding=0, dilation=1):
        return _conv_act_applicable(x, w, gamma, beta, residual, stride, padding, dilation) and \
            _frozen_stats_ok(running_mean, running_var, w.shape[0])

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, residual, stride, pad, dil, relu, eps, keep):
        return _conv_act_forward(ctx, True, x, w, (gamma, beta, running_mean, running_var), residual, stride, pad, dil, relu, eps,
                                 keep)[0]

    @staticmethod
    def backward(ctx, dout):
        dx, dw, dg, db, dres = _conv_act_backward(ctx, True, dout, ctx.needs_input_grad[6])
        return (dx, dw, dg, db, None, None, dres) + (None,) * 6


def conv_bn_act(x, w, gamma, beta, residual=None, stride=1, padding=0, dilation=1, relu_in=False, eps=1e-5):
    """out = relu(batch_norm(conv2d(relu(x) if relu_in else x, w)) [+ residual]) with batch statistics; returns (out, stats) as
    conv_bn does.  residual: a tensor of the output's shape (any layout; channels_last is read as it is) or None."""
    _needs_gpu('conv_bn_act', x)
    return ConvBnAct.apply(x, w, gamma, beta, residual, _pair(stride), _pair(padding), int(dilation), bool(relu_in), float(eps))


def conv_bn_act_eval(x, w, gamma, beta, running_mean, running_var, residual=None, stride=1, padding=0, dilation=1, relu_in=False,
                     eps=1e-5):
    """The same with the given running statistics (a BatchNorm in eval mode); returns out.  Under torch.no_grad(), or when no
    input requires a gradient, nothing is saved."""
    _needs_gpu('conv_bn_act_eval', x)
    return ConvBnActEval.apply(x, w, gamma, beta, running_mean, running_var, residual, _pair(stride), _pair(padding), int(dilation),
                               bool(relu_in), float(eps), _wants_grad(x, w, gamma, beta, residual))


def conv_act_reference(x, w, gamma, beta, residual=None, stride=1, padding=0, dilation=1, relu_in=False, eps=1e-5,
                       running_mean=None, running_var=None):
    """The stock layers the two nodes replace, functional form -- the parity reference of the tests.  With running statistics
    given they normalise (eval mode) and are not updated."""
    y = F.conv2d(F.relu(x) if relu_in else x, w, None, stride, padding, dilation)
    y = F.batch_norm(y, running_mean, running_var, gamma, beta, running_mean is None, 0.1, eps)
    return F.relu(y if residual is None else y + residual)


# ---- the "bias" member of the dense-convolution family: [ReLU ->] convolution + bias [+ skip] [-> ReLU] ------------------------
# The layers of torch.nn networks WITHOUT norm layers (VGG, AlexNet, SqueezeNet: nn.Conv2d with its default bias=True, then a
# ReLU), and any other biased convolution.  Opt-in through ghn3_amd.nativize(biased=True); ghn3_conv_bias_act_*.
CONV_ACT_OUT = 4                  # include/ghn3_hip.h GHN3_CONV_ACT_OUT
_BIAS_SCRATCH = 'ghn3_conv_bias_act_scratch_floats'   # (desc, backward)


def bias_enabled():
    """GHN3_NATIVE_BIAS=0 keeps every biased-convolution window on the stock layers."""
    return os.environ.get('GHN3_NATIVE_BIAS', '1') != '0'


def _bias_desc(x, w, stride, pad, dil, relu_in, relu):
    d = _conv_desc(x, w, stride, pad, dil, relu_in, 0.0)
    if relu:
        d.relu |= CONV_ACT_OUT
    return d


class ConvBiasAct(torch.autograd.Function):
    """[ReLU ->] dense kh x kw convolution + bias [+ residual] [-> ReLU] as ONE autograd node on ghn3_conv_bias_act_fwd / _bwd.
    Conventions of ConvBn.  Saved between the directions: x, w, and -- with the ReLU -- out, which carries its mask."""

    @staticmethod
    def applicable(x, w, bias, residual=None, stride=1, padding=0, dilation=1):
        """Every limit of the C side (check_cdesc, the two 2^31 rules included), and what the op asks of the bias and the skip
        tensor: fp32 CUDA tensors of C_out elements / of the output's shape."""
        return bias_enabled() and _conv_applicable(x, w) and _f32_cuda(bias) and bias.numel() == w.shape[0] and \
            _conv_geometry_fits(x, w, residual, stride, padding, dilation)

    @staticmethod
    def forward(ctx, x, w, bias, residual, stride, pad, dil, relu, relu_in, keep):
        lib = L.load()
        xc = x.contiguous(memory_format=torch.channels_last)
        wc, bc = w.contiguous(), bias.contiguous()
        rc = None if residual is None else residual.contiguous(memory_format=torch.channels_last)
        d = _bias_desc(xc, wc, stride, pad, dil, relu_in, relu)
        out = torch.empty((d.N, d.C_out, d.Ho, d.Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        scratch = torch.empty(_scratch_floats(_BIAS_SCRATCH, d, 0), dtype=torch.float32, device=x.device)
        L._check(lib.ghn3_conv_bias_act_fwd(ctypes.byref(d), *_ptrs(xc, wc, bc, rc, out, scratch), _stream()), 'ghn3_conv_bias_act_fwd')
        if keep:
            ctx.save_for_backward(xc, wc, *((out,) if relu else ()))
            ctx.cfg = (stride, pad, dil, relu, relu_in)
            ctx.has_res = residual is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        """(dx, dw, dbias, dres): tensors of their own, not views of one buffer with the scratch area (`_carve`) -- the
        parameters of a plain network are leaves, whose .grad would pin it."""
        lib = L.load()
        xc, wc, *saved = ctx.saved_tensors
        stride, pad, dil, relu, relu_in = ctx.cfg
        out = saved[0] if relu else None
        d = _bias_desc(xc, wc, stride, pad, dil, relu_in, relu)
        do = dout.contiguous(memory_format=torch.channels_last)
        dx, dw = torch.empty_like(xc), torch.empty_like(wc)
        db = torch.empty(d.C_out, dtype=torch.float32, device=xc.device)
        dres = torch.empty_like(do) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        scratch = torch.empty(_scratch_floats(_BIAS_SCRATCH, d, 1), dtype=torch.float32, device=xc.device)
        L._check(lib.ghn3_conv_bias_act_bwd(ctypes.byref(d), *_ptrs(do, out, xc, wc, dx, dw, db, dres, scratch), _stream()),
                 'ghn3_conv_bias_act_bwd')
        return (dx, dw, db, dres) + (None,) * 6


def conv_bias_act(x, w, bias, residual=None, stride=1, padding=0, dilation=1, relu=True, relu_in=False):
    """out = act(conv2d(relu(x) if relu_in else x, w, bias) [+ residual]), act = ReLU when `relu` else the identity.  x: (N, C, H, W)
    fp32 CUDA tensor (channels_last preferred), w (C_out, C, kh, kw), bias (C_out), residual: a tensor of the output's shape (any
    layout; channels_last is read as it is) or None.  Under torch.no_grad(), or when no input requires a gradient, nothing is
    saved."""
    _needs_gpu('conv_bias_act', x)
    return ConvBiasAct.apply(x, w, bias, residual, _pair(stride), _pair(padding), int(dilation), bool(relu), bool(relu_in),
                             _wants_grad(x, w, bias, residual))


def conv_bias_act_reference(x, w, bias, residual=None, stride=1, padding=0, dilation=1, relu=True, relu_in=False):
    """The stock layers ConvBiasAct replaces, functional form -- the parity reference of the tests."""
    y = F.conv2d(F.relu(x) if relu_in else x, w, bias, stride, padding, dilation)
    if residual is not None:
        y = y + residual
    return F.relu(y) if relu else y


# ---- a BatchNorm [-> ReLU] that stands alone: ghn3_bn_act_* (csrc/tnet_bnact.hip) -------------------------------------------------
# The leading layers of a DenseNet's dense layer and of a pre-activation residual block: no convolution in front of the norm layer.
# Opt-in through ghn3_amd.nativize(windows='all'); GHN3_NATIVE_BNACT=0 keeps the layers stock even there.
BNACT_MAX_C = 16384
_BNACT_SCRATCH = 'ghn3_bn_act_scratch_floats'         # (desc, mode): mode = backward | 2 frozen


class _BnActDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('P', 'C', 'relu')] + [('eps', ctypes.c_float)]


def bnact_enabled():
    """GHN3_NATIVE_BNACT=0 keeps every stand-alone BatchNorm [-> ReLU] on the stock layers."""
    return os.environ.get('GHN3_NATIVE_BNACT', '1') != '0'


def bn_act_refusal(x, gamma, beta, frozen=False, running_mean=None, running_var=None):
    """Why ghn3_bn_act_* do not take the layer, or None when they do.  The rules in the order they are asked -- those of the
    shape first, so they can be asked of CPU and meta tensors, and they mirror every limit of the C side, so a network never
    meets the C refusal:
      'type'     x a 4-d fp32 tensor with at least one element;
      'channels' C % 4 == 0;
      'width'    C <= BNACT_MAX_C;
      'size'     fewer than 2^31 elements;
      'rows'     batch statistics: P = N H W >= 2 (torch raises for one value per channel: the stock layer has to);
      'params'   gamma, beta (and the running statistics of a frozen layer) fp32 tensors of C elements on x's device;
      'device'   CUDA tensors;
      'switch'   GHN3_NATIVE_BNACT / GHN3_NATIVE_OPS / GHN3_NATIVE_AMP under autocast."""
    if not (torch.is_tensor(x) and x.dim() == 4 and x.dtype == torch.float32 and x.numel() > 0):
        return 'type'
    C = x.shape[1]
    if C % 4:
        return 'channels'
    if C > BNACT_MAX_C:
        return 'width'
    if x.numel() >= 2 ** 31:
        return 'size'
    if not frozen and x.numel() // C < 2:
        return 'rows'
    for t in (gamma, beta) + ((running_mean, running_var) if frozen else ()):
        if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() == C and t.device == x.device):
            return 'params'
    if not x.is_cuda:
        return 'device'
    if not (enabled() and bnact_enabled()) or _autocast_excludes():
        return 'switch'
    return None


def _bn_act_forward(ctx, frozen, x, norm, relu, eps, keep):
    """The forward of BnAct (norm = (gamma, beta)) and BnActEval (norm = (gamma, beta, running_mean, running_var)): x in either
    dense layout, the result channels_last.  Returns (out, stats -- None when frozen).  With `keep`, x, the parameters and the
    statistics are saved; the ReLU mask is recomputed from x in the backward, so `out` is not."""
    lib = L.load()
    xc = _aligned(x.contiguous(memory_format=torch.channels_last))
    norm = [t.contiguous() for t in norm]
    N, C, H, W = xc.shape
    d = _BnActDesc(N * H * W, C, int(bool(relu)), float(eps))
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
    if frozen:
        stats = None
        L._check(lib.ghn3_bn_act_frozen_fwd(ctypes.byref(d), *_ptrs(xc, *norm, out), _stream()), 'ghn3_bn_act_frozen_fwd')
    else:
        stats = torch.empty(3 * C, dtype=torch.float32, device=x.device)
        scratch = torch.empty(_scratch_floats(_BNACT_SCRATCH, d, 0), dtype=torch.float32, device=x.device)
        L._check(lib.ghn3_bn_act_fwd(ctypes.byref(d), *_ptrs(xc, *norm, out, stats, scratch), _stream()), 'ghn3_bn_act_fwd')
    if keep:
        ctx.save_for_backward(xc, *norm, *(() if frozen else (stats,)))
        ctx.desc = d
    return out, stats


def _bn_act_backward(ctx, frozen, dout):
    """(dx, dgamma, dbeta) of both members; the parameter gradients are tensors of their own (leaves' .grad)."""
    lib = L.load()
    d = ctx.desc
    xc, g, b, *st = ctx.saved_tensors
    do = _aligned(dout.contiguous(memory_format=torch.channels_last))
    dx = torch.empty_like(xc)
    dg, db = torch.empty_like(g), torch.empty_like(g)
    scratch = torch.empty(_scratch_floats(_BNACT_SCRATCH, d, 3 if frozen else 1), dtype=torch.float32, device=xc.device)
    if frozen:
        rm, rv = st
        L._check(lib.ghn3_bn_act_frozen_bwd(ctypes.byref(d), *_ptrs(do, xc, g, b, rm, rv, dx, dg, db, scratch), _stream()),
                 'ghn3_bn_act_frozen_bwd')
    else:
        stats, = st
        L._check(lib.ghn3_bn_act_bwd(ctypes.byref(d), *_ptrs(do, xc, stats, g, b, dx, dg, db, scratch), _stream()), 'ghn3_bn_act_bwd')
    return dx, dg, db


class BnAct(torch.autograd.Function):
    """BatchNorm (batch statistics) [-> ReLU] on its own as ONE autograd node on ghn3_bn_act_fwd / _bwd (2 launches each); returns
    (out, stats), stats [3 C] = mean, rstd, biased variance as ConvBn's, not differentiable."""

    @staticmethod
    def applicable(x, gamma, beta, training_stats=True):
        return bool(training_stats) and bn_act_refusal(x, gamma, beta) is None

    @staticmethod
    def forward(ctx, x, gamma, beta, relu, eps, keep):
        out, stats = _bn_act_forward(ctx, False, x, (gamma, beta), relu, eps, keep)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dout, _dstats):
        return _bn_act_backward(ctx, False, dout) + (None,) * 3


class BnActEval(torch.autograd.Function):
    """The same with RUNNING statistics (eval mode), read only: ghn3_bn_act_frozen_fwd / _bwd, the per-channel affine map [+ ReLU]."""

    @staticmethod
    def applicable(x, gamma, beta, running_mean, running_var):
        return bn_act_refusal(x, gamma, beta, True, running_mean, running_var) is None

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, relu, eps, keep):
        return _bn_act_forward(ctx, True, x, (gamma, beta, running_mean, running_var), relu, eps, keep)[0]

    @staticmethod
    def backward(ctx, dout):
        return _bn_act_backward(ctx, True, dout) + (None,) * 5


def bn_act(x, gamma, beta, relu=True, eps=1e-5):
    """out = relu(batch_norm(x)) (relu=False: batch_norm(x)) with batch statistics; returns (out, stats).  x: (N, C, H, W) fp32
    CUDA tensor in either dense layout; out is channels_last.  Under torch.no_grad(), or when no input requires a gradient,
    nothing is saved."""
    _needs_gpu('bn_act', x)
    return BnAct.apply(x, gamma, beta, bool(relu), float(eps), _wants_grad(x, gamma, beta))


def bn_act_eval(x, gamma, beta, running_mean, running_var, relu=True, eps=1e-5):
    """The same with the given running statistics (a BatchNorm in eval mode); returns out."""
    _needs_gpu('bn_act_eval', x)
    return BnActEval.apply(x, gamma, beta, running_mean, running_var, bool(relu), float(eps), _wants_grad(x, gamma, beta))


def bn_act_reference(x, gamma, beta, relu=True, eps=1e-5, running_mean=None, running_var=None):
    """The stock layers the two nodes replace, functional form -- the parity reference of the tests."""
    y = F.batch_norm(x, running_mean, running_var, gamma, beta, running_mean is None, 0.1, eps)
    return F.relu(y) if relu else y


class _PatchDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C_in', 'C_out', 'kh', 'kw', 'stride_h', 'stride_w', 'Ho', 'Wo', 'nhwc')]


PATCH_KERNEL = (8, 32)            # max(kh, kw) the patch-embedding op takes: what the dense-convolution op (<= 7) refuses
PATCH_MAX_IN = 4                  # image channels
PATCH_MAX_RED = 4096              # C_in kh kw
PATCH_MAX_OUT = 4096


def _patch_desc(x, w, stride, nhwc=0):
    N, C, H, W = x.shape
    C_out, _, kh, kw = w.shape
    sh, sw = _pair(stride)
    Ho, Wo = (H - kh) // sh + 1 if H >= kh else 0, (W - kw) // sw + 1 if W >= kw else 0
    return _PatchDesc(N, H, W, C, C_out, kh, kw, sh, sw, Ho, Wo, int(nhwc))


class PatchEmbed(torch.autograd.Function):
    """A bias-free convolution whose windows do not overlap (stride >= kernel, no padding, no dilation) with a kernel of 8 .. 32 a
    side, as ONE autograd node on ghn3_patch_fwd / _bwd (ghn3_amd/csrc/tnet_patch.hip): the patch embedding of the ImageNet-sized
    ViT-style networks, Conv2d(3, C, 16, stride=16).  x is read as stored (NCHW-contiguous or channels_last; three channels as
    three), the weight [C_out][C_in][kh][kw] in place; the result is channels_last, dx has x's layout and is computed only when x
    requires a gradient."""

    @staticmethod
    def applicable(x, w, stride, padding=0, dilation=1):
        """The limits of the C side (check_pdesc), so that a layer that passes never raises in the middle of a network."""
        if not (_native_input(x, 'GHN3_NATIVE_CONV') and _f32_cuda(w) and w.dim() == 4):
            return False
        if isinstance(padding, str) or _pair(padding) != (0, 0) or _pair(dilation) != (1, 1):
            return False
        (N, C_in, H, W), (C_out, w_in, kh, kw), (sh, sw) = x.shape, w.shape, _pair(stride)
        if not (PATCH_KERNEL[0] <= max(kh, kw) <= PATCH_KERNEL[1] and w_in == C_in and 1 <= C_in <= PATCH_MAX_IN and
                C_in * kh * kw <= PATCH_MAX_RED and C_out % 4 == 0 and 0 < C_out <= PATCH_MAX_OUT and sh >= kh and sw >= kw):
            return False
        d = _patch_desc(x, w, stride)
        return N > 0 and d.Ho > 0 and d.Wo > 0 and x.numel() < 2 ** 31 and N * d.Ho * d.Wo * C_out < 2 ** 31

    @staticmethod
    def forward(ctx, x, w, stride, keep):
        lib = L.load()
        nhwc = not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
        xc = x if (nhwc or x.is_contiguous()) else x.contiguous()
        wc = w.contiguous()
        d = _patch_desc(xc, wc, stride, nhwc)
        z = torch.empty((d.N, d.C_out, d.Ho, d.Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        L._check(lib.ghn3_patch_fwd(ctypes.byref(d), _ptr(xc), _ptr(wc), _ptr(z), None, _stream()), 'ghn3_patch_fwd')
        if keep:
            ctx.save_for_backward(xc, wc)
            ctx.cfg = (stride, nhwc)
        return z

    @staticmethod
    def backward(ctx, dz):
        lib = L.load()
        xc, wc = ctx.saved_tensors
        stride, nhwc = ctx.cfg
        d = _patch_desc(xc, wc, stride, nhwc)
        do = dz.contiguous(memory_format=torch.channels_last)
        if do.data_ptr() % 16:                                 # (a view into a larger gradient: the kernels read whole quads)
            do = do.clone(memory_format=torch.channels_last)
        dx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(wc) if ctx.needs_input_grad[1] else None      # (a tensor of its own: it becomes a leaf's .grad)
        n = _scratch_floats('ghn3_patch_scratch_floats', d, 1)
        scratch = torch.empty(n, dtype=torch.float32, device=xc.device) if (n and dw is not None) else None
        L._check(lib.ghn3_patch_bwd(ctypes.byref(d), _ptr(do), _ptr(xc), _ptr(wc), _ptr(dx), _ptr(dw), _ptr(scratch), _stream()),
                 'ghn3_patch_bwd')
        return dx, dw, None, None


def patch_embed(x, w, stride):
    """conv2d(x, w, stride=stride) for non-overlapping windows (see PatchEmbed); x (N, C_in <= 4, H, W) fp32 CUDA tensor, w (C_out,
    C_in, kh, kw); the result is a channels_last tensor.  Under torch.no_grad(), or when neither input requires a gradient, nothing
    is saved."""
    _needs_gpu('patch_embed', x)
    return PatchEmbed.apply(x, w, _pair(stride), _wants_grad(x, w))


class SqueezeExcite(torch.autograd.Function):
    """y = x * hardswish(W2 relu(W1 mean_hw(x) + b1) + b2) as ONE autograd node on ghn3_se_fwd / _bwd (round 6:
    `ChannelSELayer`, ops.py:239-274).  NHWC storage inside; the Linear layers' weights and biases are read in place."""

    @staticmethod
    def applicable(x, w1, b1, w2, b2):
        if not (_native_input(x, 'GHN3_NATIVE_SE') and _f32_cuda(w1, b1, w2, b2)):
            return False
        C, J = x.shape[1], w1.shape[0]
        if not (C % 4 == 0 and C <= SE_MAX and J <= SE_MAX and tuple(w1.shape) == (J, C) and tuple(w2.shape) == (C, J) and
                b1.numel() == J and b2.numel() == C and x.numel() < 2 ** 31):
            return False
        return max(C, J) <= SE_NARROW or _wide()

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        lib = L.load()
        xc = x.contiguous(memory_format=torch.channels_last)
        w1c, b1c, w2c, b2c = w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous()
        N, C, H, W = xc.shape
        J = int(w1c.shape[0])
        y = torch.empty_like(xc)
        save = torch.empty(N * (2 * C + J), dtype=torch.float32, device=x.device)
        L._check(lib.ghn3_se_fwd(N, H * W, C, J, _ptr(xc), _ptr(w1c), _ptr(b1c), _ptr(w2c), _ptr(b2c), _ptr(y), _ptr(save), _stream()),
                 'ghn3_se_fwd')
        ctx.save_for_backward(xc, w1c, w2c, save)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        xc, w1c, w2c, save = ctx.saved_tensors
        N, C, H, W = xc.shape
        J = int(w1c.shape[0])
        do = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty_like(xc)
        (dw1, dw2, db1, db2), scratch = _carve(xc, N * (C + J), (J, C), (C, J), (J,), (C,))
        L._check(lib.ghn3_se_bwd(N, H * W, C, J, _ptr(do), _ptr(xc), _ptr(w1c), _ptr(w2c), _ptr(save), _ptr(dx), _ptr(dw1), _ptr(db1),
                                 _ptr(dw2), _ptr(db2), _ptr(scratch), _stream()), 'ghn3_se_bwd')
        return dx, dw1, db1, dw2, db2


def se_layer(x, w1, b1, w2, b2):
    """Squeeze-and-excitation with a hard-swish gate on the fused op: x (N, C, H, W) fp32 CUDA; w1 (J, C), b1 (J), w2 (C, J), b2 (C)."""
    _needs_gpu('se_layer', x)
    return SqueezeExcite.apply(x, w1, b1, w2, b2)


def run_se_layer(fc1, fc2, x, keep_layout=False):
    """`ChannelSELayer` body (before its stride slicing) on the fused op where it applies; None otherwise (the caller keeps its
    stock layers)."""
    w1, b1, w2, b2 = (getattr(fc1, 'weight', None), getattr(fc1, 'bias', None), getattr(fc2, 'weight', None),
                      getattr(fc2, 'bias', None))
    if not SqueezeExcite.applicable(x, w1, b1, w2, b2):
        return None
    y = se_layer(x, w1, b1, w2, b2)
    return _hand_on(y, keep_layout, fc1, fc2)


class _PoolDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C', 'k', 'stride', 'pad', 'Ho', 'Wo', 'mode')]


class Pool2d(torch.autograd.Function):
    """k x k max (mode 1) / average over the valid taps (mode 0) pooling on NHWC storage: ghn3_pool_fwd / _bwd (round 6; the
    `max_pool_3x3` / `avg_pool_3x3` ops and the stems' MaxPool2d, ops.py:289-291,452)."""

    @staticmethod
    def applicable(x, k, stride, pad):
        return _native_input(x, 'GHN3_NATIVE_POOL') and x.shape[1] % 4 == 0 and \
            isinstance(k, int) and isinstance(stride, int) and isinstance(pad, int) and 0 < k <= 15 and 2 * pad <= k and \
            stride > 0 and x.shape[2] + 2 * pad >= k and x.shape[3] + 2 * pad >= k and x.numel() < 2 ** 31

    @staticmethod
    def forward(ctx, x, k, stride, pad, mode):
        lib = L.load()
        xc = x.contiguous(memory_format=torch.channels_last)
        N, C, H, W = xc.shape
        d = _PoolDesc(N, H, W, C, k, stride, pad, (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1, mode)
        y = torch.empty((N, C, d.Ho, d.Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        idx = torch.empty(y.numel(), dtype=torch.uint8, device=x.device) if mode else None
        L._check(lib.ghn3_pool_fwd(ctypes.byref(d), _ptr(xc), _ptr(y), _ptr(idx), _stream()), 'ghn3_pool_fwd')
        ctx.desc, ctx.idx = d, idx
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = L.load()
        d = ctx.desc
        do = dy.contiguous(memory_format=torch.channels_last)
        dx = torch.empty((d.N, d.C, d.H, d.W), dtype=torch.float32, device=dy.device, memory_format=torch.channels_last)
        L._check(lib.ghn3_pool_bwd(ctypes.byref(d), _ptr(do), _ptr(ctx.idx), _ptr(dx), _stream()), 'ghn3_pool_bwd')
        return dx, None, None, None, None


def _as_int(v):
    """An int for a square kernel / stride / padding given as int or equal pair, else None."""
    if isinstance(v, (tuple, list)):
        return int(v[0]) if len(v) == 2 and v[0] == v[1] else None
    return int(v) if isinstance(v, int) else None


def run_pool(x, kernel_size, stride, padding, mode):
    """max (mode 1) / average (mode 0, valid taps only) pooling on the fused op where it applies; None otherwise."""
    k, s, p = _as_int(kernel_size), _as_int(stride), _as_int(padding)
    if k is None or s is None or p is None or not Pool2d.applicable(x, k, s, p):
        return None
    return Pool2d.apply(x, k, s, p, mode)


# ---- the runners: a block's layers -> the member of a family that fits its norm slot, or the stock layers --------------------
_Slot = collections.namedtuple('_Slot', 'kind gamma beta mean var eps bn update')
_BARE = _Slot('none', None, None, None, None, 0.0, None, False)       # (no norm layer: an Identity, or no norm slot at all)
_STOCK = _Slot('stock', None, None, None, None, 0.0, None, False)


def _norm_slot(bn):
    """What a block's norm slot asks of the op families in this call, decided once: kind 'none' (an Identity, `_no_norm`: the
    members without a norm layer), 'batch' (batch statistics: DwPwBn / ConvBn; `update`: the layer's running statistics follow,
    as torch's would), 'frozen' (running statistics outside training, `_frozen_norm`: DwPwBnEval / ConvBnEval) or 'stock' (leave
    the block to the stock layers: a layer without `eps`, or one of the two switches says so), with the tensors the members
    read."""
    if _no_norm(bn):
        return _BARE
    gamma, beta, has_run, batch_stats = _norm_inputs(bn)
    if not hasattr(bn, 'eps'):
        return _STOCK
    if batch_stats:
        return _Slot('batch', gamma, beta, None, None, bn.eps, bn,
                     has_run and getattr(bn, 'training', True) and getattr(bn, 'track_running_stats', False))
    if _frozen_norm(batch_stats):
        return _Slot('frozen', gamma, beta, bn.running_mean, bn.running_var, bn.eps, bn, False)
    return _STOCK


def _update_running_stats(slot, stats, out):
    if slot.update:
        bn = slot.bn
        with torch.no_grad():
            C = bn.weight.numel()
            n = out.numel() // C
            # torch.nn.modules.batchnorm._BatchNorm.forward: the counter moves first; momentum=None = cumulative average
            nbt = getattr(bn, 'num_batches_tracked', None)
            if nbt is not None:
                nbt += 1
            if bn.momentum is not None:
                mom = float(bn.momentum)
            else:
                mom = 1.0 / float(nbt) if nbt is not None else 0.1
            bn.running_mean.mul_(1 - mom).add_(stats[:C], alpha=mom)
            bn.running_var.mul_(1 - mom).add_(stats[2 * C:] * (n / max(n - 1, 1)), alpha=mom)


def _conv_dispatch(x, w, slot, stride, pad, dil, relu, first=None):
    """[ReLU ->] convolution -> the norm slot on the member of the dense-convolution family the slot names, where that member
    applies -- its NHWC output; the running statistics of a batch member are updated --, else None (the caller keeps the stock
    layers).  `first`: x only stands for the input (its shape, type and device); the real one is first() -- a block's first node,
    a layer that has to run before --, called once the member is known to apply."""
    g, b = slot.gamma, slot.beta
    if slot.kind == 'none':
        if ConvOnly.applicable(x, w):
            return conv_only(first() if first else x, w, stride, pad, dil, relu)
    elif slot.kind == 'frozen':
        # (running statistics in eval mode: the statistics are not touched)
        if ConvBnEval.applicable(x, w, g, b, slot.mean, slot.var, stride, pad, dil):
            return conv_bn_eval(first() if first else x, w, g, b, slot.mean, slot.var, stride, pad, dil, relu, slot.eps)
    elif slot.kind == 'batch':
        if ConvBn.applicable(x, w, g, b):
            out, stats = conv_bn(first() if first else x, w, g, b, stride, pad, dil, relu, slot.eps)
            _update_running_stats(slot, stats, out)
            return out
    return None


def _dwpw_dispatch(x, w_dw, w_pw, slot, stride, pad, dil):
    """ReLU -> depthwise (w_dw None: none) -> pointwise -> the norm slot on the member of the fused depthwise + pointwise family
    the slot names; as _conv_dispatch."""
    ks = w_dw.shape[-1] if torch.is_tensor(w_dw) else 1
    g, b = slot.gamma, slot.beta
    if slot.kind == 'none':
        if DwPw.applicable(x, w_dw, w_pw, ks):
            return dwpw(x, w_dw, w_pw, stride, pad, dil)
    elif slot.kind == 'frozen':
        if DwPwBnEval.applicable(x, w_dw, w_pw, g, b, slot.mean, slot.var, ks):
            return dwpw_bn_eval(x, w_dw, w_pw, g, b, slot.mean, slot.var, stride, pad, dil, slot.eps)
    elif slot.kind == 'batch':
        if DwPwBn.applicable(x, w_dw, w_pw, g, b, ks):
            out, stats = dwpw_bn(x, w_dw, w_pw, g, b, stride, pad, dil, slot.eps)
            _update_running_stats(slot, stats, out)
            return out
    return None


def _stand_in(x, N, C, H, W):
    """The input of a block's second node before the first one has run, for `applicable`: x's type and device, the
    intermediate's true shape, one element (no storage of that size)."""
    return x.new_empty(1).expand(N, C, H, W)


def _stock(layers, x):
    for m in layers:
        x = m(x)
    return x


def _plain_conv(conv, biased=False):
    """An ungrouped convolution with numeric padding and one dilation for both axes (what the dense kernels take): bias-free, or
    -- biased=True -- with a bias tensor."""
    bias = getattr(conv, 'bias', None)
    return hasattr(conv, 'kernel_size') and (torch.is_tensor(bias) if biased else bias is None) and \
        not isinstance(conv.padding, str) and getattr(conv, 'groups', 1) == 1 and \
        torch.is_tensor(getattr(conv, 'weight', None)) and len(set(_pair(getattr(conv, 'dilation', 1)))) == 1


def _image_pad(x, w):
    """A 3-channel image (the first convolution of every network) is given a zero fourth channel -- and the weight a zero fourth
    input slice, through autograd -- because the kernels read channels in groups of four."""
    if x.shape[1] == 3 and w.shape[1] == 3:
        return F.pad(x, (0, 0, 0, 0, 0, 1)), F.pad(w, (0, 0, 0, 0, 0, 1))
    return x, w


def run_conv_block(layers, x, keep_layout=False):
    """[ReLU, k x k Conv2d, BatchNorm2d] -- `ReLUConvBN` (ops.py:180-198) -- on the fused dense-convolution op where it applies,
    else layer by layer.  Same layout contract as run_block.  An Identity in the norm slot (norm=None): ConvOnly with the ReLU."""
    relu, conv, bn = layers
    out = None
    if _plain_conv(conv):
        out = _conv_dispatch(x, conv.weight, _norm_slot(bn), conv.stride, conv.padding, _pair(conv.dilation)[0], True)
    return _stock(layers, x) if out is None else _hand_on(out, keep_layout, conv, bn)


def run_conv_pair_block(layers, x, keep_layout=False):
    """[ReLU, 1 x k Conv2d, k x 1 Conv2d, BatchNorm2d] -- `ReLUConvBN(double=True)`, the `conv_1x7_7x1` op (ops.py:186-190,
    298) -- as two dense-convolution nodes: ReLU + the first convolution alone (ConvOnly), then the second one with the norm
    slot's member, without a ReLU; the intermediate stays NHWC.  Else layer by layer."""
    relu, conv_a, conv_b, bn = layers
    out = None
    if _plain_conv(conv_a) and _plain_conv(conv_b) and ConvOnly.applicable(x, conv_a.weight) and \
            conv_b.weight.shape[1] == conv_a.weight.shape[0]:
        a = (conv_a.weight, conv_a.stride, conv_a.padding, _pair(conv_a.dilation)[0], True)
        da = _conv_desc(x, *a, 0.0)
        if conv_desc_fits(da):
            # (the second node's input has conv_a's channel count, x's type and the first convolution's output size)
            out = _conv_dispatch(_stand_in(x, da.N, da.C_out, da.Ho, da.Wo), conv_b.weight, _norm_slot(bn), conv_b.stride,
                                 conv_b.padding, _pair(conv_b.dilation)[0], False, first=lambda: conv_only(x, *a))
    return _stock(layers, x) if out is None else _hand_on(out, keep_layout, conv_a, conv_b, bn)


def run_conv_layer(conv, x):
    """A bare Conv2d without bias (the patch embedding of the ViT-style networks, ops.py:296 `conv_stride`), handing an NCHW
    tensor on: up to 7 x 7 (CIFAR-sized inputs: 3 x 3, stride 3) on the dense-convolution op -- 3-channel images padded as in
    run_layer_seq --, a larger kernel with non-overlapping windows (ImageNet-sized inputs: 16 x 16, stride 16) on the patch-embedding
    op, which reads the image as it is; else the stock layer.  GHN3_NATIVE_STEM=0 keeps the stock layer, as for the other stems."""
    if _plain_conv(conv) and torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and os.environ.get('GHN3_NATIVE_STEM', '1') != '0':
        w, y = conv.weight, None
        if w.dim() == 4 and max(w.shape[2], w.shape[3]) > 7:              # (what ConvOnly refuses for its kernel size)
            if PatchEmbed.applicable(x, w, conv.stride, conv.padding, conv.dilation):
                y = patch_embed(x, w, conv.stride)
        else:
            y = _conv_dispatch(*_image_pad(x, w), _BARE, conv.stride, conv.padding, _pair(conv.dilation)[0], False)
        if y is not None:
            return y.contiguous(memory_format=torch.contiguous_format)
    return conv(x)


def run_layer_seq(seq, x):
    """A stem (`nn.Sequential` of Conv2d / BatchNorm2d / ReLU / MaxPool2d / Identity, ops.py:443-463) with every
    [Conv2d, norm] and [ReLU, Conv2d, norm] window -- norm a BatchNorm2d, or the Identity of a norm=None stem -- on the
    dense-convolution member that fits the norm slot and the rest layer by layer; 3-channel images as `_image_pad` says."""
    layers = list(seq)
    k, n = 0, len(layers)
    while k < n:
        m = layers[k]
        relu = _is_kind(m, 'ReLU') and k + 2 < n
        conv = layers[k + 1] if relu else m
        bn = layers[k + 2] if relu else (layers[k + 1] if k + 1 < n else None)
        out = None
        if _is_kind(conv, 'Conv2d') and bn is not None and _plain_conv(conv) and torch.is_tensor(x) and x.is_cuda and x.dim() == 4:
            slot = _norm_slot(bn)
            if slot.kind == 'none' or _is_kind(bn, 'BatchNorm2d'):
                xin, w = _image_pad(x, conv.weight)
                # an in-place ReLU at the head of the sequence rewrites the CALLER's tensor (stem1 of the two-stem networks:
                # the cells read relu(stem0's output) afterwards, ops.py:449,545-546): kept as the layer it is
                head = relu and k == 0 and getattr(m, 'inplace', False)
                out = _conv_dispatch(xin, w, slot, conv.stride, conv.padding, _pair(conv.dilation)[0], relu and not head,
                                     first=(lambda: m(xin)) if head else None)
        if out is None:
            x = m(x)
            k += 1
        else:
            x = _hand_on(out, False, conv, bn)
            k += 3 if relu else 2
    return x


def zero_padded_conv(conv, biased=False):
    """`_plain_conv` and zero padding: what a convolution of a torch.nn network has to be for the dense kernels (the layers of
    ghn3_amd.ops never pad otherwise; an arbitrary nn.Conv2d may reflect, replicate or wrap)."""
    return _plain_conv(conv, biased) and getattr(conv, 'padding_mode', 'zeros') == 'zeros'


def run_conv_window(conv, bn, x, relu, residual=None):
    """Conv2d [-> BatchNorm2d] [-> + residual] [-> ReLU] of a torch.nn network (`bn` None: no norm layer) on the member of the
    dense-convolution family the window names; the NHWC result, or None where no member applies and the caller keeps its stock
    layers:

        bn           conv.bias  relu    member
        BatchNorm2d  none       yes     ConvBnAct / ConvBnActEval, chosen by `_norm_slot`; residual allowed; GHN3_NATIVE_ACT=0: None
        BatchNorm2d  none       no      ConvBn / ConvBnEval through `_conv_dispatch`; no residual; GHN3_NATIVE_ACT is not asked
        None         tensor     either  ConvBiasAct; residual allowed; GHN3_NATIVE_BIAS=0: None
        None         none       no      ConvOnly through `_conv_dispatch(_BARE)`; no residual
        anything else                   None: a bias together with a norm layer, a bare convolution with a ReLU or a residual,
                                        a norm layer without a ReLU but with a residual, a norm layer that is no BatchNorm2d

    Every row: None for CPU tensors, another dtype, GHN3_NATIVE_OPS=0, GHN3_NATIVE_CONV=0, autocast with GHN3_NATIVE_AMP=0, a
    grouped or oddly padded convolution (`zero_padded_conv`) and a limit of the kernels (the member's `applicable`; the two rows
    of `_conv_dispatch`, whose members leave the 2^31 rules to the C side, ask `_conv_geometry_fits` first); 3-channel images as
    `_image_pad` says; the running statistics of a batch-statistics member follow as torch's would (`_update_running_stats`)."""
    biased = getattr(conv, 'bias', None) is not None
    if not (_native_input(x, 'GHN3_NATIVE_CONV') and zero_padded_conv(conv, biased)):
        return None
    if bn is None:
        if not (bias_enabled() if biased else not relu and residual is None):
            return None
        slot = _BARE
    else:
        if biased or not _is_kind(bn, 'BatchNorm2d') or not (act_enabled() if relu else residual is None):
            return None
        slot = _norm_slot(bn)
    xin, w = _image_pad(x, conv.weight)
    args = (residual, conv.stride, conv.padding, _pair(conv.dilation)[0])
    if biased:
        if ConvBiasAct.applicable(xin, w, conv.bias, *args):
            return conv_bias_act(xin, w, conv.bias, *args, relu, False)
    elif not relu:
        if _conv_geometry_fits(xin, w, *args):
            return _conv_dispatch(xin, w, slot, *args[1:], False)
    elif slot.kind == 'frozen':
        if ConvBnActEval.applicable(xin, w, slot.gamma, slot.beta, slot.mean, slot.var, *args):
            return conv_bn_act_eval(xin, w, slot.gamma, slot.beta, slot.mean, slot.var, *args, False, slot.eps)
    elif slot.kind == 'batch':
        if ConvBnAct.applicable(xin, w, slot.gamma, slot.beta, *args):
            out, stats = conv_bn_act(xin, w, slot.gamma, slot.beta, *args, False, slot.eps)
            _update_running_stats(slot, stats, out)
            return out
    return None


def run_conv_bn_act(conv, bn, x, residual=None):
    """Conv2d -> BatchNorm2d [-> + residual] -> ReLU: the first row of `run_conv_window`."""
    return None if bn is None else run_conv_window(conv, bn, x, True, residual)


def run_conv_bias_act(conv, x, relu, residual=None):
    """Conv2d WITH a bias [-> + residual] [-> ReLU]: the third row of `run_conv_window`; None for an unbiased convolution."""
    return None if getattr(conv, 'bias', None) is None else run_conv_window(conv, None, x, relu, residual)


def run_bn_act(bn, x, relu):
    """BatchNorm2d [-> ReLU] of a torch.nn network, with no convolution in front of it, on the stand-alone member that fits the
    norm slot (`_norm_slot`: BnAct with batch statistics, whose running statistics follow as torch's would; BnActEval in eval
    mode); the NHWC result, or None where the node does not apply -- CPU tensors, another dtype, GHN3_NATIVE_OPS=0,
    GHN3_NATIVE_BNACT=0, autocast with GHN3_NATIVE_AMP=0, a limit of the kernels, a slot of kind 'none' / 'stock' -- and the
    caller keeps its stock layers."""
    if not (bnact_enabled() and _native_input(x) and _is_kind(bn, 'BatchNorm2d')):
        return None
    slot = _norm_slot(bn)
    g, b = slot.gamma, slot.beta
    if slot.kind == 'batch':
        if BnAct.applicable(x, g, b):
            out, stats = bn_act(x, g, b, relu, slot.eps)
            _update_running_stats(slot, stats, out)
            return out
    elif slot.kind == 'frozen':
        if BnActEval.applicable(x, g, b, slot.mean, slot.var):
            return bn_act_eval(x, g, b, slot.mean, slot.var, relu, slot.eps)
    return None


def run_factorized_reduce(relu, conv_1, conv_2, bn, x, stride=2, keep_layout=False):
    """`FactorizedReduce` (ops.py:163-178: ReLU, two 1 x 1 convolutions of stride 2 on the even and the odd pixel grid, concat,
    norm) as ONE dense-convolution node: a 2 x 2 kernel of stride 2 whose tap (0, 0) carries conv_1's weights for the first half
    of the output channels and whose tap (1, 1) carries conv_2's for the second half (the other entries are zeros) reads exactly
    the pixels the two strided convolutions read.  The 2 x 2 weight is assembled by differentiable torch ops, so the gradients
    reach conv_1 / conv_2 (views of the GHN's prediction buffer) through autograd.  Returns None when the fused op does not
    apply (the caller keeps the stock layers)."""
    w1, w2 = getattr(conv_1, 'weight', None), getattr(conv_2, 'weight', None)
    slot = _norm_slot(bn)
    if not (stride == 2 and slot.kind != 'stock' and torch.is_tensor(w1) and torch.is_tensor(w2) and
            x.dim() == 4 and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and getattr(conv_1, 'bias', None) is None and
            getattr(conv_2, 'bias', None) is None and w1.shape == w2.shape and tuple(w1.shape[2:]) == (1, 1)):
        return None
    half, C_in = int(w1.shape[0]), int(w1.shape[1])
    w = torch.zeros(2 * half, C_in, 2, 2, dtype=w1.dtype, device=w1.device)
    w[:half, :, 0, 0] = w1[:, :, 0, 0]
    w[half:, :, 1, 1] = w2[:, :, 0, 0]
    out = _conv_dispatch(x, w, slot, 2, 0, 1, True)
    return None if out is None else _hand_on(out, keep_layout, conv_1, conv_2, bn)


def run_pointwise_block(layers, x, keep_layout=False):
    """[ReLU, 1 x 1 Conv2d, BatchNorm2d] -- `ReLUConvBN` with a 1 x 1 kernel (ops.py:180-198: the preprocessing layer of every
    cell, the `conv_1x1` op) -- on the fused op without a depthwise stage where it applies, else as run_conv_block."""
    relu, pw, bn = layers
    w_pw = getattr(pw, 'weight', None)
    out = None
    if getattr(pw, 'bias', None) is None and hasattr(pw, 'kernel_size') and \
            tuple(pw.kernel_size) == (1, 1) and pw.stride[0] == pw.stride[1] and not isinstance(pw.padding, str) and \
            tuple(pw.padding) == (0, 0) and getattr(pw, 'groups', 1) == 1 and torch.is_tensor(w_pw):
        out = _dwpw_dispatch(x, None, w_pw, _norm_slot(bn), pw.stride[0], 0, 1)
    if out is None:
        # (more than 512 channels on either side -- the concatenated states of a cell, the layers of a wide network: the
        # dense-convolution op takes those)
        return run_conv_block(layers, x, keep_layout)
    return _hand_on(out, keep_layout, pw, bn)


def _wide_block(dw, pw, slot, x):
    """[ReLU, depthwise Conv2d, pointwise Conv2d, norm] wider than the fused depthwise + pointwise kernels take, as two nodes:
    Depthwise, then the 1 x 1 member of the dense-convolution family that fits the norm slot, without a ReLU; the intermediate
    stays NHWC.  None when one of the two does not apply (the caller keeps the stock layers).  The caller has checked the
    layers' attributes (`layers_ok` of run_block)."""
    w_dw, w_pw = getattr(dw, 'weight', None), getattr(pw, 'weight', None)
    if not (torch.is_tensor(x) and x.dim() == 4 and torch.is_tensor(w_pw) and w_pw.dim() == 4 and _plain_conv(pw) and
            max(x.shape[1], w_pw.shape[0]) > DWPW_MAX and _wide()):
        return None
    stride, pad, dil = int(dw.stride[0]), int(dw.padding[0]), int(dw.dilation[0])
    if not Depthwise.applicable(x, w_dw, stride, pad, dil):
        return None
    d = _desc(x, x.shape[1], w_dw.shape[-1], stride, pad, dil, 0.0)
    mid = _stand_in(x, d.N, d.C_in, d.Ho, d.Wo)
    if slot.kind == 'batch' and not conv_desc_fits(_conv_desc(mid, w_pw, 1, 0, 1, False, 0.0)):
        return None                                # (ConvBnEval.applicable asks this itself, ConvBn.applicable does not)
    return _conv_dispatch(mid, w_pw, slot, 1, 0, 1, False, first=lambda: depthwise_relu(x, w_dw, stride, pad, dil))


def run_block(layers, x, keep_layout=False):
    """[ReLU, depthwise Conv2d, pointwise Conv2d, BatchNorm2d] (light or torch.nn flavour) on the fused op when it applies,
    else layer by layer.  Running statistics of a tracking BatchNorm are updated as torch does (momentum, unbiased variance).

    The fused op works on NHWC storage.  Its output is handed to the neighbouring (stock ATen / MIOpen) layers as a plain
    NCHW-contiguous tensor unless keep_layout is set (the next layer is another fused block): on this ROCm build the stock
    layers compute wrong parameter gradients for channels_last activations (tools/diag/target_ops_diag.py,
    profiles/r05c_target_ops_channels_last_diag.txt), so the layout must not leak into them -- one transposing copy per
    direction at the op's boundary until the neighbouring layers are native as well."""
    relu, dw, pw, bn = layers
    layers_ok = getattr(dw, 'bias', None) is None and getattr(pw, 'bias', None) is None and \
        hasattr(dw, 'kernel_size') and dw.kernel_size[0] == dw.kernel_size[1] and dw.stride[0] == dw.stride[1] and \
        not isinstance(dw.padding, str) and dw.padding[0] == dw.padding[1] and dw.dilation[0] == dw.dilation[1] and \
        getattr(dw, 'groups', 1) == x.shape[1] and tuple(pw.kernel_size) == (1, 1) and \
        tuple(getattr(pw, 'stride', (1, 1))) == (1, 1) and not isinstance(getattr(pw, 'padding', 0), str) and \
        tuple(getattr(pw, 'padding', (0, 0))) == (0, 0) and getattr(pw, 'groups', 1) == 1 and \
        tuple(getattr(pw, 'dilation', (1, 1))) == (1, 1)
    out = None
    if layers_ok:
        slot = _norm_slot(bn)
        out = _dwpw_dispatch(x, getattr(dw, 'weight', None), getattr(pw, 'weight', None), slot, dw.stride[0], dw.padding[0],
                             dw.dilation[0])
        if out is None:
            out = _wide_block(dw, pw, slot, x)                 # (wider than the fused kernels: two nodes)
    return _stock(layers, x) if out is None else _hand_on(out, keep_layout, dw, pw, bn)


class _MsaDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('B', 'H', 'W', 'C', 'heads', 'hidden', 'stride', 'Ho', 'Wo', 'layout')] + \
        [('eps', ctypes.c_float), ('has_qkv_bias', ctypes.c_int32)]


MSA_PARAM_NAMES = ('ln1_w', 'ln1_b', 'w_qkv', 'b_qkv', 'w_o', 'b_o', 'ln2_w', 'ln2_b', 'w1', 'b1', 'w2', 'b2')


class _MsaPtrs(ctypes.Structure):
    """ghn3_msa_params and ghn3_msa_grads (include/ghn3_hip.h): twelve pointers in MSA_PARAM_NAMES order."""
    _fields_ = [(n, ctypes.c_void_p) for n in MSA_PARAM_NAMES]


def _msa_ptrs(tensors):
    return _MsaPtrs(*[None if t is None else t.data_ptr() for t in tensors])


def _aligned(t):
    """t itself when its storage starts on 16 bytes (the kernels read it as float4), else a copy in the same memory format (a
    weight view of the GHN's flat buffer may start anywhere)."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _no_dropout(m):
    if _is_kind(m, 'Identity'):
        return True
    return _is_kind(m, 'Dropout') and (float(getattr(m, 'p', 1.0)) == 0.0 or not getattr(m, 'training', True))


def _msa_modules(layer):
    """(ln1, to_qkv, to_out linear, ln2, ff1, ff2, the four dropout slots, activation) of a `_TransformerLayer`, or None when the
    layer is not built the way the `msa` op builds it."""
    attn, ff = getattr(layer, 'attn', None), getattr(layer, 'ff', None)
    try:
        to_out, net = list(attn.to_out), list(ff.net)
    except (AttributeError, TypeError):
        return None
    if len(to_out) != 2 or len(net) != 5:
        return None
    return (layer.ln1, attn.to_qkv, to_out[0], layer.ln2, net[0], net[3], (attn.attn_drop, to_out[1], net[2], net[4]), net[1])


# ---- attention without a saved P ("lean": ghn3_attn_lean_* / ghn3_msa_lean_*, ghn3_amd/csrc/tnet_attn.hip) -----------------------
# The saved-P path keeps the attention probabilities, B heads N^2 floats per layer, for its backward and refuses 2^31 elements or
# more; the lean path keeps one float per query row and recomputes P, so it reaches those shapes.  MSA_LEAN_THRESHOLD is the
# element count of P from which `auto` takes the lean path.  It is 2^31: the default adds only the shapes the saved-P path
# refuses.  The measurement (profiles/r09a_tnet_msa_lean.txt) has the lean path level below 2^24 elements and faster from 3.4e7
# on (0.87 of the saved-P time there, 0.62 - 0.76 at 5e8 - 6e8), so its rule would allow 2^24 -- never less: the shapes of the
# layer tests, at most 64 * 8 * 121^2 = 7.5e6, stay on the saved-P path under the default setting --, but the whole GPU suite has
# not been run with a lower value yet, and until it has the default moves no existing shape to another kernel.
MSA_LEAN_THRESHOLD = 2 ** 31


def msa_lean(B, heads, N):
    """Whether an msa layer of B sequences of N tokens runs on the lean attention.  GHN3_MSA_LEAN=0: never (the saved-P path
    with its refusal at 2^31 elements of P); 1: wherever the lean limits allow; auto (default): iff B heads N^2 >=
    MSA_LEAN_THRESHOLD.  The rule reads the shape and the environment only -- never the grad mode: a no_grad forward and a
    training forward of one layer take the same attention kernel and agree bit for bit."""
    mode = os.environ.get('GHN3_MSA_LEAN', 'auto')
    if mode == '0':
        return False
    if mode == '1':
        return True
    return B * heads * N * N >= MSA_LEAN_THRESHOLD


class LeanAttention(torch.autograd.Function):
    """Plain multi-head self-attention softmax(q k^T / sqrt(d)) v on qkv (B, N, 3 C) -- columns q | k | v, head h at columns
    h d .. h d + d - 1 of each -- returning (B, N, C), on ghn3_attn_lean_fwd / _bwd: the backward recomputes the probabilities
    from qkv and one saved float per query row.  fp32 CUDA tensors, C % 4 == 0, d = C / heads <= 32, N <= 4096."""

    @staticmethod
    def forward(ctx, qkv, heads):
        if not (_f32_cuda(qkv) and qkv.dim() == 3 and qkv.shape[2] % 3 == 0):
            raise L.Ghn3Error('lean_attention takes a float32 CUDA tensor (B, N, 3 C); there is no other implementation')
        lib = L.load()
        q = _aligned(qkv.contiguous())
        B, N, C = q.shape[0], q.shape[1], q.shape[2] // 3
        out = torch.empty((B, N, C), dtype=torch.float32, device=q.device)
        lse = torch.empty((B, heads, N), dtype=torch.float32, device=q.device) if ctx.needs_input_grad[0] else None
        L._check(lib.ghn3_attn_lean_fwd(_ptr(out), _ptr(lse), _ptr(q), B, N, C, heads, _stream()),
                 'ghn3_attn_lean_fwd')
        if lse is not None:
            ctx.save_for_backward(q, lse, out)
            ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, lse, out = ctx.saved_tensors
        B, N, C = out.shape
        do = _aligned(dout.contiguous())
        dqkv = torch.empty_like(q)
        L._check(L.load().ghn3_attn_lean_bwd(_ptr(dqkv), _ptr(do), _ptr(q), _ptr(lse), _ptr(out), B, N, C, ctx.heads, _stream()),
                 'ghn3_attn_lean_bwd')
        return dqkv, None


def lean_attention(qkv, heads):
    """LeanAttention as a function: qkv (B, N, 3 C) -> (B, N, C)."""
    return LeanAttention.apply(qkv, int(heads))


class WideAttention(torch.autograd.Function):
    """`LeanAttention` for head dims up to 64, on ghn3_attn_wide_fwd / _bwd (ghn3_amd/csrc/tnet_msa_wide.hip): the same qkv
    (B, N, 3 C) -> (B, N, C), one saved float per query row, the probabilities recomputed in the backward.  d <= 32 runs the
    kernels of `LeanAttention` (bit-equal results).  fp32 CUDA tensors, C % 4 == 0, d = C / heads <= 64, N <= 4096."""

    @staticmethod
    def forward(ctx, qkv, heads):
        if not (_f32_cuda(qkv) and qkv.dim() == 3 and qkv.shape[2] % 3 == 0):
            raise L.Ghn3Error('wide_attention takes a float32 CUDA tensor (B, N, 3 C); there is no other implementation')
        lib = L.load()
        q = _aligned(qkv.contiguous())
        B, N, C = q.shape[0], q.shape[1], q.shape[2] // 3
        out = torch.empty((B, N, C), dtype=torch.float32, device=q.device)
        lse = torch.empty((B, heads, N), dtype=torch.float32, device=q.device) if ctx.needs_input_grad[0] else None
        L._check(lib.ghn3_attn_wide_fwd(_ptr(out), _ptr(lse), _ptr(q), B, N, C, heads, _stream()),
                 'ghn3_attn_wide_fwd')
        if lse is not None:
            ctx.save_for_backward(q, lse, out)
            ctx.heads = heads
        return out

    @staticmethod
    def backward(ctx, dout):
        q, lse, out = ctx.saved_tensors
        B, N, C = out.shape
        do = _aligned(dout.contiguous())
        dqkv = torch.empty_like(q)
        L._check(L.load().ghn3_attn_wide_bwd(_ptr(dqkv), _ptr(do), _ptr(q), _ptr(lse), _ptr(out), B, N, C, ctx.heads, _stream()),
                 'ghn3_attn_wide_bwd')
        return dqkv, None


def wide_attention(qkv, heads):
    """WideAttention as a function: qkv (B, N, 3 C) -> (B, N, C)."""
    return WideAttention.apply(qkv, int(heads))


def _msa_layer_dims(layer, x):
    """(B, C, H, W, heads, hidden) of an msa layer that meets every condition of the native msa ops except the size limits of
    C, the head dim and hidden, which differ between `MsaLayer` and `MsaWideLayer`; else None.  The conditions: x a 4-d fp32 CUDA
    tensor below 2^31 elements, GHN3_NATIVE_MSA / GHN3_NATIVE_OPS / GHN3_NATIVE_AMP, the module structure of the `msa` op without
    edge features, an integer stride, C % heads == 0, C % 4 == 0, at most 4096 tokens, inactive dropout, exact GELU, one LayerNorm
    eps, fp32 CUDA parameters of the expected shapes, hidden % 4 == 0, B N 3C and B N hidden below 2^31."""
    if not (_native_input(x, 'GHN3_NATIVE_MSA') and x.numel() < 2 ** 31):
        return None
    mods = _msa_modules(layer)
    if mods is None or getattr(layer, 'edge_dim', 0) != 0:
        return None
    ln1, qkv, out, ln2, ff1, ff2, drops, act = mods
    B, C, H, W = x.shape
    heads = int(getattr(layer.attn, 'num_heads', 0))
    stride = getattr(layer, 'stride', 1)
    if not (isinstance(stride, int) and stride >= 1 and heads > 0 and C % heads == 0 and C % 4 == 0 and H * W <= 4096):
        return None
    if not (all(_no_dropout(m) for m in drops) and _is_kind(act, 'GELU') and getattr(act, 'approximate', 'none') == 'none'):
        return None
    if not (tuple(getattr(ln1, 'normalized_shape', ())) == (C,) and tuple(getattr(ln2, 'normalized_shape', ())) == (C,) and
            getattr(ln1, 'eps', None) == getattr(ln2, 'eps', None)):
        return None
    w = [getattr(m, a, None) for m in (ln1, qkv, out, ln2, ff1, ff2) for a in ('weight', 'bias')]
    if w[3] is None:                                   # (to_qkv without a bias, the search space's default)
        w = w[:3] + w[4:]
    if not _f32_cuda(*w):
        return None
    hidden = int(ff1.weight.shape[0])
    want = [(ln1.weight, (C,)), (ln1.bias, (C,)), (qkv.weight, (3 * C, C)), (out.weight, (C, C)), (out.bias, (C,)),
            (ln2.weight, (C,)), (ln2.bias, (C,)), (ff1.weight, (hidden, C)), (ff1.bias, (hidden,)), (ff2.weight, (C, hidden)),
            (ff2.bias, (C,))] + ([] if qkv.bias is None else [(qkv.bias, (3 * C,))])
    if not (all(tuple(t.shape) == s for t, s in want) and hidden % 4 == 0 and B * H * W * 3 * C < 2 ** 31 and
            B * H * W * hidden < 2 ** 31):
        return None
    return B, C, H, W, heads, hidden


def _msa_narrow(C, heads, hidden):
    """The size limits of `MsaLayer` (ghn3_msa_* / ghn3_msa_lean_*); above them `MsaWideLayer` has limits of its own."""
    return C <= 256 and C // heads <= 32 and hidden <= 1024


class MsaLayer(torch.autograd.Function):
    """The pre-LN transformer layer of the ViT-style target networks -- the `msa` op, ops._TransformerLayer with edge_dim = 0
    (graphormer.py:144-248) -- as ONE autograd node on ghn3_msa_fwd / _bwd (ghn3_amd/csrc/tnet_msa.hip): x (B, C, H, W) in NCHW or
    channels_last storage, read as it is; the output (B, C, Ho, Wo) in channels_last storage.  The twelve tensors (MSA_PARAM_NAMES;
    b_qkv may be None) are read in place; their gradients leave as tensors of their own.  Where `msa_lean` says so the node runs
    on ghn3_msa_lean_fwd / _bwd instead: no P tensor exists, and B heads N^2 may be anything."""

    @staticmethod
    def applicable(layer, x):
        dims = _msa_layer_dims(layer, x)
        if dims is None:
            return False
        B, C, H, W, heads, hidden = dims
        return _msa_narrow(C, heads, hidden) and \
            (B <= 65535 if msa_lean(B, heads, H * W) else B * heads * (H * W) ** 2 < 2 ** 31)

    @staticmethod
    def forward(ctx, x, cfg, *params):
        heads, stride, eps, train = cfg
        lib = L.load()
        layout = 1 if (x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()) else 0
        xc = _aligned(x.contiguous(memory_format=torch.channels_last) if layout else x.contiguous())
        ps = [None if t is None else _aligned(t.contiguous()) for t in params]
        B, C, H, W = xc.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        d = _MsaDesc(B, H, W, C, heads, int(ps[8].shape[0]), stride, Ho, Wo, layout, float(eps), int(ps[3] is not None))
        dev = x.device
        out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
        if msa_lean(B, heads, H * W):
            # (lse instead of P; it and everything else the backward reads only when the layer is differentiated)
            scratch = torch.empty(_scratch_floats('ghn3_msa_lean_scratch_floats', d, 0), dtype=torch.float32, device=dev)
            L._check(lib.ghn3_msa_lean_fwd(ctypes.byref(d), _ptr(xc), ctypes.byref(_msa_ptrs(ps)), _ptr(out), _ptr(scratch),
                                           int(train), _stream()), 'ghn3_msa_lean_fwd')
            if train:
                ctx.save_for_backward(xc, scratch, None, *ps)
                ctx.desc = d
            return out
        scratch = torch.empty(_scratch_floats('ghn3_msa_scratch_floats', d, 0), dtype=torch.float32, device=dev)
        # (P and everything the backward reads only when the layer is differentiated)
        P = torch.empty(B * heads * H * W * H * W, dtype=torch.float32, device=dev) if train else None
        L._check(lib.ghn3_msa_fwd(ctypes.byref(d), _ptr(xc), ctypes.byref(_msa_ptrs(ps)), _ptr(out),
                                  _ptr(P), _ptr(scratch), _stream()), 'ghn3_msa_fwd')
        if train:
            ctx.save_for_backward(xc, scratch, P, *ps)
            ctx.desc = d
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = L.load()
        xc, scratch, P, *ps = ctx.saved_tensors
        d = ctx.desc
        do = _aligned(dout.contiguous(memory_format=torch.channels_last))
        dx = torch.empty_like(xc)
        grads = [None if t is None else torch.empty_like(t, memory_format=torch.contiguous_format) for t in ps]
        if P is None:                                      # (the forward ran on the lean attention)
            bscratch = torch.empty(_scratch_floats('ghn3_msa_lean_scratch_floats', d, 1), dtype=torch.float32, device=xc.device)
            L._check(lib.ghn3_msa_lean_bwd(ctypes.byref(d), _ptr(do), _ptr(xc), ctypes.byref(_msa_ptrs(ps)), _ptr(scratch), _ptr(dx),
                                           ctypes.byref(_msa_ptrs(grads)), _ptr(bscratch), _stream()), 'ghn3_msa_lean_bwd')
            return (dx, None) + tuple(grads)
        bscratch = torch.empty(_scratch_floats('ghn3_msa_scratch_floats', d, 1), dtype=torch.float32, device=xc.device)
        L._check(lib.ghn3_msa_bwd(ctypes.byref(d), _ptr(do), _ptr(xc), ctypes.byref(_msa_ptrs(ps)), _ptr(scratch), _ptr(P),
                                  _ptr(dx), ctypes.byref(_msa_ptrs(grads)), _ptr(bscratch), _stream()), 'ghn3_msa_bwd')
        return (dx, None) + tuple(grads)


MSA_WIDE_MAX_C, MSA_WIDE_MAX_D, MSA_WIDE_MAX_HIDDEN = 1024, 64, 4096        # (tnet_msa_wide.hip check_wide)


def msa_wide_enabled():
    """GHN3_NATIVE_MSA_WIDE=1 sends msa layers above `MsaLayer`'s limits to `MsaWideLayer`.  The default is 0: an existing GPU
    test (tests/test_gpu_target_msa.py, the TransformerLayer(512) case) pins the default routing of such a layer to the stock
    path, bit for bit, so the wide op is opt-in."""
    return os.environ.get('GHN3_NATIVE_MSA_WIDE', '0') == '1'


class MsaWideLayer(torch.autograd.Function):
    """`MsaLayer` for the layers above its limits -- C <= 1024, head dim <= 64, hidden <= 4096 -- as ONE autograd node on
    ghn3_msa_wide_fwd / _bwd (ghn3_amd/csrc/tnet_msa_wide.hip): the same layer, arguments, layouts and gradients; attention
    always without a saved P.  A class of its own, so that `MsaLayer.apply` and the node name `MsaLayerBackward` keep meaning
    the narrow op."""

    @staticmethod
    def applicable(layer, x):
        """Every condition of `MsaLayer.applicable` but its limits of C, head dim and hidden, which must be EXCEEDED (narrow
        layers never come here), inside the limits of the C check (ghn3_msa_wide_scratch_floats: every one is mirrored here, so
        that GHN3_E_LIMIT cannot surface in the middle of a network), and GHN3_NATIVE_MSA_WIDE=1."""
        if not msa_wide_enabled():
            return False
        dims = _msa_layer_dims(layer, x)
        if dims is None:
            return False
        B, C, H, W, heads, hidden = dims
        return not _msa_narrow(C, heads, hidden) and C <= MSA_WIDE_MAX_C and C // heads <= MSA_WIDE_MAX_D and \
            hidden <= MSA_WIDE_MAX_HIDDEN and B <= 65535

    @staticmethod
    def forward(ctx, x, cfg, *params):
        heads, stride, eps, train = cfg
        lib = L.load()
        layout = 1 if (x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()) else 0
        xc = _aligned(x.contiguous(memory_format=torch.channels_last) if layout else x.contiguous())
        ps = [None if t is None else _aligned(t.contiguous()) for t in params]
        B, C, H, W = xc.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        d = _MsaDesc(B, H, W, C, heads, int(ps[8].shape[0]), stride, Ho, Wo, layout, float(eps), int(ps[3] is not None))
        out = torch.empty((B, C, Ho, Wo), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        scratch = torch.empty(_scratch_floats('ghn3_msa_wide_scratch_floats', d, 0), dtype=torch.float32, device=x.device)
        L._check(lib.ghn3_msa_wide_fwd(ctypes.byref(d), _ptr(xc), ctypes.byref(_msa_ptrs(ps)), _ptr(out), _ptr(scratch),
                                       int(train), _stream()), 'ghn3_msa_wide_fwd')
        if train:                                          # (else nothing is kept: the scratch goes back to the allocator)
            ctx.save_for_backward(xc, scratch, *ps)
            ctx.desc = d
        return out

    @staticmethod
    def backward(ctx, dout):
        xc, scratch, *ps = ctx.saved_tensors
        d = ctx.desc
        do = _aligned(dout.contiguous(memory_format=torch.channels_last))
        dx = torch.empty_like(xc)
        grads = [None if t is None else torch.empty_like(t, memory_format=torch.contiguous_format) for t in ps]
        bscratch = torch.empty(_scratch_floats('ghn3_msa_wide_scratch_floats', d, 1), dtype=torch.float32, device=xc.device)
        L._check(L.load().ghn3_msa_wide_bwd(ctypes.byref(d), _ptr(do), _ptr(xc), ctypes.byref(_msa_ptrs(ps)), _ptr(scratch),
                                            _ptr(dx), ctypes.byref(_msa_ptrs(grads)), _ptr(bscratch), _stream()),
                 'ghn3_msa_wide_bwd')
        return (dx, None) + tuple(grads)


def msa_params(layer):
    """The twelve tensors of a `_TransformerLayer` in MSA_PARAM_NAMES order (b_qkv None without a QKV bias)."""
    ln1, qkv, out, ln2, ff1, ff2, _, _ = _msa_modules(layer)
    return (ln1.weight, ln1.bias, qkv.weight, qkv.bias, out.weight, out.bias, ln2.weight, ln2.bias, ff1.weight, ff1.bias,
            ff2.weight, ff2.bias)


def run_msa_layer(layer, x):
    """`_TransformerLayer.forward` of a (B, C, H, W) input (tokens, pre-LN attention and feed-forward blocks, stride slicing) on
    the fused op where it applies; None otherwise (the caller keeps its stock layers).  Under torch.no_grad (or with nothing to
    differentiate) the op saves nothing for a backward."""
    if MsaLayer.applicable(layer, x):
        node = MsaLayer
    elif MsaWideLayer.applicable(layer, x):
        node = MsaWideLayer
    else:
        return None
    params = msa_params(layer)
    train = torch.is_grad_enabled() and (x.requires_grad or any(t is not None and t.requires_grad for t in params))
    cfg = (int(layer.attn.num_heads), int(layer.stride), float(layer.ln1.eps), bool(train))
    y = node.apply(x, cfg, *params)
    return _hand_on(y, False, layer.ln1, layer.attn.to_qkv)


# ---- the classifier head and the meta-batch cross-entropy (ghn3_head_* / ghn3_xent_*, ghn3_amd/csrc/tnet_head.hip) ----------
HEAD_MAX_LINEAR = 4
HEAD_MAX_B, HEAD_MAX_F, HEAD_MAX_D = 4096, 32768, 4096     # (ghn3_hip.h: the limits of ghn3_head_desc)
XENT_MAX_B = 4096


class _HeadDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('B', 'C', 'H', 'W', 'layout', 'glob_avg', 'n_lin')] + \
        [('dims', ctypes.c_int32 * (HEAD_MAX_LINEAR + 1)), ('p', ctypes.c_float * (HEAD_MAX_LINEAR - 1))]


class _HeadParams(ctypes.Structure):
    _fields_ = [('w', ctypes.c_void_p * HEAD_MAX_LINEAR), ('b', ctypes.c_void_p * HEAD_MAX_LINEAR),
                ('mask', ctypes.c_void_p * (HEAD_MAX_LINEAR - 1))]


class _HeadGrads(ctypes.Structure):
    _fields_ = [('w', ctypes.c_void_p * HEAD_MAX_LINEAR), ('b', ctypes.c_void_p * HEAD_MAX_LINEAR)]


class _XentDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('n_nets', 'B', 'K')] + [('eps', ctypes.c_float)]


def _head_desc(B, C, H, W, layout, glob_avg, dims, ps=()):
    d = _HeadDesc(B, C, H, W, layout, int(glob_avg), len(dims) - 1)
    for j, v in enumerate(dims[:HEAD_MAX_LINEAR + 1]):        # (more linears than that: refused by the n_lin check)
        d.dims[j] = int(v)
    for j, v in enumerate(ps[:HEAD_MAX_LINEAR - 1]):
        d.p[j] = float(v)
    return d


def head_enabled():
    """GHN3_NATIVE_HEAD=0 (or GHN3_NATIVE_OPS=0) keeps the classifier head and the loss on the stock layers."""
    return enabled() and os.environ.get('GHN3_NATIVE_HEAD', '1') != '0'


def _head_modules(classifier):
    """(linears, dropouts) of a classifier `Linear (ReLU Dropout Linear)*` (ops.network_plan's head table), or None."""
    try:
        mods = list(classifier)
    except TypeError:
        return None
    if len(mods) % 3 != 1:
        return None
    lin, drops = [mods[0]], []
    for j in range(1, len(mods), 3):
        relu, drop, nxt = mods[j:j + 3]
        if not (_is_kind(relu, 'ReLU') and _is_kind(drop, 'Dropout')):
            return None
        drops.append(drop)
        lin.append(nxt)
    if not all(_is_kind(m, 'Linear') for m in lin):
        return None
    return lin, drops


def _is_global_pool(pool):
    if pool is None:
        return False
    size = getattr(pool, 'output_size', None)
    return _is_kind(pool, 'AdaptiveAvgPool2d') and (size == 1 or (isinstance(size, (tuple, list)) and tuple(size) == (1, 1)))


class ClassifierHead(torch.autograd.Function):
    """The end of every target network -- AdaptiveAvgPool2d(1) (glob_avg) or the flatten, then the classifier
    `Linear (ReLU Dropout Linear)*` in fp32 (ops._Network.forward) -- as ONE autograd node on ghn3_head_fwd / _bwd
    (ghn3_amd/csrc/tnet_head.hip): x (B, C, H, W) in NCHW or channels_last storage, read as it is; logits (B, K) fp32.  The
    weights and biases are read in place (the kernels make scalar loads: no alignment, no copy); their gradients leave as
    tensors of their own.  The dropout keep masks are uint8 tensors drawn by torch (one launch each), saved for the
    backward."""

    @staticmethod
    def shape_ok(B, C, H, W, glob_avg, dims):
        """The C limits of ghn3_head_desc (ghn3_head_scratch_floats refuses exactly what this refuses)."""
        F = C if glob_avg else C * H * W
        return 1 <= len(dims) - 1 <= HEAD_MAX_LINEAR and dims[0] == F and 0 < B <= HEAD_MAX_B and F <= HEAD_MAX_F and \
            all(0 < d <= HEAD_MAX_D for d in dims[1:]) and B * C * H * W < 2 ** 31

    @staticmethod
    def applicable(pool, classifier, x):
        if not _native_input(x, 'GHN3_NATIVE_HEAD'):
            return False
        if pool is not None and not _is_global_pool(pool):
            return False
        mods = _head_modules(classifier)
        if mods is None:
            return False
        lin, drops = mods
        if not all(0.0 <= float(getattr(m, 'p', 1.0)) < 1.0 for m in drops):
            return False
        B, C, H, W = x.shape
        dims = [C if pool is not None else C * H * W]
        for m in lin:
            w, b = getattr(m, 'weight', None), getattr(m, 'bias', None)
            if not _f32_cuda(w, b):
                return False
            if w.dim() != 2 or w.shape[1] != dims[-1] or tuple(b.shape) != (w.shape[0],):
                return False
            dims.append(int(w.shape[0]))
        return ClassifierHead.shape_ok(B, C, H, W, pool is not None, dims)

    @staticmethod
    def forward(ctx, x, cfg, *tensors):
        n, glob_avg, ps, train = cfg
        masks, params = tensors[:n - 1], tensors[n - 1:]
        lib = L.load()
        layout = 1 if (x.is_contiguous(memory_format=torch.channels_last) and not x.is_contiguous()) else 0
        xc = x.contiguous(memory_format=torch.channels_last) if layout else x.contiguous()
        ws = [t.contiguous() for t in params]
        B, C, H, W = xc.shape
        dims = [C if glob_avg else C * H * W] + [int(w.shape[0]) for w in ws[0::2]]
        d = _head_desc(B, C, H, W, layout, glob_avg, dims, ps)
        hp = _HeadParams()
        for j in range(n):
            hp.w[j], hp.b[j] = ws[2 * j].data_ptr(), ws[2 * j + 1].data_ptr()
        for j, m in enumerate(masks):
            hp.mask[j] = None if m is None else m.data_ptr()
        logits = torch.empty((B, dims[-1]), dtype=torch.float32, device=x.device)
        scratch = torch.empty(_scratch_floats('ghn3_head_scratch_floats', d, 0), dtype=torch.float32, device=x.device)
        L._check(lib.ghn3_head_fwd(ctypes.byref(d), _ptr(xc), ctypes.byref(hp), _ptr(logits), _ptr(scratch), _stream()),
                 'ghn3_head_fwd')
        if train:
            ctx.save_for_backward(xc, scratch, *masks, *ws)
            ctx.desc, ctx.n = d, n
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        lib = L.load()
        n, d = ctx.n, ctx.desc
        xc, scratch, *rest = ctx.saved_tensors
        masks, ws = rest[:n - 1], rest[n - 1:]
        do = dlogits.contiguous()
        dx = torch.empty_like(xc)
        grads = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in ws]
        hp, hg = _HeadParams(), _HeadGrads()
        for j in range(n):
            hp.w[j], hp.b[j] = ws[2 * j].data_ptr(), ws[2 * j + 1].data_ptr()
            hg.w[j], hg.b[j] = grads[2 * j].data_ptr(), grads[2 * j + 1].data_ptr()
        for j, m in enumerate(masks):
            hp.mask[j] = None if m is None else m.data_ptr()
        bscratch = torch.empty(_scratch_floats('ghn3_head_scratch_floats', d, 1), dtype=torch.float32, device=xc.device)
        L._check(lib.ghn3_head_bwd(ctypes.byref(d), _ptr(do), _ptr(xc), ctypes.byref(hp), _ptr(scratch), _ptr(dx),
                                   ctypes.byref(hg), _ptr(bscratch), _stream()), 'ghn3_head_bwd')
        return (dx, None) + (None,) * (n - 1) + tuple(grads)


def classifier_head(x, weights, biases, masks=(), ps=(), glob_avg=True):
    """The head on the fused op with explicit tensors: weights[j] (d_j+1, d_j), biases[j]; masks[j] (uint8 (B, d_j+1) or
    None) the keep mask of the dropout after linear j (rate ps[j])."""
    _needs_gpu('classifier_head', x)
    n = len(weights)
    masks = list(masks) + [None] * (n - 1 - len(masks))
    ps = [float(p) if m is not None else 0.0 for p, m in zip(list(ps) + [0.0] * (n - 1), masks)]
    params = [t for wb in zip(weights, biases) for t in wb]
    train = torch.is_grad_enabled() and any(t.requires_grad for t in [x] + params)
    return ClassifierHead.apply(x, (n, bool(glob_avg), tuple(ps), bool(train)), *masks, *params)


def run_classifier_head(pool, classifier, x):
    """Global pooling (`pool` = AdaptiveAvgPool2d(1), or None for the flatten of glob_avg = False) + `classifier` on the fused
    op where it applies; None otherwise (the caller keeps its stock layers).  A Dropout in training mode with p > 0 draws its
    keep mask with torch's generator on the current stream, as F.dropout would there.  Under torch.no_grad the op saves nothing for a backward."""
    if not ClassifierHead.applicable(pool, classifier, x):
        return None
    lin, drops = _head_modules(classifier)
    B = x.shape[0]
    masks, ps = [], []
    for drop, nxt in zip(drops, lin[1:]):
        p = float(drop.p)
        if getattr(drop, 'training', True) and p > 0:
            # (torch's own dropout kernel on an uninitialised tensor of the activation's shape: one launch, and the draws the
            # stock F.dropout makes in the same place, so both paths drop the same units)
            keep = torch.native_dropout(torch.empty((B, nxt.weight.shape[1]), device=x.device), p, True)[1]
            masks.append(keep.view(torch.uint8))
            ps.append(p)
        else:
            masks.append(None)
            ps.append(0.0)
    return classifier_head(x, [m.weight for m in lin], [m.bias for m in lin], masks, ps, glob_avg=pool is not None)


class MetaCrossEntropy(torch.autograd.Function):
    """F.cross_entropy(logits_n, targets, label_smoothing) for every network of a meta-batch at once (ghn3_xent_fwd / _bwd):
    ce [n] with autograd, and the top-1 / top-5 hit counts (int32 [2], not differentiable).  A hit is "fewer than k logits
    strictly greater than the target's", topk's rule except on exact ties.  A target outside [0, K) gives a NaN ce[n]."""

    @staticmethod
    def forward(ctx, targets, eps, *logits):
        lib = L.load()
        n, (B, K) = len(logits), logits[0].shape
        dev = logits[0].device
        d = _XentDesc(n, B, K, float(eps))
        ce = torch.empty(n, dtype=torch.float32, device=dev)
        lse = torch.empty(n * B, dtype=torch.float32, device=dev)
        hits = torch.zeros(2, dtype=torch.int32, device=dev)
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in logits])
        L._check(lib.ghn3_xent_fwd(ctypes.byref(d), ptrs, _ptr(targets), _ptr(ce), _ptr(lse), _ptr(hits), _stream()),
                 'ghn3_xent_fwd')
        ctx.mark_non_differentiable(hits)
        ctx.save_for_backward(targets, lse, *logits)
        ctx.desc = d
        return ce, hits

    @staticmethod
    def backward(ctx, dce, _dhits):
        lib = L.load()
        targets, lse, *logits = ctx.saved_tensors
        n = len(logits)
        g = dce.contiguous()
        dl = [torch.empty_like(t) for t in logits]
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in logits])
        dptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dl])
        L._check(lib.ghn3_xent_bwd(ctypes.byref(ctx.desc), ptrs, _ptr(targets), _ptr(lse), _ptr(g), dptrs, _stream()),
                 'ghn3_xent_bwd')
        return (None, None) + tuple(dl)


def _xent_native(logits, targets):
    if not (head_enabled() and not _autocast_excludes() and len(logits) > 0 and torch.is_tensor(targets) and
            targets.is_cuda and targets.dtype == torch.int64 and targets.dim() == 1 and targets.is_contiguous()):
        return False
    shape, dev = logits[0].shape, logits[0].device
    if len(shape) != 2 or shape[0] != targets.shape[0] or targets.device != dev or not 0 < shape[0] <= XENT_MAX_B or \
            shape[1] < 1 or shape[0] * shape[1] >= 2 ** 31:
        return False
    return all(torch.is_tensor(y) and y.is_cuda and y.device == dev and y.dtype == torch.float32 and y.shape == shape and
               y.is_contiguous() for y in logits)


def meta_cross_entropy(logits, targets, label_smoothing=0.0):
    """(ce [n], hits [2]) for the logits of n networks on one batch: ce[n] = F.cross_entropy(logits[n], targets,
    label_smoothing) with autograd; hits = the top-1 / top-5 hit counts over all (network, sample) pairs, on the device, not
    differentiable.  One native launch per 32 networks (MetaCrossEntropy) when every logits tensor is an fp32 contiguous CUDA
    tensor of one shape; else the stock per-network F.cross_entropy and topk."""
    logits = list(logits)
    if _xent_native(logits, targets):
        return MetaCrossEntropy.apply(targets, float(label_smoothing), *logits)
    ce = torch.stack([F.cross_entropy(y.float(), targets, label_smoothing=label_smoothing) for y in logits])
    with torch.no_grad():
        lg = torch.stack([y.detach().float() for y in logits])          # models x batch x classes
        top = lg.topk(min(5, lg.shape[-1]), dim=-1).indices
        hit = top == targets.view(1, -1, 1)
        hits = torch.stack([hit[..., :1].any(-1).sum(), hit.any(-1).sum()])
    return ce, hits


# ---- a cell's state sums, its concatenation and the positional encoding (ghn3_join_* / ghn3_posenc_bwd, csrc/tnet_join.hip) --
JOIN_MAX_SLICES = 16                  # include/ghn3_hip.h GHN3_JOIN_MAX_SLICES
NCHW, NHWC = 0, 1


class _JoinSrc(ctypes.Structure):
    _fields_ = [('p', ctypes.c_void_p), ('grad', ctypes.c_void_p)] + \
        [(n, ctypes.c_int32) for n in ('H', 'W', 'step', 'layout', 'broadcast_n', '_pad')]


class _JoinSlice(ctypes.Structure):
    _fields_ = [('a', _JoinSrc), ('b', _JoinSrc), ('c0', ctypes.c_int32), ('C', ctypes.c_int32)]


class _JoinDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C', 'layout', 'n_slices')] + [('s', _JoinSlice * JOIN_MAX_SLICES)]


def join_enabled():
    """GHN3_NATIVE_JOIN=0 (or GHN3_NATIVE_OPS=0) keeps the stock expressions (a + b, torch.cat, x + weight) everywhere."""
    return enabled() and os.environ.get('GHN3_NATIVE_JOIN', '1') != '0'


def _layout(t):
    """NCHW / NHWC when the 4-d tensor t is dense in that order in memory, else None."""
    if t.is_contiguous():
        return NCHW
    return NHWC if t.is_contiguous(memory_format=torch.channels_last) else None


def _fmt(layout):
    return torch.channels_last if layout else torch.contiguous_format


def join_refusal(slices, broadcast_b=False):
    """Why ghn3_join_fwd / _bwd do not take `slices` = [(a, b or None, a_step, b_step), ...] (the output's channel slices in
    order, each a[:, :, ::a_step, ::a_step] (+ b[...])), or None when they do.  The rules, in the order they are checked --
    the shape rules come before the device's, so they can be asked of CPU and meta tensors, and they mirror the limits of
    include/ghn3_hip.h, so a step never meets the C refusal:
      'slices'   1 .. JOIN_MAX_SLICES slices;
      'type'     every source a 4-d fp32 tensor, every step 1 or 2;
      'channels' C_j % 4 == 0 (so every c0_j % 4 == 0), both sources of a slice of one width;
      'dense'    every source dense in memory in NCHW or in NHWC order;
      'map'      one N (a broadcast b: N == 1) and one output map ceil(H_j / step_j) x ceil(W_j / step_j) for all sources;
      'size'     every source and the output below 2^31 elements;
      'align'    an NHWC source starts on 16 bytes;
      'device'   CUDA tensors of one device;
      'switch'   GHN3_NATIVE_JOIN / GHN3_NATIVE_OPS / GHN3_NATIVE_AMP under autocast."""
    if not 1 <= len(slices) <= JOIN_MAX_SLICES:
        return 'slices'
    srcs = [(t, st, broadcast_b and k == 1) for sl in slices for k, (t, st) in enumerate(((sl[0], sl[2]), (sl[1], sl[3])))
            if k == 0 or t is not None]
    if not all(torch.is_tensor(t) and t.dim() == 4 and t.dtype == torch.float32 and st in (1, 2) for t, st, _ in srcs):
        return 'type'
    if any(a.shape[1] % 4 or (b is not None and b.shape[1] != a.shape[1]) for a, b, _, _ in slices):
        return 'channels'
    if any(_layout(t) is None for t, _, _ in srcs):
        return 'dense'
    a0, _, s0, _ = slices[0]
    N, H, W = a0.shape[0], -(-a0.shape[2] // s0), -(-a0.shape[3] // s0)
    if any(t.shape[0] != (1 if bc else N) or -(-t.shape[2] // st) != H or -(-t.shape[3] // st) != W for t, st, bc in srcs):
        return 'map'
    if any(t.numel() >= 2 ** 31 for t, _, _ in srcs) or N * H * W * sum(sl[0].shape[1] for sl in slices) >= 2 ** 31:
        return 'size'
    if any(_layout(t) == NHWC and t.data_ptr() % 16 for t, _, _ in srcs if t.device.type != 'meta'):
        return 'align'
    if not all(t.is_cuda and t.device == a0.device for t, _, _ in srcs):
        return 'device'
    if not join_enabled() or _autocast_excludes():
        return 'switch'
    return None


def join_applicable(slices, broadcast_b=False):
    """What the join kernels take (join_refusal lists the rules)."""
    return join_refusal(slices, broadcast_b) is None


def _src(t, step, broadcast=False):
    return _JoinSrc(t.data_ptr(), None, t.shape[2], t.shape[3], step, _layout(t), int(broadcast), 0)


def _join_fwd(slices, nhwc, broadcast_b=False):
    """One ghn3_join_fwd launch for slices that passed join_refusal; returns (out, metas) with metas[j] = the
    (shape, step, layout) of slice j's sources, what the backward needs of them."""
    a0, _, s0, _ = slices[0]
    N, H, W = a0.shape[0], -(-a0.shape[2] // s0), -(-a0.shape[3] // s0)
    C = sum(sl[0].shape[1] for sl in slices)
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=a0.device, memory_format=_fmt(nhwc))
    d = _JoinDesc(N, H, W, C, int(bool(nhwc)), len(slices))
    c0, metas = 0, []
    for j, (a, b, sa, sb) in enumerate(slices):
        s = d.s[j]
        s.a, s.c0, s.C = _src(a, sa), c0, a.shape[1]
        if b is not None:
            s.b = _src(b, sb, broadcast_b)
        metas.append(((a.shape, sa, _layout(a)), None if b is None else (b.shape, sb, _layout(b))))
        c0 += a.shape[1]
    L._check(L.load().ghn3_join_fwd(ctypes.byref(d), _ptr(out), _stream()), 'ghn3_join_fwd')
    return out, metas


def _dense_grad(dout, nhwc):
    """(dout as a dense tensor the kernels read, its layout): as it is when it is dense (and starts on 16 bytes if NHWC), else
    a copy (a fresh allocation: aligned) in the forward output's layout."""
    lo = _layout(dout)
    if lo is None or (lo == NHWC and dout.data_ptr() % 16):
        lo = int(bool(nhwc))
        dout = dout.clone(memory_format=_fmt(lo))
    return dout, lo


def _join_bwd(metas, wanted, dout, nhwc):
    """The gradients of the sources of a join, [(grad a, grad b or None), ...]: dout itself for a source that spans all of its
    channels in dout's layout at step 1 (no launch), else a dense tensor of the source's layout and size written by ONE
    ghn3_join_bwd launch for all of them.  wanted[j] = (a needs one, b needs one)."""
    dout, lo = _dense_grad(dout, nhwc)
    N, C, H, W = dout.shape
    d = _JoinDesc(N, H, W, C, lo, len(metas))
    c0, grads, launch = 0, [], False
    for j, (pair, want) in enumerate(zip(metas, wanted)):
        s, row = d.s[j], []
        s.c0, s.C = c0, pair[0][0][1]
        for k, m in enumerate(pair):
            g = None
            if m is not None and want[k]:
                shape, step, layout = m
                if len(metas) == 1 and step == 1 and layout == lo and shape[0] == N:
                    g = dout
                else:
                    g = torch.empty(tuple(shape), dtype=torch.float32, device=dout.device, memory_format=_fmt(layout))
                    src = _JoinSrc(None, g.data_ptr(), shape[2], shape[3], step, layout, 0, 0)
                    if k:
                        s.b = src
                    else:
                        s.a = src
                    launch = True
            row.append(g)
        grads.append(tuple(row))
        c0 += s.C
    if launch:
        L._check(L.load().ghn3_join_bwd(ctypes.byref(d), _ptr(dout), _stream()), 'ghn3_join_bwd')
    return grads, dout, lo


class Join(torch.autograd.Function):
    """Channel slices a_j[:, :, ::sa_j, ::sa_j] (+ b_j[:, :, ::sb_j, ::sb_j]) written side by side as ONE autograd node on
    ghn3_join_fwd / _bwd: one slice of two sources is an intermediate state of a cell (pair_sum), single-source slices are the
    cell's concatenation (cell_concat).  spec[j] = (a_step, b_step or 0 for a single source); the tensors follow in slice
    order.  Nothing is saved for the backward but the sources' shapes; the stock backward of torch.cat hands out strided
    slices of dout, which every fused layer below then copies for itself -- here every source gets a dense gradient from one
    launch, or dout itself where that is the gradient (a sum's source in dout's layout at step 1)."""

    @staticmethod
    def forward(ctx, spec, nhwc, *tensors):
        slices, k = [], 0
        for sa, sb in spec:
            slices.append((tensors[k], tensors[k + 1] if sb else None, sa, sb or 1))
            k += 2 if sb else 1
        out, ctx.metas = _join_fwd(slices, nhwc)
        ctx.nhwc = nhwc
        return out

    @staticmethod
    def backward(ctx, dout):
        need, wanted = list(ctx.needs_input_grad[2:]), []
        for _, b in ctx.metas:
            wanted.append((need.pop(0), need.pop(0) if b is not None else False))
        grads = _join_bwd(ctx.metas, wanted, dout, ctx.nhwc)[0]
        return (None, None) + tuple(g for (ga, gb), (_, b) in zip(grads, ctx.metas) for g in ((ga, gb) if b is not None else (ga,)))


class PosEnc(torch.autograd.Function):
    """x + w for w (1, C, ks, ks), the learned positional encoding of the ViT-style networks: the forward is a join whose second
    source is read for every n; dx is dout (copied only when x was stored in the other order), dw = the sum of dout over n in
    a fixed order (ghn3_posenc_bwd), a dense tensor of w's shape."""

    @staticmethod
    def forward(ctx, x, w, nhwc):
        out, ctx.metas = _join_fwd([(x, w.contiguous(), 1, 1)], nhwc, broadcast_b=True)
        ctx.nhwc = nhwc
        return out

    @staticmethod
    def backward(ctx, dout):
        grads, dout, lo = _join_bwd(ctx.metas, [(ctx.needs_input_grad[0], False)], dout, ctx.nhwc)
        dx, dw = grads[0][0], None
        if ctx.needs_input_grad[1]:
            N, C, H, W = dout.shape
            dw = torch.empty((1, C, H, W), dtype=torch.float32, device=dout.device)
            L._check(L.load().ghn3_posenc_bwd(N, C, H, W, lo, _ptr(dout), _ptr(dw), _stream()), 'ghn3_posenc_bwd')
        return dx, dw, None


def join(slices, nhwc=True):
    """The general form: slices = [(a, b or None, a_step, b_step), ...] -> one native node writing the (N, sum of C_j, H, W)
    tensor in NHWC (channels_last) or NCHW storage; None where the kernels do not apply (join_refusal): the caller keeps its
    torch expression."""
    slices = list(slices)
    if join_refusal(slices) is not None:
        return None
    spec = tuple((int(sa), 0 if b is None else int(sb)) for _, b, sa, sb in slices)
    return Join.apply(spec, bool(nhwc), *[t for a, b, _, _ in slices for t in ((a,) if b is None else (a, b))])


def pair_sum(a, b, a_step=1, b_step=1, nhwc=True):
    """a[:, :, ::a_step, ::a_step] + b[:, :, ::b_step, ::b_step], one intermediate state of a cell, as one native node (or
    None, as join).  In the backward a source stored as dout is and read at step 1 receives dout itself, without a launch."""
    return join([(a, b, a_step, b_step)], nhwc)


def cell_concat(states, nhwc=True):
    """torch.cat(states, dim=1), the end of a cell, as one native node (or None, as join)."""
    return join([(t, None, 1, 1) for t in states], nhwc)


def pos_enc(x, w, nhwc=None):
    """x + w for the (1, C, ks, ks) weight view the GHN assigned, as one native node; the output is stored as x is unless nhwc
    says otherwise.  None where the kernels do not apply."""
    if not (torch.is_tensor(x) and torch.is_tensor(w) and x.dim() == 4 and tuple(w.shape) == (1,) + tuple(x.shape[1:])):
        return None
    if join_refusal([(x, w if w.is_contiguous() else w.contiguous(), 1, 1)], broadcast_b=True) is not None:
        return None
    return PosEnc.apply(x, w, _layout(x) == NHWC if nhwc is None else bool(nhwc))
