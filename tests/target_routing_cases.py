"""The routing table of the target-network convolution blocks (tests/test_target_routing_cpu.py): which C entry points a block
reaches through ghn3_amd.target_ops' runners, with which descriptor, which pointers null, and what the backward's one allocation
looks like -- for every runner, norm slot, switch and hand-over rule.  No GPU and no kernel runs: the test replaces the library
by a recorder.

CASES says what is run; EXPECT says, case by case and as literals, what must be recorded.  The literals were RECORDED from the
commit before the runners were folded into one norm-slot dispatch and one node core per family (the six-node, seven-runner
target_ops.py), and must stay as they are when that code is reorganised: a changed literal is a changed routing decision.

A recorded line is one of

    <C function> [<descriptor fields>] ptrs=<one character per argument after the descriptor, the stream left out: x a pointer,
                 - null>  and, for a *_bwd function, `carve=` how its gradients lie in the backward's one allocation:
                 dbeta|dgamma -- dgamma starts 4 C_out bytes after dbeta (the pair the kernels sum in one pass),
                 scratch%256  -- the scratch area starts a multiple of 256 bytes (64 floats) after the first gradient
    stock:<kind>    a stand-in layer was called (the stock path)
    stats:<what>    the norm layer's running statistics after the call: `moved` (num_batches_tracked + 1) or `untouched` (the
                    three buffers bit-identical)
    out:<layout>    NCHW or NHWC storage of the result, `None` where the runner declines

EXPECT[case]['grad'] is a forward in grad mode followed by out.sum().backward(); EXPECT[case]['no_grad'] a forward under
torch.no_grad().
"""
import torch

TRACE = []                      # what the stand-in layers and the recording library append to


# ---- stand-in layers: the runners ask type(m).__name__ and attributes only ----------------------------------------------------
def _flavour(base):
    class _Layer(base):
        def __init__(self, **kw):
            super().__init__()
            self.__dict__.update(kw)

        def __call__(self, x):
            TRACE.append('stock:' + type(self).__name__)
            return x

    return {k: type(k, (_Layer,), {}) for k in ('ReLU', 'Conv2d', 'BatchNorm2d', 'Identity', 'MaxPool2d')}


FLAVOURS = {'light': _flavour(object), 'nn': _flavour(torch.nn.Module)}
SLOTS = ('batch_run', 'batch', 'frozen', 'identity')


def _t(*shape, grad=True, dtype=torch.float32):
    return (0.1 * torch.randn(*shape)).to(dtype).requires_grad_(grad)


def conv(K, C_out, C_in, kernel, stride=1, padding=0, dilation=1, groups=1, bias=False):
    pair = lambda v: v if isinstance(v, (tuple, str)) else (v, v)
    kh, kw = pair(kernel)
    return K['Conv2d'](weight=_t(C_out, C_in // groups, kh, kw), bias=_t(C_out) if bias else None, kernel_size=(kh, kw),
                       stride=pair(stride), padding=pair(padding), dilation=pair(dilation), groups=groups)


def norm(K, slot, C):
    """The four norm slots: BatchNorm2d in training mode with / without running statistics, with them in eval mode, Identity."""
    if slot == 'identity':
        return K['Identity']()
    run = slot != 'batch'
    return K['BatchNorm2d'](weight=_t(C), bias=_t(C), eps=1e-5, momentum=0.1, training=slot != 'frozen', track_running_stats=run,
                            running_mean=torch.zeros(C) if run else None, running_var=torch.ones(C) if run else None,
                            num_batches_tracked=torch.tensor(0) if run else None)


# ---- builders: name -> (runner, its arguments before keep_layout, the norm layers) ------------------------------------------
def block(K, slot, C_in=8, C_out=16, ks=3, stride=1, pad=1, dil=1, N=2, H=8, groups=None, dtype=torch.float32, pw_bias=False):
    bn = norm(K, slot, C_out)
    layers = [K['ReLU'](inplace=False), conv(K, C_in, C_in, ks, stride, pad, dil, groups=groups or C_in),
              conv(K, C_out, C_in, 1, bias=pw_bias), bn]
    return 'run_block', (layers, _t(N, C_in, H, H, dtype=dtype)), [bn]


def pointwise(K, slot, C_in=8, C_out=8, stride=1, N=2, H=4):
    bn = norm(K, slot, C_out)
    return 'run_pointwise_block', ([K['ReLU'](inplace=False), conv(K, C_out, C_in, 1, stride), bn], _t(N, C_in, H, H)), [bn]


def conv_block(K, slot, C_in=8, C_out=16, ks=3, stride=1, pad=1, N=2, H=4, bias=False):
    bn = norm(K, slot, C_out)
    return 'run_conv_block', ([K['ReLU'](inplace=False), conv(K, C_out, C_in, ks, stride, pad, bias=bias), bn],
                              _t(N, C_in, H, H)), [bn]


def conv_pair(K, slot, C=8, mid=8, N=1, H=8):
    bn = norm(K, slot, C)
    layers = [K['ReLU'](inplace=False), conv(K, mid, C, (1, 7), 1, (0, 3)), conv(K, C, mid, (7, 1), 1, (3, 0)), bn]
    return 'run_conv_pair_block', (layers, _t(N, C, H, H)), [bn]


def factorized_reduce(K, slot, C_in=8, half=4, N=2, H=4):
    bn = norm(K, slot, 2 * half)
    return 'run_factorized_reduce', (K['ReLU'](inplace=False), conv(K, half, C_in, 1, 2), conv(K, half, C_in, 1, 2), bn,
                                     _t(N, C_in, H, H)), [bn]


def seq_stem(K, slot, N=1, H=8):
    """[Conv2d(3 -> 8), norm, ReLU, Conv2d, norm, MaxPool2d] on an image."""
    bn1, bn2 = norm(K, slot, 8), norm(K, slot, 8)
    layers = [conv(K, 8, 3, 3, 1, 1), bn1, K['ReLU'](inplace=False), conv(K, 8, 8, 3, 2, 1), bn2,
              K['MaxPool2d'](kernel_size=3, stride=2, padding=1)]
    return 'run_layer_seq', (layers, _t(N, 3, H, H, grad=False)), [bn1, bn2]


def seq_inplace_relu(K, slot, N=2, H=4):
    """[ReLU(inplace=True), Conv2d, norm]: the ReLU runs as the layer it is, the node gets relu = 0."""
    bn = norm(K, slot, 8)
    return 'run_layer_seq', ([K['ReLU'](inplace=True), conv(K, 8, 8, 3, 1, 1), bn], _t(N, 8, H, H)), [bn]


def conv_layer(K, slot, ks=3, H=6, N=2):
    return 'run_conv_layer', (conv(K, 8, 3, ks, ks), _t(N, 3, H, H, grad=False)), []


BUILDERS = {f.__name__: f for f in (block, pointwise, conv_block, conv_pair, factorized_reduce, seq_stem, seq_inplace_relu,
                                    conv_layer)}


def case(builder, slot='batch_run', modes=('grad',), flavour='light', keep_layout=None, env=None, autocast=False, **kw):
    return dict(builder=builder, slot=slot, modes=modes, flavour=flavour, keep_layout=keep_layout, env=env or {},
                autocast=autocast, kw=kw)


def _every_slot(name, builder, **kw):
    return {'%s/%s' % (name, s): case(builder, s, ('grad', 'no_grad'), **kw) for s in SLOTS}


CASES = {}
# runner x norm slot, each forward + backward and under no_grad
CASES.update(_every_slot('block_k3_s2', 'block', ks=3, stride=2, pad=1))
CASES.update(_every_slot('block_k5_d2', 'block', C_out=8, ks=5, pad=4, dil=2))
CASES.update(_every_slot('block_wide_in', 'block', C_in=516, C_out=8, N=1, H=2))
CASES.update(_every_slot('block_wide_out', 'block', C_in=8, C_out=516, N=1, H=2))
CASES.update(_every_slot('pointwise_c8', 'pointwise'))
CASES.update(_every_slot('pointwise_wide_in', 'pointwise', C_in=516, N=1, H=2))
CASES.update(_every_slot('conv_3x3', 'conv_block'))
CASES.update(_every_slot('pair_same_mid', 'conv_pair'))
CASES.update(_every_slot('pair_other_mid', 'conv_pair', mid=12))
CASES.update(_every_slot('factorized_reduce', 'factorized_reduce'))
CASES.update(_every_slot('seq_stem', 'seq_stem'))
CASES.update(_every_slot('seq_inplace_relu', 'seq_inplace_relu'))
CASES['conv_layer_3x3_s3'] = case('conv_layer', None, ('grad', 'no_grad'))
CASES['conv_layer_16x16_s16'] = case('conv_layer', None, ('grad', 'no_grad'), ks=16, H=32)
# falling back to the stock layers
CASES['off/GHN3_NATIVE_OPS'] = case('block', env={'GHN3_NATIVE_OPS': '0'})
CASES['off/GHN3_NATIVE_OPS/factorized_reduce'] = case('factorized_reduce', env={'GHN3_NATIVE_OPS': '0'})
CASES['off/GHN3_NATIVE_CONV'] = case('conv_block', env={'GHN3_NATIVE_CONV': '0'})
CASES['off/GHN3_NATIVE_CONV/pointwise_c8_stays_native'] = case('pointwise', env={'GHN3_NATIVE_CONV': '0'})
CASES['off/GHN3_NATIVE_NONORM'] = case('block', 'identity', env={'GHN3_NATIVE_NONORM': '0'})
CASES['off/GHN3_NATIVE_NONORM/conv_3x3'] = case('conv_block', 'identity', env={'GHN3_NATIVE_NONORM': '0'})
CASES['off/GHN3_NATIVE_EVALBN'] = case('block', 'frozen', env={'GHN3_NATIVE_EVALBN': '0'})
CASES['off/GHN3_NATIVE_EVALBN/conv_3x3'] = case('conv_block', 'frozen', env={'GHN3_NATIVE_EVALBN': '0'})
CASES['off/GHN3_NATIVE_WIDE'] = case('block', C_in=516, C_out=8, N=1, H=2, env={'GHN3_NATIVE_WIDE': '0'})
CASES['off/GHN3_NATIVE_WIDE/pointwise_wide_out'] = case('pointwise', C_out=516, N=1, H=2, env={'GHN3_NATIVE_WIDE': '0'})
CASES['off/GHN3_NATIVE_STEM'] = case('conv_layer', None, env={'GHN3_NATIVE_STEM': '0'})
CASES['off/GHN3_NATIVE_STEM/16x16'] = case('conv_layer', None, ks=16, H=32, env={'GHN3_NATIVE_STEM': '0'})
CASES['off/autocast_without_amp'] = case('conv_block', autocast=True, env={'GHN3_NATIVE_AMP': '0'})
CASES['on/autocast_with_amp'] = case('conv_block', autocast=True)
CASES['off/conv_bias'] = case('conv_block', bias=True)
CASES['off/pointwise_bias'] = case('block', pw_bias=True)
CASES['off/depthwise_groups'] = case('block', groups=4)
CASES['off/c_in_6'] = case('pointwise', C_in=6)
CASES['off/fp16_input'] = case('block', dtype=torch.float16)
CASES['off/padding_same'] = case('conv_block', pad='same')
# hand-over: the layout the next layer receives
CASES['hand_on/nn'] = case('block', flavour='nn')
CASES['hand_on/nn/keep_layout'] = case('block', flavour='nn', keep_layout=True)
CASES['hand_on/light'] = case('block', flavour='light', keep_layout=False)
CASES['hand_on/light/eager_layout'] = case('block', flavour='light', keep_layout=False, env={'GHN3_NATIVE_LAZY_LAYOUT': '0'})
CASES['hand_on/light/eager_layout/keep_layout'] = case('block', flavour='light', keep_layout=True,
                                                       env={'GHN3_NATIVE_LAZY_LAYOUT': '0'})
CASES['hand_on/nn/wide'] = case('block', flavour='nn', C_in=516, C_out=8, N=1, H=2)
CASES['hand_on/nn/pair/frozen'] = case('conv_pair', 'frozen', flavour='nn')
CASES['hand_on/nn/seq_stem'] = case('seq_stem', flavour='nn')

EXPECT = {
    'block_k3_s2/batch_run': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'block_k3_s2/batch': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxxxx',
            'out:NHWC',
        ],
    },
    'block_k3_s2/frozen': {
        'grad': [
            'ghn3_dwpw_frozen_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_frozen_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_frozen_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxxxxx-x',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'block_k3_s2/identity': {
        'grad': [
            'ghn3_dwpw_plain_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=0] ptrs=xxxx',
            'ghn3_dwpw_plain_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=0] ptrs=xxxxxxxx carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_plain_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=2 pad=1 dil=1 Ho=4 Wo=4 eps=0] ptrs=xxxx',
            'out:NHWC',
        ],
    },
    'block_k5_d2/batch_run': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'block_k5_d2/batch': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'out:NHWC',
        ],
    },
    'block_k5_d2/frozen': {
        'grad': [
            'ghn3_dwpw_frozen_fwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_frozen_bwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_frozen_fwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxx-x',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'block_k5_d2/identity': {
        'grad': [
            'ghn3_dwpw_plain_fwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=0] ptrs=xxxx',
            'ghn3_dwpw_plain_bwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=0] ptrs=xxxxxxxx carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_plain_fwd [N=2 H=8 W=8 C_in=8 C_out=8 ks=5 stride=1 pad=4 dil=2 Ho=8 Wo=8 eps=0] ptrs=xxxx',
            'out:NHWC',
        ],
    },
    'block_wide_in/batch_run': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'block_wide_in/batch': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'out:NHWC',
        ],
    },
    'block_wide_in/frozen': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_frozen_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_frozen_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxx-xx',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'block_wide_in/identity': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x--x',
            'out:NHWC',
        ],
    },
    'block_wide_out/batch_run': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'block_wide_out/batch': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'out:NHWC',
        ],
    },
    'block_wide_out/frozen': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_frozen_fwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_frozen_fwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxx-xx',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'block_wide_out/identity': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=8 C_out=8 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=8 C_out=516 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x--x',
            'out:NHWC',
        ],
    },
    'pointwise_c8/batch_run': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=x-xxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxx-xxx-xxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=x-xxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'pointwise_c8/batch': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=x-xxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxx-xxx-xxxx carve=dbeta|dgamma,scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=x-xxxxxxx',
            'out:NHWC',
        ],
    },
    'pointwise_c8/frozen': {
        'grad': [
            'ghn3_dwpw_frozen_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=x-xxxxxxx',
            'ghn3_dwpw_frozen_bwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxx-xxxxx-xxxx carve=dbeta|dgamma,scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_frozen_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=x-xxxxx-x',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'pointwise_c8/identity': {
        'grad': [
            'ghn3_dwpw_plain_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=0] ptrs=x-xx',
            'ghn3_dwpw_plain_bwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=0] ptrs=xx-xx-xx carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_dwpw_plain_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=0] ptrs=x-xx',
            'out:NHWC',
        ],
    },
    'pointwise_wide_in/batch_run': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'pointwise_wide_in/batch': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'out:NHWC',
        ],
    },
    'pointwise_wide_in/frozen': {
        'grad': [
            'ghn3_conv_frozen_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_frozen_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxx-xx',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'pointwise_wide_in/identity': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=3 eps=0] ptrs=xx--x--x',
            'out:NHWC',
        ],
    },
    'conv_3x3/batch_run': {
        'grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'conv_3x3/batch': {
        'grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'out:NHWC',
        ],
    },
    'conv_3x3/frozen': {
        'grad': [
            'ghn3_conv_frozen_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_frozen_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxx-xx',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'conv_3x3/identity': {
        'grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=3 eps=0] ptrs=xx--x--x',
            'out:NHWC',
        ],
    },
    'pair_same_mid/batch_run': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'pair_same_mid/batch': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'out:NHWC',
        ],
    },
    'pair_same_mid/frozen': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxx-xx',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'pair_same_mid/identity': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x--x',
            'out:NHWC',
        ],
    },
    'pair_other_mid/batch_run': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'pair_other_mid/batch': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'out:NHWC',
        ],
    },
    'pair_other_mid/frozen': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxx-xx',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'pair_other_mid/identity': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=12 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=12 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x--x',
            'out:NHWC',
        ],
    },
    'factorized_reduce/batch_run': {
        'grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'factorized_reduce/batch': {
        'grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'out:NHWC',
        ],
    },
    'factorized_reduce/frozen': {
        'grad': [
            'ghn3_conv_frozen_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_frozen_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=1 eps=1e-05] ptrs=xxxxxx-xx',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'factorized_reduce/identity': {
        'grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=2 kw=2 stride_h=2 stride_w=2 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=3 eps=0] ptrs=xx--x--x',
            'out:NHWC',
        ],
    },
    'seq_stem/batch_run': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'stock:MaxPool2d',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'stock:MaxPool2d',
            'stats:moved',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'seq_stem/batch': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'stock:MaxPool2d',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'stock:MaxPool2d',
            'out:NHWC',
        ],
    },
    'seq_stem/frozen': {
        'grad': [
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxx',
            'stock:MaxPool2d',
            'ghn3_conv_frozen_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_frozen_bwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:untouched',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxx-xx',
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxx-xx',
            'stock:MaxPool2d',
            'stats:untouched',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'seq_stem/identity': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=3 eps=0] ptrs=xx--x--x',
            'stock:MaxPool2d',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=2 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=3 eps=0] ptrs=xx--x--x',
            'stock:MaxPool2d',
            'out:NHWC',
        ],
    },
    'seq_inplace_relu/batch_run': {
        'grad': [
            'stock:ReLU',
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
        'no_grad': [
            'stock:ReLU',
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'seq_inplace_relu/batch': {
        'grad': [
            'stock:ReLU',
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'stock:ReLU',
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'out:NHWC',
        ],
    },
    'seq_inplace_relu/frozen': {
        'grad': [
            'stock:ReLU',
            'ghn3_conv_frozen_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:untouched',
            'out:NHWC',
        ],
        'no_grad': [
            'stock:ReLU',
            'ghn3_conv_frozen_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=0 eps=1e-05] ptrs=xxxxxx-xx',
            'stats:untouched',
            'out:NHWC',
        ],
    },
    'seq_inplace_relu/identity': {
        'grad': [
            'stock:ReLU',
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=2 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=2 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NHWC',
        ],
        'no_grad': [
            'stock:ReLU',
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=2 eps=0] ptrs=xx--x--x',
            'out:NHWC',
        ],
    },
    'conv_layer_3x3_s3': {
        'grad': [
            'ghn3_conv_bn_fwd [N=2 H=6 W=6 C_in=4 C_out=8 kh=3 kw=3 stride_h=3 stride_w=3 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x--x',
            'ghn3_conv_bn_bwd [N=2 H=6 W=6 C_in=4 C_out=8 kh=3 kw=3 stride_h=3 stride_w=3 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'out:NCHW',
        ],
        'no_grad': [
            'ghn3_conv_bn_fwd [N=2 H=6 W=6 C_in=4 C_out=8 kh=3 kw=3 stride_h=3 stride_w=3 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=2 eps=0] ptrs=xx--x--x',
            'out:NCHW',
        ],
    },
    'conv_layer_16x16_s16': {
        'grad': [
            'ghn3_patch_fwd [N=2 H=32 W=32 C_in=3 C_out=8 kh=16 kw=16 stride_h=16 stride_w=16 Ho=2 Wo=2 nhwc=0] ptrs=xxx-',
            'ghn3_patch_bwd [N=2 H=32 W=32 C_in=3 C_out=8 kh=16 kw=16 stride_h=16 stride_w=16 Ho=2 Wo=2 nhwc=0] ptrs=xxx-xx',
            'out:NCHW',
        ],
        'no_grad': [
            'ghn3_patch_fwd [N=2 H=32 W=32 C_in=3 C_out=8 kh=16 kw=16 stride_h=16 stride_w=16 Ho=2 Wo=2 nhwc=0] ptrs=xxx-',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_OPS': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_OPS/factorized_reduce': {
        'grad': [
            'stats:untouched',
            'out:None',
        ],
    },
    'off/GHN3_NATIVE_CONV': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_CONV/pointwise_c8_stays_native': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=x-xxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=8 ks=1 stride=1 pad=0 dil=1 Ho=4 Wo=4 eps=1e-05] ptrs=xxxx-xxx-xxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'off/GHN3_NATIVE_NONORM': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:Conv2d',
            'stock:Identity',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_NONORM/conv_3x3': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:Identity',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_EVALBN': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_EVALBN/conv_3x3': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_WIDE': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_WIDE/pointwise_wide_out': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_STEM': {
        'grad': [
            'stock:Conv2d',
            'out:NCHW',
        ],
    },
    'off/GHN3_NATIVE_STEM/16x16': {
        'grad': [
            'stock:Conv2d',
            'out:NCHW',
        ],
    },
    'off/autocast_without_amp': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'on/autocast_with_amp': {
        'grad': [
            'ghn3_conv_bn_fwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=2 H=4 W=4 C_in=8 C_out=16 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'off/conv_bias': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/pointwise_bias': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/depthwise_groups': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/c_in_6': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/fp16_input': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'off/padding_same': {
        'grad': [
            'stock:ReLU',
            'stock:Conv2d',
            'stock:BatchNorm2d',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'hand_on/nn': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NCHW',
        ],
    },
    'hand_on/nn/keep_layout': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'hand_on/light': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'hand_on/light/eager_layout': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NCHW',
        ],
    },
    'hand_on/light/eager_layout/keep_layout': {
        'grad': [
            'ghn3_dwpw_bn_fwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_dwpw_bn_bwd [N=2 H=8 W=8 C_in=8 C_out=16 ks=3 stride=1 pad=1 dil=1 Ho=8 Wo=8 eps=1e-05] ptrs=xxxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'out:NHWC',
        ],
    },
    'hand_on/nn/wide': {
        'grad': [
            'ghn3_dw_fwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxx',
            'ghn3_conv_bn_fwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_bwd [N=1 H=2 W=2 C_in=516 C_out=8 kh=1 kw=1 stride_h=1 stride_w=1 pad_h=0 pad_w=0 dil=1 Ho=2 Wo=2 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_dw_bwd [N=1 H=2 W=2 C_in=516 C_out=516 ks=3 stride=1 pad=1 dil=1 Ho=2 Wo=2 eps=0] ptrs=xxxxxx carve=scratch%256',
            'stats:moved',
            'out:NCHW',
        ],
    },
    'hand_on/nn/pair/frozen': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x--x',
            'ghn3_conv_frozen_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxx',
            'ghn3_conv_frozen_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=7 kw=1 stride_h=1 stride_w=1 pad_h=3 pad_w=0 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=1 kw=7 stride_h=1 stride_w=1 pad_h=0 pad_w=3 dil=1 Ho=8 Wo=8 relu=3 eps=0] ptrs=xx--x-xx--x carve=scratch%256',
            'stats:untouched',
            'out:NCHW',
        ],
    },
    'hand_on/nn/seq_stem': {
        'grad': [
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxx',
            'ghn3_conv_bn_fwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxx',
            'stock:MaxPool2d',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=8 C_out=8 kh=3 kw=3 stride_h=2 stride_w=2 pad_h=1 pad_w=1 dil=1 Ho=4 Wo=4 relu=1 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'ghn3_conv_bn_bwd [N=1 H=8 W=8 C_in=4 C_out=8 kh=3 kw=3 stride_h=1 stride_w=1 pad_h=1 pad_w=1 dil=1 Ho=8 Wo=8 relu=0 eps=1e-05] ptrs=xxxxxxxxxxx carve=dbeta|dgamma,scratch%256',
            'stats:moved',
            'stats:moved',
            'out:NCHW',
        ],
    },
}
