"""The host contract of the target-network convolution ops' C entry points (ghn3_amd/csrc/target_ops.hip), pinned without a GPU
(tests/test_target_host_cpu.py): what the seven `*_scratch_floats` functions answer -- the exact size, or the exact code and
ghn3_last_error() text of the refusal -- and which calls of the twelve forward / backward entry points are refused, with which
code and text.  Every call here returns before the first HIP call.

DWPW / CONV / PATCH say which descriptors are asked, ENTRY which pointers an entry point requires; SIZES and REFUSALS say, as
literals, what must come back.  The literals were RECORDED (`python tests/target_host_cases.py <library>` prints them) from the
library of the commit before the host code of the two families was folded into one core per family and one description of
each scratch layout, and must stay as they are when that code is reorganised: a changed size is a buffer the caller allocates
differently from how the entry point carves it, a changed text a changed rule.

This module needs ctypes alone: the test runs it in a process of its own that sees no GPU (a call that should have been refused
and is not then fails at its first launch instead of launching a kernel on dummy pointers).
"""
import ctypes
import json
import os
import sys

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ghn3_amd', 'lib', 'libghn3_hip.so')
NO_NORM = 2                          # GHN3_CONV_NO_NORM
DUMMY = 16                           # a non-null pointer nothing dereferences


class Dwpw(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C_in', 'C_out', 'ks', 'stride', 'pad', 'dil', 'Ho', 'Wo')] + \
        [('eps', ctypes.c_float)]


class Conv(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C_in', 'C_out', 'kh', 'kw', 'stride_h', 'stride_w', 'pad_h', 'pad_w',
                                              'dil', 'Ho', 'Wo', 'relu')] + [('eps', ctypes.c_float)]


class Patch(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ('N', 'H', 'W', 'C_in', 'C_out', 'kh', 'kw', 'stride_h', 'stride_w', 'Ho', 'Wo', 'nhwc')]


def _out(size, k, stride, pad, dil):
    return (size + 2 * pad - dil * (k - 1) - 1) // stride + 1


def dwpw(N, H, W, C_in, C_out, ks=3, stride=1, pad=None, dil=1, dHo=0):
    """A ghn3_dwpw_desc; pad defaults to `same` at stride 1, Ho / Wo follow from the arithmetic (dHo: Ho off by that much)."""
    pad = dil * (ks - 1) // 2 if pad is None else pad
    return (N, H, W, C_in, C_out, ks, stride, pad, dil, _out(H, ks, max(stride, 1), pad, dil) + dHo, _out(W, ks, max(stride, 1), pad, dil))


def conv(N, H, W, C_in, C_out, k=(3, 3), stride=(1, 1), pad=None, dil=1, relu=0, dHo=0):
    pad = (dil * (k[0] - 1) // 2, dil * (k[1] - 1) // 2) if pad is None else pad
    return (N, H, W, C_in, C_out, k[0], k[1], stride[0], stride[1], pad[0], pad[1], dil,
            _out(H, k[0], max(stride[0], 1), pad[0], dil) + dHo, _out(W, k[1], max(stride[1], 1), pad[1], dil), relu)


# ---- descriptors of the size functions ------------------------------------------------------------------------------------------
# P = N Ho Wo output pixels; the pixel tile is 64, a reduction step 32 pixels
DWPW = {
    'spot/n2_8x8_c32': dwpw(2, 8, 8, 32, 32),
    'spot/n3_7x5_c4_c8_s2': dwpw(3, 7, 5, 4, 8, stride=2),
    # pixel tile: P = 1, 40, 64, 65, 243
    'P1': dwpw(1, 1, 1, 4, 4, ks=1),
    'P40': dwpw(2, 9, 7, 8, 12, stride=2, pad=1),
    'P64': dwpw(1, 8, 8, 8, 8),
    'P65': dwpw(1, 13, 5, 8, 8),
    'P243': dwpw(3, 9, 9, 8, 12),
    # chunks of the pointwise weight gradient: clamped at ceil(P / 32) (one block of 64 x 64: 768 wanted), at 768 blocks (64
    # blocks: 12), and a single chunk
    'pw_chunks/P40_c4': dwpw(1, 8, 5, 4, 4),
    'pw_chunks/P200_c4': dwpw(2, 10, 10, 4, 4),
    'pw_chunks/P4096_c512': dwpw(4, 32, 32, 512, 512),
    'pw_chunks/P4096_c64_c512': dwpw(4, 32, 32, 64, 512),
    # pixels per chunk of the depthwise weight gradient: 16 (P <= 4096), in between (P = 10000: 48), 128 (P = 32768 exactly, beyond)
    'dw_chunk_px/P4096': dwpw(1, 64, 64, 4, 4),
    'dw_chunk_px/P4097': dwpw(1, 241, 17, 4, 4),
    'dw_chunk_px/P10000': dwpw(1, 100, 100, 4, 4),
    'dw_chunk_px/P32768': dwpw(2, 128, 128, 4, 4),
    'dw_chunk_px/P65536': dwpw(4, 128, 128, 4, 4),
    # widths: 4, 64, 68, 128, 256, 260, 512 accepted (the column tiles of the forward change at 64, 128, 256); 516 and 6 refused
    'width/c4_c64': dwpw(2, 6, 6, 4, 64),
    'width/c64_c68': dwpw(2, 6, 6, 64, 68),
    'width/c68_c128': dwpw(2, 6, 6, 68, 128),
    'width/c128_c256': dwpw(2, 6, 6, 128, 256),
    'width/c256_c260': dwpw(2, 6, 6, 256, 260),
    'width/c260_c512': dwpw(2, 6, 6, 260, 512),
    'width/c512_c4': dwpw(2, 6, 6, 512, 4),
    'width/c516_in': dwpw(2, 6, 6, 516, 8),
    'width/c516_out': dwpw(2, 6, 6, 8, 516),
    'width/c516_both': dwpw(1, 2, 2, 516, 516),
    'width/c6_in': dwpw(2, 6, 6, 6, 8),
    'width/c6_out': dwpw(2, 6, 6, 8, 6),
    # the depthwise kernel: ks 1, 2, 3, 7, 8 (refused); stride 2; dilation 2; no padding
    'ks1': dwpw(2, 6, 6, 8, 16, ks=1),
    'ks1_s2': dwpw(2, 6, 6, 8, 16, ks=1, stride=2),
    'ks1_pad1': dwpw(2, 6, 6, 8, 16, ks=1, pad=1),
    'ks2': dwpw(2, 6, 6, 8, 8, ks=2, pad=1),
    'ks7': dwpw(1, 9, 9, 8, 8, ks=7),
    'ks8': dwpw(1, 9, 9, 8, 8, ks=8, pad=4),
    'ks5_d2': dwpw(2, 8, 8, 8, 8, ks=5, dil=2),
    'ks3_s2_d2': dwpw(2, 9, 9, 8, 8, stride=2, pad=2, dil=2),
    'ks3_pad0': dwpw(2, 6, 6, 8, 8, pad=0),
    # descriptor errors
    'bad/null': None,
    'bad/Ho_plus_1': dwpw(2, 6, 6, 8, 8, dHo=1),
    'bad/Ho_minus_1': dwpw(2, 6, 6, 8, 8, dHo=-1),
    'bad/kernel_larger_than_image': dwpw(1, 2, 2, 8, 8, ks=5, pad=0),
    'bad/N0': dwpw(0, 6, 6, 8, 8),
    'bad/C_out0': dwpw(2, 6, 6, 8, 0),
    'bad/stride0': dwpw(2, 6, 6, 8, 8, stride=0),
    'bad/pad_negative': dwpw(2, 6, 6, 8, 8, pad=-1),
    # N H W C: the largest that fits with C = 508 (2^31 - 131072), 2^31 exactly, and N Ho Wo C_out alone at 2^31 or more
    '2^31/just_below': dwpw(1, 2048, 2064, 508, 508, ks=1),
    '2^31/exactly': dwpw(64, 256, 256, 512, 512, ks=1),
    '2^31/output_only': dwpw(64, 255, 255, 512, 512, ks=1, pad=1),
    # the depthwise stage alone: C_out == C_in, C <= 16384
    'alone/c1024': dwpw(2, 4, 4, 1024, 1024),
    'alone/c16384': dwpw(1, 2, 2, 16384, 16384),
    'alone/c16388': dwpw(1, 2, 2, 16388, 16388),
    'alone/c1024_c512': dwpw(2, 4, 4, 1024, 512),
}

CONV = {
    'spot/n2_9x9_c16_c24_3x1': conv(2, 9, 9, 16, 24, k=(3, 1), stride=(2, 1), pad=(1, 0), relu=1),
    # pixel tile
    'P1': conv(1, 1, 1, 4, 4, k=(1, 1)),
    'P40': conv(2, 9, 7, 8, 12, stride=(2, 2), pad=(1, 1)),
    'P64': conv(1, 8, 8, 8, 8),
    'P65': conv(1, 13, 5, 8, 8),
    'P243': conv(3, 9, 9, 8, 12),
    # chunks of the weight gradient: clamped at ceil(P / 32); 9 taps of one block: 86; at 768 blocks; a single chunk
    'w_chunks/P40_c4_1x1': conv(1, 8, 5, 4, 4, k=(1, 1)),
    'w_chunks/P4096_c64_3x3': conv(4, 32, 32, 64, 64),
    'w_chunks/P4096_c512_1x1': conv(4, 32, 32, 512, 512, k=(1, 1)),
    'w_chunks/P4096_c512_3x3': conv(4, 32, 32, 512, 512),
    # columns per workgroup of the convolution kernel: 32, 64 and more columns, few and many tiles
    'nt/c32_P1024': conv(1, 32, 32, 16, 32),
    'nt/c64_P16384': conv(16, 32, 32, 16, 64),
    'nt/c128_P16384': conv(16, 32, 32, 16, 128),
    'nt/c128_P64': conv(1, 8, 8, 16, 128),
    # kernels: 1 x 1, 3 x 3, 1 x 7, 7 x 1, 7 x 7; 8 x 1 and 1 x 8 refused
    'k/1x7': conv(2, 8, 8, 8, 8, k=(1, 7)),
    'k/7x1': conv(2, 8, 8, 8, 8, k=(7, 1)),
    'k/7x7_d2': conv(1, 14, 14, 8, 8, k=(7, 7), dil=2),
    'k/8x1': conv(2, 8, 8, 8, 8, k=(8, 1), pad=(4, 0)),
    'k/1x8': conv(2, 8, 8, 8, 8, k=(1, 8), pad=(0, 4)),
    'stride_2x1_pad0': conv(2, 9, 8, 8, 8, stride=(2, 1), pad=(0, 0)),
    'stride_1x3': conv(2, 9, 8, 8, 8, stride=(1, 3)),
    # widths: C_out 4096 / 4100, C_in 16384 / 16388, 6; a weight of 2^30 elements (refused) and 15 * 2^26
    'width/c_out4096': conv(1, 2, 2, 8, 4096, k=(1, 1)),
    'width/c_out4100': conv(1, 2, 2, 8, 4100, k=(1, 1)),
    'width/c_in16384': conv(1, 2, 2, 16384, 8, k=(1, 1)),
    'width/c_in16388': conv(1, 2, 2, 16388, 8, k=(1, 1)),
    'width/c_in6': conv(1, 2, 2, 6, 8, k=(1, 1)),
    'width/c_out6': conv(1, 2, 2, 8, 6, k=(1, 1)),
    'weight/2^30': conv(1, 4, 4, 16384, 4096, k=(4, 4), pad=(2, 2)),
    'weight/15*2^26': conv(1, 4, 4, 16384, 4096, k=(3, 5)),
    # relu: bit 0 the ReLU, bit 1 GHN3_CONV_NO_NORM (which does not change a size)
    'relu0': conv(2, 6, 6, 8, 16, relu=0),
    'relu1': conv(2, 6, 6, 8, 16, relu=1),
    'relu2': conv(2, 6, 6, 8, 16, relu=2),
    'relu3': conv(2, 6, 6, 8, 16, relu=3),
    # descriptor errors
    'bad/null': None,
    'bad/Ho_plus_1': conv(2, 6, 6, 8, 8, dHo=1),
    'bad/H0': conv(2, 0, 6, 8, 8),
    'bad/stride_w0': conv(2, 6, 6, 8, 8, stride=(1, 0)),
    'bad/pad_negative': conv(2, 6, 6, 8, 8, pad=(1, -1)),
    '2^31/just_below': conv(1, 2048, 2064, 508, 8, k=(1, 1)),
    '2^31/exactly': conv(64, 256, 256, 8, 512, k=(1, 1)),
    '2^31/output_only': conv(64, 255, 255, 512, 512, k=(1, 1), pad=(1, 1)),
}

# (N, H, W, C_in, C_out, kh, kw, stride_h, stride_w, Ho, Wo, nhwc): the unchanged control
PATCH = {
    'vit_16x16': (2, 224, 224, 3, 384, 16, 16, 16, 16, 14, 14, 0),
    'vit_16x16_nhwc': (2, 224, 224, 3, 384, 16, 16, 16, 16, 14, 14, 1),
    'one_chunk': (1, 32, 32, 3, 4096, 32, 32, 32, 32, 1, 1, 0),
    '8x8_trailing_rows': (3, 35, 37, 3, 64, 8, 8, 8, 8, 4, 4, 0),
    'kernel_7': (2, 28, 28, 3, 64, 7, 7, 7, 7, 4, 4, 0),
    'overlapping': (2, 32, 32, 3, 64, 16, 16, 8, 8, 3, 3, 0),
    'bad/Ho': (2, 224, 224, 3, 384, 16, 16, 16, 16, 15, 14, 0),
    'bad/null': None,
}

SIZE_FUNCTIONS = {
    'dwpw': (Dwpw, DWPW, ('ghn3_dwpw_scratch_floats', 'ghn3_dwpw_plain_scratch_floats', 'ghn3_dwpw_frozen_scratch_floats',
                          'ghn3_dw_scratch_floats')),
    'conv': (Conv, CONV, ('ghn3_conv_scratch_floats', 'ghn3_conv_frozen_scratch_floats')),
    'patch': (Patch, PATCH, ('ghn3_patch_scratch_floats',)),
}

# ---- the entry points: the arguments between the descriptor and the stream, `?` in front of the optional ones -----------------------
ENTRY = {
    'ghn3_dwpw_bn_fwd': 'x ?w_dw w_pw gamma beta z out stats scratch',
    'ghn3_dwpw_bn_bwd': 'dout x z stats ?w_dw w_pw gamma dx ?dw_dw dw_pw dgamma dbeta scratch',
    'ghn3_dwpw_plain_fwd': 'x ?w_dw w_pw out',
    'ghn3_dwpw_plain_bwd': 'dout x ?w_dw w_pw dx ?dw_dw dw_pw scratch',
    'ghn3_dwpw_frozen_fwd': 'x ?w_dw w_pw gamma beta mean var ?z out',
    'ghn3_dwpw_frozen_bwd': 'dout x z ?w_dw w_pw gamma mean var dx ?dw_dw dw_pw dgamma dbeta scratch',
    'ghn3_dw_fwd': 'x w_dw y',
    'ghn3_dw_bwd': 'dout x w_dw dx dw_dw scratch',
    'ghn3_conv_bn_fwd': 'x w gamma beta z out stats scratch',
    'ghn3_conv_bn_bwd': 'dout x z stats w gamma dx dw dgamma dbeta scratch',
    'ghn3_conv_frozen_fwd': 'x w gamma beta mean var ?z out scratch',
    'ghn3_conv_frozen_bwd': 'dout x z w gamma mean var dx dw dgamma dbeta scratch',
}
# under GHN3_CONV_NO_NORM the norm layer's arguments of ghn3_conv_bn_* may be null; the others are still required
NO_NORM_OPTIONAL = {'ghn3_conv_bn_fwd': ('gamma', 'beta', 'out', 'stats'), 'ghn3_conv_bn_bwd': ('z', 'stats', 'gamma', 'dgamma', 'dbeta')}
GOOD_DWPW = dwpw(2, 9, 7, 8, 12, stride=2, pad=1)                # ks = 3
GOOD_DW = dwpw(2, 9, 7, 8, 8, stride=2, pad=1)
GOOD_CONV = conv(2, 9, 7, 8, 12, stride=(2, 2), pad=(1, 1), relu=1)


def entry_calls():
    """(case name, function, descriptor tuple or None, relu flags or None, {argument: null?}) of every refused call."""
    for fn, spec in ENTRY.items():
        args = [a.lstrip('?') for a in spec.split()]
        required = [a.lstrip('?') for a in spec.split() if not a.startswith('?')]
        family = 'conv' if '_conv_' in fn else 'dw' if fn.startswith('ghn3_dw_') else 'dwpw'
        good = {'conv': GOOD_CONV, 'dw': GOOD_DW, 'dwpw': GOOD_DWPW}[family]
        yield fn + '/null_descriptor', fn, None, args, ()
        yield fn + '/bad_descriptor', fn, good[:-2] + (good[-2] + 1, good[-1]) if family != 'conv' else good[:12] + (good[12] + 1,) + good[13:], \
            args, ()
        for a in required:                                          # each required pointer null in turn
            yield '%s/null_%s' % (fn, a), fn, good, args, (a,)
        if family == 'dwpw':
            yield fn + '/no_w_dw_with_ks3', fn, good, args, ('w_dw',) + (('dw_dw',) if 'dw_dw' in args else ())
            if 'dw_dw' in args:                                     # depthwise weights without room for their gradient
                yield fn + '/w_dw_without_dw_dw', fn, good, args, ('dw_dw',)
            if '?z' in spec.split():                                # z is optional: the call gets as far as the w_dw rule
                yield fn + '/no_z_no_w_dw_with_ks3', fn, good, args, ('z', 'w_dw')
        if family == 'conv' and '_frozen_' in fn:
            yield fn + '/no_norm_flag', fn, good[:-1] + (good[-1] | NO_NORM,), args, ()
            yield fn + '/no_norm_flag_and_null_x', fn, good[:-1] + (good[-1] | NO_NORM,), args, ('x',)
        if fn in NO_NORM_OPTIONAL:                                  # the norm's arguments all null: still refused for the other one
            for a in required:
                if a not in NO_NORM_OPTIONAL[fn]:
                    yield '%s/no_norm_null_%s' % (fn, a), fn, good[:-1] + (good[-1] | NO_NORM,), args, NO_NORM_OPTIONAL[fn] + (a,)


def record(lib_path=LIB):
    """{'sizes': {family: {descriptor: {function: [forward, backward]}}}, 'refusals': {case: [code, text]}}; a refusal of a size
    function is [code, text] in place of the size."""
    lib = ctypes.CDLL(lib_path)
    lib.ghn3_last_error.restype = ctypes.c_char_p
    sizes = {}
    for family, (struct, descs, functions) in SIZE_FUNCTIONS.items():
        sizes[family] = {}
        for name, fields in descs.items():
            d = None if fields is None else ctypes.byref(struct(*fields))
            row = sizes[family][name] = {}
            for fn in functions:
                f = getattr(lib, fn)
                f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int]
                row[fn] = []
                for backward in (0, 1):
                    n = int(f(d, backward))
                    row[fn].append(n if n >= 0 else [n, lib.ghn3_last_error().decode()])
    refusals = {}
    for case, fn, fields, args, null in entry_calls():
        struct = Conv if '_conv_' in fn else Dwpw
        d = None if fields is None else ctypes.byref(struct(*fields))
        f = getattr(lib, fn)
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p] * (len(args) + 2)
        rc = int(f(d, *[None if a in null else DUMMY for a in args], None))
        refusals[case] = [rc, lib.ghn3_last_error().decode()]
    return {'sizes': sizes, 'refusals': refusals}


def _literals(rec):
    lines = ['SIZES = {']
    for family, descs in rec['sizes'].items():
        lines.append('    %r: {' % family)
        for name, row in descs.items():
            lines.append('        %r: {' % name)
            lines += ['            %r: %r,' % kv for kv in row.items()]
            lines.append('        },')
        lines.append('    },')
    lines += ['}', '', 'REFUSALS = {']
    lines += ['    %r: %r,' % kv for kv in rec['refusals'].items()]
    return '\n'.join(lines + ['}'])


if __name__ == '__main__':
    rec = record(*[a for a in sys.argv[1:] if not a.startswith('--')])
    print(json.dumps(rec) if '--json' in sys.argv else _literals(rec))
    sys.exit(0)

# ---- recorded from the library of the commit before the reorganisation ------------------------------------------------------------
SIZES = {
    'dwpw': {
        'spot/n2_8x8_c32': {
            'ghn3_dwpw_scratch_floats': [192, 10944],
            'ghn3_dwpw_plain_scratch_floats': [0, 10752],
            'ghn3_dwpw_frozen_scratch_floats': [0, 11008],
            'ghn3_dw_scratch_floats': [0, 2560],
        },
        'spot/n3_7x5_c4_c8_s2': {
            'ghn3_dwpw_scratch_floats': [80, 604],
            'ghn3_dwpw_plain_scratch_floats': [0, 572],
            'ghn3_dwpw_frozen_scratch_floats': [0, 620],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'P1': {
            'ghn3_dwpw_scratch_floats': [72, 296],
            'ghn3_dwpw_plain_scratch_floats': [0, 280],
            'ghn3_dwpw_frozen_scratch_floats': [0, 304],
            'ghn3_dw_scratch_floats': [0, 260],
        },
        'P40': {
            'ghn3_dwpw_scratch_floats': [88, 1032],
            'ghn3_dwpw_plain_scratch_floats': [0, 984],
            'ghn3_dwpw_frozen_scratch_floats': [0, 1056],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'P64': {
            'ghn3_dwpw_scratch_floats': [80, 1216],
            'ghn3_dwpw_plain_scratch_floats': [0, 1184],
            'ghn3_dwpw_frozen_scratch_floats': [0, 1232],
            'ghn3_dw_scratch_floats': [0, 544],
        },
        'P65': {
            'ghn3_dwpw_scratch_floats': [96, 1376],
            'ghn3_dwpw_plain_scratch_floats': [0, 1328],
            'ghn3_dwpw_frozen_scratch_floats': [0, 1392],
            'ghn3_dw_scratch_floats': [0, 616],
        },
        'P243': {
            'ghn3_dwpw_scratch_floats': [160, 4240],
            'ghn3_dwpw_plain_scratch_floats': [0, 4120],
            'ghn3_dwpw_frozen_scratch_floats': [0, 4264],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'pw_chunks/P40_c4': {
            'ghn3_dwpw_scratch_floats': [72, 572],
            'ghn3_dwpw_plain_scratch_floats': [0, 556],
            'ghn3_dwpw_frozen_scratch_floats': [0, 580],
            'ghn3_dw_scratch_floats': [0, 364],
        },
        'pw_chunks/P200_c4': {
            'ghn3_dwpw_scratch_floats': [96, 1676],
            'ghn3_dwpw_plain_scratch_floats': [0, 1636],
            'ghn3_dwpw_frozen_scratch_floats': [0, 1684],
            'ghn3_dw_scratch_floats': [0, 724],
        },
        'pw_chunks/P4096_c512': {
            'ghn3_dwpw_scratch_floats': [65600, 6489344],
            'ghn3_dwpw_plain_scratch_floats': [0, 6422784],
            'ghn3_dwpw_frozen_scratch_floats': [0, 6490368],
            'ghn3_dw_scratch_floats': [0, 1179904],
        },
        'pw_chunks/P4096_c64_c512': {
            'ghn3_dwpw_scratch_floats': [65600, 2573568],
            'ghn3_dwpw_plain_scratch_floats': [0, 2507008],
            'ghn3_dwpw_frozen_scratch_floats': [0, 2574592],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'dw_chunk_px/P4096': {
            'ghn3_dwpw_scratch_floats': [576, 28424],
            'ghn3_dwpw_plain_scratch_floats': [0, 27904],
            'ghn3_dwpw_frozen_scratch_floats': [0, 28432],
            'ghn3_dw_scratch_floats': [0, 9472],
        },
        'dw_chunk_px/P4097': {
            'ghn3_dwpw_scratch_floats': [584, 23880],
            'ghn3_dwpw_plain_scratch_floats': [0, 23352],
            'ghn3_dwpw_frozen_scratch_floats': [0, 23888],
            'ghn3_dw_scratch_floats': [0, 4900],
        },
        'dw_chunk_px/P10000': {
            'ghn3_dwpw_scratch_floats': [1320, 54052],
            'ghn3_dwpw_plain_scratch_floats': [0, 52788],
            'ghn3_dwpw_frozen_scratch_floats': [0, 54060],
            'ghn3_dw_scratch_floats': [0, 7780],
        },
        'dw_chunk_px/P32768': {
            'ghn3_dwpw_scratch_floats': [4160, 152840],
            'ghn3_dwpw_plain_scratch_floats': [0, 148736],
            'ghn3_dwpw_frozen_scratch_floats': [0, 152848],
            'ghn3_dw_scratch_floats': [0, 9472],
        },
        'dw_chunk_px/P65536': {
            'ghn3_dwpw_scratch_floats': [8256, 299960],
            'ghn3_dwpw_plain_scratch_floats': [0, 291760],
            'ghn3_dwpw_frozen_scratch_floats': [0, 299968],
            'ghn3_dw_scratch_floats': [0, 18688],
        },
        'width/c4_c64': {
            'ghn3_dwpw_scratch_floats': [320, 1876],
            'ghn3_dwpw_plain_scratch_floats': [0, 1492],
            'ghn3_dwpw_frozen_scratch_floats': [0, 2004],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c64_c68': {
            'ghn3_dwpw_scratch_floats': [336, 21208],
            'ghn3_dwpw_plain_scratch_floats': [0, 20800],
            'ghn3_dwpw_frozen_scratch_floats': [0, 21344],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c68_c128': {
            'ghn3_dwpw_scratch_floats': [576, 35092],
            'ghn3_dwpw_plain_scratch_floats': [0, 34324],
            'ghn3_dwpw_frozen_scratch_floats': [0, 35348],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c128_c256': {
            'ghn3_dwpw_scratch_floats': [1088, 115072],
            'ghn3_dwpw_plain_scratch_floats': [0, 113536],
            'ghn3_dwpw_frozen_scratch_floats': [0, 115584],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c256_c260': {
            'ghn3_dwpw_scratch_floats': [1104, 231448],
            'ghn3_dwpw_plain_scratch_floats': [0, 229888],
            'ghn3_dwpw_frozen_scratch_floats': [0, 231968],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c260_c512': {
            'ghn3_dwpw_scratch_floats': [2112, 433108],
            'ghn3_dwpw_plain_scratch_floats': [0, 430036],
            'ghn3_dwpw_frozen_scratch_floats': [0, 434132],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c512_c4': {
            'ghn3_dwpw_scratch_floats': [80, 66328],
            'ghn3_dwpw_plain_scratch_floats': [0, 66304],
            'ghn3_dwpw_frozen_scratch_floats': [0, 66336],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c516_in': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 8, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 8, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 8, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 8, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 8, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 8, ks 3)']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c516_out': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 516, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 516, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 516, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 516, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 516, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 516, ks 3)']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c516_both': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 516, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 516, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 516, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 516, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 516, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 516 -> 516, ks 3)']],
            'ghn3_dw_scratch_floats': [0, 4900],
        },
        'width/c6_in': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 6 -> 8, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 6 -> 8, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 6 -> 8, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 6 -> 8, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 6 -> 8, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 6 -> 8, ks 3)']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'width/c6_out': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 6, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 6, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 6, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 6, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 6, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 6, ks 3)']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'ks1': {
            'ghn3_dwpw_scratch_floats': [128, 1352],
            'ghn3_dwpw_plain_scratch_floats': [0, 1256],
            'ghn3_dwpw_frozen_scratch_floats': [0, 1384],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'ks1_s2': {
            'ghn3_dwpw_scratch_floats': [96, 608],
            'ghn3_dwpw_plain_scratch_floats': [0, 544],
            'ghn3_dwpw_frozen_scratch_floats': [0, 640],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'ks1_pad1': {
            'ghn3_dwpw_scratch_floats': [128, 1952],
            'ghn3_dwpw_plain_scratch_floats': [0, 1856],
            'ghn3_dwpw_frozen_scratch_floats': [0, 1984],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'ks2': {
            'ghn3_dwpw_scratch_floats': [96, 1568],
            'ghn3_dwpw_plain_scratch_floats': [0, 1520],
            'ghn3_dwpw_frozen_scratch_floats': [0, 1584],
            'ghn3_dw_scratch_floats': [0, 480],
        },
        'ks7': {
            'ghn3_dwpw_scratch_floats': [96, 3496],
            'ghn3_dwpw_plain_scratch_floats': [0, 3448],
            'ghn3_dwpw_frozen_scratch_floats': [0, 3512],
            'ghn3_dw_scratch_floats': [0, 2608],
        },
        'ks8': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 8, ks 8)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 8, ks 8)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 8, ks 8)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 8, ks 8)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 8, ks 8)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 8 -> 8, ks 8)']],
            'ghn3_dw_scratch_floats': [[-2, 'dw: needs C a multiple of 4 and <= 16384, ks <= 7 (got 8, ks 8)'], [-2, 'dw: needs C a multiple of 4 and <= 16384, ks <= 7 (got 8, ks 8)']],
        },
        'ks5_d2': {
            'ghn3_dwpw_scratch_floats': [96, 3184],
            'ghn3_dwpw_plain_scratch_floats': [0, 3136],
            'ghn3_dwpw_frozen_scratch_floats': [0, 3200],
            'ghn3_dw_scratch_floats': [0, 1856],
        },
        'ks3_s2_d2': {
            'ghn3_dwpw_scratch_floats': [80, 1104],
            'ghn3_dwpw_plain_scratch_floats': [0, 1072],
            'ghn3_dwpw_frozen_scratch_floats': [0, 1120],
            'ghn3_dw_scratch_floats': [0, 544],
        },
        'ks3_pad0': {
            'ghn3_dwpw_scratch_floats': [80, 752],
            'ghn3_dwpw_plain_scratch_floats': [0, 720],
            'ghn3_dwpw_frozen_scratch_floats': [0, 768],
            'ghn3_dw_scratch_floats': [0, 400],
        },
        'bad/null': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: null descriptor'], [-1, 'dwpw: null descriptor']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: null descriptor'], [-1, 'dwpw: null descriptor']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: null descriptor'], [-1, 'dwpw: null descriptor']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: null descriptor'], [-1, 'dw: null descriptor']],
        },
        'bad/Ho_plus_1': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: output size 7 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'dwpw: output size 7 x 6 does not match the convolution arithmetic (6 x 6)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: output size 7 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'dwpw: output size 7 x 6 does not match the convolution arithmetic (6 x 6)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: output size 7 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'dwpw: output size 7 x 6 does not match the convolution arithmetic (6 x 6)']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: output size 7 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'dw: output size 7 x 6 does not match the convolution arithmetic (6 x 6)']],
        },
        'bad/Ho_minus_1': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: output size 5 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'dwpw: output size 5 x 6 does not match the convolution arithmetic (6 x 6)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: output size 5 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'dwpw: output size 5 x 6 does not match the convolution arithmetic (6 x 6)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: output size 5 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'dwpw: output size 5 x 6 does not match the convolution arithmetic (6 x 6)']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: output size 5 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'dw: output size 5 x 6 does not match the convolution arithmetic (6 x 6)']],
        },
        'bad/kernel_larger_than_image': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: output size -2 x -2 does not match the convolution arithmetic (-2 x -2)'], [-1, 'dwpw: output size -2 x -2 does not match the convolution arithmetic (-2 x -2)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: output size -2 x -2 does not match the convolution arithmetic (-2 x -2)'], [-1, 'dwpw: output size -2 x -2 does not match the convolution arithmetic (-2 x -2)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: output size -2 x -2 does not match the convolution arithmetic (-2 x -2)'], [-1, 'dwpw: output size -2 x -2 does not match the convolution arithmetic (-2 x -2)']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: output size -2 x -2 does not match the convolution arithmetic (-2 x -2)'], [-1, 'dw: output size -2 x -2 does not match the convolution arithmetic (-2 x -2)']],
        },
        'bad/N0': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'bad/C_out0': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'bad/stride0': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        'bad/pad_negative': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: non-positive size in the descriptor'], [-1, 'dwpw: non-positive size in the descriptor']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
        '2^31/just_below': {
            'ghn3_dwpw_scratch_floats': [67104832, 2234331576],
            'ghn3_dwpw_plain_scratch_floats': [0, 2167225792],
            'ghn3_dwpw_frozen_scratch_floats': [0, 2234332592],
            'ghn3_dw_scratch_floats': [0, 16776448],
        },
        '2^31/exactly': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: activation tensors of 2^31 elements or more are not supported'], [-1, 'dwpw: activation tensors of 2^31 elements or more are not supported']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: activation tensors of 2^31 elements or more are not supported'], [-1, 'dwpw: activation tensors of 2^31 elements or more are not supported']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: activation tensors of 2^31 elements or more are not supported'], [-1, 'dwpw: activation tensors of 2^31 elements or more are not supported']],
            'ghn3_dw_scratch_floats': [[-2, 'dw: activation tensors of 2^31 elements or more are not supported'], [-2, 'dw: activation tensors of 2^31 elements or more are not supported']],
        },
        '2^31/output_only': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: activation tensors of 2^31 elements or more are not supported'], [-1, 'dwpw: activation tensors of 2^31 elements or more are not supported']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: activation tensors of 2^31 elements or more are not supported'], [-1, 'dwpw: activation tensors of 2^31 elements or more are not supported']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: activation tensors of 2^31 elements or more are not supported'], [-1, 'dwpw: activation tensors of 2^31 elements or more are not supported']],
            'ghn3_dw_scratch_floats': [[-2, 'dw: activation tensors of 2^31 elements or more are not supported'], [-2, 'dw: activation tensors of 2^31 elements or more are not supported']],
        },
        'alone/c1024': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 1024, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 1024, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 1024, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 1024, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 1024, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 1024, ks 3)']],
            'ghn3_dw_scratch_floats': [0, 18688],
        },
        'alone/c16384': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16384 -> 16384, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16384 -> 16384, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16384 -> 16384, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16384 -> 16384, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16384 -> 16384, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16384 -> 16384, ks 3)']],
            'ghn3_dw_scratch_floats': [0, 147712],
        },
        'alone/c16388': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16388 -> 16388, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16388 -> 16388, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16388 -> 16388, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16388 -> 16388, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16388 -> 16388, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 16388 -> 16388, ks 3)']],
            'ghn3_dw_scratch_floats': [[-2, 'dw: needs C a multiple of 4 and <= 16384, ks <= 7 (got 16388, ks 3)'], [-2, 'dw: needs C a multiple of 4 and <= 16384, ks <= 7 (got 16388, ks 3)']],
        },
        'alone/c1024_c512': {
            'ghn3_dwpw_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 512, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 512, ks 3)']],
            'ghn3_dwpw_plain_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 512, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 512, ks 3)']],
            'ghn3_dwpw_frozen_scratch_floats': [[-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 512, ks 3)'], [-1, 'dwpw: needs C_in, C_out multiples of 4 and <= 512, ks <= 7 (got 1024 -> 512, ks 3)']],
            'ghn3_dw_scratch_floats': [[-1, 'dw: non-positive size in the descriptor, or C_out != C_in'], [-1, 'dw: non-positive size in the descriptor, or C_out != C_in']],
        },
    },
    'conv': {
        'spot/n2_9x9_c16_c24_3x1': {
            'ghn3_conv_scratch_floats': [3616, 8320],
            'ghn3_conv_frozen_scratch_floats': [3520, 8368],
        },
        'P1': {
            'ghn3_conv_scratch_floats': [264, 484],
            'ghn3_conv_frozen_scratch_floats': [256, 492],
        },
        'P40': {
            'ghn3_conv_scratch_floats': [5272, 5968],
            'ghn3_conv_frozen_scratch_floats': [5248, 5992],
        },
        'P64': {
            'ghn3_conv_scratch_floats': [3536, 5408],
            'ghn3_conv_frozen_scratch_floats': [3520, 5424],
        },
        'P65': {
            'ghn3_conv_scratch_floats': [3552, 6008],
            'ghn3_conv_frozen_scratch_floats': [3520, 6024],
        },
        'P243': {
            'ghn3_conv_scratch_floats': [5344, 13660],
            'ghn3_conv_frozen_scratch_floats': [5248, 13684],
        },
        'w_chunks/P40_c4_1x1': {
            'ghn3_conv_scratch_floats': [264, 656],
            'ghn3_conv_frozen_scratch_floats': [256, 664],
        },
        'w_chunks/P4096_c64_3x3': {
            'ghn3_conv_scratch_floats': [63552, 2685312],
            'ghn3_conv_frozen_scratch_floats': [55360, 2685440],
        },
        'w_chunks/P4096_c512_1x1': {
            'ghn3_conv_scratch_floats': [458816, 5702912],
            'ghn3_conv_frozen_scratch_floats': [393280, 5703936],
        },
        'w_chunks/P4096_c512_3x3': {
            'ghn3_conv_scratch_floats': [3604544, 10421504],
            'ghn3_conv_frozen_scratch_floats': [3539008, 10422528],
        },
        'nt/c32_P1024': {
            'ghn3_conv_scratch_floats': [14912, 188480],
            'ghn3_conv_frozen_scratch_floats': [13888, 188544],
        },
        'nt/c64_P16384': {
            'ghn3_conv_scratch_floats': [60480, 1888128],
            'ghn3_conv_frozen_scratch_floats': [27712, 1888256],
        },
        'nt/c128_P16384': {
            'ghn3_conv_scratch_floats': [120896, 2983424],
            'ghn3_conv_frozen_scratch_floats': [55360, 2983680],
        },
        'nt/c128_P64': {
            'ghn3_conv_scratch_floats': [55616, 73472],
            'ghn3_conv_frozen_scratch_floats': [55360, 73728],
        },
        'k/1x7': {
            'ghn3_conv_scratch_floats': [2784, 5808],
            'ghn3_conv_frozen_scratch_floats': [2752, 5824],
        },
        'k/7x1': {
            'ghn3_conv_scratch_floats': [2784, 5808],
            'ghn3_conv_frozen_scratch_floats': [2752, 5824],
        },
        'k/7x7_d2': {
            'ghn3_conv_scratch_floats': [18944, 42672],
            'ghn3_conv_frozen_scratch_floats': [18880, 42688],
        },
        'k/8x1': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 8, 8 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 8, 8 x 1)']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 8, 8 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 8, 8 x 1)']],
        },
        'k/1x8': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 8, 1 x 8)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 8, 1 x 8)']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 8, 1 x 8)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 8, 1 x 8)']],
        },
        'stride_2x1_pad0': {
            'ghn3_conv_scratch_floats': [3536, 5280],
            'ghn3_conv_frozen_scratch_floats': [3520, 5296],
        },
        'stride_1x3': {
            'ghn3_conv_scratch_floats': [3536, 5328],
            'ghn3_conv_frozen_scratch_floats': [3520, 5344],
        },
        'width/c_out4096': {
            'ghn3_conv_scratch_floats': [204864, 114944],
            'ghn3_conv_frozen_scratch_floats': [196672, 123136],
        },
        'width/c_out4100': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 4100, 1 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 4100, 1 x 1)']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 4100, 1 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 4100, 1 x 1)']],
        },
        'width/c_in16384': {
            'ghn3_conv_scratch_floats': [196688, 917824],
            'ghn3_conv_frozen_scratch_floats': [196672, 917840],
        },
        'width/c_in16388': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 16388 -> 8, 1 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 16388 -> 8, 1 x 1)']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 16388 -> 8, 1 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 16388 -> 8, 1 x 1)']],
        },
        'width/c_in6': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 6 -> 8, 1 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 6 -> 8, 1 x 1)']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 6 -> 8, 1 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 6 -> 8, 1 x 1)']],
        },
        'width/c_out6': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 6, 1 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 6, 1 x 1)']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 6, 1 x 1)'], [-2, 'conv: needs C_in, C_out multiples of 4, C_out <= 4096, C_in <= 16384, kernel <= 7 x 7 (got 8 -> 6, 1 x 1)']],
        },
        'weight/2^30': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: weight tensors of 2^30 elements or more are not supported'], [-2, 'conv: weight tensors of 2^30 elements or more are not supported']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: weight tensors of 2^30 elements or more are not supported'], [-2, 'conv: weight tensors of 2^30 elements or more are not supported']],
        },
        'weight/15*2^26': {
            'ghn3_conv_scratch_floats': [1509957696, 2516664576],
            'ghn3_conv_frozen_scratch_floats': [1509949504, 2516672768],
        },
        'relu0': {
            'ghn3_conv_scratch_floats': [7040, 8416],
            'ghn3_conv_frozen_scratch_floats': [6976, 8448],
        },
        'relu1': {
            'ghn3_conv_scratch_floats': [7040, 8416],
            'ghn3_conv_frozen_scratch_floats': [6976, 8448],
        },
        'relu2': {
            'ghn3_conv_scratch_floats': [7040, 8416],
            'ghn3_conv_frozen_scratch_floats': [6976, 8448],
        },
        'relu3': {
            'ghn3_conv_scratch_floats': [7040, 8416],
            'ghn3_conv_frozen_scratch_floats': [6976, 8448],
        },
        'bad/null': {
            'ghn3_conv_scratch_floats': [[-1, 'conv: null descriptor'], [-1, 'conv: null descriptor']],
            'ghn3_conv_frozen_scratch_floats': [[-1, 'conv: null descriptor'], [-1, 'conv: null descriptor']],
        },
        'bad/Ho_plus_1': {
            'ghn3_conv_scratch_floats': [[-1, 'conv: output size 7 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'conv: output size 7 x 6 does not match the convolution arithmetic (6 x 6)']],
            'ghn3_conv_frozen_scratch_floats': [[-1, 'conv: output size 7 x 6 does not match the convolution arithmetic (6 x 6)'], [-1, 'conv: output size 7 x 6 does not match the convolution arithmetic (6 x 6)']],
        },
        'bad/H0': {
            'ghn3_conv_scratch_floats': [[-1, 'conv: non-positive size in the descriptor'], [-1, 'conv: non-positive size in the descriptor']],
            'ghn3_conv_frozen_scratch_floats': [[-1, 'conv: non-positive size in the descriptor'], [-1, 'conv: non-positive size in the descriptor']],
        },
        'bad/stride_w0': {
            'ghn3_conv_scratch_floats': [[-1, 'conv: non-positive size in the descriptor'], [-1, 'conv: non-positive size in the descriptor']],
            'ghn3_conv_frozen_scratch_floats': [[-1, 'conv: non-positive size in the descriptor'], [-1, 'conv: non-positive size in the descriptor']],
        },
        'bad/pad_negative': {
            'ghn3_conv_scratch_floats': [[-1, 'conv: non-positive size in the descriptor'], [-1, 'conv: non-positive size in the descriptor']],
            'ghn3_conv_frozen_scratch_floats': [[-1, 'conv: non-positive size in the descriptor'], [-1, 'conv: non-positive size in the descriptor']],
        },
        '2^31/just_below': {
            'ghn3_conv_scratch_floats': [1062976, 35288144],
            'ghn3_conv_frozen_scratch_floats': [6208, 35288160],
        },
        '2^31/exactly': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: activation tensors of 2^31 elements or more are not supported'], [-2, 'conv: activation tensors of 2^31 elements or more are not supported']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: activation tensors of 2^31 elements or more are not supported'], [-2, 'conv: activation tensors of 2^31 elements or more are not supported']],
        },
        '2^31/output_only': {
            'ghn3_conv_scratch_floats': [[-2, 'conv: activation tensors of 2^31 elements or more are not supported'], [-2, 'conv: activation tensors of 2^31 elements or more are not supported']],
            'ghn3_conv_frozen_scratch_floats': [[-2, 'conv: activation tensors of 2^31 elements or more are not supported'], [-2, 'conv: activation tensors of 2^31 elements or more are not supported']],
        },
    },
    'patch': {
        'vit_16x16': {
            'ghn3_patch_scratch_floats': [0, 1179648],
        },
        'vit_16x16_nhwc': {
            'ghn3_patch_scratch_floats': [0, 1179648],
        },
        'one_chunk': {
            'ghn3_patch_scratch_floats': [0, 0],
        },
        '8x8_trailing_rows': {
            'ghn3_patch_scratch_floats': [0, 0],
        },
        'kernel_7': {
            'ghn3_patch_scratch_floats': [[-2, 'patch: needs max(kh, kw) in 8 .. 32, C_in <= 4, C_in kh kw <= 4096, C_out a multiple of 4 and <= 4096, stride >= kernel (got 3 -> 64, 7 x 7, stride 7 x 7)'], [-2, 'patch: needs max(kh, kw) in 8 .. 32, C_in <= 4, C_in kh kw <= 4096, C_out a multiple of 4 and <= 4096, stride >= kernel (got 3 -> 64, 7 x 7, stride 7 x 7)']],
        },
        'overlapping': {
            'ghn3_patch_scratch_floats': [[-2, 'patch: needs max(kh, kw) in 8 .. 32, C_in <= 4, C_in kh kw <= 4096, C_out a multiple of 4 and <= 4096, stride >= kernel (got 3 -> 64, 16 x 16, stride 8 x 8)'], [-2, 'patch: needs max(kh, kw) in 8 .. 32, C_in <= 4, C_in kh kw <= 4096, C_out a multiple of 4 and <= 4096, stride >= kernel (got 3 -> 64, 16 x 16, stride 8 x 8)']],
        },
        'bad/Ho': {
            'ghn3_patch_scratch_floats': [[-1, 'patch: output size 15 x 14 does not match the convolution arithmetic (14 x 14)'], [-1, 'patch: output size 15 x 14 does not match the convolution arithmetic (14 x 14)']],
        },
        'bad/null': {
            'ghn3_patch_scratch_floats': [[-1, 'patch: null descriptor'], [-1, 'patch: null descriptor']],
        },
    },
}

REFUSALS = {
    'ghn3_dwpw_bn_fwd/null_descriptor': [-1, 'dwpw: null descriptor'],
    'ghn3_dwpw_bn_fwd/bad_descriptor': [-1, 'dwpw: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_dwpw_bn_fwd/null_x': [-1, 'dwpw fwd: null pointer'],
    'ghn3_dwpw_bn_fwd/null_w_pw': [-1, 'dwpw fwd: null pointer'],
    'ghn3_dwpw_bn_fwd/null_gamma': [-1, 'dwpw fwd: null pointer'],
    'ghn3_dwpw_bn_fwd/null_beta': [-1, 'dwpw fwd: null pointer'],
    'ghn3_dwpw_bn_fwd/null_z': [-1, 'dwpw fwd: null pointer'],
    'ghn3_dwpw_bn_fwd/null_out': [-1, 'dwpw fwd: null pointer'],
    'ghn3_dwpw_bn_fwd/null_stats': [-1, 'dwpw fwd: null pointer'],
    'ghn3_dwpw_bn_fwd/null_scratch': [-1, 'dwpw fwd: null pointer'],
    'ghn3_dwpw_bn_fwd/no_w_dw_with_ks3': [-1, 'dwpw: without depthwise weights the op is ReLU -> 1x1 conv -> norm: ks = 1, pad = 0'],
    'ghn3_dwpw_bn_bwd/null_descriptor': [-1, 'dwpw: null descriptor'],
    'ghn3_dwpw_bn_bwd/bad_descriptor': [-1, 'dwpw: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_dwpw_bn_bwd/null_dout': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_x': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_z': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_stats': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_w_pw': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_gamma': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_dx': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_dw_pw': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_dgamma': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_dbeta': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/null_scratch': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_bn_bwd/no_w_dw_with_ks3': [-1, 'dwpw: without depthwise weights ks = 1, pad = 0'],
    'ghn3_dwpw_bn_bwd/w_dw_without_dw_dw': [-1, 'dwpw bwd: null pointer'],
    'ghn3_dwpw_plain_fwd/null_descriptor': [-1, 'dwpw: null descriptor'],
    'ghn3_dwpw_plain_fwd/bad_descriptor': [-1, 'dwpw: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_dwpw_plain_fwd/null_x': [-1, 'dwpw plain fwd: null pointer'],
    'ghn3_dwpw_plain_fwd/null_w_pw': [-1, 'dwpw plain fwd: null pointer'],
    'ghn3_dwpw_plain_fwd/null_out': [-1, 'dwpw plain fwd: null pointer'],
    'ghn3_dwpw_plain_fwd/no_w_dw_with_ks3': [-1, 'dwpw: without depthwise weights the op is ReLU -> 1x1 conv: ks = 1, pad = 0'],
    'ghn3_dwpw_plain_bwd/null_descriptor': [-1, 'dwpw: null descriptor'],
    'ghn3_dwpw_plain_bwd/bad_descriptor': [-1, 'dwpw: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_dwpw_plain_bwd/null_dout': [-1, 'dwpw plain bwd: null pointer'],
    'ghn3_dwpw_plain_bwd/null_x': [-1, 'dwpw plain bwd: null pointer'],
    'ghn3_dwpw_plain_bwd/null_w_pw': [-1, 'dwpw plain bwd: null pointer'],
    'ghn3_dwpw_plain_bwd/null_dx': [-1, 'dwpw plain bwd: null pointer'],
    'ghn3_dwpw_plain_bwd/null_dw_pw': [-1, 'dwpw plain bwd: null pointer'],
    'ghn3_dwpw_plain_bwd/null_scratch': [-1, 'dwpw plain bwd: null pointer'],
    'ghn3_dwpw_plain_bwd/no_w_dw_with_ks3': [-1, 'dwpw: without depthwise weights ks = 1, pad = 0'],
    'ghn3_dwpw_plain_bwd/w_dw_without_dw_dw': [-1, 'dwpw plain bwd: null pointer'],
    'ghn3_dwpw_frozen_fwd/null_descriptor': [-1, 'dwpw: null descriptor'],
    'ghn3_dwpw_frozen_fwd/bad_descriptor': [-1, 'dwpw: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_dwpw_frozen_fwd/null_x': [-1, 'dwpw frozen fwd: null pointer'],
    'ghn3_dwpw_frozen_fwd/null_w_pw': [-1, 'dwpw frozen fwd: null pointer'],
    'ghn3_dwpw_frozen_fwd/null_gamma': [-1, 'dwpw frozen fwd: null pointer'],
    'ghn3_dwpw_frozen_fwd/null_beta': [-1, 'dwpw frozen fwd: null pointer'],
    'ghn3_dwpw_frozen_fwd/null_mean': [-1, 'dwpw frozen fwd: null pointer'],
    'ghn3_dwpw_frozen_fwd/null_var': [-1, 'dwpw frozen fwd: null pointer'],
    'ghn3_dwpw_frozen_fwd/null_out': [-1, 'dwpw frozen fwd: null pointer'],
    'ghn3_dwpw_frozen_fwd/no_w_dw_with_ks3': [-1, 'dwpw: without depthwise weights the op is ReLU -> 1x1 conv -> norm: ks = 1, pad = 0'],
    'ghn3_dwpw_frozen_fwd/no_z_no_w_dw_with_ks3': [-1, 'dwpw: without depthwise weights the op is ReLU -> 1x1 conv -> norm: ks = 1, pad = 0'],
    'ghn3_dwpw_frozen_bwd/null_descriptor': [-1, 'dwpw: null descriptor'],
    'ghn3_dwpw_frozen_bwd/bad_descriptor': [-1, 'dwpw: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_dwpw_frozen_bwd/null_dout': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_x': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_z': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_w_pw': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_gamma': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_mean': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_var': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_dx': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_dw_pw': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_dgamma': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_dbeta': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/null_scratch': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dwpw_frozen_bwd/no_w_dw_with_ks3': [-1, 'dwpw: without depthwise weights ks = 1, pad = 0'],
    'ghn3_dwpw_frozen_bwd/w_dw_without_dw_dw': [-1, 'dwpw frozen bwd: null pointer'],
    'ghn3_dw_fwd/null_descriptor': [-1, 'dw: null descriptor'],
    'ghn3_dw_fwd/bad_descriptor': [-1, 'dw: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_dw_fwd/null_x': [-1, 'dw fwd: null pointer'],
    'ghn3_dw_fwd/null_w_dw': [-1, 'dw fwd: null pointer'],
    'ghn3_dw_fwd/null_y': [-1, 'dw fwd: null pointer'],
    'ghn3_dw_bwd/null_descriptor': [-1, 'dw: null descriptor'],
    'ghn3_dw_bwd/bad_descriptor': [-1, 'dw: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_dw_bwd/null_dout': [-1, 'dw bwd: null pointer'],
    'ghn3_dw_bwd/null_x': [-1, 'dw bwd: null pointer'],
    'ghn3_dw_bwd/null_w_dw': [-1, 'dw bwd: null pointer'],
    'ghn3_dw_bwd/null_dx': [-1, 'dw bwd: null pointer'],
    'ghn3_dw_bwd/null_dw_dw': [-1, 'dw bwd: null pointer'],
    'ghn3_dw_bwd/null_scratch': [-1, 'dw bwd: null pointer'],
    'ghn3_conv_bn_fwd/null_descriptor': [-1, 'conv: null descriptor'],
    'ghn3_conv_bn_fwd/bad_descriptor': [-1, 'conv: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_conv_bn_fwd/null_x': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/null_w': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/null_gamma': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/null_beta': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/null_z': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/null_out': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/null_stats': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/null_scratch': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/no_norm_null_x': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/no_norm_null_w': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/no_norm_null_z': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_fwd/no_norm_null_scratch': [-1, 'conv fwd: null pointer'],
    'ghn3_conv_bn_bwd/null_descriptor': [-1, 'conv: null descriptor'],
    'ghn3_conv_bn_bwd/bad_descriptor': [-1, 'conv: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_conv_bn_bwd/null_dout': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_x': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_z': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_stats': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_w': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_gamma': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_dx': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_dw': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_dgamma': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_dbeta': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/null_scratch': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/no_norm_null_dout': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/no_norm_null_x': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/no_norm_null_w': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/no_norm_null_dx': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/no_norm_null_dw': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_bn_bwd/no_norm_null_scratch': [-1, 'conv bwd: null pointer'],
    'ghn3_conv_frozen_fwd/null_descriptor': [-1, 'conv: null descriptor'],
    'ghn3_conv_frozen_fwd/bad_descriptor': [-1, 'conv: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_conv_frozen_fwd/null_x': [-1, 'conv frozen fwd: null pointer'],
    'ghn3_conv_frozen_fwd/null_w': [-1, 'conv frozen fwd: null pointer'],
    'ghn3_conv_frozen_fwd/null_gamma': [-1, 'conv frozen fwd: null pointer'],
    'ghn3_conv_frozen_fwd/null_beta': [-1, 'conv frozen fwd: null pointer'],
    'ghn3_conv_frozen_fwd/null_mean': [-1, 'conv frozen fwd: null pointer'],
    'ghn3_conv_frozen_fwd/null_var': [-1, 'conv frozen fwd: null pointer'],
    'ghn3_conv_frozen_fwd/null_out': [-1, 'conv frozen fwd: null pointer'],
    'ghn3_conv_frozen_fwd/null_scratch': [-1, 'conv frozen fwd: null pointer'],
    'ghn3_conv_frozen_fwd/no_norm_flag': [-1, 'conv frozen: GHN3_CONV_NO_NORM has no meaning here'],
    'ghn3_conv_frozen_fwd/no_norm_flag_and_null_x': [-1, 'conv frozen: GHN3_CONV_NO_NORM has no meaning here'],
    'ghn3_conv_frozen_bwd/null_descriptor': [-1, 'conv: null descriptor'],
    'ghn3_conv_frozen_bwd/bad_descriptor': [-1, 'conv: output size 6 x 4 does not match the convolution arithmetic (5 x 4)'],
    'ghn3_conv_frozen_bwd/null_dout': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_x': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_z': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_w': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_gamma': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_mean': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_var': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_dx': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_dw': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_dgamma': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_dbeta': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/null_scratch': [-1, 'conv frozen bwd: null pointer'],
    'ghn3_conv_frozen_bwd/no_norm_flag': [-1, 'conv frozen: GHN3_CONV_NO_NORM has no meaning here'],
    'ghn3_conv_frozen_bwd/no_norm_flag_and_null_x': [-1, 'conv frozen: GHN3_CONV_NO_NORM has no meaning here'],
}
