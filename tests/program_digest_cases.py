"""Every compiled Program, pinned byte for byte without a GPU (tests/test_program_digest_cpu.py).

A Program is plain host bookkeeping: its op arrays, GEMM problem table, index blob and scheduling fields are a pure function of
the batch, the arguments and the GHN3_* switches, and two compiles in separate processes give equal bytes.  CASES says which
programs are built; EXPECT holds, case by case and as literals, one short sha256 digest PER FIELD (in the order of FIELDS), so
that a failure names the field that moved.

The literals were RECORDED from the commit before Program._build_backward was cut into stage methods (the 750-line method, the
scheduling inside __init__, the attributes found with hasattr), with

    python tests/program_digest_cases.py            # prints the EXPECT table; --check compares instead

and must stay as they are when that code is reorganised: a changed literal is a changed program.  Fields that the recorded
commit only set on some programs are read through `field()` with the default its readers assumed (DEFAULTS); since the
refactor those defaults are the declared ones.

Three groups of programs, all built from Program(...) directly:
  tiny/...    the recipe cases of tests/test_program_cpu.py x operand type x side stream (training); b2 and noln once more with
              the lowered K-split threshold
  syn/...     the configurations of tests/test_gpu_configs.py on synthetic_batch(nodes, 6) x operand type x training / eval x
              side stream, and one case each for the Program arguments decoder_bwd_ctype, direct16 and graphormer_x3
  switch/...  one program per non-default switch setting, each set singly, on ghn3lm8 [33, 60] f16 (BASE; a few need another base,
              see SWITCH_BASE).  When recording, every one of them gave a digest set different from its base program's -- the
              test asserts that of the literals too.
"""
import hashlib
import os
import sys

import numpy as np

if __name__ == '__main__':
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'),
                    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]

import recipe

from ghn3_amd import Graph, GraphBatch, _lib as L
from ghn3_amd.program import Program
from ghn3_amd.synthetic import synthetic_batch

CFGS = {
    'ghn3tm8': dict(max_shape=(64, 64, 16, 16), num_classes=1000, hid=64, heads=8, layers=3),
    'ghn3lm8': dict(max_shape=(256, 256, 16, 16), num_classes=1000, hid=256, heads=16, layers=12),
    'ghn3xlm16': dict(max_shape=(384, 384, 16, 16), num_classes=1000, hid=384, heads=16, layers=24),
}                                                  # (= CFGS of tests/test_gpu_configs.py, which needs a GPU to import)
CTYPES = {'f32': None, 'f16': L.CT_F16, 'bf16': L.CT_BF16}
TINY = [('b1', 'reference'), ('b2', 'reference'), ('b2', 'correct'), ('big', 'reference'), ('big_b2', 'reference'),
        ('nonorm', 'reference'), ('noln', 'reference'), ('only1d', 'reference'), ('single', 'reference'),
        ('ragged3', 'reference'), ('ragged3', 'correct'), ('mixed1d', 'reference')]
SYN = [('ghn3tm8', (64,), 6), ('ghn3tm8', (128,), 6), ('ghn3lm8', (33, 60), 6), ('ghn3xlm16', (256,), 6),
       ('ghn3xlm16', (256, 256), 6), ('ghn3xlm16', (33, 60), 6), ('ghn3xlm16', (256,), 256000)]

# ---- what is recorded ------------------------------------------------------------------------------------------------------------
ARRAYS = ('fwd_ops', 'bwd_ops', 'shadow_ops', 'shadow_ops_rest', 'problems', 'idx_blob', 'bwd_ops_a', 'bwd_ops_b')
REPRS = ('ws_bytes', 'scal_bytes', 'ws_zero', 'ws_zero_dout', 'ddp_index', 'd16_on_idx', 'd16_off_idx', 'd16_kinds',
         'tile_bwd_op', 'tile_bwd_refs', 'tile_bwd_h16', 'memset_grad_op', 'bwd_split', 'bwd_cut_w2', 'wgrad_op_range',
         'wgrad_cap', 'wgrad_order', 'dgrad_sub', 'grad_no_memset', 'grad_sumsq', 'decoder_slots')
FIELDS = ARRAYS + ('norm_fin_ops', 'norm_ops_fwd', 'norm_ops_bwd', 'bwd_parts') + REPRS + ('tag_flops', 'route_direct',
                                                                                         'route_fp32')
# the value a reader of the recorded commit assumed where a program did not have the attribute
DEFAULTS = dict(bwd_ops_a=None, bwd_ops_b=None, bwd_parts=(), ws_zero=None, ws_zero_dout=(), ddp_index={}, d16_on_idx=[],
                d16_off_idx=[], d16_kinds={}, tile_bwd_op=None, tile_bwd_refs={}, tile_bwd_h16=0, memset_grad_op=None,
                bwd_split=None, bwd_cut_w2=None, wgrad_op_range=None, wgrad_cap=0, wgrad_order=None, dgrad_sub=None,
                grad_no_memset=[], grad_sumsq=None, decoder_slots=None)


def field(prog, name):
    return getattr(prog, name, DEFAULTS[name]) if name in DEFAULTS else getattr(prog, name)


def _h(*chunks):
    m = hashlib.sha256()
    for c in chunks:
        if isinstance(c, np.ndarray):
            m.update(('%s%s' % (c.dtype.descr if c.dtype.names else c.dtype.str, c.shape)).encode())
            m.update(np.ascontiguousarray(c).tobytes())
        else:
            m.update(repr(c).encode())
    return m.hexdigest()[:6]


def digests(prog):
    """{field: digest} of one program (FIELDS order).  The route switch is recorded last: it edits bwd_ops in place."""
    out = {}
    for name in ARRAYS:
        out[name] = _h(field(prog, name))
    out['norm_fin_ops'] = _h(prog.norm_fin_ops())
    out['norm_ops_fwd'], out['norm_ops_bwd'] = (_h(a) for a in prog.norm_ops(1.0))
    out['bwd_parts'] = _h(*[x for ops, slots in field(prog, 'bwd_parts') for x in (ops, slots)])
    for name in REPRS:
        out[name] = _h(field(prog, name))
    out['tag_flops'] = _h(sorted(prog.tag_flops.items()))
    for name, direct in (('route_direct', True), ('route_fp32', False)):
        out[name] = _h(sorted(prog.set_tile_route(direct)), prog.bwd_ops) if prog.training else _h(None)
    assert tuple(out) == FIELDS
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def _case(src, env=None, patch=None, **kw):
    return dict(src=src, kw=kw, env=env or {}, patch=patch or {})


def _syn_id(name, nodes, seed):
    return 'syn/%s/%s%s' % (name, '-'.join(str(n) for n in nodes), '' if seed == 6 else '/seed%d' % seed)


CASES = {}
for _case_name, _mode in TINY:
    for _ct in CTYPES:
        for _side in (True, False):
            CASES['tiny/%s%s/%s/%s' % (_case_name, '-correct' if _mode == 'correct' else '', _ct, 'side' if _side else 'noside')] = \
                _case(('tiny', _case_name, _mode), decoder_ctype=CTYPES[_ct], side_stream=_side)
for _case_name in ('b2', 'noln'):
    CASES['tiny/%s/f32/side/split_k2_min64' % _case_name] = _case(('tiny', _case_name, 'reference'),
                                                                  env={'GHN3_SPLIT_K2_MIN': '64'})
for _name, _nodes, _seed in SYN:
    for _ct in CTYPES:
        for _train in (True, False):
            for _side in (True, False):
                CASES['%s/%s/%s/%s' % (_syn_id(_name, _nodes, _seed), _ct, 'train' if _train else 'eval',
                                       'side' if _side else 'noside')] = \
                    _case(('syn', _name, _nodes, _seed), decoder_ctype=CTYPES[_ct], training=_train, side_stream=_side)
_LM8 = ('syn', 'ghn3lm8', (33, 60), 6)
_XL = ('syn', 'ghn3xlm16', (256,), 6)
CASES['syn/ghn3lm8/33-60/f16/train/side/bwd_bf16'] = _case(_LM8, decoder_ctype=L.CT_F16, decoder_bwd_ctype=L.CT_BF16)
CASES['syn/ghn3lm8/33-60/f16/train/side/no_direct16'] = _case(_LM8, decoder_ctype=L.CT_F16, direct16=False)
CASES['syn/ghn3lm8/33-60/f16/train/side/no_x3'] = _case(_LM8, decoder_ctype=L.CT_F16, graphormer_x3=False)

BASE = 'syn/ghn3lm8/33-60/f16/train/side'
SWITCHES = ['X3=0', 'X3S=0', 'X3_F16=0', 'P8=0', 'TILE_D16=0', 'DGRAD_PLANES=0', 'DGRAD_PIN=0', 'DGRAD_EQ=0', 'DGRAD_SUB=3,1',
            'WGRAD_MAIN=0', 'WGRAD_CAP=96', 'WGRAD_ORDER=early', 'WGRAD_LATE=0', 'WGRAD_PREP_LATE=0', 'WGRAD_TILE=30',
            'WGRAD_SUMSQ=0', 'EARLY_1D=0', 'D2_DGRAD_KS=2', 'D2_DGRAD_TILE=20', 'D1_DGRAD_TILE=64', 'D1_BWD=f16',
            'LAYER_WGRAD_DEFER=0', 'LAYER_WGRAD_GROUP=4', 'LAYER_WGRAD_TILE=64', 'LAYER_WGRAD_CAP=64', 'EMBED_BWD_MAIN=0',
            'DDP_WGRAD_FIRST=0', 'CLS_FAMILY=0', 'PAD_I8=0', 'P8_MIN_ROWS=8']
# Switches that change nothing on BASE (found when recording: its W2 weight gradient stays on the chain's stream) are set on
# ghn3xlm16 [256] instead.  Three change nothing there either when set singly and are left out: GHN3_WGRAD_ORDER=first (the
# default order), GHN3_SIDE_GROUP=2 (read only with GHN3_LAYER_WGRAD_DEFER=0) and GHN3_DGRAD_RECT=0 (the 8-phase dgrad of
# GHN3_P8 / GHN3_DGRAD_PIN takes every family the rectangular tiles would).
SWITCHES_XL = ['WGRAD_MAIN=1', 'WGRAD_ORDER=late', 'WGRAD_TPW=2']
SWITCH_BASE = dict({_sw: 'syn/ghn3xlm16/256/f16/train/side' for _sw in SWITCHES_XL},
                   **{'DGRAD_PLANES=0/f32': 'syn/ghn3lm8/33-60/f32/train/side'})
for _sw in SWITCHES + SWITCHES_XL:
    _k, _v = _sw.split('=')
    CASES['switch/' + _sw] = _case(_XL if _sw in SWITCHES_XL else _LM8, env={'GHN3_' + _k: _v}, decoder_ctype=L.CT_F16)
CASES['switch/DGRAD_PLANES=0/f32'] = _case(_LM8, env={'GHN3_DGRAD_PLANES': '0'}, decoder_ctype=None)
CASES['switch/P8_FINE=False'] = _case(_LM8, patch={'P8_FINE': False}, decoder_ctype=L.CT_F16)
CASES['switch/P8_BALANCED=False'] = _case(_LM8, patch={'P8_BALANCED': False}, decoder_ctype=L.CT_F16)


def switch_base(case):
    return SWITCH_BASE.get(case[len('switch/'):], BASE)


_BATCHES = {}


def _batch(src):
    """(Program's positional arguments, keyword arguments of the source) -- built once per source."""
    if src not in _BATCHES:
        if src[0] == 'tiny':
            case, mode = src[1:]
            over = recipe.EXTRA_CASES[case][1] if case in recipe.EXTRA_CASES else {}
            cfg = dict(recipe.TINY_CFG, **over)
            specs = recipe.edge_specs(case) if case in recipe.EDGE_CASES else \
                recipe.EXTRA_CASES[case][0] if case in recipe.EXTRA_CASES else [recipe.TINY_NETS[i] for i in recipe.TINY_CASES[case]]
            nets = [recipe.build_torch_net(s) for s in specs]
            graphs = []
            for s in specs:
                nf, info, A = recipe.graph_arrays(s)
                graphs.append(Graph(node_feat=nf, node_info=info, A=A))
            gb = GraphBatch(graphs, dense=True)
            kw = dict(index_mode=mode, layernorm=cfg['layernorm'], weight_norm=cfg['weight_norm'])
        else:
            cfg = CFGS[src[1]]
            gb, nets = synthetic_batch(list(src[2]), src[3])
            kw = {}
        gb._cat()
        pcfg = {k: cfg[k] for k in ('hid', 'heads', 'layers', 'num_classes', 'max_shape')}
        _BATCHES[src] = ((pcfg, gb.node_info, gb.host_n_nodes(), gb._node_type_host, gb.max_edge, nets), kw)
    return _BATCHES[src]


def build(name, setenv, setattr_):
    """Compiles the program of CASES[name]; setenv(key, value) and setattr_(obj, attr, value) are the caller's (undoable)
    ways to set a switch -- the caller has removed every GHN3_* variable before."""
    spec = CASES[name]
    args, kw = _batch(spec['src'])
    for k, v in spec['env'].items():
        setenv(k, v)
    for k, v in spec['patch'].items():
        setattr_(Program, k, v)
    return Program(*args, **dict(kw, **spec['kw']))


def _record(check):
    import time
    for k in [k for k in os.environ if k.startswith('GHN3_')]:
        del os.environ[k]
    t0, got = time.time(), {}
    for name, spec in CASES.items():
        saved = {k: getattr(Program, k) for k in spec['patch']}
        got[name] = ' '.join(digests(build(name, os.environ.__setitem__, setattr)).values())
        for k in spec['env']:
            del os.environ[k]
        for k, v in saved.items():
            setattr(Program, k, v)
    if check:
        bad = [n for n in CASES if got[n] != EXPECT.get(n)]
        for n in bad:
            print(n, [f for f, a, b in zip(FIELDS, got[n].split(), EXPECT.get(n, '').split() or [''] * len(FIELDS)) if a != b])
        print('%d programs, %d differ, %.1f s' % (len(CASES), len(bad), time.time() - t0))
        return
    same = [n for n in CASES if n.startswith('switch/') and got[n] == got[switch_base(n)]]
    print('EXPECT = {')
    for name in CASES:
        print('    %r:\n        %r,' % (name, got[name]))
    print('}')
    print('# %d programs in %.1f s; switch cases equal to their base: %s' % (len(CASES), time.time() - t0, same), file=sys.stderr)


EXPECT = {
    'tiny/b1/f32/side':
        '94e516 783c22 860050 860050 f687da 94560a adb85a 1a6a2c ab888b a63931 8eebd7 ba2b89 c0298f 68f10b dc937b 86362a 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 59e197 c23560 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 5ce275 76cc19 76cc19',
    'tiny/b1/f32/noside':
        'd4a615 c66b80 860050 860050 8a561d 8bfce8 77fb8f 275745 ab888b a63931 8eebd7 997719 85346c 68f10b dc937b 86362a 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 670671 452354 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 5ce275 9e0d0e 9e0d0e',
    'tiny/b1/f16/side':
        'efc016 6e701e 6fe941 689975 dab091 db36df 507583 1699ff a1ade1 b6e98f de58f1 c7238d 8e9039 68f10b f7f066 3ba3a2 ed988f 73731e 6b5d1a 6825ab 4e0740 fb4b70 72bdf4 5feceb eb1e33 535fa3 7ebfd4 5feceb 5e032c 28cb03 042ed9 449df9 66ba7e 13d177 cb6119 163ad2',
    'tiny/b1/f16/noside':
        'e2b93f 38f5ec adc823 77d435 c1c557 e4e8e6 791c59 df451e a1ade1 b6e98f de58f1 4ac011 bdd8b5 68f10b 2db563 3ba3a2 1387cc 14ec8c 9ca282 7810b7 4e0740 fb4b70 72bdf4 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 28cb03 042ed9 5e261b 66ba7e 13d177 1c6d00 9713d4',
    'tiny/b1/bf16/side':
        '3c1a74 1c7785 6fe941 689975 2de45e b1d5ea 40e88d 396af6 a1ade1 b6e98f de58f1 78cf80 8e9039 68f10b f7f066 3ba3a2 a59fd9 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a 6f4b66 08c31f 5feceb 5e032c 28cb03 042ed9 449df9 66ba7e 13d177 c52f30 c52f30',
    'tiny/b1/bf16/noside':
        '67e021 23c598 adc823 77d435 11a159 814268 890c8e a78d51 a1ade1 b6e98f de58f1 cc8457 bdd8b5 68f10b 2db563 3ba3a2 9822a2 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 59e197 8527a8 a4b127 5feceb 5b7c47 28cb03 042ed9 5e261b 66ba7e 13d177 a45488 a45488',
    'tiny/b2/f32/side':
        'e7dcd4 042a2b 860050 860050 b6273c a5b119 60f432 0d3578 13f8be e44dab 58e7b4 46e3e9 3a6518 5e74cb dc937b cfccf3 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a b7a568 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 17a55f 29de88 29de88',
    'tiny/b2/f32/noside':
        'e2ef14 123a49 860050 860050 5545bd dbc753 df10f1 5a8152 13f8be e44dab 58e7b4 4a66a0 0bffbd 5e74cb dc937b cfccf3 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 59e197 4ec959 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 17a55f da0701 da0701',
    'tiny/b2/f16/side':
        '8a303a 331288 6fe941 689975 5d7872 717bff d56b2e a4c2d3 c88b9b 128e6f 21bb45 f9625f ad05a5 5e74cb c82b74 5ef47a 4b1374 2513f6 73731e 6504a9 4e0740 fb4b70 24f4c4 5feceb e29c9c c23560 0a93af 5feceb 5e032c 28cb03 042ed9 34c290 66ba7e fb10ed 513040 bd1ca1',
    'tiny/b2/f16/noside':
        '4bbab9 747ef5 adc823 77d435 e7495c 22cf30 0dfda8 582bff c88b9b 128e6f 21bb45 256638 8fce45 5e74cb 6e4015 5ef47a 4cc2cf db3de1 14ec8c 2730d8 4e0740 fb4b70 24f4c4 5feceb eb1e33 452354 115aa7 5feceb 5b7c47 28cb03 042ed9 9096b6 66ba7e fb10ed a72588 e5f3b4',
    'tiny/b2/bf16/side':
        '13b2fa a2547f 6fe941 689975 8c6883 c01c8f 3f3e4c b61d40 c88b9b 128e6f 21bb45 c775ef ad05a5 5e74cb c82b74 5ef47a 222997 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 624b60 785f3e f1c775 5feceb 5e032c 28cb03 042ed9 34c290 66ba7e fb10ed 3e7b7a 3e7b7a',
    'tiny/b2/bf16/noside':
        'c75d6e d916e9 adc823 77d435 8d1a2f 03838d 6fd918 5e1d89 c88b9b 128e6f 21bb45 4f9095 8fce45 5e74cb 6e4015 5ef47a 215fbe 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a e629fa a7d54b 5feceb 5b7c47 28cb03 042ed9 9096b6 66ba7e fb10ed 221a6f 221a6f',
    'tiny/b2-correct/f32/side':
        'e7dcd4 042a2b 860050 860050 b6273c a380a9 60f432 0d3578 13f8be e44dab 58e7b4 46e3e9 3a6518 5e74cb dc937b cfccf3 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a b7a568 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 17a55f 29de88 29de88',
    'tiny/b2-correct/f32/noside':
        'e2ef14 123a49 860050 860050 5545bd a20411 df10f1 5a8152 13f8be e44dab 58e7b4 4a66a0 0bffbd 5e74cb dc937b cfccf3 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 59e197 4ec959 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 17a55f da0701 da0701',
    'tiny/b2-correct/f16/side':
        '8a303a 331288 6fe941 689975 5d7872 cc038c d56b2e a4c2d3 c88b9b 128e6f 21bb45 f9625f ad05a5 5e74cb c82b74 5ef47a 4b1374 2513f6 73731e 6504a9 4e0740 fb4b70 24f4c4 5feceb e29c9c c23560 0a93af 5feceb 5e032c 28cb03 042ed9 34c290 66ba7e fb10ed 513040 bd1ca1',
    'tiny/b2-correct/f16/noside':
        '4bbab9 747ef5 adc823 77d435 e7495c 06324b 0dfda8 582bff c88b9b 128e6f 21bb45 256638 8fce45 5e74cb 6e4015 5ef47a 4cc2cf db3de1 14ec8c 2730d8 4e0740 fb4b70 24f4c4 5feceb eb1e33 452354 115aa7 5feceb 5b7c47 28cb03 042ed9 9096b6 66ba7e fb10ed a72588 e5f3b4',
    'tiny/b2-correct/bf16/side':
        '13b2fa a2547f 6fe941 689975 8c6883 a4171b 3f3e4c b61d40 c88b9b 128e6f 21bb45 c775ef ad05a5 5e74cb c82b74 5ef47a 222997 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 624b60 785f3e f1c775 5feceb 5e032c 28cb03 042ed9 34c290 66ba7e fb10ed 3e7b7a 3e7b7a',
    'tiny/b2-correct/bf16/noside':
        'c75d6e d916e9 adc823 77d435 8d1a2f 0b6e8d 6fd918 5e1d89 c88b9b 128e6f 21bb45 4f9095 8fce45 5e74cb 6e4015 5ef47a 215fbe 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a e629fa a7d54b 5feceb 5b7c47 28cb03 042ed9 9096b6 66ba7e fb10ed 221a6f 221a6f',
    'tiny/big/f32/side':
        '284217 14367d 860050 860050 a69d49 37eb03 a9576d 0096f1 734611 ac2b40 b0c3b5 c72d6d 97ceb2 1e5ee5 dc937b 708585 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb b7a568 6f4b66 dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e eb0c9c 4c798b 4c798b',
    'tiny/big/f32/noside':
        '86c67f e8a165 860050 860050 0a0acd f0ce98 39b7b5 f7f649 734611 ac2b40 b0c3b5 8e2349 2d59eb 1e5ee5 dc937b 708585 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb c23560 8527a8 dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e eb0c9c 25e152 25e152',
    'tiny/big/f16/side':
        'c04986 8e9134 6fe941 689975 1d1138 7bf98a 038996 5fd46e faa06a a81f15 d7ec81 d7bca8 8e8219 1e5ee5 b1208c e0851c 4b1374 2513f6 73731e 6504a9 4e0740 fb4b70 045784 5feceb e29c9c c23560 0a93af 5feceb 5e032c 28cb03 042ed9 005e4a 66ba7e e69461 efc323 48ba0a',
    'tiny/big/f16/noside':
        'c929d9 da2b16 adc823 77d435 09a87f 87eeda 464522 cfc794 faa06a a81f15 d7ec81 ce5fcd f4ee7d 1e5ee5 675d95 e0851c 4cc2cf db3de1 14ec8c 2730d8 4e0740 fb4b70 045784 5feceb eb1e33 452354 115aa7 5feceb 5b7c47 28cb03 042ed9 29f33b 66ba7e e69461 f153c5 934540',
    'tiny/big/bf16/side':
        'fb2962 cd6876 6fe941 689975 638912 27e74d 497494 f96403 faa06a a81f15 d7ec81 3c4b6b 8e8219 1e5ee5 b1208c e0851c 222997 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 624b60 785f3e f1c775 5feceb 5e032c 28cb03 042ed9 005e4a 66ba7e e69461 2e0884 2e0884',
    'tiny/big/bf16/noside':
        'ba2115 b8dbc1 adc823 77d435 5ad8d8 cda4b2 4d0e75 cef900 faa06a a81f15 d7ec81 765a4e f4ee7d 1e5ee5 675d95 e0851c 215fbe 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a e629fa a7d54b 5feceb 5b7c47 28cb03 042ed9 29f33b 66ba7e e69461 78a5c9 78a5c9',
    'tiny/big_b2/f32/side':
        '1306c9 a71457 860050 860050 ca9b94 b59288 9e2470 55920b 743ebd 4e5930 b96bfc dac094 b7f3fe ecac90 dc937b 2c08e5 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 670671 535fa3 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 898a5e fa6189 fa6189',
    'tiny/big_b2/f32/noside':
        '5977d9 d226cf 860050 860050 a16dae 1a329d 2d5b1d b19a12 743ebd 4e5930 b96bfc bfa971 55f6ab ecac90 dc937b 2c08e5 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 5f9c4a b17ef6 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 898a5e 9d4a65 9d4a65',
    'tiny/big_b2/f16/side':
        'bdc717 ec7bd4 6fe941 689975 a1f457 1e12e3 a5e1d5 c3726c 41cecf d97ff4 c5c4d5 36a5d7 bfb420 ecac90 649a1f 42f344 2208c8 af3e2c 2513f6 7be10e 4e0740 fb4b70 03ca1c 5feceb c6f3ac b7a568 7280b3 5feceb 5e032c 28cb03 042ed9 4c1301 66ba7e c1189d b0c786 eec1fa',
    'tiny/big_b2/f16/noside':
        'f91f15 001e2f adc823 77d435 7f720a 1ab8ef b304dc 2aa2e2 41cecf d97ff4 c5c4d5 abcb67 540ff8 ecac90 2befb0 42f344 a71412 8069a9 db3de1 2550f1 4e0740 fb4b70 03ca1c 5feceb e29c9c 4ec959 84f851 5feceb 5b7c47 28cb03 042ed9 e9e861 66ba7e c1189d 990091 6966d8',
    'tiny/big_b2/bf16/side':
        '6d1c86 bbcf9e 6fe941 689975 fd6ad0 6693c4 dc7c9b 2b00d0 41cecf d97ff4 c5c4d5 4f72bd bfb420 ecac90 649a1f 42f344 07b63a 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb eb1e33 535fa3 7ebfd4 5feceb 5e032c 28cb03 042ed9 4c1301 66ba7e c1189d 80bde1 80bde1',
    'tiny/big_b2/bf16/noside':
        'a38d40 686f08 adc823 77d435 b67749 871d6e 04fd48 03c20d 41cecf d97ff4 c5c4d5 a54174 540ff8 ecac90 2befb0 42f344 7bff4d 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 28cb03 042ed9 e9e861 66ba7e c1189d d639b8 d639b8',
    'tiny/nonorm/f32/side':
        '94e516 783c22 860050 860050 f687da bee96a adb85a 1a6a2c ab888b a63931 8eebd7 ba2b89 c0298f 68f10b dc937b 86362a 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 59e197 c23560 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 5ce275 76cc19 76cc19',
    'tiny/nonorm/f32/noside':
        'd4a615 c66b80 860050 860050 8a561d 3a98d5 77fb8f 275745 ab888b a63931 8eebd7 997719 85346c 68f10b dc937b 86362a 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 670671 452354 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 5ce275 9e0d0e 9e0d0e',
    'tiny/nonorm/f16/side':
        'efc016 6e701e 6fe941 689975 dab091 5a26ca 507583 1699ff a1ade1 b6e98f de58f1 c7238d 8e9039 68f10b f7f066 3ba3a2 ed988f 73731e 6b5d1a 6825ab 4e0740 fb4b70 72bdf4 5feceb eb1e33 535fa3 7ebfd4 5feceb 5e032c 28cb03 042ed9 449df9 66ba7e 13d177 cb6119 163ad2',
    'tiny/nonorm/f16/noside':
        'e2b93f 38f5ec adc823 77d435 c1c557 6e95d6 791c59 df451e a1ade1 b6e98f de58f1 4ac011 bdd8b5 68f10b 2db563 3ba3a2 1387cc 14ec8c 9ca282 7810b7 4e0740 fb4b70 72bdf4 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 28cb03 042ed9 5e261b 66ba7e 13d177 1c6d00 9713d4',
    'tiny/nonorm/bf16/side':
        '3c1a74 1c7785 6fe941 689975 2de45e b18ce1 40e88d 396af6 a1ade1 b6e98f de58f1 78cf80 8e9039 68f10b f7f066 3ba3a2 a59fd9 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a 6f4b66 08c31f 5feceb 5e032c 28cb03 042ed9 449df9 66ba7e 13d177 c52f30 c52f30',
    'tiny/nonorm/bf16/noside':
        '67e021 23c598 adc823 77d435 11a159 40db45 890c8e a78d51 a1ade1 b6e98f de58f1 cc8457 bdd8b5 68f10b 2db563 3ba3a2 9822a2 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 59e197 8527a8 a4b127 5feceb 5b7c47 28cb03 042ed9 5e261b 66ba7e 13d177 a45488 a45488',
    'tiny/noln/f32/side':
        '327275 347519 860050 860050 52bf58 94560a 6c9a73 b58758 5c6b4e 5f0cf2 d9cc22 944a23 c0298f 68f10b dc937b 86362a 44136f 4f53cd 4f53cd 44136f 4e0740 a9ecca 5feceb 5feceb 59e197 c23560 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b a5b221 5ce275 98aae5 98aae5',
    'tiny/noln/f32/noside':
        'e496f1 b9d048 860050 860050 659bf0 8bfce8 f67b77 11507d 5c6b4e 5f0cf2 d9cc22 f33940 85346c 68f10b dc937b 86362a 44136f 4f53cd 4f53cd 44136f 4e0740 a9ecca 5feceb 5feceb 670671 452354 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b a5b221 5ce275 a8eed5 a8eed5',
    'tiny/noln/f16/side':
        'feaf80 f6048f 02d26d fc9313 aaa23a db36df 3c080a 30a70c 4e4e47 def5cb 4578ee 832a0f 8e9039 68f10b f7f066 3ba3a2 ed988f 73731e 6b5d1a 6825ab 4e0740 a9ecca 72bdf4 5feceb eb1e33 535fa3 7ebfd4 5feceb 5e032c 28cb03 042ed9 449df9 a5b221 13d177 1595f8 53fb6e',
    'tiny/noln/f16/noside':
        '703035 bcbcd2 c28e08 da1256 927bcf e4e8e6 f42753 ef529f 4e4e47 def5cb 4578ee 528b22 bdd8b5 68f10b 2db563 3ba3a2 1387cc 14ec8c 9ca282 7810b7 4e0740 a9ecca 72bdf4 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 28cb03 042ed9 5e261b a5b221 13d177 0f31ea 7db87e',
    'tiny/noln/bf16/side':
        '58eba8 1e1e17 02d26d fc9313 524f10 b1d5ea 874ec9 62953d 4e4e47 def5cb 4578ee 2bf318 8e9039 68f10b f7f066 3ba3a2 a59fd9 4f53cd 4f53cd 44136f 4e0740 a9ecca 5feceb 5feceb 35135a 6f4b66 08c31f 5feceb 5e032c 28cb03 042ed9 449df9 a5b221 13d177 a8f6af a8f6af',
    'tiny/noln/bf16/noside':
        '5cf581 e8bbfd c28e08 da1256 a1f13b 814268 8773b0 820d4c 4e4e47 def5cb 4578ee 9bbcab bdd8b5 68f10b 2db563 3ba3a2 9822a2 4f53cd 4f53cd 44136f 4e0740 a9ecca 5feceb 5feceb 59e197 8527a8 a4b127 5feceb 5b7c47 28cb03 042ed9 5e261b a5b221 13d177 3e2d60 3e2d60',
    'tiny/only1d/f32/side':
        '1aaab2 fb54d8 860050 860050 dc0205 c98883 d5ab53 10eda4 ab9bdf a9d282 85ced9 bff7b1 35571d 67e0bd dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 2c6242 5feceb dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 4f53cd bed15e bed15e',
    'tiny/only1d/f32/noside':
        '135300 ea24f9 860050 860050 9ccded 0e6bc5 04984c 950d9e ab9bdf a9d282 85ced9 455261 3eb892 67e0bd dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 2c6242 5feceb dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 4f53cd 69c5f2 69c5f2',
    'tiny/only1d/f16/side':
        '1aaab2 fb54d8 860050 860050 dc0205 c98883 d5ab53 10eda4 ab9bdf a9d282 85ced9 bff7b1 35571d 67e0bd dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 2c6242 5feceb dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 4f53cd bed15e bed15e',
    'tiny/only1d/f16/noside':
        '135300 ea24f9 860050 860050 9ccded 0e6bc5 04984c 950d9e ab9bdf a9d282 85ced9 455261 3eb892 67e0bd dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 2c6242 5feceb dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 4f53cd 69c5f2 69c5f2',
    'tiny/only1d/bf16/side':
        '1aaab2 5d2510 860050 860050 dc0205 c98883 d6f3cd 10eda4 ab9bdf a9d282 85ced9 599ffe 35571d 67e0bd dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 2c6242 5feceb dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 4f53cd a4d175 a4d175',
    'tiny/only1d/bf16/noside':
        '135300 cedf79 860050 860050 9ccded 0e6bc5 0d7aff 950d9e ab9bdf a9d282 85ced9 e7db6e 3eb892 67e0bd dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 2c6242 5feceb dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 4f53cd e535c2 e535c2',
    'tiny/single/f32/side':
        '3e97f3 29fe39 860050 860050 e27476 9c0510 1ac1f4 1d4cde 6e7b77 0abe8e 5782b1 37775b 1b965d 3c1b70 dc937b 47d8e6 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 8527a8 4a44dc dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 9754c1 2f959b 2f959b',
    'tiny/single/f32/noside':
        '98cb9d 8a6d71 860050 860050 9d9b3a b8357e c16d09 4f0936 6e7b77 0abe8e 5782b1 696794 57f132 3c1b70 dc937b 47d8e6 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 8527a8 4a44dc dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 9754c1 8809e0 8809e0',
    'tiny/single/f16/side':
        'fa7b7b db722f 860050 860050 ec7d74 9c0510 164a5d 1d4cde 6e7b77 0abe8e 5782b1 b55db6 1b965d 3c1b70 dc937b 47d8e6 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 8527a8 4a44dc dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 9754c1 65c9bc 65c9bc',
    'tiny/single/f16/noside':
        '9b0b6a dc377d 860050 860050 f303fa b8357e 2f4d89 4f0936 6e7b77 0abe8e 5782b1 8f83eb 57f132 3c1b70 dc937b 47d8e6 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 8527a8 4a44dc dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 9754c1 d86d7c d86d7c',
    'tiny/single/bf16/side':
        '4bf90e d9e2cd 860050 860050 ec7d74 9c0510 ee121c 1d4cde 6e7b77 0abe8e 5782b1 8204ef 1b965d 3c1b70 dc937b 47d8e6 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 8527a8 4a44dc dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 9754c1 d2340a d2340a',
    'tiny/single/bf16/noside':
        '10bc68 2b51ce 860050 860050 f303fa b8357e 7a55fe 4f0936 6e7b77 0abe8e 5782b1 cbe872 57f132 3c1b70 dc937b 47d8e6 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 8527a8 4a44dc dc937b 5feceb 5b7c47 dc937b 4f53cd dc937b 66ba7e 9754c1 7502f7 7502f7',
    'tiny/ragged3/f32/side':
        '286485 39efff 860050 860050 576a07 b6ffc8 3739b3 e2d041 00b9db ff595a a1df0d 05e384 de6d81 f3457d dc937b 05a8bc 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb c6f3ac 35135a dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e c72e14 d79fbb d79fbb',
    'tiny/ragged3/f32/noside':
        '9d4475 1aec0b 860050 860050 f4cb9d e4e0c2 da73e6 1e58ee 00b9db ff595a a1df0d 7315ce 8c1b48 f3457d dc937b 05a8bc 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb e29c9c 785f3e dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e c72e14 e3101c e3101c',
    'tiny/ragged3/f16/side':
        '351145 a974bf 6fe941 689975 fad355 fe4f31 bb89da 32b8b9 0bf8e7 200192 778daa e8d489 13f08d f3457d 1799ee dbdf49 766663 82dd34 c873e1 499365 4e0740 fb4b70 4f3adc 5feceb 9f1402 670671 0df77b 5feceb 5e032c 28cb03 042ed9 dc937b 66ba7e ce7e01 b384f1 6c5e15',
    'tiny/ragged3/f16/noside':
        '5500de 0c6bac adc823 77d435 c2d080 165a9a 498361 b3dc56 0bf8e7 200192 778daa bb98f0 9ac734 f3457d 185feb dbdf49 640825 02bf0b 9cb9ea 98c1b0 4e0740 fb4b70 4f3adc 5feceb 86e501 f5ca38 d09954 5feceb 5b7c47 28cb03 042ed9 dc937b 66ba7e ce7e01 862a2d d98df6',
    'tiny/ragged3/bf16/side':
        'a407c3 d24633 6fe941 689975 1242af 4534d7 36ff7b 0a08db 0bf8e7 200192 778daa 5c1661 13f08d f3457d 1799ee dbdf49 a8e569 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb c6f3ac b7a568 7280b3 5feceb 5e032c 28cb03 042ed9 dc937b 66ba7e ce7e01 faad24 faad24',
    'tiny/ragged3/bf16/noside':
        '0abd62 b8a667 adc823 77d435 a993d9 3af974 076569 f89ee2 0bf8e7 200192 778daa 9027b9 9ac734 f3457d 185feb dbdf49 ad871a 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb e29c9c 4ec959 84f851 5feceb 5b7c47 28cb03 042ed9 dc937b 66ba7e ce7e01 568883 568883',
    'tiny/ragged3-correct/f32/side':
        '286485 39efff 860050 860050 576a07 3bf3bc 3739b3 e2d041 00b9db ff595a a1df0d 05e384 de6d81 f3457d dc937b 05a8bc 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb c6f3ac 35135a dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e c72e14 d79fbb d79fbb',
    'tiny/ragged3-correct/f32/noside':
        '9d4475 1aec0b 860050 860050 f4cb9d 75bfae da73e6 1e58ee 00b9db ff595a a1df0d 7315ce 8c1b48 f3457d dc937b 05a8bc 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb e29c9c 785f3e dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e c72e14 e3101c e3101c',
    'tiny/ragged3-correct/f16/side':
        '351145 a974bf 6fe941 689975 fad355 b62a7e bb89da 32b8b9 0bf8e7 200192 778daa e8d489 13f08d f3457d 1799ee dbdf49 766663 82dd34 c873e1 499365 4e0740 fb4b70 4f3adc 5feceb 9f1402 670671 0df77b 5feceb 5e032c 28cb03 042ed9 dc937b 66ba7e ce7e01 b384f1 6c5e15',
    'tiny/ragged3-correct/f16/noside':
        '5500de 0c6bac adc823 77d435 c2d080 2e4dbc 498361 b3dc56 0bf8e7 200192 778daa bb98f0 9ac734 f3457d 185feb dbdf49 640825 02bf0b 9cb9ea 98c1b0 4e0740 fb4b70 4f3adc 5feceb 86e501 f5ca38 d09954 5feceb 5b7c47 28cb03 042ed9 dc937b 66ba7e ce7e01 862a2d d98df6',
    'tiny/ragged3-correct/bf16/side':
        'a407c3 d24633 6fe941 689975 1242af 689100 36ff7b 0a08db 0bf8e7 200192 778daa 5c1661 13f08d f3457d 1799ee dbdf49 a8e569 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb c6f3ac b7a568 7280b3 5feceb 5e032c 28cb03 042ed9 dc937b 66ba7e ce7e01 faad24 faad24',
    'tiny/ragged3-correct/bf16/noside':
        '0abd62 b8a667 adc823 77d435 a993d9 994770 076569 f89ee2 0bf8e7 200192 778daa 9027b9 9ac734 f3457d 185feb dbdf49 ad871a 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb e29c9c 4ec959 84f851 5feceb 5b7c47 28cb03 042ed9 dc937b 66ba7e ce7e01 568883 568883',
    'tiny/mixed1d/f32/side':
        '1c6144 923240 860050 860050 674079 3cba58 e71c58 53a767 5cf63c d5d7e3 430d4e 3b2bc0 20a334 549a2f dc937b 8feefb 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 535fa3 9400f1 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 05f1d6 de16dd de16dd',
    'tiny/mixed1d/f32/noside':
        'cd26f2 2dd95f 860050 860050 380f52 08d5af be6cce 2d1ef4 5cf63c d5d7e3 430d4e bd2b1d 8f0c89 549a2f dc937b 8feefb 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 785f3e 6b51d4 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 05f1d6 ecfaa1 ecfaa1',
    'tiny/mixed1d/f16/side':
        '102a60 12fbf1 6fe941 689975 9f463f abc4f9 b4a8d7 397b31 498f87 2d8234 6eaf99 ad64ac e39794 549a2f e3c032 e9c0a7 ed988f 73731e 6b5d1a 6825ab 4e0740 fb4b70 da2ada 5feceb eb1e33 535fa3 7ebfd4 5feceb 5e032c 28cb03 042ed9 8b5a61 66ba7e 8da77a 73e504 a43580',
    'tiny/mixed1d/f16/noside':
        'ea41c4 081bb7 adc823 77d435 d977bc 60620b 65e038 dcf7ef 498f87 2d8234 6eaf99 81611c e6aaac 549a2f a24e6d e9c0a7 1387cc 14ec8c 9ca282 7810b7 4e0740 fb4b70 da2ada 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 28cb03 042ed9 0dc667 66ba7e 8da77a 5b9a00 cda20c',
    'tiny/mixed1d/bf16/side':
        '4ac65e b2b408 6fe941 689975 be38cd d88755 47d015 5a8d54 498f87 2d8234 6eaf99 634848 e39794 549a2f e3c032 e9c0a7 a59fd9 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a 6f4b66 08c31f 5feceb 5e032c 28cb03 042ed9 8b5a61 66ba7e 8da77a 17736b 17736b',
    'tiny/mixed1d/bf16/noside':
        'dc8132 e0693e adc823 77d435 0665f0 9a2962 1c4f6f b8b775 498f87 2d8234 6eaf99 34ecf0 e6aaac 549a2f a24e6d e9c0a7 9822a2 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 59e197 8527a8 a4b127 5feceb 5b7c47 28cb03 042ed9 0dc667 66ba7e 8da77a f154fa f154fa',
    'tiny/b2/f32/side/split_k2_min64':
        '28a67a e78a42 860050 860050 dd5a22 0bb3c3 321a95 ac7545 201cce e44dab 58e7b4 1a0a51 4fb918 5e74cb dc937b bc798a 44136f 4f53cd 4f53cd 44136f 4e0740 fb4b70 5feceb 5feceb 35135a b7a568 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 17a55f acb9a0 acb9a0',
    'tiny/noln/f32/side/split_k2_min64':
        'fdae82 56567b 860050 860050 48cdd2 a560a2 053bf2 7b394c a14b0c 5f0cf2 d9cc22 81ea42 fe08dc 68f10b dc937b 761199 44136f 4f53cd 4f53cd 44136f 4e0740 a9ecca 5feceb 5feceb 59e197 c23560 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b a5b221 5ce275 ce589d ce589d',
    'syn/ghn3tm8/64/f32/train/side':
        'dd0872 b8a986 860050 860050 8f007f 07c833 d106fb 9d61fc 30fa83 e9cd7f 7b4888 abb259 047825 3b5bec dc937b d5153d 44136f 4f53cd 4f53cd 44136f 4e0740 b2e89f 5feceb 5feceb 535fa3 9400f1 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 923705 632463 632463',
    'syn/ghn3tm8/64/f32/train/noside':
        '98d8a2 3b0ba4 860050 860050 ed1a76 a40647 93208c 7e960c 30fa83 e9cd7f 7b4888 1931f7 4a7bb7 3b5bec dc937b d5153d 44136f 4f53cd 4f53cd 44136f 4e0740 b2e89f 5feceb 5feceb 785f3e 6b51d4 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 923705 175263 175263',
    'syn/ghn3tm8/64/f32/eval/side':
        'a7f127 860050 860050 860050 49800c 4d15c4 dc937b dc937b 47ebd0 e9cd7f 7b4888 e3b0c4 9144ae 3b5bec dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b b82d8d dc937b dc937b',
    'syn/ghn3tm8/64/f32/eval/noside':
        '966a03 860050 860050 860050 49800c 4d15c4 dc937b dc937b 47ebd0 e9cd7f 7b4888 e3b0c4 9144ae 3b5bec dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b b82d8d dc937b dc937b',
    'syn/ghn3tm8/64/f16/train/side':
        'c9a81e 1a8d13 46c2cc e2b9f5 08bef5 e7b74e a30b6c bb7cc1 c74abe bceab4 ac2bb0 344d9f bc36de 3b5bec b06666 4b9672 ed988f 73731e 6b5d1a 6825ab 4e0740 b2e89f c39b45 5feceb eb1e33 535fa3 7ebfd4 5feceb 5e032c 28cb03 042ed9 24075b 66ba7e b84e07 37b8f4 09b249',
    'syn/ghn3tm8/64/f16/train/noside':
        '9150d9 319e87 03fad2 7c64ad e7dbc2 63486e d6a0da 6c9ce6 c74abe bceab4 ac2bb0 e0c77b d4baf9 3b5bec 5296d1 4b9672 1387cc 14ec8c 9ca282 7810b7 4e0740 b2e89f c39b45 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 28cb03 042ed9 d1074e 66ba7e b84e07 d427cd 5d060c',
    'syn/ghn3tm8/64/f16/eval/side':
        '893349 860050 e2f625 d39e26 85dbd0 1bbeb5 dc937b dc937b 47ebd0 598e00 cdb91f e3b0c4 56dd17 3b5bec 0f4f8f 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b a08483 dc937b dc937b',
    'syn/ghn3tm8/64/f16/eval/noside':
        '805d2d 860050 14622a 144326 85dbd0 1bbeb5 dc937b dc937b 47ebd0 598e00 cdb91f e3b0c4 56dd17 3b5bec 0f4f8f 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b a08483 dc937b dc937b',
    'syn/ghn3tm8/64/bf16/train/side':
        'a7ca8c 6b4dd2 46c2cc e2b9f5 637702 06fa5c a69546 7f5f49 c74abe bceab4 ac2bb0 a781c5 bc36de 3b5bec b06666 4b9672 a59fd9 4f53cd 4f53cd 44136f 4e0740 b2e89f 5feceb 5feceb 35135a 6f4b66 08c31f 5feceb 5e032c 28cb03 042ed9 24075b 66ba7e b84e07 39ca06 39ca06',
    'syn/ghn3tm8/64/bf16/train/noside':
        '9ae3f7 160cf9 03fad2 7c64ad d7fd06 9f357d a5b41d f3f820 c74abe bceab4 ac2bb0 eab65d d4baf9 3b5bec 5296d1 4b9672 9822a2 4f53cd 4f53cd 44136f 4e0740 b2e89f 5feceb 5feceb 59e197 8527a8 a4b127 5feceb 5b7c47 28cb03 042ed9 d1074e 66ba7e b84e07 e157db e157db',
    'syn/ghn3tm8/64/bf16/eval/side':
        '64d74e 860050 e2f625 d39e26 85dbd0 480564 dc937b dc937b 47ebd0 598e00 cdb91f e3b0c4 56dd17 3b5bec 0f4f8f 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b a08483 dc937b dc937b',
    'syn/ghn3tm8/64/bf16/eval/noside':
        'a813da 860050 14622a 144326 85dbd0 480564 dc937b dc937b 47ebd0 598e00 cdb91f e3b0c4 56dd17 3b5bec 0f4f8f 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b a08483 dc937b dc937b',
    'syn/ghn3tm8/128/f32/train/side':
        'da8a00 67ba2e 860050 860050 84d43e 96a216 11b4cc 5a650c b4e058 7b3aba fcccb7 d92e7e cc3dae 2464d5 dc937b 3300f6 44136f 4f53cd 4f53cd 44136f 4e0740 b2e89f 5feceb 5feceb 535fa3 9400f1 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e fffc38 23ae0a 23ae0a',
    'syn/ghn3tm8/128/f32/train/noside':
        'c12704 6ac90f 860050 860050 c34fd7 23e91a 514baa ae864c b4e058 7b3aba fcccb7 8692b6 dea56b 2464d5 dc937b 3300f6 44136f 4f53cd 4f53cd 44136f 4e0740 b2e89f 5feceb 5feceb 785f3e 6b51d4 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e fffc38 213d2f 213d2f',
    'syn/ghn3tm8/128/f32/eval/side':
        '28d3c2 860050 860050 860050 cb0e4b 5c7195 dc937b dc937b 47ebd0 7b3aba fcccb7 e3b0c4 6ffc91 2464d5 dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 5aa4ca dc937b dc937b',
    'syn/ghn3tm8/128/f32/eval/noside':
        'e3e3de 860050 860050 860050 cb0e4b 5c7195 dc937b dc937b 47ebd0 7b3aba fcccb7 e3b0c4 6ffc91 2464d5 dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 5aa4ca dc937b dc937b',
    'syn/ghn3tm8/128/f16/train/side':
        '85f3f8 2b0cc0 46c2cc e2b9f5 774279 e69f68 b49505 294fa0 3e65db 2c5169 c10c09 9798ed 2102ee 2464d5 2f01d2 be5d0e ed988f 73731e 6b5d1a 6825ab 4e0740 b2e89f 6f3bf5 5feceb eb1e33 535fa3 7ebfd4 5feceb 5e032c 28cb03 042ed9 0e6c02 66ba7e 5451d7 2e6124 71bb15',
    'syn/ghn3tm8/128/f16/train/noside':
        '2541b1 c01c44 03fad2 7c64ad c97542 08db16 e6042a b28c27 3e65db 2c5169 c10c09 ae228e 201247 2464d5 a54e9c be5d0e 1387cc 14ec8c 9ca282 7810b7 4e0740 b2e89f 6f3bf5 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 28cb03 042ed9 8043cf 66ba7e 5451d7 569121 d6d254',
    'syn/ghn3tm8/128/f16/eval/side':
        '7d5fa9 860050 e2f625 d39e26 d22daa 88fa90 dc937b dc937b 47ebd0 5a18e2 449326 e3b0c4 aeed5b 2464d5 033b91 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 06fa0f dc937b dc937b',
    'syn/ghn3tm8/128/f16/eval/noside':
        'fdbcb1 860050 14622a 144326 d22daa 88fa90 dc937b dc937b 47ebd0 5a18e2 449326 e3b0c4 aeed5b 2464d5 033b91 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 06fa0f dc937b dc937b',
    'syn/ghn3tm8/128/bf16/train/side':
        '33f845 861822 46c2cc e2b9f5 53f61e 191997 7de759 828f2f 3e65db 2c5169 c10c09 0e259f 2102ee 2464d5 2f01d2 be5d0e a59fd9 4f53cd 4f53cd 44136f 4e0740 b2e89f 5feceb 5feceb 35135a 6f4b66 08c31f 5feceb 5e032c 28cb03 042ed9 0e6c02 66ba7e 5451d7 1e7c37 1e7c37',
    'syn/ghn3tm8/128/bf16/train/noside':
        '5e8c34 b70041 03fad2 7c64ad 5fd099 8b9931 b6bb30 9d75b1 3e65db 2c5169 c10c09 4126c9 201247 2464d5 a54e9c be5d0e 9822a2 4f53cd 4f53cd 44136f 4e0740 b2e89f 5feceb 5feceb 59e197 8527a8 a4b127 5feceb 5b7c47 28cb03 042ed9 8043cf 66ba7e 5451d7 a2a0ae a2a0ae',
    'syn/ghn3tm8/128/bf16/eval/side':
        '00dcdc 860050 e2f625 d39e26 d22daa c530b8 dc937b dc937b 47ebd0 5a18e2 449326 e3b0c4 aeed5b 2464d5 033b91 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 06fa0f dc937b dc937b',
    'syn/ghn3tm8/128/bf16/eval/noside':
        'da2e45 860050 14622a 144326 d22daa c530b8 dc937b dc937b 47ebd0 5a18e2 449326 e3b0c4 aeed5b 2464d5 033b91 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 06fa0f dc937b dc937b',
    'syn/ghn3lm8/33-60/f32/train/side':
        'f0050a 14c185 860050 860050 894f3f 41a5ed 3c7ced 9ea854 41f3b9 fbfe5b 0462b3 c279f0 dc5476 3c3ccb dc937b 4dcc2d 44136f 4f53cd 4f53cd 44136f 4e0740 b998d4 5feceb 5feceb 624b60 5f9c4a dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 18621b 4fb2a1 4fb2a1',
    'syn/ghn3lm8/33-60/f32/train/noside':
        '7f5b52 01e0e2 860050 860050 5da4bb 7cb545 2aabe5 d95e57 41f3b9 fbfe5b 0462b3 267c00 cd62a6 3c3ccb dc937b 4dcc2d 44136f 4f53cd 4f53cd 44136f 4e0740 b998d4 5feceb 5feceb 35135a 9400f1 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 18621b 024675 024675',
    'syn/ghn3lm8/33-60/f32/eval/side':
        'a9759b 860050 860050 860050 649013 5741c7 dc937b dc937b d5eb4a fbfe5b 0462b3 e3b0c4 1a7ced 3c3ccb dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 7ecd45 dc937b dc937b',
    'syn/ghn3lm8/33-60/f32/eval/noside':
        '8e8988 860050 860050 860050 649013 5741c7 dc937b dc937b d5eb4a fbfe5b 0462b3 e3b0c4 1a7ced 3c3ccb dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 7ecd45 dc937b dc937b',
    'syn/ghn3lm8/33-60/f16/train/side':
        '7a2629 603e45 91f40e 245724 8374de cd03c0 30a663 f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 45d72c 5a0c7a',
    'syn/ghn3lm8/33-60/f16/train/noside':
        'cc154f 940435 23e38f 07f941 b185d1 a437a4 05cf67 0ceedb da8b90 3e807a f1e89c 1ff047 08529d 3c3ccb 5ebbeb 1e3fac 4cc2cf db3de1 14ec8c 2730d8 4e0740 b998d4 d18b44 5feceb eb1e33 452354 115aa7 5feceb 5b7c47 d02b5b 042ed9 df3fef 66ba7e 5a8631 155cef d99217',
    'syn/ghn3lm8/33-60/f16/eval/side':
        '15e41a 860050 0eaf66 5c6e8b d51e4b d18bac dc937b dc937b d5eb4a ff1890 ef9d1d e3b0c4 6e0928 3c3ccb 741e56 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 225507 dc937b dc937b',
    'syn/ghn3lm8/33-60/f16/eval/noside':
        '6657c2 860050 ef9b93 f557c6 d51e4b d18bac dc937b dc937b d5eb4a ff1890 ef9d1d e3b0c4 6e0928 3c3ccb 741e56 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 225507 dc937b dc937b',
    'syn/ghn3lm8/33-60/bf16/train/side':
        '618bb9 c46ca9 91f40e 245724 411749 7fc495 291c0c 033446 da8b90 3e807a f1e89c 11e1df 87d740 3c3ccb 6487f7 1e3fac 222997 4f53cd 4f53cd 44136f 4e0740 b998d4 5feceb 5feceb 624b60 785f3e f1c775 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 ca9ae5 ca9ae5',
    'syn/ghn3lm8/33-60/bf16/train/noside':
        '8e9c21 fa89ef 23e38f 07f941 4ea3b6 e1af1a eb9621 18a440 da8b90 3e807a f1e89c 7e6817 08529d 3c3ccb 5ebbeb 1e3fac 215fbe 4f53cd 4f53cd 44136f 4e0740 b998d4 5feceb 5feceb 35135a e629fa a7d54b 5feceb 5b7c47 d02b5b 042ed9 df3fef 66ba7e 5a8631 e5b4fa e5b4fa',
    'syn/ghn3lm8/33-60/bf16/eval/side':
        '4de443 860050 0eaf66 5c6e8b d51e4b aa0d6c dc937b dc937b d5eb4a ff1890 ef9d1d e3b0c4 6e0928 3c3ccb 741e56 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 225507 dc937b dc937b',
    'syn/ghn3lm8/33-60/bf16/eval/noside':
        '68280c 860050 ef9b93 f557c6 d51e4b aa0d6c dc937b dc937b d5eb4a ff1890 ef9d1d e3b0c4 6e0928 3c3ccb 741e56 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 225507 dc937b dc937b',
    'syn/ghn3xlm16/256/f32/train/side':
        '877187 543aa8 860050 860050 c3628e 4fe2c6 c1aa6b 583d91 c8877e 15a546 1212d5 15f565 d447e2 31c247 dc937b 8fcd1e 44136f 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb aea921 86e501 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 245599 51a553 51a553',
    'syn/ghn3xlm16/256/f32/train/noside':
        'b9d16a 7fb05e 860050 860050 06d602 3df41b c62edb 35f59b c8877e 15a546 1212d5 955558 0caa19 31c247 dc937b 8fcd1e 44136f 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 7a61b5 670671 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 245599 11c979 11c979',
    'syn/ghn3xlm16/256/f32/eval/side':
        '9a6b2e 860050 860050 860050 742632 0d765a dc937b dc937b 71238c 15a546 1212d5 e3b0c4 6b61f9 31c247 dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 8e3a2c dc937b dc937b',
    'syn/ghn3xlm16/256/f32/eval/noside':
        '8e8f9c 860050 860050 860050 742632 0d765a dc937b dc937b 71238c 15a546 1212d5 e3b0c4 6b61f9 31c247 dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 8e3a2c dc937b dc937b',
    'syn/ghn3xlm16/256/f16/train/side':
        '97a03d 5f5154 c10f17 8af74e cc9d87 b4c07f e4d930 f0166f f62780 59c73c 18cfc2 1f5f36 d48aef 31c247 c85eea ad3c8a fe1ea8 b8333f 9a7578 45c8c2 4e0740 c843cd 1bd606 5feceb eb1e33 535fa3 7ebfd4 2747b7 ee5ee4 2039c2 042ed9 a861a4 66ba7e f8d73d 26564e feb8d4',
    'syn/ghn3xlm16/256/f16/train/noside':
        'da48f0 24170e 216412 c5c028 f2a8e0 cdcc06 287223 f79b2d f62780 59c73c 18cfc2 25a8a0 e6e55b 31c247 83ad95 ad3c8a 1387cc 14ec8c 9ca282 7810b7 4e0740 c843cd 1bd606 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 2039c2 042ed9 1dc048 66ba7e f8d73d b46b85 49c11c',
    'syn/ghn3xlm16/256/f16/eval/side':
        'd2d949 860050 c7d01c 106049 430fda 441f26 dc937b dc937b 71238c 70af68 65c79a e3b0c4 c8afaf 31c247 24201e 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b f6ea46 dc937b dc937b',
    'syn/ghn3xlm16/256/f16/eval/noside':
        'be50a4 860050 b0f8c5 8c525e 430fda 441f26 dc937b dc937b 71238c 70af68 65c79a e3b0c4 c8afaf 31c247 24201e 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b f6ea46 dc937b dc937b',
    'syn/ghn3xlm16/256/bf16/train/side':
        '073aaf d9a584 c10f17 8af74e b35256 b1f167 2e283f 60cd1e f62780 59c73c 18cfc2 157c46 d48aef 31c247 c85eea ad3c8a 0367e8 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 35135a 6f4b66 08c31f 2747b7 ee5ee4 2039c2 042ed9 a861a4 66ba7e f8d73d 950511 950511',
    'syn/ghn3xlm16/256/bf16/train/noside':
        'dfde72 0ceb2a 216412 c5c028 86013f 17eba6 a241d2 1b6399 f62780 59c73c 18cfc2 98a6a7 e6e55b 31c247 83ad95 ad3c8a 9822a2 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 59e197 8527a8 a4b127 5feceb 5b7c47 2039c2 042ed9 1dc048 66ba7e f8d73d 668344 668344',
    'syn/ghn3xlm16/256/bf16/eval/side':
        '008545 860050 c7d01c 106049 430fda e19747 dc937b dc937b 71238c 70af68 65c79a e3b0c4 c8afaf 31c247 24201e 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b f6ea46 dc937b dc937b',
    'syn/ghn3xlm16/256/bf16/eval/noside':
        '31329b 860050 b0f8c5 8c525e 430fda e19747 dc937b dc937b 71238c 70af68 65c79a e3b0c4 c8afaf 31c247 24201e 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b f6ea46 dc937b dc937b',
    'syn/ghn3xlm16/256-256/f32/train/side':
        'ba1b14 441b67 860050 860050 cdad4e 660b80 0c0422 4116d1 8a1703 1b0655 e2d6a8 5c832e 2c6472 62be80 dc937b d5d496 44136f 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 44cb73 0b9189 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 46ddaa 260d7f 260d7f',
    'syn/ghn3xlm16/256-256/f32/train/noside':
        'aae58f 004007 860050 860050 61fb35 3a8a3b 3df886 0eb7f9 8a1703 1b0655 e2d6a8 9c61f8 1a8e51 62be80 dc937b d5d496 44136f 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 73475c e29c9c dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 46ddaa b08538 b08538',
    'syn/ghn3xlm16/256-256/f32/eval/side':
        '57bf35 860050 860050 860050 7c3cb8 55a5e7 dc937b dc937b 71238c 1b0655 e2d6a8 e3b0c4 cc25ad 62be80 dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b d56db6 dc937b dc937b',
    'syn/ghn3xlm16/256-256/f32/eval/noside':
        'f26358 860050 860050 860050 7c3cb8 55a5e7 dc937b dc937b 71238c 1b0655 e2d6a8 e3b0c4 cc25ad 62be80 dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b d56db6 dc937b dc937b',
    'syn/ghn3xlm16/256-256/f16/train/side':
        '8bb8ff 22c460 c10f17 8af74e c1aab7 115d8b 371146 742c80 3423c7 cca714 4b5874 78a011 919070 62be80 ac6fe0 1fc05c f43090 8ae6b5 3495d5 6384e3 4e0740 c843cd 3c767f 5feceb c6f3ac 5f9c4a 87dc60 2747b7 ee5ee4 28cb03 042ed9 ff13d6 66ba7e 917911 374269 9ed614',
    'syn/ghn3xlm16/256-256/f16/train/noside':
        'f8eec1 ef55e9 216412 c5c028 16ba76 cefbc6 99a1a7 6ede19 3423c7 cca714 4b5874 3575ad 3aa232 62be80 f22cec 1fc05c 9bc1f7 9cb9ea 8069a9 3d6ae6 4e0740 c843cd 3c767f 5feceb e29c9c 9400f1 360d75 5feceb 5b7c47 28cb03 042ed9 6d04df 66ba7e 917911 7b3c02 572f21',
    'syn/ghn3xlm16/256-256/f16/eval/side':
        '6ee4d5 860050 c7d01c 106049 f972f0 34da0f dc937b dc937b 71238c fb7315 d937cd e3b0c4 aae92d 62be80 d9b9b4 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b aa9dd8 dc937b dc937b',
    'syn/ghn3xlm16/256-256/f16/eval/noside':
        'de245d 860050 b0f8c5 8c525e f972f0 34da0f dc937b dc937b 71238c fb7315 d937cd e3b0c4 aae92d 62be80 d9b9b4 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b aa9dd8 dc937b dc937b',
    'syn/ghn3xlm16/256-256/bf16/train/side':
        '0cd5c3 9f3f71 c10f17 8af74e e36b19 c3b8ba 7a3d5d 1d57d3 3423c7 cca714 4b5874 2a5baf 919070 62be80 ac6fe0 1fc05c 184ea0 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb eb1e33 c23560 0a93af 2747b7 ee5ee4 28cb03 042ed9 ff13d6 66ba7e 917911 6b79b9 6b79b9',
    'syn/ghn3xlm16/256-256/bf16/train/noside':
        '3a929e db99df 216412 c5c028 21a2eb 9fdeac 3e8ecf ee4995 3423c7 cca714 4b5874 c9e7fb 3aa232 62be80 f22cec 1fc05c e7ca8a 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 624b60 452354 115aa7 5feceb 5b7c47 28cb03 042ed9 6d04df 66ba7e 917911 d1d9af d1d9af',
    'syn/ghn3xlm16/256-256/bf16/eval/side':
        'c33f8e 860050 c7d01c 106049 f972f0 410a35 dc937b dc937b 71238c fb7315 d937cd e3b0c4 aae92d 62be80 d9b9b4 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b aa9dd8 dc937b dc937b',
    'syn/ghn3xlm16/256-256/bf16/eval/noside':
        'a18c1a 860050 b0f8c5 8c525e f972f0 410a35 dc937b dc937b 71238c fb7315 d937cd e3b0c4 aae92d 62be80 d9b9b4 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b aa9dd8 dc937b dc937b',
    'syn/ghn3xlm16/33-60/f32/train/side':
        '673943 9d618a 860050 860050 21b0d8 f02d90 1cdb61 dbdaef 06b814 3b66a0 285d15 d7d8d4 8022c0 3c3ccb dc937b 8066c9 44136f 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 7a61b5 c6f3ac dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e e9cbae b53b4d b53b4d',
    'syn/ghn3xlm16/33-60/f32/train/noside':
        '24393e 11b4d5 860050 860050 8f3697 7abe7a 678302 f71b43 06b814 3b66a0 285d15 27f455 55dc0a 3c3ccb dc937b 8066c9 44136f 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 76a508 5f9c4a dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e e9cbae 09f5be 09f5be',
    'syn/ghn3xlm16/33-60/f32/eval/side':
        '67f3f7 860050 860050 860050 ff9b72 8e2209 dc937b dc937b 71238c 3b66a0 285d15 e3b0c4 d89c9c 3c3ccb dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b bb0b13 dc937b dc937b',
    'syn/ghn3xlm16/33-60/f32/eval/noside':
        '528758 860050 860050 860050 ff9b72 8e2209 dc937b dc937b 71238c 3b66a0 285d15 e3b0c4 d89c9c 3c3ccb dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b bb0b13 dc937b dc937b',
    'syn/ghn3xlm16/33-60/f16/train/side':
        'f1146b a96416 c10f17 8af74e 791cf1 aa1745 e076b0 b6e099 1f165a ac9b15 d511d3 50b052 197950 3c3ccb 08aca2 097eb9 1ce12b c873e1 af3e2c 6b78ee 4e0740 c843cd b7ee30 5feceb 86e501 5f9c4a 87dc60 5feceb 5e032c 28cb03 042ed9 9567b6 66ba7e c99ea5 47e221 9216ca',
    'syn/ghn3xlm16/33-60/f16/train/noside':
        '9a5351 e6ca4a 216412 c5c028 aa6b16 7f1a98 8cfe43 4099a6 1f165a ac9b15 d511d3 f31e53 92d21b 3c3ccb df6a16 097eb9 9bc1f7 9cb9ea 8069a9 3d6ae6 4e0740 c843cd b7ee30 5feceb c6f3ac 9400f1 360d75 5feceb 5b7c47 28cb03 042ed9 47931b 66ba7e c99ea5 acb5e0 d9e4dd',
    'syn/ghn3xlm16/33-60/f16/eval/side':
        'a9e278 860050 c7d01c 106049 58fa62 0a4da5 dc937b dc937b 71238c 3d6de0 b79fb8 e3b0c4 d92fd9 3c3ccb 158654 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b c3604e dc937b dc937b',
    'syn/ghn3xlm16/33-60/f16/eval/noside':
        '61d7d4 860050 b0f8c5 8c525e 58fa62 0a4da5 dc937b dc937b 71238c 3d6de0 b79fb8 e3b0c4 d92fd9 3c3ccb 158654 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b c3604e dc937b dc937b',
    'syn/ghn3xlm16/33-60/bf16/train/side':
        '37bf9b c6b947 c10f17 8af74e 100877 81d087 74bfde 4dc244 1f165a ac9b15 d511d3 01551d 197950 3c3ccb 08aca2 097eb9 6ddd5e 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb e29c9c c23560 0a93af 5feceb 5e032c 28cb03 042ed9 9567b6 66ba7e c99ea5 830814 830814',
    'syn/ghn3xlm16/33-60/bf16/train/noside':
        '0d9e9a 777d6b 216412 c5c028 4935b5 875744 99b4bf be0a25 1f165a ac9b15 d511d3 503ee9 92d21b 3c3ccb df6a16 097eb9 e7ca8a 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb eb1e33 452354 115aa7 5feceb 5b7c47 28cb03 042ed9 47931b 66ba7e c99ea5 d57023 d57023',
    'syn/ghn3xlm16/33-60/bf16/eval/side':
        '37b569 860050 c7d01c 106049 58fa62 365ebe dc937b dc937b 71238c 3d6de0 b79fb8 e3b0c4 d92fd9 3c3ccb 158654 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b c3604e dc937b dc937b',
    'syn/ghn3xlm16/33-60/bf16/eval/noside':
        '57e87a 860050 b0f8c5 8c525e 58fa62 365ebe dc937b dc937b 71238c 3d6de0 b79fb8 e3b0c4 d92fd9 3c3ccb 158654 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b c3604e dc937b dc937b',
    'syn/ghn3xlm16/256/seed256000/f32/train/side':
        '95768d 081d25 860050 860050 885f54 26e6ca 87550d 69929e 503c91 84149e f22786 dcf782 f4659b 5d7a74 dc937b 288629 44136f 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 76a508 e29c9c dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e b553af 0f565b 0f565b',
    'syn/ghn3xlm16/256/seed256000/f32/train/noside':
        'd4b8c4 a55734 860050 860050 dffc02 6ec388 0cf0ac c38748 503c91 84149e f22786 aadb2a d30cee 5d7a74 dc937b 288629 44136f 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 9f1402 b7a568 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e b553af 7791dd 7791dd',
    'syn/ghn3xlm16/256/seed256000/f32/eval/side':
        '96782f 860050 860050 860050 feb9e3 101ccb dc937b dc937b 71238c 84149e f22786 e3b0c4 06141b 5d7a74 dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 0744fd dc937b dc937b',
    'syn/ghn3xlm16/256/seed256000/f32/eval/noside':
        '26c896 860050 860050 860050 feb9e3 101ccb dc937b dc937b 71238c 84149e f22786 e3b0c4 06141b 5d7a74 dc937b 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 0744fd dc937b dc937b',
    'syn/ghn3xlm16/256/seed256000/f16/train/side':
        '1be6c2 c556e7 c10f17 8af74e 325816 0d432c d7811d e2b64f cd86c0 663c54 c3cba0 1c7ae7 cad255 5d7a74 0cded9 426185 fe1ea8 b8333f 9a7578 45c8c2 4e0740 c843cd db5a19 5feceb eb1e33 535fa3 7ebfd4 2747b7 ee5ee4 2039c2 042ed9 eb49b0 66ba7e 290de4 f60fcd bfc65f',
    'syn/ghn3xlm16/256/seed256000/f16/train/noside':
        '784b1b 5dfed6 216412 c5c028 420c6d ae7aa2 5b9c43 6937d3 cd86c0 663c54 c3cba0 336bad 4781eb 5d7a74 d8b893 426185 1387cc 14ec8c 9ca282 7810b7 4e0740 c843cd db5a19 5feceb 624b60 b17ef6 cd7ea3 5feceb 5b7c47 2039c2 042ed9 a81f59 66ba7e 290de4 193c80 8d3d84',
    'syn/ghn3xlm16/256/seed256000/f16/eval/side':
        'c4f000 860050 c7d01c 106049 bc5bd5 b39d67 dc937b dc937b 71238c c21f34 541a5a e3b0c4 5eea90 5d7a74 ad79a1 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 1ace04 dc937b dc937b',
    'syn/ghn3xlm16/256/seed256000/f16/eval/noside':
        '2bdf14 860050 b0f8c5 8c525e bc5bd5 b39d67 dc937b dc937b 71238c c21f34 541a5a e3b0c4 5eea90 5d7a74 ad79a1 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 1ace04 dc937b dc937b',
    'syn/ghn3xlm16/256/seed256000/bf16/train/side':
        '5361b2 192a70 c10f17 8af74e 03d1a3 591d0b 6be565 cb1261 cd86c0 663c54 c3cba0 379b33 cad255 5d7a74 0cded9 426185 0367e8 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 35135a 6f4b66 08c31f 2747b7 ee5ee4 2039c2 042ed9 eb49b0 66ba7e 290de4 f7fb12 f7fb12',
    'syn/ghn3xlm16/256/seed256000/bf16/train/noside':
        'b81c4e 4c8460 216412 c5c028 3dd249 da351b 7ecb43 fd4b55 cd86c0 663c54 c3cba0 c10e48 4781eb 5d7a74 d8b893 426185 9822a2 4f53cd 4f53cd 44136f 4e0740 c843cd 5feceb 5feceb 59e197 8527a8 a4b127 5feceb 5b7c47 2039c2 042ed9 a81f59 66ba7e 290de4 1cb8b5 1cb8b5',
    'syn/ghn3xlm16/256/seed256000/bf16/eval/side':
        'b34940 860050 c7d01c 106049 bc5bd5 131e44 dc937b dc937b 71238c c21f34 541a5a e3b0c4 5eea90 5d7a74 ad79a1 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 1ace04 dc937b dc937b',
    'syn/ghn3xlm16/256/seed256000/bf16/eval/noside':
        'dce04a 860050 b0f8c5 8c525e bc5bd5 131e44 dc937b dc937b 71238c c21f34 541a5a e3b0c4 5eea90 5d7a74 ad79a1 2e38e7 44136f 4f53cd 4f53cd 44136f dc937b 44136f 5feceb dc937b dc937b dc937b dc937b 5feceb dc937b dc937b 4f53cd dc937b dc937b 1ace04 dc937b dc937b',
    'syn/ghn3lm8/33-60/f16/train/side/bwd_bf16':
        '7a2629 c46ca9 91f40e 245724 411749 489e64 291c0c 033446 da8b90 3e807a f1e89c 11e1df 87d740 3c3ccb 6487f7 1e3fac 222997 4f53cd 4f53cd 44136f 4e0740 b998d4 5feceb 5feceb 624b60 785f3e f1c775 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 ca9ae5 ca9ae5',
    'syn/ghn3lm8/33-60/f16/train/side/no_direct16':
        '6e7ad4 7a2b88 6520bf 6520bf adeefe d07ac7 9c10c6 64f114 d37af7 099177 736722 e3ffe7 d385c2 3c3ccb dc937b 6e8ac0 44136f 4f53cd 4f53cd 44136f 4e0740 b998d4 5feceb 5feceb 624b60 5f9c4a dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 18621b 4a2eaa 4a2eaa',
    'syn/ghn3lm8/33-60/f16/train/side/no_x3':
        '330f63 a003e1 1de5b7 fef380 23163e cfc874 2ce6dc d7f684 e6468a 704f11 89d4c3 aa4884 e037d6 3c3ccb f14b23 3a7951 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 c1db39 66ba7e 5a8631 d5c725 4e5809',
    'switch/X3=0':
        '330f63 a003e1 1de5b7 fef380 23163e cfc874 2ce6dc d7f684 e6468a 704f11 89d4c3 aa4884 e037d6 3c3ccb f14b23 3a7951 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 c1db39 66ba7e 5a8631 d5c725 4e5809',
    'switch/X3S=0':
        '1aa026 dc9685 91f40e 245724 9f49aa 2f4a59 e68f1a 05a2d8 3c38ea 3e807a f1e89c 5cb00b 272145 3c3ccb c5232a cd67eb 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 1a9081 66ba7e 5a8631 b7d322 f01d39',
    'switch/X3_F16=0':
        '7a2629 603e45 91f40e 245724 01a12d 32f040 30a663 f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 45d72c 5a0c7a',
    'switch/P8=0':
        '30204b 449f8e 91f40e 245724 3b0354 2332ce 8c48bd 1b341d 4be206 0f1780 f69c51 b88cc7 5f1498 3c3ccb 487c0c 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c 28cb03 042ed9 ed5bf4 66ba7e 5a8631 ec484c 0a22be',
    'switch/TILE_D16=0':
        '7a2629 1dd4dd 91f40e 245724 f43838 9336d5 044e0c 033446 da8b90 3e807a f1e89c e32534 87d740 3c3ccb 6487f7 1e3fac 222997 4f53cd 4f53cd 44136f 4e0740 b998d4 5feceb 5feceb 624b60 785f3e f1c775 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 d5cc57 d5cc57',
    'switch/DGRAD_PLANES=0':
        '7a2629 089114 91f40e 245724 3831db d67ade 67a07e 739f96 da8b90 3e807a f1e89c 7194dd 5311bf 3c3ccb e2a6b3 1e3fac 2208c8 af3e2c 2513f6 7be10e 4e0740 b998d4 d18b44 5feceb c6f3ac b7a568 7280b3 5feceb 5e032c dc937b 042ed9 277025 66ba7e 5a8631 b33a88 3db035',
    'switch/DGRAD_PIN=0':
        '7a2629 599886 91f40e 245724 7a0e9f 23f54f 91ceab b40c4c da8b90 3e807a f1e89c 0969f6 5f1498 3c3ccb 487c0c 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c 28cb03 042ed9 ed5bf4 66ba7e 5a8631 10e757 623d69',
    'switch/DGRAD_EQ=0':
        '7a2629 603e45 91f40e 245724 f72758 441a84 30a663 f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 45d72c 5a0c7a',
    'switch/DGRAD_SUB=3,1':
        '7a2629 603e45 91f40e 245724 afeec8 8cefa0 30a663 f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c 2039c2 042ed9 6148ea 66ba7e 5a8631 45d72c 5a0c7a',
    'switch/WGRAD_MAIN=0':
        '7a2629 d125b9 91f40e 245724 8374de cd03c0 7e93b8 f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 71ab85 0a9ff8 b8333f 812147 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 2747b7 ee5ee4 d02b5b 042ed9 6148ea 66ba7e 5a8631 c1c75e a32f5b',
    'switch/WGRAD_CAP=96':
        '7a2629 936a00 91f40e 245724 8374de cd03c0 2b8cf6 f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 71ab85 0a9ff8 b8333f 812147 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 7b1a27 ee5ee4 d02b5b 042ed9 6148ea 66ba7e 5a8631 ac0a77 b604e2',
    'switch/WGRAD_ORDER=early':
        '7a2629 3abb7d 91f40e 245724 8374de cd03c0 30a663 f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5b7c47 d02b5b 042ed9 6148ea 66ba7e 5a8631 d52e79 4eab28',
    'switch/WGRAD_LATE=0':
        '7a2629 3abb7d 91f40e 245724 8374de cd03c0 30a663 f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5b7c47 d02b5b 042ed9 6148ea 66ba7e 5a8631 d52e79 4eab28',
    'switch/WGRAD_PREP_LATE=0':
        '7a2629 a4f588 91f40e 245724 8374de cd03c0 49707c f9fcf5 da8b90 3e807a f1e89c fe67ff 87d740 3c3ccb 6487f7 1e3fac 44136f 0a9ff8 b8333f 812147 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 69c8be c4f414',
    'switch/WGRAD_TILE=30':
        '7a2629 8ebc25 91f40e 245724 a1edf3 5ffddd 28afca 3b5094 da8b90 3e807a f1e89c d86ad3 886701 3c3ccb 97db58 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 c9f208 66ba7e 5a8631 4c1e1c d56244',
    'switch/WGRAD_SUMSQ=0':
        '7a2629 143e97 91f40e 245724 638da3 489941 dad0ac 6eba8e da8b90 3e807a f1e89c 4ebd6c 877be3 3c3ccb 762d9b 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb eb1e33 535fa3 a4a3ca 5feceb 5e032c d02b5b 042ed9 dc937b 66ba7e 5a8631 02b7a3 702d28',
    'switch/EARLY_1D=0':
        '7a2629 0fdfbb 91f40e 245724 e801a6 b450e6 e81f47 5c65a3 da8b90 3e807a f1e89c 938212 87d740 3c3ccb 5ebbeb 1e3fac 4cc2cf db3de1 14ec8c 2730d8 4e0740 b998d4 d18b44 5feceb eb1e33 452354 115aa7 5feceb 5e032c d02b5b 042ed9 df3fef 66ba7e 5a8631 5d3573 e40585',
    'switch/D2_DGRAD_KS=2':
        '7a2629 431fca 91f40e 245724 60003b c7d448 a8a09f c842c6 da8b90 3e807a f1e89c 0d6069 448590 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 4bce58 f9a4f5',
    'switch/D2_DGRAD_TILE=20':
        '7a2629 ff891f 91f40e 245724 8374de cd03c0 14eb12 f9fcf5 da8b90 3e807a f1e89c 561a6f 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 12748f 197fd9',
    'switch/D1_DGRAD_TILE=64':
        '7a2629 a9f093 91f40e 245724 8374de cd03c0 0a4264 f9fcf5 da8b90 3e807a f1e89c 717573 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 863d93 aa51b1',
    'switch/D1_BWD=f16':
        '7a2629 c1b53f 91f40e 245724 8374de cd03c0 da0405 f9fcf5 da8b90 3e807a f1e89c 069b01 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 9c56fb ccff15',
    'switch/LAYER_WGRAD_DEFER=0':
        '7a2629 ba3060 91f40e 245724 1dae0c cc7117 30a663 c1e5a3 da8b90 3e807a f1e89c fe1297 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 b7cad5 36e3e2',
    'switch/LAYER_WGRAD_GROUP=4':
        '7a2629 5723f3 91f40e 245724 e91b8c cd03c0 30a663 58d9ac da8b90 3e807a f1e89c 689859 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 957093 d672e0',
    'switch/LAYER_WGRAD_TILE=64':
        '7a2629 497d58 91f40e 245724 8374de cd03c0 30a663 e32186 da8b90 3e807a f1e89c 0975da 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 143c3e 376c00',
    'switch/LAYER_WGRAD_CAP=64':
        '7a2629 8bffbd 91f40e 245724 8374de cd03c0 30a663 0516d7 da8b90 3e807a f1e89c 7e2ac4 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 7c4186 0ca458',
    'switch/EMBED_BWD_MAIN=0':
        '7a2629 dd3740 91f40e 245724 8374de cd03c0 30a663 0e78cf da8b90 3e807a f1e89c 0cb81b 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 9b0e5f 0dfc0e',
    'switch/DDP_WGRAD_FIRST=0':
        '7a2629 603e45 91f40e 245724 8374de cd03c0 30a663 f9fcf5 da8b90 3e807a f1e89c 33a720 87d740 3c3ccb 6487f7 1e3fac 44136f 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 45d72c 5a0c7a',
    'switch/CLS_FAMILY=0':
        '594a44 eff882 91f40e 245724 d9795a 05df92 de4c39 392461 da8b90 3e807a f1e89c db5a53 b787f2 3c3ccb 20e0ca 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 ae1acf 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 471c53 66ba7e 5a8631 2506b9 7099ba',
    'switch/PAD_I8=0':
        'e814d5 8dfe0b 91f40e 245724 1d1f91 6ecf9b 2b7d9b afb6a7 be6c07 5dc9ba 26d04a 62b9b3 a04e08 3c3ccb aadff9 ed3460 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d1feb1 5feceb c6f3ac b7a568 4f5683 5feceb 5e032c d02b5b 042ed9 dc937b 66ba7e 18621b 866168 3c0684',
    'switch/P8_MIN_ROWS=8':
        '5304f0 208ef4 91f40e 245724 5c6ba6 7dde8f 188d4c 85eedb fc565d efe1f6 fec241 79e368 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 b83e85 dfb050',
    'switch/WGRAD_MAIN=1':
        '97a03d 7857a9 c10f17 8af74e cc9d87 b4c07f d017f0 f0166f f62780 59c73c 18cfc2 1f5f36 d48aef 31c247 c85eea ad3c8a ed988f 73731e 6b5d1a 6825ab 4e0740 c843cd 1bd606 5feceb eb1e33 535fa3 7ebfd4 5feceb 5e032c 2039c2 042ed9 a861a4 66ba7e f8d73d fced03 12d253',
    'switch/WGRAD_ORDER=late':
        '97a03d 983ae3 c10f17 8af74e cc9d87 b4c07f 7d5949 f0166f f62780 59c73c 18cfc2 1f5f36 d48aef 31c247 c85eea ad3c8a ed988f 73731e 6b5d1a 6825ab 4e0740 c843cd 1bd606 5feceb eb1e33 535fa3 7ebfd4 2abaca 5e032c 2039c2 042ed9 a861a4 66ba7e f8d73d bf8440 897dab',
    'switch/WGRAD_TPW=2':
        '97a03d 12434a c10f17 8af74e cc9d87 b4c07f 00625f f0166f f62780 59c73c 18cfc2 1f5f36 d48aef 31c247 c85eea ad3c8a fe1ea8 b8333f 9a7578 45c8c2 4e0740 c843cd 1bd606 5feceb eb1e33 535fa3 7ebfd4 2747b7 ee5ee4 2039c2 042ed9 a861a4 66ba7e f8d73d e0686a 298edc',
    'switch/DGRAD_PLANES=0/f32':
        'f0050a 3998c7 860050 860050 3204f7 ed411f d86b4a eb8d35 41f3b9 fbfe5b 0462b3 14dac6 c18674 3c3ccb dc937b 4dcc2d 44136f 4f53cd 4f53cd 44136f 4e0740 b998d4 5feceb 5feceb eb1e33 670671 dc937b 5feceb 5b7c47 dc937b 042ed9 dc937b 66ba7e 18621b c10bee c10bee',
    'switch/P8_FINE=False':
        '7a2629 710325 91f40e 245724 aa6875 505dac ca6c95 2e974a da8b90 3e807a f1e89c 3fa99d 5f1498 3c3ccb 487c0c 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c 28cb03 042ed9 ed5bf4 66ba7e 5a8631 7db63a 38455f',
    'switch/P8_BALANCED=False':
        '273038 86686f 91f40e 245724 e14fed 29b50e 7bd7b1 be9127 259819 5dc9ba 26d04a ecad89 87d740 3c3ccb 6487f7 1e3fac 4b1374 2513f6 73731e 6504a9 4e0740 b998d4 d18b44 5feceb e29c9c c23560 0a93af 5feceb 5e032c d02b5b 042ed9 6148ea 66ba7e 5a8631 00b56b c45c30',
}

if __name__ == '__main__':
    _record('--check' in sys.argv)
