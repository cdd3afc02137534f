"""The routing table of target_ops' convolution runners, pinned without a GPU (the cases and the expected traces, recorded as
literals, are in tests/target_routing_cases.py; the kernels themselves are tested in tests/test_gpu_target_*.py).

The real runners and autograd nodes run, forward and backward, on CPU tensors that say they live on the GPU; the library is
replaced by a recorder whose ghn3_* functions note their name, the descriptor, which arguments are null and how the backward's
gradients lie in its one allocation, and return 0.  The stand-in layers note `stock:<kind>` when the stock path calls them."""
import contextlib

import pytest
import torch

import target_routing_cases as R

# *_bwd function -> positions of (first gradient: the start of the one allocation, alternatives in order; dgamma; dbeta; scratch)
CARVED = {'ghn3_dwpw_bn_bwd': ((9, 10), 11, 12, 13), 'ghn3_dwpw_plain_bwd': ((6, 7), None, None, 8),
          'ghn3_dwpw_frozen_bwd': ((10, 11), 12, 13, 14), 'ghn3_dw_bwd': ((5,), None, None, 6),
          'ghn3_conv_bn_bwd': ((8,), 9, 10, 11), 'ghn3_conv_frozen_bwd': ((9,), 10, 11, 12)}


class _Recorder:
    """Stands for the loaded library: every ghn3_* attribute is a function that records its call and reports success."""

    def __getattr__(self, name):
        if not name.startswith('ghn3_'):
            raise AttributeError(name)
        if name.endswith('_scratch_floats'):
            return lambda d, backward: 8                  # (not recorded: asked once per descriptor; non-empty scratch areas)
        return lambda *args: self._record(name, args)

    @staticmethod
    def _record(name, args):
        d = args[0]._obj
        fields = ' '.join('%s=%g' % (f, getattr(d, f)) for f, _ in d._fields_)
        line = '%s [%s] ptrs=%s' % (name, fields, ''.join('x' if a else '-' for a in args[1:-1]))
        if name in CARVED:
            first, dg, db, scratch = CARVED[name]
            start = next(args[k] for k in first if args[k])
            carve = []
            if dg is not None and args[dg]:
                carve.append('dbeta|dgamma' if args[dg] - args[db] == 4 * d.C_out else 'dbeta,dgamma APART')
            carve.append('scratch%256' if (args[scratch] - start) % 256 == 0 else 'scratch UNALIGNED')
            line += ' carve=' + ','.join(carve)
        R.TRACE.append(line)
        return 0


@pytest.fixture
def routed(monkeypatch):
    from ghn3_amd import target_ops as T
    monkeypatch.setattr(torch.Tensor, 'is_cuda', True, raising=False)    # (also on the tensors a node allocates itself)
    monkeypatch.setattr(T, '_stream', lambda: 0)
    monkeypatch.setattr(T.L, 'load', lambda: _Recorder())
    monkeypatch.setattr(T, '_SCRATCH', {})
    for name in ('OPS', 'CONV', 'NONORM', 'EVALBN', 'WIDE', 'STEM', 'AMP', 'LAZY_LAYOUT'):
        monkeypatch.delenv('GHN3_NATIVE_' + name, raising=False)
    return T


def _layout(out):
    if out is None:
        return 'None'
    assert out.dim() == 4 and min(out.shape[1:]) > 1               # (else both layouts hold at once)
    return 'NCHW' if out.is_contiguous() else 'NHWC' if out.is_contiguous(memory_format=torch.channels_last) else 'strided'


def _run(T, monkeypatch, spec, mode):
    torch.manual_seed(0)
    runner, args, norms = R.BUILDERS[spec['builder']](R.FLAVOURS[spec['flavour']], spec['slot'], **spec['kw'])
    kw = {} if spec['keep_layout'] is None else {'keep_layout': spec['keep_layout']}
    tracked = [bn for bn in norms if getattr(bn, 'running_mean', None) is not None]
    before = [[t.clone() for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)] for bn in tracked]
    del R.TRACE[:]
    with monkeypatch.context() as m, torch.no_grad() if mode == 'no_grad' else contextlib.nullcontext():
        for k, v in spec['env'].items():
            m.setenv(k, v)
        if spec['autocast']:
            m.setattr(torch, 'is_autocast_enabled', lambda *a: True)
        out = getattr(T, runner)(*args, **kw)
        if mode == 'grad' and out is not None and out.requires_grad:
            out.sum().backward()
    trace = list(R.TRACE)
    for bn, old in zip(tracked, before):
        new = (bn.running_mean, bn.running_var, bn.num_batches_tracked)
        same = all(torch.equal(a, b) for a, b in zip(old, new))
        moved = int(bn.num_batches_tracked) == int(old[2]) + 1
        assert same != moved
        trace.append('stats:' + ('untouched' if same else 'moved'))
    trace.append('out:' + _layout(out))
    return trace, out


ALL = [(name, mode) for name, spec in R.CASES.items() for mode in spec['modes']]


def test_every_case_has_its_literal_and_every_literal_its_case():
    assert set(R.EXPECT) == set(R.CASES)
    for name, spec in R.CASES.items():
        assert set(R.EXPECT[name]) == set(spec['modes']), name
        for lines in R.EXPECT[name].values():
            assert lines and all(isinstance(s, str) for s in lines), name


@pytest.mark.parametrize('name,mode', ALL, ids=['%s-%s' % c for c in ALL])
def test_the_block_reaches_the_recorded_calls(routed, monkeypatch, name, mode):
    spec = R.CASES[name]
    trace, out = _run(routed, monkeypatch, spec, mode)
    print('\n'.join(trace))
    assert trace == R.EXPECT[name][mode]
    native = [s for s in trace if s.startswith('ghn3_')]
    # what holds for every case, whatever was recorded
    assert not any('APART' in s or 'UNALIGNED' in s for s in trace)
    if name.startswith('off/') and 'stays_native' not in name:
        assert not native and (any(s.startswith('stock:') for s in trace) or trace[-1] == 'out:None')
    if mode == 'no_grad':
        assert out.grad_fn is None and not any('_bwd' in s for s in native)
        for s in native:
            if '_frozen_fwd' in s:                     # (nothing saved: the pre-norm tensor is not even written)
                z = 7 if s.startswith('ghn3_dwpw') else 6
                assert s.split('ptrs=')[1][z] == '-', s
    if native:
        stats = [s for s in trace if s.startswith('stats:')]
        assert stats == {'batch_run': ['stats:moved'], 'frozen': ['stats:untouched']}.get(spec['slot'], []) * len(stats)
        assert len(stats) == {'batch_run': 1, 'frozen': 1}.get(spec['slot'], 0) * (2 if spec['builder'] == 'seq_stem' else 1)


def test_an_inplace_relu_at_the_head_stays_the_layer_it_is(routed, monkeypatch):
    for slot in R.SLOTS:
        trace, _ = _run(routed, monkeypatch, R.CASES['seq_inplace_relu/' + slot], 'grad')
        assert trace[0] == 'stock:ReLU' and ' relu=%d ' % (2 if slot == 'identity' else 0) in trace[1], trace


def test_hand_over_layouts(routed, monkeypatch):
    want = {'hand_on/nn': 'NCHW', 'hand_on/nn/keep_layout': 'NHWC', 'hand_on/light': 'NHWC', 'hand_on/light/eager_layout': 'NCHW',
            'hand_on/light/eager_layout/keep_layout': 'NHWC', 'hand_on/nn/wide': 'NCHW'}
    for name, layout in want.items():
        assert _run(routed, monkeypatch, R.CASES[name], 'grad')[0][-1] == 'out:' + layout, name
