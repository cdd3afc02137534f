"""Shared helpers of the GPU tests of ghn3_amd.target_ops: the NaN-filled-buffers variant of a case and the names of the autograd
nodes behind a result.  A test file that asks for the `buffers` fixture imports it by name (the fixture lives where it is
imported)."""
import pytest
import torch


class _GarbageTorch:
    """Stands in for the `torch` global of ghn3_amd.target_ops: every buffer the ops allocate (outputs, saved tensors,
    gradients, scratch) starts as NaN -- all-ones bytes for the integer ones -- instead of whatever the allocator holds."""

    def __init__(self):
        self.spoiled = 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def _spoil(self, t):
        self.spoiled += 1
        return t.fill_(float('nan') if t.is_floating_point() else 255)

    def empty(self, *args, **kw):
        return self._spoil(torch.empty(*args, **kw))

    def empty_like(self, *args, **kw):
        return self._spoil(torch.empty_like(*args, **kw))


@pytest.fixture(params=['allocator', 'nan-filled'])
def buffers(request, monkeypatch):
    """The op's buffers as the caching allocator hands them out, or pre-filled with NaN."""
    if request.param == 'allocator':
        yield None
        return
    from ghn3_amd import target_ops as T
    proxy = _GarbageTorch()
    monkeypatch.setattr(T, 'torch', proxy)
    yield proxy
    assert proxy.spoiled >= 2, 'the ops no longer allocate through torch.empty / empty_like: the variant checks nothing'


def _graph_nodes(t):
    """Names of the autograd nodes between t and its leaves, joined."""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo += [f for f, _ in fn.next_functions]
    return ' '.join(names)
