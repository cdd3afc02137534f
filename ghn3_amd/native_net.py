"""
``nativize(model)``: an arbitrary ``torch.nn`` network on the native target-network nodes, without rewriting it by hand.

The native ops of ``ghn3_amd.target_ops`` are called from the block classes of ``ghn3_amd.ops``, which run the DeepNets-1M order
``ReLU -> conv -> BatchNorm``.  The networks the plain ``Trainer`` branch fine-tunes are ResNet-shaped ``torch.nn`` modules that run
``conv -> BatchNorm -> ReLU`` and, at the end of a block, ``conv -> BatchNorm -> (+ skip) -> ReLU``.  ``nativize`` traces such a module
with ``torch.fx`` and replaces these windows of the graph by calls of the runners:

    window                                               runner                                   report key
    Conv2d -> BatchNorm2d -> ReLU                        target_ops.run_conv_window(relu=True)    'conv_bn_relu'
    Conv2d -> BatchNorm2d -> add(., r) -> ReLU           ... (relu=True, residual=r)              'conv_bn_add_relu'
    Conv2d -> BatchNorm2d -> add (the other operand;     ... (relu=False)                         'conv_bn'
      a block's downsample branch)
    MaxPool2d / AvgPool2d / F.max_pool2d / F.avg_pool2d  target_ops.run_pool                      'pool'
    global average pool -> flatten -> Linear             target_ops.run_classifier_head           'head'

The result is a ``torch.fx.GraphModule`` that SHARES the original's submodules, Parameters and buffers (same ``state_dict`` keys; the
original is not modified, and ``train()`` / ``eval()`` / ``to()`` on either reach the same layers).  Every replaced window keeps the
very modules it replaced -- every convolution window is one class, NativeConvWindow, whose runner's table (run_conv_window) names
the member -- and runs them whenever its runner does not apply -- CPU tensors, a switch that is off
(GHN3_NATIVE_OPS / _CONV / _ACT / _POOL / _HEAD / _EVALBN = 0), a limit of the kernels, autocast with GHN3_NATIVE_AMP=0 --, so on the
CPU the nativized module computes what the original computes, bit for bit.  Tensors stay channels_last between native nodes; a stock
node that reads a native node's result gets it NCHW-contiguous (the stock layers of this ROCm build return wrong gradients for
channels_last inputs: target_ops' module text).

``nativize(model, windows='all')`` -- opt-in; the default 'resnet' is the table above and nothing else -- adds, after the convolution
pass, the windows of pre-activation (v2) ResNets and DenseNets, whose BatchNorm does not follow a convolution:

    BatchNorm2d whose only user is a ReLU                target_ops.run_bn_act(relu=True)         'bn_relu'
    any other BatchNorm2d the first pass left            target_ops.run_bn_act(relu=False)        'bn'
    any other Conv2d the first pass left for which       target_ops.run_conv_window(bn=None): the 'conv'
      `conv_refusal` is None; it leaves `stock_convs`      no-norm member, ConvOnly
    torch.cat([...], 1) of 2 .. 16 nodes                 target_ops.cell_concat                   'concat'
    an add of two nodes no window above consumed         target_ops.pair_sum                      'add'

Their counts are in ``report()['windows']`` in that mode only.  The convolutions the dense kernels refuse (`conv_refusal`) keep
their stock layer and their reason in both modes.  Measured against warmed stock layers the stand-alone BatchNorm node is reported in README.md ("Plain networks");
it is opt-in whatever the figure.

``nativize(model, biased=True)`` -- a third opt-in, with either `windows` value -- takes the convolutions WITH a bias (``nn.Conv2d``'s
default; VGG, AlexNet, SqueezeNet and other networks without norm layers), which `conv_refusal` otherwise answers first, and the
classifier such networks end in:

    Conv2d(bias) -> ReLU                                 target_ops.run_conv_window(bn=None,      'conv_bias_relu'
                                                           relu=True)
    Conv2d(bias) -> add(., r) -> ReLU                    ... (relu=True, residual=r)              'conv_bias_add_relu'
    any other Conv2d(bias) for which `conv_refusal(conv, ... (relu=False); it leaves              'conv_bias'
      biased=True)` is None                                `stock_convs`
    flatten(1) -> Linear (-> ReLU -> Dropout -> Linear)  target_ops.run_classifier_head(None, .)  'mlp_head'
      x 1 .. 3: 2 .. 4 linears                             on a Sequential over the SAME modules
    AdaptiveAvgPool2d(size) / F.adaptive_avg_pool2d      the input itself where its map already   'same_size_pool'
      with a constant size other than 1                    has that size (the mean of ONE element:
                                                           exact), else the stock layer

Their counts are in ``report()['windows']`` in that mode only (BIAS_KINDS).  A bias is never folded into a BatchNorm behind the
convolution: that BatchNorm is taken by the 'bn_relu' / 'bn' windows under windows='all' and stays stock under 'resnet'.  The
one-linear 'head' window is tried first and is unchanged.  Measured against warmed stock layers the node is reported in README.md
("Plain networks"); it is opt-in whatever the figure.

Every intermediate node of a window has exactly one user; the convolution is ungrouped, zero-padded with numeric padding, at most
7 x 7 and of one dilation -- and bias-free unless biased=True.  Anything else stays stock, and ``report()`` says why.
"""

import operator

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import target_ops as T
from .utils import log

WINDOW_KINDS = ('conv_bn_relu', 'conv_bn_add_relu', 'conv_bn', 'pool', 'head')
EXTRA_KINDS = ('bn_relu', 'bn', 'conv', 'concat', 'add')          # the opt-in windows of nativize(windows='all')
BIAS_KINDS = ('conv_bias_relu', 'conv_bias_add_relu', 'conv_bias', 'mlp_head', 'same_size_pool')     # those of nativize(biased=True)


def _stock_layout(t):
    """A native node's channels_last result as a stock layer takes it: NCHW-contiguous (the tensor itself when it is already)."""
    if torch.is_tensor(t) and t.dim() == 4 and not t.is_contiguous():
        return t.contiguous()
    return t


class _Window(nn.Module):
    """A replaced window: the layers it stands for are kept OUTSIDE the module registry (they are registered once, where the
    original network has them), so the nativized module's state_dict is the original's."""

    def __init__(self, **layers):
        super().__init__()
        self.__dict__['layers'] = layers

    def extra_repr(self):
        return ', '.join('%s=%s' % (k, type(v).__name__) for k, v in self.layers.items() if v is not None)


class NativeConvWindow(_Window):
    """Conv2d [-> BatchNorm2d] [-> + residual] [-> ReLU]: the member of the dense-convolution family `target_ops.run_conv_window`
    names for it, else the replaced layers in that order."""

    def __init__(self, conv, bn=None, relu=False):
        super().__init__(conv=conv, bn=bn)
        self.relu = bool(relu)

    @property
    def conv_bn_relu(self):
        """The window is a conv -> norm [-> + skip] -> ReLU one (what a downsample branch asks of the node that reads it)."""
        return self.layers['bn'] is not None and self.relu

    def forward(self, x, residual=None):
        conv, bn = self.layers['conv'], self.layers['bn']
        out = T.run_conv_window(conv, bn, x, self.relu, residual)
        if out is not None:
            return out
        y = conv(_stock_layout(x))
        if bn is not None:
            y = bn(y)
        if residual is not None:
            y = y + _stock_layout(residual)
        return F.relu(y) if self.relu else y


class NativePool(_Window):
    """MaxPool2d / AvgPool2d (module or functional form; `stock` re-runs the replaced call)."""

    def __init__(self, stock, kernel_size, stride, padding, mode):
        super().__init__(pool=stock if isinstance(stock, nn.Module) else None)
        self.__dict__['stock'] = stock
        self.cfg = (kernel_size, kernel_size if stride is None else stride, padding, mode)

    def forward(self, x):
        out = T.run_pool(x, *self.cfg) if torch.is_tensor(x) and x.dim() == 4 else None
        return self.__dict__['stock'](_stock_layout(x)) if out is None else out


class NativeHead(_Window):
    """Global average pool -> flatten -> Linear."""

    def __init__(self, fc):
        super().__init__(fc=fc)
        self.__dict__['pool'] = nn.AdaptiveAvgPool2d(1)

    def forward(self, x):
        pool, fc = self.__dict__['pool'], self.layers['fc']
        out = T.run_classifier_head(pool, [fc], x) if torch.is_tensor(x) and x.dim() == 4 else None
        return fc(torch.flatten(pool(_stock_layout(x)), 1)) if out is None else out


class NativeBnAct(_Window):
    """BatchNorm2d [-> ReLU] with no convolution in front of it (windows='all')."""

    def __init__(self, bn, relu):
        super().__init__(bn=bn)
        self.relu = bool(relu)

    def forward(self, x):
        bn = self.layers['bn']
        out = T.run_bn_act(bn, x, self.relu) if torch.is_tensor(x) and x.dim() == 4 else None
        if out is not None:
            return out
        y = bn(_stock_layout(x))
        return F.relu(y) if self.relu else y


class NativeMlpHead(_Window):
    """flatten(1) -> Linear (-> ReLU -> Dropout -> Linear)*, 2 .. 4 linears (biased=True): the classifier head without its pool."""

    def __init__(self, modules):
        super().__init__(**{'m%d' % k: m for k, m in enumerate(modules)})
        self.__dict__['seq'] = nn.Sequential(*modules)             # (over the SAME modules; outside the registry)

    def forward(self, x):
        seq = self.__dict__['seq']
        out = T.run_classifier_head(None, seq, x) if torch.is_tensor(x) and x.dim() == 4 else None
        return seq(torch.flatten(_stock_layout(x), 1)) if out is None else out


class NativeSameSizePool(_Window):
    """An adaptive average pool to a constant size (biased=True): the input itself where its map has that size already."""

    def __init__(self, stock, size):
        super().__init__(pool=stock if isinstance(stock, nn.Module) else None)
        self.__dict__['stock'] = stock
        self.size = size

    def forward(self, x):
        if torch.is_tensor(x) and x.dim() == 4 and tuple(x.shape[-2:]) == self.size:
            return x
        return self.__dict__['stock'](_stock_layout(x))


class NativeConcat(_Window):
    """torch.cat([...], 1) (windows='all'): one join node."""

    def forward(self, *xs):
        out = T.cell_concat(list(xs)) if all(torch.is_tensor(t) and t.dim() == 4 for t in xs) else None
        return torch.cat([_stock_layout(t) for t in xs], 1) if out is None else out


class NativeAdd(_Window):
    """a + b of two activations (windows='all'): one join node."""

    def forward(self, a, b):
        ok = torch.is_tensor(a) and torch.is_tensor(b) and a.dim() == 4 and a.shape == b.shape
        out = T.pair_sum(a, b) if ok else None
        return _stock_layout(a) + _stock_layout(b) if out is None else out


class NativeReport(dict):
    """What nativize did: `windows` (kind -> count), `stock_convs` (module name -> reason), and `traced`."""

    def __str__(self):
        rows = ['%-18s %d' % kv for kv in self['windows'].items()]
        rows += ['stock %s: %s' % kv for kv in self['stock_convs'].items()]
        return '\n'.join(rows)


# ---- the matcher ------------------------------------------------------------------------------------------------------------------
_RELU_FUNCTIONS = (F.relu, torch.relu, torch.relu_, F.relu_)
_ADD_FUNCTIONS = (operator.add, operator.iadd, torch.add)


def conv_refusal(conv, biased=False):
    """Why the dense kernels do not take this Conv2d, or None.  Asked of the layer itself, padding_mode included.  biased=True:
    the answer of nativize(biased=True), where a bias is no reason."""
    if conv.bias is not None and not biased:
        return 'biased convolution'
    if conv.groups != 1:
        return 'grouped convolution (groups=%d)' % conv.groups
    if conv.padding_mode != 'zeros':
        return "padding_mode='%s'" % conv.padding_mode
    if isinstance(conv.padding, str):
        return "padding='%s'" % conv.padding
    if max(conv.kernel_size) > 7:
        return 'kernel %d x %d is larger than 7 x 7' % tuple(conv.kernel_size)
    if len(set(T._pair(conv.dilation))) != 1:
        return 'two dilations'
    return None


class _Matcher:
    def __init__(self, gm, extra=False, biased=False):
        self.gm, self.graph = gm, gm.graph
        self.mods = dict(gm.named_modules())
        self.native = set()                 # the windows' nodes: they read either layout
        self.nhwc = set()                   # those of them whose result is channels_last
        self.extra = extra                  # windows='all': the opt-in passes, and their keys in the report
        self.biased = biased                # biased=True: the windows of biased convolutions, and their keys in the report
        self.windows = dict.fromkeys(WINDOW_KINDS + (EXTRA_KINDS if extra else ()) + (BIAS_KINDS if biased else ()), 0)
        self.stock = {}
        self.n = 0

    def mod(self, node, cls):
        """The module a call_module node calls when it is exactly a `cls`, else None."""
        if node.op == 'call_module':
            m = self.mods.get(node.target)
            if type(m) is cls:
                return m
        return None

    def is_relu(self, node):
        if node.op == 'call_module':
            return self.mod(node, nn.ReLU) is not None
        if node.op == 'call_function':
            return node.target in _RELU_FUNCTIONS
        return node.op == 'call_method' and node.target in ('relu', 'relu_')

    @staticmethod
    def is_add(node):
        if not ((node.op == 'call_function' and node.target in _ADD_FUNCTIONS) or
                (node.op == 'call_method' and node.target in ('add', 'add_'))):
            return False
        return len(node.args) == 2 and not node.kwargs and all(isinstance(a, torch.fx.Node) for a in node.args)

    @staticmethod
    def input_of(node):
        return node.args[0] if node.args else node.kwargs.get('input')

    def skip_add(self, r, add, same_kind):
        """(the other operand, the ReLU node) when the window whose result is `r` takes `add`, the one node that reads r, and
        the ReLU behind it: the add's only user is a ReLU, and r is not added to itself.  When both operands are results of the
        same kind (`same_kind(node)`), the first one takes them.  Else None."""
        other = add.args[1] if add.args[0] is r else add.args[0]
        relu = next(iter(add.users)) if len(add.users) == 1 else None
        if relu is None or not self.is_relu(relu) or self.input_of(relu) is not add or other is r:
            return None
        if add.args[1] is r and same_kind(add.args[0]):
            return None
        return other, relu

    def flattened(self, fl):
        """x when `fl`, a node with one user, is flatten(x, 1) -- nn.Flatten() or the function / method form --, else None."""
        if not isinstance(fl, torch.fx.Node) or len(fl.users) != 1:
            return None
        if fl.op == 'call_module':
            m = self.mods.get(fl.target)
            ok = type(m) is nn.Flatten and m.start_dim == 1 and m.end_dim == -1
        else:
            ok = ((fl.op == 'call_function' and fl.target is torch.flatten) or (fl.op == 'call_method' and fl.target == 'flatten')) and \
                tuple(fl.args[1:]) + tuple(fl.kwargs.values()) == (1,)
        x = self.input_of(fl) if ok else None
        return x if isinstance(x, torch.fx.Node) else None

    def adaptive_pool(self, node):
        """(size, stock) of an adaptive average pool node -- the nn.AdaptiveAvgPool2d itself, or a call of F.adaptive_avg_pool2d
        with that size --, else (None, None)."""
        m = self.mod(node, nn.AdaptiveAvgPool2d)
        if m is not None:
            return m.output_size, m
        if node.op == 'call_function' and node.target is F.adaptive_avg_pool2d:
            size = node.args[1] if len(node.args) > 1 else node.kwargs.get('output_size')
            return size, lambda t: F.adaptive_avg_pool2d(t, size)
        return None, None

    def chain(self, bn_node):
        """(conv node, conv, bn) when bn_node is the BatchNorm2d of a fusable Conv2d -> BatchNorm2d pair with one user each."""
        if not isinstance(bn_node, torch.fx.Node) or self.mod(bn_node, nn.BatchNorm2d) is None or len(bn_node.users) != 1:
            return None
        c = self.input_of(bn_node)
        if not isinstance(c, torch.fx.Node) or len(c.users) != 1:
            return None
        conv = self.mod(c, nn.Conv2d)
        if conv is None or conv_refusal(conv) is not None:
            return None
        return c, conv, self.mods[bn_node.target]

    def put(self, module, args, last, dead, kind, nhwc=True):
        """The window's module in place of its `last` node; `dead`: the window's nodes, last first."""
        name = '_native_%d' % self.n
        self.n += 1
        self.gm.add_module(name, module)
        self.mods[name] = module
        with self.graph.inserting_before(last):
            new = self.graph.call_module(name, args)
        last.replace_all_uses_with(new)
        for node in dead:
            self.graph.erase_node(node)
        self.native.add(new)
        if nhwc:
            self.nhwc.add(new)
        self.windows[kind] += 1
        return new

    def conv_window(self, c):
        conv = self.mod(c, nn.Conv2d)
        if conv is None:
            return
        if self.biased and conv.bias is not None:
            return self.bias_window(c, conv)
        why = conv_refusal(conv)
        users = list(c.users)
        if why is None and len(users) != 1:
            why = 'the convolution has %d users' % len(users)
        if why is None and (self.mod(users[0], nn.BatchNorm2d) is None or self.input_of(users[0]) is not c):
            why = 'not followed by a BatchNorm2d'
        if why is None and len(users[0].users) != 1:
            why = 'the norm layer has %d users' % len(users[0].users)
        if why is not None:
            self.stock[c.target] = why
            return
        b = users[0]
        bn, x = self.mods[b.target], self.input_of(c)
        nxt = next(iter(b.users))
        if self.is_relu(nxt) and self.input_of(nxt) is b:
            self.put(NativeConvWindow(conv, bn, True), (x,), nxt, (nxt, b, c), 'conv_bn_relu')
            return
        if nxt in self.native and getattr(self.mods[nxt.target], 'conv_bn_relu', False) and nxt.args[0] is not b:
            # (the skip operand of a window that is in place already: the other branch of the block)
            self.put(NativeConvWindow(conv, bn), (x,), b, (b, c), 'conv_bn')
            return
        if self.is_add(nxt):
            # (a block with a downsample branch: both operands are conv -> norm results)
            skip = self.skip_add(b, nxt, lambda node: self.chain(node) is not None)
            if skip:
                self.put(NativeConvWindow(conv, bn, True), (x, skip[0]), skip[1], (skip[1], nxt, b, c), 'conv_bn_add_relu')
            else:
                self.put(NativeConvWindow(conv, bn), (x,), b, (b, c), 'conv_bn')
            return
        what = type(self.mods[nxt.target]).__name__ if nxt.op == 'call_module' else getattr(nxt.target, '__name__', str(nxt.target))
        self.stock[c.target] = 'the norm layer is followed by %s, neither a ReLU nor an add' % what

    def pool_window(self, node):
        m = self.mods.get(node.target) if node.op == 'call_module' else None
        if type(m) is nn.MaxPool2d:
            if T._pair(m.dilation) == (1, 1) and not m.ceil_mode and not m.return_indices:
                self.put(NativePool(m, m.kernel_size, m.stride, m.padding, 1), (self.input_of(node),), node, (node,), 'pool')
        elif type(m) is nn.AvgPool2d:
            if not m.ceil_mode and m.divisor_override is None and (not m.count_include_pad or T._pair(m.padding) == (0, 0)):
                self.put(NativePool(m, m.kernel_size, m.stride, m.padding, 0), (self.input_of(node),), node, (node,), 'pool')
        elif node.op == 'call_function' and node.target in (F.max_pool2d, F.avg_pool2d):
            # (input, kernel_size, stride=None, padding=0, ...): anything beyond the three, or a traced value among them, stays stock
            # (torch.fx records max_pool2d's defaults as keyword arguments)
            names = ('input', 'kernel_size', 'stride', 'padding')
            defaults = {'dilation': (1, (1, 1)), 'ceil_mode': (False,), 'return_indices': (False,), 'divisor_override': (None,),
                        'count_include_pad': (True, False)}
            if len(node.args) > 4 or any(k not in names and not (k in defaults and not isinstance(v, torch.fx.Node) and v in defaults[k])
                                         for k, v in node.kwargs.items()):
                return
            a = dict(zip(names, node.args), **{k: v for k, v in node.kwargs.items() if k in names})
            cfg = (a.get('kernel_size'), a.get('stride'), a.get('padding', 0))
            if not isinstance(a.get('input'), torch.fx.Node) or any(isinstance(v, torch.fx.Node) for v in cfg):
                return
            if node.target is F.avg_pool2d and T._pair(cfg[2]) != (0, 0):      # (count_include_pad=True: not the kernel's average)
                return
            fn, kw = node.target, dict(kernel_size=cfg[0], stride=cfg[1], padding=cfg[2])
            self.put(NativePool(lambda t: fn(t, **kw), *cfg, 1 if fn is F.max_pool2d else 0), (a['input'],), node, (node,), 'pool')

    def head_window(self, node):
        """node: a Linear; its input flatten(global average pool(x), 1)."""
        fc = self.mod(node, nn.Linear)
        fl = self.input_of(node)
        gp = self.flattened(fl) if fc is not None else None
        if gp is None or len(gp.users) != 1:
            return
        size, stock = self.adaptive_pool(gp)
        if T._is_global_pool(stock) if isinstance(stock, nn.Module) else size in (1, (1, 1), [1, 1]):
            self.put(NativeHead(fc), (self.input_of(gp),), node, (node, fl, gp), 'head', nhwc=False)

    # ---- the opt-in windows of biased convolutions (biased=True) ----
    def biased_result(self, node):
        """node is the result of a Conv2d with a bias the kernels take, read by one node only."""
        conv = self.mod(node, nn.Conv2d) if isinstance(node, torch.fx.Node) else None
        return conv is not None and conv.bias is not None and conv_refusal(conv, biased=True) is None and len(node.users) == 1

    def bias_window(self, c, conv):
        """A Conv2d with a bias: with its ReLU, with a skip add and the ReLU behind it (the operand rules of conv_window), or alone."""
        why = conv_refusal(conv, biased=True)
        x = self.input_of(c)
        if why is None and not isinstance(x, torch.fx.Node):
            why = 'its input is not a node of the graph'
        if why is not None:
            self.stock[c.target] = why
            return
        nxt = next(iter(c.users)) if len(c.users) == 1 else None
        if nxt is not None and self.is_relu(nxt) and self.input_of(nxt) is c:
            self.put(NativeConvWindow(conv, relu=True), (x,), nxt, (nxt, c), 'conv_bias_relu')
            return
        skip = self.skip_add(c, nxt, self.biased_result) if nxt is not None and self.is_add(nxt) else None
        if skip:
            self.put(NativeConvWindow(conv, relu=True), (x, skip[0]), skip[1], (skip[1], nxt, c), 'conv_bias_add_relu')
        else:
            self.put(NativeConvWindow(conv), (x,), c, (c,), 'conv_bias')

    def mlp_head_window(self, node):
        """node: a Linear whose input is flatten(x, 1); behind it (ReLU, Dropout, Linear) one to three times, one user each."""
        first = self.mod(node, nn.Linear)
        fl = self.input_of(node)
        x = self.flattened(fl) if first is not None else None
        if x is None:
            return
        modules, nodes, last = [first], [node, fl], node
        while len(modules) < 3 * T.HEAD_MAX_LINEAR - 2:
            trio, at = [], last
            for cls in (nn.ReLU, nn.Dropout, nn.Linear):
                nxt = next(iter(at.users)) if len(at.users) == 1 else None
                if nxt is None or self.mod(nxt, cls) is None or self.input_of(nxt) is not at:
                    break
                trio.append(nxt)
                at = nxt
            if len(trio) != 3:
                break
            modules += [self.mods[n.target] for n in trio]
            nodes = trio[::-1] + nodes
            last = trio[-1]
        if len(modules) >= 4:
            self.put(NativeMlpHead(modules), (x,), last, tuple(nodes), 'mlp_head', nhwc=False)

    def same_size_pool_window(self, node):
        x, (size, stock) = self.input_of(node), self.adaptive_pool(node)
        if isinstance(size, int):
            size = (size, size)
        if not (isinstance(x, torch.fx.Node) and isinstance(size, (tuple, list)) and len(size) == 2 and
                all(isinstance(v, int) for v in size)) or tuple(size) == (1, 1):
            return
        # (the result may be the input itself, channels_last from a native node: a stock reader gets it converted)
        self.put(NativeSameSizePool(stock, tuple(size)), (x,), node, (node,), 'same_size_pool')

    # ---- the opt-in windows (windows='all') ----
    def bn_window(self, b):
        """A BatchNorm2d the conv pass left: with its ReLU when that is its only user, else alone."""
        bn, x = self.mod(b, nn.BatchNorm2d), self.input_of(b)
        if bn is None or not isinstance(x, torch.fx.Node):
            return
        users = list(b.users)
        if len(users) == 1 and self.is_relu(users[0]) and self.input_of(users[0]) is b:
            self.put(NativeBnAct(bn, True), (x,), users[0], (users[0], b), 'bn_relu')
        else:
            self.put(NativeBnAct(bn, False), (x,), b, (b,), 'bn')

    def bare_conv_window(self, c):
        """A Conv2d the dense kernels take that the first pass left -- not followed by a norm layer (the end of a dense layer, of
        a transition, of a pre-activation block), several users (a stem whose result is also a skip operand), a norm layer with
        several users --: it leaves the stock list."""
        conv, x = self.mod(c, nn.Conv2d), self.input_of(c)
        if conv is not None and conv_refusal(conv) is None and isinstance(x, torch.fx.Node):
            self.stock.pop(c.target, None)
            self.put(NativeConvWindow(conv), (x,), c, (c,), 'conv')

    def concat_window(self, node):
        if not ((node.op == 'call_function' and node.target in (torch.cat, torch.concat)) and node.args):
            return
        parts = node.args[0]
        dim = node.args[1] if len(node.args) > 1 else node.kwargs.get('dim', 0)
        if len(node.args) > 2 or set(node.kwargs) - {'dim'} or dim != 1 or not isinstance(parts, (list, tuple)):
            return
        if 2 <= len(parts) <= T.JOIN_MAX_SLICES and all(isinstance(p, torch.fx.Node) for p in parts):
            self.put(NativeConcat(), tuple(parts), node, (node,), 'concat')

    def add_window(self, node):
        if not self.is_add(node):
            return
        in_place = node.target in (operator.iadd, 'add_')
        if in_place and len(node.args[0].users) != 1:      # (its other readers see the sum: the call stays what it is)
            return
        self.put(NativeAdd(), tuple(node.args), node, (node,), 'add')

    def run(self):
        # (every window method looks at any node and returns where it is not the one the window starts from)
        passes = ((True, self.conv_window),
                  (self.extra, self.bn_window), (self.extra, self.bare_conv_window), (self.extra, self.concat_window),
                  (self.extra, self.add_window),
                  (True, self.pool_window), (True, self.head_window),
                  (self.biased, self.mlp_head_window), (self.biased, self.same_size_pool_window))
        for on, window in passes:
            for node in list(self.graph.nodes) if on else ():
                if node not in self.native:
                    window(node)
        # a stock node (the output included) reads a native node's result NCHW-contiguous; the head reads either layout
        for node in list(self.nhwc):
            readers = [u for u in node.users if u not in self.native]
            if readers:
                with self.graph.inserting_after(node):
                    plain = self.graph.call_function(_stock_layout, (node,))
                for u in readers:
                    u.replace_input_with(node, plain)
        self.graph.lint()
        self.gm.recompile()
        return NativeReport(traced=True, windows=self.windows, stock_convs=self.stock)


def nativize(model, strict=False, windows='resnet', biased=False):
    """`model` (a torch.nn.Module) with its conv -> norm [-> add] -> ReLU, pooling and head windows on the native nodes: a
    torch.fx.GraphModule over the SAME submodules, Parameters and buffers, with `report()`.  A model torch.fx cannot trace (data-
    dependent control flow) is returned unchanged and the reason logged; strict=True raises instead.  windows='all' adds the
    opt-in windows of pre-activation and densely connected networks (the module text; EXTRA_KINDS in the report); biased=True
    those of convolutions with a bias and of the flatten -> MLP classifier (BIAS_KINDS)."""
    if windows not in ('resnet', 'all'):
        raise ValueError("windows is 'resnet' or 'all', not %r" % (windows,))
    try:
        gm = torch.fx.symbolic_trace(model)
    except Exception as e:                                  # (torch.fx raises TraceError, TypeError, ... depending on the construct)
        if strict:
            raise
        log('nativize: %s cannot be traced (%s: %s): it stays on the stock layers'
            % (type(model).__name__, type(e).__name__, str(e).splitlines()[0] if str(e) else ''))
        return model
    report = _Matcher(gm, extra=windows == 'all', biased=bool(biased)).run()
    gm.report = lambda: report
    return gm
