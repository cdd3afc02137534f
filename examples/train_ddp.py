#!/usr/bin/env python3
"""
Counterpart of the reference's train_ddp.py without the image files (none are available offline): one plain network, its initial
parameters predicted by a GHN-3 checkpoint (--ckpt) plus a little noise (--beta), fine-tuned with SGD through
``ghn3_amd.Trainer`` -- the same call sequence (``update`` / ``log`` / ``save`` / ``scheduler_step``) -- on seeded random images.

    python examples/train_ddp.py --ckpt ghn3xlm16.pt [--lr 0.025] [--wd 3e-5] [--momentum 0.9] [--label_smooth 0.1]
                                 [--beta 1e-5] [--amp] [--arch resnet|densenet|preact|vgg|genotype] [--steps 30] [--epochs 2]
                                 [--save DIR] [--native-layers] [--native-windows resnet|all] [--native-biased]

Without --ckpt the network keeps its own initialisation.  The optimizer step is the fused multi-tensor SGD (ghn3_amd.FusedSGD);
GHN3_FUSED_SGD=0 runs stock clip_grad_norm_ + torch.optim.SGD instead.

Data parallel, like the reference's recipes, under torchrun (one process per GPU):

    torchrun --standalone --nproc_per_node=4 examples/train_ddp.py --ckpt ghn3xlm16.pt ...

Rank 0's parameters and buffers become every rank's, each rank draws its own images (seed + 1 + rank, standing in for
DistributedSampler's shards; --batch-size is per rank), the gradients are averaged through one flat buffer inside the optimizer
step (Trainer(..., data_parallel=True)), and rank 0 logs and saves.  Without torchrun the script is the one-GPU run it always was.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        y = self.bn2(self.conv2(F.relu(self.bn1(self.conv1(x)))))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)))


class SmallResNet(nn.Module):
    """A ResNet-18-shaped network for 32 x 32 images at a quarter of the width."""

    def __init__(self, num_classes=10, width=16):
        super().__init__()
        self.conv1 = nn.Conv2d(3, width, 3, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        layers, cin = [], width
        for i, cout in enumerate((width, 2 * width, 4 * width, 8 * width)):
            layers += [Block(cin, cout, 1 if i == 0 else 2), Block(cout, cout, 1)]
            cin = cout
        self.layers = nn.Sequential(*layers)
        self.fc = nn.Linear(cin, num_classes)

    def forward(self, x):
        x = self.layers(F.relu(self.bn1(self.conv1(x))))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


class DenseLayer(nn.Module):
    def __init__(self, cin, growth, bn_size=4):
        super().__init__()
        self.norm1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, bn_size * growth, 1, bias=False)
        self.norm2 = nn.BatchNorm2d(bn_size * growth)
        self.conv2 = nn.Conv2d(bn_size * growth, growth, 3, 1, 1, bias=False)

    def forward(self, x):
        y = self.conv1(F.relu(self.norm1(x)))
        return torch.cat([x, self.conv2(F.relu(self.norm2(y)))], 1)


class Transition(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.norm = nn.BatchNorm2d(cin)
        self.conv = nn.Conv2d(cin, cout, 1, bias=False)

    def forward(self, x):
        return F.avg_pool2d(self.conv(F.relu(self.norm(x))), 2)


class SmallDenseNet(nn.Module):
    """A DenseNet-BC for 32 x 32 images: three dense blocks of four bottleneck layers (growth 16: every channel count a multiple
    of four, as the native nodes ask), transitions that halve the channels.  Its BatchNorm layers lead their convolutions:
    --native-windows all puts them on the native nodes."""

    def __init__(self, num_classes=10, growth=16, layers=4):
        super().__init__()
        c = 2 * growth
        self.conv0 = nn.Conv2d(3, c, 3, 1, 1, bias=False)
        stages = []
        for i in range(3):
            for _ in range(layers):
                stages.append(DenseLayer(c, growth))
                c += growth
            if i < 2:
                stages.append(Transition(c, c // 2))
                c //= 2
        self.features = nn.Sequential(*stages)
        self.norm = nn.BatchNorm2d(c)
        self.fc = nn.Linear(c, num_classes)

    def forward(self, x):
        x = F.relu(self.norm(self.features(self.conv0(x))))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


class PreActBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.bn1 = nn.BatchNorm2d(cin)
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.shortcut = nn.Conv2d(cin, cout, 1, stride, bias=False) if (stride != 1 or cin != cout) else None

    def forward(self, x):
        o = F.relu(self.bn1(x))
        skip = x if self.shortcut is None else self.shortcut(o)
        return self.conv2(F.relu(self.bn2(self.conv1(o)))) + skip


class SmallPreActResNet(nn.Module):
    """A pre-activation (v2) ResNet-18-shaped network for 32 x 32 images at a quarter of the width."""

    def __init__(self, num_classes=10, width=16):
        super().__init__()
        self.conv1 = nn.Conv2d(3, width, 3, 1, 1, bias=False)
        layers, cin = [], width
        for i, cout in enumerate((width, 2 * width, 4 * width, 8 * width)):
            layers += [PreActBlock(cin, cout, 1 if i == 0 else 2), PreActBlock(cout, cout, 1)]
            cin = cout
        self.layers = nn.Sequential(*layers)
        self.bn = nn.BatchNorm2d(cin)
        self.fc = nn.Linear(cin, num_classes)

    def forward(self, x):
        x = F.relu(self.bn(self.layers(self.conv1(x))))
        return self.fc(torch.flatten(F.adaptive_avg_pool2d(x, 1), 1))


class SmallVgg(nn.Module):
    """A VGG-shaped network for 32 x 32 images: biased 3 x 3 convolutions (nn.Conv2d's default) each followed by a ReLU, no norm
    layers, max pooling between the stages, the classifier Linear-ReLU-Dropout x 2, Linear.  Every convolution has a bias:
    --native-biased (with --native-layers) puts them, and the classifier, on the native nodes."""

    def __init__(self, num_classes=10, width=32, hidden=256):
        super().__init__()
        layers, cin = [], 3
        for stage, n in enumerate((1, 1, 2, 2)):
            for _ in range(n):
                layers += [nn.Conv2d(cin, width << stage, 3, 1, 1), nn.ReLU(inplace=True)]
                cin = width << stage
            layers.append(nn.MaxPool2d(2, 2))
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((2, 2))
        self.classifier = nn.Sequential(nn.Linear(cin * 4, hidden), nn.ReLU(inplace=True), nn.Dropout(0.5),
                                        nn.Linear(hidden, hidden), nn.ReLU(inplace=True), nn.Dropout(0.5),
                                        nn.Linear(hidden, num_classes))

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


PLAIN_NETWORKS = {'resnet': SmallResNet, 'densenet': SmallDenseNet, 'preact': SmallPreActResNet, 'vgg': SmallVgg}


def genotype_network(num_classes):
    """A DARTS-style network of the DeepNets-1M search space on the native layers (ghn3_amd.ops.Network)."""
    from ghn3_amd import ops
    geno = ops.Genotype(normal=[('sep_conv_3x3', 0), ('sep_conv_3x3', 1), ('skip_connect', 0), ('conv_1x1', 2)],
                        normal_concat=[2, 3],
                        reduce=[('max_pool_3x3', 0), ('sep_conv_3x3', 1), ('skip_connect', 2), ('avg_pool_3x3', 0)],
                        reduce_concat=[2, 3])
    return ops.Network(genotype=geno, C=16, num_classes=num_classes, n_cells=5, is_imagenet_input=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ckpt', default=None, help='GHN-3 checkpoint that predicts the initial parameters')
    ap.add_argument('--arch', choices=('resnet', 'densenet', 'preact', 'vgg', 'genotype'), default='resnet')
    ap.add_argument('--lr', type=float, default=0.025)
    ap.add_argument('--wd', type=float, default=3e-5)
    ap.add_argument('--momentum', type=float, default=0.9)
    ap.add_argument('--label_smooth', type=float, default=0.1)
    ap.add_argument('--beta', type=float, default=1e-5, help='standard deviation of the noise added to the predicted parameters')
    ap.add_argument('--amp', action='store_true')
    ap.add_argument('--batch-size', type=int, default=64)
    ap.add_argument('--steps', type=int, default=30, help='steps per epoch')
    ap.add_argument('--epochs', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--save', default=None)
    ap.add_argument('--native-layers', action='store_true',
                    help='run the conv-norm-ReLU, pooling and head layers on the native nodes (ghn3_amd.nativize)')
    ap.add_argument('--native-windows', choices=('resnet', 'all'), default=None,
                    help="which windows --native-layers takes; 'all' (implies --native-layers) adds the stand-alone BatchNorm, bare "
                         'convolutions, concatenations and sums of pre-activation and densely connected networks')
    ap.add_argument('--native-biased', action='store_true',
                    help='with --native-layers: also take the convolutions that have a bias, and a flatten -> MLP classifier '
                         '(nativize(biased=True); --arch vgg)')
    args = ap.parse_args()
    native = 'all' if args.native_windows == 'all' else bool(args.native_layers or args.native_windows)

    from ghn3_amd import Trainer, log, setup_ddp, clean_ddp
    ddp = setup_ddp()                      # (under torchrun: the process group, device = cuda:LOCAL_RANK; else rank 0 of 1)
    torch.manual_seed(args.seed)
    num_classes = 10
    model = PLAIN_NETWORKS[args.arch](num_classes) if args.arch in PLAIN_NETWORKS else genotype_network(num_classes)
    trainer = Trainer(model, opt='sgd', opt_args={'lr': args.lr, 'weight_decay': args.wd, 'momentum': args.momentum},
                      scheduler='cosine', n_batches=args.steps, grad_clip=5, device=ddp.device, log_interval=10,
                      label_smoothing=args.label_smooth, save_dir=args.save, ckpt=args.ckpt, epochs=args.epochs, amp=args.amp,
                      beta=args.beta, native_layers=native, data_parallel=ddp.ddp, native_biased=args.native_biased)
    log('training %s (%d parameters in %d tensors), %d x %d images per step'
        % (type(model).__name__, sum(p.numel() for p in model.parameters()), len(list(model.parameters())), args.batch_size, 32))
    report = getattr(trainer._plain_forward_model(), 'report', None) if native else None
    if report is not None:
        log('native windows:\n%s' % report())
    gen = torch.Generator().manual_seed(args.seed + 1 + ddp.rank)
    images = torch.randn(args.batch_size, 3, 32, 32, generator=gen).to(ddp.device)
    targets = torch.randint(0, num_classes, (args.batch_size,), generator=gen).to(ddp.device)
    t0, n_timed = None, 0
    for epoch in range(trainer.start_epoch, args.epochs):
        trainer.reset_metrics(epoch)
        for step in range(trainer.start_step, args.steps):
            if t0 is None and step == min(3, args.steps - 1):
                torch.cuda.synchronize()
                t0, n_timed = time.perf_counter(), 0
            trainer.update(images, targets)
            trainer.log(step)              # (on every rank -- its check of skipped steps moves the loss scale; rank 0 prints)
            n_timed += 1
            if args.save:
                trainer.save(epoch, step, {})
        trainer.scheduler_step()
    torch.cuda.synchronize()
    if t0 is not None and n_timed:
        log('%.2f ms per step over %d steps; %d updates skipped'
            % (1e3 * (time.perf_counter() - t0) / n_timed, n_timed, trainer.skipped_updates))
    if ddp.ddp:
        trainer._sync_skips()
        log('final loss %.4f on %d ranks; %d updates skipped'
            % (trainer.metrics.avg()['loss'], ddp.world_size, trainer.skipped_updates))
    clean_ddp()


if __name__ == '__main__':
    main()
