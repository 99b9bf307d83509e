"""Synthetic-weight model definitions for the BASELINE.json configs (no torchvision here).

Only shapes matter: the configs use random-init weights and synthetic data.  ResNet-18 follows the
CIFAR layout named in SURVEY.md §8 (3x3 stride-1 stem, no max-pool, BasicBlock x [2,2,2,2]); its
BatchNorm affine parameters are frozen by default because the reference's KFAC path supports nn.Linear /
nn.Conv2d only (docs/index.md:364-366; baselaplace.py:115-125 treats frozen params as non-Laplace).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F
from torch import nn


NORM_LAYERS = (nn.BatchNorm2d, nn.GroupNorm)


def norm_layer(norm: str, channels: int) -> nn.Module:
    """``"bn"``: ``BatchNorm2d``; ``"gn"``: ``GroupNorm(32, channels)`` (the usual BatchNorm-free ResNet of Bayesian deep learning)"""
    if norm == "bn":
        return nn.BatchNorm2d(channels)
    if norm == "gn":
        return nn.GroupNorm(32, channels)
    raise ValueError(f"norm must be 'bn' or 'gn', got {norm!r}")


class BasicBlock(nn.Module):
    def __init__(self, cin: int, cout: int, stride: int, act=torch.relu, norm: str = "bn"):
        super().__init__()
        self.act = act
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = norm_layer(norm, cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = norm_layer(norm, cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), norm_layer(norm, cout))

    def forward(self, x):
        out = self.act(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.act(out + (x if self.downsample is None else self.downsample(x)))


class ResNet18(nn.Module):
    """``act`` defaults to ReLU (the benchmark model).  Tests that compare two *separately executed*
    forward/backward passes use a smooth activation: with ReLU, fp32 rounding differences between MIOpen
    solvers flip a handful of pre-activations that sit within 1e-6 of zero, which changes individual
    gradients by O(1) and is a property of the host framework, not of the curvature kernels.

    ``freeze_bn=True`` is needed for KFAC only (the reference has no Kronecker factors for normalisation parameters and
    refuses them, as this backend does).  With ``freeze_bn=False`` the 9 600 BatchNorm weights and biases are Laplace
    parameters like any other: ``jacobians`` / ``diag`` / ``full`` / the EF / the diagonal predictive serve them on the
    device in eval mode (csrc/lk_norm.hip).

    ``norm="gn"`` puts ``GroupNorm(32, C)`` wherever a BatchNorm is (same attribute names; ``freeze_bn`` freezes its affine
    parameters alike).  Its reverse sweep goes through csrc/lk_normvjp.hip.

    ``stem="imagenet"`` is the torchvision stem - a 7 x 7 stride-2 convolution, norm, activation, ``MaxPool2d(3, 2, 1)`` - in
    front of the same blocks (the pool runs through csrc/lk_pool.hip); the default ``"cifar"`` is the 3 x 3 stride-1 stem
    without a pool."""

    def __init__(self, num_classes: int = 10, freeze_bn: bool = True, act=torch.relu, norm: str = "bn", stem: str = "cifar"):
        super().__init__()
        if stem not in ("cifar", "imagenet"):
            raise ValueError(f"stem must be 'cifar' or 'imagenet', got {stem!r}")
        self.act = act
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False) if stem == "imagenet" else nn.Conv2d(3, 64, 3, 1, 1, bias=False)
        self.bn1 = norm_layer(norm, 64)
        self.maxpool = nn.MaxPool2d(3, 2, 1) if stem == "imagenet" else None
        blocks, cin = [], 64
        for cout, stride in ((64, 1), (64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1)):
            blocks.append(BasicBlock(cin, cout, stride, act, norm))
            cin = cout
        self.layers = nn.Sequential(*blocks)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(512, num_classes)
        if freeze_bn:
            for m in self.modules():
                if isinstance(m, NORM_LAYERS):
                    m.weight.requires_grad_(False)
                    m.bias.requires_grad_(False)

    def forward(self, x):
        x = self.act(self.bn1(self.conv1(x)))
        if self.maxpool is not None:
            x = self.maxpool(x)
        x = self.layers(x)
        return self.fc(torch.flatten(self.pool(x), 1))


def lenet5(num_classes: int = 10) -> nn.Sequential:
    """Config c2: LeNet-5 on 3x32x32 inputs."""
    return nn.Sequential(
        nn.Conv2d(3, 6, 5), nn.Tanh(), nn.MaxPool2d(2), nn.Conv2d(6, 16, 5), nn.Tanh(), nn.MaxPool2d(2),
        nn.Flatten(), nn.Linear(400, 120), nn.Tanh(), nn.Linear(120, 84), nn.Tanh(), nn.Linear(84, num_classes),
    )


def mlp_1_50_1() -> nn.Sequential:
    """Config c1 (examples/regression_example.py:17-21 of the reference)."""
    return nn.Sequential(nn.Linear(1, 50), nn.Tanh(), nn.Linear(50, 1))


class InvertedResidual(nn.Module):
    """MobileNetV2 block: 1x1 expansion (skipped at ``expand = 1``), depthwise 3x3, linear 1x1 projection; identity shortcut
    when the shape is kept.  None of its convolutions has a bias."""

    def __init__(self, cin: int, cout: int, stride: int, expand: int, act=nn.ReLU6):
        super().__init__()
        hidden = cin * expand
        layers = []
        if expand != 1:
            layers += [nn.Conv2d(cin, hidden, 1, bias=False), nn.BatchNorm2d(hidden), act()]
        layers += [nn.Conv2d(hidden, hidden, 3, stride, 1, groups=hidden, bias=False), nn.BatchNorm2d(hidden), act(),
                   nn.Conv2d(hidden, cout, 1, bias=False), nn.BatchNorm2d(cout)]
        self.block = nn.Sequential(*layers)
        self.use_res = stride == 1 and cin == cout

    def forward(self, x):
        return x + self.block(x) if self.use_res else self.block(x)


class MobileNetV2Small(nn.Module):
    """A small MobileNetV2-style network for 3 x 32 x 32 inputs (3x3 stride-1 stem, nine inverted residuals, 1x1 head
    convolution, pool, linear): the workload of the grouped-convolution route (csrc/lk_gconv.hip).  Its depthwise layers
    have no Kronecker factors here (``kron`` refuses them by name); ``jacobians`` / ``diag`` / ``full`` / the EF / the
    diagonal predictive serve every parameter, BatchNorm included, on the device in eval mode.

    ``width`` scales every channel count (multiples of 8 are kept); ``act`` is the activation module's class - tests that
    compare two separately executed passes use a smooth one, as with :class:`ResNet18`."""

    #: (expansion, output channels, blocks, stride of the first block)
    SETTINGS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 2, 2), (6, 64, 2, 2), (6, 96, 1, 1), (6, 160, 1, 1))

    def __init__(self, num_classes: int = 10, width: float = 1.0, freeze_bn: bool = False, act=nn.ReLU6):
        super().__init__()

        def ch(c):
            return max(8, int(c * width + 4) // 8 * 8)

        cin = ch(32)
        self.stem = nn.Sequential(nn.Conv2d(3, cin, 3, 1, 1, bias=False), nn.BatchNorm2d(cin), act())
        blocks = []
        for t, c, n, s in self.SETTINGS:
            for i in range(n):
                blocks.append(InvertedResidual(cin, ch(c), s if i == 0 else 1, t, act))
                cin = ch(c)
        self.layers = nn.Sequential(*blocks)
        self.head = nn.Sequential(nn.Conv2d(cin, ch(320), 1, bias=False), nn.BatchNorm2d(ch(320)), act())
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(ch(320), num_classes)
        if freeze_bn:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.weight.requires_grad_(False)
                    m.bias.requires_grad_(False)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(self.head(self.layers(self.stem(x)))), 1))


class MobileNetV1(nn.Module):
    """A MobileNetV1-style network for 3 x 32 x 32 inputs: 3x3 stride-1 stem, thirteen depthwise-separable blocks (depthwise
    3x3, BatchNorm, activation, pointwise 1x1, BatchNorm, activation), pool, linear.  Every channel count is a multiple of 32
    (``ch(c) = max(32, int(c * width + 16) // 32 * 32)``), so the pointwise layers match the split-fp16 MFMA kernels and the
    depthwise layers can run through csrc/lk_dwconv.hip (``SplitSweep.nhwc_depthwise = True``): the workload of the depthwise route of the
    NHWC sweep.  No convolution
    has a bias.

    ``freeze_depthwise=True`` takes the depthwise weights out of the Laplace parameters: the supported way to run ``kron``, which
    has no rule for a grouped layer.  ``act`` is the activation module's class, as with :class:`MobileNetV2Small`."""

    #: (output channels, stride) of the separable blocks
    SETTINGS = ((64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1), (512, 1), (512, 1),
                (1024, 2), (1024, 1))

    def __init__(self, num_classes: int = 10, width: float = 1.0, freeze_bn: bool = True, freeze_depthwise: bool = False,
                 act=nn.ReLU):
        super().__init__()

        def ch(c):
            return max(32, int(c * width + 16) // 32 * 32)

        cin = ch(32)
        self.stem = nn.Sequential(nn.Conv2d(3, cin, 3, 1, 1, bias=False), nn.BatchNorm2d(cin), act())
        blocks = []
        for c, s in self.SETTINGS:
            blocks.append(nn.Sequential(nn.Conv2d(cin, cin, 3, s, 1, groups=cin, bias=False), nn.BatchNorm2d(cin), act(),
                                        nn.Conv2d(cin, ch(c), 1, bias=False), nn.BatchNorm2d(ch(c)), act()))
            cin = ch(c)
        self.layers = nn.Sequential(*blocks)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)
        for m in self.modules():
            if freeze_bn and isinstance(m, nn.BatchNorm2d):
                m.weight.requires_grad_(False)
                m.bias.requires_grad_(False)
            if freeze_depthwise and isinstance(m, nn.Conv2d) and m.groups != 1:
                m.weight.requires_grad_(False)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(self.layers(self.stem(x))), 1))


class DenseLayer(nn.Module):
    """DenseNet-BC layer: BN - act - 1x1 convolution (to ``4 * growth``) - BN - act - 3x3 convolution (to ``growth``), and the
    result concatenated behind the input along the channels"""

    def __init__(self, cin: int, growth: int, act=nn.ReLU):
        super().__init__()
        self.bn1, self.act1, self.conv1 = nn.BatchNorm2d(cin), act(), nn.Conv2d(cin, 4 * growth, 1, bias=False)
        self.bn2, self.act2 = nn.BatchNorm2d(4 * growth), act()
        self.conv2 = nn.Conv2d(4 * growth, growth, 3, 1, 1, bias=False)

    def forward(self, x):
        new = self.conv2(self.act2(self.bn2(self.conv1(self.act1(self.bn1(x))))))
        return torch.cat([x, new], 1)


class DenseNetSmall(nn.Module):
    """A CIFAR DenseNet-BC for 3 x 32 x 32 inputs: 3x3 stem convolution, dense blocks of :class:`DenseLayer` s joined by
    transitions (BN - act - 1x1 convolution - ``AvgPool2d(2)``; the width is half the input's, rounded down to a multiple of 32,
    at least 32), then BN - act - global average - flatten - ``Linear``.  Every channel count is a multiple of 32 when ``growth``
    and ``stem`` are, so every convolution matches the split-fp16 MFMA kernels; the concatenations run through csrc/lk_cat.hip
    and the transitions' pools through csrc/lk_pool.hip: the workload of the concatenation rule of both reverse sweeps.  No
    convolution has a bias.  ``act`` is the activation module's class, as with :class:`MobileNetV1`; ``freeze_bn`` as with
    :class:`ResNet18` (KFAC needs it)."""

    def __init__(self, num_classes: int = 10, growth: int = 32, blocks=(4, 4, 4), stem: int = 64, freeze_bn: bool = True,
                 act=nn.ReLU):
        super().__init__()
        self.conv1 = nn.Conv2d(3, stem, 3, 1, 1, bias=False)
        layers, cin = [], stem
        for i, n in enumerate(blocks):
            for _ in range(n):
                layers.append(DenseLayer(cin, growth, act))
                cin += growth
            if i + 1 < len(blocks):
                cout = max(32, cin // 2 // 32 * 32)
                layers.append(nn.Sequential(nn.BatchNorm2d(cin), act(), nn.Conv2d(cin, cout, 1, bias=False), nn.AvgPool2d(2)))
                cin = cout
        self.layers = nn.Sequential(*layers)
        self.bn, self.act = nn.BatchNorm2d(cin), act()
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)
        if freeze_bn:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.weight.requires_grad_(False)
                    m.bias.requires_grad_(False)

    def forward(self, x):
        x = self.layers(self.conv1(x))
        return self.fc(torch.flatten(self.pool(self.act(self.bn(x))), 1))


class AttentionBlock(nn.Module):
    """Pre-LN transformer block on ``[B, T, dim]``: ``x + proj(attention(LN(x)))`` then ``x + MLP(LN(x))``.  ``q`` / ``k`` /
    ``v`` / ``proj`` are separate ``nn.Linear`` layers (KFAC hangs its factors on them) and the attention core is
    ``F.scaled_dot_product_attention`` on ``Linear -> view -> transpose`` operands, which the seed-batched sweep serves
    (csrc/lk_attn.hip).  The head split reads ``x.size(..)``: ``.shape[..]`` does not trace to a served node."""

    def __init__(self, dim: int, heads: int, mlp_ratio: float = 4.0, act=nn.GELU, causal: bool = False):
        super().__init__()
        if dim % heads:
            raise ValueError(f"heads ({heads}) must divide dim ({dim})")
        self.heads, self.causal = heads, causal
        self.norm1 = nn.LayerNorm(dim)
        self.q, self.k, self.v, self.proj = (nn.Linear(dim, dim) for _ in range(4))
        self.norm2 = nn.LayerNorm(dim)
        hidden = int(dim * mlp_ratio)
        self.fc1, self.act, self.fc2 = nn.Linear(dim, hidden), act(), nn.Linear(hidden, dim)

    def forward(self, x):
        B, T = x.size(0), x.size(1)
        h = self.norm1(x)
        q = self.q(h).view(B, T, self.heads, -1).transpose(1, 2)
        k = self.k(h).view(B, T, self.heads, -1).transpose(1, 2)
        v = self.v(h).view(B, T, self.heads, -1).transpose(1, 2)
        a = nn.functional.scaled_dot_product_attention(q, k, v, is_causal=self.causal)
        x = x + self.proj(a.transpose(1, 2).reshape(B, T, -1))
        return x + self.fc2(self.act(self.fc1(self.norm2(x))))


def sincos_positions(T: int, dim: int) -> torch.Tensor:
    """fixed sine-cosine positional table ``[1, T, dim]``"""
    pos = torch.arange(T, dtype=torch.float32).unsqueeze(1)
    freq = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * (-math.log(10000.0) / dim))
    table = torch.zeros(T, dim)
    table[:, 0::2] = torch.sin(pos * freq)
    table[:, 1::2] = torch.cos(pos * freq)[:, :dim // 2]
    return table.unsqueeze(0)


class ViTSmall(nn.Module):
    """Small vision transformer without a class token: ``Conv2d(3, dim, patch, patch)`` patch embedding, a fixed sin-cos
    positional buffer, ``depth`` pre-LN :class:`AttentionBlock` s, a final LayerNorm, the mean over the positions and a
    ``Linear`` head.  The defaults give ``T = 64`` positions and head dim 64.

    ``freeze_norm=True`` freezes the LayerNorm affines, which KFAC needs (it refuses tracked norm parameters, as with
    ``freeze_bn`` of :class:`ResNet18`); with ``freeze_norm=False``, ``diag`` / ``full`` / ``jacobians`` serve them through
    csrc/lk_norm.hip."""

    def __init__(self, num_classes: int = 10, image: int = 32, patch: int = 4, dim: int = 192, depth: int = 6, heads: int = 3,
                 act=nn.GELU, freeze_norm: bool = True, causal: bool = False):
        super().__init__()
        if image % patch:
            raise ValueError(f"patch ({patch}) must divide image ({image})")
        self.embed = nn.Conv2d(3, dim, patch, patch)
        self.register_buffer("pos", sincos_positions((image // patch) ** 2, dim))
        self.blocks = nn.ModuleList(AttentionBlock(dim, heads, act=act, causal=causal) for _ in range(depth))
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)
        if freeze_norm:
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    for p in m.parameters():
                        p.requires_grad_(False)

    def forward(self, x):
        x = self.embed(x).flatten(2).transpose(1, 2) + self.pos
        for blk in self.blocks:
            x = blk(x)
        return self.head(self.norm(x).mean(1))


class ViTStock(nn.Module):
    """:class:`ViTSmall`'s sizes built from PyTorch's own transformer: the patches (unfolded by a reshape) through a ``Linear``, a
    fixed sin-cos positional buffer, ``nn.TransformerEncoder`` of ``depth`` pre-norm GELU ``nn.TransformerEncoderLayer`` s
    (``batch_first``, dropout 0, no nested tensors) with a final LayerNorm, the mean over the positions and a ``Linear`` head.
    Each layer's ``nn.MultiheadAttention`` is served as the two Linear layers around its attention core (`laplace_amd.mha`): its
    packed projection is read where it lies (csrc/lk_attn.hip, the strided entry points).  ``freeze_norm=True`` freezes the
    LayerNorm affines, which KFAC needs."""

    def __init__(self, num_classes: int = 10, image: int = 32, patch: int = 4, dim: int = 192, depth: int = 6, heads: int = 3,
                 freeze_norm: bool = True):
        super().__init__()
        if image % patch:
            raise ValueError(f"patch ({patch}) must divide image ({image})")
        self.patch, self.grid = patch, image // patch
        self.embed = nn.Linear(3 * patch * patch, dim)
        self.register_buffer("pos", sincos_positions(self.grid ** 2, dim))
        layer = nn.TransformerEncoderLayer(dim, heads, 4 * dim, 0.0, "gelu", batch_first=True, norm_first=True)
        self.encoder = nn.TransformerEncoder(layer, depth, norm=nn.LayerNorm(dim), enable_nested_tensor=False)
        self.head = nn.Linear(dim, num_classes)
        if freeze_norm:
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    for p in m.parameters():
                        p.requires_grad_(False)

    def forward(self, x):
        p, g = self.patch, self.grid
        x = x.view(x.size(0), 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(x.size(0), g * g, 3 * p * p)
        return self.head(self.encoder(self.embed(x) + self.pos).mean(1))


class CSPBlock(nn.Module):
    """Residual block of a CSP stage: ``act(x + BN(conv3x3(act(BN(conv3x3(x))))))`` at constant width; no convolution has a bias"""

    def __init__(self, c: int, act=nn.ReLU):
        super().__init__()
        self.conv1, self.bn1, self.act1 = nn.Conv2d(c, c, 3, 1, 1, bias=False), nn.BatchNorm2d(c), act()
        self.conv2, self.bn2, self.act2 = nn.Conv2d(c, c, 3, 1, 1, bias=False), nn.BatchNorm2d(c), act()

    def forward(self, x):
        return self.act2(self.bn2(self.conv2(self.act1(self.bn1(self.conv1(x))))) + x)


class CSPStage(nn.Module):
    """Cross-stage-partial stage: the channels are split in two halves (``a, b = x.chunk(2, 1)``), ``b`` runs through ``depth``
    :class:`CSPBlock` s, the halves are concatenated again and mixed by a 1x1 convolution - BN - act transition"""

    def __init__(self, c: int, depth: int, act=nn.ReLU):
        super().__init__()
        if c % 2:
            raise ValueError(f"a CSP stage splits its width ({c}) in two halves")
        self.blocks = nn.Sequential(*(CSPBlock(c // 2, act) for _ in range(depth)))
        self.mix = nn.Sequential(nn.Conv2d(c, c, 1, bias=False), nn.BatchNorm2d(c), act())

    def forward(self, x):
        a, b = x.chunk(2, 1)
        return self.mix(torch.cat([a, self.blocks(b)], 1))


class CSPNetSmall(nn.Module):
    """A CIFAR CSP-ResNet for 3 x 32 x 32 inputs: 3x3 stem convolution - BN - act, one :class:`CSPStage` per entry of ``widths``
    joined by stride-2 3x3 convolution - BN - act down-sampling to the next width, then global average - flatten - ``Linear``.
    With the default widths every half is a multiple of 32, so every convolution matches the split-fp16 MFMA kernels; the channel
    splits run through csrc/lk_slice.hip and the concatenations through csrc/lk_cat.hip: the workload of the slicing rule of both
    reverse sweeps.  No convolution has a bias.  ``act`` and ``freeze_bn`` as with :class:`DenseNetSmall`."""

    def __init__(self, num_classes: int = 10, widths=(64, 128, 256), depth: int = 2, freeze_bn: bool = True, act=nn.ReLU):
        super().__init__()
        cin = widths[0]
        self.stem = nn.Sequential(nn.Conv2d(3, cin, 3, 1, 1, bias=False), nn.BatchNorm2d(cin), act())
        layers = []
        for i, c in enumerate(widths):
            if i:
                layers.append(nn.Sequential(nn.Conv2d(cin, c, 3, 2, 1, bias=False), nn.BatchNorm2d(c), act()))
            layers.append(CSPStage(c, depth, act))
            cin = c
        self.layers = nn.Sequential(*layers)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)
        if freeze_bn:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.weight.requires_grad_(False)
                    m.bias.requires_grad_(False)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(self.layers(self.stem(x))), 1))


class PackedAttentionBlock(nn.Module):
    """:class:`AttentionBlock` in the spelling of GPT-2 / nanoGPT: ONE packed projection ``qkv = nn.Linear(dim, 3 * dim)`` whose
    output is split with ``.split(dim, dim=2)`` (KFAC hangs one weight-sharing factor on it).  The three slices are served by the
    slicing rule of the seed-batched sweep; the attention operands it leaves are strided views, which the attention rule copies."""

    def __init__(self, dim: int, heads: int, mlp_ratio: float = 4.0, act=nn.GELU, causal: bool = False):
        super().__init__()
        if dim % heads:
            raise ValueError(f"heads ({heads}) must divide dim ({dim})")
        self.dim, self.heads, self.causal = dim, heads, causal
        self.norm1 = nn.LayerNorm(dim)
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim)
        hidden = int(dim * mlp_ratio)
        self.fc1, self.act, self.fc2 = nn.Linear(dim, hidden), act(), nn.Linear(hidden, dim)

    def forward(self, x):
        B, T = x.size(0), x.size(1)
        q, k, v = self.qkv(self.norm1(x)).split(self.dim, dim=2)
        q = q.view(B, T, self.heads, -1).transpose(1, 2)
        k = k.view(B, T, self.heads, -1).transpose(1, 2)
        v = v.view(B, T, self.heads, -1).transpose(1, 2)
        a = nn.functional.scaled_dot_product_attention(q, k, v, is_causal=self.causal)
        x = x + self.proj(a.transpose(1, 2).reshape(B, T, -1))
        return x + self.fc2(self.act(self.fc1(self.norm2(x))))


class ViTClassToken(nn.Module):
    """:class:`ViTSmall` as ViT / BERT classifiers are written: a FROZEN class token prepended to the patch sequence
    (``torch.cat([self.cls.expand(B, -1, -1), x], 1)``; a frozen ``nn.Parameter``, so that the tracer sees the ``expand``),
    ``depth`` :class:`PackedAttentionBlock` s, a final LayerNorm and the ``Linear`` head on the class token ``x[:, 0]``.  The
    defaults give ``T = 65`` positions and head dim 64.  ``freeze_norm`` as with :class:`ViTSmall`.

    ``train_tokens=True`` is the model as it is actually trained: the class token is trainable and the sin-cos buffer is replaced
    by a trainable position parameter (initialised to the same table).  Both are lone parameters: ``diag`` / ``full`` /
    ``jacobians`` serve them through the parameter rule of the seed-batched sweep; KFAC refuses them, as the reference does."""

    def __init__(self, num_classes: int = 10, image: int = 32, patch: int = 4, dim: int = 192, depth: int = 6, heads: int = 3,
                 act=nn.GELU, freeze_norm: bool = True, causal: bool = False, train_tokens: bool = False):
        super().__init__()
        if image % patch:
            raise ValueError(f"patch ({patch}) must divide image ({image})")
        self.embed = nn.Conv2d(3, dim, patch, patch)
        self.cls = nn.Parameter(torch.zeros(1, 1, dim).normal_(0.0, 0.02), requires_grad=bool(train_tokens))
        if train_tokens:
            self.pos = nn.Parameter(sincos_positions((image // patch) ** 2 + 1, dim))
        else:
            self.register_buffer("pos", sincos_positions((image // patch) ** 2 + 1, dim))
        self.blocks = nn.ModuleList(PackedAttentionBlock(dim, heads, act=act, causal=causal) for _ in range(depth))
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)
        if freeze_norm:
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    for p in m.parameters():
                        p.requires_grad_(False)

    def forward(self, x):
        x = self.embed(x).flatten(2).transpose(1, 2)
        x = torch.cat([self.cls.expand(x.size(0), -1, -1), x], 1) + self.pos
        for blk in self.blocks:
            x = blk(x)
        return self.head(self.norm(x)[:, 0])


class TextTransformer(nn.Module):
    """Token classifier on ids ``[B, T]`` (int64): ``nn.Embedding(vocab, dim, padding_idx)`` plus a learned ``[1, T, dim]``
    position parameter, ``depth`` pre-LN :class:`AttentionBlock` s, a final LayerNorm, the mean over the tokens and a ``Linear``
    head - the workload of the embedding route (csrc/lk_embed.hip, tools/embed_bench.py).

    ``freeze_embed=True`` freezes the embedding and the position table, which KFAC needs (it has no rule for either, as the
    reference); ``freeze_norm`` as with :class:`ViTSmall`."""

    def __init__(self, vocab: int = 1000, T: int = 64, dim: int = 192, depth: int = 6, heads: int = 3, num_classes: int = 10,
                 padding_idx: int | None = 0, act=nn.GELU, freeze_embed: bool = False, freeze_norm: bool = True,
                 causal: bool = False):
        super().__init__()
        self.embed = nn.Embedding(vocab, dim, padding_idx=padding_idx)
        self.pos = nn.Parameter(torch.zeros(1, T, dim).normal_(0.0, 0.02))
        self.blocks = nn.ModuleList(AttentionBlock(dim, heads, act=act, causal=causal) for _ in range(depth))
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)
        if freeze_embed:
            self.embed.weight.requires_grad_(False)
            self.pos.requires_grad_(False)
        if freeze_norm:
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    for p in m.parameters():
                        p.requires_grad_(False)

    def forward(self, ids):
        x = self.embed(ids) + self.pos
        for blk in self.blocks:
            x = blk(x)
        return self.head(self.norm(x).mean(1))


class SEBlock(nn.Module):
    """Squeeze-and-excitation gate: ``x * sigmoid(fc2(act(fc1(avgpool(x)))))`` with 1x1 convolutions on the pooled ``[B, C, 1, 1]``
    map (``C / reduction`` channels in between).  The product of the map with the ``[B, C, 1, 1]`` gate is the row-gate form of the
    product rule of the seed-batched sweep (csrc/lk_mul.hip)."""

    def __init__(self, c: int, reduction: int = 4, act=nn.ReLU):
        super().__init__()
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc1, self.act, self.fc2 = nn.Conv2d(c, max(c // reduction, 1), 1), act(), nn.Conv2d(max(c // reduction, 1), c, 1)
        self.gate = nn.Sigmoid()

    def forward(self, x):
        return x * self.gate(self.fc2(self.act(self.fc1(self.pool(x)))))


class SEBasicBlock(nn.Module):
    """:class:`BasicBlock` with an :class:`SEBlock` on the residual branch, before the add: ``act(se(bn2(conv2(..))) + shortcut)``"""

    def __init__(self, cin: int, cout: int, stride: int, reduction: int = 4, act=nn.ReLU):
        super().__init__()
        self.conv1, self.bn1, self.act1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False), nn.BatchNorm2d(cout), act()
        self.conv2, self.bn2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout)
        self.se, self.act2 = SEBlock(cout, reduction, act), act()
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        out = self.se(self.bn2(self.conv2(self.act1(self.bn1(self.conv1(x))))))
        return self.act2(out + (x if self.downsample is None else self.downsample(x)))


class SEResNetSmall(nn.Module):
    """A CIFAR SE-ResNet for 3 x 32 x 32 inputs: 3x3 stem convolution - BN - act, ``depth`` :class:`SEBasicBlock` s per entry of
    ``widths`` (stride 2 into every stage but the first), then global average - flatten - ``Linear``.  Eval-mode BatchNorm; the gate
    branches are 1x1 convolutions on 1x1 maps with ``width / reduction`` channels.  By default the model runs the NCHW sweep (the
    split sweep names the product): the workload of the row-gate form of the product rule.  With ``SplitSweep.nhwc_mul = True`` it
    stays on the NHWC split-fp16 walk: the gates run on csrc/lk_gate.hip and the gate branches on plain ``[B, C, 1, 1]`` tensors.
    ``act`` and ``freeze_bn`` as with :class:`DenseNetSmall`."""

    def __init__(self, num_classes: int = 10, widths=(32, 64, 128), depth: int = 2, reduction: int = 4, freeze_bn: bool = True,
                 act=nn.ReLU):
        super().__init__()
        cin = widths[0]
        self.stem = nn.Sequential(nn.Conv2d(3, cin, 3, 1, 1, bias=False), nn.BatchNorm2d(cin), act())
        blocks = []
        for i, c in enumerate(widths):
            for j in range(depth):
                blocks.append(SEBasicBlock(cin, c, 2 if i and j == 0 else 1, reduction, act))
                cin = c
        self.layers = nn.Sequential(*blocks)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)
        if freeze_bn:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    m.weight.requires_grad_(False)
                    m.bias.requires_grad_(False)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(self.layers(self.stem(x))), 1))


class SwiGLUBlock(nn.Module):
    """The pre-LN block of :class:`AttentionBlock` with the MLP replaced by the gated feed-forward of LLaMA / PaLM:
    ``x + w2(silu(w1(LN(x))) * w3(LN(x)))``.  The product of the two ``[B, T, hidden]`` branches is the full form of the product
    rule of the seed-batched sweep (csrc/lk_mul.hip).  ``hidden = round(dim * mlp_ratio)`` (8 / 3: the parameter count of a
    plain MLP of ratio 4)."""

    def __init__(self, dim: int, heads: int, mlp_ratio: float = 8.0 / 3.0, causal: bool = False):
        super().__init__()
        if dim % heads:
            raise ValueError(f"heads ({heads}) must divide dim ({dim})")
        self.heads, self.causal = heads, causal
        self.norm1 = nn.LayerNorm(dim)
        self.q, self.k, self.v, self.proj = (nn.Linear(dim, dim) for _ in range(4))
        self.norm2 = nn.LayerNorm(dim)
        hidden = int(round(dim * mlp_ratio))
        self.w1, self.w3, self.w2 = nn.Linear(dim, hidden), nn.Linear(dim, hidden), nn.Linear(hidden, dim)

    def forward(self, x):
        B, T = x.size(0), x.size(1)
        h = self.norm1(x)
        q = self.q(h).view(B, T, self.heads, -1).transpose(1, 2)
        k = self.k(h).view(B, T, self.heads, -1).transpose(1, 2)
        v = self.v(h).view(B, T, self.heads, -1).transpose(1, 2)
        a = nn.functional.scaled_dot_product_attention(q, k, v, is_causal=self.causal)
        x = x + self.proj(a.transpose(1, 2).reshape(B, T, -1))
        h = self.norm2(x)
        return x + self.w2(nn.functional.silu(self.w1(h)) * self.w3(h))


class ViTSwiGLU(nn.Module):
    """:class:`ViTSmall` with :class:`SwiGLUBlock` s: patch embedding, the fixed sin-cos positional buffer, ``depth`` blocks, a final
    LayerNorm, the mean over the positions and a ``Linear`` head.  The defaults give ``T = 64`` positions, head dim 64 and 512
    hidden units.  ``image`` is the side of a square image or ``(height, width)``.  ``freeze_norm`` as with :class:`ViTSmall`."""

    def __init__(self, num_classes: int = 10, image=32, patch: int = 4, dim: int = 192, depth: int = 6, heads: int = 3,
                 mlp_ratio: float = 8.0 / 3.0, freeze_norm: bool = True, causal: bool = False):
        super().__init__()
        ih, iw = image if isinstance(image, (tuple, list)) else (image, image)
        if ih % patch or iw % patch:
            raise ValueError(f"patch ({patch}) must divide image ({image})")
        self.embed = nn.Conv2d(3, dim, patch, patch)
        self.register_buffer("pos", sincos_positions((ih // patch) * (iw // patch), dim))
        self.blocks = nn.ModuleList(SwiGLUBlock(dim, heads, mlp_ratio, causal=causal) for _ in range(depth))
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)
        if freeze_norm:
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    for p in m.parameters():
                        p.requires_grad_(False)

    def forward(self, x):
        x = self.embed(x).flatten(2).transpose(1, 2) + self.pos
        for blk in self.blocks:
            x = blk(x)
        return self.head(self.norm(x).mean(1))


class EagerAttentionBlock(nn.Module):
    """:class:`AttentionBlock` with the attention core written out, as BERT, the annotated transformer and every model that inspects
    its attention maps spell it: ``softmax(q @ k^T / sqrt(head_dim) [+ bias]) @ v``.  The seed-batched sweep serves it with its
    matrix-product, scale and softmax rules (csrc/lk_matmul.hip, csrc/lk_softmax.hip); the ``[B, H, T, T]`` scores live in device
    memory.  ``bias``: an additive ``[1, H, T, T]`` tensor of the owner (a frozen relative-position table, a static mask), which
    ``F.scaled_dot_product_attention``'s rule refuses.  ``head_dim`` is a Python int, so the scale is a number of the traced graph;
    it is spelled ``/ math.sqrt(d)`` (``* d ** -0.5`` is a product with a number, which the sweep refuses).
    ``softmax_module=True`` spells the softmax ``nn.Softmax(-1)``, else ``.softmax(-1)``."""

    def __init__(self, dim: int, heads: int, mlp_ratio: float = 4.0, act=nn.GELU, softmax_module: bool = True):
        super().__init__()
        if dim % heads:
            raise ValueError(f"heads ({heads}) must divide dim ({dim})")
        self.heads, self.head_dim = heads, dim // heads
        self.norm1 = nn.LayerNorm(dim)
        self.q, self.k, self.v, self.proj = (nn.Linear(dim, dim) for _ in range(4))
        self.softmax = nn.Softmax(-1) if softmax_module else None
        self.norm2 = nn.LayerNorm(dim)
        hidden = int(dim * mlp_ratio)
        self.fc1, self.act, self.fc2 = nn.Linear(dim, hidden), act(), nn.Linear(hidden, dim)

    def forward(self, x, bias=None):
        B, T = x.size(0), x.size(1)
        h = self.norm1(x)
        q = self.q(h).view(B, T, self.heads, -1).transpose(1, 2)
        k = self.k(h).view(B, T, self.heads, -1).transpose(1, 2)
        v = self.v(h).view(B, T, self.heads, -1).transpose(1, 2)
        scores = q @ k.transpose(-2, -1) / math.sqrt(self.head_dim)
        if bias is not None:
            scores = scores + bias
        p = self.softmax(scores) if self.softmax is not None else scores.softmax(-1)
        x = x + self.proj((p @ v).transpose(1, 2).reshape(B, T, -1))
        return x + self.fc2(self.act(self.fc1(self.norm2(x))))


class ViTEager(nn.Module):
    """:class:`ViTSmall` with :class:`EagerAttentionBlock` s (the defaults give ``T = 64`` positions, 3 heads of dim 64).
    ``rel_bias=True`` adds a frozen relative-position buffer ``[1, heads, T, T]`` (a Swin-style table over the offsets of the
    patch grid, fixed at construction) to the scores of every block - what the fused attention rule cannot serve.  ``image`` is the
    side of a square image or ``(height, width)``.  ``freeze_norm`` as with :class:`ViTSmall`."""

    def __init__(self, num_classes: int = 10, image=32, patch: int = 4, dim: int = 192, depth: int = 6, heads: int = 3,
                 act=nn.GELU, freeze_norm: bool = True, rel_bias: bool = True, softmax_module: bool = True):
        super().__init__()
        ih, iw = image if isinstance(image, (tuple, list)) else (image, image)
        if ih % patch or iw % patch:
            raise ValueError(f"patch ({patch}) must divide image ({image})")
        gh, gw = ih // patch, iw // patch
        self.embed = nn.Conv2d(3, dim, patch, patch)
        self.register_buffer("pos", sincos_positions(gh * gw, dim))
        self.blocks = nn.ModuleList(EagerAttentionBlock(dim, heads, act=act, softmax_module=softmax_module) for _ in range(depth))
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)
        if rel_bias:
            ys, xs = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
            dy = ys.reshape(-1, 1) - ys.reshape(1, -1) + gh - 1
            dx = xs.reshape(-1, 1) - xs.reshape(1, -1) + gw - 1
            table = torch.randn(heads, (2 * gh - 1) * (2 * gw - 1)) * 0.2
            self.register_buffer("rel_bias", table[:, dy * (2 * gw - 1) + dx].unsqueeze(0).contiguous())
        else:
            self.rel_bias = None
        if freeze_norm:
            for m in self.modules():
                if isinstance(m, nn.LayerNorm):
                    for p in m.parameters():
                        p.requires_grad_(False)

    def forward(self, x):
        x = self.embed(x).flatten(2).transpose(1, 2) + self.pos
        for blk in self.blocks:
            x = blk(x, self.rel_bias)
        return self.head(self.norm(x).mean(1))


def rope_tables(T: int, d: int, base: float = 10000.0):
    """``(cos, sin)``, each ``[T, d]``, of a rotary position embedding in the rotate-half convention (LLaMA, GPT-NeoX): the angle
    of position ``t`` and channel pair ``(i, i + d / 2)`` is ``t * base ** (-2 i / d)``"""
    if d % 2:
        raise ValueError(f"rotary embeddings need an even head dim, got {d}")
    inv = base ** (-torch.arange(0, d, 2, dtype=torch.float32) / d)
    ang = torch.arange(T, dtype=torch.float32).unsqueeze(1) * inv.unsqueeze(0)
    ang = torch.cat((ang, ang), -1)
    return ang.cos(), ang.sin()


class LlamaBlock(nn.Module):
    """The block of LLaMA / Mistral / Gemma: RMSNorm pre-norms, rotary position embeddings on ``q`` and ``k``, causal
    ``scaled_dot_product_attention`` and the SwiGLU feed-forward of :class:`SwiGLUBlock`, no biases.  The rotary embedding is
    written the usual way, ``x * cos + cat((-x[..., half:], x[..., :half]), -1) * sin`` with non-persistent ``cos`` / ``sin``
    buffers ``[T, head_dim]``: the seed-batched sweep serves it with its slice, negation, concatenation, product and add rules, the
    norms with csrc/lk_rmsnorm.hip."""

    def __init__(self, dim: int, heads: int, T: int, mlp_ratio: float = 8.0 / 3.0, causal: bool = True, eps: float | None = 1e-6):
        super().__init__()
        if dim % heads:
            raise ValueError(f"heads ({heads}) must divide dim ({dim})")
        self.heads, self.causal, self.half = heads, causal, dim // heads // 2
        self.norm1 = nn.RMSNorm(dim, eps=eps)
        self.q, self.k, self.v, self.proj = (nn.Linear(dim, dim, bias=False) for _ in range(4))
        self.norm2 = nn.RMSNorm(dim, eps=eps)
        hidden = int(round(dim * mlp_ratio))
        self.w1, self.w3 = nn.Linear(dim, hidden, bias=False), nn.Linear(dim, hidden, bias=False)
        self.w2 = nn.Linear(hidden, dim, bias=False)
        cos, sin = rope_tables(T, dim // heads)
        self.register_buffer("cos", cos, persistent=False)
        self.register_buffer("sin", sin, persistent=False)

    def rope(self, x):
        rot = torch.cat((-x[..., self.half:], x[..., :self.half]), -1)
        return x * self.cos + rot * self.sin

    def forward(self, x):
        B, T = x.size(0), x.size(1)
        h = self.norm1(x)
        q = self.rope(self.q(h).view(B, T, self.heads, -1).transpose(1, 2))
        k = self.rope(self.k(h).view(B, T, self.heads, -1).transpose(1, 2))
        v = self.v(h).view(B, T, self.heads, -1).transpose(1, 2)
        a = nn.functional.scaled_dot_product_attention(q, k, v, is_causal=self.causal)
        x = x + self.proj(a.transpose(1, 2).reshape(B, T, -1))
        h = self.norm2(x)
        return x + self.w2(nn.functional.silu(self.w1(h)) * self.w3(h))


class ViTLlama(nn.Module):
    """:class:`ViTSwiGLU` with :class:`LlamaBlock` s: the patches of the image through a ``Linear`` embedding, no positional buffer
    (the rotary embedding of every block carries the positions), ``depth`` blocks, a final RMSNorm, the mean over the tokens and a
    ``Linear`` head.  The defaults give ``T = 64`` tokens, head dim 64 and 512 hidden units.  ``image`` is the side of a square
    image or ``(height, width)``.  ``freeze_norm``: the RMSNorm weights are not tracked, so that KFAC runs."""

    def __init__(self, num_classes: int = 10, image=32, patch: int = 4, dim: int = 192, depth: int = 6, heads: int = 3,
                 mlp_ratio: float = 8.0 / 3.0, freeze_norm: bool = True, causal: bool = True, eps: float | None = 1e-6):
        super().__init__()
        ih, iw = image if isinstance(image, (tuple, list)) else (image, image)
        if ih % patch or iw % patch:
            raise ValueError(f"patch ({patch}) must divide image ({image})")
        self.patch, self.grid = patch, (ih // patch, iw // patch)
        T = self.grid[0] * self.grid[1]
        self.embed = nn.Linear(3 * patch * patch, dim)
        self.blocks = nn.ModuleList(LlamaBlock(dim, heads, T, mlp_ratio, causal=causal, eps=eps) for _ in range(depth))
        self.norm = nn.RMSNorm(dim, eps=eps)
        self.head = nn.Linear(dim, num_classes)
        if freeze_norm:
            for m in self.modules():
                if isinstance(m, nn.RMSNorm):
                    for p in m.parameters():
                        p.requires_grad_(False)

    def forward(self, x):
        (gh, gw), p = self.grid, self.patch
        x = x.view(x.size(0), 3, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(x.size(0), gh * gw, 3 * p * p)
        x = self.embed(x)
        for blk in self.blocks:
            x = blk(x)
        return self.head(self.norm(x).mean(1))


# ---- 1-D convolutional networks (``dims=2``: the unit-height 2-D twin, the same function of the same state dict with the conv
# weights unsqueezed at dim 2; it exists so that an oracle that knows nn.Conv2d only can be run on the model) ----------------------
def _conv_nd(dims: int, cin: int, cout: int, k: int, stride: int = 1, padding: int = 0, dilation: int = 1, groups: int = 1,
             bias: bool = False) -> nn.Module:
    if dims == 1:
        return nn.Conv1d(cin, cout, k, stride, padding, dilation, groups, bias)
    if dims == 2:
        return nn.Conv2d(cin, cout, (1, k), (1, stride), (0, padding), (1, dilation), groups, bias)
    raise ValueError(f"dims must be 1 or 2, got {dims!r}")


class BasicBlock1d(nn.Module):
    """The basic residual block on ``[B, C, L]`` maps: two ``k = 3`` convolutions (the first carries the stride and the dilation,
    the second may be depthwise) with BatchNorm, a strided 1x1 shortcut where the shape changes."""

    def __init__(self, cin: int, cout: int, stride: int, act=nn.ReLU, dims: int = 1, dilation: int = 1, depthwise: bool = False):
        super().__init__()
        bn = nn.BatchNorm1d if dims == 1 else nn.BatchNorm2d
        self.conv1, self.bn1, self.act1 = _conv_nd(dims, cin, cout, 3, stride, dilation, dilation), bn(cout), act()
        self.conv2, self.bn2 = _conv_nd(dims, cout, cout, 3, 1, 1, groups=cout if depthwise else 1), bn(cout)
        self.act2 = act()
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(_conv_nd(dims, cin, cout, 1, stride), bn(cout))

    def forward(self, x):
        out = self.bn2(self.conv2(self.act1(self.bn1(self.conv1(x)))))
        return self.act2(out + (x if self.downsample is None else self.downsample(x)))


class ResNet1d(nn.Module):
    """A 1-D ResNet-18 as used on ECG, audio and sensor data: stem ``Conv1d(k=7, s=2)``, BatchNorm1d, activation,
    ``MaxPool1d(3, 2, 1)``; four stages of ``depth`` :class:`BasicBlock1d` each (``widths``; every stage after the first halves the
    length); ``AdaptiveAvgPool1d(1)``, flatten, ``Linear``.  Input ``[B, in_channels, L]``.  ``freeze_norm``: the BatchNorm
    affine parameters are not tracked, so that KFAC runs (the Conv1d layers are served as the unit-height Conv2d they equal,
    `laplace_amd.conv.lift`).  ``dilation``: of the strided convolution that opens stages two to four; ``depthwise``: the second
    convolution of every block is depthwise (``freeze_depthwise``: and not tracked - KFAC has no rule for grouped layers).
    ``dims=2``: the unit-height twin on ``[B, in_channels, 1, L]``."""

    def __init__(self, num_classes: int = 10, in_channels: int = 12, widths=(64, 128, 256, 512), depth: int = 2, act=nn.ReLU,
                 freeze_norm: bool = True, dims: int = 1, dilation: int = 1, depthwise: bool = False, freeze_depthwise: bool = False):
        super().__init__()
        bn = nn.BatchNorm1d if dims == 1 else nn.BatchNorm2d
        self.conv1, self.bn1, self.act1 = _conv_nd(dims, in_channels, widths[0], 7, 2, 3), bn(widths[0]), act()
        self.maxpool = nn.MaxPool1d(3, 2, 1) if dims == 1 else nn.MaxPool2d((1, 3), (1, 2), (0, 1))
        blocks, cin = [], widths[0]
        for i, cout in enumerate(widths):
            for j in range(depth):
                first = i > 0 and j == 0
                blocks.append(BasicBlock1d(cin, cout, 2 if first else 1, act, dims, dilation if first else 1, depthwise))
                cin = cout
        self.layers = nn.Sequential(*blocks)
        self.pool = nn.AdaptiveAvgPool1d(1) if dims == 1 else nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)
        for m in self.modules():
            if freeze_norm and isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                m.weight.requires_grad_(False), m.bias.requires_grad_(False)
            if freeze_depthwise and isinstance(m, (nn.Conv1d, nn.Conv2d)) and m.groups != 1:
                m.weight.requires_grad_(False)

    def forward(self, x):
        x = self.maxpool(self.act1(self.bn1(self.conv1(x))))
        return self.fc(torch.flatten(self.pool(self.layers(x)), 1))


class TextCNN(nn.Module):
    """The text CNN with max-over-time pooling (Kim 2014): token ids ``[B, T]`` through an embedding, ``transpose(1, 2)`` to
    ``[B, E, T]``, parallel ``Conv1d`` s of widths ``widths`` each followed by an activation and ``amax(2)`` (the maximum over the
    positions: csrc/lk_reduce.hip in the reverse sweep), ``cat``, ``Linear``.  ``freeze_embed``: the embedding table is not tracked,
    so that KFAC runs (a tracked one is served through ``use_embed_kernels``).  ``dims=2``: the unit-height twin."""

    def __init__(self, num_classes: int = 4, vocab: int = 2000, embed_dim: int = 128, channels: int = 100, widths=(3, 4, 5),
                 act=nn.ReLU, freeze_embed: bool = True, dims: int = 1):
        super().__init__()
        self.dims = dims
        self.embed = nn.Embedding(vocab, embed_dim)
        self.convs = nn.ModuleList(_conv_nd(dims, embed_dim, channels, k, bias=True) for k in widths)
        self.acts = nn.ModuleList(act() for _ in widths)
        self.fc = nn.Linear(channels * len(widths), num_classes)
        if freeze_embed:
            self.embed.weight.requires_grad_(False)

    def forward(self, x):
        e = self.embed(x).transpose(1, 2)
        if self.dims == 2:
            e = e.unsqueeze(2)
        feats = [act(conv(e)).amax(2 if self.dims == 1 else (2, 3)) for conv, act in zip(self.convs, self.acts)]
        return self.fc(torch.cat(feats, 1))


# ---- networks that change the resolution of a map by something other than a convolution or a pool (csrc/lk_resample.hip) -----------
class FPNSmall(nn.Module):
    """A CIFAR-sized feature pyramid used as a classifier: three levels (a 3x3 stem and two stride-2 3x3 convolutions, each with
    BatchNorm and an activation; ``widths`` are multiples of 32), 1x1 laterals to ``fpn`` channels, a top-down path that upsamples
    the coarser level by two and adds it to the lateral, a 3x3 smoothing convolution and a global average pool per level, ``cat``,
    ``Linear``.  ``mode="nearest"``: the top-down path is ``nn.Upsample(scale_factor=2, mode="nearest")``; ``mode="bilinear"``: it is
    ``F.interpolate(size=y.size()[2:], mode="bilinear", align_corners=False)`` with ``y`` the lateral it joins.  ``freeze_norm``:
    the BatchNorm affine parameters are not tracked, so that KFAC runs."""

    def __init__(self, num_classes: int = 10, widths=(32, 64, 128), fpn: int = 64, mode: str = "nearest", act=nn.ReLU,
                 freeze_norm: bool = True):
        super().__init__()
        if mode not in ("nearest", "bilinear"):
            raise ValueError(f"mode must be 'nearest' or 'bilinear', got {mode!r}")
        self.mode = mode
        cin, stages = 3, []
        for i, w in enumerate(widths):
            stages.append(nn.Sequential(nn.Conv2d(cin, w, 3, 1 if i == 0 else 2, 1, bias=False), nn.BatchNorm2d(w), act()))
            cin = w
        self.stages = nn.ModuleList(stages)
        self.laterals = nn.ModuleList(nn.Conv2d(w, fpn, 1) for w in widths)
        self.smooth = nn.ModuleList(nn.Conv2d(fpn, fpn, 3, 1, 1) for _ in widths)
        self.up = nn.Upsample(scale_factor=2, mode="nearest")
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(fpn * len(widths), num_classes)
        for m in self.modules():
            if freeze_norm and isinstance(m, nn.BatchNorm2d):
                m.weight.requires_grad_(False), m.bias.requires_grad_(False)

    def forward(self, x):
        feats = []
        for stage in self.stages:
            x = stage(x)
            feats.append(x)
        top, levels = None, []
        for f, lateral in zip(reversed(feats), reversed(self.laterals)):  # (coarse to fine)
            y = lateral(f)
            if top is not None:
                if self.mode == "nearest":
                    y = y + self.up(top)
                else:
                    y = y + F.interpolate(top, size=y.size()[2:], mode="bilinear", align_corners=False)
            top = y
            levels.append(y)
        pooled = [torch.flatten(self.pool(s(p)), 1) for s, p in zip(self.smooth, reversed(levels))]
        return self.fc(torch.cat(pooled, 1))


class TCNBlock(nn.Module):
    """One causal block of a temporal convolution network on ``[B, C, L]`` maps: a left pad of ``dilation * (k - 1)`` positions
    (``F.pad`` with zeros, or ``nn.ReflectionPad1d`` where ``reflect``), a dilated ``Conv1d``, an activation, a residual add (through
    a 1x1 convolution where the channel count changes).  ``dims=2``: the unit-height twin."""

    def __init__(self, cin: int, cout: int, k: int, dilation: int, act=nn.ReLU, reflect: bool = False, dims: int = 1):
        super().__init__()
        self.left = dilation * (k - 1)
        self.reflect = None
        if reflect:
            self.reflect = nn.ReflectionPad1d((self.left, 0)) if dims == 1 else nn.ReflectionPad2d((self.left, 0, 0, 0))
        self.conv, self.act = _conv_nd(dims, cin, cout, k, dilation=dilation, bias=True), act()
        self.short = None if cin == cout else _conv_nd(dims, cin, cout, 1)

    def forward(self, x):
        y = self.reflect(x) if self.reflect is not None else F.pad(x, (self.left, 0))
        return self.act(self.conv(y)) + (x if self.short is None else self.short(x))


class TCNSmall(nn.Module):
    """A causal temporal convolution network (Bai et al. 2018) as a sequence classifier: :class:`TCNBlock` s of ``channels`` with
    kernel ``k`` and the ``dilations`` (the block ``reflect_block`` pads by reflection, the others with zeros), the mean over time,
    ``Linear``.  Input ``[B, in_channels, L]``.  ``dims=2``: the unit-height twin on ``[B, in_channels, 1, L]``."""

    def __init__(self, num_classes: int = 10, in_channels: int = 8, channels: int = 64, k: int = 3, dilations=(1, 2, 4, 8),
                 act=nn.ReLU, reflect_block: int = 1, dims: int = 1):
        super().__init__()
        self.dims = dims
        blocks, cin = [], in_channels
        for i, d in enumerate(dilations):
            blocks.append(TCNBlock(cin, channels, k, d, act, i == reflect_block, dims))
            cin = channels
        self.blocks = nn.Sequential(*blocks)
        self.fc = nn.Linear(channels, num_classes)

    def forward(self, x):
        x = self.blocks(x)
        return self.fc(x.mean(2) if self.dims == 1 else x.mean((2, 3)))
