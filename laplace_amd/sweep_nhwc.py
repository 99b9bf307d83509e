"""The reverse sweep on NHWC split-fp16 cotangents: our own convolution kernels instead of MIOpen's.

:class:`laplace_amd.sweep.SeedBatchedSweep` walks the traced graph backwards with ONE cotangent of batch ``S*B`` and
hands every convolution to the library's fp32 backward-data (60 % of a ResNet-18 KFAC step).  This subclass keeps the
graph walk and replaces the data path (SURVEY.md §8f-1 "our own layer-local backward"; the reverse passes of
laplace/curvature/curvlinops.py:87-100):

* cotangents of feature maps live in HBM as NHWC *split tensors* — two fp16 planes and a power-of-two scale
  (csrc/lk_conv.hip) — produced by the element-wise VJP kernel ``lk_vjp_nhwc_split_f16x2`` (activation mask x folded
  BatchNorm scale x residual add, all seeds in one pass);
* a convolution's backward-data is ``lk_conv_nhwc_f16x2`` (implicit GEMM, three fp16 MFMAs per fp32 product block),
  writing fp32 NHWC plus max|.| for the next producer's scale; a strided 1x1 down-sampling branch ACCUMULATES into
  the main branch's result instead of materialising its three-quarters-zero cotangent;
* the G factor of a convolution layer is the Gram of the split tensor itself (``lk_gram_tn_f16x2``).

Max and average pooling run on the fp32 NHWC maps (csrc/lk_pool.hip: one byte of window-local argmax per output element for
all seeds, a gather-form VJP), and - with ``nhwc_depthwise = True`` - depthwise convolutions on their own streaming kernels
(csrc/lk_dwconv.hip: an fp32 forward, a gather-form backward-data that reads the split cotangent and writes fp32 for all seeds in
one launch).  With ``nhwc_norm_taps = True`` a tapped eval-mode BatchNorm2d hands its Jacobian kernel the unscaled split cotangent of its
output (csrc/lk_normtap.hip) and a tapped GroupNorm on a feature map the fp32 NHWC cotangent and ``xhat`` of its VJP (layout 1 of
csrc/lk_norm.hip).  A concatenation of feature maps along the channels (DenseNet blocks) runs on csrc/lk_cat.hip: one copy launch per
source in the forward, and per source one launch that reads its channel slice of all cotangent parts - fp32 maps and split tensors as
they lie - and writes their fp32 sum (``nhwc_cat``).  A channel slice of a feature map (``chunk`` / ``split`` / ``narrow`` / ``x[:, a:b]``:
CSP stages) runs on csrc/lk_slice.hip: one copy launch in the forward, and per sliced map one launch that sums the pieces its slices hand
back and the full-width parts into an fp32 map (``nhwc_slice``).  With ``nhwc_mul = True`` a squeeze-and-excitation gate - a feature map
times the ``[B, C, 1, 1]`` end of a chain of pointwise convolutions / Linear layers / activations that starts at the global average
pooling of that same map - runs on csrc/lk_gate.hip: per block and sweep one launch that reduces the cotangent against the map for
all seeds and one that writes the map's cotangent, gate product and pooling cotangent together; the chain in between runs on plain
``[S*B, C]`` tensors and its taps leave as fp32, as the NCHW sweep hands them out.  Graphs with nodes this path has no rule for (pooling with ``ceil_mode`` or dilation, adaptive pooling to several
cells, convolutions whose channel counts are not multiples of 32, ...) run through the parent class unchanged.
"""
from __future__ import annotations

import weakref

import torch
import torch.fx as fx
from torch import nn

from laplace_amd import conv as cv
from laplace_amd._lib import SplitTensor
from laplace_amd.sweep import (ACT, ADD, ATTN, AVGPOOL, BN, CAT, CONST, CONV, _EMBED, _EXPAND, GETITEM, GPOOL, IDENTITY, LINEAR, MATMUL, MAXPOOL, MEAN, MUL, NEG, NORM,
                               _MAXRED, _MHA, _MHAOUT, _PARAM, PERMUTE, _RESAMPLE, RESHAPE, SCALE, SIZE, SLICE, SOFTMAX, SPLIT, SUB, _SUMRED, SeedBatchedSweep, SweepUnsupported, _sum, _Walk)

# node kinds by what the NHWC walk does with them
_LAZY = {CONV, BN, ACT, IDENTITY}  # hand all incoming cotangent parts to ``_to_split`` (which can fuse a pending convolution)
_PASS_THROUGH = {ACT, IDENTITY, ADD}  # shape-preserving: the cotangent keeps the representation it arrives in
GN_MAP = "group-norm on a feature map"  # what `_walk` reports for an nn.GroupNorm node (NORM covers nn.LayerNorm in the head too)
CAT_MAP = "concatenation of feature maps"  # what `_walk` reports for a CAT whose sources sit on feature maps (CAT: one in the head)
SLICE_MAP = "channel slice of a feature map"  # what `_walk` reports for a SLICE whose source sits on a feature map (SLICE: one in the head)
GATE_MAP = "gated feature map"  # what `_walk` reports for a MUL that `nhwc_mul` serves: a feature map times its [B, C, 1, 1] gate
_POOL = {MAXPOOL, AVGPOOL}  # spatial pooling: fp32 NHWC in, fp32 NHWC out (lk_pool.hip)
_FEATURE = {CONV, BN, GPOOL, GN_MAP, CAT_MAP, SLICE_MAP, GATE_MAP} | _POOL  # produce / consume NHWC feature maps
_MAP_SOURCES = {CONV, BN, GN_MAP, CAT_MAP, SLICE_MAP, GATE_MAP, "placeholder"} | _POOL  # what a node that sits on a feature map has upstream
# a graph with one of these runs through the NCHW sweep (MUL: unless ``nhwc_mul`` serves it as a squeeze-and-excitation gate on
# csrc/lk_gate.hip, or both its operands lie in the head region)
_NO_RULE = {MEAN, SIZE, GETITEM, ATTN, PERMUTE, CONST, MUL, MATMUL, SOFTMAX, SCALE, NEG, SUB, _EMBED, _PARAM, _EXPAND, _MAXRED, _SUMRED, _MHA, _MHAOUT, _RESAMPLE}
_GATE_CHAIN = {CONV, LINEAR, ACT, IDENTITY, RESHAPE}  # what the branch from the pooled tensor to a served gate may hold
# kinds the head region holds too (plain tensors after the flatten): a node of these whose parts are all plain tensors, and that is
# no served gate, runs the parent's rule for its kind (`SplitSweep._head_vjp`).  The value: the refusal where another part reaches
# it; ``None``: the NHWC table has a rule for feature maps
_HEAD = {LINEAR: "Linear layer inside the NHWC region", NORM: None, ACT: None, CAT: None, SLICE: None,
         MUL: "product of a feature map outside the gate rule of the NHWC region", RESHAPE: "reshape inside the NHWC region"}


class _F32:
    """fp32 NHWC cotangent ``[S*B, H, W, C]`` + device word with the bit pattern of max|.|"""

    __slots__ = ("t", "amax")

    def __init__(self, t, amax):
        self.t, self.amax = t, amax


class NhwcNormGrad:
    """What a GroupNorm tapped on the NHWC sweep hands over (``nhwc_norm_taps``): the fp32 NHWC cotangent of its output
    ``g`` ``[S*B, H, W, C]`` and the NHWC ``xhat`` ``[B, H, W, C]`` its forward kept - the operands of layout 1 of
    lk_jac_norm_affine_f32 as they lie"""

    __slots__ = ("g", "xhat")

    def __init__(self, g, xhat):
        self.g, self.xhat = g, xhat


class _PendingConv:
    """A forward convolution that has not run yet: its only consumer is an eval-mode BatchNorm, which runs it with the
    per-channel affine map, the residual add and the ReLU in the convolution's epilogue (lk_conv_bn_act_nhwc_f16x2) —
    or, where that launch does not apply, materialises it as before.  Quacks like its fp32 ``[N, C, H, W]`` result as far
    as the traced forward looks at it (``shape``, ``dtype``, ``dim()``)."""

    __slots__ = ("prep", "xs", "shape", "dtype", "device", "_run")

    def __init__(self, prep, xs, shape, run):
        self.prep, self.xs, self.shape, self._run = prep, xs, torch.Size(shape), run
        self.dtype, self.device = torch.float32, xs.planes.device

    def dim(self) -> int:
        return len(self.shape)

    def materialize(self) -> torch.Tensor:
        return self._run()


class _LazyConv:
    """A stride-1 convolution's backward-data that has not run yet: whoever consumes the cotangent decides whether it is
    materialised as an fp32 tensor (``f32()``) or comes out of the convolution kernel already multiplied / joined / split
    (``fused(...)``, lk_conv_nhwc_f16x2_vjp) — the element-wise VJP kernel and the fp32 tensor's round trip then vanish."""

    __slots__ = ("_f32", "_fused", "_done")

    def __init__(self, f32, fused):
        self._f32, self._fused, self._done = f32, fused, None

    def f32(self) -> "_F32":
        if self._done is None:
            self._done = self._f32()
        return self._done

    def fused(self, **kw) -> SplitTensor:
        assert self._done is None
        return self._fused(**kw)


class _LazyStrided(_LazyConv):
    """A STRIDED convolution's backward-data that has not run yet (``desc = (prep, g, cscale)``, input ``hw``): one or two
    of them reaching the same node (the 3 x 3 main branch and the 1 x 1 shortcut of a residual down-sampling block) leave
    ``_to_split`` as ONE launch over all residue classes with the element-wise VJP fused
    (lk_conv_nhwc_f16x2_vjp_strided); ``f32(into)`` is the fallback: class by class into an fp32 tensor."""

    __slots__ = ("desc", "hw", "_run")

    def __init__(self, run, desc, hw):
        super().__init__(None, None)
        self._run, self.desc, self.hw = run, desc, hw

    def f32(self, into=None) -> "_F32":
        if self._done is None:
            self._done = self._run(into)
        return self._done


def _materialize(parts):
    out, first = [], None
    for p in parts:  # (plain tensors first: a pending strided convolution then adds into one instead of making its own)
        if isinstance(p, _F32) and first is None:
            first = p
    for p in parts:
        if isinstance(p, _LazyStrided):
            if p._done is None and first is not None:
                p.f32(first)  # accumulated into the tensor that is already there
                continue
            p = p.f32()
            first = first if first is not None else p
        elif isinstance(p, _LazyConv):
            p = p.f32()
            first = first if first is not None else p
        out.append(p)
    return out


def _as_f32(parts):
    """the parts as plain fp32 NHWC tensors: a split tensor converted, an fp32 map as it lies"""
    return [p.float() if isinstance(p, SplitTensor) else p.t for p in parts]


def _run_deferred(fns):
    """deferred strided branches that nothing else joins: the first makes the fp32 tensor, the others add into it"""
    part = fns[0](None)
    for fn in fns[1:]:
        fn(part)
    return part


class _NhwcWalk(_Walk):
    """The state of one reverse walk of :class:`SplitSweep`: the parent's, and what the NHWC rules share."""

    def __init__(self, sweep, seeds, on_tap, defer_bn_scale, keep_split):
        super().__init__(sweep, seeds, on_tap, defer_bn_scale)
        self.keep_split, self.K = keep_split, sweep.kernels()
        # conv taps whose own gradient is owed a BatchNorm scale that the CALLER did not ask to receive (a tapped BatchNorm left
        # it to the backward-data launch): applied in the conversion at the end, never handed out through ``grad_scale``
        self.own_scale: set = set()
        self.owed: dict[str, torch.Tensor] = {}
        self.norm_names: set = set()  # taps that leave in NHWC form whatever the caller asked for
        self.deferred: dict[fx.Node, list] = {}  # node -> strided 1x1 branches waiting for the main branch's tensor
        self.mult_cache: dict = {}  # activation node -> its NHWC multiplier (`SplitSweep._nhwc_mult`)
        # zeroed max|.| words of this sweep's conv outputs (one fill per 64 of them)
        self._words, self._word_i = torch.zeros(64, dtype=torch.float32, device=seeds.device), 0

    def new_word(self):
        if self._word_i == self._words.numel():
            self._words, self._word_i = torch.zeros_like(self._words), 0
        self._word_i += 1
        return self._words[self._word_i - 1:self._word_i]

    def push(self, n, part):
        if not isinstance(n, fx.Node) or n.op == "placeholder":  # (no CONST test: such a graph never takes this walk, `_NO_RULE`)
            return
        if isinstance(part, _LazyConv) and n in self.deferred:
            part = part.f32()
        if isinstance(part, _F32) and n in self.deferred:
            for fn in self.deferred.pop(n):  # strided 1x1 branches waiting for the main branch's tensor: add into it
                fn(part)
        self.cot.setdefault(n, []).append(part)

    def feature_f32(self, t4_nchw_like):
        """fp32 [S*B, C, H, W]-shaped tensor -> NHWC _F32"""
        t = t4_nchw_like.permute(0, 2, 3, 1).contiguous()
        return _F32(t, self.K.absmax(t))


class SplitSweep(SeedBatchedSweep):
    """Seed-batched reverse sweep whose feature-map cotangents are NHWC split tensors (needs the HIP kernels)."""

    def __init__(self, model, tap_modules, kernels=None, nhwc_norm_taps=None):
        super().__init__(model, tap_modules, kernels)
        if nhwc_norm_taps is not None:
            self.nhwc_norm_taps = bool(nhwc_norm_taps)
        self._prep: dict[str, cv.PreparedConv] = {}
        self._amax_cache: dict = {}
        self._on_map_cache: dict = {}
        # MUL node -> (index of the gate operand, node of the gated map, chain [GPOOL, ..., gate]) of a product `nhwc_mul` serves;
        # chain node -> its MUL node; id(rule) of a MUL -> its node (`_run_mul` receives the rule)
        self._gates: dict = {}
        self._gate_nodes: dict = {}
        self._mul_node = {id(r): n for n, r in self.rule.items() if r.kind == MUL}
        self.split_reason = self._split_eligible()
        self.split_ok = self.split_reason is None

    #: callable ``(tap name, NHWC shape, device) -> fp32 tensor or None``, set around a forward by the KFAC accumulator: where the
    #: activation that a tapped convolution reads is to be written (see `_run_bn_act`)
    act_sink = None
    #: ``False``: every backward-data writes fp32 and the element-wise VJP kernel runs on it
    fuse_vjp = True
    #: ``False``: strided convolutions run class by class into an fp32 tensor (one launch per
    #: residue class and branch) instead of the strided fused launch
    fuse_strided = True

    # ---- static eligibility ---------------------------------------------------------------------------------------
    def _split_eligible(self):
        for node, r in self.rule.items():  # (token models and lone parameters: named first, the NCHW walk serves them)
            if r.kind == _EMBED:
                return f"{node.target}: Embedding has no NHWC rule"
            if r.kind in (_PARAM, _EXPAND):
                return f"parameter {r.args[0]} has no NHWC rule"
        for node, r in self.rule.items():  # (nn.MultiheadAttention, the stock encoder: token models, the NCHW walk serves them)
            if r.kind == _MHA:
                return f"{node.target}: MultiheadAttention has no NHWC rule"
        for node, r in self.rule.items():  # (1-D convolutional networks: [B, C, L] maps and the reduction they end in)
            if r.kind == CONV and isinstance(r.mod, nn.Conv1d):
                return f"{node.target}: Conv1d has no NHWC rule"
            if r.kind in (_MAXRED, _SUMRED) or r.flavour == "1d":
                return f"{node.target if node.op == 'call_module' else node.name}: {r.what} has no NHWC rule"
        for node, r in self.rule.items():  # (upsampling and padding: named before the ``size()`` a traced ``size=`` reads)
            if r.kind == _RESAMPLE:
                return f"{node.target if node.op == 'call_module' else node.name}: {r.what} has no NHWC rule"
        for node, r in self.rule.items():
            if r.kind == ATTN:  # (named first: it is what decides the walk of a transformer block)
                return f"{node.name}: {r.what} has no NHWC rule"
        for node, r in self.rule.items():
            if r.kind == MUL:  # (named before the narrow 1x1 convolutions of a gate branch, which only exist because of it)
                if not self.nhwc_mul:
                    return f"{r.what} has no NHWC rule"
                why = self._mul_refusal(node, r)
                if why is not None:
                    return why
        for node, r in self.rule.items():
            if r.kind in (MATMUL, SOFTMAX, SCALE):  # (hand-written attention: named before the transposes around it)
                return f"{r.what} has no NHWC rule"
        for node, r in self.rule.items():
            if r.kind in (NEG, SUB):  # (a sign: the rotate-half of a rotary embedding, a hand-written residual)
                return f"{r.what} has no NHWC rule"
        for node, r in self.rule.items():
            if r.kind == NORM and isinstance(r.mod, nn.RMSNorm):  # (normalises rows of the last dims: never a channel group of a map)
                return f"{node.target}: RMSNorm has no NHWC rule"
        for name in sorted(self.tap_names):
            m = self.modules.get(name)
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                if self._bn_tap_served(m):
                    if self.kernels is None or not hasattr(self.kernels(), "jac_norm_affine_nhwc"):
                        return f"{name}: tapped BatchNorm (kernels without the NHWC norm-tap entry point)"
                    continue  # (its Jacobian reads the split cotangent where it lies: lk_normtap.hip)
                # its weight / bias Jacobian reads the fp32 NCHW cotangent of the BatchNorm's output (lk_norm.hip, layout 0)
                return f"{name}: tapped BatchNorm (its cotangent is delivered by the NCHW sweep)"
            if isinstance(m, nn.GroupNorm) and self.nhwc_norm_taps:
                continue  # (on a feature map, which the NORM rule below checks: layout 1 of lk_norm.hip on the NHWC cotangent)
            if isinstance(m, (nn.GroupNorm, nn.LayerNorm)):
                return f"{name}: tapped {type(self.modules[name]).__name__} (its cotangent is delivered by the NCHW sweep)"
        if self.kernels is None or not hasattr(self.kernels(), "conv_nhwc_f16x2"):
            return "kernels without the split-fp16 convolution"
        n_conv = 0
        for node, r in self.rule.items():
            if r.kind == CONV:
                m, first = r.mod, r.src[0].op == "placeholder"
                if node in self._gate_nodes:
                    continue  # (a 1x1 convolution on the pooled [B, C, 1, 1] tensor of a gate branch: parent-class math)
                if m.groups != 1:
                    why = self._depthwise_refusal(node, m)
                    if why is not None:
                        return f"{node.target}: grouped convolution ({why}; the NCHW sweep serves it)"
                    continue  # (served by lk_dwconv.hip; a graph still needs a dense convolution)
                if not cv.supported(m) and not (first and node.target in self.tap_names and m.out_channels % 8 == 0):
                    return f"{node.target}: convolution outside the implicit-GEMM kernel's coverage"
                n_conv += 1
            elif r.kind == MUL:
                continue  # (`_mul_refusal` above: a served gate, or a product in the head region)
            elif r.kind in _NO_RULE or isinstance(r.mod, nn.BatchNorm1d) or (r.kind in _POOL and not self.nhwc_pool):
                return (f"{node.target}: " if node.op == "call_module" else "") + f"{r.what} has no NHWC rule"
            elif r.kind in _POOL:
                why = self._pool_refusal(node, r)
                if why is not None:
                    return f"{node.target if node.op == 'call_module' else node.name}: {why}"
            elif r.kind == NORM:
                on_map = any(k in _MAP_SOURCES for k in self._walk(node, False))
                if isinstance(r.mod, nn.LayerNorm) and on_map:
                    return f"{node.target}: LayerNorm applied to a feature map (the NHWC kernels normalise per channel group)"
                if isinstance(r.mod, nn.GroupNorm) and not on_map:
                    return f"{node.target}: GroupNorm outside the feature maps"
                if isinstance(r.mod, nn.GroupNorm) and not all(hasattr(self.kernels(), f) for f in ("norm_forward", "norm_vjp")):
                    return f"{node.target}: kernels without the per-sample normalisation entry points"
            elif r.kind == GPOOL and tuple(self._pair2(r.args[0])) != (1, 1):
                return f"{node.target if node.op == 'call_module' else node.name}: adaptive pooling to more than one cell"
            elif r.kind == CAT:
                why = self._cat_refusal(node, r)
                if why is not None:
                    return f"{node.name}: {why}"
            elif r.kind == SLICE:
                why = self._slice_refusal(node, r)
                if why is not None:
                    return f"{node.name}: {why}"
        if not n_conv:
            return "no convolution in the graph"
        return self._region_check()

    #: ``False``: a model with max / average pooling runs through the NCHW sweep, as it did before lk_pool.hip
    nhwc_pool = True
    #: ``True``: a model whose eval-mode BatchNorm2d or feature-map GroupNorm parameters are tracked stays on the NHWC walk; the
    #: BatchNorm's Jacobian reads the split cotangent of its output where it lies (csrc/lk_normtap.hip), the GroupNorm's the fp32
    #: NHWC cotangent its VJP forms anyway (layout 1 of csrc/lk_norm.hip).  ``False`` (the default): such a model runs through the
    #: NCHW sweep, as it did before lk_normtap.hip (tools/norm_tap_bench.py)
    nhwc_norm_taps = False

    #: ``False``: a model with a ``torch.cat`` runs through the NCHW sweep (whose CAT rule serves it), as it would without
    #: csrc/lk_cat.hip (tools/cat_bench.py)
    nhwc_cat = True

    def _on_map(self, n) -> bool:
        """does the value of node ``n`` sit on a feature map (decided on the graph alone)?"""
        hit = self._on_map_cache.get(n)
        if hit is None:
            kind = self.rule[n].kind
            if kind == CAT:
                hit = any(self._on_map(a) for a in self.rule[n].src)
            elif kind == MUL:
                hit = n in self._gates
            elif kind in (SLICE, SPLIT):
                hit = self._on_map(self.rule[n].src[0])
            elif kind in _PASS_THROUGH:
                hit = any(k in _MAP_SOURCES for k in self._walk(n, False))
            else:
                hit = (GN_MAP if kind == NORM and isinstance(self.rule[n].mod, nn.GroupNorm) else kind) in _MAP_SOURCES
            self._on_map_cache[n] = hit
        return hit

    def _cat_refusal(self, node, r):
        """why this CAT node keeps the model off the NHWC walk (None: lk_cat.hip serves it, or it is a concatenation of plain
        tensors in the head region, which takes the parent-class math)"""
        if not self.nhwc_cat:
            return f"{r.what} has no NHWC rule"
        on_map = [self._on_map(a) for a in r.src]
        if not any(on_map):
            return None
        if not all(on_map):
            return f"{r.what} of feature maps with tensors outside the feature maps"
        if r.args[0] not in (1, -3):
            return f"{r.what} of feature maps along dim {r.args[0]} (the NHWC kernels concatenate channels: dim 1 of a 4-D map)"
        if not all(hasattr(self.kernels(), f) for f in ("cat_forward", "cat_vjp")):
            return "kernels without the concatenation entry points"
        return None

    #: ``False``: a model that slices a feature map (``chunk`` / ``split`` / ``narrow`` / static indexing) runs through the NCHW
    #: sweep (whose SLICE rule serves it), as it would without csrc/lk_slice.hip (tools/slice_bench.py)
    nhwc_slice = True

    @staticmethod
    def _slice_dim_as_written(spec):
        """``(dim, drops)`` of a SLICE rule as far as the graph alone tells: the dim as written (counted from the end behind a
        ``...``) and whether an int index drops it"""
        if spec[0] == "index":
            entries, i = spec[1], spec[2]
            dim = i if not any(e is Ellipsis for e in entries[:i]) else i - len(entries)
            return dim, not isinstance(entries[i], slice)
        return (spec[1] if spec[0] == "narrow" else spec[3]), False

    def _slice_refusal(self, node, r):
        """why this SLICE node keeps the model off the NHWC walk (None: lk_slice.hip serves it, or it is a slice of a plain tensor
        in the head region, which takes the parent-class math)"""
        if not self.nhwc_slice:
            return f"{r.what} has no NHWC rule"
        if not self._on_map(r.src[0]):
            return None
        dim, drops = self._slice_dim_as_written(r.args)
        if drops:
            return f"{r.what}: an int index on a feature map (the NHWC kernels slice channel ranges and keep the dim)"
        if dim not in (1, -3):
            return f"{r.what}: slice of a feature map along dim {dim} (H or W; the NHWC kernels slice channels: dim 1 of a 4-D map)"
        if any(k not in _FEATURE and k not in _PASS_THROUGH for k in self._walk(node, True)):
            return f"{r.what}: slice of a feature map mixed with consumers outside the feature maps"
        if not all(hasattr(self.kernels(), f) for f in ("slice_forward", "slice_vjp")):
            return "kernels without the slicing entry points"
        return None

    #: ``True``: a squeeze-and-excitation gate - a feature map times the ``[B, C, 1, 1]`` end of a chain that starts at the
    #: ``AdaptiveAvgPool2d(1)`` of that same map - runs on csrc/lk_gate.hip and its model stays on the NHWC walk.  ``False`` (the
    #: default): a model with a product runs through the NCHW sweep (whose MUL rule serves it), as it did before lk_gate.hip
    #: (tools/se_nhwc_bench.py)
    nhwc_mul = False

    def _back_to_pool(self, n):
        """the GPOOL node that the first inputs upstream of ``n`` lead to, or ``None``"""
        for _ in range(len(self.rule)):
            if not isinstance(n, fx.Node) or n.op == "placeholder":
                return None
            r = self.rule[n]
            if r.kind == GPOOL:
                return n
            if r.kind == CONST or len(r.src) != 1:
                return None
            n = r.src[0]
        return None

    def _gate_chain(self, gate, pool):
        """the chain ``[pool, ..., gate]`` of a gate branch, or the reason (a string that names the offending node) why the branch
        is none: every node has one traced input and one consumer and is a pointwise convolution, a Linear, an activation, an
        identity or a reshape with static arguments"""
        chain, n = [], gate
        while True:
            r = self.rule[n]
            if len(n.users) != 1:
                return f"mul: gate branch node {n.name} has {len(n.users)} consumers (a gate branch is a chain without a fork)"
            if n is pool:
                if tuple(self._pair2(r.args[0])) != (1, 1):
                    return f"mul: gate branch node {n.name}: adaptive pooling to more than one cell"
                chain.append(n)
                return chain[::-1]
            if len(n.all_input_nodes) != 1:
                return (f"mul: gate branch node {n.name} reads {len(n.all_input_nodes)} traced values (a gate branch is a chain: no "
                        "join, no view built from x.size())")
            if r.kind not in _GATE_CHAIN:
                return f"mul: gate branch node {n.name} ({r.what}) is no pointwise convolution, Linear, activation, identity or reshape"
            if r.kind == CONV:
                m = r.mod
                if not (tuple(m.kernel_size) == (1, 1) and tuple(m.stride) == (1, 1) and m.padding in ((0, 0), 0, "valid")
                        and m.groups == 1):
                    return f"mul: gate branch node {n.name}: {n.target} is no pointwise convolution (1x1, stride 1, no padding, one group)"
            chain.append(n)
            n = r.src[0]

    def _mul_refusal(self, node, r):
        """why this MUL node keeps the model off the NHWC walk (None: lk_gate.hip serves it and it is entered in ``_gates``, or it is
        a product of plain tensors in the head region, which takes the parent-class math)"""
        for gi in (1, 0):
            gate, x = r.src[gi], r.src[1 - gi]
            pool = self._back_to_pool(gate)
            if pool is None or gate is x or self.rule[pool].src[0] is not x or not self._on_map(x):
                continue
            chain = self._gate_chain(gate, pool)
            if isinstance(chain, str):
                return chain
            if self.kernels is None or not all(hasattr(self.kernels(), f) for f in ("gate_reduce", "gate_vjp")):
                return "mul: kernels without the gate entry points"
            self._gates[node] = (gi, x, chain)
            for n in chain:
                self._gate_nodes[n] = node
            return None
        on_map = [isinstance(a, fx.Node) and self._on_map(a) for a in r.src]
        if not any(on_map):
            return None
        if all(on_map):
            return "mul: product of two feature maps (the NHWC kernels serve a [B, C, 1, 1] gate)"
        return (f"mul: {node.name} multiplies a feature map by a tensor that is no [B, C, 1, 1] gate of that map (a chain from its "
                "global average pooling)")

    def _bn_tap_served(self, m) -> bool:
        """is this tapped BatchNorm one the NHWC walk delivers the cotangent of (``nhwc_norm_taps``)?"""
        return bool(self.nhwc_norm_taps and isinstance(m, nn.BatchNorm2d) and m.running_var is not None and not m.training)

    @staticmethod
    def norm_grad_nchw(g, S, B):
        """a norm tap's NHWC gradient (SplitTensor / NhwcNormGrad) as the ``[S, B, C, H, W]`` fp32 tensor of the NCHW sweep"""
        t = g.g if isinstance(g, NhwcNormGrad) else g.float()
        return t.reshape(S, B, *t.shape[1:]).permute(0, 1, 4, 2, 3).contiguous()
    #: ``True``: depthwise convolutions run on csrc/lk_dwconv.hip and their model stays on the NHWC walk.  ``False`` (the default):
    #: such a model runs through the NCHW sweep, as it did before lk_dwconv.hip.  Off by default because the route has to lose on
    #: neither line of tools/dwconv_bench.py and lost on one: on MobileNetV1 at minibatch 128 it halves `kron` with the depthwise
    #: weights frozen, but `diag` with them tracked came out 0.3 % slower, in every round (profiles/dwconv_bench.json)
    nhwc_depthwise = False

    def _depthwise_refusal(self, node, m):
        """why this grouped convolution keeps the model off the NHWC walk (None: lk_dwconv.hip serves it)"""
        if not self.nhwc_depthwise:
            return "foreign to the NHWC kernels"
        why = cv.depthwise_refusal(m)
        if why is not None:
            return f"{why}: outside the depthwise kernels' contract"
        if not any(k in _MAP_SOURCES for k in self._walk(node, False)):
            return "depthwise convolution outside the feature maps"
        if not all(hasattr(self.kernels(), f) for f in ("dwconv_forward", "dwconv_backward")):
            return "kernels without the depthwise entry points"
        return None

    def _is_depthwise(self, m) -> bool:
        return self.split_ok and isinstance(m, nn.Conv2d) and m.groups != 1

    def _defers_scale_to(self, src, cot) -> bool:
        # (the depthwise backward-data takes no folded BatchNorm scale)
        r = self.rule.get(src)
        return not (r is not None and self._is_depthwise(r.mod)) and super()._defers_scale_to(src, cot)

    def _pool_refusal(self, node, r):
        """why this MAXPOOL / AVGPOOL node keeps the model off the NHWC walk (None: lk_pool.hip serves it)"""
        p = self.pool_params(r)
        if not any(k in _MAP_SOURCES for k in self._walk(node, False)):
            return f"{r.what} outside the feature maps"
        if p["dilation"] != (1, 1):
            return f"dilated pooling (dilation {p['dilation']}; the NHWC kernels take none)"
        if p["ceil_mode"]:
            return "pooling with ceil_mode=True (the NHWC kernels take ceil_mode=False only)"
        (kh, kw), (sh, sw), (ph, pw) = p["kernel"], p["stride"], p["padding"]
        if not (1 <= kh <= 8 and 1 <= kw <= 8 and sh >= 1 and sw >= 1 and 0 <= ph <= kh // 2 and 0 <= pw <= kw // 2):
            return (f"pooling window {(kh, kw)} / stride {(sh, sw)} / padding {(ph, pw)} outside the NHWC kernels' contract "
                    "(1 <= window <= 8, stride >= 1, padding <= window / 2)")
        if not all(hasattr(self.kernels(), f) for f in ("pool_forward", "pool_vjp", "POOL_MAX", "POOL_AVG")):
            return "kernels without the pooling entry points"
        return None

    # The reverse sweep must not fail half-way (`on_tap` has already added G factors by then): every structural
    # condition `backward` would raise on is checked here, on the graph alone, so that such a model runs through the
    # parent class's NCHW sweep from the start.
    def _walk(self, start, downstream: bool):
        """kinds of the nodes reachable from ``start`` through shape-preserving nodes (users if ``downstream`` else inputs)"""
        seen, todo, out = set(), [start], []
        while todo:
            n = todo.pop()
            for m in (n.users if downstream else n.all_input_nodes):
                if m in seen:
                    continue
                seen.add(m)
                kind = self.rule[m].kind
                if kind == SPLIT:  # (a tuple of parts: its items, which look through it, are what is walked)
                    todo.append(m)
                    continue
                if kind == CAT and self._on_map(m):
                    kind = CAT_MAP  # (a producer and consumer of feature maps, not pass-through)
                if kind == SLICE and self._on_map(m):
                    kind = SLICE_MAP
                if kind == MUL and m in self._gates:
                    kind = GATE_MAP
                out.append(GN_MAP if kind == NORM and isinstance(self.rule[m].mod, nn.GroupNorm) else kind)
                if kind in _PASS_THROUGH:
                    todo.append(m)
        return out

    def _region_check(self):
        for node, r in self.rule.items():
            if node in self._gate_nodes:
                continue  # (a gate branch: plain [B, C, 1, 1] / [B, C] tensors between the pooling and the product)
            if r.kind == RESHAPE and any(k in _FEATURE for k in self._walk(node, True)):
                return f"{node.name}: view / reshape / flatten whose result is used as a feature map"
            if r.kind == GPOOL:
                users = list(node.users)
                if len(users) != 1 or self.rule[users[0]].kind != RESHAPE:
                    return f"{node.name}: pooled tensor with a consumer other than one flatten"
            if r.kind == LINEAR and any(k in _MAP_SOURCES for k in self._walk(node, False)):
                return f"{node.target}: Linear layer applied to a feature map"
        return None

    # ---- forward: own convolution + fused BatchNorm/add/activation kernels on NHWC -----------------------------------
    #: ``False``: the forward stays on the library's NCHW convolutions
    nhwc_forward = True

    @torch.no_grad()
    def forward(self, x, need_vjp: bool = True, keep_tap_splits: bool = False):
        """``keep_tap_splits``: keep the NHWC split copy of every tapped convolution's input (``tap_splits``) until
        ``release()`` — only the Kron predictive's eigenbasis rotation reads it; a fit would hold a second
        activation-sized copy through the whole reverse sweep for nothing."""
        self._keep_tap_splits = keep_tap_splits
        # data_ptr of a feature map produced here -> {"in_amax": [B] words, "mul": word, "add": word | None} (a convolution's
        # output: a per-image bound without a pass over it) / {"split": SplitTensor, "bound": [B] words} (an activation)
        self._aux = {}
        self.tap_splits = {}  # tap name -> NHWC SplitTensor of the tap's input (what its forward convolution consumed)
        self._fwd_words = None
        try:
            return super().forward(x, need_vjp)
        finally:
            self._aux = {}  # (the split copies of the activations are only needed while the forward runs)

    def _aux_put(self, t, entry):
        """register what is known about the feature map ``t`` (keyed by address, OWNED by the tensor object: a map that was
        freed — a materialised convolution output behind its BatchNorm launch — may hand its address to a later tensor that
        registers nothing, which must not inherit a stale per-image bound: too small a bound saturates fp16 planes silently)"""
        entry["_owner"] = weakref.ref(t)
        self._aux[t.data_ptr()] = entry

    def _aux_get(self, t):
        entry = self._aux.get(t.data_ptr())
        if entry is not None and entry["_owner"]() is not t:
            del self._aux[t.data_ptr()]
            return None
        return entry

    def _fwd_word(self, dev, n=1):
        """``n`` zeroed device words out of a per-forward pool (one fill launch per pool)"""
        if self._fwd_words is None or self._fwd_words[1] + n > self._fwd_words[0].numel():
            self._fwd_words = [torch.zeros(max(64, 32 * n), dtype=torch.float32, device=dev), 0]
        w = self._fwd_words[0][self._fwd_words[1]:self._fwd_words[1] + n]
        self._fwd_words[1] += n
        return w

    def _use_nhwc_forward(self, t) -> bool:
        return self.split_ok and self.nhwc_forward and torch.is_tensor(t) and t.dim() == 4 and t.dtype == torch.float32 \
            and t.shape[0] > 0

    def _split_input(self, inp, pad_to=None):
        aux = self._aux_get(inp)
        if aux is not None and "split" in aux and aux["split"] is not None and pad_to is None:
            return aux["split"]
        K = self.kernels()
        xh = inp.permute(0, 2, 3, 1).contiguous()  # (a view when inp is already NHWC in memory)
        if pad_to is not None and xh.shape[-1] != pad_to:
            xp = xh.new_zeros(*xh.shape[:3], pad_to)
            xp[..., :xh.shape[-1]] = xh
            xh = xp
        return K.split_images_f16x2(xh)  # one scale per image (lk_split_images_f16x2)

    def _run_depthwise(self, node, m, inp):
        """depthwise convolution on a feature map: lk_dwconv_fwd_nhwc_f32 on the NHWC memory of the input; returns the
        NCHW-logical view over NHWC memory, as `_run_pool` does.  Where the input carries per-image ``"bound"`` words the output
        registers the guaranteed bound ``max|x_n| * l1 + max|bias|``, as a dense convolution does, and the BatchNorm launch behind
        it needs no pass over the map."""
        # (also with ``nhwc_forward = False``: the reverse sweep is NHWC either way)
        if not (torch.is_tensor(inp) and inp.dim() == 4 and inp.dtype == torch.float32):
            raise SweepUnsupported(f"{node.target}: depthwise convolution of the NHWC sweep expects an fp32 feature map")
        prep = self._prep.get(node.target)
        if prep is None:
            prep = self._prep[node.target] = cv.PreparedDepthwise(m)
        xh = inp.permute(0, 2, 3, 1).contiguous()  # (a view when inp is already NHWC in memory)
        y = self.kernels().dwconv_forward(xh, prep.w_tap, prep.bias, m.kernel_size, m.stride, m.padding)
        out = y.permute(0, 3, 1, 2)
        aux = self._aux_get(inp)
        if aux is not None and aux.get("bound") is not None:
            l1, bmax = prep.forward_l1()
            self._aux_put(out, {"in_amax": aux["bound"], "mul": l1, "add": bmax})
        return out

    def _run_conv(self, node, m, inp):
        if node in self._gate_nodes:
            return m(inp)  # (a gate branch's convolution on [B, C, 1, 1]: no own-convolution launch, no split copy)
        if self._is_depthwise(m):
            return self._run_depthwise(node, m, inp)
        if not (self._use_nhwc_forward(inp) and cv.forward_supported(m)):
            return m(inp)
        prep = self._prep.get(node.target)
        if prep is None:
            prep = self._prep[node.target] = cv.PreparedConv(m)
        xs = self._split_input(inp, pad_to=prep.padded_in if prep.padded_in != m.in_channels else None)
        if self._keep_tap_splits and node.target in self.tap_names and prep.padded_in == m.in_channels:
            # consumers of the tap's input that run our convolution on it again (the Kron predictive's eigenbasis
            # rotation) take the split copy instead of measuring and splitting the activation a second time
            self.tap_splits[node.target] = xs

        def run():
            out = cv.conv_forward(prep, xs)
            if m.bias is not None:
                out += m.bias
            y = out.permute(0, 3, 1, 2)  # logical [B, C, H, W] over NHWC memory
            if xs.amax is not None:
                # per-image bound of the output without a pass over it: measured max of the input image * l1(W) + max|bias|
                l1, bmax = prep.forward_l1()
                self._aux_put(y, {"in_amax": xs.amax, "mul": l1, "add": bmax})
            return y

        if self._bn_takes_conv(node, m, xs):
            s_, (ph, pw), (KH, KW) = m.stride[0], m.padding, m.kernel_size
            Ho, Wo = (xs.shape[1] + 2 * ph - KH) // s_ + 1, (xs.shape[2] + 2 * pw - KW) // s_ + 1
            return _PendingConv(prep, xs, (xs.shape[0], m.out_channels, Ho, Wo), run)
        return run()

    def _run_norm(self, node, m, inp):
        """GroupNorm on a feature map: layout 1 of lk_norm_fwd_f32 on the NHWC memory of the convolution output; returns the
        NCHW-logical view over NHWC memory, as `_run_bn_act` does.  Nothing is registered in ``_aux``: the next convolution
        measures and splits its input itself (`_split_input`).  A LayerNorm of the head region runs the parent's math."""
        if not (self.split_ok and isinstance(m, nn.GroupNorm)):
            return super()._run_norm(node, m, inp)
        # (also with ``nhwc_forward = False``: the reverse sweep is NHWC either way)
        if not (torch.is_tensor(inp) and inp.dim() == 4 and inp.dtype == torch.float32 and inp.shape[0] > 0):
            raise SweepUnsupported(f"{node.target}: GroupNorm of the NHWC sweep expects a non-empty fp32 feature map")
        if inp.shape[1] != m.num_channels:
            raise SweepUnsupported(f"{node.target}: GroupNorm({m.num_groups}, {m.num_channels}) on {tuple(inp.shape)}")
        xh = inp.permute(0, 2, 3, 1).contiguous()  # (a view when inp is already NHWC in memory)
        w = None if m.weight is None else m.weight.detach().to(torch.float32).contiguous()
        b = None if m.bias is None else m.bias.detach().to(torch.float32).contiguous()
        y, xhat, rstd = self.kernels().norm_forward(xh, w, b, m.num_groups, 1, m.eps)
        return y.permute(0, 3, 1, 2), (xhat, rstd, m.num_groups, 1)

    def _run_pool(self, node, r, args, kwargs):
        """max / average pooling on a feature map: lk_pool_fwd_nhwc_f32 on the NHWC memory of the input; returns the NCHW-logical
        view over NHWC memory, as `_run_norm` does, and keeps ``(arg, in_shape)`` (max: one byte of window-local argmax per
        output element, shared by all seeds) or ``in_shape`` (average).  Pooling cannot raise a map's maximum, so the output
        inherits the input's per-image ``"bound"`` words; no ``"split"`` is registered: the next convolution splits its input
        itself (`_split_input`)."""
        if not self.split_ok:
            return super()._run_pool(node, r, args, kwargs)
        # (also with ``nhwc_forward = False``: the reverse sweep is NHWC either way)
        inp = args[0]
        if not (torch.is_tensor(inp) and inp.dim() == 4 and inp.dtype == torch.float32):
            raise SweepUnsupported(f"{node.name}: pooling of the NHWC sweep expects an fp32 feature map")
        K, p = self.kernels(), self.pool_params(r)
        is_max = r.kind == MAXPOOL
        xh = inp.permute(0, 2, 3, 1).contiguous()  # (a view when inp is already NHWC in memory)
        y, arg = K.pool_forward(xh, K.POOL_MAX if is_max else K.POOL_AVG, p["kernel"], p["stride"], p["padding"],
                                p["count_include_pad"], p["divisor_override"])
        out = y.permute(0, 3, 1, 2)
        aux = self._aux_get(inp)
        # (an average with a divisor of its own may exceed the map's maximum: it inherits nothing)
        if aux is not None and aux.get("bound") is not None and (is_max or p["divisor_override"] is None):
            self._aux_put(out, {"split": None, "bound": aux["bound"]})
        return out, ((arg, inp.shape) if is_max else inp.shape)

    def _run_cat(self, node, r, tensors, dim):
        """concatenation of feature maps along the channels: ONE NHWC allocation ``[B, H, W, Ct]`` and one lk_cat_fwd_nhwc_f32 per
        source on the NHWC memory of each input; returns the NCHW-logical view over NHWC memory, as `_run_pool` does.  The output
        inherits a per-image ``"bound"``: the element-wise maximum of the sources' bound words when every source has one; no
        ``"split"`` is registered.  A concatenation of plain tensors in the head region runs the parent's math."""
        if not (self.split_ok and self._on_map(node)):
            return super()._run_cat(node, r, tensors, dim)
        # (also with ``nhwc_forward = False``: the reverse sweep is NHWC either way)
        if dim != 1 or not all(t.dim() == 4 and t.dtype == torch.float32 for t in tensors):
            raise SweepUnsupported(f"{node.name}: concatenation of the NHWC sweep expects fp32 feature maps and dim 1")
        y = self.kernels().cat_forward([t.permute(0, 2, 3, 1).contiguous() for t in tensors])  # (views of NHWC memory)
        out = y.permute(0, 3, 1, 2)
        bounds = [aux.get("bound") if aux is not None else None for aux in (self._aux_get(t) for t in tensors)]
        if all(b is not None and b.shape == bounds[0].shape and b.dtype == bounds[0].dtype for b in bounds):
            bound = bounds[0]
            for b in bounds[1:]:
                bound = torch.maximum(bound, b)
            self._aux_put(out, {"split": None, "bound": bound})
        return out

    def _run_slice(self, node, r, inp, dim, start, length, dropped):
        """channel slice of a feature map: ONE lk_slice_fwd_f32 launch on the ``[B H W][C]`` view of the input's NHWC memory into a
        contiguous NHWC map (what the convolutions read); returns the NCHW-logical view over NHWC memory, as `_run_cat` does.  A
        slice cannot raise a map's maximum, so the output inherits the input's per-image ``"bound"`` words; no ``"split"`` is
        registered.  A slice of a plain tensor in the head region is the parent's view."""
        if not (self.split_ok and self._on_map(node)):
            return super()._run_slice(node, r, inp, dim, start, length, dropped)
        # (also with ``nhwc_forward = False``: the reverse sweep is NHWC either way)
        if dim != 1 or dropped or not (inp.dim() == 4 and inp.dtype == torch.float32):
            raise SweepUnsupported(f"{node.name}: slicing of the NHWC sweep expects an fp32 feature map and a channel range")
        xh = inp.permute(0, 2, 3, 1).contiguous()  # (a view when inp is already NHWC in memory)
        B, H, W, C = xh.shape
        y = self.kernels().slice_forward(xh, B * H * W, C, start, length).reshape(B, H, W, length)
        out = y.permute(0, 3, 1, 2)
        aux = self._aux_get(inp)
        if aux is not None and aux.get("bound") is not None:
            self._aux_put(out, {"split": None, "bound": aux["bound"]})
        return out

    def _gate_is_bounded_by_one(self, n) -> bool:
        """is the value of node ``n`` in [0, 1] whatever its input (a Sigmoid / Hardsigmoid)?"""
        r = self.rule[n]
        if r.kind != ACT:
            return False
        if r.flavour == "sigmoid":
            return True
        if n.op == "call_module":
            return isinstance(self.modules.get(n.target), nn.Hardsigmoid)
        return n.op == "call_function" and n.target is torch.nn.functional.hardsigmoid

    def _run_mul(self, r, args):
        """a feature map times its ``[B, C, 1, 1]`` gate (``nhwc_mul``): torch's product on the NHWC memory of the map (1 / S of the
        sweep's work); returns the NCHW-logical view over NHWC memory, as `_run_pool` does, and keeps the map's ``[B, H, W, C]``
        view and the gate ``[B, C]`` for lk_gate.hip.  A gate in [0, 1] cannot raise the map's maximum, so the output then inherits
        the map's per-image ``"bound"`` words; otherwise nothing is registered.  Any other product runs the parent's math."""
        node = self._mul_node.get(id(r))
        if not (self.split_ok and node in self._gates):
            return super()._run_mul(r, args)
        gi, _, chain = self._gates[node]
        gate, x = args[gi], args[1 - gi]
        if not (torch.is_tensor(x) and x.dim() == 4 and x.dtype == torch.float32 and torch.is_tensor(gate)
                and gate.dtype == torch.float32 and tuple(gate.shape) == (x.shape[0], x.shape[1], 1, 1)):
            raise SweepUnsupported(f"{node.name}: the gate of the NHWC sweep expects an fp32 feature map [B, C, H, W] and a gate "
                                   f"[B, C, 1, 1], got {tuple(getattr(x, 'shape', ()))} and {tuple(getattr(gate, 'shape', ()))}")
        xh = x.permute(0, 2, 3, 1).contiguous()  # (a view when x is already NHWC in memory)
        g2 = gate.reshape(gate.shape[0], gate.shape[1]).contiguous()
        out = (xh * g2[:, None, None, :]).permute(0, 3, 1, 2)
        aux = self._aux_get(x)
        if aux is not None and aux.get("bound") is not None and self._gate_is_bounded_by_one(chain[-1]):
            self._aux_put(out, {"split": None, "bound": aux["bound"]})
        return out, ("gate", xh, g2)

    #: ``False``: a convolution and the BatchNorm / add / ReLU behind it stay two launches
    fuse_conv_bn = True

    def _bn_takes_conv(self, node, m, xs) -> bool:
        """does this convolution's output go to exactly one consumer, an eval-mode BatchNorm2d that the traced forward
        hands to ``_run_bn_act`` (laplace_amd/sweep.py: the conditions of its BatchNorm branch), so that both run as one
        launch?"""
        K = self.kernels()
        if not (self.fuse_conv_bn and getattr(K, "use_conv_bn_act", False) and m.bias is None and xs.amax is not None
                and xs.shape[0] <= getattr(K, "MAX_IMAGES_PER_LAUNCH", 65535) and m.out_channels % 8 == 0
                and len(node.users) == 1):
            return False
        nxt = next(iter(node.users))
        bn = self.rule[nxt].mod
        return (isinstance(bn, nn.BatchNorm2d) and len(nxt.args) == 1 and nxt.args[0] is node and not nxt.kwargs
                and bn.running_var is not None and nxt.target not in self.tap_names)

    def _run_bn_act(self, node, inp, scale, shift, relu, addend, want_mask):
        K = self.kernels()
        if isinstance(inp, _PendingConv):
            if addend is None or (torch.is_tensor(addend) and addend.dtype == torch.float32 and K.is_channels_last(addend)
                                  and addend.shape == inp.shape):
                a_h = a_bound = None
                if addend is not None:
                    a_h = addend.permute(0, 2, 3, 1)
                    a_aux = self._aux_get(addend)
                    a_bound = a_aux["bound"] if a_aux is not None and "bound" in a_aux else K.absmax(a_h)
                scale = scale.to(torch.float32).contiguous()
                shift = shift.to(torch.float32).contiguous()
                # `act_sink` (the KFAC accumulator): a tapped 3x3 convolution that reads this output may want it written straight
                # into its pixel-pair stack — the copy it would otherwise make of every activation (13 per c4 minibatch)
                y_out = None
                sink, fin = self.act_sink, getattr(self, "_group_out_node", None)
                if sink is not None and fin is not None:
                    for u in fin.users:
                        if u.op == "call_module" and u.target in self.tap_names and u.args and u.args[0] is fin:
                            y_out = sink(u.target, (inp.shape[0], inp.shape[2], inp.shape[3], inp.shape[1]), inp.device)
                            if y_out is not None:
                                break
                y, mask, split, bound = cv.conv_forward_bn_act(
                    inp.prep, inp.xs, scale, shift, self._amax_of((node.target, "s"), scale),
                    self._amax_of((node.target, "t"), shift), 1 if relu else 0, addend=a_h, addend_bound=a_bound,
                    want_mask=want_mask, amax_words=self._fwd_word(inp.device, inp.shape[0]), y_out=y_out)
                out = y.permute(0, 3, 1, 2)
                self._aux_put(out, {"split": split, "bound": split.amax if split is not None else bound})
                if mask is not None:
                    mask = mask.view(torch.bool).permute(0, 3, 1, 2)
                return out, mask
            inp = inp.materialize()
        if not (self._use_nhwc_forward(inp) and K.is_channels_last(inp) and inp.shape[1] % 8 == 0
                and (addend is None or K.is_channels_last(addend))):
            return super()._run_bn_act(node, inp, scale, shift, relu, addend, want_mask)
        aux = self._aux_get(inp)
        xh = inp.permute(0, 2, 3, 1)
        x_mul = x_add = None
        if aux is not None and "in_amax" in aux:
            x_amax, x_mul, x_add = aux["in_amax"], aux["mul"], aux["add"]
        else:
            x_amax = K.absmax(xh)  # (one bound for every image: coarser scales, still guaranteed)
        a_h = a_bound = None
        if addend is not None:
            a_h = addend.permute(0, 2, 3, 1)
            a_aux = self._aux_get(addend)
            a_bound = a_aux["bound"] if a_aux is not None and "bound" in a_aux else K.absmax(a_h)
        scale = scale.to(torch.float32).contiguous()
        shift = shift.to(torch.float32).contiguous()
        y, mask, split, bound = K.bn_act_forward_nhwc(xh, x_amax, scale, shift, self._amax_of((node.target, "s"), scale),
                                                      self._amax_of((node.target, "t"), shift), 1 if relu else 0,
                                                      addend=a_h, addend_bound=a_bound, want_mask=want_mask, x_mul=x_mul,
                                                      x_add=x_add, amax_words=self._fwd_word(inp.device, inp.shape[0]))
        out = y.permute(0, 3, 1, 2)
        # (the MEASURED per-image maxima are the bound a later residual join adds: tighter than the guaranteed one)
        self._aux_put(out, {"split": split, "bound": split.amax if split is not None else bound})
        if mask is not None:
            mask = mask.view(torch.bool).permute(0, 3, 1, 2)  # logical NCHW view of the NHWC mask bytes
        return out, mask

    # ---- helpers ----------------------------------------------------------------------------------------------------
    def _amax_of(self, key, t):
        """device word with max|t| of a per-model constant (BatchNorm scale), cached until it changes"""
        k = (t._version, t.data_ptr())
        hit = self._amax_cache.get(key)
        if hit is None or hit[0] != k:
            hit = (k, self.kernels().absmax(t.contiguous()))
            self._amax_cache[key] = hit
        return hit[1]

    def _nhwc_mult(self, walk, node, flavour):
        """per-sample multiplier of an activation as an NHWC tensor (+ its max| | word for generic derivatives)"""
        hit = walk.mult_cache.get(node)
        if hit is None:
            saved = self.saved[node]
            mult = self._act_mult(flavour, saved)
            if mult.dim() != 4:
                raise SweepUnsupported("activation on a non-feature-map tensor inside the NHWC region")
            amax = None
            if mult.dtype == torch.bool:
                mult = mult.permute(0, 2, 3, 1).contiguous().view(torch.uint8)
            else:
                mult = mult.to(torch.float32).permute(0, 2, 3, 1).contiguous()
                if flavour == "generic":  # tanh' and sigmoid' are bounded by 1; anything else is measured
                    amax = self.kernels().absmax(mult)
            hit = (mult, amax)
            walk.mult_cache[node] = hit
        return hit

    def _to_split(self, walk, parts, mult=None, mult_amax=None, scale=None, scale_amax=None):
        """sum of cotangent parts (x multiplier x channel scale) -> one SplitTensor"""
        K, S = self.kernels(), walk.S
        lazy = [p for p in parts if isinstance(p, _LazyConv)]
        if lazy:
            rest = [p for p in parts if not isinstance(p, _LazyConv)]
            strided = [p for p in lazy if isinstance(p, _LazyStrided)]
            if (strided and len(strided) == len(lazy) <= 2 and all(p._done is None and p.hw == strided[0].hw for p in strided)
                    and len(rest) <= 1 and all(isinstance(p, SplitTensor) for p in rest)
                    and cv.strided_taps([p.desc for p in strided], strided[0].hw) is not None):
                return cv.conv_backward_data_vjp_strided(
                    [p.desc for p in strided], strided[0].hw, add=rest[0] if rest else None, mult=mult, mult_amax=mult_amax,
                    scale=scale, scale_amax=scale_amax, amax_word=walk.new_word())
            if len(lazy) == 1 and not strided and lazy[0]._done is None and len(rest) <= 1 and all(isinstance(p, SplitTensor) for p in rest):
                return lazy[0].fused(add=rest[0] if rest else None, mult=mult, mult_amax=mult_amax, scale=scale,
                                     scale_amax=scale_amax, amax_word=walk.new_word())
            parts = _materialize(parts)
        f32 = [p for p in parts if isinstance(p, _F32)]
        spl = [p for p in parts if isinstance(p, SplitTensor)]
        if len(f32) > 1:  # (no graph of the supported families gets here: two un-activated conv branches joining)
            t = f32[0].t
            for p in f32[1:]:
                t = t + p.t
            f32 = [_F32(t, K.absmax(t))]
        if len(spl) > 1:  # several split addends (rare: joins of more than two branches): fold them through fp32
            t = spl[0].float()
            for p in spl[1:]:
                t = t + p.float()
            if f32:
                t = t + f32[0].t
            t = t.contiguous()
            f32, spl = [_F32(t, K.absmax(t))], []
        g = f32[0] if f32 else None
        g2 = spl[0] if spl else None
        if g is None and mult is None and scale is None:
            return g2
        shape = g.t.shape if g is not None else g2.shape
        return K.vjp_nhwc_split(None if g is None else g.t, None if g is None else g.amax, g2, mult, mult_amax, scale,
                                scale_amax, S, tuple(shape))

    # ---- reverse sweep ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def backward(self, seeds, on_tap=None, defer_bn_scale: bool = False, keep_split: bool = False):
        """``keep_split``: hand conv-tap gradients back as NHWC SplitTensors (consumers with their own kernels for
        them) instead of converting to ``[S, B, C, H, W]`` fp32.  Norm-tap gradients (``nhwc_norm_taps``) always leave in NHWC
        form: the unscaled SplitTensor of a BatchNorm's output cotangent, a :class:`NhwcNormGrad` for a GroupNorm."""
        if not self.split_ok:
            return super().backward(seeds, on_tap=on_tap, defer_bn_scale=defer_bn_scale)
        walk = _NhwcWalk(self, seeds, on_tap, defer_bn_scale, keep_split)
        self.grad_scale = walk.grad_scale
        for node, r in reversed(self.rule.items()):
            parts = self._nhwc_parts(walk, node, r)
            if parts is not None and self._nhwc_vjp_rule(node, r, parts)(walk, node, r, parts):
                break  # (a rule returns ``True`` when its tap was the last one owed)
        if walk.remaining:
            raise SweepUnsupported(f"no cotangent reached {sorted(walk.remaining)}")
        grads = walk.grads
        if on_tap is None and not keep_split:
            # consumers that read the gradients as tensors (Jacobians, diagonal, predictive): [S, B, C, H, W] fp32
            for name, g in list(grads.items()):
                if isinstance(g, SplitTensor) and name not in walk.norm_names:
                    t = g.float()
                    if name in walk.owed:
                        t = t * walk.owed[name]  # (channels are the last dim here)
                    grads[name] = t.reshape(walk.S, walk.B, *g.shape[1:]).permute(0, 1, 4, 2, 3).contiguous()
        return grads

    def _nhwc_parts(self, walk, node, r):
        """the cotangent parts of ``node`` as its rule takes them, or ``None`` where no cotangent reached it: deferred strided
        branches run or added in, lazy convolutions materialised for every kind but `_LAZY`, the pieces of its SLICE consumers
        assembled with the full-width parts"""
        cot, deferred, pieces = walk.cot, walk.deferred, walk.pieces
        if node in deferred and node not in cot:
            # nothing else reached this node: the deferred branches produce the cotangent on their own
            cot[node] = [_run_deferred(deferred.pop(node))]
        if node not in cot and node not in pieces:
            return None
        parts = cot.pop(node, [])
        if node in deferred or node in pieces or r.kind not in _LAZY:
            parts = _materialize(parts)
        if node in pieces:
            pcs = pieces.pop(node)
            SB = walk.S * walk.B
            if torch.is_tensor(pcs[0][0]):
                # slices in the head region (plain tensors after the flatten): parent-class math
                parts = [self._assemble_slices(parts, [p[:4] for p in pcs], (SB,) + tuple(pcs[0][4][1:]))]
            else:
                # ONE launch: the full-width parts and the channel pieces, as they lie, summed into an fp32 map with its max|.|
                Ct = int(pcs[0][4][1])
                ops = [(p if isinstance(p, SplitTensor) else p.t, 0, Ct) for p in parts]
                ops += [(p if isinstance(p, SplitTensor) else p.t, start, length) for p, _, start, length, _ in pcs]
                shape, word = (SB, int(pcs[0][4][2]), int(pcs[0][4][3]), Ct), walk.new_word()
                t = self.slice_vjp_launches(walk.K, ops, shape[0] * shape[1] * shape[2], Ct, amax=word)
                parts = [_F32(t.reshape(shape), word)]
        if node in deferred:
            f32p = [p for p in parts if isinstance(p, _F32)]
            fns = deferred.pop(node)
            if f32p:
                for fn in fns:
                    fn(f32p[0])
            else:
                parts.append(_run_deferred(fns))
        return parts

    #: kind -> the method that pushes a node's cotangent parts on to its sources, ``(walk, node, r, parts) -> True`` when its tap
    #: was the last one the walk owed.  The kinds of `_HEAD` that are missing here live in the head region only
    _NHWC_VJP = {CONV: "_nhwc_vjp_conv", BN: "_nhwc_vjp_bn", NORM: "_nhwc_vjp_norm", MAXPOOL: "_nhwc_vjp_pool",
                 AVGPOOL: "_nhwc_vjp_pool", ACT: "_nhwc_vjp_act", IDENTITY: "_nhwc_vjp_identity", ADD: "_nhwc_vjp_add",
                 CAT: "_nhwc_vjp_cat", SLICE: "_nhwc_vjp_slice", MUL: "_nhwc_vjp_gate", GPOOL: "_nhwc_vjp_gpool"}

    def _nhwc_vjp_rule(self, node, r, parts):
        """the bound method that serves ``node``: the head-region fallback, its rule of `_NHWC_VJP`, or the refusal by name"""
        if r.kind in _HEAD and node not in self._gates:
            if all(torch.is_tensor(p) for p in parts):
                return self._head_vjp
            if _HEAD[r.kind] is not None:
                raise SweepUnsupported(_HEAD[r.kind])
        name = self._NHWC_VJP.get(r.kind)
        if name is None:
            raise SweepUnsupported(f"no NHWC rule for {r.what}")
        return getattr(self, name)

    def _head_vjp(self, walk, node, r, parts):
        """a node of the head region (plain tensors after the flatten): the parent's rule for its kind on the sum of the parts
        (an activation without a second addend; a 4-D result of a reshape is a feature map again)"""
        g = _sum(parts)
        if r.mod is not None and node.target in self.tap_names and walk.tap(node.target, g.reshape(walk.S, walk.B, *g.shape[1:])):
            return True
        if r.kind == RESHAPE:
            self._vjp_reshape(walk, node, r, g, None, as_map=walk.feature_f32)
        else:
            self._vjp_rule(r)(walk, node, r, g, None)

    def _nhwc_vjp_conv(self, walk, node, r, parts):
        m, src, K = r.mod, r.src[0], walk.K
        g = self._to_split(walk, parts)
        if node.target in self.tap_names:
            if node in walk.own_scale:
                walk.owed[node.target] = walk.pending_scale[node]
            elif node in walk.pending_scale:
                walk.grad_scale[node.target] = walk.pending_scale[node]
            if walk.tap(node.target, g):
                return True
        if src.op == "placeholder":
            return
        if self._is_depthwise(m):
            # one launch for all seeds into fp32 (lk_dwconv_bwd_nhwc_f16x2): no lazy part, no fused epilogue
            prep = self._prep.get(node.target)
            if prep is None:
                prep = self._prep[node.target] = cv.PreparedDepthwise(m)
            in_shape, word = self.saved[node], walk.new_word()  # [B, C, Hin, Win]
            walk.push(src, _F32(K.dwconv_backward(g, prep.w_tap, walk.S, (int(in_shape[2]), int(in_shape[3])), m.kernel_size,
                                                  m.stride, m.padding, amax=word), word))
            return
        prep = self._prep.get(node.target)
        if prep is None:
            prep = self._prep[node.target] = cv.PreparedConv(m)
        in_shape = self.saved[node]  # [B, Cin, Hin, Win]
        hw = (int(in_shape[2]), int(in_shape[3]))
        cscale = walk.pending_scale.get(node)
        sparse = any(not p[4] for p in cv.backward_plan(m, *hw))

        def run(into):
            if into is None:
                w = walk.new_word()
                out = cv.conv_backward_data(prep, g, hw, cscale=cscale, amax_out=w)
                return _F32(out, w)
            cv.conv_backward_data(prep, g, hw, cscale=cscale, out=into.t, accumulate=True, amax_out=into.amax)
            return into

        cot, deferred = walk.cot, walk.deferred
        if (self.fuse_vjp and self.fuse_strided and cv.strided_fused_ok(m, hw) and src not in deferred
                and hasattr(K, "conv_nhwc_f16x2_vjp_strided")
                and all(isinstance(p, (_LazyStrided, SplitTensor)) for p in cot.get(src, []))):
            # (the consumer of the cotangent decides: alone or with the block's other strided branch in one
            # fused launch, or — something else joined — class by class into an fp32 tensor)
            walk.push(src, _LazyStrided(run, (prep, g, cscale), hw))
            return
        if src in cot:
            cot[src] = _materialize(cot[src])
        existing = [p for p in cot.get(src, []) if isinstance(p, _F32)]
        if existing:
            run(existing[0])
        elif sparse and len(src.users) > 1:
            deferred.setdefault(src, []).append(run)  # wait for the dense branch, then add into it
        elif self.fuse_vjp and cv.fused_backward_ok(m) and hasattr(K, "conv_nhwc_f16x2_vjp"):
            def run_fused(**kw):
                return cv.conv_backward_data_vjp(prep, g, hw, cscale=cscale, **kw)

            walk.push(src, _LazyConv(lambda: run(None), run_fused))
        else:
            walk.push(src, run(None))

    def _nhwc_vjp_bn(self, walk, node, r, parts):
        src, scale = r.src[0], self._bn_scale(node.target, r.mod)
        if node.target in self.tap_names:
            # the cotangent of the BatchNorm's OWN output, unscaled, as one split tensor: what lk_normtap.hip reads
            u = parts[0] if len(parts) == 1 and isinstance(parts[0], SplitTensor) else self._to_split(walk, parts)
            walk.norm_names.add(node.target)
            if walk.tap(node.target, u):
                return True
            # the scale: left to the source convolution's backward-data launch (no pass over the cotangent) where that
            # convolution reads nothing else; a tapped one's own gradient is then owed the scale, which only the fp32
            # conversion at the end can pay unasked
            rs = self.rule.get(src)
            lone = (rs is not None and rs.kind == CONV and len(src.users) == 1 and src not in walk.cot
                    and not self._is_depthwise(rs.mod))
            src_tapped = lone and src.target in self.tap_names
            if lone and (not src_tapped or walk.defer_bn_scale or (walk.on_tap is None and not walk.keep_split)):
                walk.pending_scale[src] = scale
                if src_tapped and not walk.defer_bn_scale:
                    walk.own_scale.add(src)
                walk.push(src, u)
            else:
                walk.push(src, self._to_split(walk, [u], scale=scale, scale_amax=self._amax_of(node.target, scale)))
        elif (walk.defer_bn_scale and self._defers_scale_to(src, walk.cot) and len(parts) == 1
                and isinstance(parts[0], SplitTensor)):
            walk.pending_scale[src] = scale
            walk.push(src, parts[0])
        else:
            walk.push(src, self._to_split(walk, parts, scale=scale, scale_amax=self._amax_of(node.target, scale)))

    def _nhwc_vjp_norm(self, walk, node, r, parts):
        """GroupNorm on a feature map: the parts as ONE fp32 NHWC tensor (the VJP reads fp32; a kernel that reads split planes is
        out of scope)"""
        m = r.mod
        g = _sum(_as_f32(parts)).contiguous()
        xhat, rstd, G, _ = self.saved[node]
        w = None if m.weight is None else m.weight.detach().to(torch.float32).contiguous()
        if node.target in self.tap_names:
            # the Jacobian's operands as they lie (layout 1 of lk_jac_norm_affine_f32): no recomputed xhat, no NCHW copy
            walk.norm_names.add(node.target)
            if walk.tap(node.target, NhwcNormGrad(g, xhat)):
                return True
        word = walk.new_word()
        walk.push(r.src[0], _F32(walk.K.norm_vjp(g, xhat, rstd, w, walk.S, G, 1, amax=word), word))

    def _nhwc_vjp_pool(self, walk, node, r, parts):
        """max / average pooling: the parts as ONE fp32 NHWC tensor, as the NORM rule (a pool that reads split planes is out of
        scope)"""
        K, is_max = walk.K, r.kind == MAXPOOL
        g = _sum(_as_f32(parts))
        pp, keep = self.pool_params(r), self.saved[node]
        arg, shp = keep if is_max else (None, keep)  # [B, C, H, W]
        word = walk.new_word()
        dx = K.pool_vjp(g.contiguous(), arg, walk.S, (int(shp[2]), int(shp[3])), K.POOL_MAX if is_max else K.POOL_AVG,
                        pp["kernel"], pp["stride"], pp["padding"], pp["count_include_pad"], pp["divisor_override"], amax=word)
        walk.push(r.src[0], _F32(dx, word))

    def _nhwc_vjp_act(self, walk, node, r, parts):
        scale, dst = self._fold_bn(r.src[0])
        mult, mult_amax = self._nhwc_mult(walk, node, r.flavour)
        scale_amax = None if scale is None else self._amax_of(r.src[0].target, scale)
        walk.push(dst, self._to_split(walk, parts, mult=mult, mult_amax=mult_amax, scale=scale, scale_amax=scale_amax))

    def _nhwc_vjp_identity(self, walk, node, r, parts):
        for p in parts:
            walk.push(r.src[0], p)

    def _nhwc_vjp_add(self, walk, node, r, parts):
        for a in r.src:
            for p in parts:
                walk.push(a, p)

    def _nhwc_vjp_cat(self, walk, node, r, parts):
        """concatenation of feature maps: one launch per source writes its channel slice of the sum of the parts, as they lie"""
        K = walk.K
        dim, sizes = self.saved[node]
        if len(parts) > K.CAT_MAX_PARTS:  # the surplus as ONE fp32 tensor (rare: a map read by more than four nodes)
            parts = parts[:K.CAT_MAX_PARTS - 1] + [_F32(_sum(_as_f32(parts[K.CAT_MAX_PARTS - 1:])).contiguous(), None)]
        ops, off = [p if isinstance(p, SplitTensor) else p.t for p in parts], 0
        for a, n in zip(r.src, sizes):  # one launch per source: its slice of the sum, and max|.| of it
            if walk.live(a):
                word = walk.new_word()
                walk.push(a, _F32(K.cat_vjp(ops, off, n, amax=word), word))
            off += n

    def _nhwc_vjp_slice(self, walk, node, r, parts):
        """channel slice of a feature map: the parts as they lie (split tensors and fp32 maps) are channels
        [start, start + length) of the source"""
        dim, start, length, dropped, in_shape = self.saved[node]
        if walk.live(r.src[0]):
            for p in parts:
                walk.pieces.setdefault(r.src[0], []).append((p, dim, start, length, in_shape))

    def _nhwc_vjp_gate(self, walk, node, r, parts):
        """a feature map times its gate (lk_gate.hip).  The cotangent as ONE operand, as it lies (several parts: folded through
        fp32, as the NORM rule does)"""
        K, S, SB = walk.K, walk.S, walk.S * walk.B
        _, x_node, chain = self._gates[node]
        _, xh, gate = self.saved[node]
        if len(parts) == 1:
            op = parts[0] if isinstance(parts[0], SplitTensor) else parts[0].t
        else:
            op = _sum(_as_f32(parts)).contiguous()
        C = int(xh.shape[3])
        # ds [S*B, C], the cotangent of the [B, C, 1, 1] gate: one launch for all seeds
        t = K.gate_reduce(op, xh, S).reshape(SB, C, 1, 1)
        # the chain back to the pooled tensor on plain [S*B, ...] tensors; its taps leave as the NCHW sweep hands them out
        for n in reversed(chain[1:]):
            rn = self.rule[n]
            if rn.kind == ACT:
                t = self._scale_mask(t, S, self._act_mult(rn.flavour, self.saved[n]), None)
            elif rn.kind in (CONV, LINEAR):
                if n.target in self.tap_names:
                    walk.tap(n.target, t.reshape(S, walk.B, *t.shape[1:]))
                w = rn.mod.weight
                if rn.kind == CONV:
                    t = (t.reshape(SB, -1) @ w.reshape(w.shape[0], w.shape[1])).reshape(SB, w.shape[1], 1, 1)
                else:
                    t = t @ w
            elif rn.kind == RESHAPE:
                t = t.reshape((SB,) + tuple(self.saved[n])[1:])
        if not walk.remaining:
            return True  # (only after the whole chain: every tap of it has left)
        if walk.live(x_node):
            # the pooled tensor's cotangent, divided by H W, rides on the gate's VJP: ONE launch writes the map's cotangent
            rp = (t.reshape(SB, C) / float(xh.shape[1] * xh.shape[2])).contiguous()
            word = walk.new_word()
            walk.push(x_node, _F32(K.gate_vjp(op, gate, rp, S, amax=word), word))

    def _nhwc_vjp_gpool(self, walk, node, r, parts):
        shp, p = self.saved[node], parts[0]  # [B, C, H, W]
        if len(parts) != 1 or not isinstance(p, _F32):
            raise SweepUnsupported("global average pooling expects one fp32 cotangent")
        H, W = int(shp[-2]), int(shp[-1])
        t = (p.t / (H * W)).expand(walk.S * walk.B, H, W, p.t.shape[-1]).contiguous()
        walk.push(r.src[0], _F32(t, walk.K.absmax(t)))
