"""Extraction of per-layer inputs ``a`` and output gradients ``g`` from stock autograd.

Host-side plumbing around the model (the model forward/backward stays PyTorch-ROCm): one forward
with hooks on the supported modules, then reverse passes that deliver, for every seed (a column of
the likelihood-Hessian root), the gradient w.r.t. every tapped module's *output* — no weight
gradients are ever formed and there is no second forward for the loss (cf. the reference's default
backend, laplace/curvature/curvlinops.py:87-106, and the ``jacrev`` materialisation of
laplace/curvature/curvature.py:88-129).  Pure-Linear models use one vmapped pass
(``is_grads_batched``); conv models run one pass per seed and hand the per-seed gradients to the
Gram kernel unstacked.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import torch
from torch import nn

from laplace_amd import mha
from laplace_amd.conv import lift_maps

SUPPORTED = (nn.Linear, nn.Conv2d, nn.Conv1d)
#: convolution modules: an nn.Conv1d is served AS the unit-height nn.Conv2d it equals (`laplace_amd.conv.lift`): its taps carry the
#: kinds of a Conv2d ('conv2d', 'gconv'), their ``a`` and output gradients arrive lifted to ``[B, C, 1, L]`` / ``[S, B, C, 1, L']``
CONV = (nn.Conv2d, nn.Conv1d)
#: affine normalisation layers: their weight / bias Jacobian is a per-channel reduction of ``g * xhat`` (csrc/lk_norm.hip)
NORM = (nn.BatchNorm1d, nn.BatchNorm2d, nn.LayerNorm, nn.GroupNorm, nn.RMSNorm)
#: the tap kinds beyond Linear / dense Conv2d, in the order in which `Tape.active_taps` appends them (= the order of `grad_fn`'s
#: gradients).  A ROUTE is a frozenset of these kinds: what one call taps beside `Tape.taps`
EXTRA_KINDS = ("gconv", "norm", "embed", "param")


@dataclass
class Tap:
    name: str
    module: nn.Module
    kind: str  # 'linear' | 'conv2d' | 'gconv' | 'norm' | 'embed' | 'param'
    w_off: int  # column offset of the weight in the flattened parameter vector (a norm tap: -1 if absent / frozen)
    b_off: int  # column offset of the bias, -1 if the module has no (tracked) bias
    a: torch.Tensor | None = None  # module input (detached)
    a_split: object | None = None  # the same input as an NHWC SplitTensor, when the forward pass produced one
    out: object | None = None  # gradient edge of the module output in the autograd graph
    # the nn.MultiheadAttention a 'linear' tap is one half of (`laplace_amd.mha.lift`: ``module`` is that half's nn.Linear view,
    # which holds the real parameters and never runs itself); ``None`` for every other tap
    owner: nn.Module | None = None

    @property
    def has_bias(self) -> bool:
        return self.b_off >= 0


class MhaTapRefused(NotImplementedError):
    """a tapped nn.MultiheadAttention was called in a way that is not served as Linear, attention, Linear (a mask,
    cross-attention, ...: `laplace_amd.mha.refusal`); ``name``: the module.  The caller drops its taps (`Tape.drop_mha`): the
    module's parameters are ``uncovered`` from then on"""

    def __init__(self, name, why):
        super().__init__(f"{name}: {why}")
        self.name = name


class NormTapReused(NotImplementedError):
    """a tapped normalisation layer ran twice in one forward: the caller goes back to the route without norm taps"""


class EmbedTapForeign(NotImplementedError):
    """a tapped nn.Embedding does not read the model's input (a position table written ``nn.Embedding(arange)``): its cotangent is
    not per sample; the caller goes back to the route without embedding taps"""


def norm_servable(m: nn.Module) -> bool:
    """Is the layer, as it stands NOW, an affine map of a per-sample ``xhat``?  A BatchNorm in training mode or without
    running statistics normalises with the statistics of the batch: its Jacobian mixes samples."""
    if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
        return not m.training and m.running_mean is not None and m.running_var is not None
    return True


def _conv_checks(m, name: str):
    if isinstance(m.padding, str):
        raise NotImplementedError(f"{name}: string padding ('{m.padding}') not supported")
    if m.padding_mode != "zeros":
        raise NotImplementedError(f"{name}: padding_mode={m.padding_mode!r} not supported")


class Tape:
    """Finds the supported modules whose weight is Laplace-tracked (``named_modules`` order, as
    laplace/curvature/curvlinops.py:55-75) and records their inputs/outputs during a forward."""

    def __init__(self, model: nn.Module, params: Sequence[nn.Parameter]):
        self.model = model
        self._params = list(params)
        offsets, off = {}, 0
        for p in params:
            offsets[id(p)] = off
            off += p.numel()
        self.n_params = off
        self.taps: list[Tap] = []
        covered = set()
        # nn.MultiheadAttention: served as the two nn.Linear layers around its attention core (`laplace_amd.mha.lift`), both
        # 'linear' taps at the module's place in this order.  Its real ``out_proj`` is an nn.Linear that never runs (the
        # module's forward reads the raw weights): never tapped itself.  What `mha.refusal` names stays in `uncovered`
        self.mha_refused: dict[str, str] = {}
        never_run = {id(m.out_proj) for m in model.modules() if isinstance(m, nn.MultiheadAttention)}
        for name, mod in model.named_modules():
            if isinstance(mod, nn.MultiheadAttention):
                why = mha.refusal(mod)
                if why is not None:
                    self.mha_refused[name] = f"{name}: {why}"
                    continue
                for half, lin in zip(("in_proj", "out_proj"), mha.lift(mod)):
                    if id(lin.weight) not in offsets or id(lin.weight) in covered:
                        continue
                    b_off = -1
                    if lin.bias is not None and id(lin.bias) in offsets:
                        b_off = offsets[id(lin.bias)]
                        covered.add(id(lin.bias))
                    covered.add(id(lin.weight))
                    self.taps.append(Tap(f"{name}.{half}", lin, "linear", offsets[id(lin.weight)], b_off, owner=mod))
                continue
            if not isinstance(mod, SUPPORTED) or id(mod.weight) not in offsets or id(mod) in never_run:
                continue
            if isinstance(mod, CONV):
                _conv_checks(mod, name)
                if mod.groups != 1:
                    continue  # (a tap list of its own, below)
            b_off = -1
            if mod.bias is not None and id(mod.bias) in offsets:
                b_off = offsets[id(mod.bias)]
                covered.add(id(mod.bias))
            covered.add(id(mod.weight))
            self.taps.append(Tap(name, mod, "linear" if isinstance(mod, nn.Linear) else "conv2d",
                                 offsets[id(mod.weight)], b_off))
        # tracked parameters that no supported module owns (norm layers, embeddings, lone biases ...)
        self.uncovered = [p for p in params if id(p) not in covered]
        # grouped convolutions (groups > 1) with a tracked weight, in a list of their own: no KFAC rule exists for them, their
        # Jacobian block comes from csrc/lk_gconv.hip.  Their parameters stay in `uncovered`, which keeps meaning "no
        # Linear / dense Conv2d owns it" (what the KFAC accumulator, the Kron predictive and the batched grids refuse on).
        self.gconv_taps: list[Tap] = []
        for name, mod in model.named_modules():
            if isinstance(mod, CONV) and mod.groups != 1 and id(mod.weight) in offsets:
                b_off = offsets[id(mod.bias)] if mod.bias is not None and id(mod.bias) in offsets else -1
                self.gconv_taps.append(Tap(name, mod, "gconv", offsets[id(mod.weight)], b_off))
        # affine normalisation layers with a tracked weight and / or bias, in a list of their own: `taps` stays the list
        # of Linear / Conv2d layers that the KFAC accumulator, the Kron predictive and the last-layer shortcut walk
        self.norm_taps: list[Tap] = []
        for name, mod in model.named_modules():
            if not isinstance(mod, NORM):
                continue
            w_off = b_off = -1
            if getattr(mod, "weight", None) is not None and id(mod.weight) in offsets and id(mod.weight) not in covered:
                w_off = offsets[id(mod.weight)]
            if getattr(mod, "bias", None) is not None and id(mod.bias) in offsets and id(mod.bias) not in covered:
                b_off = offsets[id(mod.bias)]
            if w_off >= 0 or b_off >= 0:
                self.norm_taps.append(Tap(name, mod, "norm", w_off, b_off))
        # nn.Embedding layers with a tracked weight that no other module owns, in a list of their own (csrc/lk_embed.hip).  What
        # is refused by name in `embed_refused` (module name -> reason) stays unserved: a weight tied to a Linear head,
        # `max_norm` (the forward renormalises the rows in place), `scale_grad_by_freq`, `sparse=True`, nn.EmbeddingBag.
        self.embed_taps: list[Tap] = []
        self.embed_refused: dict[str, str] = {}
        for name, mod in model.named_modules():
            if isinstance(mod, nn.EmbeddingBag) and id(mod.weight) in offsets:
                self.embed_refused[name] = f"{name}: nn.EmbeddingBag has no device rule"
            if not isinstance(mod, nn.Embedding) or id(mod.weight) not in offsets:
                continue
            why = None
            if id(mod.weight) in covered:
                why = "its weight is tied to a Linear / Conv2d layer"
            elif mod.max_norm is not None:
                why = "max_norm renormalises the weight in the forward pass"
            elif mod.scale_grad_by_freq:
                why = "scale_grad_by_freq has no device rule"
            elif mod.sparse:
                why = "sparse=True has no device rule"
            elif any(t.module.weight is mod.weight for t in self.embed_taps):
                why = "its weight is shared with another nn.Embedding"
            if why is not None:
                self.embed_refused[name] = f"{name}: nn.Embedding is not served ({why})"
                continue
            self.embed_taps.append(Tap(name, mod, "embed", offsets[id(mod.weight)], -1))
        # tracked parameters that NO module of the model owns (a class token, a learned position table: bare nn.Parameter
        # attributes), served only by the seed-batched sweep (autograd alone yields their batch-summed gradient); `name`: the
        # attribute path, which is what the traced graph's `get_attr` node names
        self.param_taps: list[Tap] = []
        for name, p in model.named_parameters():
            if id(p) in offsets and isinstance(p, nn.Parameter) and self._is_lone(model, name):
                self.param_taps.append(Tap(name, None, "param", offsets[id(p)], -1))
        self._lone = {t.name: p for t in self.param_taps for n, p in model.named_parameters() if n == t.name}
        self.extra_taps = {"gconv": self.gconv_taps, "norm": self.norm_taps, "embed": self.embed_taps, "param": self.param_taps}
        self.route = frozenset()  # the route of the latest forward
        self.disabled: set[str] = set()  # kinds that a forward of this model found it cannot tap: off from then on
        self.sweeps: dict = {}  # route -> the reverse sweep that taps it (False: the model has none, `sweep_reason` says why)

    @staticmethod
    def _is_lone(model, path) -> bool:
        """is the parameter ``path`` a bare attribute of a module that does not use it as a layer parameter?  (Linear, Conv2d,
        the norm layers and Embedding own theirs; every module type this package taps is a leaf of torch.nn)"""
        owner = model
        for part in path.split(".")[:-1]:
            owner = getattr(owner, part)
        return not type(owner).__module__.startswith("torch.nn.")

    @property
    def sweep(self):
        """the sweep of the empty route (Linear / Conv2d taps only); ``None`` before one was built"""
        return self.sweeps.get(frozenset())

    def owned(self, kind: str):
        """the parameters that the taps of one extra kind own - decided per call for ``norm``: a BatchNorm switched to training
        mode (or one without running statistics) is not served"""
        if kind == "param":
            return list(self._lone.values())
        # (nn.RMSNorm and nn.Embedding have no bias attribute)
        return [p for t in self.extra_taps[kind] if kind != "norm" or norm_servable(t.module)
                for p in (t.module.weight, getattr(t.module, "bias", None)) if p is not None]

    @property
    def unserved(self):
        """``uncovered`` minus what the norm taps own: embeddings, lone parameters, ... are not served"""
        return self.unserved_by(frozenset({"norm"}))

    def refuse_kfac(self):
        """KFAC (the accumulator, ``kron``, the Kron predictive) has no rule for a grouped convolution: what the reference's
        KFAC (curvlinops) does with ``groups > 1`` is not pinned by any golden here, so nothing is guessed.  A dense nn.Conv1d is
        NOT refused and nothing is guessed for it either: it is served as the nn.Conv2d with a unit-height window that computes
        the same function of the same parameter vector in the same order, and its factors are the reference's Conv2d factors of
        that layer (the oracle computes them on the model's 2-D twin); a grouped Conv1d is refused like a grouped Conv2d"""
        if self.gconv_taps:
            t = self.gconv_taps[0]
            raise NotImplementedError(f"{t.name}: KFAC has no rule for a grouped convolution (groups={t.module.groups}); "
                                      "freeze the layer (requires_grad=False) or use hessian_structure 'diag' or 'full'")

    def unserved_by(self, route):
        """``uncovered`` minus what the taps of the kinds in ``route`` own"""
        owned = {id(p) for kind in route for p in self.owned(kind)}
        return [p for p in self.uncovered if id(p) not in owned]

    def active_taps(self, route=frozenset()):
        """the taps of one call, in the order in which ``grad_fn`` returns their gradients"""
        return self.taps + [t for kind in EXTRA_KINDS if kind in route for t in self.extra_taps[kind]]

    def forward(self, x, route=frozenset()):
        """Run ``model(x)`` with hooks; returns ``f`` (attached to the graph).  ``route``: the extra kinds tapped too (an
        embedding's ``tap.a``: the token ids).  Lone parameters have no module to hook (``"param"`` is ignored): the seed-batched
        sweep alone serves them."""
        handles, seen = [], set()
        self._active = self.active_taps(route - {"param"})
        for owner in {id(t.owner): t.owner for t in self._active if t.owner is not None}.values():
            handles.append(owner.register_forward_hook(self._mha_hook(owner, seen), with_kwargs=True))
        for tap in self._active:
            if tap.owner is not None:
                continue
            def hook(m, inp, out, tap=tap):
                if id(m) in seen:
                    if tap.kind == "norm":
                        raise NormTapReused(f"{tap.name}: module is applied more than once per forward")
                    raise NotImplementedError(f"{tap.name}: module is applied more than once per forward")
                seen.add(id(m))
                if tap.kind == "embed" and inp[0] is not x:
                    raise EmbedTapForeign(f"{tap.name}: the Embedding does not read the model's input")
                tap.a = lift_maps(m, inp[0].detach())[0]
                # the gradient EDGE of the output as it is now: models that go on to modify the tensor in place
                # (torchvision's `out += identity; relu_(out)`) would otherwise hand back the gradient w.r.t. the
                # mutated tensor — the reference's curvlinops hooks see the pre-mutation gradient as well
                tap.out = torch.autograd.graph.get_gradient_edge(out) if out.requires_grad else out
            handles.append(tap.module.register_forward_hook(hook))
        try:
            with torch.enable_grad():
                f = self.model(x)
        finally:
            for h in handles:
                h.remove()
        for tap in self._active:
            if tap.out is None:
                raise RuntimeError(f"{tap.name}: module did not run in the forward pass")
        return f

    def _mha_hook(self, owner, seen):
        """the forward hook of a tapped nn.MultiheadAttention: evaluates what the module equals - ``F.linear``, scaled dot-product
        attention, ``F.linear`` on the module's own parameters (`laplace_amd.mha.decomposed`) - from the module's input and
        returns that value as the module's output, so that the inputs and the gradient edges of both halves exist"""
        halves = {t.name.rsplit(".", 1)[1]: t for t in self._active if t.owner is owner}
        name = next(iter(halves.values())).name.rsplit(".", 1)[0]

        def hook(m, args, kwargs, out):
            if id(m) in seen:
                raise NotImplementedError(f"{name}: module is applied more than once per forward")
            seen.add(id(m))
            why = mha.refusal(m, (args, kwargs))
            if why is not None:
                raise MhaTapRefused(name, why)
            y, qkv, ctx = mha.decomposed(m, args[0] if args else kwargs["query"])
            for half, a, t in (("in_proj", args[0] if args else kwargs["query"], qkv), ("out_proj", ctx, y)):
                if half in halves:
                    halves[half].a = a.detach()
                    halves[half].out = torch.autograd.graph.get_gradient_edge(t) if t.requires_grad else t
            weights = out[1]
            if weights is not None and weights.requires_grad:  # (the taps see the path through the output only)
                def consumed(_):
                    raise NotImplementedError(f"{name}: nn.MultiheadAttention whose attention weights are consumed is not served "
                                              "(call it with need_weights=False, or freeze the module)")
                weights.register_hook(consumed)
            return y, weights

        return hook

    def drop_mha(self, name: str, why: str):
        """stop serving the nn.MultiheadAttention ``name`` (a call of it was refused): its taps leave `taps`, its parameters are
        `uncovered` from here on, and the sweeps built for the old tap list are forgotten"""
        gone = [t for t in self.taps if t.owner is not None and t.name.rsplit(".", 1)[0] == name]
        self.taps = [t for t in self.taps if t not in gone]
        back = {id(p) for t in gone for p in (t.module.weight, t.module.bias) if p is not None}
        self.uncovered = [p for p in self._params if id(p) in back or any(p is q for q in self.uncovered)]
        self.mha_refused[name] = why
        self.sweeps = {}

    def output_grads(self, f: torch.Tensor, seeds: torch.Tensor, stack: bool = True):
        """``seeds[s]`` is a cotangent of ``f``; returns, per tap, the gradients w.r.t. the module output
        for every seed: a ``[S, *out.shape]`` tensor, or — for conv taps when ``stack=False`` — the
        list of the ``S`` per-seed tensors exactly as autograd produced them (the Gram kernel reads
        them through a pointer table, so the multi-GB ``[S, B, C, H, W]`` stack is never written).

        Pure-Linear models use ONE vmapped reverse pass (``is_grads_batched``); conv models run one
        reverse pass per seed because functorch has no fused batching rule for MIOpen's conv backward
        (it loops internally and then pays an extra concatenation).
        """
        taps = getattr(self, "_active", self.taps)  # (the taps of the forward this pass belongs to)
        outs = [t.out for t in taps]
        if any(torch.is_tensor(o) for o in outs):
            raise RuntimeError("a tapped module's output does not require grad (frozen parameters upstream and "
                               "downstream?)")
        S = seeds.shape[0]
        has_conv = any(t.kind in ("conv2d", "gconv") for t in taps)
        if S == 1:
            return [lift_maps(t.module, g=g.unsqueeze(0).contiguous())[1]
                    for t, g in zip(taps, torch.autograd.grad(f, outs, grad_outputs=seeds[0]))]
        if not has_conv:
            try:
                grads = torch.autograd.grad(f, outs, grad_outputs=seeds, is_grads_batched=True, retain_graph=True)
                return [g.contiguous() for g in grads]
            except RuntimeError:
                pass  # an op without a batching rule: fall through to one reverse pass per seed
        per_seed = [torch.autograd.grad(f, outs, grad_outputs=seeds[s], retain_graph=(s + 1 < S)) for s in range(S)]
        result = []
        for i, tap in enumerate(taps):
            gs = [ps[i].contiguous() for ps in per_seed]
            if tap.kind == "conv2d" and not stack:  # (dense convolutions only: a grouped one is always stacked)
                result.append(lift_maps(tap.module, g=gs)[1])
            else:
                result.append(lift_maps(tap.module, g=torch.stack(gs))[1])
        return result

    def release(self):
        for t in self.active_taps(frozenset(EXTRA_KINDS)):
            t.a = None
            t.a_split = None
            t.out = None
        for sweep in [*self.sweeps.values(), getattr(self, "feature_sweep", None)]:
            if sweep:
                sweep.release()
