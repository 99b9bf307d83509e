"""Seed-batched reverse sweep: all C-1 likelihood-Hessian seeds in ONE pass with batch ``S*B``.

Stock autograd gives the per-seed output gradients only one seed at a time on ROCm (functorch has
no fused batching rule for MIOpen's convolution backward, so ``is_grads_batched`` loops and then
concatenates).  For a ResNet-18 minibatch that is ~120 small conv launches and ~550 tiny
element-wise kernels per step.  This module is the "fused host-side extraction" of SURVEY.md §8f:

* ``torch.fx`` traces the model once into a graph of modules / functions;
* the forward is executed node by node on the ``B`` samples, keeping only what a vector-Jacobian
  product needs (ReLU masks, pooling indices, BatchNorm-eval scales, ...);
* the reverse sweep pushes a cotangent of batch ``S*B`` (seed-major) through closed-form VJP rules:
  one MIOpen backward-data call per conv for *all* seeds, one element-wise kernel per activation, one row-reduction kernel
  per GroupNorm / LayerNorm (csrc/lk_normvjp.hip: these normalise with per-sample statistics, so their VJP is a reduction per
  statistics row that reuses one ``xhat`` / ``rstd`` per sample for all seeds; csrc/lk_rmsnorm.hip does the same for RMSNorm from
  the layer's input and ``rstd`` alone).

It produces exactly what :class:`laplace_amd.capture.Tape` produces (layer inputs ``a`` and output
gradients ``g`` per tapped module), so everything downstream is unchanged.  Unsupported graphs
(untraceable control flow, modules in training mode, ops without a rule here) raise
:class:`SweepUnsupported` and the caller falls back to the autograd tape.  The model still runs on
stock PyTorch-ROCm kernels — this is host-side plumbing, not a replacement for them.
"""
from __future__ import annotations

import operator
from typing import Any, NamedTuple

import torch
import torch.fx as fx
import torch.nn.functional as F
from torch import nn

from laplace_amd import mha


class SweepUnsupported(RuntimeError):
    pass


# canonical node kinds ("placeholder" / "output" nodes carry their fx op as kind)
CONV, LINEAR, BN, ACT, IDENTITY, RESHAPE, GPOOL, AVGPOOL, MAXPOOL, MEAN, ADD, SIZE, GETITEM, NORM, ATTN, PERMUTE, CONST, CAT = (
    "conv", "linear", "batch-norm", "activation", "identity", "reshape", "adaptive-avg-pool", "avg-pool", "max-pool",
    "mean", "add", "size", "getitem", "per-sample-norm", "attention", "permute", "constant", "concatenation")
# SPLIT: a tuple-valued chunk / split node (no VJP of its own, like SIZE: its items are SLICE nodes that look through it);
# SLICE: one static range along ONE non-batch dim of a traced tensor
SPLIT, SLICE = "split", "slice"
# MUL: the element-wise product of two tensors of the graph (gates, GLU); a product with a Python number is refused
MUL = "product"
# MATMUL: the batched matrix product of two tensors of the graph (``@``, ``torch.matmul``, ``bmm``); SOFTMAX: softmax / log-softmax
# along one static non-batch dim; SCALE: division by a Python number (the ``/ math.sqrt(d)`` of hand-written attention)
MATMUL, SOFTMAX, SCALE = "matrix-product", "softmax", "scale"
# NEG: ``-x`` (the rotate-half of a rotary embedding); SUB: the difference of two tensors of the graph, or of one and a constant
# or a Python number.  A sign has no reduction and nothing to fuse: both are torch math
NEG, SUB = "negation", "difference"
# _EMBED: nn.Embedding applied to the (integer) input: a gather, no input cotangent - the walk ends there; _PARAM: a TRACKED parameter
# that the graph reads through ``get_attr`` (a class token, a learned position table); _EXPAND: ``expand`` / ``expand_as`` of such a
# parameter along the batch dim only.  A _PARAM is live: its cotangent is its Jacobian block (`backend._layer_jacobian`).  (The rules
# EMBED / PARAM of token models; module-private names: these kinds live at the integer input and at leaves of the graph, which the
# NHWC walk never meets - `SplitSweep._split_eligible` sends such a model to the NCHW walk - so they are no part of the public kind list
# that the two walks' tables are held against)
_EMBED, _PARAM, _EXPAND = "embedding", "parameter", "batch-expansion"
# _MAXRED: the maximum along one static non-batch dim or along adjacent ones (``amax``, ``max(dim)[0]``, ``AdaptiveMaxPool1d(1)``:
# what 1-D convolutional networks end in; csrc/lk_reduce.hip); _SUMRED: ``sum`` along static non-batch dims (an ``expand``, as
# MEAN's).  (Module-private names: the NHWC walk sends a model that holds one to the NCHW walk, `SplitSweep._split_eligible`)
_MAXRED, _SUMRED = "max-reduction", "sum-reduction"
# _MHA: an nn.MultiheadAttention called as unmasked self-attention - a tuple-valued node (output, attention weights) that is looked
# through by its items, as SPLIT is; the node itself runs Linear, attention, Linear on the module's own parameters
# (`laplace_amd.mha`) and fills the taps of both halves.  _MHAOUT: ``[0]`` of it, the output (``[1]``, the weights, is served only
# when nothing consumes it).  (Module-private names: the NHWC walk sends a model that holds one to the NCHW walk)
_MHA, _MHAOUT = "multi-head-attention", "attention-output"
# _RESAMPLE: a static, separable, linear resampling of the last one or two dims - nn.Upsample / F.interpolate in every 1-D and 2-D
# mode, F.pad and the padding modules in every mode.  Per plane ``y = Mh x Mw^T + const`` with axis matrices read off torch's own
# operator (`resample_tables`); the VJP of all seeds is one launch of csrc/lk_resample.hip.  (A module-private name: the NHWC walk
# sends a model that holds one to the NCHW walk)
_RESAMPLE = "static-resampling"


class Rule(NamedTuple):
    """What the sweeps know about one traced node, decided once at construction (:func:`classify`)."""

    kind: str
    # input node(s), where the cotangent goes: one, two for ADD (either may be a constant), three for ATTN, the listed tensors in
    # order for CAT (a node may be listed twice; a constant receives nothing); for a SLICE that is a part of a SPLIT the split's source
    src: tuple = ()
    fn: Any = None  # evaluates the node: ``fn(*args, **kwargs)`` on the forward values of ``call``
    call: tuple = ((), {})  # ``(args, kwargs)`` of ``fn`` as fx arguments (nodes and constants)
    what: str = ""  # the operation as messages name it
    flavour: str | None = None  # ACT: "relu" | "tanh" | "sigmoid" | "generic"
    mod: nn.Module | None = None  # CONV / LINEAR / BN / NORM: the module
    # static arguments: AVGPOOL's parameters, GPOOL's output size, MEAN's (dim, keepdim) as written, ATTN's (is_causal, scale),
    # PERMUTE's (spelling, dims), CONST's attribute path (none for an expanded constant, which has ``fn``), CAT's (dim as written,),
    # SPLIT's (spelling, sizes, dim as written), SLICE's ("index", entries, position) / ("narrow", dim, start, length) /
    # ("split", spelling, sizes, dim, item): resolved on the value by `slice_range`; MUL has none (``src``: its two operands, a
    # node may be both; a constant or the input receives nothing)
    args: tuple = ()


# any other element-wise activation: its per-sample derivative is taken ONCE from autograd on the [B, ...]
# forward value (1/S of the sweep's work) and then applied to all seeds by the same fused kernel
_GENERIC_ACT_MODULES = (nn.GELU, nn.SiLU, nn.LeakyReLU, nn.ELU, nn.Softplus, nn.Hardtanh, nn.ReLU6, nn.Mish,
                        nn.Hardswish, nn.Hardsigmoid, nn.SELU, nn.CELU, nn.Softsign, nn.LogSigmoid)
_GENERIC_ACT_FN = (F.gelu, F.silu, F.leaky_relu, F.elu, F.softplus, F.hardtanh, F.relu6, F.mish, F.hardswish,
                   F.hardsigmoid, F.selu, F.celu, F.softsign, F.logsigmoid)

# the three spellings of an operation -> (kind, activation flavour); adding an operation starts here
_MODULE_KINDS = (
    ((nn.Conv2d, nn.Conv1d), CONV, None), ((nn.Linear,), LINEAR, None), ((nn.BatchNorm2d, nn.BatchNorm1d), BN, None),
    # (normalisation with per-sample statistics; the functional spellings read their weights through `get_attr` and stay refused)
    ((nn.GroupNorm, nn.LayerNorm, nn.RMSNorm), NORM, None),
    ((nn.ReLU,), ACT, "relu"), ((nn.Tanh,), ACT, "tanh"), ((nn.Sigmoid,), ACT, "sigmoid"),
    (_GENERIC_ACT_MODULES, ACT, "generic"), ((nn.Identity, nn.Dropout), IDENTITY, None), ((nn.Flatten,), RESHAPE, None),
    ((nn.AdaptiveAvgPool2d,), GPOOL, None), ((nn.AvgPool2d,), AVGPOOL, None), ((nn.MaxPool2d,), MAXPOOL, None),
    # (the 1-D pools are the unit-height window of the 2-D rules, lifted at the node: flavour "1d")
    ((nn.AdaptiveAvgPool1d,), GPOOL, "1d"), ((nn.AvgPool1d,), AVGPOOL, "1d"), ((nn.MaxPool1d,), MAXPOOL, "1d"),
    ((nn.AdaptiveMaxPool1d, nn.AdaptiveMaxPool2d), _MAXRED, None),
    ((nn.Softmax, nn.LogSoftmax), SOFTMAX, None), ((nn.Embedding,), _EMBED, None), ((nn.MultiheadAttention,), _MHA, None),
    # (nn.UpsamplingNearest2d / nn.UpsamplingBilinear2d are nn.Upsample; nn.ZeroPad1d / 2d are nn.ConstantPad1d / 2d)
    ((nn.Upsample,), _RESAMPLE, "interpolate"),
    ((nn.ConstantPad1d, nn.ConstantPad2d, nn.ReflectionPad1d, nn.ReflectionPad2d, nn.ReplicationPad1d, nn.ReplicationPad2d,
      nn.CircularPad1d, nn.CircularPad2d), _RESAMPLE, "pad"))
_FUNCTION_KINDS = {
    torch.relu: (ACT, "relu"), F.relu: (ACT, "relu"), torch.tanh: (ACT, "tanh"), F.tanh: (ACT, "tanh"),
    torch.sigmoid: (ACT, "sigmoid"), F.sigmoid: (ACT, "sigmoid"), **{f: (ACT, "generic") for f in _GENERIC_ACT_FN},
    operator.add: (ADD, None), torch.add: (ADD, None), operator.iadd: (ADD, None), torch.flatten: (RESHAPE, None),
    F.adaptive_avg_pool2d: (GPOOL, None), F.avg_pool2d: (AVGPOOL, None), F.max_pool2d: (MAXPOOL, None),
    F.adaptive_avg_pool1d: (GPOOL, "1d"), F.avg_pool1d: (AVGPOOL, "1d"), F.max_pool1d: (MAXPOOL, "1d"),
    torch.amax: (_MAXRED, None), torch.max: (_MAXRED, None), F.adaptive_max_pool1d: (_MAXRED, None),
    F.adaptive_max_pool2d: (_MAXRED, None), torch.sum: (_SUMRED, None),
    torch.mean: (MEAN, None), operator.getitem: (GETITEM, None), F.scaled_dot_product_attention: (ATTN, None),
    torch.transpose: (PERMUTE, None), torch.permute: (PERMUTE, None),
    torch.cat: (CAT, None), torch.concat: (CAT, None), torch.concatenate: (CAT, None),
    torch.chunk: (SPLIT, None), torch.split: (SPLIT, None), torch.narrow: (SLICE, None),
    operator.mul: (MUL, None), torch.mul: (MUL, None), torch.multiply: (MUL, None), operator.imul: (MUL, None),
    torch.matmul: (MATMUL, None), operator.matmul: (MATMUL, None), torch.bmm: (MATMUL, None),
    F.softmax: (SOFTMAX, None), torch.softmax: (SOFTMAX, None), F.log_softmax: (SOFTMAX, None), torch.log_softmax: (SOFTMAX, None),
    operator.truediv: (SCALE, None), operator.itruediv: (SCALE, None), torch.div: (SCALE, None), torch.true_divide: (SCALE, None),
    operator.neg: (NEG, None), torch.neg: (NEG, None), torch.negative: (NEG, None),
    operator.sub: (SUB, None), operator.isub: (SUB, None), torch.sub: (SUB, None), torch.subtract: (SUB, None),
    F.interpolate: (_RESAMPLE, "interpolate"), F.pad: (_RESAMPLE, "pad")}
_METHOD_KINDS = {
    "relu": (ACT, "relu"), "tanh": (ACT, "tanh"), "sigmoid": (ACT, "sigmoid"), "contiguous": (IDENTITY, None),
    "view": (RESHAPE, None), "reshape": (RESHAPE, None), "flatten": (RESHAPE, None), "mean": (MEAN, None),
    "size": (SIZE, None), "transpose": (PERMUTE, None), "permute": (PERMUTE, None),
    "amax": (_MAXRED, None), "max": (_MAXRED, None), "sum": (_SUMRED, None),
    "chunk": (SPLIT, None), "split": (SPLIT, None), "narrow": (SLICE, None), "expand": (CONST, None), "expand_as": (CONST, None),
    "mul": (MUL, None), "multiply": (MUL, None), "mul_": (MUL, None),
    "matmul": (MATMUL, None), "bmm": (MATMUL, None), "softmax": (SOFTMAX, None), "log_softmax": (SOFTMAX, None),
    "div": (SCALE, None), "true_divide": (SCALE, None), "div_": (SCALE, None), "true_divide_": (SCALE, None),
    "neg": (NEG, None), "negative": (NEG, None), "neg_": (NEG, None),
    "sub": (SUB, None), "subtract": (SUB, None), "sub_": (SUB, None)}
# relatives of the matrix product that have no rule: refused by name
_NO_MATMUL_RULE = {torch.einsum: "einsum", torch.baddbmm: "baddbmm", "baddbmm": "baddbmm"}
# relatives of the slicing rules that have none: refused by name
_NO_SLICE_RULE = {torch.unbind: "unbind", torch.tensor_split: "tensor_split", torch.stack: "stack", "unbind": "unbind",
                  "tensor_split": "tensor_split"}
_ATTN_PARAMS = (("key", "value", "attn_mask", "dropout_p", "is_causal", "scale", "enable_gqa"),
                (None, None, None, 0.0, False, None, False))
_POOL_PARAMS = {  # names and defaults of the functional form; the modules carry attributes of the same names
    MAXPOOL: (("kernel_size", "stride", "padding", "dilation", "ceil_mode", "return_indices"), (None, None, 0, 1, False, False)),
    AVGPOOL: (("kernel_size", "stride", "padding", "ceil_mode", "count_include_pad", "divisor_override"),
              (None, None, 0, False, True, None))}


def _unit_height(name, v):
    """a 1-D pool's parameter as that of the 2-D pool with a unit-height window that it equals on ``[B, C, 1, L]``"""
    if name not in ("kernel_size", "stride", "padding", "dilation") or v is None or (isinstance(v, (tuple, list)) and not v):
        return v
    v = v[0] if isinstance(v, (tuple, list)) else v
    return (0 if name == "padding" else 1, v)


def _bind(node, names, defaults):
    """positional / keyword arguments of a functional call -> dict (input excluded)"""
    vals = dict(zip(names, defaults))
    for n, a in zip(names, node.args[1:]):
        vals[n] = a
    for k, v in node.kwargs.items():
        if k in vals:
            vals[k] = v
    if any(isinstance(v, fx.Node) for v in vals.values()):
        raise SweepUnsupported("data-dependent pooling arguments")
    return vals


def _fetch_attr(root, target):
    """the attribute a ``get_attr`` node names (``a.b.c`` below the traced module)"""
    obj = root
    for part in target.split("."):
        obj = getattr(obj, part)
    return obj


def _classify_attn(node):
    """``(src, (is_causal, scale))`` of an ``F.scaled_dot_product_attention`` call, or the refusal that names the argument"""
    names, defaults = _ATTN_PARAMS
    vals = dict(zip(names, defaults))
    for n, a in zip(names, node.args[1:]):
        vals[n] = a
    for k, v in node.kwargs.items():
        if k == "query":
            continue
        if k not in vals:
            raise SweepUnsupported(f"scaled_dot_product_attention: unknown argument {k}")
        vals[k] = v
    q = node.args[0] if node.args else node.kwargs.get("query")
    if vals["attn_mask"] is not None:
        raise SweepUnsupported("scaled_dot_product_attention with an attn_mask (only is_causal is served)")
    if isinstance(vals["dropout_p"], fx.Node) or vals["dropout_p"] != 0:
        raise SweepUnsupported("scaled_dot_product_attention with dropout_p != 0")
    if isinstance(vals["enable_gqa"], fx.Node) or vals["enable_gqa"]:
        raise SweepUnsupported("scaled_dot_product_attention with enable_gqa (grouped-query attention)")
    for n in ("is_causal", "scale"):
        if isinstance(vals[n], fx.Node):
            raise SweepUnsupported(f"scaled_dot_product_attention with a data-dependent {n}")
    src = (q, vals["key"], vals["value"])
    if not all(isinstance(t, fx.Node) for t in src):
        raise SweepUnsupported("scaled_dot_product_attention: query, key and value must be traced tensors")
    return src, (bool(vals["is_causal"]), None if vals["scale"] is None else float(vals["scale"]))


def _classify_mha(node, m):
    """the source of an nn.MultiheadAttention call that is served as Linear, attention, Linear, or the refusal that names why it
    is not (`laplace_amd.mha.refusal`; the attention weights count as consumed when ``[1]`` of the node has a user)"""
    weights_used = False
    for u in node.users:
        item = u.args[1] if u.op == "call_function" and u.target is operator.getitem and len(u.args) == 2 else None
        if isinstance(item, bool) or item not in (0, 1):
            raise SweepUnsupported(f"{node.target}: the (output, weights) pair of nn.MultiheadAttention must be indexed with [0] or [1]")
        weights_used |= item == 1 and bool(u.users)
    try:
        why = mha.refusal(m, (node.args, node.kwargs), weights_used)
    except TypeError as e:
        why = str(e)
    if why is not None:
        raise SweepUnsupported(f"{node.target}: {why}")
    return (mha.bind_call(node.args, node.kwargs)["query"],)


def _classify_permute(node, what):
    """``(spelling, dims)`` of a transpose / permute with static integer dims (the batch dim must stay: checked on the value)"""
    dims = node.args[1:] if node.args[1:] else tuple(node.kwargs.values())
    if len(dims) == 1 and isinstance(dims[0], (tuple, list)):
        dims = tuple(dims[0])
    if not dims or not all(isinstance(d, int) and not isinstance(d, bool) for d in dims):
        raise SweepUnsupported(f"{what} with data-dependent dims")
    spelling = "transpose" if str(getattr(node.target, "__name__", node.target)) == "transpose" else "permute"
    if spelling == "transpose" and (len(dims) != 2 or 0 in dims):
        raise SweepUnsupported(f"{what}{tuple(dims)} moves the batch dim (dim 0 must stay in place)")
    if spelling == "permute" and dims[0] != 0:
        raise SweepUnsupported(f"{what}{tuple(dims)} moves the batch dim (dim 0 must stay in place)")
    return spelling, tuple(int(d) for d in dims)


def _classify_cat(node, what):
    """``(src, (dim,))`` of a ``torch.cat`` / ``concat`` / ``concatenate`` call: the listed tensors are traced nodes, the dim is
    a static integer as written (it may be negative: resolved on the value, `cat_dim`), or the refusal that names the reason"""
    kwargs = dict(node.kwargs)
    if kwargs.pop("out", None) is not None:
        raise SweepUnsupported(f"{what} with an out= argument (the sweep keeps its own values)")
    tensors = node.args[0] if node.args else kwargs.pop("tensors", None)
    dim = node.args[1] if len(node.args) > 1 else kwargs.pop("dim", kwargs.pop("axis", 0))
    if kwargs or len(node.args) > 2:
        raise SweepUnsupported(f"{what}: unknown argument {sorted(kwargs) or node.args[2:]}")
    if isinstance(dim, fx.Node) or isinstance(dim, bool) or not isinstance(dim, int):
        raise SweepUnsupported(f"{what} with a data-dependent dim")
    if not isinstance(tensors, (tuple, list)) or not tensors:
        raise SweepUnsupported(f"{what}: the tensors must be a non-empty list or tuple of traced tensors")
    for t in tensors:
        if not isinstance(t, fx.Node):
            raise SweepUnsupported(f"{what}: an entry of the list is not a traced tensor ({type(t).__name__}: a Python constant or "
                                   "a tensor literal has no node to push a cotangent to)")
    if dim == 0:
        raise SweepUnsupported(f"{what} along dim 0 (the batch dim: the seeds are stacked there)")
    return tuple(tensors), (dim,)


def cat_dim(dim, ndim, what="cat"):
    """the dim of a CAT rule resolved on a value of ``ndim`` dims (never the batch dim)"""
    if not -ndim <= dim < ndim:
        raise SweepUnsupported(f"{what} along dim {dim} of a value with {ndim} dims")
    if dim % ndim == 0:
        raise SweepUnsupported(f"{what} along dim {dim} of a value with {ndim} dims (the batch dim: the seeds are stacked there)")
    return dim % ndim


_BATCH_SLICE = "dim 0 (the batch dim: the seeds are stacked there)"


def _static_int(v, what, name):
    """a static Python integer argument, or the refusal that names it"""
    if isinstance(v, fx.Node) or torch.is_tensor(v):
        raise SweepUnsupported(f"{what} with a data-dependent {name}")
    if isinstance(v, bool) or not isinstance(v, int):
        raise SweepUnsupported(f"{what}: {name} must be a static integer, got {type(v).__name__}")
    return int(v)


def _classify_split(node, what):
    """``(spelling, sizes, dim)`` of a ``chunk`` / ``split`` call (function or method) with static arguments: ``sizes`` is the
    number of chunks, the size of a part or the tuple of sections; the dim as written (negative allowed: resolved on the value)"""
    spelling = "chunk" if str(getattr(node.target, "__name__", node.target)) == "chunk" else "split"
    kwargs = dict(node.kwargs)
    names = ("chunks",) if spelling == "chunk" else ("split_size_or_sections", "split_size")
    sizes = node.args[1] if len(node.args) > 1 else next((kwargs.pop(n) for n in names if n in kwargs), None)
    dim = node.args[2] if len(node.args) > 2 else kwargs.pop("dim", 0)
    kwargs.pop("input", None), kwargs.pop("tensor", None)
    if kwargs or len(node.args) > 3 or sizes is None:
        raise SweepUnsupported(f"{what}: unknown or missing argument {sorted(kwargs) or node.args[3:]}")
    dim = _static_int(dim, what, "dim")
    if isinstance(sizes, (tuple, list)):
        if spelling == "chunk" or not sizes:
            raise SweepUnsupported(f"{what}: the sections must be a non-empty list of static integers")
        sizes = tuple(_static_int(s, what, "section") for s in sizes)
        if min(sizes) < 0:
            raise SweepUnsupported(f"{what}: negative section in {sizes}")
    else:
        sizes = _static_int(sizes, what, "number of chunks" if spelling == "chunk" else "split size")
        if sizes < 1:
            raise SweepUnsupported(f"{what}: {sizes} is no {'number of chunks' if spelling == 'chunk' else 'split size'}")
    if dim == 0:
        raise SweepUnsupported(f"{what} along {_BATCH_SLICE}")
    return spelling, sizes, dim


def _classify_index(idx, what):
    """the static index of a ``tensor[idx]`` as a tuple of ``:`` / ``...`` / ints / unit-step slices with exactly one entry that
    is not a full slice (``None`` when every entry is full: the node is an identity), or the refusal that names the reason"""
    entries = tuple(idx) if isinstance(idx, tuple) else (idx,)
    hit = []
    for i, e in enumerate(entries):
        if isinstance(e, fx.Node):
            raise SweepUnsupported(f"{what} with a data-dependent index")
        if e is None or isinstance(e, (bool, list)) or torch.is_tensor(e):
            kind = "None" if e is None else "tensor" if torch.is_tensor(e) else "list" if isinstance(e, list) else "bool"
            raise SweepUnsupported(f"{what} with a {kind} index (only ints, unit-step slices, ':' and '...' are served)")
        if e is Ellipsis:
            if sum(x is Ellipsis for x in entries) > 1:
                raise SweepUnsupported(f"{what} with more than one '...'")
        elif isinstance(e, slice):
            if any(isinstance(v, fx.Node) or torch.is_tensor(v) for v in (e.start, e.stop, e.step)):
                raise SweepUnsupported(f"{what} with data-dependent bounds")
            for v in (e.start, e.stop, e.step):
                if v is not None and (isinstance(v, bool) or not isinstance(v, int)):
                    raise SweepUnsupported(f"{what}: slice bounds must be static integers, got {type(v).__name__}")
            if e.step not in (None, 1):
                raise SweepUnsupported(f"{what} with a step other than 1 (step {e.step})")
            if not (e.start in (None, 0) and e.stop is None):
                hit.append(i)
        elif isinstance(e, int):
            hit.append(i)
        else:
            raise SweepUnsupported(f"{what} with a {type(e).__name__} index (only ints, unit-step slices, ':' and '...' are served)")
    if len(hit) > 1:
        raise SweepUnsupported(f"{what} slices more than one dim (index one dim at a time)")
    if hit and hit[0] == 0:
        raise SweepUnsupported(f"{what} slices {_BATCH_SLICE}")
    return (entries, hit[0]) if hit else None


def slice_range(spec, shape, what="slice"):
    """``(dim, start, length, dropped)`` of a SLICE rule resolved on a value of ``shape``: the sliced dim (never the batch dim),
    the range along it and whether an int index drops the dim"""
    ndim, dropped = len(shape), False
    if spec[0] == "index":
        entries, i = spec[1], spec[2]
        n = sum(e is not Ellipsis for e in entries)
        if n > ndim:
            raise SweepUnsupported(f"{what}: {n} indices for a value with {ndim} dims")
        dim = i if not any(e is Ellipsis for e in entries[:i]) else ndim - (len(entries) - i)
        if dim <= 0:
            raise SweepUnsupported(f"{what} slices {_BATCH_SLICE}")
        e, D = entries[i], int(shape[dim])
        if isinstance(e, slice):
            start, stop, _ = e.indices(D)
            length = stop - start
        else:
            if not -D <= e < D:
                raise SweepUnsupported(f"{what}: index {e} is out of range for dim {dim} of size {D}")
            start, length, dropped = e % D, 1, True
    elif spec[0] == "narrow":
        dim, start, length = cat_dim(spec[1], ndim, what), spec[2], spec[3]
        D = int(shape[dim])
        start = start + D if start < 0 else start
        if not (0 <= start and 0 <= length and start + length <= D):
            raise SweepUnsupported(f"{what}: range [{spec[2]}, {spec[2]} + {length}) leaves dim {dim} of size {D}")
    else:  # item ``spec[4]`` of a chunk / split
        _, spelling, sizes, dim, item = spec
        dim = cat_dim(dim, ndim, what)
        D = int(shape[dim])
        if isinstance(sizes, tuple):
            if sum(sizes) != D:
                raise SweepUnsupported(f"{what}: sections {sizes} do not sum to dim {dim} of size {D}")
            bounds = [0]
            for s in sizes:
                bounds.append(bounds[-1] + s)
        else:
            size = -(-D // sizes) if spelling == "chunk" else sizes  # (chunk: ceil(D / chunks) per part, fewer parts if need be)
            bounds = list(range(0, D, max(size, 1))) + [D]
        n = len(bounds) - 1
        if not -n <= item < n:
            raise SweepUnsupported(f"{what}: part {item} of {n}")
        start, length = bounds[item % n], bounds[item % n + 1] - bounds[item % n]
    if length < 1:
        raise SweepUnsupported(f"{what}: an empty range along dim {dim}")
    return dim, int(start), int(length), dropped


def _classify_slice(node, modules, what):
    """the Rule of a SLICE node - ``getitem`` of a chunk / split (looked through: the source is the split's source), ``getitem``
    of a traced tensor with a static index, ``narrow`` - or ``None`` for a ``getitem`` of a non-tensor (a ``size()`` tuple)"""
    src = node.args[0] if node.args else node.kwargs.get("input")
    if node.target is operator.getitem:
        up = classify(src, modules) if isinstance(src, fx.Node) else None
        if up is None or up.kind in (SIZE, GETITEM):
            return None
        what = f"indexing of {src.name}"
        if up.kind == SPLIT:
            item = node.args[1]
            if isinstance(item, fx.Node) or isinstance(item, bool) or not isinstance(item, int):
                raise SweepUnsupported(f"{up.what}: its parts must be taken one by one with a static integer index")
            return Rule(SLICE, up.src, None, (up.src, {}), f"part {item} of {up.what}", args=("split", *up.args, item))
        hit = _classify_index(node.args[1], what)
        if hit is None:  # (x[:], x[...]: a view of everything)
            return Rule(IDENTITY, (src,), operator.getitem, (tuple(node.args), {}), what)
        return Rule(SLICE, (src,), None, ((src,), {}), what, args=("index", *hit))
    kwargs = dict(node.kwargs)
    kwargs.pop("input", None)
    vals = [*node.args[1:], *(kwargs.pop(n) for n in ("dim", "start", "length")[len(node.args) - 1:] if n in kwargs)]
    if kwargs or len(vals) != 3 or not isinstance(src, fx.Node):
        raise SweepUnsupported(f"{what}: expected (input, dim, start, length)")
    dim, start, length = (_static_int(v, what, n) for v, n in zip(vals, ("dim", "start", "length")))
    if dim == 0:
        raise SweepUnsupported(f"{what} along {_BATCH_SLICE}")
    return Rule(SLICE, (src,), None, ((src,), {}), what, args=("narrow", dim, start, length))


def _classify_mul(node, modules):
    """the two operands of a product (``*``, ``torch.mul`` / ``multiply``, the methods, ``*=`` / ``mul_``): each a traced tensor
    or a constant of the sweep, at least one traced, or the refusal that names the reason (every message holds ``mul``)"""
    if node.kwargs.get("out") is not None:
        raise SweepUnsupported("mul with an out= argument (the sweep keeps its own values)")
    if node.kwargs or len(node.args) != 2:
        raise SweepUnsupported(f"mul: expected two positional operands, got {len(node.args)} and the keywords {sorted(node.kwargs)}")
    for t in node.args:
        if isinstance(t, (bool, int, float, complex)):
            raise SweepUnsupported(f"mul by the Python number {t!r} is not served (fold the factor into the layer: scale its weights "
                                   "and bias)")
        if not isinstance(t, fx.Node):
            raise SweepUnsupported(f"mul: an operand is not a tensor of the graph ({type(t).__name__})")
    if all(classify(t, modules).kind == CONST for t in node.args):
        raise SweepUnsupported("mul of two constants (at least one operand must be a traced tensor)")
    return tuple(node.args)


def mul_form(sa, sb):
    """how the shapes of two traced operands of a product go together: ``("full", None, 0)`` for equal shapes, ``("row", gate, k)``
    when operand ``gate`` (0 / 1) is ``other.shape[:k] + (1,) * (ndim - k)`` with ``1 <= k < ndim`` (``[B, C, 1, 1]`` against
    ``[B, C, H, W]``); anything else is refused with both shapes"""
    sa, sb = tuple(int(d) for d in sa), tuple(int(d) for d in sb)
    if sa == sb:
        return "full", None, 0
    if len(sa) == len(sb):
        for gate, (sg, so) in enumerate(((sa, sb), (sb, sa))):
            k = next((i for i, d in enumerate(sg) if d == 1 and so[i] != 1), len(sg))
            if 1 <= k < len(sg) and sg[:k] == so[:k] and all(d == 1 for d in sg[k:]):
                return "row", gate, k
        try:
            torch.broadcast_shapes(sa, sb)
        except RuntimeError:
            pass
        else:
            raise SweepUnsupported(f"mul of {sa} and {sb}: a traced operand broadcast along a dim before the last kept one needs a "
                                   "strided reduction (only a gate of trailing ones, [B, C, 1, 1] or [B, T, 1], is served)")
    raise SweepUnsupported(f"mul of {sa} and {sb}: the traced operands must have equal shapes, or one must be a gate of trailing ones")


def _classify_matmul(node, modules):
    """the two operands of a matrix product (``@``, ``torch.matmul`` / ``bmm``, the methods): each a traced tensor or a constant of
    the sweep, at least one traced, or the refusal that names the reason (every message holds ``matmul``); the shapes are resolved
    on the forward values (`SeedBatchedSweep._run_matmul`)"""
    if node.kwargs.get("out") is not None:
        raise SweepUnsupported("matmul with an out= argument (the sweep keeps its own values)")
    if node.kwargs or len(node.args) != 2:
        raise SweepUnsupported(f"matmul: expected two positional operands, got {len(node.args)} and the keywords {sorted(node.kwargs)}")
    for t in node.args:
        if not isinstance(t, fx.Node):
            raise SweepUnsupported(f"matmul: an operand is not a tensor of the graph ({type(t).__name__})")
    if all(classify(t, modules).kind == CONST for t in node.args):
        raise SweepUnsupported("matmul of two constants (at least one operand must be a traced tensor)")
    return tuple(node.args)


def _classify_softmax(node, m, what):
    """``(src, (dim as written, is_log))`` of a softmax / log-softmax (functions, methods, ``nn.Softmax`` / ``nn.LogSoftmax``) with
    one static dim, or the refusal that names the reason (every message holds ``softmax``)"""
    name = type(m).__name__ if m is not None else str(getattr(node.target, "__name__", node.target))
    is_log = "log" in name.lower()
    name = "log_softmax" if is_log else "softmax"
    if m is not None:
        dim, dtype = m.dim, None
    else:
        kwargs = dict(node.kwargs)
        kwargs.pop("input", None), kwargs.pop("_stacklevel", None)
        rest = list(node.args[1:])
        dim = rest.pop(0) if rest else kwargs.pop("dim", None)
        if node.target in (F.softmax, F.log_softmax) and rest:  # (the functional form: input, dim, _stacklevel, dtype)
            rest.pop(0)
        dtype = rest.pop(0) if rest else kwargs.pop("dtype", None)
        if rest or kwargs:
            raise SweepUnsupported(f"{name}: unknown argument {sorted(kwargs) or rest}")
    if dtype is not None:
        raise SweepUnsupported(f"{name} with dtype= (the sweep keeps the dtype of the traced value)")
    if isinstance(dim, fx.Node) or torch.is_tensor(dim):
        raise SweepUnsupported(f"{name} with a data-dependent dim")
    if dim is None:
        raise SweepUnsupported(f"{name} without a dim (the implicit-dim legacy picks one from the number of dims: name it)")
    if isinstance(dim, bool) or not isinstance(dim, int):
        raise SweepUnsupported(f"{name}: dim must be a static integer, got {type(dim).__name__}")
    if dim == 0:
        raise SweepUnsupported(f"{name} along {_BATCH_SLICE}")
    if not (node.args and isinstance(node.args[0], fx.Node)):
        raise SweepUnsupported(f"{name}: the tensor must be the first positional argument and a traced tensor")
    return (node.args[0],), (int(dim), is_log), name


def _classify_scale(node, modules):
    """``(src, (divisor,))`` of a division by a Python number (``/``, ``torch.div`` / ``true_divide``, the methods, ``/=`` /
    ``div_``), or the refusal that names the reason (every message holds ``div``)"""
    kwargs = dict(node.kwargs)
    if kwargs.pop("rounding_mode", None) is not None:
        raise SweepUnsupported("div with a rounding_mode (floor and trunc have no derivative to sweep)")
    if kwargs.pop("out", None) is not None:
        raise SweepUnsupported("div with an out= argument (the sweep keeps its own values)")
    if kwargs or len(node.args) != 2:
        raise SweepUnsupported(f"div: expected two positional operands, got {len(node.args)} and the keywords {sorted(kwargs)}")
    x, c = node.args
    if not isinstance(x, fx.Node):
        raise SweepUnsupported(f"div of the number {x!r} by a tensor (number / tensor needs the quotient rule: out of scope)")
    if isinstance(c, fx.Node):
        if classify(c, modules).kind in (SIZE, GETITEM):
            raise SweepUnsupported(f"div by the traced value {c.name} (the divisor must be a Python number when the graph is traced)")
        raise SweepUnsupported(f"div of the tensor {x.name} by the tensor {c.name} (tensor / tensor needs the quotient rule: out of scope)")
    if isinstance(c, (bool, complex)) or not isinstance(c, (int, float)):
        raise SweepUnsupported(f"div by a {type(c).__name__} (the divisor must be a Python int or float)")
    return (x,), (c,)


def _classify_neg(node):
    """the operand of a negation (``-x``, ``torch.neg`` / ``negative``, the methods, ``neg_``), or the refusal that names the
    reason (every message holds ``neg``)"""
    if node.kwargs.get("out") is not None:
        raise SweepUnsupported("neg with an out= argument (the sweep keeps its own values)")
    x = node.args[0] if node.args else node.kwargs.get("input")
    if len(node.args) > 1 or set(node.kwargs) - {"input", "out"} or not isinstance(x, fx.Node):
        raise SweepUnsupported("neg: expected one operand, a tensor of the graph")
    return (x,)


def _classify_sub(node, modules):
    """the two operands of a difference (``-``, ``torch.sub`` / ``subtract``, the methods, ``-=`` / ``sub_``): each a traced tensor,
    a constant of the sweep or a Python number, at least one a tensor that is not a constant, or the refusal that names the reason
    (every message holds ``sub``); the shapes are resolved on the forward values (`SeedBatchedSweep._run_sub`)"""
    kwargs = dict(node.kwargs)
    alpha = kwargs.pop("alpha", 1)
    if isinstance(alpha, fx.Node) or alpha != 1:
        raise SweepUnsupported("sub with alpha != 1 (fold the factor into the layer that produces the subtrahend)")
    if kwargs.pop("out", None) is not None:
        raise SweepUnsupported("sub with an out= argument (the sweep keeps its own values)")
    if kwargs or len(node.args) != 2:
        raise SweepUnsupported(f"sub: expected two positional operands, got {len(node.args)} and the keywords {sorted(kwargs)}")
    nodes = [t for t in node.args if isinstance(t, fx.Node)]
    for t in node.args:
        if not isinstance(t, fx.Node) and (isinstance(t, (bool, complex)) or not isinstance(t, (int, float))):
            raise SweepUnsupported(f"sub: an operand is neither a tensor of the graph nor a Python int or float ({type(t).__name__})")
    if not nodes:
        raise SweepUnsupported("sub of two Python numbers")
    if all(classify(t, modules).kind == CONST for t in nodes):
        raise SweepUnsupported("sub of two constants (at least one operand must be a traced tensor)" if len(nodes) == 2 else
                               "sub of a constant and a Python number (at least one operand must be a traced tensor)")
    return tuple(node.args)


_RESAMPLE_PARAMS = {  # names and defaults of the functional forms (the input excluded)
    "interpolate": (("size", "scale_factor", "mode", "align_corners", "recompute_scale_factor", "antialias"),
                    (None, None, "nearest", None, None, False)),
    "pad": (("pad", "mode", "value"), (None, "constant", None))}
_PAD_MODULE_MODES = ((nn.ConstantPad1d, "constant"), (nn.ConstantPad2d, "constant"), (nn.ReflectionPad1d, "reflect"),
                     (nn.ReflectionPad2d, "reflect"), (nn.ReplicationPad1d, "replicate"), (nn.ReplicationPad2d, "replicate"),
                     (nn.CircularPad1d, "circular"), (nn.CircularPad2d, "circular"))


def _holds_node(v):
    return isinstance(v, fx.Node) or (isinstance(v, (tuple, list)) and any(_holds_node(e) for e in v))


def _classify_resample(node, m, op, modules):
    """``(x, keyword arguments of the functional form, what)`` of an ``F.interpolate`` / ``F.pad`` call or of a module that makes
    one (nn.Upsample and its two subclasses, the eight padding modules): every argument bound by name, the mode and the pad static,
    ``size`` / ``scale_factor`` static or made of values the sweep evaluates to ints (``y.size(2)``, items of ``y.size()``), or the
    refusal that names the operation and the reason"""
    names, defaults = _RESAMPLE_PARAMS[op]
    vals = dict(zip(names, defaults))
    if m is not None:
        what = f"{type(m).__name__} ({node.target})"
        if op == "interpolate":
            vals.update(size=m.size, scale_factor=m.scale_factor, mode=m.mode, align_corners=m.align_corners,
                        recompute_scale_factor=m.recompute_scale_factor)
        else:
            vals.update(pad=tuple(m.padding), mode=next(md for t, md in _PAD_MODULE_MODES if isinstance(m, t)),
                        value=getattr(m, "value", None))
        extra = list(node.args[1:]) + sorted(node.kwargs)
        if extra and set(node.kwargs) != {"input"}:
            raise SweepUnsupported(f"{what}: unknown argument {extra}")
    else:
        what = op
        kwargs = dict(node.kwargs)
        if kwargs.pop("out", None) is not None:
            raise SweepUnsupported(f"{what} with an out= argument (the sweep keeps its own values)")
        for n, a in zip(names, node.args[1:]):
            vals[n] = a
        for k in list(kwargs):
            if k in vals:
                vals[k] = kwargs.pop(k)
        kwargs.pop("input", None)
        if kwargs or len(node.args) > 1 + len(names):
            raise SweepUnsupported(f"{what}: unknown argument {sorted(kwargs) or node.args[1 + len(names):]}")
    x = node.args[0] if node.args else node.kwargs.get("input")
    if not isinstance(x, fx.Node):
        raise SweepUnsupported(f"{what}: the operand must be a traced tensor")
    for n in ("mode", "align_corners", "recompute_scale_factor", "antialias", "pad"):
        if n in vals and _holds_node(vals[n]):
            raise SweepUnsupported(f"{what} with a data-dependent {n}")
    if not isinstance(vals["mode"], str):
        raise SweepUnsupported(f"{what}: mode must be a string, got {type(vals['mode']).__name__}")
    if op == "interpolate":
        if vals["mode"] == "trilinear":
            raise SweepUnsupported(f"{what} in mode trilinear (3-D resampling is out of scope: the last two dims are what the rule serves)")
        for n in ("size", "scale_factor"):
            for e in (vals[n] if isinstance(vals[n], (tuple, list)) else (vals[n],)):
                if isinstance(e, fx.Node) and classify(e, modules).kind not in (SIZE, GETITEM):
                    raise SweepUnsupported(f"{what} with a data-dependent {n} ({e.name}: only values of a size() are resolved)")
                if torch.is_tensor(e):
                    raise SweepUnsupported(f"{what} with a tensor {n}")
        if isinstance(vals["scale_factor"], fx.Node) or _holds_node(vals["scale_factor"]):
            raise SweepUnsupported(f"{what} with a data-dependent scale_factor")
    else:
        if isinstance(vals["value"], fx.Node) or torch.is_tensor(vals["value"]):
            raise SweepUnsupported(f"{what} with a traced value (the constant of a pad must be a Python number)")
        pad = vals["pad"]
        if not isinstance(pad, (tuple, list)) or len(pad) % 2 or not pad or \
                not all(isinstance(v, int) and not isinstance(v, bool) for v in pad):
            raise SweepUnsupported(f"{what}: pad must be a non-empty tuple of static integers of even length, got {pad!r}")
        vals["pad"] = tuple(int(v) for v in pad)
    return x, vals, what


def resample_dims(op, vals, shape, what):
    """how many of the LAST dims (1 or 2) a _RESAMPLE rule resamples on a value of ``shape``, never dim 0 (the seeds are stacked
    there), or the refusal that names the reason"""
    ndim = len(shape)
    if op == "interpolate":
        if ndim == 5:
            raise SweepUnsupported(f"{what} of a 5-D value (3-D resampling is out of scope)")
        if ndim not in (3, 4):
            raise SweepUnsupported(f"{what} of a value with {ndim} dims (expected [B, C, L] or [B, C, H, W])")
        return ndim - 2
    pad = list(vals["pad"])
    while len(pad) > 2 and pad[-2:] == [0, 0]:
        del pad[-2:]
    k = len(pad) // 2
    if k >= ndim:
        raise SweepUnsupported(f"{what}{tuple(vals['pad'])} of a value with {ndim} dims pads {_BATCH_SLICE}")
    if k > 2:
        raise SweepUnsupported(f"{what}{tuple(vals['pad'])} pads more than the last two dims")
    if ndim < 3:
        raise SweepUnsupported(f"{what} of a value with {ndim} dims (the operand must have at least 3: [B, C, L], [B, T, D], [B, C, H, W])")
    return k


class ResampleTables(NamedTuple):
    """the two axis matrices of a static separable resampling and their transposes in CSR form (`resample_tables`)"""

    Mh: torch.Tensor  # [OH, H], the dtype of the value
    Mw: torch.Tensor  # [OW, W]
    csr_h: tuple  # (ptr [H + 1] int32, idx int32 ascending per entry, w float32): per input row the outputs that read it
    csr_w: tuple
    taps: tuple  # (longest list of csr_h, of csr_w)


def _axis_matrix(axis_op, L, width, like):
    """``M`` ``[OL, L]`` of one axis, read off torch's own operator: ``axis_op(basis) - axis_op(zeros)`` on the ``L`` unit vectors
    (the difference removes the constant of a pad), the other axis at extent ``width`` and constant along it"""
    eye = torch.eye(L, dtype=like.dtype, device=like.device)
    return (axis_op(eye, width) - axis_op(torch.zeros_like(eye), width)).t().contiguous()


def _csr_transposed(M):
    """the transpose of the dense ``M`` ``[OL, L]`` in CSR form: per input ``l`` the outputs ``o`` with ``M[o, l] != 0``, ascending"""
    Mt = M.t()
    nz = Mt.nonzero()  # (row-major: by l, then o ascending)
    cnt = torch.bincount(nz[:, 0], minlength=M.shape[1])
    ptr = torch.zeros(M.shape[1] + 1, dtype=torch.int64, device=M.device)
    ptr[1:] = torch.cumsum(cnt, 0)
    return (ptr.to(torch.int32), nz[:, 1].to(torch.int32).contiguous(), Mt[nz[:, 0], nz[:, 1]].float().contiguous()), \
        int(cnt.max()) if cnt.numel() else 0


def resample_tables(op, vals, in_hw, out_hw, k, like):
    """:class:`ResampleTables` of the operation ``op`` ("interpolate" / "pad") with the resolved keyword arguments ``vals`` on a
    plane of extent ``in_hw`` = ``(H, W)`` that it maps to ``out_hw``; ``k``: the number of resampled dims (1: ``H = OH = 1`` and
    the height's matrix is the identity).  Nothing is assumed about torch's index arithmetic: each axis matrix is the operator
    itself on a basis (`_axis_matrix`), in the dtype and on the device of ``like``."""
    (H, W), (OH, OW) = in_hw, out_hw

    def run(t, axis, width):
        """the operator on ``t`` ``[n, L]`` read as ``n`` planes whose axis ``axis`` (0: rows, 1: columns) has extent ``L`` and whose
        other axis has extent ``width`` (constant along it) -> ``[n, OL]`` (the first position of the other axis)"""
        n, L = t.shape
        if k == 1:
            x = t.reshape(n, 1, L)
        elif axis == 0:
            x = t.reshape(n, 1, L, 1).expand(n, 1, L, width)
        else:
            x = t.reshape(n, 1, 1, L).expand(n, 1, width, L)
        x = x.contiguous()
        if op == "pad":
            pad = list(vals["pad"][:2 * k]) + [0] * (2 * k - len(vals["pad"][:2 * k]))
            if k == 2:  # (the other axis is not padded)
                pad = [0, 0, pad[2], pad[3]] if axis == 0 else [pad[0], pad[1], 0, 0]
            y = F.pad(x, tuple(pad), mode=vals["mode"], value=vals["value"])
        else:
            kw = {n_: vals[n_] for n_ in ("mode", "align_corners", "recompute_scale_factor", "antialias")}
            if vals["size"] is not None:  # (as resolved by the forward: the output's extent)
                kw["size"] = (OW,) if k == 1 else ((OH, width) if axis == 0 else (width, OW))
            else:
                sf = vals["scale_factor"]
                sf = tuple(float(v) for v in sf) if isinstance(sf, (tuple, list)) else (float(sf),) * k
                kw["scale_factor"] = sf if k == 1 else ((sf[0], 1.0) if axis == 0 else (1.0, sf[1]))
            y = F.interpolate(x, **kw)
        if k == 1:
            return y.reshape(n, -1)
        return y[:, 0, :, 0] if axis == 0 else y[:, 0, 0, :]

    def whole(x):
        """the operator itself on ``x`` ``[n, 1, H, W]`` (``k = 1``: ``[n, 1, W]``), its constant removed"""
        fn = F.pad if op == "pad" else F.interpolate
        kw = vals if op == "pad" else {**vals, "size": None if vals["size"] is None else ((OW,) if k == 1 else (OH, OW))}
        return fn(x, **kw) - fn(torch.zeros_like(x), **kw)

    with torch.no_grad():
        # the other axis at unit extent with its argument neutral (size 1, scale 1.0, pad 0); the pair is then held against the
        # operator itself on one random plane.  Where it misses - the operator does not map a unit axis by exactly 1 (a bicubic
        # ``1 -> 1`` may sum its four clamped coefficients to ``1 +- ulp``; the antialias filters mishandle a unit extent) - the
        # other axis is tried at extent 2 and at full width, constant along it.  A mode that no derivation fits is not separable.
        one = torch.ones(1, 1, dtype=like.dtype, device=like.device)
        probe = torch.rand((1, 1, W) if k == 1 else (1, 1, H, W), generator=torch.Generator().manual_seed(H * 7919 + W),
                           dtype=torch.float64).to(like)
        want, err = whole(probe).reshape(OH, OW), None
        for width_h, width_w in dict.fromkeys(((1, 1), (min(2, W), min(2, H)), (W, H))):
            if k == 1:
                Mh = one.clone()
            else:
                Mh = _axis_matrix(lambda t, width: run(t, 0, width), H, width_h, like)
            Mw = _axis_matrix(lambda t, width: run(t, 1, width), W, width_w, like)
            if tuple(Mh.shape) != (OH, H) or tuple(Mw.shape) != (OW, W):
                continue
            if k == 2 and op == "interpolate":  # (what a unit / constant other axis is mapped by: exactly 1, or the next derivation)
                kw = {n_: vals[n_] for n_ in ("mode", "align_corners", "recompute_scale_factor", "antialias")}
                kw.update({"size": (width_w, width_h)} if vals["size"] is not None else {"scale_factor": (1.0, 1.0)})
                if not bool((F.interpolate(one.reshape(1, 1, 1, 1).expand(1, 1, width_w, width_h).contiguous(), **kw) == 1).all()):
                    continue
            got = Mh @ probe.reshape(H, W) @ Mw.t()
            err = (got - want).abs().max()
            scale = (Mh.abs() @ probe.reshape(H, W).abs() @ Mw.abs().t()).max()
            if bool(err <= 64 * torch.finfo(like.dtype).eps * scale + torch.finfo(like.dtype).tiny):
                break
        else:
            raise SweepUnsupported(f"{op} in mode {vals.get('mode')!r} is not a separable linear map of the last {k} dims of a "
                                   f"{(H, W)} plane" + ("" if err is None else f" (|y - Mh x Mw^T| = {float(err):.2e})"))
        (csr_h, th), (csr_w, tw) = _csr_transposed(Mh), _csr_transposed(Mw)
    return ResampleTables(Mh, Mw, csr_h, csr_w, (th, tw))


def resample_vjp_math(g, Mh, Mw, S=None):
    """``dx = Mh^T g Mw`` ``[..., H, W]`` for the seeds stacked in ``g`` ``[..., OH, OW]`` - the sum of lk_resample_vjp_f32 as two
    dense matrix products (any dtype; deterministic: no atomics, unlike stock ``upsample_*_backward`` / ``*_pad*_backward``)"""
    OH, OW = g.shape[-2:]
    t = (g.reshape(-1, OW) @ Mw.to(g.dtype)).reshape(*g.shape[:-1], Mw.shape[1])  # (one GEMM over all rows of all planes)
    if tuple(Mh.shape) == (1, 1) and bool(Mh[0, 0] == 1):  # (a 1-D operation: the height's matrix is the identity)
        return t
    return torch.matmul(Mh.t().to(g.dtype), t)


def _same(t):
    """the forward of a node that hands its source on (the ``[0]`` / ``.values`` of a ``max(dim)``, whose node holds the values)"""
    return t


_ADAPTIVE_MAX = {nn.AdaptiveMaxPool1d: 1, nn.AdaptiveMaxPool2d: 2, F.adaptive_max_pool1d: 1, F.adaptive_max_pool2d: 2}
# relatives of the reduction rules that have none: refused by name
_NO_REDUCE_RULE = {torch.min: "min", torch.amin: "amin", torch.logsumexp: "logsumexp", torch.topk: "topk", "min": "min", "amin": "amin",
                   "logsumexp": "logsumexp", "topk": "topk", F.adaptive_max_pool1d_with_indices: "adaptive_max_pool1d(return_indices=True)",
                   F.adaptive_max_pool2d_with_indices: "adaptive_max_pool2d(return_indices=True)",
                   F.max_pool1d_with_indices: "max_pool1d(return_indices=True)"}


def _classify_reduce(node, m, kind):
    """``(src, (name, dims as written, keepdim, tie, is_tuple))`` of a maximum or a sum over static non-batch dims - ``amax``,
    ``max(dim)``, ``sum(dim)`` (functions and methods), the adaptive max pools to ONE cell - or the refusal that names the
    operation.  ``tie``: ``"first"`` (``max(dim)`` and the pools send the cotangent to the first maximum, as autograd does),
    ``"even"`` (``amax`` splits it evenly over the maxima), ``None`` for a sum; ``is_tuple``: the node is the (values, indices)
    pair of a ``max(dim)``, whose ``[0]`` / ``.values`` hands the values on.  The dims are resolved on the value (`reduce_geometry`)."""
    key = type(m) if m is not None else node.target
    if key in _ADAPTIVE_MAX:
        nd = _ADAPTIVE_MAX[key]
        name = f"adaptive_max_pool{nd}d"
        if m is not None:
            size, ret = m.output_size, m.return_indices
        else:
            kwargs = dict(node.kwargs)
            kwargs.pop("input", None)
            size = node.args[1] if len(node.args) > 1 else kwargs.pop("output_size", None)
            ret = node.args[2] if len(node.args) > 2 else kwargs.pop("return_indices", False)
            if kwargs or len(node.args) > 3:
                raise SweepUnsupported(f"{name}: unknown argument {sorted(kwargs) or node.args[3:]}")
        if isinstance(ret, fx.Node) or ret:
            raise SweepUnsupported(f"{name}(return_indices=True): the indices of a maximum have no cotangent and no rule")
        cells = tuple(size) if isinstance(size, (tuple, list)) else (size,) * nd
        if any(isinstance(c, fx.Node) for c in cells):
            raise SweepUnsupported(f"{name} with a data-dependent output size")
        if len(cells) != nd or any(c != 1 for c in cells):
            raise SweepUnsupported(f"{name} to {size} cells (only the maximum over all positions, output size 1, is served)")
        x = node.args[0] if node.args else node.kwargs.get("input")
        if not isinstance(x, fx.Node):
            raise SweepUnsupported(f"{name}: the input must be a traced tensor")
        return (x,), (name, tuple(range(-nd, 0)), True, "first", False)
    name = str(getattr(node.target, "__name__", node.target))
    kwargs = dict(node.kwargs)
    x = node.args[0] if node.args else kwargs.pop("input", None)
    kwargs.pop("input", None)
    if not isinstance(x, fx.Node):
        raise SweepUnsupported(f"{name}: the tensor must be a traced tensor")
    if kwargs.pop("out", None) is not None:
        raise SweepUnsupported(f"{name} with an out= argument (the sweep keeps its own values)")
    if kwargs.pop("dtype", None) is not None:
        raise SweepUnsupported(f"{name} with dtype= (the sweep keeps the dtype of the traced value)")
    rest = list(node.args[1:])
    if name == "max" and ((rest and isinstance(rest[0], fx.Node)) or isinstance(kwargs.get("other"), fx.Node)):
        raise SweepUnsupported("max(x, other): the element-wise maximum of two tensors has no rule (only max over a dim is served)")
    dim = rest.pop(0) if rest else kwargs.pop("dim", kwargs.pop("axis", None))
    keepdim = rest.pop(0) if rest else kwargs.pop("keepdim", False)
    if name == "sum" and rest:  # (the method's third positional argument)
        raise SweepUnsupported("sum with dtype= (the sweep keeps the dtype of the traced value)")
    if rest or kwargs:
        raise SweepUnsupported(f"{name}: unknown argument {sorted(kwargs) or rest}")
    if dim is None or (isinstance(dim, (tuple, list)) and not dim):
        raise SweepUnsupported(f"{name}() without a dim reduces the batch dim too (name the dims: dim 0 must stay)")
    if isinstance(keepdim, fx.Node) or not isinstance(keepdim, bool):
        raise SweepUnsupported(f"{name} with a data-dependent keepdim")
    dims = tuple(dim) if isinstance(dim, (tuple, list)) else (dim,)
    if name == "max" and isinstance(dim, (tuple, list)):
        raise SweepUnsupported("max over a tuple of dims (max takes one dim; amax takes several)")
    dims = tuple(_static_int(d, name, "dim") for d in dims)
    if 0 in dims:
        raise SweepUnsupported(f"{name} over {_BATCH_SLICE}")
    tie = None if kind == _SUMRED else "first" if name == "max" else "even"
    return (x,), (name, dims, keepdim, tie, name == "max")


def reduce_geometry(dims, shape, what="reduction"):
    """``(dims, outer, L, inner)`` of a _MAXRED / _SUMRED rule resolved on a value of ``shape``: the sorted non-batch dims (a
    maximum: adjacent ones) and the view ``[outer][L][inner]`` of the contiguous value in which they are one dim"""
    ndim = len(shape)
    for d in dims:
        if not -ndim <= d < ndim:
            raise SweepUnsupported(f"{what} along dim {d} of a value with {ndim} dims")
    res = sorted({d % ndim for d in dims})
    if len(res) != len(dims):
        raise SweepUnsupported(f"{what}: dim listed twice in {tuple(dims)}")
    if res[0] == 0:
        raise SweepUnsupported(f"{what} over {_BATCH_SLICE}")
    outer = L = inner = 1
    for i, d in enumerate(shape):
        if i < res[0]:
            outer *= int(d)
        elif i <= res[-1]:
            L *= int(d)
        else:
            inner *= int(d)
    return res, outer, L, inner


def reduce_forward_math(x3):
    """``(y, idx, cnt)`` of csrc/lk_reduce.hip's forward in plain torch (any dtype): ``x3`` is ``[outer, L, inner]``; the maximum
    over ``L``, the FIRST position that holds it and how many positions compare equal to it (int32; ``0.0 == -0.0``)"""
    L = x3.shape[1]
    y = x3.amax(1)
    eq = x3 == y.unsqueeze(1)
    pos = torch.arange(L, device=x3.device, dtype=torch.int32).reshape(1, L, 1)
    idx = torch.where(eq, pos, torch.full_like(pos, L)).amin(1)
    return y, idx, eq.sum(1, dtype=torch.int32)


def reduce_vjp_math(g, L, idx=None, x=None, y=None, cnt=None):
    """``dx`` ``[S, outer, L, inner]`` for the ``S`` seeds in ``g`` ``[S, outer, inner]`` - the formulas of lk_maxred_vjp_f32 in plain
    torch (any dtype): with ``idx`` the cotangent goes to the first maximum, ``(l == idx) ? g : 0``; with ``x``, ``y``, ``cnt`` it is
    split evenly over the maxima, ``(x == y) ? g / cnt : 0``"""
    if x is not None:
        hit, q = x == y.unsqueeze(1), g / cnt.to(g.dtype)
    else:
        pos = torch.arange(L, device=g.device, dtype=idx.dtype).reshape(1, L, 1)
        hit, q = pos == idx.unsqueeze(1), g
    return torch.where(hit.unsqueeze(0), q.unsqueeze(2), q.new_zeros(()))


def _no_slice_rule(target):
    """what a refusal adds for a relative of the slicing rules (``unbind``, ``tensor_split``, ``stack``) or of the matrix product
    (``einsum``, ``baddbmm``)"""
    name = _NO_MATMUL_RULE.get(target)
    if name is not None:
        return f" ({name} is out of scope: matmul, @ and bmm are what the sweep serves)"
    name = _NO_REDUCE_RULE.get(target)
    if name is not None:
        return f" ({name} is out of scope: amax, max(dim)[0], sum(dim) and the adaptive max pools to one cell are what the sweep serves)"
    name = _NO_SLICE_RULE.get(target)
    if name is None:
        return ""
    return f" ({name} is out of scope: chunk, split, narrow, static indexing of one dim and cat are what the sweep serves)"


def permutation(spelling, dims, ndim):
    """the full permutation of a PERMUTE rule on a value of ``ndim`` dims"""
    if spelling == "transpose":
        perm = list(range(ndim))
        d0, d1 = dims[0] % ndim, dims[1] % ndim
        perm[d0], perm[d1] = perm[d1], perm[d0]
    else:
        perm = [d % ndim for d in dims]
    if len(perm) != ndim or sorted(perm) != list(range(ndim)) or perm[0] != 0:
        raise SweepUnsupported(f"{spelling}{tuple(dims)} moves the batch dim (dim 0 must stay in place)")
    return perm


def classify(node: fx.Node, modules: dict) -> Rule:
    """The :class:`Rule` of a traced node — the one place that tells ``call_module`` / ``call_function`` / ``call_method``
    apart; whatever has no VJP rule is refused here, so that neither sweep meets it half-way."""
    if node.op in ("placeholder", "output"):
        return Rule(node.op)
    if node.op == "get_attr":
        try:
            attr = _fetch_attr(modules[""], node.target)
        except (AttributeError, KeyError, TypeError):
            attr = None
        if torch.is_tensor(attr) and not attr.requires_grad:  # a buffer or a frozen parameter: a constant of the sweep
            return Rule(CONST, what=f"constant {node.target}", args=(node.target,))
        if isinstance(attr, nn.Parameter):  # a tracked parameter no module owns: live, served where its consumers allow it
            return Rule(_PARAM, what=f"parameter {node.target}", args=(node.target,))
        raise SweepUnsupported("graph reads attributes directly")
    m, args, kwargs = None, node.args, dict(node.kwargs)
    if node.op == "call_module":
        m = fn = modules[node.target]
        hit, what = next(((k, fl) for types, k, fl in _MODULE_KINDS if isinstance(m, types)), None), type(m).__name__
        if isinstance(m, nn.Sequential):
            raise SweepUnsupported("nested Sequential was not inlined by the tracer")
        if hit is None:
            raise SweepUnsupported(f"no VJP rule for module {what} ({node.target})")
        # (grouped convolutions: forward is the module itself, backward-data `_conv_input_grad`, which passes `groups`)
        # (nn.Conv1d: the same rule - the module runs the forward, `_conv_input_grad` passes geometry tuples of any length)
        if isinstance(m, (nn.Conv2d, nn.Conv1d)) and (isinstance(m.padding, str) or m.padding_mode != "zeros"):
            raise SweepUnsupported(f"{node.target}: unsupported convolution variant")
    elif node.op == "call_function":
        if node.target in (operator.getitem, getattr) and args and isinstance(args[0], fx.Node):
            up = classify(args[0], modules)
            if up.kind == _MAXRED and up.args[4]:  # (an item of the pair a `max(dim)` returns: the node itself holds the values)
                if len(args) > 1 and not isinstance(args[1], (fx.Node, bool)) and args[1] in (0, "values"):
                    return Rule(IDENTITY, (args[0],), _same, ((args[0],), {}), f"values of {up.what}")
                raise SweepUnsupported(f"{up.what}: its indices ({args[1] if len(args) > 1 else None!r}) have no cotangent and no rule "
                                       "(take the values with [0] or .values)")
            if up.kind == _MHA:  # (an item of the pair an nn.MultiheadAttention returns: `_classify_mha` checked the index)
                return Rule(_MHAOUT, (args[0],), None, ((args[0],), {}), f"item {args[1]} of {up.what}", args=(int(args[1]),))
        fn, hit, what = node.target, _FUNCTION_KINDS.get(node.target), getattr(node.target, "__name__", node.target)
        if hit is None:
            raise SweepUnsupported(f"no VJP rule for function {what}" + _no_slice_rule(node.target))
    else:
        hit, what = _METHOD_KINDS.get(node.target), f"method {node.target}"
        if hit is None:
            raise SweepUnsupported(f"no VJP rule for method {node.target}" + _no_slice_rule(node.target))
        fn = getattr(torch.Tensor, node.target)
    kind, flavour = hit
    src, static = tuple(args[:1]), ()
    if kind in (GETITEM, SLICE):
        r = _classify_slice(node, modules, what)
        if r is not None:
            return r
    elif kind == SPLIT:
        if not (args and isinstance(args[0], fx.Node)):
            raise SweepUnsupported(f"{what}: the tensor must be the first positional argument and a traced tensor")
        static = _classify_split(node, what)
    elif kind == CONST and args and isinstance(args[0], fx.Node) and classify(args[0], modules).kind == _PARAM:
        # (`expand` / `expand_as` of a tracked parameter: the batch dim only, checked on the value in the forward)
        return Rule(_EXPAND, (args[0],), fn, (tuple(args), kwargs), f"{what} of parameter {args[0].target}", args=(args[0].target,))
    elif kind == CONST:  # (`expand` / `expand_as`: a constant when what it expands is one; evaluated in the forward)
        if not (args and isinstance(args[0], fx.Node) and classify(args[0], modules).kind == CONST):
            raise SweepUnsupported(f"{what} of a traced tensor (its VJP is a reduction, which has no rule; expanding a buffer or a "
                                   "frozen parameter is served)")
        what = f"constant {what} of {args[0].name}"
    if kind == _EMBED:
        ids = args[0] if args else None
        src_kind = classify(ids, modules).kind if isinstance(ids, fx.Node) else None
        if src_kind == CONST:  # (`nn.Embedding(arange)`: a position table written as a module)
            if m.weight.requires_grad:
                raise SweepUnsupported(f"{node.target}: Embedding of a constant index buffer with a tracked weight has no rule "
                                       "(write the position table as a parameter, or freeze it)")
            return Rule(CONST, (), m, ((ids,), {}), f"constant Embedding {node.target}")
        if src_kind != "placeholder":
            raise SweepUnsupported(f"{node.target}: Embedding of a traced tensor (the token ids must be the model's input)")
        if m.max_norm is not None:
            raise SweepUnsupported(f"{node.target}: Embedding with max_norm renormalises its weight in the forward pass")
    if kind == ADD:
        if kwargs.get("alpha", 1) != 1:
            raise SweepUnsupported("add with alpha")
        src, fn = tuple(args[:2]), operator.add if fn is operator.iadd else fn  # (`+=` must not write into a kept tensor)
    elif flavour == "generic":
        kwargs.pop("inplace", None)  # (the derivative is taken by autograd on a leaf)
    elif kind in _POOL_PARAMS:
        names, defaults = _POOL_PARAMS[kind]
        # (nn.AvgPool1d has no divisor_override: the default)
        p = {n: getattr(m, n, d) for n, d in zip(names, defaults)} if m is not None else _bind(node, names, defaults)
        if p.pop("return_indices", False):
            raise SweepUnsupported("max_pool1d(return_indices=True)" if flavour == "1d" else "max_pool2d(return_indices=True)")
        if flavour == "1d":  # (the unit-height window: the node lifts its input to [B, C, 1, L], `_run_pool`)
            p = {n: _unit_height(n, v) for n, v in p.items()}
        if kind == MAXPOOL:  # always evaluated with indices: they are what its VJP scatters by
            fn, args, kwargs = F.max_pool2d, (args[0], *p.values(), True), {}
        else:
            static = tuple(p.values())
            if flavour == "1d":  # (one spelling of the lifted window)
                fn, args, kwargs = F.avg_pool2d, (args[0], *static), {}
    elif kind == GPOOL:
        static = (m.output_size if m is not None else kwargs.get("output_size", args[1] if len(args) > 1 else None),)
    elif kind == MEAN:
        static = (kwargs.get("dim", args[1] if len(args) > 1 else None),
                  kwargs.get("keepdim", args[2] if len(args) > 2 else False))
    elif kind in (_MAXRED, _SUMRED):
        src, static = _classify_reduce(node, m, kind)
        what = static[0] if m is None else f"{what} ({node.target})"
        fn, args, kwargs, m = None, src, {}, None  # (evaluated by `SeedBatchedSweep._run_reduce`)
    elif kind == ATTN:
        src, static = _classify_attn(node)
    elif kind == _MHA:
        src = _classify_mha(node, m)
        args, kwargs, what = src, {}, f"MultiheadAttention ({node.target})"
    elif kind == PERMUTE:
        static = _classify_permute(node, what)
    elif kind == CAT:
        src, static = _classify_cat(node, what)
        fn, args, kwargs = torch.cat, (list(src),), {}  # (one spelling; the dim is resolved on the value)
    elif kind == MUL:
        src = _classify_mul(node, modules)
        if fn is operator.imul or node.target == "mul_":  # (`*=` / `mul_` must not write into a kept tensor)
            fn = operator.mul
    elif kind == MATMUL:
        src = _classify_matmul(node, modules)
        fn, what = torch.matmul, "matmul"  # (one spelling)
    elif kind == SOFTMAX:
        src, static, what = _classify_softmax(node, m, what)
        fn, args, kwargs = (torch.log_softmax if static[1] else torch.softmax), src, {}
    elif kind == SCALE:
        src, static = _classify_scale(node, modules)
        fn, args, kwargs, what = operator.truediv, (src[0], static[0]), {}, "div"  # (`/=` / `div_` must not write into a kept tensor)
    elif kind == NEG:
        src = _classify_neg(node)
        fn, args, kwargs, what = torch.neg, src, {}, "neg"  # (`neg_` must not write into a kept tensor)
        if classify(src[0], modules).kind == CONST:  # (`-sin` of a frozen buffer: a constant of the sweep, evaluated in the forward)
            return Rule(CONST, (), fn, (src, {}), f"constant neg of {src[0].name}")
    elif kind == SUB:
        src = _classify_sub(node, modules)
        fn, args, kwargs, what = operator.sub, src, {}, "sub"  # (`-=` / `sub_` must not write into a kept tensor)
    elif kind == _RESAMPLE:
        x, vals, what = _classify_resample(node, m, flavour, modules)
        # (one spelling: the modules make exactly this call; every argument by name, resolved on the values in the forward)
        fn, src, args, kwargs, static = (F.interpolate if flavour == "interpolate" else F.pad), (x,), (x,), vals, (flavour,)
        if classify(x, modules).kind == CONST:  # (a resampled frozen buffer: a constant of the sweep, evaluated in the forward)
            return Rule(CONST, (), fn, ((x,), vals), f"constant {what} of {x.name}")
    return Rule(kind, src, fn, (tuple(args), kwargs), what, flavour, m if kind in (CONV, LINEAR, BN, NORM, _EMBED, _MHA) else None, static)


def norm_geometry(m, inp):
    """``(view, G, layout)`` of a per-sample normalisation layer on ``inp`` in the convention of csrc/lk_normvjp.hip:
    nn.GroupNorm is ``[B, Ch, L]`` (layout 0) with its own ``G``; nn.LayerNorm is ``[rows, 1, D]`` (layout 1, ``L = 1``) with
    ``rows`` the product of the leading dims, ``D = prod(normalized_shape)`` and ``G = 1`` (as ``backend._norm_xhat``)."""
    if isinstance(m, nn.GroupNorm):
        if inp.dim() < 2 or inp.shape[1] != m.num_channels:
            raise SweepUnsupported(f"GroupNorm({m.num_groups}, {m.num_channels}) on an input of shape {tuple(inp.shape)}")
        return (inp.shape[0], m.num_channels, max(inp.numel() // max(inp.shape[0] * m.num_channels, 1), 1)), m.num_groups, 0
    D = 1
    for d in m.normalized_shape:
        D *= int(d)
    if tuple(inp.shape[inp.dim() - len(m.normalized_shape):]) != tuple(m.normalized_shape):
        raise SweepUnsupported(f"LayerNorm({tuple(m.normalized_shape)}) on an input of shape {tuple(inp.shape)}")
    return (inp.numel() // D, 1, D), 1, 1


def _norm_rows(t, G, layout):
    """``[.., B, Ch, L]`` / ``[.., B, L, Ch]`` -> the statistics rows ``[.., B, G, Ch / G, L]`` / ``[.., B, L, G, Ch / G]``,
    the dims a row reduces over, and the shape the affine vectors broadcast in"""
    if layout == 0:
        Ch, L = t.shape[-2], t.shape[-1]
        return t.reshape(*t.shape[:-2], G, Ch // G, L), (-2, -1), (G, Ch // G, 1)
    L, Ch = t.shape[-2], t.shape[-1]
    return t.reshape(*t.shape[:-2], L, G, Ch // G), (-3, -1), (1, G, Ch // G)


def norm_forward_math(x, w, b, G, layout, eps):
    """``(y, xhat, rstd)`` of csrc/lk_normvjp.hip's forward in plain torch (any dtype): ``x`` is ``[B, Ch, L]`` (layout 0) or
    ``[B, L, Ch]`` (layout 1); mean-shifted biased variance, ``rstd`` ``[B, G]``."""
    xr, dims, wshape = _norm_rows(x, G, layout)
    mu = xr.mean(dims, keepdim=True)
    d = xr - mu
    rstd = 1.0 / torch.sqrt((d * d).mean(dims, keepdim=True) + eps)
    xhat = d * rstd
    # (``y`` never shares storage with ``xhat``: an in-place op behind the layer - ReLU(inplace=True), ``out += identity`` -
    # writes into ``y``, and ``xhat`` is kept for the VJP)
    y = xhat * w.detach().reshape(wshape) if w is not None else xhat.clone()
    if b is not None:
        y = y + b.detach().reshape(wshape)
    return y.reshape(x.shape), xhat.reshape(x.shape), rstd.reshape(x.shape[0], G)


def norm_vjp_math(g, xhat, rstd, w, S, G, layout):
    """``dx = rstd * (t - mean_row(t) - xhat * mean_row(t * xhat))``, ``t = w * g``, for the ``S`` seeds stacked in ``g``
    (``[S*B, ..]`` in the layout of ``xhat`` ``[B, ..]``) - the formula of lk_norm_vjp_f32 in plain torch"""
    xr, dims, wshape = _norm_rows(xhat, G, layout)
    t, _, _ = _norm_rows(g.reshape(S, *xhat.shape), G, layout)
    if w is not None:
        t = t * w.detach().reshape(wshape)
    rs = rstd.reshape(rstd.shape[0], G, 1, 1) if layout == 0 else rstd.reshape(rstd.shape[0], 1, G, 1)
    dx = rs * (t - t.mean(dims, keepdim=True) - xr * (t * xr).mean(dims, keepdim=True))
    return dx.reshape(g.shape)


def rmsnorm_geometry(m, inp):
    """``(rows, D, eps)`` of an nn.RMSNorm on ``inp`` in the convention of csrc/lk_rmsnorm.hip: ``D = prod(normalized_shape)``,
    ``rows`` the product of the leading dims; ``eps`` is the module's, or torch's default for the input's dtype"""
    D = 1
    for d in m.normalized_shape:
        D *= int(d)
    if tuple(inp.shape[inp.dim() - len(m.normalized_shape):]) != tuple(m.normalized_shape) or inp.dim() < len(m.normalized_shape):
        raise SweepUnsupported(f"RMSNorm({tuple(m.normalized_shape)}) on an input of shape {tuple(inp.shape)}")
    return inp.numel() // max(D, 1), D, float(m.eps) if m.eps is not None else torch.finfo(inp.dtype).eps


def rmsnorm_forward_math(x, w, eps):
    """``(y, rstd)`` of csrc/lk_rmsnorm.hip's forward in plain torch (any dtype): ``x`` is ``[rows, D]``,
    ``rstd = 1 / sqrt(mean_row(x^2) + eps)`` ``[rows]``, ``y = w * (x * rstd)`` (a tensor of its own: ``x`` is kept for the VJP)"""
    rstd = 1.0 / torch.sqrt((x * x).mean(-1) + eps)
    y = x * rstd.unsqueeze(-1)
    if w is not None:
        y = y * w.detach().reshape(-1)
    return y, rstd


def rmsnorm_vjp_math(g, x, rstd, w, S):
    """``dx = rstd * (t - xh * mean_row(t * xh))``, ``t = w * g``, ``xh = x * rstd``, for the ``S`` seeds stacked in ``g``
    (``[S*rows, D]``, ``x`` ``[rows, D]``) - the formula of lk_rmsnorm_vjp_f32 in plain torch"""
    t = g.reshape(S, *x.shape)
    if w is not None:
        t = t * w.detach().reshape(-1)
    rs = rstd.unsqueeze(-1)
    xh = x * rs
    return (rs * (t - xh * (t * xh).mean(-1, keepdim=True))).reshape(g.shape)


def attn_layout(t):
    """memory layout of an attention operand ``[B, H, T, D]`` in the convention of csrc/lk_attn.hip: 0 when it is contiguous
    (``[B][H][T][D]``), 1 when its ``transpose(1, 2)`` is (``[B][T][H][D]``, what ``Linear -> view -> transpose`` leaves), else
    ``None``"""
    if t.is_contiguous():
        return 0
    return 1 if t.transpose(1, 2).is_contiguous() else None


def attn_operands(*ts):
    """``(layout, tensors)``: the operands as they are when all of them lie in the same one of the two layouts (nothing is
    copied), else contiguous copies (layout 0)"""
    layouts = {attn_layout(t) for t in ts}
    if len(layouts) == 1 and None not in layouts:
        return layouts.pop(), ts
    return 0, tuple(t.contiguous() for t in ts)


def attn_like(shape, layout, like):
    """an uninitialised ``[N, H, T, D]`` tensor (a view, in ``layout``) of the dtype and device of ``like``"""
    N, H, T, D = shape
    if layout == 0:
        return like.new_empty(N, H, T, D)
    return like.new_empty(N, T, H, D).transpose(1, 2)


def attn_forward_math(q, k, v, scale, causal):
    """``(o, p)`` of scaled dot-product self-attention on ``[B, H, T, D]`` operands in plain torch (any dtype):
    ``p = softmax(scale * q k^T (+ causal mask: key j <= query i))``, ``o = p v``"""
    s = (q @ k.transpose(-1, -2)) * scale
    if causal:
        T = q.shape[-2]
        s = s.masked_fill(~torch.ones(T, T, dtype=torch.bool, device=q.device).tril(), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return p @ v, p


def attn_vjp_math(go, q, k, v, o, p, S, scale, max_bytes=None):
    """``(dq, dk, dv)``, each ``[S*B, H, T, D]``, for the ``S`` seeds stacked in ``go`` ``[S*B, H, T, D]`` from ONE ``q``, ``k``,
    ``v``, ``o``, ``p`` per sample - the formula of lk_attn_vjp_f32 in plain torch:
    ``dv = p^T go``, ``dp = go v^T``, ``delta = rowsum(go * o)``, ``ds = p * (dp - delta)``, ``dq = scale ds k``,
    ``dk = scale ds^T q``.  ``max_bytes``: the seeds go through in chunks whose three ``[s, B, H, T, T]`` temporaries stay below it."""
    B, H, T, D = q.shape
    g = go.reshape(S, B, H, T, D)
    per_seed = 3 * max(B * H * T * T, 1) * go.element_size()
    chunk = S if max_bytes is None else max(1, min(S, int(max_bytes) // per_seed))
    dq, dk, dv = (go.new_empty(S, B, H, T, D) for _ in range(3))
    pt, vt = p.transpose(-1, -2), v.transpose(-1, -2)
    for s0 in range(0, S, chunk):
        gc = g[s0:s0 + chunk]
        torch.matmul(pt, gc, out=dv[s0:s0 + chunk])
        ds = p * (gc @ vt - (gc * o).sum(-1, keepdim=True))
        torch.matmul(ds, k, out=dq[s0:s0 + chunk])
        torch.matmul(ds.transpose(-1, -2), q, out=dk[s0:s0 + chunk])
    dq *= scale
    dk *= scale
    return dq.reshape(S * B, H, T, D), dk.reshape(S * B, H, T, D), dv.reshape(S * B, H, T, D)


def matmul_vjp_math(g, a, b, S, want=(True, True), max_bytes=None):
    """``(da, db)`` of ``out = a @ b`` for the ``S`` seeds stacked in ``g`` ``[S*B, *, M, N]`` from ONE ``a`` ``[B, *, M, K]`` and ``b``
    ``[B, *, K, N]`` per sample - the formula of lk_matmul_vjp_f32 in plain torch (any dtype): ``da = g b^T``, ``db = a^T g``.
    ``max_bytes``: the seeds go through in chunks whose broadcast operands (torch expands ``b`` / ``a`` once per seed) stay below it."""
    gv = g.reshape(S, *a.shape[:-2], a.shape[-2], b.shape[-1])
    per_seed = max(a.numel() + b.numel(), 1) * g.element_size()
    chunk = S if max_bytes is None else max(1, min(S, int(max_bytes) // per_seed))
    da = g.new_empty(S, *a.shape) if want[0] else None
    db = g.new_empty(S, *b.shape) if want[1] else None
    at, bt = a.transpose(-1, -2), b.transpose(-1, -2)
    for s0 in range(0, S, chunk):
        if want[0]:
            torch.matmul(gv[s0:s0 + chunk], bt, out=da[s0:s0 + chunk])
        if want[1]:
            torch.matmul(at, gv[s0:s0 + chunk], out=db[s0:s0 + chunk])
    return (None if da is None else da.reshape(S * a.shape[0], *a.shape[1:]),
            None if db is None else db.reshape(S * b.shape[0], *b.shape[1:]))


def softmax_vjp_math(g, y, S, dim, is_log=False, max_bytes=None):
    """``dx`` for the ``S`` seeds stacked in ``g`` ``[S*B, ...]`` from ONE output ``y`` ``[B, ...]`` per sample - the formula of
    lk_softmax_vjp_f32 in plain torch (any dtype, any non-batch ``dim`` of ``y``): ``y * (g - sum(g y))``, or
    ``g - exp(y) sum(g)`` for a log-softmax.  ``max_bytes``: the seeds go through in chunks whose two temporaries stay below it."""
    gv = g.reshape(S, *y.shape)
    per_seed = 2 * max(y.numel(), 1) * g.element_size()
    chunk = S if max_bytes is None else max(1, min(S, int(max_bytes) // per_seed))
    dx = g.new_empty(S, *y.shape)
    p = torch.exp(y) if is_log else y
    for s0 in range(0, S, chunk):
        gc = gv[s0:s0 + chunk]
        if is_log:
            dx[s0:s0 + chunk] = gc - p * gc.sum(dim + 1, keepdim=True)
        else:
            dx[s0:s0 + chunk] = p * (gc - (gc * p).sum(dim + 1, keepdim=True))
    return dx.reshape(g.shape)


def _sum(parts):
    """the sum of a non-empty list of cotangent parts, left to right"""
    return parts[0] if len(parts) == 1 else sum(parts[1:], parts[0])


class _Walk:
    """The state of ONE reverse walk (`SeedBatchedSweep.backward` creates it; nothing of it outlives the call)."""

    def __init__(self, sweep, seeds, on_tap, defer_bn_scale):
        self.rule, self.on_tap, self.defer_bn_scale = sweep.rule, on_tap, defer_bn_scale
        self.S, self.B = seeds.shape[0], seeds.shape[1]
        # per node: the pending addends of its output cotangent (summed lazily, so that an activation can fold
        # the residual-branch addition into its own kernel)
        self.cot: dict[fx.Node, list] = {sweep.out_node: [seeds.reshape(self.S * self.B, *seeds.shape[2:])]}
        # per node: the pieces ``(cotangent, dim, start, length, input shape)`` its SLICE consumers hand back, assembled with the
        # full-width parts ONCE, when the node itself is reached
        self.pieces: dict[fx.Node, list] = {}
        self.grads: dict = {}
        self.remaining = set(sweep.tap_names)
        self.pending_scale: dict[fx.Node, torch.Tensor] = {}  # conv node -> the BatchNorm scale its backward-data applies
        self.grad_scale: dict[str, torch.Tensor] = {}  # (the sweep's public ``grad_scale`` of this walk)

    def live(self, n) -> bool:
        """does ``n`` receive a cotangent?  (a constant, a Python number and the input have none)"""
        return isinstance(n, fx.Node) and n.op != "placeholder" and self.rule[n].kind != CONST

    def push(self, n, g):
        if self.live(n):
            self.cot.setdefault(n, []).append(g)

    def tap(self, name, g) -> bool:
        """record the gradient of the tapped module ``name``; ``True``: it was the last one the walk owed"""
        self.grads[name] = g
        if self.on_tap is not None:
            self.on_tap(name, g)
        self.remaining.discard(name)
        return not self.remaining


class SeedBatchedSweep:
    """Forward + seed-batched reverse sweep over an fx-traced module."""

    @staticmethod
    def _with_derivative(fn, inp):
        """(fn(inp), d fn / d inp) for an element-wise ``fn``"""
        with torch.enable_grad():
            xin = inp.detach().requires_grad_(True)
            out = fn(xin)
            (d,) = torch.autograd.grad(out.sum(), xin)
        return out.detach(), d

    def __init__(self, model: nn.Module, tap_modules: dict[str, nn.Module], kernels=None):
        """``kernels``: callable returning the kernel object (``laplace_amd._lib.get_kernels``) whose
        ``vjp_scale_mask`` applies the element-wise VJPs to all seeds in one launch (lk_vjp.hip); ``None``
        = plain torch math (reference implementation of the same rule, used by the CPU tests)."""
        self.kernels = kernels
        self._bn_cache: dict[str, tuple] = {}
        self._w_cache: dict[str, tuple] = {}
        try:
            self.gm = fx.symbolic_trace(model)
        except Exception as e:  # data-dependent control flow, non-tensor inputs, ...
            raise SweepUnsupported(f"torch.fx cannot trace the model: {e}") from e
        mha.expand_encoders(self.gm)  # (the stock encoder: a leaf of the tracer, rewritten into nodes for its sub-modules)
        self.modules = dict(self.gm.named_modules())
        self.tap_names = set(tap_modules)
        #: node -> :class:`Rule`, in graph order (the graph does not change after tracing)
        self.rule: dict[fx.Node, Rule] = {}
        for node in self.gm.graph.nodes:
            try:
                self.rule[node] = classify(node, self.modules)
            except SweepUnsupported as e:  # (a refusal of an operation that reads a tracked parameter names the parameter)
                lone = [a.target for a in node.all_input_nodes if self.rule.get(a, Rule("")).kind == _PARAM]
                if not lone:
                    raise
                raise SweepUnsupported(f"parameter {lone[0]}: {e}") from e
        for node, r in self.rule.items():
            if r.kind == _PARAM:
                if node.target not in self.tap_names:  # (nobody asked for its cotangent: the refusal such a graph always got)
                    raise SweepUnsupported("graph reads attributes directly")
                for u in node.users:
                    self._param_consumer(node.target, u, self.rule[u])
        if sum(r.kind == "placeholder" for r in self.rule.values()) != 1:
            raise SweepUnsupported("models with one tensor input only")
        for node, r in self.rule.items():  # (a tuple of parts has no cotangent: only its items do)
            if r.kind == SPLIT and any(self.rule[u].kind != SLICE for u in node.users):
                raise SweepUnsupported(f"{r.what}: its parts must be taken one by one with a static integer index")
            if r.kind == _MAXRED and r.args[4] and any(self.rule[u].fn is not _same for u in node.users):
                raise SweepUnsupported(f"{r.what}(dim) returns (values, indices): take the values with [0] or .values")
        self.out_node = next(reversed(self.rule)).args[0]
        if not isinstance(self.out_node, fx.Node):
            raise SweepUnsupported("model must return a single tensor")
        # the modules whose VJP rules assume eval mode
        self._mode_mods = [m for m in self.gm.modules() if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d, nn.Dropout))]

    _PARAM_REFUSALS = {MUL: "a product with a tracked parameter (LayerScale) has no rule",
                       MATMUL: "matmul with a tracked parameter has no rule"}

    def _param_consumer(self, target, user, ru):
        """a tracked lone parameter is served where its per-sample cotangent is the arriving one: under ``+`` and under an
        ``expand`` of the batch dim; everything else is refused by a message that names the parameter"""
        if ru.kind == _EXPAND:
            return
        if ru.kind == ADD:
            if all(isinstance(a, fx.Node) and self.rule[a].kind in (_PARAM, _EXPAND, CONST) for a in ru.src):
                raise SweepUnsupported(f"parameter {target}: the sum has no per-sample operand")
            return
        why = self._PARAM_REFUSALS.get(ru.kind, f"{ru.what} reads a tracked parameter, which has no rule")
        raise SweepUnsupported(f"parameter {target}: {why}")

    @staticmethod
    def _param_shape_check(target, p_shape, full_shape, what):
        """the parameter's shape is the per-sample operand's with a 1, or nothing, at the batch dim: no reduction is owed"""
        p, full = tuple(p_shape), tuple(full_shape)
        if not (p == full[1:] or (len(p) == len(full) and p[0] == 1 and p[1:] == full[1:])):
            raise SweepUnsupported(f"parameter {target}: {what} broadcasts {p} along a non-batch dim of {full}: its cotangent "
                                   "needs a reduction, which has no rule")

    # ---- forward ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x: torch.Tensor, need_vjp: bool = True):
        """Returns ``f``; fills ``self.saved`` (per node: what the VJP needs) and ``self.taps[name]['a']``.
        ``need_vjp=False``: inference only (the feature pass of the last-layer flavours) — nothing is kept for a
        reverse sweep, only the tapped inputs."""
        if self.gm.training or any(m.training for m in self._mode_mods):
            raise SweepUnsupported("model must be in eval mode (BatchNorm / Dropout VJPs assume it)")
        env: dict[fx.Node, Any] = {}
        self.saved: dict[fx.Node, Any] = {}
        self.taps: dict[str, dict] = {}
        fused_relu: dict[fx.Node, tuple] = {}  # ReLU node -> (output, mask) already produced by the BatchNorm kernel
        self.max_act_numel = 1  # largest per-sample activation: bounds the memory of a seed-batched cotangent
        self._attn_math_numel = 0  # largest [B, H, T, T] an attention node on the torch math forms per seed
        for node, r in self.rule.items():
            if node in fused_relu:
                env[node], keep = fused_relu.pop(node)
                if keep is not None:
                    self.saved[node] = keep
                continue
            kind = r.kind
            if kind == "placeholder":
                env[node] = x
                continue
            if kind == "output":
                continue
            if kind == CONST:
                if r.fn is None:
                    env[node] = _fetch_attr(self.gm, r.args[0]).detach()
                else:  # (an expanded constant)
                    args, kwargs = fx.node.map_arg(r.call, env.__getitem__)
                    env[node] = r.fn(*args, **kwargs)
                continue
            if kind == _PARAM:
                env[node] = _fetch_attr(self.gm, r.args[0]).detach()
                if node.target in self.tap_names:
                    self.taps[node.target] = {"a": None, "node": node}
                continue
            args, kwargs = fx.node.map_arg(r.call, env.__getitem__)
            if kind == _EXPAND:
                out = r.fn(*args, **kwargs)
                self._param_shape_check(r.args[0], args[0].shape, (x.shape[0],) + tuple(out.shape[1:]), "expand")
                if out.shape[0] != x.shape[0] or args[0].dim() != out.dim():
                    raise SweepUnsupported(f"parameter {r.args[0]}: expand along a non-batch dim needs a reduction, which has no rule")
                env[node] = out
                continue
            if kind == ADD:
                for a, other in zip(r.src, reversed(r.src)):
                    if isinstance(a, fx.Node) and self.rule[a].kind == _PARAM:
                        if not torch.is_tensor(env.get(other)):
                            raise SweepUnsupported(f"parameter {a.target}: add with a Python number")
                        self._param_shape_check(a.target, env[a].shape, env[other].shape, "add")
            inp, keep = args[0], None  # (keep: what the node's VJP needs)
            if (kind == BN and self.kernels is not None and inp.dim() >= 2 and inp.dtype == torch.float32
                    and r.mod.running_var is not None):
                # eval-mode BatchNorm = per-channel affine map: one fused launch, with the ReLU that follows it
                # (and the mask its VJP needs) when the BatchNorm output has no other consumer
                scale, shift = self._bn_scale(node.target, r.mod), self._bn_shift(node.target, r.mod)
                nxt = next(iter(node.users)) if len(node.users) == 1 else None
                addend, add_node = None, None
                if nxt is not None and self.rule[nxt].kind == ADD and all(isinstance(a, fx.Node) for a in nxt.args):
                    # residual join `bn(..) + other`: folded in when the other branch is already available
                    other = nxt.args[1] if nxt.args[0] is node else nxt.args[0]
                    if other in env and torch.is_tensor(env[other]) \
                            and env[other].shape == inp.shape and env[other].dtype == inp.dtype:
                        addend, add_node = env[other], nxt
                        nxt = next(iter(add_node.users)) if len(add_node.users) == 1 else None
                relu = nxt is not None and self.rule[nxt].flavour == "relu" and nxt.args[0] is (add_node or node)
                self._group_out_node = nxt if relu else (add_node or node)  # (whose users read this launch's output)
                out, mask = self._run_bn_act(node, inp, scale, shift, relu, addend, need_vjp)
                if add_node is not None:
                    fused_relu[add_node] = (out, None)  # (the add node itself keeps nothing for its VJP)
                if relu:
                    fused_relu[nxt] = (out, mask)
            elif kind == CONV:
                out, keep = self._run_conv(node, r.mod, inp), inp.shape
            elif kind == NORM:
                out, keep = self._run_norm(node, r.mod, inp)
                keep = keep if need_vjp else None
            elif kind in (MAXPOOL, AVGPOOL):
                out, keep = self._run_pool(node, r, args, kwargs)
                keep = keep if need_vjp else None
            elif kind in (_MAXRED, _SUMRED):
                out, keep = self._run_reduce(r, inp)
                keep = keep if need_vjp else None
            elif kind == ATTN:
                out, keep = self._run_attn(r, *(env[n] for n in r.src))
                keep = keep if need_vjp else None
            elif kind == _MHA:
                out, keep = self._run_mha(node, r, inp)
                keep = keep if need_vjp else None
            elif kind == _MHAOUT:
                out = inp[r.args[0]]
            elif kind == PERMUTE:
                perm = permutation(*r.args, inp.dim())
                out, keep = inp.permute(perm), [perm.index(i) for i in range(len(perm))]  # (keep: the inverse permutation)
            elif kind == CAT:
                if not all(torch.is_tensor(t) for t in inp):
                    raise SweepUnsupported(f"{r.what}: an entry of the list is not a tensor")
                dim = cat_dim(r.args[0], inp[0].dim(), r.what)
                out, keep = self._run_cat(node, r, inp, dim), (dim, tuple(int(t.shape[dim]) for t in inp))
            elif kind == SLICE:
                if not torch.is_tensor(inp):
                    raise SweepUnsupported(f"{r.what}: the source is not a tensor")
                keep = (*slice_range(r.args, inp.shape, r.what), inp.shape)
                out = self._run_slice(node, r, inp, *keep[:4])
            elif kind == SPLIT:
                try:
                    out = r.fn(*args, **kwargs)
                except (RuntimeError, TypeError, IndexError) as e:  # (sections that do not fit the value: torch's own words)
                    raise SweepUnsupported(f"{r.what}: {e}") from e
            elif kind == MUL:
                out, keep = self._run_mul(r, args)
                keep = keep if need_vjp else None
            elif kind == MATMUL:
                out, keep = self._run_matmul(r, args)
                keep = keep if need_vjp else None
            elif kind == SOFTMAX:
                out, keep = self._run_softmax(r, inp)
                keep = keep if need_vjp else None
            elif kind == SCALE:
                if not torch.is_tensor(inp):
                    raise SweepUnsupported(f"div: the dividend is not a tensor ({type(inp).__name__})")
                out = inp / r.args[0]
            elif kind == NEG:
                if not torch.is_tensor(inp):
                    raise SweepUnsupported(f"neg: the operand is not a tensor ({type(inp).__name__})")
                out = torch.neg(inp)
            elif kind == SUB:
                out = self._run_sub(r, args)
            elif kind == _RESAMPLE:
                out, keep = self._run_resample(node, r, inp, kwargs, need_vjp)
            elif kind == ADD and any(isinstance(a, fx.Node) and self.rule[a].kind == CONST for a in r.src):
                out = self._add_const(r, args, kwargs)
            elif r.flavour == "generic" and need_vjp:
                out, keep = self._with_derivative(lambda t: r.fn(t, *args[1:], **kwargs), inp)
            elif kind == GETITEM and torch.is_tensor(inp):
                raise SweepUnsupported("tensor indexing")
            else:
                out = r.fn(*args, **kwargs)
                if kind == ACT and need_vjp:  # (tanh / sigmoid: the derivative is a function of the value)
                    keep = (out > 0) if r.flavour == "relu" else out
                elif kind in (RESHAPE, GPOOL):
                    keep = inp.shape
                elif kind == MEAN:
                    dim, keepdim = fx.node.map_arg(r.args, env.__getitem__)
                    keep = (inp.shape, bool(keepdim), self._mean_dims(dim, inp.dim()))
            if keep is not None:
                self.saved[node] = keep
            if r.mod is not None and node.target in self.tap_names:
                if node.target in self.taps:
                    raise SweepUnsupported(f"{node.target}: module is applied more than once per forward")
                self.taps[node.target] = {"a": inp, "node": node}
            env[node] = out
        if not need_vjp:
            self.saved = {}
        nb = max(int(x.shape[0]), 1)
        self.max_act_numel = max(self.max_act_numel, self._attn_math_numel // nb)
        for v in env.values():
            if torch.is_tensor(v):
                self.max_act_numel = max(self.max_act_numel, v.numel() // nb)
        missing = self.tap_names - set(self.taps)
        if missing:
            raise SweepUnsupported(f"tapped modules not reached by the traced forward: {sorted(missing)}")
        out = env[self.out_node]
        self.out_shape = tuple(out.shape[1:])
        return out

    # ---- forward hooks (the NHWC sweep replaces them with its own kernels) -----------------------------------------
    def _run_conv(self, node, m, inp):
        return m(inp)

    def _run_bn_act(self, node, inp, scale, shift, relu, addend, want_mask):
        return self.kernels().bn_act_forward(inp.contiguous(), scale, shift, relu,
                                             None if addend is None else addend.contiguous(), want_mask=want_mask)

    def _run_pool(self, node, r, args, kwargs):
        """max / average pooling forward -> ``(out, keep)``: a max pool is evaluated with indices (`classify`), which are what
        its VJP scatters by; the average's VJP needs the input's shape only"""
        if r.flavour == "1d":  # (lifted at the node: [B, C, L] -> [B, C, 1, L] in, the height squeezed out; the VJP lifts back)
            if not torch.is_tensor(args[0]) or args[0].dim() != 3:
                raise SweepUnsupported(f"{r.what}: a 1-D pool on a value that is not [B, C, L]")
            args = (args[0].unsqueeze(2), *args[1:])
        if r.kind == MAXPOOL:
            out, idx = r.fn(*args)
            keep = (idx, args[0].shape)
        else:
            out, keep = r.fn(*args, **kwargs), args[0].shape
        return (out.squeeze(2) if r.flavour == "1d" else out), keep

    def _run_cat(self, node, r, tensors, dim):
        """concatenation forward along the resolved ``dim`` (the VJP needs the sources' sizes along it only)"""
        return torch.cat(list(tensors), dim)

    def _run_slice(self, node, r, inp, dim, start, length, dropped):
        """static slice forward: a view (the VJP needs the range and the input's shape only)"""
        return inp.select(dim, start) if dropped else inp.narrow(dim, start, length)

    #: ``False``: the cotangent of a sliced tensor is assembled by the torch sequence (zero fill, ``narrow(...).add_`` per
    #: slice, a sum with the full-width parts) whatever the kernel object offers
    use_slice_kernels = True

    def _slice_kernels(self, ts):
        """the kernel object when csrc/lk_slice.hip assembles the cotangent of a sliced tensor from ``ts`` (an object with the entry
        points - the stock emulation has none -, fp32), else ``None``: the same formula in torch"""
        K = self.kernels() if self.kernels is not None and self.use_slice_kernels else None
        if K is None or not hasattr(K, "slice_vjp") or not all(t.dtype == torch.float32 for t in ts):
            return None
        return K

    @staticmethod
    def slice_columns(shape, dim, start, length):
        """``(R, Ct, c0, cs)``: a slice along ``dim`` of a contiguous tensor of ``shape`` as the column range ``[c0, c0 + cs)`` of
        the row matrix ``[R = prod(dims before dim)][Ct = prod(dims from dim)]``"""
        R = inner = 1
        for d in shape[:dim]:
            R *= int(d)
        for d in shape[dim + 1:]:
            inner *= int(d)
        return R, int(shape[dim]) * inner, start * inner, length * inner

    @staticmethod
    def slice_vjp_launches(K, pieces, R, Ct, amax=None):
        """the ``[R, Ct]`` sum of the pieces ``(value, c0, cs)`` in ONE launch of lk_slice_vjp_f32; beyond ``K.SLICE_MAX_PIECES``
        the result so far is the full-width first piece of a further launch (rare: a tensor read by more than eight nodes)"""
        pieces, n = list(pieces), K.SLICE_MAX_PIECES
        while len(pieces) > n:
            pieces = [(K.slice_vjp(pieces[:n], R, Ct), 0, Ct)] + pieces[n:]
        return K.slice_vjp(pieces, R, Ct, amax=amax)

    def _assemble_slices(self, parts, pieces, shape):
        """the cotangent ``[S*B, ...]`` (``shape``) of a tensor some of whose consumers are slices: the sum of the full-width
        ``parts`` and, per range, of the ``pieces`` ``(g, dim, start, length)``; zero where no piece reaches.  One launch of
        lk_slice_vjp_f32 per sliced dim (every network here slices one), or the same formula in torch."""
        K = self._slice_kernels([*parts, *(p[0] for p in pieces)])
        if K is not None and shape[0] > 0:
            out, full = None, [(g.contiguous(), 0, None) for g in parts]
            for dim in sorted({p[1] for p in pieces}):
                R, Ct, _, _ = self.slice_columns(shape, dim, 0, 1)
                if not (Ct < (1 << 30) and R * Ct < (1 << 40)):
                    out = None
                    break
                cols = [(g, 0, Ct) for g, _, _ in full]
                cols += [(g.contiguous(), *self.slice_columns(shape, dim, st, ln)[2:]) for g, d, st, ln in pieces if d == dim]
                out = self.slice_vjp_launches(K, cols, R, Ct).reshape(shape)
                full = [(out, 0, None)]
            if out is not None:
                return out
        out = parts[0].clone() if len(parts) == 1 else sum(parts[1:], parts[0]) if parts else pieces[0][0].new_zeros(shape)
        for g, dim, start, length in pieces:
            out.narrow(dim, start, length).add_(g)
        return out

    @staticmethod
    def pool_params(r) -> dict:
        """the static arguments of a MAXPOOL / AVGPOOL rule by name (``stride``: the window when none is given, as torch)"""
        if r.kind == MAXPOOL:  # (`classify` made the call positional: input, the five parameters, return_indices)
            p = dict(zip(_POOL_PARAMS[MAXPOOL][0][:5], r.call[0][1:6]))
        else:
            p = dict(zip(_POOL_PARAMS[AVGPOOL][0], r.args))
        pair = SeedBatchedSweep._pair2
        k = tuple(int(v) for v in pair(p["kernel_size"]))
        st = k if p["stride"] in (None, [], ()) else tuple(int(v) for v in pair(p["stride"]))
        return {"kernel": k, "stride": st, "padding": tuple(int(v) for v in pair(p["padding"])),
                "dilation": tuple(int(v) for v in pair(p.get("dilation", 1))), "ceil_mode": bool(p["ceil_mode"]),
                "count_include_pad": bool(p.get("count_include_pad", True)), "divisor_override": p.get("divisor_override")}

    def _norm_kernels(self, t):
        """the kernel object when it serves per-sample normalisation of ``t`` (fp32 and an object with the entry points; the
        stock emulation has none), else ``None``: plain torch math with the same formula"""
        K = self.kernels() if self.kernels is not None else None
        return K if K is not None and hasattr(K, "norm_forward") and t.dtype == torch.float32 else None

    #: ``False``: nn.RMSNorm stays on the torch math of its rule (`rmsnorm_forward_math`, `rmsnorm_vjp_math`) whatever the kernel
    #: object offers
    use_rmsnorm_kernels = True

    def _rmsnorm_kernels(self, t, S, rows, D):
        """the kernel object when csrc/lk_rmsnorm.hip serves an nn.RMSNorm on ``t`` (an object with the entry points - the stock
        emulation has none -, fp32, a shape inside the contract), else ``None``: the same formulas in torch"""
        K = self.kernels() if self.kernels is not None and self.use_rmsnorm_kernels else None
        if K is None or not hasattr(K, "rmsnorm_forward") or t.dtype != torch.float32 or rows == 0:
            return None
        return K if K.rmsnorm_variant(S, rows, D) is not None else None

    def _run_rmsnorm(self, m, inp):
        """nn.RMSNorm forward -> ``(out, ("rms", x [rows, D], rstd))``: ``xhat = x * rstd`` is one multiply away from the input,
        so the VJP keeps the input's view and one ``rstd`` per row, shared by all seeds (csrc/lk_rmsnorm.hip)"""
        rows, D, eps = rmsnorm_geometry(m, inp)
        x = inp.contiguous().reshape(rows, D)
        w = None if m.weight is None else m.weight.detach().reshape(-1)
        K = self._rmsnorm_kernels(x, 1, rows, D)
        if K is not None:
            y, rstd = K.rmsnorm_forward(x, None if w is None else w.contiguous(), eps)
        else:
            y, rstd = rmsnorm_forward_math(x, w, eps)
        return y.reshape(inp.shape), ("rms", x, rstd)

    def _rmsnorm_vjp(self, m, saved, g, S):
        """input cotangent of an nn.RMSNorm for all seeds: ONE launch of lk_rmsnorm_vjp_f32 (or the same formula in torch);
        ``g`` is ``[S*B, ...]``"""
        _, x, rstd = saved
        w = None if m.weight is None else m.weight.detach().reshape(-1)
        gv = g.contiguous().reshape(S * x.shape[0], x.shape[1])
        K = self._rmsnorm_kernels(gv, S, x.shape[0], x.shape[1]) if x.dtype == torch.float32 else None
        if K is not None:
            return K.rmsnorm_vjp(gv, x, rstd, None if w is None else w.contiguous(), S).reshape(g.shape)
        return rmsnorm_vjp_math(gv, x, rstd, w, S).reshape(g.shape)

    def _run_sub(self, r, args):
        """difference forward: two traced tensors of equal shape, a traced tensor and a constant that broadcasts to exactly its
        shape (`_add_const`'s condition), or a traced tensor and a Python number on either side; the VJP is a sign and keeps
        nothing"""
        a, b = args
        nodes = [isinstance(n, fx.Node) for n in r.src]
        for t, is_node in zip((a, b), nodes):
            if is_node and not torch.is_tensor(t):
                raise SweepUnsupported(f"sub: an operand is not a tensor ({type(t).__name__})")
        if all(nodes):
            const = [self.rule[n].kind == CONST for n in r.src]
            if any(const):
                c, other = (a, b) if const[0] else (b, a)
                if tuple(torch.broadcast_shapes(c.shape, other.shape)) != tuple(other.shape):
                    raise SweepUnsupported(f"sub: {tuple(other.shape)} broadcasts against the {self.rule[r.src[const.index(True)]].what} "
                                           f"of shape {tuple(c.shape)} (the VJP needs a reduction)")
            elif a.shape != b.shape:
                raise SweepUnsupported(f"sub of {tuple(a.shape)} and {tuple(b.shape)}: traced operands of different shapes (the VJP "
                                       "needs a reduction)")
        return a - b

    def _run_norm(self, node, m, inp):
        """GroupNorm / LayerNorm forward -> ``(out, (xhat, rstd, G, layout))``: what the VJP needs is one normalised input
        and one ``rstd`` per statistics row, shared by all seeds (csrc/lk_normvjp.hip); nn.RMSNorm: `_run_rmsnorm`"""
        if isinstance(m, nn.RMSNorm):
            return self._run_rmsnorm(m, inp)
        view, G, layout = norm_geometry(m, inp)
        x = inp.contiguous().reshape(view)
        K = self._norm_kernels(x)
        w = None if m.weight is None else m.weight.detach().reshape(-1)
        b = None if m.bias is None else m.bias.detach().reshape(-1)
        if K is not None:
            y, xhat, rstd = K.norm_forward(x, None if w is None else w.contiguous(), None if b is None else b.contiguous(),
                                           G, layout, m.eps)
        else:
            y, xhat, rstd = norm_forward_math(x, w, b, G, layout, m.eps)
        return y.reshape(inp.shape), (xhat, rstd, G, layout)

    def _norm_vjp(self, m, saved, g, S):
        """input cotangent of a GroupNorm / LayerNorm for all seeds: ONE launch of lk_norm_vjp_f32 (or the same formula in
        torch); ``g`` is ``[S*B, ...]``"""
        if saved[0] == "rms":
            return self._rmsnorm_vjp(m, saved, g, S)
        xhat, rstd, G, layout = saved
        K = self._norm_kernels(g)
        w = None if m.weight is None else m.weight.detach().reshape(-1)
        gv = g.contiguous().reshape(S * xhat.shape[0], *xhat.shape[1:])  # (the seeds stacked over the view the forward took)
        if K is not None and xhat.dtype == torch.float32:
            return K.norm_vjp(gv, xhat, rstd, None if w is None else w.contiguous(), S, G, layout).reshape(g.shape)
        return norm_vjp_math(gv, xhat, rstd, w, S, G, layout).reshape(g.shape)

    #: ``False``: attention nodes stay on the torch math (`attn_forward_math`, `attn_vjp_math`) whatever the kernel object offers
    use_attn_kernels = True
    #: what the ``[s, B, H, T, T]`` temporaries of the torch-math attention VJP may take (the seeds go through in chunks)
    attn_mem_bytes = 4 << 30

    def _attn_kernels(self, q, causal):
        """the kernel object when csrc/lk_attn.hip serves this attention node (an object with the entry points - the stock
        emulation has none -, fp32, a shape inside the kernels' contract), else ``None``: plain torch math"""
        K = self.kernels() if self.kernels is not None and self.use_attn_kernels else None
        if K is None or not hasattr(K, "attn_forward") or q.dtype != torch.float32:
            return None
        B, H, T, D = q.shape
        return K if D % 4 == 0 and K.attn_variant(1, B, H, T, D, 0, causal) is not None else None

    def _run_attn(self, r, q, k, v):
        """scaled dot-product self-attention forward -> ``(out, keep)``; what the VJP needs belongs to the sample, not to the
        seed: the operands and either ``(o, lse)`` (kernels: the probabilities are rebuilt on chip) or ``(o, p)`` (torch math)"""
        causal, scale = r.args
        if not (q.dim() == 4 and q.shape == k.shape == v.shape):
            raise SweepUnsupported(f"scaled_dot_product_attention on query {tuple(q.shape)}, key {tuple(k.shape)}, value "
                                   f"{tuple(v.shape)}: only self-attention with equal [B, H, T, D] operands (Tq == Tk) is served")
        scale = float(q.shape[-1]) ** -0.5 if scale is None else scale
        K = self._attn_kernels(q, causal)
        if K is not None:
            _, (q, k, v) = attn_operands(q, k, v)
            o, lse = K.attn_forward(q, k, v, scale, causal)
            return o, (K, q, k, v, o, lse, scale, causal)
        o, p = attn_forward_math(q, k, v, scale, causal)
        self._attn_math_numel = max(self._attn_math_numel, p.numel())
        return o, (None, q, k, v, o, p, scale, causal)

    def _attn_vjp(self, saved, g, S):
        """``(dq, dk, dv)`` for all seeds: ONE call of lk_attn_vjp_f32 (views in the operands' layout), or the same formula in
        torch; ``g`` is ``[S*B, H, T, D]``"""
        K, q, k, v, o, aux, scale, causal = saved
        if K is not None:
            return K.attn_vjp(g, q, k, v, o, aux, S, scale, causal)
        return attn_vjp_math(g, q, k, v, o, aux, S, scale, self.attn_mem_bytes)

    #: ``False``: an nn.MultiheadAttention node hands the layout-1 entry points contiguous copies of the three slices of its packed
    #: projection and concatenates the three cotangents, instead of giving the strided entry points the packed buffers themselves
    use_strided_attn = True

    def _mha_kernels(self, x, B, H, T, D):
        """the kernel object when csrc/lk_attn.hip serves the attention core of an nn.MultiheadAttention node (as `_attn_kernels`;
        a head dim that is no multiple of 4 falls to the torch math), else ``None``"""
        K = self.kernels() if self.kernels is not None and self.use_attn_kernels else None
        if K is None or not hasattr(K, "attn_forward") or x.dtype != torch.float32:
            return None
        return K if D % 4 == 0 and K.attn_variant(1, B, H, T, D, 1, False) is not None else None

    def _run_mha(self, node, r, x):
        """nn.MultiheadAttention forward as what it equals -> ``((out, None), keep)``: ``F.linear`` into ONE ``[B, T, 3 E]`` buffer,
        the attention core on its three slices where they lie (lk_attn_fwd_strided_f32; contiguous copies and the layout-1 entry
        point with ``use_strided_attn = False``; the torch math of the ATTN rule without kernels), ``F.linear``.  Fills the taps
        of both halves: ``<target>.in_proj`` reads ``x``, ``<target>.out_proj`` the attention context ``[B, T, E]``"""
        m = r.mod
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[-1] != m.embed_dim:
            raise SweepUnsupported(f"{node.target}: nn.MultiheadAttention on an input that is not [B, T, {m.embed_dim}]")
        B, T, E = x.shape
        H, D = m.num_heads, m.head_dim
        scale = float(D) ** -0.5
        b_in = None if m.in_proj_bias is None else m.in_proj_bias.detach()
        qkv = F.linear(x, m.in_proj_weight.detach(), b_in)
        K = self._mha_kernels(x, B, H, T, D) if B > 0 else None
        if K is not None and self.use_strided_attn and hasattr(K, "attn_forward_strided"):
            q, k, v = qkv.view(B, T, 3, H, D).unbind(2)  # (views: rows of E floats, 3 E apart)
            o, lse = K.attn_forward_strided(q, k, v, scale, False)
            ctx, keep = o.view(B, T, E), ("strided", K, q, k, v, o, lse, scale)
        elif K is not None:
            q, k, v = (t.contiguous().transpose(1, 2) for t in qkv.view(B, T, 3, H, D).unbind(2))  # (copies, in layout 1)
            o, lse = K.attn_forward(q, k, v, scale, False)
            ctx, keep = o.transpose(1, 2).reshape(B, T, E), ("copies", K, q, k, v, o, lse, scale)
        else:
            q, k, v = mha.heads(qkv, H)
            o, p = attn_forward_math(q, k, v, scale, False)
            self._attn_math_numel = max(self._attn_math_numel, p.numel())
            ctx, keep = o.transpose(1, 2).reshape(B, T, E), ("math", None, q, k, v, o, p, scale)
        self.max_act_numel = max(self.max_act_numel, qkv.numel() // max(B, 1))
        b_out = None if m.out_proj.bias is None else m.out_proj.bias.detach()
        out = F.linear(ctx, m.out_proj.weight.detach(), b_out)
        for half, a in (("in_proj", x), ("out_proj", ctx)):
            name = f"{node.target}.{half}"
            if name in self.tap_names:
                if name in self.taps:
                    raise SweepUnsupported(f"{name}: module is applied more than once per forward")
                self.taps[name] = {"a": a, "node": node}
        return (out, None), keep

    def _vjp_mha(self, walk, node, r, g, g2):
        """``g [S*B, T, E]``: the cotangent of the module's output, which is ``out_proj``'s tap; ``dctx = g W_out``; the attention
        VJP of all seeds straight into ONE ``[S*B, T, 3 E]`` buffer (lk_attn_vjp_strided_f32), which is ``in_proj``'s tap;
        ``dx = dqkv W_in``"""
        m, S = r.mod, walk.S
        how, K, q, k, v, o, aux, scale = self.saved[node]
        SB, T, E = g.shape
        H, D = m.num_heads, m.head_dim
        done = f"{node.target}.out_proj" in self.tap_names and walk.tap(f"{node.target}.out_proj", g.reshape(S, SB // S, T, E))
        if done:
            return
        dctx = g @ m.out_proj.weight.detach()
        if how == "strided":
            dqkv = g.new_empty(SB, T, 3 * E)
            K.attn_vjp_strided(dctx.view(SB, T, H, D), q, k, v, o, aux, S, scale, False, *dqkv.view(SB, T, 3, H, D).unbind(2))
        else:
            go = dctx.view(SB, T, H, D).transpose(1, 2)
            if how == "copies":
                parts = K.attn_vjp(go, q, k, v, o, aux, S, scale, False)
            else:
                parts = attn_vjp_math(go, q, k, v, o, aux, S, scale, self.attn_mem_bytes)
            dqkv = torch.cat([d.transpose(1, 2).reshape(SB, T, E) for d in parts], -1)
        if f"{node.target}.in_proj" in self.tap_names and walk.tap(f"{node.target}.in_proj", dqkv.reshape(S, SB // S, T, 3 * E)):
            return
        walk.push(r.src[0], dqkv @ m.in_proj_weight.detach())

    def _vjp_mhaout(self, walk, node, r, g, g2):
        walk.push(r.src[0], g)

    #: ``False``: the VJP of a product stays on the torch math of its rule (``g * b``, ``(g * a).sum(...)``) whatever the kernel
    #: object offers
    use_mul_kernels = True

    def _mul_kernels(self, ts):
        """the kernel object when csrc/lk_mul.hip serves the VJP of a product of ``ts`` (an object with the entry point - the stock
        emulation has none -, fp32), else ``None``: the same formula in torch"""
        K = self.kernels() if self.kernels is not None and self.use_mul_kernels else None
        if K is None or not hasattr(K, "mul_vjp") or not all(t.dtype == torch.float32 for t in ts):
            return None
        return K

    def _run_mul(self, r, args):
        """product forward -> ``(out, (form, a, b, gate, k))``: both operands belong to the sample, not to the seed.  ``form``:
        ``"const"`` (operand ``gate`` is a constant that broadcasts to exactly the other's shape and receives nothing), ``"full"``
        or ``"row"`` (operand ``gate`` is the other's shape with trailing ones from dim ``k``: `mul_form`)"""
        a, b = args
        if not (torch.is_tensor(a) and torch.is_tensor(b)):
            raise SweepUnsupported(f"mul: an operand is not a tensor ({type(a).__name__} * {type(b).__name__})")
        const = [self.rule[n].kind == CONST for n in r.src]
        if any(const):
            gate = const.index(True)
            c, other = (a, b) if gate == 0 else (b, a)
            if tuple(torch.broadcast_shapes(c.shape, other.shape)) != tuple(other.shape):
                raise SweepUnsupported(f"mul: {tuple(other.shape)} broadcasts against the {self.rule[r.src[gate]].what} of shape "
                                       f"{tuple(c.shape)} (the VJP needs a reduction)")
            form, k = "const", 0
        else:
            form, gate, k = mul_form(a.shape, b.shape)
        return r.fn(a, b), (form, a, b, gate, k)

    def _mul_vjp(self, saved, g, S, want):
        """``(d first, d second)`` of a product for all seeds, ``g`` ``[S*B, ...]``: ``d first = g * second`` and ``d second =
        g * first`` - summed over the trailing dims for a row gate - from ONE pair of operands per sample; an operand that is not
        in ``want`` gets ``None``.  ONE launch of lk_mul_vjp_f32 (the gate as its ``b``), or the same formula in torch; a constant
        operand is a plain torch product."""
        form, a, b, gate, k = saved
        if form == "const":
            c, other = (a, b) if gate == 0 else (b, a)
            d = (g.reshape(S, *other.shape) * c).reshape(g.shape) if want[1 - gate] else None
            return (None, d) if gate == 0 else (d, None)
        if form == "row" and gate == 0:  # (the kernel's and the formula's second operand is the gate)
            db, da = self._mul_vjp((form, b, a, 1, k), g, S, (want[1], want[0]))
            return da, db
        row = form == "row"
        K = self._mul_kernels((g, a, b))
        L = 1
        for d in a.shape[k:] if row else a.shape[1:]:
            L *= int(d)
        if K is not None and a.numel() > 0 and L < (1 << 30) and g.numel() < (1 << 40):
            return K.mul_vjp(g.contiguous(), a.contiguous(), b.contiguous(), S, row, want)
        gv = g.reshape(S, *a.shape)
        da = (gv * b).reshape(g.shape) if want[0] else None
        db = None
        if want[1]:
            db = gv * a
            db = db.sum(tuple(range(k + 1, gv.dim())), keepdim=True).reshape(S * b.shape[0], *b.shape[1:]) if row else db.reshape(g.shape)
        return da, db

    #: ``False``: the VJP of a matrix product stays on the torch math of its rule (`matmul_vjp_math`) whatever the kernel object offers
    use_matmul_kernels = True
    #: ``False``: the VJP of a softmax stays on the torch math of its rule (`softmax_vjp_math`) whatever the kernel object offers
    use_softmax_kernels = True

    def _matmul_kernels(self, g, a, b):
        """the kernel object when csrc/lk_matmul.hip serves the VJP of ``a @ b`` (an object with the entry point - the stock
        emulation has none -, fp32, a shape inside the kernel's contract), else ``None``: the same formula in torch"""
        K = self.kernels() if self.kernels is not None and self.use_matmul_kernels else None
        if K is None or not hasattr(K, "matmul_vjp") or not all(t.dtype == torch.float32 for t in (g, a, b)):
            return None
        M, Kd, N = int(a.shape[-2]), int(a.shape[-1]), int(b.shape[-1])
        if min(M, Kd, N) < 1 or a.numel() == 0:
            return None
        S = g.numel() // max(a.numel() // Kd * N, 1)
        return K if K.matmul_vjp_variant(S, a.numel() // (M * Kd), M, Kd, N) is not None else None

    def _run_matmul(self, r, args):
        """matrix product forward -> ``(out, (form, a, b, gate))``: both operands belong to the sample, not to the seed.  ``form``:
        ``"const"`` (operand ``gate`` is a constant - 2-D, or with the other's leading dims or ones there - and receives nothing)
        or ``"full"`` (two traced ``[B, *, M, K] @ [B, *, K, N]`` with equal leading dims)"""
        a, b = args
        if not (torch.is_tensor(a) and torch.is_tensor(b)):
            raise SweepUnsupported(f"matmul: an operand is not a tensor ({type(a).__name__} @ {type(b).__name__})")
        const = [self.rule[n].kind == CONST for n in r.src]
        form, gate = ("const", const.index(True)) if any(const) else ("full", None)
        t = b if gate == 0 else a  # (a traced operand)
        if t.dim() < 3 or (form == "full" and b.dim() < 3):
            raise SweepUnsupported(f"matmul of {tuple(a.shape)} and {tuple(b.shape)}: a traced operand must be [B, *, rows, columns] "
                                   "with at least three dims (a 1-D or 2-D one mixes the batch into the product: the VJP needs a reduction)")
        if form == "const":
            c = a if gate == 0 else b
            lead = tuple(c.shape[:-2])
            if c.dim() < 2 or (c.dim() > 2 and (c.dim() != t.dim() or any(d not in (1, e) for d, e in zip(lead, t.shape[:-2])))):
                raise SweepUnsupported(f"matmul: the {self.rule[r.src[gate]].what} of shape {tuple(c.shape)} must be 2-D or have the leading "
                                       f"dims of the other operand {tuple(t.shape)} (or ones there)")
        elif a.dim() != b.dim() or a.shape[:-2] != b.shape[:-2]:
            raise SweepUnsupported(f"matmul of {tuple(a.shape)} and {tuple(b.shape)}: the leading dims of two traced operands must be "
                                   "equal (where they broadcast the VJP needs a reduction)")
        try:
            out = torch.matmul(a, b)
        except RuntimeError as e:  # (inner dims that do not fit: torch's own words)
            raise SweepUnsupported(f"matmul of {tuple(a.shape)} and {tuple(b.shape)}: {e}") from e
        return out, (form, a, b, gate)

    def _matmul_vjp(self, saved, g, S, want):
        """``(d first, d second)`` of a matrix product for all seeds, ``g`` ``[S*B, *, M, N]``: ``d first = g second^T`` and
        ``d second = first^T g`` from ONE pair of operands per sample; an operand that is not in ``want`` gets ``None``.  One launch
        of lk_matmul_vjp_f32's kernel per output on ``g`` as it lies (the per-sample operands are made contiguous, 1/S of the
        work), or the same formula in torch (`matmul_vjp_math`); a constant operand is a plain torch product."""
        form, a, b, gate = saved
        if form == "const":
            t = b if gate == 0 else a
            gv = g.reshape(S, t.shape[0], *g.shape[1:])
            if gate == 0:  # (constant @ traced)
                d = (a.transpose(-1, -2) @ gv).reshape(S * t.shape[0], *t.shape[1:]) if want[1] else None
                return None, d
            d = (gv @ b.transpose(-1, -2)).reshape(S * t.shape[0], *t.shape[1:]) if want[0] else None
            return d, None
        K = self._matmul_kernels(g, a, b)
        if K is not None:
            return K.matmul_vjp(g.contiguous(), a.contiguous(), b.contiguous(), S, want)
        return matmul_vjp_math(g, a, b, S, want, self.attn_mem_bytes)

    def _softmax_kernels(self, g, y, dim):
        """the kernel object when csrc/lk_softmax.hip serves the VJP of a softmax along ``dim`` of ``y`` (an object with the entry
        point, fp32, the last dim, a shape inside the contract), else ``None``: the same formula in torch"""
        K = self.kernels() if self.kernels is not None and self.use_softmax_kernels else None
        if K is None or not hasattr(K, "softmax_vjp") or g.dtype != torch.float32 or y.dtype != torch.float32:
            return None
        if dim != y.dim() - 1 or y.numel() == 0:
            return None
        L = int(y.shape[-1])
        return K if K.softmax_vjp_variant(g.numel() // y.numel(), y.numel() // L, L) is not None else None

    def _run_softmax(self, r, inp):
        """softmax / log-softmax forward (torch's own, on the ``B`` samples) -> ``(y, (y, dim, is_log))``: the output is what the
        VJP needs, one per sample for all seeds"""
        dim, is_log = r.args
        if not torch.is_tensor(inp):
            raise SweepUnsupported(f"{r.what}: the input is not a tensor")
        dim = cat_dim(dim, inp.dim(), r.what)
        y = r.fn(inp, dim)
        return y, (y, dim, is_log)

    def _softmax_vjp(self, saved, g, S):
        """input cotangent of a softmax / log-softmax for all seeds, ``g`` ``[S*B, ...]``: ONE launch of lk_softmax_vjp_f32 when the
        dim is the last one, or the same formula in torch (`softmax_vjp_math`, any dim)"""
        y, dim, is_log = saved
        K = self._softmax_kernels(g, y, dim)
        if K is not None:
            return K.softmax_vjp(g.contiguous(), y.contiguous(), S, is_log)
        return softmax_vjp_math(g, y, S, dim, is_log, self.attn_mem_bytes)

    #: ``False``: a maximum over positions stays on the torch math of its rule (`reduce_forward_math`, `reduce_vjp_math`) whatever
    #: the kernel object offers
    use_reduce_kernels = True

    def _reduce_kernels(self, t, S, outer, L, inner):
        """the kernel object when csrc/lk_reduce.hip serves a maximum over ``L`` of ``t`` read as ``[outer, L, inner]`` (an object
        with the entry points - the stock emulation has none -, fp32, a shape inside the contract), else ``None``: the same
        formulas in torch"""
        K = self.kernels() if self.kernels is not None and self.use_reduce_kernels else None
        if K is None or not hasattr(K, "maxred_forward") or t.dtype != torch.float32 or outer == 0:
            return None
        return K if K.reduce_variant(True, S, outer, L, inner) is not None else None

    def _run_reduce(self, r, inp):
        """maximum / sum over static non-batch dims, forward -> ``(out, keep)``.  A maximum keeps what belongs to the sample, not to
        the seed: the first position of the maximum (``tie`` "first") or the input, the maximum and the number of positions that
        hold it ("even"); a sum keeps the shape only."""
        name, dims, keepdim, tie, _ = r.args
        if not torch.is_tensor(inp):
            raise SweepUnsupported(f"{r.what}: the input is not a tensor")
        dims, outer, L, inner = reduce_geometry(dims, inp.shape, r.what)
        if tie is None:
            return inp.sum(dims, keepdim=keepdim), (inp.shape, keepdim, dims)
        if dims != list(range(dims[0], dims[-1] + 1)):
            raise SweepUnsupported(f"{r.what} over the non-adjacent dims {tuple(dims)} (reduce one run of adjacent dims at a time)")
        if L == 0:
            raise SweepUnsupported(f"{r.what} over an empty dim")
        x3 = inp.contiguous().reshape(outer, L, inner)
        K = self._reduce_kernels(x3, 1, outer, L, inner)
        y, idx, cnt = K.maxred_forward(x3, outer, L, inner) if K is not None else reduce_forward_math(x3)
        shape = [1 if i in dims else int(d) for i, d in enumerate(inp.shape)] if keepdim else \
            [int(d) for i, d in enumerate(inp.shape) if i not in dims]
        return y.reshape(shape), (inp.shape, L, idx if tie == "first" else None, *((x3, y, cnt) if tie == "even" else (None,) * 3))

    def _reduce_vjp(self, saved, g, S):
        """input cotangent of a maximum over positions for all seeds, ``g`` ``[S*B, ...]``: ONE launch of lk_maxred_vjp_f32, which
        writes every element (no zero fill, no scatter), or the same formula in torch (`reduce_vjp_math`)"""
        shp, L, idx, x3, y, cnt = saved
        outer, inner = (idx if idx is not None else y).shape
        gv = g.contiguous().reshape(S, outer, inner)
        K = self._reduce_kernels(gv, S, outer, L, inner) if (idx is not None or x3.dtype == torch.float32) else None
        if K is not None:
            dx = K.maxred_vjp(gv, S, outer, L, inner, idx=idx, x=x3, y=y, cnt=cnt)
        else:
            dx = reduce_vjp_math(gv, L, idx, x3, y, cnt)
        return dx.reshape(S * shp[0], *shp[1:])

    #: ``False``: a static resampling stays on the torch math of its rule (`resample_vjp_math`: two dense matrix products)
    #: whatever the kernel object offers
    use_resample_kernels = True

    def _resample_kernels(self, g, entry, P):
        """``(kernel object, None)`` when csrc/lk_resample.hip serves the cotangent ``g`` of a resampling with the cached ``entry``
        (an object with the entry points - the stock emulation has none -, fp32, tap lists inside the kernel's cap, a shape inside
        the contract), else ``(None, why)``: the same sum in torch.  The tables are packed for the device (and validated) once."""
        tables = entry[0]
        if not self.use_resample_kernels:
            return None, "use_resample_kernels is off"
        K = self.kernels() if self.kernels is not None else None
        if K is None or not hasattr(K, "resample_vjp"):
            return None, "the kernel object has no resample_vjp"
        if g.dtype != torch.float32:
            return None, f"dtype {g.dtype}"
        if max(tables.taps) > K.RESAMPLE_MAX_TAPS:
            return None, f"{max(tables.taps)} taps per input exceed the kernel's cap of {K.RESAMPLE_MAX_TAPS}"
        (OH, H), (OW, W) = tables.Mh.shape, tables.Mw.shape
        if P < 1 or K.resample_variant(P, OH, OW, H, W, *tables.taps) is None:
            return None, "a shape outside the kernel's contract"
        if entry[1] is None:
            entry[1] = (K.resample_pack(*tables.csr_h, H, OH), K.resample_pack(*tables.csr_w, W, OW))
        return K, None

    def _run_resample(self, node, r, x, kw, need_vjp=True):
        """static resampling forward -> ``(out, (cache entry, input shape, k))``: torch's own call on the ``[B, ...]`` value (bit-equal
        to the model's); the axis matrices of the resolved geometry are derived once (`resample_tables`, which holds them against the
        operator itself: a mode that is not separable is refused by name) and cached on the sweep"""
        op, kw = r.args[0], dict(kw)
        if not torch.is_tensor(x):
            raise SweepUnsupported(f"{r.what}: the operand is not a tensor ({type(x).__name__})")
        if not x.is_floating_point():
            raise SweepUnsupported(f"{r.what}: the operand is the integer input (a resampling of token ids has no cotangent)")
        if op == "interpolate" and kw["size"] is not None:  # (values of a size(): plain ints for torch and for the cache key)
            kw["size"] = tuple(int(v) for v in kw["size"]) if isinstance(kw["size"], (tuple, list)) else int(kw["size"])
        k = resample_dims(op, kw, x.shape, r.what)
        try:
            out = r.fn(x, **kw)
        except (RuntimeError, ValueError, TypeError, NotImplementedError, AssertionError) as e:  # (torch's own words)
            raise SweepUnsupported(f"{r.what}: {e}") from e
        if out.dim() != x.dim() or tuple(out.shape[:-k]) != tuple(x.shape[:-k]):
            raise SweepUnsupported(f"{r.what}: {tuple(x.shape)} -> {tuple(out.shape)} changes more than the last {k} dims")
        if not need_vjp:
            return out, None
        in_hw = (1 if k == 1 else int(x.shape[-2]), int(x.shape[-1]))
        out_hw = (1 if k == 1 else int(out.shape[-2]), int(out.shape[-1]))
        key = (op, repr(sorted(kw.items())), in_hw, out_hw, k, x.dtype, str(x.device))
        cache = self.__dict__.setdefault("_resample_cache", {})
        entry = cache.get(key)
        if entry is None:
            tables = resample_tables(op, kw, in_hw, out_hw, k, x)
            entry = cache[key] = [tables, None]  # ([1]: the tables as the kernel object packed them)
        return out, (entry, tuple(x.shape), k)

    def _resample_vjp(self, node, saved, g, S):
        """input cotangent of a static resampling for all seeds, ``g`` ``[S*B, ...]``: ONE launch of lk_resample_vjp_f32 over the
        ``S B C`` planes, which writes every element, or ``Mh^T g Mw`` in torch (`resample_vjp_math`); both deterministic.
        ``self.resample_route[node name]`` says which one ran, and why"""
        entry, shp, k = saved
        tables = entry[0]
        (OH, H), (OW, W) = tables.Mh.shape, tables.Mw.shape
        P = g.numel() // (OH * OW)
        gv = g.contiguous().reshape(P, OH, OW)
        K, why = self._resample_kernels(gv, entry, P)
        self.__dict__.setdefault("resample_route", {})[node.name] = "kernel" if K is not None else f"torch math: {why}"
        dx = K.resample_vjp(gv, *entry[1]) if K is not None else resample_vjp_math(gv, tables.Mh, tables.Mw, S)
        return dx.reshape(g.shape[0], *shp[1:])

    def _add_const(self, r, args, kwargs):
        """``x + constant``: the constant must broadcast to exactly the other operand's shape (the other way round the VJP is
        a reduction, which has no rule)"""
        a, b = args[0], args[1]
        for n, c, other in ((r.src[0], a, b), (r.src[1], b, a)):
            if isinstance(n, fx.Node) and self.rule[n].kind == CONST and torch.is_tensor(other):
                if tuple(torch.broadcast_shapes(c.shape, other.shape)) != tuple(other.shape):
                    raise SweepUnsupported(f"add: {tuple(other.shape)} broadcasts against the {self.rule[n].what} of shape "
                                           f"{tuple(c.shape)} (the VJP needs a reduction)")
        return r.fn(*args, **kwargs)

    @staticmethod
    def _pair2(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    @staticmethod
    def _avgpool_vjp(g, in_shape, SB, kernel, stride, padding, ceil_mode=False, count_include_pad=True,
                     divisor_override=None):
        """VJP of ``avg_pool2d`` for the whole seed batch: non-overlapping, unpadded windows that tile the input are an
        upsampling; every other geometry (padding, overlap, ragged edges, ceil_mode) goes through the pooling
        operator's own backward, which needs the input only for its shape."""
        k, st = SeedBatchedSweep._pair2(kernel), SeedBatchedSweep._pair2(kernel if stride in (None, []) else stride)
        if (SeedBatchedSweep._pair2(padding) == (0, 0) and k == st and in_shape[-2] % k[0] == 0
                and in_shape[-1] % k[1] == 0 and divisor_override is None):
            return g.repeat_interleave(k[0], -2).repeat_interleave(k[1], -1) / (k[0] * k[1])
        dummy = g.new_empty((SB,) + tuple(in_shape[1:]))
        return torch.ops.aten.avg_pool2d_backward(g.contiguous(), dummy, list(k), list(st),
                                                  list(SeedBatchedSweep._pair2(padding)), bool(ceil_mode),
                                                  bool(count_include_pad), divisor_override)

    @staticmethod
    def _adaptive_avgpool_vjp(g, in_shape, SB):
        if tuple(g.shape[-2:]) == (1, 1):
            return (g / (in_shape[-1] * in_shape[-2])).expand(SB, *in_shape[1:])
        return torch.ops.aten._adaptive_avg_pool2d_backward(g.contiguous(), g.new_empty((SB,) + tuple(in_shape[1:])))

    @staticmethod
    def _maxpool_vjp(g, idx, in_shape, S, B):
        idx_s = idx.unsqueeze(0).expand(S, *idx.shape).reshape(S * B, *idx.shape[1:])
        out = torch.zeros(S * B, in_shape[1], in_shape[2] * in_shape[3], dtype=g.dtype, device=g.device)
        out.scatter_add_(2, idx_s.reshape(S * B, in_shape[1], -1), g.reshape(S * B, in_shape[1], -1))
        return out.reshape(S * B, *in_shape[1:])

    @staticmethod
    def _mean_dims(dim, ndim):
        """sorted non-batch dims a ``mean`` reduces (spatial pooling of a conv map, pooling over the positions of a
        sequence, ...); the batch dim must survive"""
        if dim is None:
            raise SweepUnsupported("mean over all dims (the batch dim included)")
        dims = sorted({d % ndim for d in (dim if isinstance(dim, (tuple, list)) else (dim,))})
        if 0 in dims:
            raise SweepUnsupported("mean over the batch dim")
        return dims

    @staticmethod
    def _mean_vjp(g, saved, SB):
        shp, keep, dims = saved
        if not keep:
            for d in dims:
                g = g.unsqueeze(d)
        count = 1
        for d in dims:
            count *= shp[d]
        return (g / count).expand(SB, *shp[1:])

    def _scaled_weight(self, name, m, scale):
        """``scale[co] * W`` for a deferred BatchNorm scale (cached until the weight or the scale changes)"""
        if scale is None:
            return m.weight
        key = (m.weight._version, m.weight.data_ptr(), id(scale))
        hit = self._w_cache.get(name)
        if hit is None or hit[0] != key:
            hit = (key, (m.weight.detach() * scale.reshape(-1, *([1] * (m.weight.dim() - 1)))).contiguous(), scale)
            self._w_cache[name] = hit
        return hit[1]

    @staticmethod
    def _conv_input_grad(in_shape, m, g, weight=None):
        """Backward-data of a convolution for the whole seed batch.  ``torch.nn.grad.conv2d_input`` hands the op a
        stride-0 dummy input, from which PyTorch infers a channels-last result that then has to be copied back to
        NCHW (20 copies of [S*B, C, H, W] per ResNet-18 step); a contiguous, never-read dummy keeps it NCHW."""
        dummy = g.new_empty(in_shape)
        return torch.ops.aten.convolution_backward(g, dummy, m.weight if weight is None else weight, None, m.stride, m.padding, m.dilation, False,
                                                   [0] * len(m.stride), m.groups, [True, False, False])[0]

    # ---- element-wise VJPs ----------------------------------------------------------------------------------
    def _bn_scale(self, name: str, m) -> torch.Tensor:
        """gamma / sqrt(running_var + eps), cached until the module's buffers change."""
        key = (m.running_var._version, None if m.weight is None else m.weight._version, m.running_var.data_ptr())
        hit = self._bn_cache.get(name)
        if hit is None or hit[0] != key:
            scale = torch.rsqrt(m.running_var + m.eps)
            if m.weight is not None:
                scale = scale * m.weight.detach()
            hit = (key, scale)
            self._bn_cache[name] = hit
        return hit[1]

    def _bn_shift(self, name: str, m) -> torch.Tensor:
        """beta - running_mean * scale (cached like the scale)"""
        key = (m.running_mean._version, m.running_var._version, None if m.weight is None else m.weight._version,
               None if m.bias is None else m.bias._version, m.running_mean.data_ptr())
        hit = self._bn_cache.get(name + "/shift")
        if hit is None or hit[0] != key:
            shift = -m.running_mean * self._bn_scale(name, m)
            if m.bias is not None:
                shift = shift + m.bias.detach()
            hit = (key, shift)
            self._bn_cache[name + "/shift"] = hit
        return hit[1]

    def _scale_mask(self, g, S, mult, scale, g2=None):
        """``(g[s] + g2[s]) * mult * scale[channel]`` for all seeds (``g``: [S*B, C, ...], ``mult``: [B, C, ...])."""
        if mult is None and scale is None:
            return g if g2 is None else g + g2
        hw = 1
        for d in g.shape[2:]:
            hw *= d
        if self.kernels is not None:
            return self.kernels().vjp_scale_mask(g.contiguous(), S, mult, scale, hw,
                                                 None if g2 is None else g2.contiguous())
        out = g if g2 is None else g + g2
        if mult is not None:
            out = (out.reshape(S, *mult.shape) * mult).reshape(g.shape)
        if scale is not None:
            out = out * scale.reshape((1, -1) + (1,) * (g.dim() - 2))
        return out

    @staticmethod
    def _act_mult(flavour, saved):
        """per-sample derivative of the activation from what the forward kept (ReLU: the mask; generic: the derivative)"""
        if flavour == "tanh":
            return 1 - saved * saved
        if flavour == "sigmoid":
            return saved * (1 - saved)
        return saved

    def _fold_bn(self, src):
        """If the activation's input is an eval-mode BatchNorm used only by it, its scale folds into the
        activation's VJP: returns (scale, node to push the cotangent to)."""
        r = self.rule.get(src)
        if r is not None and r.kind == BN and len(src.users) == 1 and src.target not in self.tap_names:
            return self._bn_scale(src.target, r.mod), r.src[0]
        # (a TAPPED BatchNorm must see ``act'(.) * g``, the cotangent of its own output, before its scale is applied:
        # the activation hands it over unscaled and the BatchNorm rule of `backward` multiplies afterwards)
        return None, src

    def _defers_scale_to(self, src, cot) -> bool:
        """may the BatchNorm reading ``src`` leave its scale to it (`backward`, ``defer_bn_scale``)?  A tapped convolution
        that feeds only this BatchNorm and has no cotangent yet."""
        r = self.rule.get(src)
        return (r is not None and r.kind == CONV and len(src.users) == 1 and src.target in self.tap_names
                and src not in cot)

    # ---- reverse sweep -----------------------------------------------------------------------------------
    @torch.no_grad()
    def backward(self, seeds: torch.Tensor, on_tap=None, defer_bn_scale: bool = False) -> dict[str, torch.Tensor]:
        """``seeds``: ``[S, B, C]`` cotangents of the output.  Returns per tapped module the gradient w.r.t.
        its output, ``[S, B, ...]`` (a view of the ``S*B``-batched cotangent).  ``on_tap(name, g)`` is called the
        moment a tapped module's gradient is complete — the accumulator uses it to start that layer's G-factor
        kernel on a side stream while the sweep goes on through the earlier layers.

        ``defer_bn_scale``: a conv whose output feeds ONLY an eval-mode BatchNorm that is not followed by an
        activation (``bn2`` / the down-sampling branch of a residual block) normally costs one full pass over the
        cotangent just to multiply by the per-channel scale ``s``.  Deferred, that pass disappears: the conv's
        backward-data uses the pre-scaled weights ``s[co] * W`` and the tap receives the UNSCALED gradient ``g`` with
        ``self.grad_scale[name] = s`` — the caller owes ``G <- diag(s) G diag(s)``, which a KFAC accumulator applies
        once per fit because ``s`` is constant."""
        walk = _Walk(self, seeds, on_tap, defer_bn_scale)
        self.grad_scale = walk.grad_scale
        S, B = walk.S, walk.B
        for node, r in reversed(self.rule.items()):
            if node not in walk.cot and node not in walk.pieces:
                continue
            parts, g2 = walk.cot.pop(node, []), None
            if node in walk.pieces:
                pcs = walk.pieces.pop(node)
                parts = [self._assemble_slices(parts, [p[:4] for p in pcs], (S * B,) + tuple(pcs[0][4][1:]))]
            g = parts[0]
            if len(parts) > 1:
                if r.kind == ACT:  # (the activation's kernel folds the residual-branch addition in)
                    g2 = _sum(parts[1:])
                else:
                    g = _sum(parts)
            if (r.mod is not None or r.kind == _PARAM) and node.target in self.tap_names:
                if node in walk.pending_scale:
                    self.grad_scale[node.target] = walk.pending_scale[node]
                if walk.tap(node.target, g.reshape(S, B, *g.shape[1:])):
                    break  # nothing upstream of the first tapped module is needed
            rule = self._vjp_rule(r)
            if rule is not None:
                rule(walk, node, r, g, g2)
        if walk.remaining:
            raise SweepUnsupported(f"no cotangent reached {sorted(walk.remaining)}")
        return walk.grads

    #: kind -> the method that pushes a node's cotangent ``g`` on to its sources, ``(walk, node, r, g, g2)`` (``g2``: the second
    #: addend of an ACT, which its kernel folds in); ``None``: a kind that has no cotangent by design.  A kind that `classify`
    #: learns and this table does not know is refused by name (`_vjp_rule`)
    _VJP = {CONV: "_vjp_conv", LINEAR: "_vjp_linear", BN: "_vjp_bn", NORM: "_vjp_norm", ACT: "_vjp_act", IDENTITY: "_vjp_identity",
            RESHAPE: "_vjp_reshape", GPOOL: "_vjp_gpool", AVGPOOL: "_vjp_avgpool", MAXPOOL: "_vjp_maxpool", MEAN: "_vjp_mean",
            ATTN: "_vjp_attn", PERMUTE: "_vjp_permute", ADD: "_vjp_add", MUL: "_vjp_mul", MATMUL: "_vjp_matmul",
            SOFTMAX: "_vjp_softmax", SCALE: "_vjp_scale", NEG: "_vjp_neg", SUB: "_vjp_sub", CAT: "_vjp_cat", SLICE: "_vjp_slice",
            _EXPAND: "_vjp_identity", _EMBED: "_vjp_leaf", _PARAM: "_vjp_leaf", _MAXRED: "_vjp_maxred", _SUMRED: "_vjp_sumred",
            _MHA: "_vjp_mha", _MHAOUT: "_vjp_mhaout", _RESAMPLE: "_vjp_resample",
            SIZE: None, GETITEM: None, SPLIT: None, CONST: None, "placeholder": None, "output": None}

    def _vjp_rule(self, r):
        """the bound method of `_VJP` for the rule ``r`` (``None``: nothing to push), or the refusal that names the operation"""
        try:
            name = self._VJP[r.kind]
        except KeyError:
            raise SweepUnsupported(f"no reverse rule for {r.what} (kind {r.kind!r})") from None
        return None if name is None else getattr(self, name)

    def _vjp_conv(self, walk, node, r, g, g2):
        in_shape = (walk.S * walk.B,) + tuple(self.saved[node][1:])
        walk.push(r.src[0], self._conv_input_grad(in_shape, r.mod, g,
                                                  self._scaled_weight(node.target, r.mod, walk.pending_scale.get(node))))

    def _vjp_linear(self, walk, node, r, g, g2):
        walk.push(r.src[0], g @ r.mod.weight)

    def _vjp_bn(self, walk, node, r, g, g2):
        src, scale = r.src[0], self._bn_scale(node.target, r.mod)
        if walk.defer_bn_scale and self._defers_scale_to(src, walk.cot):
            walk.pending_scale[src] = scale  # the conv sees the unscaled cotangent (see the docstring of `backward`)
            walk.push(src, g)
        else:
            walk.push(src, self._scale_mask(g, walk.S, None, scale))

    def _vjp_norm(self, walk, node, r, g, g2):
        walk.push(r.src[0], self._norm_vjp(r.mod, self.saved[node], g, walk.S))

    def _vjp_act(self, walk, node, r, g, g2):
        scale, dst = self._fold_bn(r.src[0])
        walk.push(dst, self._scale_mask(g, walk.S, self._act_mult(r.flavour, self.saved[node]), scale, g2))

    def _vjp_identity(self, walk, node, r, g, g2):
        walk.push(r.src[0], g)

    def _vjp_leaf(self, walk, node, r, g, g2):
        """an embedding of the integer input, a tapped parameter: the cotangent is the tap's (handed over in `backward`), the walk ends here"""

    def _vjp_reshape(self, walk, node, r, g, g2, as_map=None):
        """``as_map``: what the NHWC walk makes of a 4-D result (a feature map again)"""
        g = g.reshape((walk.S * walk.B,) + tuple(self.saved[node][1:]))
        walk.push(r.src[0], as_map(g) if as_map is not None and g.dim() == 4 else g)

    # (a 1-D pool, flavour "1d": the cotangent is lifted to the unit-height map at the node and the height squeezed out again)
    def _vjp_gpool(self, walk, node, r, g, g2):
        shp = self.saved[node]
        if r.flavour == "1d":
            d = self._adaptive_avgpool_vjp(g.unsqueeze(2), (shp[0], shp[1], 1, shp[2]), walk.S * walk.B).squeeze(2)
        else:
            d = self._adaptive_avgpool_vjp(g, shp, walk.S * walk.B)
        walk.push(r.src[0], d)

    def _vjp_avgpool(self, walk, node, r, g, g2):
        lift = r.flavour == "1d"  # (the forward kept the lifted shape)
        d = self._avgpool_vjp(g.unsqueeze(2) if lift else g, self.saved[node], walk.S * walk.B, *r.args)
        walk.push(r.src[0], d.squeeze(2) if lift else d)

    def _vjp_maxpool(self, walk, node, r, g, g2):
        idx, shp = self.saved[node]
        lift = r.flavour == "1d"
        d = self._maxpool_vjp(g.unsqueeze(2) if lift else g, idx, shp, walk.S, walk.B)
        walk.push(r.src[0], d.squeeze(2) if lift else d)

    def _vjp_maxred(self, walk, node, r, g, g2):
        walk.push(r.src[0], self._reduce_vjp(self.saved[node], g, walk.S))

    def _vjp_resample(self, walk, node, r, g, g2):
        walk.push(r.src[0], self._resample_vjp(node, self.saved[node], g, walk.S))

    def _vjp_sumred(self, walk, node, r, g, g2):
        shp, keep, dims = self.saved[node]
        if not keep:
            for d in dims:
                g = g.unsqueeze(d)
        walk.push(r.src[0], g.expand(walk.S * walk.B, *shp[1:]))

    def _vjp_mean(self, walk, node, r, g, g2):
        walk.push(r.src[0], self._mean_vjp(g, self.saved[node], walk.S * walk.B))

    def _vjp_attn(self, walk, node, r, g, g2):
        for a, d in zip(r.src, self._attn_vjp(self.saved[node], g, walk.S)):
            walk.push(a, d)

    def _vjp_permute(self, walk, node, r, g, g2):
        walk.push(r.src[0], g.permute(self.saved[node]))

    def _vjp_add(self, walk, node, r, g, g2):
        for a in r.src:
            walk.push(a, g)

    def _vjp_mul(self, walk, node, r, g, g2):
        want = tuple(walk.live(n) for n in r.src)
        if any(want):
            for a, d in zip(r.src, self._mul_vjp(self.saved[node], g, walk.S, want)):  # (`x * x`: x receives two parts)
                walk.push(a, d)

    def _vjp_matmul(self, walk, node, r, g, g2):
        want = tuple(walk.live(n) for n in r.src)
        if any(want):
            for a, d in zip(r.src, self._matmul_vjp(self.saved[node], g, walk.S, want)):  # (`x @ x^T`: x receives two parts)
                walk.push(a, d)

    def _vjp_softmax(self, walk, node, r, g, g2):
        walk.push(r.src[0], self._softmax_vjp(self.saved[node], g, walk.S))

    def _vjp_scale(self, walk, node, r, g, g2):
        walk.push(r.src[0], g / r.args[0])

    def _vjp_neg(self, walk, node, r, g, g2):
        walk.push(r.src[0], -g)

    def _vjp_sub(self, walk, node, r, g, g2):
        """the minuend receives g, the subtrahend -g; a constant, a number or the input nothing"""
        walk.push(r.src[0], g)
        if walk.live(r.src[1]):
            walk.push(r.src[1], -g)

    def _vjp_cat(self, walk, node, r, g, g2):
        dim, sizes = self.saved[node]
        off = 0
        for a, n in zip(r.src, sizes):  # (a node listed twice receives two parts)
            walk.push(a, g.narrow(dim, off, n).contiguous())
            off += n

    def _vjp_slice(self, walk, node, r, g, g2):
        dim, start, length, dropped, in_shape = self.saved[node]
        if walk.live(r.src[0]):
            walk.pieces.setdefault(r.src[0], []).append((g.unsqueeze(dim) if dropped else g, dim, start, length, in_shape))

    def release(self):
        self.saved = {}
        self.taps = {}
        self.tap_splits = {}
