"""nn.MultiheadAttention served AS the layers it equals, and the stock encoder built from it opened up for the tracer.

An unmasked self-attention ``nn.MultiheadAttention(E, H, batch_first=True)`` is exactly ``nn.Linear(E, 3E)`` with the packed
``in_proj_weight`` / ``in_proj_bias``, scaled dot-product attention on ``H`` heads of ``E / H``, and ``nn.Linear(E, E)`` with
``out_proj``'s parameters: the same function of the same parameter vector in the same order.  :func:`lift` returns that pair of
``nn.Linear`` layers; they hold the module's own ``Parameter`` objects, so a tap on them carries the real parameters' offsets and
the reference's KFAC of the two weight-sharing Linear layers is the definition of the module's factors (as `laplace_amd.conv.lift`
serves an ``nn.Conv1d`` as the ``nn.Conv2d`` it equals: no new tap kind, nothing guessed).  Whatever :func:`refusal` names is not
served and keeps the route it had.

``nn.TransformerEncoderLayer`` / ``nn.TransformerEncoder`` are leaves of ``torch.fx`` whose own ``forward`` does not trace (its
fast-path checks read tensors' properties); :func:`expand_encoders` rewrites such a ``call_module`` node into nodes for its
sub-modules, which are ``call_module`` targets of the same root.
"""
from __future__ import annotations

import operator
import weakref

import torch
import torch.fx as fx
import torch.nn.functional as F
from torch import nn

_LIFTED: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()  # nn.MultiheadAttention -> (in_proj, out_proj) (`lift`)

#: names and defaults of ``nn.MultiheadAttention.forward`` after ``query``
_CALL = (("key", "value", "key_padding_mask", "need_weights", "attn_mask", "average_attn_weights", "is_causal"),
         (None, None, None, True, None, True, False))


def _linear_view(weight, bias):
    """an ``nn.Linear`` that holds the given ``Parameter`` objects themselves"""
    lin = nn.Linear.__new__(nn.Linear)
    nn.Module.__init__(lin)
    lin.out_features, lin.in_features = int(weight.shape[0]), int(weight.shape[1])
    lin.register_parameter("weight", weight)
    lin.register_parameter("bias", bias)
    return lin


def lift(m: nn.MultiheadAttention):
    """``(in_proj, out_proj)``: the two ``nn.Linear`` layers around the attention core of ``m`` - ``Linear(E, 3E)`` on the packed
    projection, ``Linear(E, E)`` on ``out_proj``'s parameters.  Both hold the module's own ``Parameter`` objects (same ``id``,
    same storage, same ``_version``); cached weakly per module and rebuilt when the module's parameters were replaced."""
    if not isinstance(m, nn.MultiheadAttention):
        raise TypeError(f"lift: expected nn.MultiheadAttention, got {type(m).__name__}")
    why = refusal(m)
    if why is not None:
        raise NotImplementedError(why)
    hit = _LIFTED.get(m)
    if (hit is None or hit[0].weight is not m.in_proj_weight or hit[0].bias is not m.in_proj_bias
            or hit[1].weight is not m.out_proj.weight or hit[1].bias is not m.out_proj.bias):
        hit = (_linear_view(m.in_proj_weight, m.in_proj_bias), _linear_view(m.out_proj.weight, m.out_proj.bias))
        _LIFTED[m] = hit
    for lin in hit:
        lin.training = m.training
    return hit


def bind_call(args, kwargs):
    """the arguments of one call of ``nn.MultiheadAttention.forward`` by name (``query`` included)"""
    names, defaults = _CALL
    vals = dict(zip(names, defaults))
    vals["query"] = args[0] if args else kwargs.get("query")
    for n, a in zip(names, args[1:]):
        vals[n] = a
    for k, v in kwargs.items():
        if k != "query":
            if k not in vals:
                raise TypeError(f"nn.MultiheadAttention: unknown argument {k}")
            vals[k] = v
    return vals


def refusal(m, call=None, weights_used=False):
    """why the module ``m`` - or one call of it, ``call = (args, kwargs)`` as its ``forward`` receives them (tensors, or the
    nodes of a traced graph) - is not served as Linear, attention, Linear; ``None`` when it is.  ``weights_used``: something
    consumes the attention weights the call returns."""
    if not m._qkv_same_embed_dim:
        return "nn.MultiheadAttention with kdim / vdim (separate q, k, v projection weights) is not served"
    if m.bias_k is not None or m.bias_v is not None:
        return "nn.MultiheadAttention with add_bias_kv (bias_k / bias_v) is not served"
    if m.add_zero_attn:
        return "nn.MultiheadAttention with add_zero_attn is not served"
    if not m.batch_first:
        return "nn.MultiheadAttention with batch_first=False is not served"
    if m.dropout > 0 and m.training:
        return "nn.MultiheadAttention with dropout > 0 in training mode is not served"
    if call is None:
        return None
    vals = bind_call(*call)
    q, k, v = vals["query"], vals["key"], vals["value"]
    if q is None or q is not k or k is not v:
        return "nn.MultiheadAttention with query is not key or key is not value (cross-attention) is not served"
    if vals["attn_mask"] is not None:
        return "nn.MultiheadAttention with an attn_mask is not served"
    if vals["key_padding_mask"] is not None:
        return "nn.MultiheadAttention with a key_padding_mask is not served"
    if vals["is_causal"] is not False:
        return "nn.MultiheadAttention with is_causal is not served"
    if weights_used:
        return "nn.MultiheadAttention whose attention weights are consumed is not served"
    if torch.is_tensor(q) and q.dim() != 3:
        return f"nn.MultiheadAttention on an unbatched input of shape {tuple(q.shape)} is not served"
    return None


def heads(qkv, H):
    """``(q, k, v)`` ``[B, H, T, D]`` of a packed projection ``[B, T, 3 E]``: views, nothing is copied (layout 1 rows, 3 E apart)"""
    B, T, E3 = qkv.shape
    return qkv.view(B, T, 3, H, E3 // (3 * H)).permute(2, 0, 3, 1, 4).unbind(0)


def decomposed(m, x):
    """``(out, qkv, ctx)`` of the servable module ``m`` on ``x [B, T, E]`` evaluated as what it equals - ``F.linear``, scaled
    dot-product attention, ``F.linear`` - on the module's own parameters (differentiable: the autograd-tape route returns
    ``out`` as the module's output, so that the gradient edges of both halves exist); ``qkv [B, T, 3 E]``: the output of
    ``in_proj``, ``ctx [B, T, E]``: the attention context, the input of ``out_proj``"""
    B, T, E = x.shape
    qkv = F.linear(x, m.in_proj_weight, m.in_proj_bias)
    q, k, v = heads(qkv, m.num_heads)
    ctx = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, T, E)
    return F.linear(ctx, m.out_proj.weight, m.out_proj.bias), qkv, ctx


# ---- the stock encoder, opened up for the tracer -----------------------------------------------------------------------------------
ENCODERS = (nn.TransformerEncoderLayer, nn.TransformerEncoder)
_ACTIVATIONS = {F.relu: F.relu, F.gelu: F.gelu}


def _layer_call(node, names):
    """the arguments of a call of an encoder (layer) by name, or the refusal that names the argument"""
    from laplace_amd.sweep import SweepUnsupported

    what = f"{node.target}: nn.{names[0]}"
    vals = {"src": node.args[0] if node.args else node.kwargs.get("src")}
    for n, a in zip(names[1:], node.args[1:]):
        vals[n] = a
    for k, v in node.kwargs.items():
        if k != "src":
            vals[k] = v
    for n in names[1:]:
        v = vals.get(n)
        if v is not None and v is not False:
            raise SweepUnsupported(f"{what} with {n} is not served")
    unknown = set(vals) - set(names[1:]) - {"src"}
    if unknown or not isinstance(vals["src"], fx.Node):
        raise SweepUnsupported(f"{what}: unknown arguments {sorted(unknown)}")
    return vals["src"]


def _expand_layer(graph, target, layer, x):
    """nodes for the sub-modules of one nn.TransformerEncoderLayer (``target``: its path below the root) applied to the node ``x``;
    returns the node of its output"""
    from laplace_amd.sweep import SweepUnsupported

    what = f"{target}: nn.TransformerEncoderLayer"
    if not layer.self_attn.batch_first:
        raise SweepUnsupported(f"{what} with batch_first=False is not served")
    act = layer.activation
    if act not in _ACTIVATIONS:
        raise SweepUnsupported(f"{what} with the activation {getattr(act, '__name__', type(act).__name__)} is not served "
                               "(relu and gelu are, as a string or as F.relu / F.gelu)")
    if layer.training and (layer.dropout.p > 0 or layer.dropout1.p > 0 or layer.dropout2.p > 0 or layer.self_attn.dropout > 0):
        raise SweepUnsupported(f"{what} with dropout > 0 in training mode is not served")
    sub = lambda name, *args, **kw: graph.call_module(f"{target}.{name}", args, kw)  # noqa: E731

    def sa(t):
        out = sub("self_attn", t, t, t, need_weights=False)
        return sub("dropout1", graph.call_function(operator.getitem, (out, 0)))

    def ff(t):
        return sub("dropout2", sub("linear2", sub("dropout", graph.call_function(_ACTIVATIONS[act], (sub("linear1", t),)))))

    if layer.norm_first:
        x = graph.call_function(operator.add, (x, sa(sub("norm1", x))))
        return graph.call_function(operator.add, (x, ff(sub("norm2", x))))
    x = sub("norm1", graph.call_function(operator.add, (x, sa(x))))
    return sub("norm2", graph.call_function(operator.add, (x, ff(x))))


def expand_encoders(gm: fx.GraphModule) -> bool:
    """Rewrite every ``call_module`` node of ``gm`` whose target is an nn.TransformerEncoderLayer or an nn.TransformerEncoder into
    nodes for its sub-modules: ``norm1 -> self_attn -> + -> norm2 -> linear1 -> activation -> linear2 -> +`` for ``norm_first``,
    the post-norm order otherwise; an encoder becomes its layers followed by its optional final ``norm``.  What the layer's own
    forward would do otherwise (``src_mask``, ``src_key_padding_mask``, ``is_causal``, another activation callable,
    ``batch_first=False``, dropout in training mode) is refused by name.  Returns whether anything was rewritten."""
    modules, changed = dict(gm.named_modules()), False
    for node in list(gm.graph.nodes):
        m = modules.get(node.target) if node.op == "call_module" else None
        if not isinstance(m, ENCODERS):
            continue
        with gm.graph.inserting_before(node):
            if isinstance(m, nn.TransformerEncoder):
                x = _layer_call(node, ("TransformerEncoder", "mask", "src_key_padding_mask", "is_causal"))
                for i, layer in enumerate(m.layers):
                    if not isinstance(layer, nn.TransformerEncoderLayer):
                        from laplace_amd.sweep import SweepUnsupported

                        raise SweepUnsupported(f"{node.target}: nn.TransformerEncoder of {type(layer).__name__} layers is not served")
                    x = _expand_layer(gm.graph, f"{node.target}.layers.{i}", layer, x)
                if m.norm is not None:
                    x = gm.graph.call_module(f"{node.target}.norm", (x,))
            else:
                x = _expand_layer(gm.graph, node.target, m,
                                  _layer_call(node, ("TransformerEncoderLayer", "src_mask", "src_key_padding_mask", "is_causal")))
        node.replace_all_uses_with(x)
        gm.graph.erase_node(node)
        changed = True
    if changed:
        gm.graph.lint()
        gm.recompile()
    return changed
