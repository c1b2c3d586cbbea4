"""Keras functional-model JSON <-> our graph IR.

The reference ships every slice to its worker as ``model.to_json()`` and
rebuilds it with ``tf.keras.models.model_from_json`` (`src/dispatcher.py:
234-236`, `src/node.py:40,77`), and its dispatcher accepts any Keras
functional model (`src/dispatcher.py:39-53`).  This module reads that JSON
(no TensorFlow involved) into our IR so an existing Keras architecture, plus
its ``get_weights()`` list, runs on our engine unchanged; and writes our
graphs back out in the same format.

Both serialisations are understood:

* Keras 2 / tf.keras 2.x (the reference's TF 2.15): ``inbound_nodes`` is a
  list of nodes, each a list of ``[layer_name, node_index, tensor_index,
  kwargs]``; ``InputLayer`` carries ``batch_input_shape``.
* Keras 3: each node is ``{"args": [...], "kwargs": {...}}`` whose tensors
  are ``{"class_name": "__keras_tensor__", "config": {"keras_history":
  [layer, node, index]}}``; ``InputLayer`` carries ``batch_shape``.

Supported layer classes are the ones the runtime executes (graph/ir.py
OPS); anything else raises ``NotImplementedError`` naming the layer.  Only
``channels_last`` data, single-output layers and one call per layer (no
shared layers, as in the reference's `src/dag_util.py:23-25`).
"""
from __future__ import annotations

import json
from typing import Any, Dict, List, Tuple

from .ir import ACTIVATIONS, Graph, Layer, _pair, propagate_masks, with_key_masks

_BINARY = {"Multiply": "mul", "Subtract": "sub", "Maximum": "max", "Minimum": "min", "Average": "avg"}


def _inbound_names(layer: Dict[str, Any]) -> List[str]:
    nodes = layer.get("inbound_nodes") or []
    if not nodes:
        return []
    if len(nodes) > 1:
        raise NotImplementedError(f"layer {layer.get('name')!r} is called more than once (shared layer)")
    node = nodes[0]
    if isinstance(node, dict):                       # Keras 3
        names: List[str] = []

        def walk(v):
            if isinstance(v, dict):
                if v.get("class_name") == "__keras_tensor__":
                    names.append(v["config"]["keras_history"][0])
                else:
                    for x in v.values():
                        walk(x)
            elif isinstance(v, (list, tuple)):
                for x in v:
                    walk(x)
        walk(node.get("args", []))
        return names
    return [entry[0] for entry in node]               # Keras 2: [[name, node, tensor, kwargs], ...]


_MHA_ARGS = ("query", "value", "key", "attention_mask", "return_attention_scores", "training", "use_causal_mask")


def _tensor_name(v):
    """Layer name of a serialized tensor reference (Keras 2 ["name", node, tensor], Keras 3 __keras_tensor__),
    None for anything else."""
    if isinstance(v, dict) and v.get("class_name") == "__keras_tensor__":
        return v["config"]["keras_history"][0]
    if isinstance(v, (list, tuple)) and len(v) >= 3 and isinstance(v[0], str) and isinstance(v[1], int):
        return v[0]
    return None


# the attention classes whose call `_mha_inputs` parses; the grouped-query ones (Keras 3 GroupedQueryAttention and
# the project's own RotaryGroupedQueryAttention, which rotates Q and K between projection and core) read to an
# `mha` layer with `kv_heads` (and `rope`) and take one source only
_ATTENTION_CLASSES = ("MultiHeadAttention", "GroupedQueryAttention", "RotaryGroupedQueryAttention")


def _mha_inputs(layer: Dict[str, Any], name: str, cross_attention: bool,
                causal_attention: bool = False) -> Tuple[List[str], bool]:
    """The tensors a MultiHeadAttention call attends over, as the `mha` op's inputs: [query] for plain
    self-attention, [query, value] when the key is the value, else [query, value, key].  Keras 2 keeps `value` /
    `key` in the first inbound entry's kwargs, Keras 3 in the node's "kwargs" (or all of them in "args"); no mask,
    no scores returned.  Without `cross_attention` a call whose three tensors are not one is refused by layer
    name, as it was before the `mha` op took separate sources.  Also returned: whether the call sets
    `use_causal_mask` (Keras 2 kwargs, Keras 3 "args" / "kwargs"), which is read under `causal_attention` only, and
    only for one source: by default it is refused by layer name, as it always was."""
    nodes = layer.get("inbound_nodes") or []
    if len(nodes) != 1:
        raise NotImplementedError(f"layer {name!r} is called {len(nodes)} times (one call per layer)")
    node = nodes[0]
    if isinstance(node, dict):                       # Keras 3
        args, kwargs = list(node.get("args", [])), dict(node.get("kwargs", {}))
    else:                                            # Keras 2
        args, kwargs = [list(e[:3]) for e in node], {}
        for e in node:
            if len(e) > 3 and isinstance(e[3], dict):
                kwargs.update(e[3])
    call = dict(zip(_MHA_ARGS, args))
    call.update(kwargs)
    q, v = _tensor_name(call.get("query")), _tensor_name(call.get("value"))
    k = _tensor_name(call.get("key")) if call.get("key") is not None else v
    if q is None or v is None or k is None:
        raise NotImplementedError(f"{name}: MultiHeadAttention call without a query and a value tensor")
    cls = layer.get("class_name", "MultiHeadAttention")
    if not q == v == k and cls != "MultiHeadAttention":
        raise NotImplementedError(f"{name}: {cls} on separate sources (query {q!r}, value {v!r}, key {k!r}); only "
                                  f"self-attention is built for grouped-query attention")
    if not q == v == k and not cross_attention:
        raise NotImplementedError(f"{name}: cross-attention (query {q!r}, value {v!r}, key {k!r}); "
                                  f"from_keras_json(..., cross_attention=True) reads it")
    if call.get("attention_mask") is not None:
        raise NotImplementedError(f"{name}: MultiHeadAttention with an attention_mask")
    causal = bool(call.get("use_causal_mask"))
    if causal and not causal_attention:
        raise NotImplementedError(f"{name}: MultiHeadAttention with use_causal_mask; "
                                  f"from_keras_json(..., causal_attention=True) reads it")
    if causal and not q == v == k:
        raise NotImplementedError(f"{name}: MultiHeadAttention with use_causal_mask on separate sources (query "
                                  f"{q!r}, value {v!r}, key {k!r}); only self-attention takes the causal mask")
    if call.get("return_attention_scores"):
        raise NotImplementedError(f"{name}: MultiHeadAttention with return_attention_scores")
    if q == v == k:
        return [q], causal
    return ([q, v] if k == v else [q, v, k]), causal


def _check_mha(cfg: Dict[str, Any], in_shape: Tuple[int, ...], name: str, cls: str = "MultiHeadAttention") -> None:
    """What the config may ask for beyond the defaults: attention over all position axes, and an output as
    wide as the input (`in_shape` is per image)."""
    rank = len(in_shape) + 1                          # with the batch axis, as Keras counts
    axes = cfg.get("attention_axes")
    if axes is not None:
        axes = [axes] if isinstance(axes, int) else list(axes)
        if sorted(a + rank if a < 0 else a for a in axes) != list(range(1, rank - 1)):
            raise NotImplementedError(f"{name}: {cls} attention_axes={cfg['attention_axes']} (only all "
                                      f"position axes)")
    osh = cfg.get("output_shape")
    if osh is not None and (list(osh) if isinstance(osh, (list, tuple)) else [osh]) != [in_shape[-1]]:
        raise NotImplementedError(f"{name}: {cls} output_shape={osh} (only the input's "
                                  f"{in_shape[-1]} channels)")


def _padding2d(p) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    if isinstance(p, int):
        return ((p, p), (p, p))
    a, b = p
    if isinstance(a, int):
        return ((a, a), (b, b))
    return ((int(a[0]), int(a[1])), (int(b[0]), int(b[1])))


def _stride(cfg: Dict[str, Any], name: str) -> int:
    sh, sw = _pair(cfg.get("strides", 1))
    if sh != sw:
        raise NotImplementedError(f"{name}: unequal strides {sh}x{sw}")
    return sh


def _check_channels_last(cfg: Dict[str, Any], name: str) -> None:
    if cfg.get("data_format", "channels_last") not in (None, "channels_last"):
        raise NotImplementedError(f"{name}: data_format {cfg['data_format']!r}")


def _activation(act, name: str):
    """A Keras activation config (a name, or a serialized function in Keras 3) -> our name."""
    if isinstance(act, dict):
        act = act.get("config", {}).get("name", act.get("class_name"))
    if act in (None, "linear"):
        return None
    if act in ("gelu_new", "gelu_approximate"):        # the tanh form under its other names
        act = "gelu_tanh"
    if act not in ACTIVATIONS and act != "softmax":
        raise NotImplementedError(f"{name}: activation {act!r}")
    return act


def _check_last_axis(axis, rank: int, name: str, cls: str = "LayerNormalization") -> None:
    """LayerNormalization (and RMSNormalization) normalises the last axis only: -1, [-1], or that axis given
    positively (`rank` counts the batch axis: [3] for NHWC, [1] for a (batch, C) input)."""
    ax = list(axis) if isinstance(axis, (list, tuple)) else [axis]
    if len(ax) != 1 or ax[0] not in (-1, rank - 1):
        raise NotImplementedError(f"{name}: {cls} over axis {axis} (only the last axis is supported)")


def _layers_from_keras(cls: str, cfg: Dict[str, Any], name: str, inputs: List[str]) -> List[Layer]:
    """Most classes map to one IR layer; SeparableConv2D lowers to a depthwise + a pointwise conv (same
    get_weights() order: depthwise_kernel, pointwise_kernel, bias), the pointwise one keeping the Keras name."""
    if cls == "SeparableConv2D":
        _check_channels_last(cfg, name)
        if int(cfg.get("depth_multiplier", 1)) != 1 or _pair(cfg.get("dilation_rate", 1)) != (1, 1):
            raise NotImplementedError(f"{name}: SeparableConv2D with depth_multiplier / dilation")
        dw = Layer(f"{name}/depthwise", "dwconv", inputs,
                   {"kernel": _pair(cfg["kernel_size"]), "stride": _stride(cfg, name),
                    "padding": cfg.get("padding", "valid"), "use_bias": False})
        a = {"filters": int(cfg["filters"]), "kernel": (1, 1), "stride": 1, "padding": "valid",
             "use_bias": bool(cfg.get("use_bias", True))}
        act = _activation(cfg.get("activation"), name)
        if act:
            a["activation"] = act
        return [dw, Layer(name, "conv", [dw.name], a)]
    return [_layer_from_keras(cls, cfg, name, inputs)]


def _gelu_form(act, cfg: Dict[str, Any]):
    """`gelu` with `approximate: true` in the layer's config (or in a Keras 3 serialized activation's) is the
    tanh form."""
    approx = cfg.get("approximate")
    src = cfg.get("activation")
    if isinstance(src, dict) and isinstance(src.get("config"), dict):
        approx = approx or src["config"].get("approximate")
    return "gelu_tanh" if act == "gelu" and approx else act


def _layer_from_keras(cls: str, cfg: Dict[str, Any], name: str, inputs: List[str]) -> Layer:
    if cls == "InputLayer":
        shp = cfg.get("batch_input_shape") or cfg.get("batch_shape")
        return Layer(name, "input", [], {"shape": tuple(int(d) for d in shp[1:])})
    _check_channels_last(cfg, name)
    if cls == "ZeroPadding2D":
        return Layer(name, "zeropad", inputs, {"pad": _padding2d(cfg["padding"])})
    if cls in ("Conv2D", "DepthwiseConv2D"):
        if _pair(cfg.get("dilation_rate", 1)) != (1, 1):
            raise NotImplementedError(f"{name}: dilated convolution (dilation_rate={cfg['dilation_rate']})")
        a = {"kernel": _pair(cfg["kernel_size"]), "stride": _stride(cfg, name),
             "padding": cfg.get("padding", "valid"), "use_bias": bool(cfg.get("use_bias", True))}
        act = _activation(cfg.get("activation", "linear"), name)
        if act == "softmax":
            raise NotImplementedError(f"{name}: softmax on a convolution")
        if act:
            a["activation"] = act
        if cls == "Conv2D":
            a["filters"] = int(cfg["filters"])
            if int(cfg.get("groups", 1) or 1) != 1:     # the attr exists on grouped convs only
                a["groups"] = int(cfg["groups"])
            return Layer(name, "conv", inputs, a)
        if int(cfg.get("depth_multiplier", 1)) != 1:
            raise NotImplementedError(f"{name}: depth_multiplier != 1")
        return Layer(name, "dwconv", inputs, a)
    if cls == "Conv2DTranspose":
        if cfg.get("output_padding") is not None:
            raise NotImplementedError(f"{name}: Conv2DTranspose with output_padding={cfg['output_padding']}")
        if _pair(cfg.get("dilation_rate", 1)) != (1, 1):
            raise NotImplementedError(f"{name}: dilated transposed convolution "
                                      f"(dilation_rate={cfg['dilation_rate']})")
        a = {"filters": int(cfg["filters"]), "kernel": _pair(cfg["kernel_size"]), "stride": _stride(cfg, name),
             "padding": cfg.get("padding", "valid"), "use_bias": bool(cfg.get("use_bias", True))}
        act = _activation(cfg.get("activation", "linear"), name)
        if act == "softmax":
            raise NotImplementedError(f"{name}: softmax on a convolution")
        if act:
            a["activation"] = act
        return Layer(name, "deconv", inputs, a)
    if cls == "UpSampling2D":
        interp = cfg.get("interpolation", "nearest")
        if interp not in ("nearest", "bilinear"):
            raise NotImplementedError(f"{name}: UpSampling2D interpolation {interp!r}")
        return Layer(name, "upsample", inputs, {"size": _pair(cfg.get("size", 2)), "interpolation": interp})
    if cls == "Cropping2D":
        return Layer(name, "crop", inputs, {"crop": _padding2d(cfg.get("cropping", 0))})
    if cls == "BatchNormalization":
        axis = cfg.get("axis", -1)
        axis = axis[0] if isinstance(axis, list) else axis
        if axis not in (-1, 3):
            raise NotImplementedError(f"{name}: BatchNormalization needs axis=-1")
        a = {"epsilon": float(cfg.get("epsilon", 1e-3))}
        for k in ("center", "scale"):
            if not cfg.get(k, True):
                a[k] = False
        return Layer(name, "bn", inputs, a)
    if cls == "LayerNormalization":
        # the axis is checked against the input's rank where that is known (from_keras_json)
        a = {"epsilon": float(cfg.get("epsilon", 1e-3))}
        for k in ("center", "scale"):
            if not cfg.get(k, True):
                a[k] = False
        return Layer(name, "layernorm", inputs, a)
    if cls == "RMSNormalization":                      # Keras 3; the axis is checked in from_keras_json
        a = {"epsilon": float(cfg.get("epsilon", 1e-6))}
        if not cfg.get("scale", True):
            a["scale"] = False
        return Layer(name, "rmsnorm", inputs, a)
    if cls in ("GroupedQueryAttention", "RotaryGroupedQueryAttention"):
        # kv_heads is always stored, also when it equals num_heads: the writer then emits the class it read
        a = {"num_heads": int(cfg["num_query_heads"]), "key_dim": int(cfg["head_dim"]),
             "kv_heads": int(cfg["num_key_value_heads"]), "use_bias": bool(cfg.get("use_bias", True))}
        if a["kv_heads"] < 1 or a["num_heads"] % a["kv_heads"]:
            raise NotImplementedError(f"{name}: {cls} with num_query_heads={a['num_heads']} not a multiple of "
                                      f"num_key_value_heads={a['kv_heads']}")
        if cls == "RotaryGroupedQueryAttention":       # frequency scaling is not built
            a["rope"] = float(cfg.get("rope_max_wavelength", 10000.0))
            if a["key_dim"] % 2:
                raise NotImplementedError(f"{name}: {cls} with an odd head_dim={a['key_dim']} (the rotation pairs "
                                          f"channel i with i + head_dim / 2)")
            if cfg.get("rope_scaling_factor") not in (None, 1, 1.0):
                raise NotImplementedError(f"{name}: {cls} with rope_scaling_factor={cfg['rope_scaling_factor']} "
                                          f"(frequency scaling is not built)")
        return Layer(name, "mha", inputs, a)
    if cls == "GroupNormalization":
        axis = cfg.get("axis", -1)
        axis = axis[0] if isinstance(axis, (list, tuple)) and len(axis) == 1 else axis
        if axis not in (-1, 3):
            raise NotImplementedError(f"{name}: GroupNormalization over axis {cfg.get('axis')} (only the channel "
                                      f"axis of an (H, W, C) map, -1 or 3, is supported)")
        a = {"groups": int(cfg.get("groups", 32)), "epsilon": float(cfg.get("epsilon", 1e-3))}
        for k in ("center", "scale"):
            if not cfg.get(k, True):
                a[k] = False
        return Layer(name, "groupnorm", inputs, a)
    if cls == "MultiHeadAttention":
        # the call (its query / value / key tensors) and attention_axes / output_shape are checked in from_keras_json
        a = {"num_heads": int(cfg["num_heads"]), "key_dim": int(cfg["key_dim"]),
             "use_bias": bool(cfg.get("use_bias", True))}
        if cfg.get("value_dim") is not None and int(cfg["value_dim"]) != a["key_dim"]:
            a["value_dim"] = int(cfg["value_dim"])
        return Layer(name, "mha", inputs, a)
    if cls == "WindowAttention":                       # the project's own layer (graph/ir.py "winattn")
        return Layer(name, "winattn", inputs,
                     {"num_heads": int(cfg["num_heads"]), "key_dim": int(cfg["key_dim"]),
                      "window": int(cfg["window_size"]), "shift": int(cfg.get("shift_size", 0)),
                      "use_bias": bool(cfg.get("use_bias", True))})
    if cls == "SpaceToDepth":                          # the project's own layer (graph/ir.py "space_to_depth")
        return Layer(name, "space_to_depth", inputs, {"block": int(cfg.get("block_size", 2))})
    if cls == "ClassTokenPositionEmbedding":           # the project's own layer (graph/ir.py "posembed")
        return Layer(name, "posembed", inputs, {"class_token": bool(cfg.get("class_token", True))})
    if cls == "LearnedQueries":                        # the project's own layer (graph/ir.py "queries")
        return Layer(name, "queries", inputs, {"length": int(cfg["length"]), "dim": int(cfg["dim"]),
                                               "initializer": str(cfg.get("initializer", "normal"))})
    if cls == "Embedding":
        a = {"input_dim": int(cfg["input_dim"]), "output_dim": int(cfg["output_dim"])}
        if cfg.get("mask_zero"):                       # from_keras_json refuses it unless asked (padding_mask=True)
            a["mask_zero"] = True
        return Layer(name, "embedding", inputs, a)
    if cls == "LayerScale":
        return Layer(name, "layerscale", inputs, {"init_values": float(cfg.get("init_values", 1e-6))})
    if cls == "StochasticDepth":                       # drops whole residual branches in training only
        return Layer(name, "identity", inputs)
    if cls == "ReLU":
        if float(cfg.get("threshold", 0.0) or 0.0) != 0.0:
            raise NotImplementedError(f"{name}: thresholded ReLU")
        mv = cfg.get("max_value")
        slope = float(cfg.get("negative_slope", 0.0) or 0.0)
        if slope:
            if mv is not None:
                raise NotImplementedError(f"{name}: ReLU with both max_value and negative_slope")
            return Layer(name, "act", inputs, {"fn": "leaky_relu", "alpha": slope})
        if mv is not None and float(mv) != 6.0:
            raise NotImplementedError(f"{name}: ReLU(max_value={mv})")
        return Layer(name, "relu", inputs, {"max_value": float(mv)} if mv is not None else {})
    if cls == "LeakyReLU":
        alpha = cfg.get("alpha", cfg.get("negative_slope", 0.3))
        return Layer(name, "act", inputs, {"fn": "leaky_relu", "alpha": float(alpha)})
    if cls == "Activation":
        act = _gelu_form(_activation(cfg["activation"], name), cfg)
        if act is None:
            return Layer(name, "identity", inputs)
        if act == "relu":
            return Layer(name, "relu", inputs)
        if act == "softmax":
            return Layer(name, "softmax", inputs)
        return Layer(name, "act", inputs, {"fn": act})
    if cls in _BINARY:
        if len(inputs) != 2:
            raise NotImplementedError(f"{name}: {cls} of {len(inputs)} inputs")
        return Layer(name, "binary", inputs, {"fn": _BINARY[cls]})
    if cls == "GlobalMaxPooling2D":
        return Layer(name, "gmp", inputs, {"keepdims": True} if cfg.get("keepdims") else {})
    if cls == "Reshape":
        return Layer(name, "reshape", inputs, {"shape": tuple(int(d) for d in cfg["target_shape"])})
    if cls == "Rescaling":
        return Layer(name, "rescale", inputs, {"scale": cfg.get("scale", 1.0), "offset": cfg.get("offset", 0.0)})
    if cls == "Normalization":
        axis = cfg.get("axis", -1)
        axis = axis[0] if isinstance(axis, list) and len(axis) == 1 else axis
        if axis not in (-1, 3) or cfg.get("invert"):
            raise NotImplementedError(f"{name}: Normalization needs axis=-1")
        return Layer(name, "normalization", inputs)
    if cls == "Softmax":
        return Layer(name, "softmax", inputs)
    if cls == "Add":
        return Layer(name, "add", inputs)
    if cls == "Concatenate":
        if cfg.get("axis", -1) not in (-1, 3):
            raise NotImplementedError(f"{name}: concat axis {cfg.get('axis')}")
        return Layer(name, "concat", inputs)
    if cls in ("MaxPooling2D", "AveragePooling2D"):
        pool = _pair(cfg.get("pool_size", 2))
        strides = cfg.get("strides") or cfg.get("pool_size", 2)
        sh, sw = _pair(strides)
        if sh != sw:
            raise NotImplementedError(f"{name}: unequal pooling strides")
        return Layer(name, "maxpool" if cls == "MaxPooling2D" else "avgpool", inputs,
                     {"pool": pool if pool[0] != pool[1] else pool[0], "stride": sh,
                      "padding": cfg.get("padding", "valid")})
    if cls == "GlobalAveragePooling2D":
        return Layer(name, "gap", inputs, {"keepdims": True} if cfg.get("keepdims") else {})
    if cls == "Flatten":
        return Layer(name, "flatten", inputs)
    if cls in ("Dropout", "SpatialDropout2D", "GaussianDropout", "GaussianNoise", "ActivityRegularization"):
        return Layer(name, "identity", inputs)
    if cls == "Dense":
        act = _gelu_form(_activation(cfg.get("activation", "linear"), name), cfg)
        a = {"units": int(cfg["units"]), "use_bias": bool(cfg.get("use_bias", True))}
        if act:
            a["activation"] = act
        return Layer(name, "dense", inputs, a)
    raise NotImplementedError(f"layer {name!r}: Keras class {cls!r} is not supported by the runtime")


def from_keras_json(s, cross_attention: bool = False, causal_attention: bool = False,
                    padding_mask: bool = False) -> Graph:
    """Parse ``model.to_json()`` output (str or already-decoded dict) into a Graph.  `cross_attention=True` reads a
    MultiHeadAttention call whose query, value and key are different tensors (the `mha` op's two- and three-input
    forms); by default such a call is refused by layer name, which is what this function has always done and what
    callers written against it may rely on.  `causal_attention=True` likewise reads a self-attention call with
    `use_causal_mask=True` (the `mha` op's `causal` attribute), refused by layer name by default.
    `padding_mask=True` reads `Embedding(mask_zero=True)`, refused by layer name by default, and propagates its
    mask as Keras does implicitly (graph/ir.py `propagate_masks`): every self-attention layer it reaches gets
    `key_mask` and the ids tensor as its last input.  Outputs at kept positions are Keras'; at padded positions
    they are defined but not Keras' (a padded query's context row is zeros, graph/ir.py "mha").
    `Model.from_keras_json`, and through it the command line, pass True for all three."""
    d = json.loads(s) if isinstance(s, (str, bytes)) else s
    if d.get("class_name") not in ("Functional", "Model"):
        raise NotImplementedError(f"only functional models are supported (got {d.get('class_name')!r})")
    cfg = d["config"]
    g = Graph(cfg.get("name", "model"))
    for ld in cfg["layers"]:
        name = ld.get("name") or ld["config"]["name"]
        mha = ld["class_name"] in _ATTENTION_CLASSES
        inputs, causal = (_mha_inputs(ld, name, cross_attention, causal_attention) if mha
                          else (_inbound_names(ld), False))
        if mha:
            for i in inputs:
                if i not in g.layers:
                    raise ValueError(f"layer {name!r} consumes unknown tensor {i!r}")
            _check_mha(ld["config"], g.layers[inputs[0]].out_shape, name, ld["class_name"])      # against the query
        if ld["class_name"] == "Embedding":
            shp = g.layers[inputs[0]].out_shape if len(inputs) == 1 and inputs[0] in g.layers else None
            il = ld["config"].get("input_length")
            il = il[0] if isinstance(il, (list, tuple)) and len(il) == 1 else il
            if shp is not None and il is not None and (len(shp) != 1 or int(il) != shp[0]):
                raise NotImplementedError(f"{name}: Embedding input_length={ld['config']['input_length']} does not "
                                          f"match its input {tuple(shp)}")
            if ld["config"].get("mask_zero") and not padding_mask:
                raise NotImplementedError(f"{name}: Embedding with mask_zero=True (masks are not propagated); "
                                          f"from_keras_json(..., padding_mask=True) reads it")
        for layer in _layers_from_keras(ld["class_name"], ld["config"], name, inputs):
            if causal:
                layer.attrs["causal"] = True
            g.add(layer)
        if ld["class_name"] in ("LayerNormalization", "RMSNormalization"):
            _check_last_axis(ld["config"].get("axis", -1), len(g.layers[name].out_shape) + 1, name,
                             ld["class_name"])

    def names(v) -> List[str]:
        if isinstance(v, list) and v and isinstance(v[0], str):
            return [v[0]]                                   # a single [name, node, tensor]
        return [e[0] for e in v]
    g.input_names = names(cfg["input_layers"])
    g.output_names = names(cfg["output_layers"])
    return with_key_masks(g) if padding_mask else g


# ------------------------------------------------------------------ export
def _keras_layer(L: Layer, g: Graph) -> Dict[str, Any]:
    a = L.attrs
    cfg: Dict[str, Any] = {"name": L.name, "trainable": True, "dtype": "float32"}
    if L.op == "input":
        cls = "InputLayer"
        cfg = {"batch_input_shape": [None] + list(a["shape"]), "dtype": "float32", "sparse": False,
               "ragged": False, "name": L.name}
    elif L.op == "zeropad":
        cls = "ZeroPadding2D"
        cfg.update(padding=[list(p) for p in a["pad"]], data_format="channels_last")
    elif L.op in ("conv", "dwconv"):
        cls = "Conv2D" if L.op == "conv" else "DepthwiseConv2D"
        cfg.update(kernel_size=list(_pair(a["kernel"])), strides=[a.get("stride", 1)] * 2,
                   padding=a.get("padding", "valid"), data_format="channels_last", dilation_rate=[1, 1],
                   activation=a.get("activation") or "linear", use_bias=a.get("use_bias", True))
        if L.op == "conv":
            cfg.update(filters=a["filters"], groups=a.get("groups", 1))
        else:
            cfg.update(depth_multiplier=1)
    elif L.op == "deconv":
        cls = "Conv2DTranspose"
        cfg.update(filters=a["filters"], kernel_size=list(_pair(a["kernel"])), strides=[a.get("stride", 1)] * 2,
                   padding=a.get("padding", "valid"), data_format="channels_last", dilation_rate=[1, 1],
                   output_padding=None, activation=a.get("activation") or "linear",
                   use_bias=a.get("use_bias", True))
    elif L.op == "upsample":
        cls = "UpSampling2D"
        cfg.update(size=list(a["size"]), data_format="channels_last", interpolation=a.get("interpolation", "nearest"))
    elif L.op == "crop":
        cls = "Cropping2D"
        cfg.update(cropping=[list(p) for p in a["crop"]], data_format="channels_last")
    elif L.op == "bn":
        cls = "BatchNormalization"
        cfg.update(axis=[3], momentum=0.99, epsilon=a.get("epsilon", 1e-3), center=a.get("center", True),
                   scale=a.get("scale", True))
    elif L.op == "layernorm":
        cls = "LayerNormalization"
        cfg.update(axis=[-1], epsilon=a.get("epsilon", 1e-3), center=a.get("center", True),
                   scale=a.get("scale", True))
    elif L.op == "groupnorm":
        cls = "GroupNormalization"
        cfg.update(groups=a["groups"], axis=-1, epsilon=a.get("epsilon", 1e-3), center=a.get("center", True),
                   scale=a.get("scale", True))
    elif L.op == "rmsnorm":
        cls = "RMSNormalization"
        cfg.update(axis=-1, epsilon=a.get("epsilon", 1e-6), scale=a.get("scale", True))
    elif L.op == "mha" and ("kv_heads" in a or "rope" in a):
        if a.get("value_dim") not in (None, a["key_dim"]):
            raise NotImplementedError(f"mha {L.name!r}: GroupedQueryAttention has one head_dim; value_dim="
                                      f"{a['value_dim']} != key_dim={a['key_dim']} cannot be written")
        cls = "RotaryGroupedQueryAttention" if "rope" in a else "GroupedQueryAttention"
        cfg.update(head_dim=a["key_dim"], num_query_heads=a["num_heads"],
                   num_key_value_heads=a.get("kv_heads", a["num_heads"]), dropout=0.0,
                   use_bias=a.get("use_bias", True))
        if "rope" in a:
            cfg.update(rope_max_wavelength=float(a["rope"]))
    elif L.op == "mha":
        cls = "MultiHeadAttention"
        cfg.update(num_heads=a["num_heads"], key_dim=a["key_dim"], value_dim=a.get("value_dim") or a["key_dim"],
                   dropout=0.0, use_bias=a.get("use_bias", True), output_shape=None, attention_axes=None)
    elif L.op == "winattn":
        cls = "WindowAttention"
        cfg.update(num_heads=a["num_heads"], key_dim=a["key_dim"], window_size=a["window"],
                   shift_size=a.get("shift", 0), use_bias=a.get("use_bias", True))
    elif L.op == "space_to_depth":
        cls = "SpaceToDepth"
        cfg.update(block_size=a.get("block", 2))
    elif L.op == "posembed":
        cls = "ClassTokenPositionEmbedding"
        cfg.update(class_token=bool(a.get("class_token")))
    elif L.op == "embedding":
        cls = "Embedding"
        cfg.update(input_dim=a["input_dim"], output_dim=a["output_dim"], mask_zero=bool(a.get("mask_zero")),
                   input_length=g.layers[L.inputs[0]].out_shape[0])
    elif L.op == "queries":
        cls = "LearnedQueries"
        cfg.update(length=a["length"], dim=a["dim"], initializer=a.get("initializer", "normal"))
    elif L.op == "layerscale":
        cls = "LayerScale"
        cfg.update(init_values=a.get("init_values", 1e-6), projection_dim=L.out_shape[-1])
    elif L.op == "relu":
        if a.get("max_value") is None:
            cls = "Activation"
            cfg.update(activation="relu")
        else:
            cls = "ReLU"
            cfg.update(max_value=a["max_value"], negative_slope=0.0, threshold=0.0)
    elif L.op == "add":
        cls = "Add"
    elif L.op == "concat":
        cls = "Concatenate"
        cfg.update(axis=-1)
    elif L.op in ("maxpool", "avgpool"):
        cls = "MaxPooling2D" if L.op == "maxpool" else "AveragePooling2D"
        cfg.update(pool_size=list(_pair(a["pool"])), strides=[a["stride"]] * 2, padding=a.get("padding", "valid"),
                   data_format="channels_last")
    elif L.op in ("gap", "gmp"):
        cls = "GlobalAveragePooling2D" if L.op == "gap" else "GlobalMaxPooling2D"
        cfg.update(data_format="channels_last", keepdims=bool(a.get("keepdims", False)))
    elif L.op == "act":
        if a["fn"] == "leaky_relu":
            cls = "LeakyReLU"
            cfg.update(alpha=a.get("alpha", 0.3))
        else:
            cls = "Activation"
            cfg.update(activation=a["fn"])
    elif L.op == "binary":
        cls = {v: k for k, v in _BINARY.items()}[a["fn"]]
    elif L.op == "reshape":
        cls = "Reshape"
        cfg.update(target_shape=list(a["shape"]))
    elif L.op == "rescale":
        cls = "Rescaling"
        cfg.update(scale=a.get("scale", 1.0), offset=a.get("offset", 0.0))
    elif L.op == "normalization":
        cls = "Normalization"
        cfg.update(axis=[-1], invert=False)
    elif L.op == "flatten":
        cls = "Flatten"
        cfg.update(data_format="channels_last")
    elif L.op == "identity":
        cls = "Activation"
        cfg.update(activation="linear")
    elif L.op == "dense":
        cls = "Dense"
        cfg.update(units=a["units"], activation=a.get("activation") or "linear", use_bias=a.get("use_bias", True))
    elif L.op == "softmax":
        cls = "Activation"
        cfg.update(activation="softmax")
    else:
        raise NotImplementedError(L.op)
    inbound = [[[i, 0, 0, {}] for i in L.inputs]] if L.inputs else []
    if L.op == "mha":           # Keras 2: mha(q, v[, key=k]) keeps `value` (and `key`) in the entry's kwargs
        src = L.inputs[:-1] if a.get("key_mask") else L.inputs      # Keras propagates the padding mask itself
        kw = {"value": [src[1] if len(src) > 1 else src[0], 0, 0]}
        if len(src) > 2:
            kw["key"] = [src[2], 0, 0]
        if a.get("causal"):
            kw["use_causal_mask"] = True
        inbound = [[[L.inputs[0], 0, 0, kw]]]
    return {"class_name": cls, "config": cfg, "name": L.name, "inbound_nodes": inbound}


def to_keras_json(g: Graph) -> str:
    """Our graph as Keras 2 functional-model JSON (``model.to_json()`` layout).  Keras propagates a padding mask
    implicitly, so an `mha` call is written without its `key_mask` input; the explicit edges must therefore be
    exactly what `propagate_masks` re-derives from the Embedding layers, else the document would not mean the
    graph and the layer is refused by name."""
    derived = propagate_masks(g)
    for n in g.order:
        L = g.layers[n]
        have = L.inputs[-1] if L.op == "mha" and L.attrs.get("key_mask") else None
        if have != derived.get(n):
            raise NotImplementedError(f"mha {n!r}: its key_mask input is {have!r} but the padding masks of the "
                                      f"graph's Embedding layers give {derived.get(n)!r}; Keras JSON cannot say "
                                      f"that")
    layers = [_keras_layer(g.layers[n], g) for n in g.order]
    outs = g.output_names or [g.order[-1]]
    return json.dumps({"class_name": "Functional",
                       "config": {"name": g.name, "trainable": True, "layers": layers,
                                  "input_layers": [[n, 0, 0] for n in g.input_names],
                                  "output_layers": [[n, 0, 0] for n in outs]},
                       "keras_version": "2.15.0", "backend": "tensorflow"})
