"""Named-layer graph IR.

The reference cuts a Keras functional graph at named layers
(`src/dag_util.py:3-62`, `src/dispatcher.py:39-53`).  We do not depend on
Keras: models are described by this small IR whose layer names, layer order
and per-layer weight lists are byte-identical to the Keras
`applications.resnet` graphs, so `part_at` lists and Keras `get_weights()`
lists port over 1:1.

Shapes are per-image NHWC (``(H, W, C)``) or ``(C,)``; the batch dimension is
implicit.  Layers are stored in Keras creation order, which is a valid
topological order.
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

# op kinds understood by the runtime
OPS = (
    "input",      # graph input, attrs: shape
    "zeropad",    # attrs: pad=((t,b),(l,r))
    "conv",       # attrs: filters, kernel=(kh,kw), stride, padding('valid'|'same'), use_bias, activation,
                  # groups (optional, > 1 only: Keras Conv2D(groups=G); absent means 1)
    "dwconv",     # DepthwiseConv2D, multiplier 1: kernel, stride, padding, use_bias, activation
    "bn",         # attrs: epsilon
    "relu",       # attrs: max_value (None | 6.0: Keras ReLU(6.))
    "add",
    "concat",     # channel concat (Keras Concatenate(axis=-1))
    "maxpool",    # attrs: pool, stride, padding
    "avgpool",    # attrs: pool, stride, padding (padding excluded from the mean)
    "gap",        # global average pool
    "flatten",    # NHWC -> (H*W*C,) in Keras channels_last order
    "identity",   # Dropout / Activation('linear') at inference
    "dense",      # attrs: units, activation(None|'relu'|'softmax'|any ACTIVATIONS), use_bias
    "softmax",
    "act",        # Keras Activation / LeakyReLU: attrs fn (ACTIVATIONS), alpha (LeakyReLU slope)
    "binary",     # Multiply / Subtract / Maximum / Minimum / Average: attrs fn; the 2nd input may be one
                  # channel row per image (squeeze-excite broadcast)
    "gmp",        # GlobalMaxPooling2D
    "reshape",    # attrs: shape (element order unchanged: NHWC row-major)
    "rescale",    # Keras Rescaling: attrs scale, offset (scalars or per-channel lists)
    "normalization",  # Keras Normalization(axis=-1): weights mean, variance, count
    "layernorm",  # Keras LayerNormalization over the last axis: attrs epsilon; center / scale only when False
    "rmsnorm",    # Keras 3 RMSNormalization over the last axis: y = x rsqrt(mean(x^2) + epsilon) scale; attrs epsilon
                  # (Keras default 1e-6); scale only when False; weight scale (C,); a (T, C) or (H, W, C) input
    "layerscale",  # ConvNeXt LayerScale: y = x * gamma (per channel); attrs init_values
    "groupnorm",  # Keras GroupNormalization over (H, W, C / G) of an (H, W, C) map: attrs groups (the resolved G;
                  # Keras' groups=-1, instance norm, is stored as C), epsilon; center / scale only when False
    "deconv",     # Keras Conv2DTranspose: filters, kernel=(kh,kw), stride, padding('valid'|'same'), use_bias,
                  # activation; kernel (kh, kw, filters, cin) (Keras HWOI), no output_padding, no dilation
    "upsample",   # Keras UpSampling2D: size=(sh,sw), interpolation ('nearest' | 'bilinear', half-pixel centres)
    "crop",       # Keras Cropping2D: crop=((t,b),(l,r))
    "mha",        # Keras MultiHeadAttention over all positions: num_heads, key_dim, value_dim (absent means key_dim),
                  # use_bias; inputs [query], [query, value] or [query, value, key] in Keras argument order (one input
                  # is self-attention, a missing key means key = value), each (H, W, C) or (T, C); value and key have
                  # the same token count, their channel counts are their own; output the query's shape.  causal
                  # (stored only when True; one input only): Keras' use_causal_mask, query i attends keys j <= i.
                  # key_mask (stored only when True; one source only, never with causal): the layer's LAST input is
                  # then a (T,) mask tensor, T the token count, and token j is padding iff -1 < mask[j] < 1 (for
                  # Embedding(mask_zero=True) simply the ids tensor the Embedding reads; `propagate_masks` derives
                  # the edge).  A padded token is not attended as a key; at kept positions this is Keras' implicit
                  # padding mask exactly.  At a padded QUERY position the context row is zeros, where Keras' fully
                  # masked softmax row yields the plain mean of V: outputs at padded positions are defined but
                  # not Keras'; nothing at a kept position reads them.
                  # kv_heads (grouped-query attention, Keras 3 GroupedQueryAttention; one source only, never with
                  # key_mask): the num_heads query heads share kv_heads key / value heads, head h reads K / V head
                  # h // (num_heads // kv_heads); the key / value kernels are then (C, kv_heads, d).  Absent means
                  # num_heads; a layer read from GroupedQueryAttention always stores it.
                  # rope (stored only when set; one source only, never with key_mask; key_dim even): the max
                  # wavelength W of a rotary position embedding applied to Q and K between the projection and the
                  # score product, rotate-half convention, theta(t, i) = t W^(-2i/d) (Keras class
                  # RotaryGroupedQueryAttention, the project's own)
    "posembed",   # ViT class token + learned position embedding: attrs class_token; (H, W, C) -> (1, T + ct, C)
    "winattn",    # Swin window attention (the project's own layer, Keras class WindowAttention): num_heads, key_dim,
                  # window (M), shift (0 <= s < M), use_bias; (H, W, C) -> (H, W, C), H and W multiples of M.
                  # Weights as `mha` plus relative_position_bias_table ((2M-1)^2, heads)
    "queries",    # a learned constant tensor (the project's own layer, Keras class LearnedQueries): attrs length N,
                  # dim C, initializer ("normal" | "zeros"); weight embeddings (N, C); the one input supplies only the
                  # batch size; output (1, N, C), the same for every image
    "embedding",  # Keras Embedding: attrs input_dim (V <= 2**24), output_dim (C); weight embeddings (V, C); input
                  # (T,) token ids carried as float32 (truncated toward zero, every id exact), output (T, C); an id
                  # outside [0, V) yields a zero row (TensorFlow's GPU gather; a kernel cannot raise).  mask_zero
                  # (stored only when True): position t is padding iff its id truncates to 0, -1 < id < 1; the
                  # mask reaches the `mha` layers that `propagate_masks` finds
    "space_to_depth",  # Swin patch merging's rearrangement (Keras class SpaceToDepth): attrs block (2);
                  # (H, W, C) -> (H/2, W/2, 4C), out[y, x, (2 dx + dy) C + c] = in[2y + dy, 2x + dx, c]: the
                  # concatenation of x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2] (not tf.nn.space_to_depth,
                  # whose block order is (2 dy + dx))
)

# activations the runtime executes (fused into conv / dense / eltwise epilogues,
# csrc/kernels/common.h ActMode), by their Keras names
ACTIVATIONS = ("linear", "relu", "relu6", "swish", "silu", "sigmoid", "tanh", "hard_sigmoid", "hard_swish", "gelu",
               "elu", "selu", "softplus", "leaky_relu", "gelu_tanh")
# Keras activation name -> kernel ActMode (csrc/kernels/common.h); leaky_relu also takes its slope
ACT_MODE = {None: 0, "linear": 0, "relu": 1, "relu6": 2, "swish": 3, "silu": 3, "sigmoid": 4, "tanh": 5,
            "hard_sigmoid": 6, "hard_swish": 7, "gelu": 8, "elu": 9, "selu": 10, "softplus": 11, "leaky_relu": 12,
            "gelu_tanh": 13}      # 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))): GPT-2's form


def bn_params(weights, name: str) -> Dict:
    """gamma / beta / moving statistics of BN layer `name`, with Keras' defaults
    (gamma 1, beta 0) for a layer built with scale=False / center=False."""
    import numpy as np
    mu = weights[f"{name}/moving_mean"]
    return {"gamma": weights.get(f"{name}/gamma", np.ones_like(mu)),
            "beta": weights.get(f"{name}/beta", np.zeros_like(mu)),
            "moving_mean": mu, "moving_variance": weights[f"{name}/moving_variance"]}


def depthwise_kernel(weights, name: str):
    """(kh, kw, C) kernel of a depthwise step: a DepthwiseConv2D's `depthwise_kernel` (kh, kw, C, 1), or the
    `kernel` (kh, kw, 1, C) of a Conv2D(groups=C) with one channel per group."""
    if f"{name}/depthwise_kernel" in weights:
        return weights[f"{name}/depthwise_kernel"][..., 0]
    return weights[f"{name}/kernel"][:, :, 0, :]


def conv_kernel(weights, p: Dict):
    """HWIO kernel of a conv step's layer `p["conv"]`; a Dense on (H, W, C) (p["dense"]) keeps the Keras
    (cin, units) shape in the weights and is a 1x1 kernel here."""
    if p.get("mha"):
        k = mha_projection(weights, p["conv"], p, p["mha"])[0]
        return k.reshape((1, 1) + tuple(k.shape))
    k = weights[f"{p['conv']}/kernel"]
    if p.get("deconv"):         # Conv2DTranspose keeps Keras' (kh, kw, filters, cin); packers and BN folding want
        return k.transpose(0, 1, 3, 2)      # the output channels last: (kh, kw, cin, filters)
    return k.reshape((1, 1) + tuple(k.shape)) if p.get("dense") else k


def conv_bias(weights, p: Dict):
    """Bias of a conv step's layer `p["conv"]`, or None."""
    if p.get("mha"):
        return mha_projection(weights, p["conv"], p, p["mha"])[1]
    return weights.get(f"{p['conv']}/bias")


MHA_PARTS = {"q": ("query",), "k": ("key",), "v": ("value",), "qk": ("query", "key"), "kv": ("key", "value"),
             "qkv": ("query", "key", "value")}


def mha_sources(inputs: Sequence[str], key_mask: bool = False) -> Tuple[str, str, str]:
    """(query, key, value) source tensors of an `mha` layer's inputs ([query], [query, value] or
    [query, value, key], Keras argument order; a missing key means key = value).  With `key_mask` (the layer's
    attribute) the last input is the mask tensor and is ignored."""
    if key_mask:
        inputs = inputs[:-1]
    q = inputs[0]
    v = inputs[1] if len(inputs) > 1 else q
    k = inputs[2] if len(inputs) > 2 else v
    return q, k, v


def mha_projection(weights, name: str, head: Dict, part: str):
    """(kernel, bias or None) of the GEMMs around the attention core of MultiHeadAttention layer `name`;
    `head` holds heads, key_dim, value_dim.  The input projections that share a source tensor stand side by side
    in one GEMM: part "qkv" is (C, h * (2 d + dv)) ordered [Q | K | V], "qk" [Q | K], "kv" [K | V], and "q", "k",
    "v" one projection each (MHA_PARTS), head-major inside each projection, with Keras' 1/sqrt(key_dim) query
    scale folded into the Q columns and the Q bias.  part "out": the output projection (h * dv, C)."""
    import numpy as np
    h, d, dv = head["heads"], head["key_dim"], head["value_dim"]
    if part == "out":
        return (weights[f"{name}/attention_output/kernel"].reshape(h * dv, -1),
                weights.get(f"{name}/attention_output/bias"))
    # The 1/sqrt(d) query scale stays folded here also under a rotary embedding (the layer's `rope`): the rotation
    # of the `rope` step is linear, so it commutes with the scale.  Grouped-query attention: K and V have
    # head["kv_heads"] heads (absent: h), so "qkv" is (C, h d + hkv d + hkv dv)
    hkv = int(head.get("kv_heads") or h)
    scale = {"query": 1.0 / np.sqrt(np.float64(d)), "key": 1.0, "value": 1.0}
    width = {"query": h * d, "key": hkv * d, "value": hkv * dv}
    ks = [(weights[f"{name}/{q}/kernel"].astype(np.float64) * scale[q]).reshape(-1, width[q])
          for q in MHA_PARTS[part]]
    kernel = np.concatenate(ks, axis=1).astype(np.float32)
    if f"{name}/query/bias" not in weights:
        return kernel, None
    bs = [(weights[f"{name}/{q}/bias"].astype(np.float64) * scale[q]).reshape(-1) for q in MHA_PARTS[part]]
    return kernel, np.concatenate(bs).astype(np.float32)


def window_index(m: int):
    """Swin's relative position index of an M x M window, (M^2, M^2) ints into the (2M-1)^2 rows of the bias
    table: index[(i, j), (k, l)] = (i - k + M - 1)(2M - 1) + (j - l + M - 1)."""
    import numpy as np
    i, j = np.divmod(np.arange(m * m), m)
    return (i[:, None] - i[None, :] + m - 1) * (2 * m - 1) + (j[:, None] - j[None, :] + m - 1)


def same_pads(size: int, k: int, s: int) -> Tuple[int, int]:
    """TF/Keras 'same' padding of one spatial dim: (before, after), the odd pixel after."""
    out = -(-size // s)
    total = max((out - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def _pair(v) -> Tuple[int, int]:
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _tokens(shape: Sequence[int]) -> int:
    """Positions of a per-image (H, W, C) or (T, C) tensor: everything but the channel axis."""
    t = 1
    for d in shape[:-1]:
        t *= d
    return t


def deconv_out_len(size: int, k: int, s: int, padding: str) -> int:
    """Keras `deconv_output_length` (no output_padding): 'same' size*s, 'valid' size*s + max(k - s, 0)."""
    return size * s if padding == "same" else size * s + max(k - s, 0)


def deconv_pad_before(k: int, s: int, padding: str) -> int:
    """Where a Conv2DTranspose's output starts in the full scatter frame of length (size-1)*s + k."""
    return max(k - s, 0) // 2 if padding == "same" else 0


@dataclass
class Layer:
    name: str
    op: str
    inputs: List[str]
    attrs: Dict = field(default_factory=dict)
    out_shape: Tuple[int, ...] = ()

    # ---- weights (Keras get_weights() order) ----
    def weight_shapes(self, in_shapes: Sequence[Tuple[int, ...]]) -> List[Tuple[str, Tuple[int, ...]]]:
        """Return [(weight_name, shape)] in Keras order.

        conv: kernel HWIO + bias; bn: gamma, beta, moving_mean, moving_variance;
        dense: kernel (in, out) + bias.
        """
        if self.op == "conv":
            kh, kw = self.attrs["kernel"]
            cin = in_shapes[0][-1]
            # grouped (Keras layout): output channel o belongs to group o // (filters // groups)
            out = [(f"{self.name}/kernel", (kh, kw, cin // self.attrs.get("groups", 1), self.attrs["filters"]))]
            if self.attrs.get("use_bias", True):
                out.append((f"{self.name}/bias", (self.attrs["filters"],)))
            return out
        if self.op == "deconv":
            kh, kw = self.attrs["kernel"]
            out = [(f"{self.name}/kernel", (kh, kw, self.attrs["filters"], in_shapes[0][-1]))]    # Keras HWOI
            if self.attrs.get("use_bias", True):
                out.append((f"{self.name}/bias", (self.attrs["filters"],)))
            return out
        if self.op == "bn":
            # Keras omits gamma for scale=False (InceptionV3) and beta for center=False
            c = in_shapes[0][-1]
            keep = (("gamma", self.attrs.get("scale", True)), ("beta", self.attrs.get("center", True)),
                    ("moving_mean", True), ("moving_variance", True))
            return [(f"{self.name}/{n}", (c,)) for n, k in keep if k]
        if self.op == "dwconv":
            kh, kw = self.attrs["kernel"]
            cin = in_shapes[0][-1]
            out = [(f"{self.name}/depthwise_kernel", (kh, kw, cin, 1))]
            if self.attrs.get("use_bias", True):
                out.append((f"{self.name}/bias", (cin,)))
            return out
        if self.op == "normalization":
            c = in_shapes[0][-1]
            return [(f"{self.name}/mean", (c,)), (f"{self.name}/variance", (c,)), (f"{self.name}/count", ())]
        if self.op in ("layernorm", "groupnorm"):
            # Keras omits gamma for scale=False and beta for center=False, as BatchNormalization does
            c = in_shapes[0][-1]
            keep = (("gamma", self.attrs.get("scale", True)), ("beta", self.attrs.get("center", True)))
            return [(f"{self.name}/{n}", (c,)) for n, k in keep if k]
        if self.op == "rmsnorm":                # Keras omits scale for scale=False
            return [(f"{self.name}/scale", (in_shapes[0][-1],))] if self.attrs.get("scale", True) else []
        if self.op == "layerscale":
            return [(f"{self.name}/gamma", (in_shapes[0][-1],))]
        if self.op == "mha":
            c, h, d = in_shapes[0][-1], self.attrs["num_heads"], self.attrs["key_dim"]
            dv = self.attrs.get("value_dim") or d
            # each projection follows its own source
            _, ck, cv = (s[-1] for s in mha_sources(in_shapes, bool(self.attrs.get("key_mask"))))
            hkv = int(self.attrs.get("kv_heads") or h)
            out = []
            for part, shp, bshp in (("query", (c, h, d), (h, d)), ("key", (ck, hkv, d), (hkv, d)),
                                    ("value", (cv, hkv, dv), (hkv, dv)), ("attention_output", (h, dv, c), (c,))):
                out.append((f"{self.name}/{part}/kernel", shp))
                if self.attrs.get("use_bias", True):
                    out.append((f"{self.name}/{part}/bias", bshp))
            return out
        if self.op == "winattn":
            c, h, d, m = in_shapes[0][-1], self.attrs["num_heads"], self.attrs["key_dim"], self.attrs["window"]
            out = []
            for part, shp, bshp in (("query", (c, h, d), (h, d)), ("key", (c, h, d), (h, d)),
                                    ("value", (c, h, d), (h, d)), ("attention_output", (h, d, c), (c,))):
                out.append((f"{self.name}/{part}/kernel", shp))
                if self.attrs.get("use_bias", True):
                    out.append((f"{self.name}/{part}/bias", bshp))
            return out + [(f"{self.name}/relative_position_bias_table", ((2 * m - 1) ** 2, h))]
        if self.op == "queries":
            return [(f"{self.name}/embeddings", (int(self.attrs["length"]), int(self.attrs["dim"])))]
        if self.op == "embedding":
            return [(f"{self.name}/embeddings", (int(self.attrs["input_dim"]), int(self.attrs["output_dim"])))]
        if self.op == "posembed":
            t, c = _tokens(in_shapes[0]), in_shapes[0][-1]
            ct = 1 if self.attrs.get("class_token") else 0
            return ([(f"{self.name}/class_token", (1, 1, c))] if ct else []) + [
                (f"{self.name}/position_embedding", (t + ct, c))]
        if self.op == "dense":
            cin = in_shapes[0][-1]
            out = [(f"{self.name}/kernel", (cin, self.attrs["units"]))]
            if self.attrs.get("use_bias", True):
                out.append((f"{self.name}/bias", (self.attrs["units"],)))
            return out
        return []

    def macs(self, in_shapes: Sequence[Tuple[int, ...]]) -> int:
        """Multiply-accumulates per image."""
        if self.op == "conv":
            kh, kw = self.attrs["kernel"]
            oh, ow, co = self.out_shape
            return oh * ow * co * kh * kw * in_shapes[0][-1] // self.attrs.get("groups", 1)
        if self.op == "dwconv":
            kh, kw = self.attrs["kernel"]
            oh, ow, co = self.out_shape
            return oh * ow * co * kh * kw
        if self.op == "deconv":                 # every input pixel meets every tap once
            kh, kw = self.attrs["kernel"]
            h, w, cin = in_shapes[0]
            return h * w * kh * kw * cin * self.attrs["filters"]
        if self.op == "dense":
            px = 1
            for d in in_shapes[0][:-1]:         # a Dense on (H, W, C) is a GEMM per pixel
                px *= d
            return px * in_shapes[0][-1] * self.attrs["units"]
        if self.op == "mha":                    # projections, Q K^T and P V, output projection
            t, c = _tokens(in_shapes[0]), in_shapes[0][-1]
            h, d = self.attrs["num_heads"], self.attrs["key_dim"]
            dv = self.attrs.get("value_dim") or d
            _, sk, sv = mha_sources(in_shapes, bool(self.attrs.get("key_mask")))
            tk = _tokens(sk)
            pairs = t * (t + 1) // 2 if self.attrs.get("causal") else t * tk      # (query, key) pairs of the core
            hkv = int(self.attrs.get("kv_heads") or h)       # the K / V projections have kv_heads heads
            return (t * c * h * d + tk * sk[-1] * hkv * d + tk * sv[-1] * hkv * dv + pairs * h * (d + dv)
                    + t * h * dv * c)
        if self.op == "winattn":                # projections (h d = C in Swin), scores and P V inside M x M windows
            (hh, ww, c), m = in_shapes[0], self.attrs["window"]
            hd = self.attrs["num_heads"] * self.attrs["key_dim"]
            return 4 * hh * ww * c * hd + 2 * hh * ww * m * m * hd
        return 0

    def to_json(self) -> Dict:
        return {"name": self.name, "op": self.op, "inputs": list(self.inputs),
                "attrs": _jsonable(self.attrs), "out_shape": list(self.out_shape)}

    @staticmethod
    def from_json(d: Dict) -> "Layer":
        attrs = dict(d.get("attrs", {}))
        for k in ("kernel", "pad", "pool", "size", "crop"):
            if k in attrs and isinstance(attrs[k], list):
                attrs[k] = _tuplify(attrs[k])
        return Layer(d["name"], d["op"], list(d["inputs"]), attrs, tuple(d.get("out_shape", ())))


def _tuplify(x):
    if isinstance(x, list):
        return tuple(_tuplify(v) for v in x)
    return x


def _jsonable(attrs: Dict) -> Dict:
    def conv(v):
        if isinstance(v, tuple):
            return [conv(x) for x in v]
        return v
    return {k: conv(v) for k, v in attrs.items()}


class Graph:
    """An ordered DAG of named layers (one output tensor per layer)."""

    def __init__(self, name: str = "model"):
        self.name = name
        self.layers: Dict[str, Layer] = {}
        self.order: List[str] = []
        self.input_names: List[str] = []
        self.output_names: List[str] = []
        self._consumers: Optional[Dict[str, List[str]]] = None

    # ---------------------------------------------------------------- build
    def add(self, layer: Layer) -> str:
        if layer.name in self.layers:
            raise ValueError(f"duplicate layer name {layer.name!r}")
        for i in layer.inputs:
            if i not in self.layers:
                raise ValueError(f"layer {layer.name!r} consumes unknown tensor {i!r}")
        if layer.op == "conv" and layer.attrs.get("groups", 1) != 1:
            gr, cin = layer.attrs["groups"], self.layers[layer.inputs[0]].out_shape[-1]
            if not isinstance(gr, int) or gr < 1 or cin % gr or layer.attrs["filters"] % gr:
                raise ValueError(f"conv {layer.name!r}: groups={gr} must divide the input channels ({cin}) "
                                 f"and filters ({layer.attrs['filters']})")
        if layer.op == "groupnorm":
            shp = self.layers[layer.inputs[0]].out_shape if len(layer.inputs) == 1 else ()
            gr = layer.attrs.get("groups", 32)
            if len(shp) != 3:
                raise ValueError(f"groupnorm {layer.name!r}: needs one (H, W, C) input, got {tuple(shp)}")
            if not isinstance(gr, int) or isinstance(gr, bool) or gr == 0 or gr < -1:
                raise ValueError(f"groupnorm {layer.name!r}: groups must be a positive int or -1, got {gr!r}")
            gr = shp[-1] if gr == -1 else gr
            if shp[-1] % gr:
                raise ValueError(f"groupnorm {layer.name!r}: groups={gr} must divide the {shp[-1]} channels")
            layer.attrs["groups"] = gr              # the resolved G
        if layer.op == "upsample":
            sz = layer.attrs.get("size")
            if (not isinstance(sz, tuple) or len(sz) != 2 or any(not isinstance(v, int) or v < 1 for v in sz)
                    or layer.attrs.get("interpolation", "nearest") not in ("nearest", "bilinear")):
                raise ValueError(f"upsample {layer.name!r}: size must be two positive ints and interpolation "
                                 f"'nearest' or 'bilinear' (got {sz}, {layer.attrs.get('interpolation')!r})")
        if layer.op == "mha":
            shapes = [self.layers[i].out_shape for i in layer.inputs]
            if "key_mask" in layer.attrs:
                if layer.attrs["key_mask"] is not True:
                    raise ValueError(f"mha {layer.name!r}: key_mask is stored only when True (got "
                                     f"{layer.attrs['key_mask']!r}); leave it out otherwise")
                if layer.attrs.get("causal"):
                    raise ValueError(f"mha {layer.name!r}: a padding mask (key_mask) together with causal is not "
                                     f"built")
                if len(layer.inputs) != 2:
                    raise ValueError(f"mha {layer.name!r}: a padding mask (key_mask) needs one source "
                                     f"(self-attention) and the mask tensor as the last input, got "
                                     f"{len(layer.inputs)} inputs")
                if len(shapes[0]) not in (2, 3) or tuple(shapes[1]) != (_tokens(shapes[0]),):
                    raise ValueError(f"mha {layer.name!r}: the mask tensor {layer.inputs[-1]!r} has shape "
                                     f"{tuple(shapes[1])}, not the token count ({_tokens(shapes[0])},) of "
                                     f"{tuple(shapes[0])}")
                shapes = shapes[:-1]                # the sources
            rank = len(shapes[0])
            if (not 1 <= len(shapes) <= 3 or any(len(s) not in (2, 3) for s in shapes)
                    or int(layer.attrs.get("num_heads", 0)) < 1 or int(layer.attrs.get("key_dim", 0)) < 1
                    or int(layer.attrs.get("value_dim") or 1) < 1):
                raise ValueError(f"mha {layer.name!r}: needs one input of rank 2 or 3 (got rank {rank}), or [query, "
                                 f"value] / [query, value, key] of rank 2 or 3 each (got {shapes}), num_heads >= 1 "
                                 f"and key_dim >= 1 (got {layer.attrs.get('num_heads')}, "
                                 f"{layer.attrs.get('key_dim')})")
            _, sk, sv = mha_sources(shapes)
            if _tokens(sk) != _tokens(sv):
                raise ValueError(f"mha {layer.name!r}: the key has {_tokens(sk)} tokens and the value "
                                 f"{_tokens(sv)}; they must agree")
            hq = int(layer.attrs["num_heads"])
            if "kv_heads" in layer.attrs:
                hkv = layer.attrs["kv_heads"]
                if not isinstance(hkv, int) or isinstance(hkv, bool) or hkv < 1 or hq % hkv:
                    raise ValueError(f"mha {layer.name!r}: kv_heads={hkv!r} must be a positive int that divides "
                                     f"num_heads={hq}")
            if "rope" in layer.attrs:
                w = layer.attrs["rope"]
                if isinstance(w, bool) or not isinstance(w, (int, float)) or not w > 0:
                    raise ValueError(f"mha {layer.name!r}: rope is the max wavelength, a positive number, and is "
                                     f"stored only when set (got {w!r})")
                if int(layer.attrs["key_dim"]) % 2:
                    raise ValueError(f"mha {layer.name!r}: a rotary embedding needs an even key_dim (got "
                                     f"{layer.attrs['key_dim']}): the rotation pairs channel i with i + key_dim / 2")
            if "kv_heads" in layer.attrs or "rope" in layer.attrs:
                what = " and ".join(k for k in ("kv_heads", "rope") if k in layer.attrs)
                if layer.attrs.get("key_mask"):
                    raise ValueError(f"mha {layer.name!r}: a padding mask (key_mask) together with {what} is not "
                                     f"built")
                if len(layer.inputs) != 1:
                    raise ValueError(f"mha {layer.name!r}: {what} needs one input (self-attention), got "
                                     f"{len(layer.inputs)} sources")
            if "causal" in layer.attrs:
                if layer.attrs["causal"] is not True:
                    raise ValueError(f"mha {layer.name!r}: causal is stored only when True (got "
                                     f"{layer.attrs['causal']!r}); leave it out otherwise")
                if len(layer.inputs) != 1:
                    raise ValueError(f"mha {layer.name!r}: a causal mask needs one input (self-attention), got "
                                     f"{len(layer.inputs)} sources")
            osh = layer.attrs.get("output_shape")
            if osh is not None and [int(v) for v in (osh if isinstance(osh, (list, tuple)) else [osh])] != [
                    shapes[0][-1]]:
                raise ValueError(f"mha {layer.name!r}: output_shape={osh} (only the query's {shapes[0][-1]} "
                                 f"channels)")
        if layer.op == "queries":
            a = layer.attrs
            if (len(layer.inputs) != 1 or int(a.get("length", 0)) < 1 or int(a.get("dim", 0)) < 1
                    or a.get("initializer", "normal") not in ("normal", "zeros")):
                raise ValueError(f"queries {layer.name!r}: needs one input (the batch size), length >= 1, dim >= 1 "
                                 f"and initializer 'normal' or 'zeros' (got {a.get('length')}, {a.get('dim')}, "
                                 f"{a.get('initializer')!r})")
        if layer.op == "winattn" and ("rope" in layer.attrs or "kv_heads" in layer.attrs):
            raise ValueError(f"winattn {layer.name!r}: a rotary embedding (rope) or kv_heads on window attention is "
                             f"not built")
        if layer.op == "rmsnorm":
            shp = self.layers[layer.inputs[0]].out_shape if len(layer.inputs) == 1 else ()
            if len(shp) not in (2, 3):
                raise ValueError(f"rmsnorm {layer.name!r}: needs one (T, C) or (H, W, C) input, got {tuple(shp)}")
        if layer.op == "embedding":
            shp = self.layers[layer.inputs[0]].out_shape if len(layer.inputs) == 1 else None
            v, c = int(layer.attrs.get("input_dim", 0)), int(layer.attrs.get("output_dim", 0))
            if shp is None or len(shp) != 1 or v < 1 or c < 1:
                raise ValueError(f"embedding {layer.name!r}: needs one (T,) input of token ids (got {shp}), "
                                 f"input_dim >= 1 and output_dim >= 1 (got {layer.attrs.get('input_dim')}, "
                                 f"{layer.attrs.get('output_dim')})")
            if v > 2 ** 24:
                raise ValueError(f"embedding {layer.name!r}: input_dim={v} exceeds 2**24; token ids are carried as "
                                 f"float32 and would no longer be exact")
        if layer.op == "winattn":
            shp = self.layers[layer.inputs[0]].out_shape
            a = layer.attrs
            m, sh = int(a.get("window", 0)), int(a.get("shift", 0))
            if (len(layer.inputs) != 1 or len(shp) != 3 or int(a.get("num_heads", 0)) < 1
                    or int(a.get("key_dim", 0)) < 1 or m < 1 or not 0 <= sh < m):
                raise ValueError(f"winattn {layer.name!r}: needs one (H, W, C) input (got {shp}), num_heads >= 1, "
                                 f"key_dim >= 1, window >= 1 and 0 <= shift < window (got {a.get('num_heads')}, "
                                 f"{a.get('key_dim')}, {a.get('window')}, {a.get('shift')})")
            if shp[0] % m or shp[1] % m:
                raise ValueError(f"winattn {layer.name!r}: the {shp[0]} x {shp[1]} map is not a multiple of the "
                                 f"{m} x {m} window")
        if layer.op == "space_to_depth":
            shp = self.layers[layer.inputs[0]].out_shape
            if (len(layer.inputs) != 1 or len(shp) != 3 or int(layer.attrs.get("block", 2)) != 2 or shp[0] % 2
                    or shp[1] % 2):
                raise ValueError(f"space_to_depth {layer.name!r}: needs block 2 and an (H, W, C) input with even "
                                 f"H and W (got block {layer.attrs.get('block')}, {shp})")
        if layer.op == "posembed":
            shp = self.layers[layer.inputs[0]].out_shape
            if len(shp) not in (2, 3):
                raise ValueError(f"posembed {layer.name!r}: needs an (H, W, C), (1, T, C) or (T, C) input, got {shp}")
        if layer.op == "crop" and layer.out_shape:
            self._infer_shape(layer)                # an empty result is refused even with a given shape
        layer.out_shape = tuple(layer.out_shape) or self._infer_shape(layer)
        self.layers[layer.name] = layer
        self.order.append(layer.name)
        if layer.op == "input":
            self.input_names.append(layer.name)
        self._consumers = None
        return layer.name

    def _infer_shape(self, layer: Layer) -> Tuple[int, ...]:
        ins = [self.layers[i].out_shape for i in layer.inputs]
        a = layer.attrs
        if layer.op == "input":
            return tuple(a["shape"])
        if layer.op == "zeropad":
            (t, b), (l, r) = a["pad"]
            h, w, c = ins[0]
            return (h + t + b, w + l + r, c)
        if layer.op in ("conv", "dwconv"):
            h, w, c = ins[0]
            kh, kw = a["kernel"]
            s = a.get("stride", 1)
            co = a["filters"] if layer.op == "conv" else c
            if a.get("padding", "valid") == "same":
                return (-(-h // s), -(-w // s), co)
            return ((h - kh) // s + 1, (w - kw) // s + 1, co)
        if layer.op == "deconv":
            h, w, _ = ins[0]
            kh, kw = a["kernel"]
            s, pad = a.get("stride", 1), a.get("padding", "valid")
            return (deconv_out_len(h, kh, s, pad), deconv_out_len(w, kw, s, pad), a["filters"])
        if layer.op == "upsample":
            h, w, c = ins[0]
            sh, sw = a["size"]
            return (h * sh, w * sw, c)
        if layer.op == "crop":
            (t, b), (l, r) = a["crop"]
            h, w, c = ins[0]
            if min(t, b, l, r) < 0 or h - t - b < 1 or w - l - r < 1:
                raise ValueError(f"crop {layer.name!r}: {a['crop']} leaves nothing of {ins[0]}")
            return (h - t - b, w - l - r, c)
        if layer.op in ("bn", "relu", "softmax", "identity", "act", "rescale", "normalization", "layernorm",
                        "layerscale", "mha", "winattn", "groupnorm", "rmsnorm"):
            return ins[0]
        if layer.op == "space_to_depth":
            return (ins[0][0] // 2, ins[0][1] // 2, 4 * ins[0][2])
        if layer.op == "posembed":
            return (1, _tokens(ins[0]) + (1 if a.get("class_token") else 0), ins[0][-1])
        if layer.op == "queries":
            return (1, int(a["length"]), int(a["dim"]))
        if layer.op == "embedding":
            return (ins[0][0], int(a["output_dim"]))
        if layer.op == "binary":
            return ins[0]
        if layer.op == "reshape":
            shp = tuple(int(d) for d in a["shape"])
            n_in = n_out = 1
            for d in ins[0]:
                n_in *= d
            for d in shp:
                n_out *= d
            if n_in != n_out:
                raise ValueError(f"reshape {layer.name}: {ins[0]} -> {shp}")
            return shp
        if layer.op == "flatten":
            n = 1
            for d in ins[0]:
                n *= d
            return (n,)
        if layer.op == "concat":
            if len(ins) < 2 or any(len(s) != 3 or s[:2] != ins[0][:2] for s in ins):
                raise ValueError(f"concat {layer.name}: inputs {ins} do not share H x W")
            return ins[0][:2] + (sum(s[2] for s in ins),)
        if layer.op == "add":
            if any(s != ins[0] for s in ins):
                raise ValueError(f"add {layer.name}: mismatched shapes {ins}")
            return ins[0]
        if layer.op in ("maxpool", "avgpool"):
            h, w, c = ins[0]
            (ph, pw), s = _pair(a["pool"]), a["stride"]
            if a.get("padding", "valid") == "same":
                return (-(-h // s), -(-w // s), c)
            return ((h - ph) // s + 1, (w - pw) // s + 1, c)
        if layer.op in ("gap", "gmp"):
            return (1, 1, ins[0][-1]) if a.get("keepdims") else (ins[0][-1],)
        if layer.op == "dense":
            return tuple(ins[0][:-1]) + (a["units"],)     # Keras Dense acts on the last axis
        raise ValueError(f"unknown op {layer.op}")

    # -------------------------------------------------------------- queries
    def __getitem__(self, name: str) -> Layer:
        return self.layers[name]

    def get_layer(self, name: str) -> Layer:
        if name not in self.layers:
            raise KeyError(f"no layer named {name!r} in {self.name}")
        return self.layers[name]

    def __len__(self) -> int:
        return len(self.order)

    def index(self, name: str) -> int:
        return self.order.index(name)

    @property
    def output(self) -> str:
        return self.output_names[0] if self.output_names else self.order[-1]

    @property
    def input(self) -> str:
        return self.input_names[0]

    def consumers(self) -> Dict[str, List[str]]:
        if self._consumers is None:
            c: Dict[str, List[str]] = {n: [] for n in self.order}
            for n in self.order:
                for i in self.layers[n].inputs:
                    c[i].append(n)
            self._consumers = c
        return self._consumers

    def in_shapes(self, name: str) -> List[Tuple[int, ...]]:
        return [self.layers[i].out_shape for i in self.layers[name].inputs]

    def weight_specs(self, names: Optional[Iterable[str]] = None) -> List[Tuple[str, Tuple[int, ...]]]:
        names = self.order if names is None else list(names)
        out = []
        for n in names:
            out.extend(self.layers[n].weight_shapes(self.in_shapes(n)))
        return out

    def count_params(self) -> int:
        total = 0
        for _, shp in self.weight_specs():
            p = 1
            for d in shp:
                p *= d
            total += p
        return total

    def layer_macs(self, name: str) -> int:
        return self.layers[name].macs(self.in_shapes(name))

    def total_macs(self) -> int:
        return sum(self.layer_macs(n) for n in self.order)

    def ancestors(self, name: str, inclusive: bool = True) -> set:
        """All layers that `name` transitively depends on."""
        seen = set()
        stack = [name]
        while stack:
            n = stack.pop()
            if n in seen:
                continue
            seen.add(n)
            stack.extend(self.layers[n].inputs)
        if not inclusive:
            seen.discard(name)
        return seen

    def tensor_bytes(self, name: str, dtype_bytes: int = 2) -> int:
        p = 1
        for d in self.layers[name].out_shape:
            p *= d
        return p * dtype_bytes

    # ------------------------------------------------------- serialization
    def to_json(self) -> str:
        return json.dumps({
            "format": "adapt-graph-v1",
            "name": self.name,
            "layers": [self.layers[n].to_json() for n in self.order],
            "inputs": self.input_names,
            "outputs": self.output_names,
        })

    @staticmethod
    def from_json(s: str) -> "Graph":
        d = json.loads(s)
        if d.get("format") != "adapt-graph-v1":
            raise ValueError("not an adapt-graph-v1 document")
        g = Graph(d["name"])
        for ld in d["layers"]:
            layer = Layer.from_json(ld)
            # sub-graph inputs may reference tensors produced elsewhere; they
            # are declared as 'input' layers by the slicer, so add() succeeds.
            g.layers[layer.name] = layer
            g.order.append(layer.name)
        g.input_names = list(d["inputs"])
        g.output_names = list(d["outputs"])
        return g

    def to_dot(self, show_shapes: bool = True) -> str:
        """Graphviz DOT of the layer DAG (the reference renders each slice with
        `tf.keras.utils.plot_model`, `src/node.py:49`); slice inputs that stand for
        another slice's tensors are drawn dashed."""
        def q(s: str) -> str:
            return '"' + s.replace('"', r'\"') + '"'
        lines = [f"digraph {q(self.name)} {{", "  rankdir=TB;", '  node [shape=record, fontsize=10];']
        for n in self.order:
            L = self.layers[n]
            label = f"{n}|{L.op}" + (f"|{tuple(L.out_shape)}" if show_shapes else "")
            style = ", style=dashed" if L.op == "input" and L.attrs.get("stands_for", "input") != "input" else ""
            lines.append(f"  {q(n)} [label={q('{' + label + '}')}{style}];")
        for n in self.order:
            for i in self.layers[n].inputs:
                lines.append(f"  {q(i)} -> {q(n)};")
        lines.append("}")
        return "\n".join(lines)

    def summary(self) -> str:
        lines = [f"Model: {self.name}", f"{'Layer':40s} {'Op':8s} {'Output':>18s} {'Params':>10s}"]
        for n in self.order:
            L = self.layers[n]
            p = 0
            for _, shp in L.weight_shapes(self.in_shapes(n)):
                q = 1
                for d in shp:
                    q *= d
                p += q
            lines.append(f"{n:40s} {L.op:8s} {str(L.out_shape):>18s} {p:>10d}")
        lines.append(f"Total params: {self.count_params():,}")
        return "\n".join(lines)


# ------------------------------------------------------------- padding masks
def holds_token_ids(g: "Graph", name: str) -> bool:
    """Whether tensor `name` is read as token ids only: it has consumers, and each is an `embedding` or takes it
    in the mask slot (the last input) of an `mha` with key_mask and nowhere else."""
    cons = g.consumers().get(name, [])

    def as_ids(L: "Layer") -> bool:
        if L.op == "embedding":
            return True
        return bool(L.op == "mha" and L.attrs.get("key_mask") and L.inputs[-1] == name
                    and name not in L.inputs[:-1])
    return bool(cons) and all(as_ids(g.layers[c]) for c in cons)


# layers a padding mask travels through unchanged (Keras >= 2.10 and Keras 3 propagate it implicitly); `add`,
# `binary`, `posembed` and `mha` have rules of their own below; every other consumer drops the mask
MASK_TRANSPARENT = ("layernorm", "dense", "act", "identity", "layerscale", "rmsnorm")


def propagate_masks(g: "Graph") -> Dict[str, str]:
    """Which padding mask reaches which self-attention layer: {mha layer name: mask tensor name}.  The one
    implementation of the rules, used by the Keras importer, the zoo builder and the Keras writer.

    A mask starts at an `embedding` with mask_zero (the mask tensor is the ids tensor it reads: position t is
    padding iff -1 < id < 1).  It travels unchanged through `add` and `binary` (the AND of the masks of those
    inputs that have one, which here must be one and the same tensor), MASK_TRANSPARENT layers, a 1x1 `conv` on
    tokens, `posembed` without a class token, and `mha` itself (its output carries the query's mask).  Any other
    consumer drops it.  Refused by layer name (NotImplementedError): a masked tensor into `gap` / `gmp` (Keras
    takes a masked mean), into a class-token `posembed` or into `winattn`; a mask on an `mha` with more than one
    source, or together with `causal`; two different masks meeting in one `add` / `binary`.  An existing
    `key_mask` edge is not trusted: the mask tensor (last input) of such a layer is left out of its sources and
    the result says what the rules derive, so a caller can compare."""
    mask: Dict[str, Optional[str]] = {}
    reached: Dict[str, str] = {}
    for n in g.order:
        L = g.layers[n]
        ins = list(L.inputs[:-1]) if L.op == "mha" and L.attrs.get("key_mask") else list(L.inputs)
        got = [mask.get(i) for i in ins]
        have = sorted({m for m in got if m})
        out = None
        if L.op == "embedding":
            out = L.inputs[0] if L.attrs.get("mask_zero") else None
        elif not have:
            out = None
        elif L.op in ("add", "binary"):
            if len(have) > 1:
                raise NotImplementedError(f"{L.op} {n!r}: two different padding masks meet ({have[0]!r} and "
                                          f"{have[1]!r})")
            out = have[0]
        elif L.op in MASK_TRANSPARENT:
            out = got[0]
        elif L.op == "conv":
            out = (got[0] if _pair(L.attrs["kernel"]) == (1, 1) and _pair(L.attrs.get("stride", 1)) == (1, 1)
                   else None)
        elif L.op == "posembed":
            if L.attrs.get("class_token"):
                raise NotImplementedError(f"posembed {n!r}: a class token on a tensor that carries a padding mask "
                                          f"({have[0]!r})")
            out = got[0]
        elif L.op == "mha":
            if len(ins) > 1:
                raise NotImplementedError(f"mha {n!r}: a padding mask ({have[0]!r}) on a call with separate "
                                          f"sources; only self-attention takes it")
            if L.attrs.get("causal"):
                raise NotImplementedError(f"mha {n!r}: a padding mask ({have[0]!r}) together with the causal mask")
            if "kv_heads" in L.attrs or "rope" in L.attrs:
                raise NotImplementedError(f"mha {n!r}: a padding mask ({have[0]!r}) together with kv_heads / rope "
                                          f"(grouped-query or rotary attention)")
            reached[n] = out = got[0]
        elif L.op == "winattn":
            raise NotImplementedError(f"winattn {n!r}: its input carries a padding mask ({have[0]!r})")
        elif L.op in ("gap", "gmp"):
            raise NotImplementedError(f"{L.op} {n!r}: pooling over a tensor that carries a padding mask "
                                      f"({have[0]!r}); Keras takes a masked mean there, which is not built")
        mask[n] = out
    return reached


def with_key_masks(g: "Graph") -> "Graph":
    """`g` with the padding masks of `propagate_masks` made explicit: every reached `mha` gets `key_mask` and the
    mask tensor as its last input, a real edge that `consumers()`, `ancestors()`, the slicer and the planner see.
    A graph no mask reaches is returned as it is."""
    reached = propagate_masks(g)
    if all(g.layers[n].attrs.get("key_mask") and g.layers[n].inputs[-1] == m for n, m in reached.items()):
        stale = [n for n in g.order if g.layers[n].attrs.get("key_mask") and n not in reached]
        if not stale:
            return g
    out = Graph(g.name)
    for n in g.order:
        L = g.layers[n]
        ins, attrs = list(L.inputs), dict(L.attrs)
        if L.op == "mha" and attrs.pop("key_mask", None):
            ins = ins[:-1]
        if n in reached:
            ins, attrs["key_mask"] = ins + [reached[n]], True
        out.add(Layer(L.name, L.op, ins, attrs, tuple(L.out_shape)))
    out.input_names, out.output_names = list(g.input_names), list(g.output_names)
    return out
