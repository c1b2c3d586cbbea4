"""Launch-plan compiler: graph (slice) -> fused kernel steps.

The reference re-creates each slice as a Keras model on the worker
(`src/node.py:40-45,77-78`) and calls `model.predict` per request
(`src/node.py:177`), i.e. one TF op per Keras layer.  Here a slice is
compiled once into a short list of fused steps that map 1:1 onto our HIP
kernels:

* ``conv``     Conv2D [+BN folded] [+Add residual] [+ReLU / ReLU6, or the
               Conv2D's own activation='relu']; a preceding ZeroPadding2D or
               'same' padding (any stride, TF placement) becomes explicit pads.
               A Dense on an (H, W, C) tensor is a 1x1 conv step, and a
               LayerScale directly after either folds in where BN's scale goes
               (elsewhere it is an ``affine`` step)
* ``maxpool``  [ZeroPadding2D +] MaxPooling2D ('same' padding excluded from the max)
* ``avgpool``  AveragePooling2D (padding excluded from the mean)
* ``dwconv``   DepthwiseConv2D, or Conv2D(groups=C) with one channel per group,
               [+BN folded] [+ReLU/ReLU6], explicit pads
* ``layernorm`` LayerNormalization over the last axis; nothing fuses into it
* ``rmsnorm``  RMSNormalization over the last axis (Keras 3); nothing fuses into it
* ``rope``     the rotary position embedding of an attention layer `n` with `rope`: reads `n#qkv`, writes `n#rot`,
               the same rows of [Q | K | V] with the Q and K heads rotated (the angles from a host-side table) and
               V copied.  Out of place: no plan step aliases its input.  The ``attention`` step then reads `n#rot`
* ``groupnorm`` GroupNormalization over (H, W, C / G) per image; an activation directly after it (an
               ``act`` or ``relu`` layer of ``ACT_MODE``, its sole consumer, not exposed by a cut or an
               output) folds into the step as `act`, the ``binary`` step's rule: GN + swish is one launch
* ``attention`` the core of a MultiHeadAttention layer `n`, softmax(Q K^T) V per head.  The layer
               compiles to three steps: a ``conv`` (1x1, the Dense path) `n#qkv` whose weights are the
               three projections side by side, [Q | K | V] with 1/sqrt(key_dim) folded into Q; this
               step, `n#qkv` -> `n#ctx`; and a ``conv`` (1x1) `n#ctx` -> `n`, the output projection,
               which takes the block's Add as its residual like any Dense.  The `#` tensors are
               internal (a cut can only name `n`); a kind of its own, so no pair, sibling, stem or
               bottleneck pass ever sees it.  A layer whose query, key and value come from different
               tensors gets one projection ``conv`` per distinct source, the parts that share a source side
               by side: `n#qk` and `n#v` (q = k = `src + pos`, v = `src`), `n#q` and `n#kv` (key = value),
               or `n#q`, `n#k`, `n#v`; its ``attention`` step takes those buffers and records `tokens_q`,
               `tokens_k` and, as `q` / `k` / `v`, (which input, first column) of each part.  A causal layer's
               step carries `"causal": True` (only then: the key is absent otherwise) and runs the masked
               kernel, which skips the key tiles above the diagonal.  A layer with `key_mask` (a padding
               mask) takes the (T,) mask tensor as a second input and carries `"key_mask": True` (only then);
               its kernel does not load the key tiles past a sample's last kept token
* ``embedding`` a Keras Embedding: a row gather of its (V, C) table by the fp32 token ids of its (T,) input
* ``posembed`` ViT class token + learned position embedding
* ``queries``  a LearnedQueries layer: its (N, C) weight broadcast to every image, one copy step
* ``winattn``  the core of a Swin window attention layer `n`: like ``attention`` three steps, a ``conv``
               `n#qkv`, this step `n#qkv` -> `n#ctx` on the (H, W, C) map (nothing is rolled or
               partitioned in memory; the relative position bias and the shift mask are packed once
               by the executor), and the output-projection ``conv`` with the block's Add as residual
* ``space_to_depth`` Swin patch merging's 2 x 2 rearrangement, one copy step
* ``gconv``    Conv2D(groups > 1) [+BN folded] [+ReLU/ReLU6], explicit pads; no
               residual fusion, and a kind of its own so that no pass written
               for dense convs (pair, siblings, stem, bottleneck) ever sees it
* ``deconv``   Conv2DTranspose [+BN folded] [+ReLU/ReLU6]; `pads` is where the output
               starts in the full scatter frame (top, left).  A kind of its own: no
               residual, pair, sibling or bottleneck pass ever sees it
* ``upsample`` UpSampling2D (nearest / bilinear); not folded into a following conv
* ``crop``     Cropping2D
* ``concat``   Concatenate along channels (one copy launch per input)
* ``copy``     a Flatten/Dropout that the slice emits under its own name
               (otherwise they alias their input: Dropout everywhere,
               Flatten when a Dense consumes it)
* ``bn``       standalone BN [+ReLU] (only when a cut exposes the raw conv output)
* ``add``      standalone Add [+ReLU]
* ``relu``, ``pad`` (materialised ZeroPadding2D), ``gap``,
* ``dense``    Dense (+softmax) as a GEMM on the conv kernel + row softmax
* ``pack``     fp32 image -> bf16 NHWC padded to 8 channels (stem input)
* ``stem``     fp32 image -> conv1 7x7/s2 (+BN, ReLU) [-> pool1 3x3/s2] in one
               launch (csrc/kernels/stem.hip); replaces pack+conv[+maxpool]
               when the cut allows it

Fusion never hides a tensor that the slice must emit or that another layer
consumes, so any cut (including the multi-tensor frontier of BASELINE
config 2) is executable.

fp32 device plan only: a ``conv`` output that nothing but stride-s 1x1 convs read is produced only at the pixels
they sample (`subsample_lattice`: `p["subsample"]`, the compact map `p["out_hw"]`, `compact_maps`); it keeps its
name and kind, and stays full size wherever a cut or an output names it.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Set

from ..graph.ir import ACT_MODE, MHA_PARTS, Graph, _pair, deconv_pad_before, mha_sources, same_pads


@dataclass
class Step:
    kind: str
    out: str                       # tensor name produced (name of the last covered layer)
    ins: List[str]                 # tensor names consumed (physical names)
    covers: List[str]              # graph layers executed by this step
    p: Dict = field(default_factory=dict)


def compact_maps(steps: List["Step"]) -> Dict[str, tuple]:
    """{tensor: (rows, columns)} of the tensors a plan produces only on the lattice its readers sample
    (`subsample_lattice`): the per-plan override `tensor_shape` takes."""
    return {st.out: tuple(st.p["out_hw"]) for st in steps if st.p.get("subsample")}


def tensor_shape(g: Graph, name: str, compact: Optional[Dict[str, tuple]] = None) -> tuple:
    """Per-image shape of a plan tensor: the layer's own, or for the two internal tensors of a
    MultiHeadAttention layer (`n#qkv`, `n#ctx`) a (1, T, channels) token map; those of a window attention
    layer keep its (H, W) map.  `compact` (`compact_maps` of the plan in force): the tensors that plan stores
    as the (ceil(H / s), ceil(W / s), C) map of the pixels its readers sample."""
    if compact and name in compact:
        return tuple(compact[name]) + (g.layers[name].out_shape[-1],)
    base, _, tag = name.partition("#")
    L = g.layers[base]
    if tag in ("qkv", "ctx") and L.op == "winattn":     # a window attention's stay (H, W, channels) maps
        hd = int(L.attrs["num_heads"]) * int(L.attrs["key_dim"])
        return tuple(L.out_shape[:-1]) + (3 * hd if tag == "qkv" else hd,)
    if tag == "rot":                            # the rotated copy of `n#qkv`
        return tensor_shape(g, base + "#qkv", compact)
    if tag == "ctx" or tag in MHA_PARTS:
        # "ctx" has the query's tokens; a projection (`n#q`, `n#kv`, ...) the tokens of the source its parts share
        h, d = int(L.attrs["num_heads"]), int(L.attrs["key_dim"])
        dv = int(L.attrs.get("value_dim") or d)
        src = dict(zip(("query", "key", "value"), mha_sources(L.inputs, bool(L.attrs.get("key_mask")))))
        shape = L.out_shape if tag == "ctx" else g.layers[src[MHA_PARTS[tag][0]]].out_shape
        tokens = 1
        for v in shape[:-1]:
            tokens *= v
        hkv = int(L.attrs.get("kv_heads") or h)
        width = {"query": h * d, "key": hkv * d, "value": hkv * dv}
        return (1, tokens, h * dv if tag == "ctx" else sum(width[p] for p in MHA_PARTS[tag]))
    return tuple(L.out_shape)


def _phys(name: str, packed: Set[str]) -> str:
    return name + "#packed" if name in packed else name


def compile_plan(g: Graph, outputs: Optional[List[str]] = None, fp32: bool = False,
                 device_fusions: bool = True) -> List[Step]:
    """fp32=True: the fp32 execution path (csrc/kernels/conv_f32.hip) keeps the
    image as it is (no bf16 pack, so no stem fusion) and runs sibling convs as
    separate GEMMs.  device_fusions=False (with fp32): only the per-layer
    fusions (BN folding, conv epilogues, folded pads) -- the plan of the native
    CPU path (runtime/cpu_executor.py), which has no stem / pair / merged
    sibling kernels."""
    outputs = list(outputs or g.output_names)
    outset = set(outputs)
    cons = g.consumers()
    done: Set[str] = set()
    produced: Set[str] = set()
    steps: List[Step] = []
    packed: Set[str] = set()
    pad_fold: Dict[str, tuple] = {}     # consumer layer -> (source tensor, pad)

    def single(n: str) -> Optional[str]:
        """The unique consumer of n, if n may be fused into it."""
        if n in outset:
            return None
        c = cons.get(n, [])
        return c[0] if len(c) == 1 else None

    for n in g.order:
        L = g.layers[n]
        if L.op != "input":
            continue
        produced.add(n)
        done.add(n)
        c = L.out_shape[-1] if L.out_shape else 0
        # the user's fp32 image becomes bf16 NHWC with channels padded to 8 (a pure cast when C % 8 == 0)
        if len(L.out_shape) == 3 and L.attrs.get("stands_for", "input") == "input" and not fp32:
            packed.add(n)
            steps.append(Step("pack", n + "#packed", [n], [], {"cin": c, "cpad": ((c + 7) // 8) * 8}))

    alias: Dict[str, str] = {}          # identity / flatten-into-dense layers -> the tensor they pass on

    def R(t: str) -> str:
        return _phys(alias.get(t, t), packed)

    def same(n: str, L, k) -> tuple:
        """Explicit pads of a 'same' conv / pool (TF: the odd pixel after)."""
        h, w = g.layers[L.inputs[0]].out_shape[:2]
        kh, kw = _pair(k)
        s = L.attrs.get("stride", 1)
        return same_pads(h, kh, s), same_pads(w, kw, s)

    def act_mode(c: Optional[str]) -> int:
        """Kernel ActMode of a fusible activation layer (ReLU, ReLU6, swish, sigmoid, ...), 0 if `c`
        is not one (LeakyReLU needs its slope: it runs as its own step)."""
        if c is None:
            return 0
        Lc = g.layers[c]
        if Lc.op == "act":
            return 0 if Lc.attrs["fn"] == "leaky_relu" else ACT_MODE[Lc.attrs["fn"]]
        if Lc.op != "relu":
            return 0
        mv = Lc.attrs.get("max_value")
        if mv is None:
            return 1
        if float(mv) == 6.0:
            return 2
        raise NotImplementedError(f"ReLU(max_value={mv}) ({c})")

    def own_act(n: str, L) -> int:
        """ActMode of a conv / dense layer's own `activation` argument."""
        act = L.attrs.get("activation")
        if act in (None, "linear"):
            return 0
        if act not in ACT_MODE or act == "leaky_relu":
            raise NotImplementedError(f"{L.op} activation {act!r} ({n})")
        return ACT_MODE[act]

    def residual_add(n: str, cover: List[str]):
        """(residual, output, relu) of a Dense-like layer `n` whose single consumer is a two-input Add with a
        tensor already produced: the Add (and a ReLU / ReLU6 after it) joins `cover` and runs in the conv
        epilogue.  (None, n, 0) when there is none."""
        c1 = single(n)
        if c1 is None or g.layers[c1].op != "add" or len(g.layers[c1].inputs) != 2:
            return None, n, 0
        other = [i for i in g.layers[c1].inputs if i != n]
        if len(other) != 1 or alias.get(other[0], other[0]) not in produced:
            return None, n, 0
        cover.append(c1)
        out, relu = c1, 0
        c2 = single(c1)
        if 0 < act_mode(c2) <= 2:
            relu = act_mode(c2)
            cover.append(c2)
            out = c2
        return alias.get(other[0], other[0]), out, relu

    for n in g.order:
        if n in done:
            continue
        L = g.layers[n]
        a = L.attrs
        if L.op == "zeropad":
            c = single(n)
            if (c is not None and g.layers[c].op in ("conv", "dwconv", "maxpool", "avgpool")
                    and g.layers[c].attrs.get("padding", "valid") == "valid"):
                pad_fold[c] = (L.inputs[0], a["pad"])
                done.add(n)
                continue
            steps.append(Step("pad", n, [R(L.inputs[0])], [n], {"pad": a["pad"]}))
        elif L.op in ("conv", "dwconv") or (L.op == "dense" and len(g.layers[L.inputs[0]].out_shape) in (2, 3)):
            if L.op == "dense":
                # Dense on (H, W, C), or on a (T, C) token tensor, is a 1x1 conv: it gets the pointwise
                # kernels, the tuning table and the conv epilogue; the weight packers reshape its
                # (cin, units) kernel (p["dense"])
                if a.get("activation") == "softmax":
                    raise NotImplementedError(f"Dense(activation='softmax') on a rank-3 tensor ({n})")
                a = {"filters": a["units"], "kernel": (1, 1), "stride": 1, "padding": "valid",
                     "activation": a.get("activation"), "use_bias": a.get("use_bias", True)}
            src = L.inputs[0]
            pads = ((0, 0), (0, 0))
            cover = [n]
            if n in pad_fold:
                src, pads = pad_fold[n]
                cover = [g.layers[n].inputs[0], n]
            if a.get("padding", "valid") == "same":
                pads = same(n, L, a["kernel"])
            bn = None
            relu = 0
            res = None
            out = n
            post_act = 0                        # an activation the MFMA epilogue does not take (swish, ...)
            is_conv = L.op in ("conv", "dense")
            # Conv2D(groups=C) with one channel per group is a depthwise conv (ConvNeXt's 7x7)
            depthwise = L.op == "dwconv" or (L.op == "conv" and a.get("groups", 1) > 1 and a["groups"] == a["filters"]
                                             == g.layers[L.inputs[0]].out_shape[-1])
            grouped = L.op == "conv" and a.get("groups", 1) > 1 and not depthwise
            scale = None                        # a LayerScale folded like BN's scale
            if own_act(n, L):
                relu = own_act(n, L)            # Conv2D(activation=...): nothing after it fuses
                if not depthwise and relu > 2:
                    post_act, relu = relu, 0
            else:
                c1 = single(n)
                if c1 is not None and (g.layers[c1].op == "bn" or (g.layers[c1].op == "layerscale" and is_conv
                                                                   and not depthwise and not grouped)):
                    if g.layers[c1].op == "bn":
                        bn = c1
                    else:
                        scale = c1
                    cover.append(c1)
                    out = c1
                    c2 = single(c1)
                    feed = c1                       # the tensor the residual Add sees from this branch
                    while (c2 is not None and g.layers[c2].op == "identity"
                           and single(c2) is not None and g.layers[single(c2)].op == "add"):
                        cover.append(c2)            # drop-connect Dropout between the BN and the residual Add
                        feed, c2 = c2, single(c2)
                    if act_mode(c2) and (depthwise or act_mode(c2) <= 2):
                        relu = act_mode(c2)
                        cover.append(c2)
                        out = c2
                    elif (is_conv and not depthwise and not grouped and c2 is not None and g.layers[c2].op == "add"
                          and len(g.layers[c2].inputs) == 2):
                        other = [i for i in g.layers[c2].inputs if i != feed]
                        if len(other) == 1 and alias.get(other[0], other[0]) in produced:
                            res = alias.get(other[0], other[0])
                            cover.append(c2)
                            out = c2
                            c3 = single(c2)
                            if 0 < act_mode(c3) <= 2:
                                relu = act_mode(c3)
                                cover.append(c3)
                                out = c3
                elif act_mode(c1) and (depthwise or act_mode(c1) <= 2):
                    relu = act_mode(c1)
                    cover.append(c1)
                    out = c1
                elif L.op == "dense":           # a transformer block's Add directly after its last Dense
                    res, out, relu = residual_add(n, cover)
            kernel = tuple(_pair(a["kernel"]))
            if depthwise:
                steps.append(Step("dwconv", out, [R(src)], cover,
                                  {"conv": n, "bn": bn, "relu": relu, "pads": pads, "stride": a.get("stride", 1),
                                   "kernel": kernel}))
            elif grouped:
                cv_out = out if not post_act else n + "#preact"
                steps.append(Step("gconv", cv_out, [R(src)], cover,
                                  {"conv": n, "bn": bn, "relu": relu, "pads": pads, "stride": a.get("stride", 1),
                                   "kernel": kernel, "filters": a["filters"], "groups": a["groups"]}))
                if post_act:
                    steps.append(Step("act", out, [cv_out], [], {"mode": post_act, "alpha": 0.3}))
            else:
                cv_out = out if not post_act else n + "#preact"
                steps.append(Step("conv", cv_out, [R(src)] + ([res] if res else []), cover,
                                  {"conv": n, "bn": bn, "relu": relu, "residual": res, "pads": pads,
                                   "stride": a.get("stride", 1), "kernel": kernel,
                                   "filters": a["filters"], "packed_input": src in packed}))
                if scale:
                    steps[-1].p["scale"] = scale
                if L.op == "dense":
                    steps[-1].p["dense"] = True
                if post_act:
                    steps.append(Step("act", out, [cv_out], [], {"mode": post_act, "alpha": 0.3}))
            done.update(cover)
        elif L.op == "deconv":
            kh, kw = _pair(a["kernel"])
            s, padding = a.get("stride", 1), a.get("padding", "valid")
            cover, out, bn, relu, post_act = [n], n, None, 0, 0
            if own_act(n, L):
                relu = own_act(n, L)
                if relu > 2:
                    post_act, relu = relu, 0
            else:
                c1 = single(n)
                if c1 is not None and g.layers[c1].op == "bn":
                    bn = c1
                    cover.append(c1)
                    out = c1
                    c1 = single(c1)
                if 0 < act_mode(c1) <= 2:
                    relu = act_mode(c1)
                    cover.append(c1)
                    out = c1
            cv_out = out if not post_act else n + "#preact"
            steps.append(Step("deconv", cv_out, [R(L.inputs[0])], cover,
                              {"conv": n, "deconv": True, "bn": bn, "relu": relu, "stride": s,
                               "kernel": (kh, kw), "filters": a["filters"],
                               "pads": (deconv_pad_before(kh, s, padding), deconv_pad_before(kw, s, padding))}))
            if post_act:
                steps.append(Step("act", out, [cv_out], [], {"mode": post_act, "alpha": 0.3}))
            done.update(cover)
        elif L.op == "upsample":
            steps.append(Step("upsample", n, [R(L.inputs[0])], [n],
                              {"size": tuple(a["size"]), "bilinear": a.get("interpolation", "nearest") == "bilinear"}))
            done.add(n)
        elif L.op == "crop":
            steps.append(Step("crop", n, [R(L.inputs[0])], [n], {"crop": a["crop"]}))
            done.add(n)
        elif L.op in ("maxpool", "avgpool"):
            src = L.inputs[0]
            pads = ((0, 0), (0, 0))
            cover = [n]
            pad_zero = True                     # a folded ZeroPadding2D: the zeros take part
            if n in pad_fold:
                src, pads = pad_fold[n]
                cover = [L.inputs[0], n]
            if a.get("padding", "valid") == "same":
                pads = same(n, L, a["pool"])
                pad_zero = False                # Keras 'same' pooling ignores the padding
            if L.op == "avgpool" and n in pad_fold:
                raise NotImplementedError(f"ZeroPadding2D before AveragePooling2D ({n})")
            steps.append(Step(L.op, n, [R(src)], cover,
                              {"pool": a["pool"], "stride": a["stride"], "pads": pads, "pad_zero": pad_zero}))
            done.update(cover)
        elif L.op == "bn":
            cover = [n]
            relu = 0
            out = n
            c = single(n)
            if act_mode(c):
                relu = act_mode(c)
                cover.append(c)
                out = c
            steps.append(Step("bn", out, [R(L.inputs[0])], cover, {"bn": n, "relu": relu}))
            done.update(cover)
        elif L.op == "add":
            cover = [n]
            relu = 0
            out = n
            c = single(n)
            if act_mode(c):
                relu = act_mode(c)
                cover.append(c)
                out = c
            if len(L.inputs) != 2:
                raise NotImplementedError("add with != 2 inputs")
            steps.append(Step("add", out, [R(i) for i in L.inputs], cover, {"relu": relu}))
            done.update(cover)
        elif L.op == "relu":
            steps.append(Step("relu", n, [R(L.inputs[0])], [n], {"mode": act_mode(n)}))
            done.add(n)
        elif L.op == "act":
            steps.append(Step("act", n, [R(L.inputs[0])], [n],
                              {"mode": ACT_MODE[a["fn"]], "alpha": float(a.get("alpha", 0.3))}))
            done.add(n)
        elif L.op == "binary":
            cover = [n]
            out = n
            mode = 0
            c = single(n)
            if act_mode(c):
                mode = act_mode(c)
                cover.append(c)
                out = c
            steps.append(Step("binary", out, [R(i) for i in L.inputs], cover, {"fn": a["fn"], "act": mode}))
            done.update(cover)
        elif L.op in ("rescale", "normalization", "layerscale"):
            # a LayerScale that did not fold into its conv (a cut exposes the conv, or none precedes it)
            steps.append(Step("affine", n, [R(L.inputs[0])], [n], {"layer": n}))
            done.add(n)
        elif L.op == "layernorm":
            steps.append(Step("layernorm", n, [R(L.inputs[0])], [n],
                              {"layer": n, "eps": float(a.get("epsilon", 1e-3))}))
            done.add(n)
        elif L.op == "rmsnorm":
            steps.append(Step("rmsnorm", n, [R(L.inputs[0])], [n],
                              {"layer": n, "eps": float(a.get("epsilon", 1e-6))}))
            done.add(n)
        elif L.op == "groupnorm":
            cover = [n]
            out = n
            mode = 0
            c = single(n)
            if act_mode(c):
                mode = act_mode(c)
                cover.append(c)
                out = c
            steps.append(Step("groupnorm", out, [R(L.inputs[0])], cover,
                              {"layer": n, "groups": int(a["groups"]), "eps": float(a.get("epsilon", 1e-3)),
                               "act": mode}))
            done.update(cover)
        elif L.op in ("mha", "winattn"):
            h, d = int(a["num_heads"]), int(a["key_dim"])
            dv = int(a.get("value_dim") or d)
            tokens = 1
            for v in L.out_shape[:-1]:
                tokens *= v
            head = {"heads": h, "key_dim": d, "value_dim": dv}
            hkv = int(a.get("kv_heads") or h)
            if hkv != h:                        # only then: every other layer's steps are what they were
                head["kv_heads"] = hkv

            def proj(part: str, filters: int, res) -> Dict:
                # a Dense step whose weights the packers assemble from the layer's projections (graph/ir.py
                # mha_projection); "dense" keeps it out of the sibling merge
                return {"conv": n, "mha": part, "dense": True, "bn": None, "relu": 0, "residual": res,
                        "pads": ((0, 0), (0, 0)), "stride": 1, "kernel": (1, 1), "filters": filters,
                        "packed_input": False, **head}

            sq, sk, sv = ((R(t) for t in mha_sources(L.inputs, bool(a.get("key_mask")))) if L.op == "mha"
                          else (R(L.inputs[0]),) * 3)
            if sq == sk == sv:
                steps.append(Step("conv", n + "#qkv", [sq], [], proj("qkv", h * d + hkv * (d + dv), None)))
            if L.op == "winattn":               # on the (H, W, C) map, windows and shift resolved by the kernel
                steps.append(Step("winattn", n + "#ctx", [n + "#qkv"], [],
                                  {"layer": n, "height": L.out_shape[0], "width": L.out_shape[1],
                                   "window": int(a["window"]), "shift": int(a.get("shift", 0)), **head}))
            elif sq == sk == sv:
                core_in = n + "#qkv"
                if a.get("rope"):               # Q and K rotated out of place; the core reads the rotated rows
                    core_in = n + "#rot"
                    steps.append(Step("rope", core_in, [n + "#qkv"], [],
                                      {"layer": n, "tokens": tokens, "rope": float(a["rope"]), **head}))
                steps.append(Step("attention", n + "#ctx", [core_in], [], {"layer": n, "tokens": tokens, **head}))
                if a.get("rope"):
                    steps[-1].p["rope"] = float(a["rope"])
                if a.get("causal"):
                    steps[-1].p["causal"] = True
                if a.get("key_mask"):           # the (T,) mask tensor (the layer's last input) as a second input
                    steps[-1].ins.append(R(L.inputs[-1]))
                    steps[-1].p["key_mask"] = True
            else:
                # separate sources: one projection per distinct source tensor, the parts that share one side by
                # side ([Q | K] from `src + pos`, [K | V] when the key is the value); the core then reads Q, K and
                # V at (which input buffer, first column)
                if sq == sk:
                    parts = [("qk", sq), ("v", sv)]
                elif sk == sv:
                    parts = [("q", sq), ("kv", sk)]
                else:
                    parts = [("q", sq), ("k", sk), ("v", sv)]
                width = {"q": h * d, "k": h * d, "v": h * dv}
                where = {}
                for j, (part, src) in enumerate(parts):
                    steps.append(Step("conv", f"{n}#{part}", [src], [],
                                      proj(part, sum(width[c] for c in part), None)))
                    col = 0
                    for c in part:
                        where[c] = (j, col)
                        col += width[c]
                tokens_k = 1
                for v in g.layers[mha_sources(L.inputs, bool(a.get("key_mask")))[1]].out_shape[:-1]:
                    tokens_k *= v
                steps.append(Step("attention", n + "#ctx", [f"{n}#{part}" for part, _ in parts], [],
                                  {"layer": n, "tokens_q": tokens, "tokens_k": tokens_k, **where, **head}))
            cover = [n]
            res, out, relu = residual_add(n, cover)
            steps.append(Step("conv", out, [n + "#ctx"] + ([res] if res else []), cover,
                              proj("out", L.out_shape[-1], res)))
            steps[-1].p["relu"] = relu
            done.update(cover)
        elif L.op == "posembed":
            steps.append(Step("posembed", n, [R(L.inputs[0])], [n],
                              {"layer": n, "class_token": bool(a.get("class_token"))}))
            done.add(n)
        elif L.op == "embedding":
            steps.append(Step("embedding", n, [R(L.inputs[0])], [n], {"layer": n}))
            done.add(n)
        elif L.op == "queries":                 # the input only supplies the batch size
            steps.append(Step("queries", n, [R(L.inputs[0])], [n], {"layer": n}))
            done.add(n)
        elif L.op == "space_to_depth":
            steps.append(Step("space_to_depth", n, [R(L.inputs[0])], [n]))
            done.add(n)
        elif L.op == "gmp":
            steps.append(Step("gmp", n, [R(L.inputs[0])], [n]))
            done.add(n)
        elif L.op == "reshape":
            src_shape = g.layers[L.inputs[0]].out_shape
            if device_fusions and src_shape[-1] != L.out_shape[-1] and (src_shape[-1] % 8 or L.out_shape[-1] % 8):
                raise NotImplementedError(f"Reshape {src_shape} -> {L.out_shape} ({n}): channels are padded to 8")
            if n in outset:
                steps.append(Step("copy", n, [R(L.inputs[0])], [n]))
                done.add(n)
            else:
                alias[n] = alias.get(L.inputs[0], L.inputs[0])
                done.add(n)
                continue
        elif L.op == "concat":
            steps.append(Step("concat", n, [R(i) for i in L.inputs], [n],
                              {"channels": [g.layers[i].out_shape[-1] for i in L.inputs]}))
            done.add(n)
        elif L.op in ("identity", "flatten"):
            c = single(n)
            src_shape = g.layers[L.inputs[0]].out_shape
            if L.op == "identity" or (c is not None and g.layers[c].op == "dense"):
                if n in outset:                 # the slice must emit it under its own name
                    steps.append(Step("copy", n, [R(L.inputs[0])], [n]))
                else:
                    alias[n] = alias.get(L.inputs[0], L.inputs[0])
                    done.add(n)
                    continue
            else:
                steps.append(Step("copy", n, [R(L.inputs[0])], [n]))
            if device_fusions and L.op == "flatten" and len(src_shape) == 3 and src_shape[-1] % 8:
                raise NotImplementedError(f"Flatten of a {src_shape[-1]}-channel tensor ({n}): channels are padded to 8")
            done.add(n)
        elif L.op == "gap":
            steps.append(Step("gap", n, [R(L.inputs[0])], [n]))
            done.add(n)
        elif L.op == "dense":
            act = a.get("activation")
            mode = 0 if act == "softmax" else own_act(n, L)
            if mode > 2:                        # not an MFMA-epilogue activation: its own step
                steps.append(Step("dense", n + "#preact", [R(L.inputs[0])], [n],
                                  {"units": a["units"], "softmax": False, "relu": 0, "layer": n}))
                steps.append(Step("act", n, [n + "#preact"], [], {"mode": mode, "alpha": 0.3}))
            else:
                steps.append(Step("dense", n, [R(L.inputs[0])], [n],
                                  {"units": a["units"], "softmax": act == "softmax", "relu": mode, "layer": n}))
            done.add(n)
        elif L.op == "softmax":
            steps.append(Step("softmax", n, [R(L.inputs[0])], [n]))
            done.add(n)
        else:
            raise NotImplementedError(f"op {L.op}")
        produced.add(steps[-1].out)
    missing = [o for o in outputs if o not in produced]
    if missing:
        raise RuntimeError(f"plan does not produce outputs {missing}")
    if fp32 and not device_fusions:
        return steps
    if fp32:
        if os.environ.get("ADAPT_NO_STEM", "0") != "1":
            steps = _fuse_stem_f32(g, steps, outset)
        if os.environ.get("ADAPT_FUSED_PAIR_F32", "1") == "1":
            steps = fuse_pairs(g, steps, outset, fp32=True)
        # ADAPT_NO_SUBSAMPLE=1 keeps every tensor at full size (A/B runs, tests)
        if os.environ.get("ADAPT_NO_SUBSAMPLE", "0") != "1":
            steps = subsample_lattice(g, steps, outset)
        if os.environ.get("ADAPT_NO_SIBLINGS", "0") != "1":
            steps = merge_siblings(steps)
        return steps
    if os.environ.get("ADAPT_FUSED_BOTTLENECK", "1") == "1":
        steps = fuse_bottlenecks(g, steps, outset)
    # ADAPT_FUSED_PAIR=0 keeps the two launches (A/B: profiles/r2/experiments/pair/)
    if os.environ.get("ADAPT_FUSED_PAIR", "1") == "1":
        steps = fuse_pairs(g, steps, outset)
    if os.environ.get("ADAPT_NO_STEM", "0") != "1":
        steps = _fuse_stem(g, steps, outset)
    if os.environ.get("ADAPT_NO_SIBLINGS", "0") != "1":
        steps = merge_siblings(steps)
    return steps


def fuse_bottlenecks(g: Graph, steps: List[Step], outset: Set[str]) -> List[Step]:
    """1x1 (->64, ReLU) -> 3x3 s1 p1 (64->64, ReLU) -> 1x1 (64->256) + shortcut + ReLU
    ==> one ``bottleneck`` step (csrc/kernels/bottleneck.hip) when the block's
    input is H x W x 256 (identity shortcut) or H x W x 64 with a stride-1 1x1
    projection shortcut, H and W multiples of 8, and no intermediate tensor is
    needed elsewhere (a cut inside the block keeps it unfused).  ResNet
    stage 2: three launches and two 51 MB round trips per block become one."""
    def users(t: str) -> List[int]:
        return [j for j, st in enumerate(steps) if t in st.ins]

    def conv(j, k, filters, relu, res):
        st = steps[j]
        p = st.p
        return (st.kind == "conv" and p.get("kernel") == k and p.get("stride") == 1 and p.get("filters") == filters
                and p.get("relu") == relu and bool(p.get("residual")) == res and not p.get("packed_input")
                and not p.get("sibling"))

    drop: Set[int] = set()
    repl: Dict[int, Step] = {}
    for j3, s3 in enumerate(steps):
        if j3 in drop or not conv(j3, (1, 1), 256, 1, True):
            continue
        y2, sc = s3.ins[0], s3.ins[1]
        u2 = [j for j, st in enumerate(steps) if st.out == y2]
        if len(u2) != 1 or y2 in outset or users(y2) != [j3] or not conv(u2[0], (3, 3), 64, 1, False):
            continue
        j2 = u2[0]
        if steps[j2].p["pads"] != ((1, 1), (1, 1)):
            continue
        y1 = steps[j2].ins[0]
        u1 = [j for j, st in enumerate(steps) if st.out == y1]
        if len(u1) != 1 or y1 in outset or users(y1) != [j2] or not conv(u1[0], (1, 1), 64, 1, False):
            continue
        j1 = u1[0]
        x = steps[j1].ins[0]
        xl = g.layers[x.split("#")[0]]
        if len(xl.out_shape) != 3 or xl.out_shape[0] % 8 or xl.out_shape[1] % 8:
            continue
        proj = None
        if sc == x and xl.out_shape[2] == 256:
            pass                                          # identity shortcut
        elif xl.out_shape[2] == 64:
            up = [j for j, st in enumerate(steps) if st.out == sc]
            if (len(up) != 1 or sc in outset or users(sc) != [j3] or not conv(up[0], (1, 1), 256, 0, False)
                    or steps[up[0]].ins[0] != x):
                continue
            proj = up[0]
        else:
            continue
        group = [j1, j2, j3] + ([proj] if proj is not None else [])
        covers = [c for jj in sorted(group) for c in steps[jj].covers]
        p = {"c1": steps[j1].p, "c2": steps[j2].p, "c3": steps[j3].p,
             "proj": steps[proj].p if proj is not None else None, "cin": xl.out_shape[2]}
        repl[j3] = Step("bottleneck", s3.out, [x], covers, p)
        drop.update(jj for jj in group if jj != j3)
    return [repl.get(j, st) for j, st in enumerate(steps) if j not in drop]


def fuse_pairs(g: Graph, steps: List[Step], outset: Set[str], fp32: bool = False) -> List[Step]:
    """1x1 (CIN -> CO) + BN + residual + ReLU (block k's ``_out``) followed by the
    1x1 (CO -> CM) + BN + ReLU that is the next block's ``_1`` ==> one ``pair``
    step with two outputs (csrc/kernels/pw_pair.hip): y is still written (it is
    the next residual) but the second GEMM reads it from LDS, and the pair is
    one launch.  Only the stride-1 pairs inside a ResNet stage qualify.  Both
    outputs land in their own named buffers, so either may be a slice frontier.
    fp32: csrc/kernels/pw_pair_f32.hip, ResNet stage 2 (64 -> 256 -> 64) only."""
    from ..ops.conv import pair_f32_supported, pair_supported   # static shape tables, no device needed

    def conv1x1(st: Step, relu: int, res: bool) -> bool:
        p = st.p
        return (st.kind == "conv" and p.get("kernel") == (1, 1) and p.get("stride") == 1
                and p.get("pads") == ((0, 0), (0, 0)) and p.get("relu") == relu and bool(p.get("residual")) == res
                and not p.get("packed_input") and not p.get("sibling"))

    drop: Set[int] = set()
    repl: Dict[int, Step] = {}
    for ja, a in enumerate(steps):
        if ja in drop or ja in repl or not conv1x1(a, 1, True):
            continue
        users = [j for j, st in enumerate(steps) if a.out in st.ins]
        firsts = [j for j in users if steps[j].ins[0] == a.out and conv1x1(steps[j], 1, False)
                  and len(steps[j].ins) == 1]
        if len(firsts) != 1 or firsts[0] <= ja or firsts[0] in repl:
            continue
        jb = firsts[0]
        b = steps[jb]
        xl = g.layers[a.ins[0].split("#")[0]]
        if len(xl.out_shape) != 3:
            continue
        cin, co, cm = xl.out_shape[2], a.p["filters"], b.p["filters"]
        if not (pair_f32_supported(cin, co, cm) if fp32 else pair_supported(cin, co, cm)):
            continue
        p = {"c3": a.p, "c1": b.p, "out2": b.out, "cin": cin, "co": co, "cm": cm}
        repl[ja] = Step("pair", a.out, list(a.ins), a.covers + b.covers, p)
        drop.add(jb)
    return [repl.get(j, st) for j, st in enumerate(steps) if j not in drop]


def merge_siblings(steps: List[Step]) -> List[Step]:
    """Two 1x1 convs that read the same tensor with the same stride and no
    residual become ONE GEMM with N = N0 + N1 and two outputs: ResNet's
    projection shortcut ``conv{s}_block1_0`` and ``conv{s}_block1_1`` (one
    launch and one read of the block input instead of two; the kernels route
    columns >= N0 to the second output, csrc/kernels/kernels.h `epi_dst`).
    The merged step sits at the first sibling's position (its input is ready
    there); the second output merely becomes available earlier."""
    out: List[Step] = []
    taken: Set[int] = set()
    for i, st in enumerate(steps):
        if i in taken:
            continue
        p = st.p
        if (st.kind == "conv" and not p.get("residual") and p.get("kernel") == (1, 1) and not p.get("packed_input")
                and not p.get("dense")):
            for j in range(i + 1, min(i + 4, len(steps))):
                sj = steps[j]
                q = sj.p
                if (j not in taken and sj.kind == "conv" and sj.ins[0] == st.ins[0] and not q.get("residual")
                        and not q.get("dense")
                        and q.get("kernel") == (1, 1) and q["stride"] == p["stride"] and q["pads"] == p["pads"]
                        and p["filters"] % 256 == 0 and q["filters"] % 8 == 0):
                    # nothing between them may consume the first sibling's output before
                    # ... (it is produced at i either way) -- only the second moves earlier
                    p["sibling"] = dict(q)
                    p["out2"] = sj.out
                    p["relu2"] = q["relu"]
                    st.covers = st.covers + sj.covers
                    taken.add(j)
                    break
        out.append(st)
    return out


_NO_PADS = ((0, 0), (0, 0))


def subsample_lattice(g: Graph, steps: List[Step], outset: Set[str]) -> List[Step]:
    """A tensor that is only ever sampled on a lattice is produced only on that lattice (fp32 device plan).

    Keras ResNet v1 puts the stride 2 of stages 3-5 on the two 1x1 convs ``conv{s}_block1_0_conv`` and
    ``conv{s}_block1_1_conv``: they read pixels (2i, 2j) of the previous stage's last ``_out`` tensor, so 3/4 of
    that tensor is computed, added to its residual, written and never read.  When every reader of a tensor T
    is ``ins[0]`` of a pad-free 1x1 conv with one common stride s > 1, and T's producer P is a pad-free 1x1 /
    stride-1 conv (a fused residual and any activation allowed), then "conv, keep pixels (s i, s j)" is the
    stride-s conv of P's input:

    * P becomes that stride-s conv (`p["stride"] = p["subsample"] = s`) and writes the compact
      (ceil(H / s), ceil(W / s)) map `p["out_hw"]` (`compact_maps` / `tensor_shape`);
    * its residual stays the full-resolution tensor, read at the same pixels (`p["res_stride"] = s`);
    * the readers become stride-1 convs of the compact map (`p["in_subsample"] = s` records it), which
      `merge_siblings` merges as before.

    T keeps its name and kind.  A T the slice emits (an output or a cut frontier), a T some step takes as
    its residual, a reader of another kind, stride or padding: any of these keeps T full size."""
    for P in steps:
        p, T = P.p, P.out
        if (P.kind != "conv" or p.get("kernel") != (1, 1) or p.get("stride") != 1 or p.get("pads") != _NO_PADS
                or p.get("sibling") or p.get("out2") or p.get("packed_input") or p.get("mha")
                or T in outset or T not in g.layers or len(g.layers[T].out_shape) != 3):
            continue
        readers = [st for st in steps if T in st.ins]
        if not readers or any(st.kind != "conv" or st.ins[0] != T or T in st.ins[1:]
                              or st.p.get("kernel") != (1, 1) or st.p.get("pads") != _NO_PADS
                              or st.p.get("packed_input") or st.p.get("sibling") for st in readers):
            continue
        strides = {st.p.get("stride") for st in readers}
        if len(strides) != 1:
            continue
        s = strides.pop()
        if not isinstance(s, int) or s <= 1:
            continue
        h, w = g.layers[T].out_shape[:2]
        p["stride"] = p["subsample"] = s
        p["out_hw"] = (-(-h // s), -(-w // s))
        if p.get("residual"):
            p["res_stride"] = s
        for st in readers:
            st.p["stride"] = 1
            st.p["in_subsample"] = s
        _subsample_front_3x3(g, steps, outset, P, s)
        _mark_live_lattice(g, steps, outset, P, s)
    return steps


# (input channels, H, W) of the 3x3 convs in front of a subsampled 1x1 that are strided too by default.  Empty:
# on ResNet-50 at batch 32 the direct stride-2 3x3 measured faster in the whole graph than the full-map Winograd
# conv on all three stages, (64, 56, 56), (128, 28, 28) and (256, 14, 14), but the suite
# pins every ResNet-50 3x3 to a Winograd kernel (tests/test_fp32_gpu.py), so taking them is left to a change that
# also moves that test.  ADAPT_SUBSAMPLE_3X3=1 takes every such 3x3, =0 none, and a list such as
# 64x56x56,256x14x14 exactly those (per-stage A/B runs).
# The default path lives one level down instead: a 3x3 left as it is gets `p["live_lattice"] = s`
# (_mark_live_lattice) and keeps its plan step, its Winograd config family and its full-size buffer, and the
# F(4x4) split kernels compute only the sampled pixels of it (csrc/kernels/wino4s_f32.hip, even lattice).
SUBSAMPLE_3X3_MEASURED: Set[tuple] = set()


def _front_3x3(g: Graph, steps: List[Step], outset: Set[str], P: Step) -> Optional[Step]:
    """The 3x3 / stride-1 / pad-1 conv whose output only `P` reads and the slice does not emit, or None."""
    cand = [st for st in steps if st.out == P.ins[0]]
    if len(cand) != 1:
        return None
    Q = cand[0]
    q = Q.p
    if (Q.kind != "conv" or q.get("kernel") != (3, 3) or q.get("stride") != 1 or q.get("pads") != ((1, 1), (1, 1))
            or q.get("residual") or q.get("sibling") or q.get("out2") or q.get("packed_input")
            or Q.out in outset or Q.out not in g.layers or [st for st in steps if Q.out in st.ins] != [P]):
        return None
    return Q


def _shape_list(text: str) -> Set[tuple]:
    return {tuple(int(v) for v in t.split("x")) for t in text.split(",") if "x" in t}


def _mark_live_lattice(g: Graph, steps: List[Step], outset: Set[str], P: Step, s: int) -> None:
    """The 3x3 in front of a subsampled 1x1 `P` that `_subsample_front_3x3` left as it is: P reads only pixels
    (s i, s j) of its full-size output, which `p["live_lattice"] = s` records and nothing else of the plan
    changes.  A launch of that step must write those pixels and may leave the others alone (ops/conv.py
    conv_forward_f32).  ADAPT_NO_LIVE_LATTICE=1 leaves the mark off; ADAPT_LIVE_LATTICE=64x56x56,256x14x14
    marks exactly the listed (input channels, H, W) (per-stage A/B runs)."""
    if os.environ.get("ADAPT_NO_LIVE_LATTICE", "0") == "1":
        return
    Q = _front_3x3(g, steps, outset, P)
    if Q is None:
        return
    only = os.environ.get("ADAPT_LIVE_LATTICE")
    if only is not None:
        h, w = g.layers[Q.out].out_shape[:2]
        cin = g.layers[Q.ins[0].split("#")[0]].out_shape[-1]
        if (cin, h, w) not in _shape_list(only):
            return
    Q.p["live_lattice"] = s


def _subsample_front_3x3(g: Graph, steps: List[Step], outset: Set[str], P: Step, s: int) -> None:
    """One step back from a subsampled 1x1 `P`: the 3x3 / stride-1 / pad-1 conv Q whose output only P reads
    needs only outputs (s i, s j) too.  It becomes a stride-s 3x3 with top / left pad 1 and the bottom / right
    pad that makes its last sampled output the full conv's (0 for even H at s = 2); P then reads a dense compact
    x at stride 1 and still samples its residual (`res_stride` is independent of the conv's stride).  The
    stride-s 3x3 leaves the Winograd kernels for the direct tile kernels; which 3x3s are taken:
    SUBSAMPLE_3X3_MEASURED / ADAPT_SUBSAMPLE_3X3."""
    mode = os.environ.get("ADAPT_SUBSAMPLE_3X3", "auto")
    Q = None if mode == "0" else _front_3x3(g, steps, outset, P)
    if Q is None:
        return
    q = Q.p
    h, w = g.layers[Q.out].out_shape[:2]
    cin = g.layers[Q.ins[0].split("#")[0]].out_shape[-1]
    chosen = SUBSAMPLE_3X3_MEASURED if mode == "auto" else _shape_list(mode)
    if mode != "1" and (cin, h, w) not in chosen:
        return
    oh, ow = P.p["out_hw"]
    q["stride"] = q["subsample"] = s
    q["pads"] = ((1, max(0, s * (oh - 1) + 2 - h)), (1, max(0, s * (ow - 1) + 2 - w)))
    q["out_hw"] = (oh, ow)
    P.p["stride"] = 1


STEM_MAX_OW = 112     # csrc/kernels/stem.hip ST_OWMAX


def _fuse_stem_f32(g: Graph, steps: List[Step], outset: Set[str]) -> List[Step]:
    """fp32 path: conv(image, 7x7/s2, 3 -> 64, BN+ReLU) -> maxpool 3x3/s2 pad 1  ==>  one
    ``stem_f32`` step (csrc/kernels/stem_f32.hip).  The image is the conv's
    input as it is (the fp32 plan has no pack step)."""
    def users(t: str) -> List[int]:
        return [j for j, s in enumerate(steps) if t in s.ins]

    for i, cv in enumerate(steps):
        if (cv.kind != "conv" or len(cv.ins) != 1 or cv.p.get("dense") or cv.ins[0] not in g.layers
                or g.layers[cv.ins[0]].op != "input"):
            continue
        p = cv.p
        h, w, c = g.layers[cv.ins[0]].out_shape
        oh, ow = g.layers[p["conv"]].out_shape[:2]
        (pt, _), (pl, _) = p["pads"]
        if (p["kernel"] != (7, 7) or p["stride"] != 2 or p["filters"] != 64 or p["relu"] != 1 or p["residual"]
                or c != 3 or w % 4 or ow > STEM_MAX_OW or pl != 3 or cv.out in outset):
            continue
        mu = users(cv.out)
        if len(mu) != 1 or steps[mu[0]].kind != "maxpool":
            continue
        mp = steps[mu[0]]
        if not (mp.p["pool"] in (3, (3, 3)) and mp.p["stride"] in (2, (2, 2)) and mp.p["pads"] == ((1, 1), (1, 1))):
            continue
        stem = Step("stem_f32", mp.out, [cv.ins[0]], list(cv.covers) + list(mp.covers),
                    {"conv": p["conv"], "bn": p["bn"], "pads": p["pads"], "pool": True, "pool_pad": 1,
                     "filters": 64})
        return [stem if j == i else s for j, s in enumerate(steps) if j != mu[0]]
    return steps


def _fuse_stem(g: Graph, steps: List[Step], outset: Set[str]) -> List[Step]:
    """pack -> conv(7x7/s2, 64 filters, BN+ReLU) [-> maxpool 3x3/s2 pad 1]  ==>  one ``stem`` step."""
    def users(t: str) -> List[int]:
        return [j for j, s in enumerate(steps) if t in s.ins]

    for i, st in enumerate(steps):
        if st.kind != "pack" or st.p["cin"] > 4:
            continue
        u = users(st.out)
        if len(u) != 1 or steps[u[0]].kind != "conv":
            continue
        cv = steps[u[0]]
        p = cv.p
        oh, ow = g.layers[p["conv"]].out_shape[:2]
        if (p["kernel"] != (7, 7) or p["stride"] != 2 or p["filters"] != 64 or p["relu"] != 1 or p["residual"]
                or ow > STEM_MAX_OW):
            continue
        drop = {i, u[0]}
        covers = list(cv.covers)
        out = cv.out
        pool = None
        mu = users(cv.out)
        if cv.out not in outset and len(mu) == 1 and steps[mu[0]].kind == "maxpool":
            mp = steps[mu[0]]
            if mp.p["pool"] in (3, (3, 3)) and mp.p["stride"] in (2, (2, 2)) and mp.p["pads"] == ((1, 1), (1, 1)):
                pool = mp.p["pads"][0][0]
                covers += mp.covers
                out = mp.out
                drop.add(mu[0])
        stem = Step("stem", out, [st.ins[0]], covers,
                    {"conv": p["conv"], "bn": p["bn"], "pads": p["pads"], "pool": pool is not None,
                     "pool_pad": pool or 0, "filters": 64})
        first = min(drop)
        return [stem if j == first else s for j, s in enumerate(steps) if j == first or j not in drop]
    return steps
