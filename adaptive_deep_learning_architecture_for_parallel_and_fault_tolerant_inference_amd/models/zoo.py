"""Other `tf.keras.applications` families, rebuilt in our IR with Keras layer
names, creation order and `get_weights()` order.

The reference's dispatcher is model-agnostic: `DEFER.run_defer(model, ...)`
takes any Keras functional model and `dag_util.construct_model` cuts it at
named layers (`src/dispatcher.py:39-53`, `src/dag_util.py:50-62`); its demo
happens to use ResNet50 (`test/test.py:13`).  These builders give that
generality a concrete footing beyond ResNet (and `graph/keras_json.py`
takes an arbitrary Keras JSON):

* VGG16 / VGG19  (plain conv stacks, Conv2D(activation='relu'), Flatten, Dense relu)
* MobileNetV2    (ReLU6, DepthwiseConv2D, 'same' padding at stride 2, inverted residuals)
* DenseNet121/169/201 (pre-activation BN-ReLU, Concatenate, AveragePooling2D)
* EfficientNetB0-B7   (Rescaling/Normalization inside the model, swish, squeeze-excite Multiply)
* InceptionV3         (BatchNormalization(scale=False), asymmetric 1x7 / 7x1 kernels, multi-branch concats)
* ResNeXt-50 / -101 (32x4d)  (Conv2D(groups=32) 3x3 in every block, ResNet layer names)
* ConvNeXt-Tiny ... -XLarge  (LayerNormalization, Dense on (H, W, C), LayerScale, a 7x7 Conv2D(groups=C))
* ViT-Ti / S / B / L at patch 16  (MultiHeadAttention as self-attention, class token + position embedding)
* Swin-Tiny / Small / Base / Large at patch 4, window 7  (WindowAttention with relative position bias and
  shifted windows, SpaceToDepth patch merging)

Parameter totals (Keras, include_top, 1000 classes; checked by tests):
VGG16 138,357,544; VGG19 143,667,240; MobileNetV2 3,538,984; DenseNet121 8,062,504;
EfficientNetB0 5,330,571; InceptionV3 23,851,784; ResNeXt50 25,097,128; ResNeXt101 44,315,560;
ConvNeXt Tiny 28,589,128, Small 50,223,688, Base 88,591,464, Large 197,767,336, XLarge 350,196,968;
ViT (published sizes, patch 16) Ti 5,717,416, S 22,050,664, B 86,567,656, L 304,326,632;
Swin (published sizes) Tiny 28,288,354, Small 49,606,258, Base 87,768,224, Large 196,532,476.

Not from `keras.applications` (models whose output is a map, not a class vector):

* U-Net (`unet`, `unet_bilinear`, test size `unet_tiny`): Conv2DTranspose or UpSampling2D decoders, skip
  Concatenates; 31,031,745 parameters at base 64, depth 4, one class, RGB input.
* Stable Diffusion VAE decoder (`sd_vae_decoder`, test size `vae_decoder_micro`): GroupNormalization + swish
  residual blocks, one-head MultiHeadAttention on the (H, W, C) map, nearest UpSampling2D; a 64 x 64 x 4 latent
  to a 512 x 512 x 3 image, 49,490,199 parameters (the published decoder's 49,490,179 and the 20 of the 1x1
  post-quantisation conv in front of it).
* DETR (`detr_resnet50`, test size `detr_micro`): the ResNet-50 backbone, a post-norm transformer encoder and
  decoder whose MultiHeadAttention layers take separate query / key / value tensors, LearnedQueries for the object
  queries and the position table; a 480 x 640 x 3 image to (1, 100, 96) class logits and boxes, 41,759,968
  parameters (Keras counting: BatchNormalization statistics, conv biases and the two tables included).
* Llama (`tinyllama_1_1b`, `llama2_7b`, test size `llama_micro`): RMSNormalization, a rotary position embedding on
  Q and K, causal grouped-query attention and the SwiGLU MLP, no bias anywhere; (T,) token ids to the next-token
  logits, the published 1,100,048,384 and 6,738,415,616 parameters.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

from ..graph.ir import Graph, Layer, with_key_masks


def _conv(g: Graph, x: str, name: str, filters: int, k: int, stride: int = 1, padding: str = "valid",
          use_bias: bool = True, activation=None) -> str:
    a = {"filters": filters, "kernel": (k, k), "stride": stride, "padding": padding, "use_bias": use_bias}
    if activation:
        a["activation"] = activation
    return g.add(Layer(name, "conv", [x], a))


# ------------------------------------------------------------------- VGG
VGG_BLOCKS = {"vgg16": (2, 2, 3, 3, 3), "vgg19": (2, 2, 4, 4, 4)}


def build_vgg(name: str = "vgg16", classes: int = 1000, input_shape=(224, 224, 3)) -> Graph:
    """`keras.applications.vgg16/vgg19` with include_top=True."""
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": tuple(input_shape)}))
    for b, (n, f) in enumerate(zip(VGG_BLOCKS[name], (64, 128, 256, 512, 512)), start=1):
        for i in range(1, n + 1):
            x = _conv(g, x, f"block{b}_conv{i}", f, 3, padding="same", activation="relu")
        x = g.add(Layer(f"block{b}_pool", "maxpool", [x], {"pool": 2, "stride": 2, "padding": "valid"}))
    x = g.add(Layer("flatten", "flatten", [x]))
    x = g.add(Layer("fc1", "dense", [x], {"units": 4096, "activation": "relu", "use_bias": True}))
    x = g.add(Layer("fc2", "dense", [x], {"units": 4096, "activation": "relu", "use_bias": True}))
    g.add(Layer("predictions", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = ["predictions"]
    return g


# ------------------------------------------------------------- MobileNetV2
MBV2_EPS = 1e-3
# (filters, stride, expansion) per inverted-residual block, block_id = index
MBV2_BLOCKS = [(16, 1, 1), (24, 2, 6), (24, 1, 6), (32, 2, 6), (32, 1, 6), (32, 1, 6), (64, 2, 6), (64, 1, 6),
               (64, 1, 6), (64, 1, 6), (96, 1, 6), (96, 1, 6), (96, 1, 6), (160, 2, 6), (160, 1, 6), (160, 1, 6),
               (320, 1, 6)]


def _make_divisible(v: float, divisor: int = 8) -> int:
    new_v = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new_v + divisor if new_v < 0.9 * v else new_v


def build_mobilenet_v2(name: str = "mobilenetv2_1.00_224", classes: int = 1000, input_shape=(224, 224, 3),
                       alpha: float = 1.0) -> Graph:
    """`keras.applications.MobileNetV2(alpha=1.0, include_top=True)`."""
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": tuple(input_shape)}))
    x = _conv(g, x, "Conv1", _make_divisible(32 * alpha), 3, stride=2, padding="same", use_bias=False)
    x = g.add(Layer("bn_Conv1", "bn", [x], {"epsilon": MBV2_EPS}))
    x = g.add(Layer("Conv1_relu", "relu", [x], {"max_value": 6.0}))
    for block_id, (filters, stride, expansion) in enumerate(MBV2_BLOCKS):
        inp = x
        cin = g.layers[x].out_shape[-1]
        out_c = _make_divisible(int(filters * alpha), 8)
        if block_id:
            prefix = f"block_{block_id}_"
            x = _conv(g, x, prefix + "expand", expansion * cin, 1, padding="same", use_bias=False)
            x = g.add(Layer(prefix + "expand_BN", "bn", [x], {"epsilon": MBV2_EPS}))
            x = g.add(Layer(prefix + "expand_relu", "relu", [x], {"max_value": 6.0}))
        else:
            prefix = "expanded_conv_"
        if stride == 2:
            h = g.layers[x].out_shape[0]
            adj = 1 - h % 2                    # imagenet_utils.correct_pad(x, 3)
            x = g.add(Layer(prefix + "pad", "zeropad", [x], {"pad": ((1 - adj, 1), (1 - adj, 1))}))
        x = g.add(Layer(prefix + "depthwise", "dwconv", [x],
                        {"kernel": (3, 3), "stride": stride, "padding": "same" if stride == 1 else "valid",
                         "use_bias": False}))
        x = g.add(Layer(prefix + "depthwise_BN", "bn", [x], {"epsilon": MBV2_EPS}))
        x = g.add(Layer(prefix + "depthwise_relu", "relu", [x], {"max_value": 6.0}))
        x = _conv(g, x, prefix + "project", out_c, 1, padding="same", use_bias=False)
        x = g.add(Layer(prefix + "project_BN", "bn", [x], {"epsilon": MBV2_EPS}))
        if cin == out_c and stride == 1:
            x = g.add(Layer(prefix + "add", "add", [inp, x]))
    last = _make_divisible(1280 * alpha, 8) if alpha > 1.0 else 1280
    x = _conv(g, x, "Conv_1", last, 1, use_bias=False)
    x = g.add(Layer("Conv_1_bn", "bn", [x], {"epsilon": MBV2_EPS}))
    x = g.add(Layer("out_relu", "relu", [x], {"max_value": 6.0}))
    x = g.add(Layer("global_average_pooling2d", "gap", [x]))
    g.add(Layer("predictions", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = ["predictions"]
    return g


# ---------------------------------------------------------------- DenseNet
DENSENET_BLOCKS = {"densenet121": (6, 12, 24, 16), "densenet169": (6, 12, 32, 32), "densenet201": (6, 12, 48, 32)}
DN_EPS = 1.001e-5


def build_densenet(name: str = "densenet121", classes: int = 1000, input_shape=(224, 224, 3)) -> Graph:
    """`keras.applications.DenseNet121/169/201(include_top=True)`."""
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": tuple(input_shape)}))
    x = g.add(Layer("zero_padding2d", "zeropad", [x], {"pad": ((3, 3), (3, 3))}))
    x = _conv(g, x, "conv1/conv", 64, 7, stride=2, use_bias=False)
    x = g.add(Layer("conv1/bn", "bn", [x], {"epsilon": DN_EPS}))
    x = g.add(Layer("conv1/relu", "relu", [x]))
    x = g.add(Layer("zero_padding2d_1", "zeropad", [x], {"pad": ((1, 1), (1, 1))}))
    x = g.add(Layer("pool1", "maxpool", [x], {"pool": 3, "stride": 2, "padding": "valid"}))
    blocks = DENSENET_BLOCKS[name]
    for s, n in enumerate(blocks, start=2):
        for i in range(1, n + 1):
            p = f"conv{s}_block{i}"
            y = g.add(Layer(p + "_0_bn", "bn", [x], {"epsilon": DN_EPS}))
            y = g.add(Layer(p + "_0_relu", "relu", [y]))
            y = _conv(g, y, p + "_1_conv", 128, 1, use_bias=False)
            y = g.add(Layer(p + "_1_bn", "bn", [y], {"epsilon": DN_EPS}))
            y = g.add(Layer(p + "_1_relu", "relu", [y]))
            y = _conv(g, y, p + "_2_conv", 32, 3, padding="same", use_bias=False)
            x = g.add(Layer(p + "_concat", "concat", [x, y]))
        if s < 2 + len(blocks) - 1:
            p = f"pool{s}"
            c = g.layers[x].out_shape[-1]
            y = g.add(Layer(p + "_bn", "bn", [x], {"epsilon": DN_EPS}))
            y = g.add(Layer(p + "_relu", "relu", [y]))
            y = _conv(g, y, p + "_conv", int(c * 0.5), 1, use_bias=False)
            x = g.add(Layer(p + "_pool", "avgpool", [y], {"pool": 2, "stride": 2, "padding": "valid"}))
    x = g.add(Layer("bn", "bn", [x], {"epsilon": DN_EPS}))
    x = g.add(Layer("relu", "relu", [x]))
    x = g.add(Layer("avg_pool", "gap", [x]))
    g.add(Layer("predictions", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = ["predictions"]
    return g


# ---------------------------------------------------------------- EfficientNet
EFFNET_BLOCKS = [  # kernel, repeats, filters_in, filters_out, expand_ratio, strides (se_ratio 0.25, id_skip)
    (3, 1, 32, 16, 1, 1), (3, 2, 16, 24, 6, 2), (5, 2, 24, 40, 6, 2), (3, 3, 40, 80, 6, 2),
    (5, 3, 80, 112, 6, 1), (5, 4, 112, 192, 6, 2), (3, 1, 192, 320, 6, 1)]
EFFNET_SCALE = {  # width, depth, resolution
    "efficientnetb0": (1.0, 1.0, 224), "efficientnetb1": (1.0, 1.1, 240), "efficientnetb2": (1.1, 1.2, 260),
    "efficientnetb3": (1.2, 1.4, 300), "efficientnetb4": (1.4, 1.8, 380), "efficientnetb5": (1.6, 2.2, 456),
    "efficientnetb6": (1.8, 2.6, 528), "efficientnetb7": (2.0, 3.1, 600)}


def build_efficientnet(name: str = "efficientnetb0", classes: int = 1000, input_shape=None) -> Graph:
    """`keras.applications.EfficientNetB0..B7(include_top=True, weights=None)` (tf.keras 2.15): Rescaling +
    Normalization preprocessing inside the model, swish, squeeze-excite (GAP -> Reshape -> 1x1 swish ->
    1x1 sigmoid -> Multiply), drop-connect Dropout before the residual Add (identity at inference)."""
    import math
    width, depth, res = EFFNET_SCALE[name]
    input_shape = tuple(input_shape or (res, res, 3))

    def round_filters(f: float) -> int:
        f *= width
        new = max(8, int(f + 4) // 8 * 8)
        return int(new + 8 if new < 0.9 * f else new)

    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": input_shape}))
    x = g.add(Layer("rescaling", "rescale", [x], {"scale": 1.0 / 255.0, "offset": 0.0}))
    x = g.add(Layer("normalization", "normalization", [x]))

    def correct_pad(t: str, k: int):
        h = g.layers[t].out_shape[0]
        adj = 1 - h % 2
        c = k // 2
        return ((c - adj, c), (c - adj, c))

    x = g.add(Layer("stem_conv_pad", "zeropad", [x], {"pad": correct_pad(x, 3)}))
    x = _conv(g, x, "stem_conv", round_filters(32), 3, stride=2, use_bias=False)
    x = g.add(Layer("stem_bn", "bn", [x], {"epsilon": 1e-3}))
    x = g.add(Layer("stem_activation", "act", [x], {"fn": "swish"}))
    total = float(sum(int(math.ceil(depth * r)) for _, r, *_ in EFFNET_BLOCKS))
    b = 0
    for i, (k, reps, f_in, f_out, expand, stride) in enumerate(EFFNET_BLOCKS):
        f_in, f_out = round_filters(f_in), round_filters(f_out)
        for j in range(int(math.ceil(depth * reps))):
            if j > 0:
                stride, f_in = 1, f_out
            p = f"block{i + 1}{chr(j + 97)}_"
            drop_rate = 0.2 * b / total
            inp = x
            filters = f_in * expand
            if expand != 1:
                x = _conv(g, x, p + "expand_conv", filters, 1, padding="same", use_bias=False)
                x = g.add(Layer(p + "expand_bn", "bn", [x], {"epsilon": 1e-3}))
                x = g.add(Layer(p + "expand_activation", "act", [x], {"fn": "swish"}))
            if stride == 2:
                x = g.add(Layer(p + "dwconv_pad", "zeropad", [x], {"pad": correct_pad(x, k)}))
            x = g.add(Layer(p + "dwconv", "dwconv", [x], {"kernel": (k, k), "stride": stride,
                                                        "padding": "valid" if stride == 2 else "same",
                                                        "use_bias": False}))
            x = g.add(Layer(p + "bn", "bn", [x], {"epsilon": 1e-3}))
            x = g.add(Layer(p + "activation", "act", [x], {"fn": "swish"}))
            se_f = max(1, int(f_in * 0.25))
            se = g.add(Layer(p + "se_squeeze", "gap", [x]))
            se = g.add(Layer(p + "se_reshape", "reshape", [se], {"shape": (1, 1, filters)}))
            se = _conv(g, se, p + "se_reduce", se_f, 1, padding="same", activation="swish")
            se = _conv(g, se, p + "se_expand", filters, 1, padding="same", activation="sigmoid")
            x = g.add(Layer(p + "se_excite", "binary", [x, se], {"fn": "mul"}))
            x = _conv(g, x, p + "project_conv", f_out, 1, padding="same", use_bias=False)
            x = g.add(Layer(p + "project_bn", "bn", [x], {"epsilon": 1e-3}))
            if stride == 1 and f_in == f_out:
                if drop_rate > 0:
                    x = g.add(Layer(p + "drop", "identity", [x]))
                x = g.add(Layer(p + "add", "add", [x, inp]))
            b += 1
    x = _conv(g, x, "top_conv", round_filters(1280), 1, padding="same", use_bias=False)
    x = g.add(Layer("top_bn", "bn", [x], {"epsilon": 1e-3}))
    x = g.add(Layer("top_activation", "act", [x], {"fn": "swish"}))
    x = g.add(Layer("avg_pool", "gap", [x]))
    x = g.add(Layer("top_dropout", "identity", [x]))
    g.add(Layer("predictions", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = ["predictions"]
    return g


# ------------------------------------------------------------- InceptionV3
def build_inception_v3(name: str = "inception_v3", classes: int = 1000, input_shape=(299, 299, 3)) -> Graph:
    """`keras.applications.InceptionV3(include_top=True)`.  Its conv2d_bn units are unnamed, so the
    layers carry Keras' auto-names of a fresh session (conv2d, conv2d_1, ..., batch_normalization_N,
    activation_N, max_pooling2d_N, average_pooling2d_N, concatenate_N) in creation order;
    BatchNormalization(scale=False) (no gamma), asymmetric 1x7 / 7x1 / 1x3 / 3x1 kernels.
    Weight-list order follows creation order: Keras' own `get_weights()` order for this
    multi-branch graph is unpinned here (no TensorFlow to compare with)."""
    g = Graph(name)
    cnt: Dict[str, int] = {}

    def auto(kind: str) -> str:
        i = cnt.get(kind, 0)
        cnt[kind] = i + 1
        return kind if i == 0 else f"{kind}_{i}"

    def cbn(x: str, f: int, kh: int, kw: int, padding: str = "same", stride: int = 1) -> str:
        x = g.add(Layer(auto("conv2d"), "conv", [x], {"filters": f, "kernel": (kh, kw), "stride": stride,
                                                       "padding": padding, "use_bias": False}))
        x = g.add(Layer(auto("batch_normalization"), "bn", [x], {"epsilon": 1e-3, "scale": False}))
        return g.add(Layer(auto("activation"), "relu", [x]))

    def maxpool(x: str) -> str:
        return g.add(Layer(auto("max_pooling2d"), "maxpool", [x], {"pool": 3, "stride": 2, "padding": "valid"}))

    def avgpool(x: str) -> str:
        return g.add(Layer(auto("average_pooling2d"), "avgpool", [x], {"pool": 3, "stride": 1, "padding": "same"}))

    def cat(xs, nm=None) -> str:
        return g.add(Layer(nm or auto("concatenate"), "concat", list(xs)))

    x = g.add(Layer("input_1", "input", [], {"shape": tuple(input_shape)}))
    x = cbn(x, 32, 3, 3, "valid", 2)
    x = cbn(x, 32, 3, 3, "valid")
    x = cbn(x, 64, 3, 3)
    x = maxpool(x)
    x = cbn(x, 80, 1, 1, "valid")
    x = cbn(x, 192, 3, 3, "valid")
    x = maxpool(x)
    for i, pool_f in enumerate((32, 64, 64)):                     # mixed0-2: 35 x 35
        b1 = cbn(x, 64, 1, 1)
        b5 = cbn(cbn(x, 48, 1, 1), 64, 5, 5)
        b3 = cbn(cbn(cbn(x, 64, 1, 1), 96, 3, 3), 96, 3, 3)
        bp = cbn(avgpool(x), pool_f, 1, 1)
        x = cat([b1, b5, b3, bp], f"mixed{i}")
    b3 = cbn(x, 384, 3, 3, "valid", 2)                            # mixed3: 17 x 17
    bd = cbn(cbn(cbn(x, 64, 1, 1), 96, 3, 3), 96, 3, 3, "valid", 2)
    x = cat([b3, bd, maxpool(x)], "mixed3")
    for i, c7 in enumerate((128, 160, 160, 192)):                 # mixed4-7
        b1 = cbn(x, 192, 1, 1)
        b7 = cbn(cbn(cbn(x, c7, 1, 1), c7, 1, 7), 192, 7, 1)
        bd = cbn(x, c7, 1, 1)
        for f, (kh, kw) in ((c7, (7, 1)), (c7, (1, 7)), (c7, (7, 1)), (192, (1, 7))):
            bd = cbn(bd, f, kh, kw)
        bp = cbn(avgpool(x), 192, 1, 1)
        x = cat([b1, b7, bd, bp], f"mixed{4 + i}")
    b3 = cbn(cbn(x, 192, 1, 1), 320, 3, 3, "valid", 2)            # mixed8: 8 x 8
    b7 = cbn(cbn(cbn(cbn(x, 192, 1, 1), 192, 1, 7), 192, 7, 1), 192, 3, 3, "valid", 2)
    x = cat([b3, b7, maxpool(x)], "mixed8")
    for i in range(2):                                            # mixed9, mixed10
        b1 = cbn(x, 320, 1, 1)
        b3 = cbn(x, 384, 1, 1)
        b3 = cat([cbn(b3, 384, 1, 3), cbn(b3, 384, 3, 1)], f"mixed9_{i}")
        bd = cbn(cbn(x, 448, 1, 1), 384, 3, 3)
        bd = cat([cbn(bd, 384, 1, 3), cbn(bd, 384, 3, 1)])
        bp = cbn(avgpool(x), 192, 1, 1)
        x = cat([b1, b3, bd, bp], f"mixed{9 + i}")
    x = g.add(Layer("avg_pool", "gap", [x]))
    g.add(Layer("predictions", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = ["predictions"]
    return g


# ----------------------------------------------------------------- ResNeXt
RESNEXT_STACKS = {"resnext50_32x4d": (3, 4, 6, 3), "resnext101_32x4d": (3, 4, 23, 3),
                  "resnext_tiny": (1, 1, 1, 1)}     # tiny: same naming/structure, for fast tests
RESNEXT_EPS = 1.001e-5


def build_resnext(name: str = "resnext50_32x4d", classes: int = 1000, input_shape=(224, 224, 3),
                  groups: int = 32) -> Graph:
    """Keras' ResNeXt (`block3` / `stack3` of keras.applications.resnet) with the ResNet layer names of
    models/resnet.py: 1x1 (w) -> ZeroPadding2D + grouped 3x3 (w, stride s) -> 1x1 (2w), projection
    shortcut on block 1, no conv bias."""
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": tuple(input_shape)}))
    x = g.add(Layer("conv1_pad", "zeropad", [x], {"pad": ((3, 3), (3, 3))}))
    x = _conv(g, x, "conv1_conv", 64, 7, stride=2, use_bias=False)
    x = g.add(Layer("conv1_bn", "bn", [x], {"epsilon": RESNEXT_EPS}))
    x = g.add(Layer("conv1_relu", "relu", [x]))
    x = g.add(Layer("pool1_pad", "zeropad", [x], {"pad": ((1, 1), (1, 1))}))
    x = g.add(Layer("pool1_pool", "maxpool", [x], {"pool": 3, "stride": 2, "padding": "valid"}))

    def bn(x: str, nm: str) -> str:
        return g.add(Layer(nm, "bn", [x], {"epsilon": RESNEXT_EPS}))

    for s, (w, blocks) in enumerate(zip((128, 256, 512, 1024), RESNEXT_STACKS[name]), start=2):
        for b in range(1, blocks + 1):
            nm = f"conv{s}_block{b}"
            stride = 2 if (b == 1 and s > 2) else 1
            sc = bn(_conv(g, x, f"{nm}_0_conv", 2 * w, 1, stride=stride, use_bias=False), f"{nm}_0_bn") if b == 1 else x
            y = g.add(Layer(f"{nm}_1_relu", "relu", [bn(_conv(g, x, f"{nm}_1_conv", w, 1, use_bias=False), f"{nm}_1_bn")]))
            y = g.add(Layer(f"{nm}_2_pad", "zeropad", [y], {"pad": ((1, 1), (1, 1))}))
            y = g.add(Layer(f"{nm}_2_conv", "conv", [y], {"filters": w, "kernel": (3, 3), "stride": stride,
                                                         "padding": "valid", "use_bias": False, "groups": groups}))
            y = g.add(Layer(f"{nm}_2_relu", "relu", [bn(y, f"{nm}_2_bn")]))
            y = bn(_conv(g, y, f"{nm}_3_conv", 2 * w, 1, use_bias=False), f"{nm}_3_bn")
            y = g.add(Layer(f"{nm}_add", "add", [sc, y]))
            x = g.add(Layer(f"{nm}_out", "relu", [y]))
    x = g.add(Layer("avg_pool", "gap", [x]))
    g.add(Layer("predictions", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = ["predictions"]
    return g


# ---------------------------------------------------------------- ConvNeXt
# name -> (depths, dims, default input); micro: same naming / structure, for fast tests
CONVNEXT = {
    "convnext_tiny": ((3, 3, 9, 3), (96, 192, 384, 768), (224, 224, 3)),
    "convnext_small": ((3, 3, 27, 3), (96, 192, 384, 768), (224, 224, 3)),
    "convnext_base": ((3, 3, 27, 3), (128, 256, 512, 1024), (224, 224, 3)),
    "convnext_large": ((3, 3, 27, 3), (192, 384, 768, 1536), (224, 224, 3)),
    "convnext_xlarge": ((3, 3, 27, 3), (256, 512, 1024, 2048), (224, 224, 3)),
    "convnext_micro": ((1, 1, 2, 1), (24, 48, 96, 192), (64, 64, 3)),
}
CONVNEXT_EPS = 1e-6


def build_convnext(name: str = "convnext_tiny", classes: int = 1000, input_shape=None) -> Graph:
    """`keras.applications.convnext` (include_top=True, no preprocessing layer) as flat layers: Keras nests
    the stem and the downsampling blocks in `Sequential` sub-models and adds the residual with a
    `TFOpLambda`; here they are plain layers and an `Add`, in the same order, so the flat `get_weights()`
    list is the same.  The 7x7 depthwise layer is Keras' `Conv2D(groups=C)` with kernel (7, 7, 1, C), the
    two pointwise layers are `Dense` on (H, W, C)."""
    depths, dims, default_shape = CONVNEXT[name]
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": tuple(input_shape or default_shape)}))

    def ln(x: str, nm: str) -> str:
        return g.add(Layer(nm, "layernorm", [x], {"epsilon": CONVNEXT_EPS}))

    x = ln(_conv(g, x, f"{name}_stem_conv", dims[0], 4, stride=4), f"{name}_stem_layernorm")
    for i, (depth, c) in enumerate(zip(depths, dims)):
        if i:
            x = _conv(g, ln(x, f"{name}_downsampling_layernorm_{i - 1}"), f"{name}_downsampling_conv_{i - 1}", c, 2,
                      stride=2)
        for j in range(depth):
            nm = f"{name}_stage_{i}_block_{j}"
            y = g.add(Layer(f"{nm}_depthwise_conv", "conv", [x],
                            {"filters": c, "kernel": (7, 7), "stride": 1, "padding": "same", "use_bias": True,
                             "groups": c}))
            y = ln(y, f"{nm}_layernorm")
            y = g.add(Layer(f"{nm}_pointwise_conv_1", "dense", [y], {"units": 4 * c, "use_bias": True}))
            y = g.add(Layer(f"{nm}_gelu", "act", [y], {"fn": "gelu"}))
            y = g.add(Layer(f"{nm}_pointwise_conv_2", "dense", [y], {"units": c, "use_bias": True}))
            y = g.add(Layer(f"{nm}_layer_scale", "layerscale", [y], {"init_values": 1e-6}))
            y = g.add(Layer(f"{nm}_identity", "identity", [y]))
            x = g.add(Layer(f"{nm}_add", "add", [x, y]))
    x = g.add(Layer("avg_pool", "gap", [x]))
    x = ln(x, f"{name}_head_layernorm")
    g.add(Layer(f"{name}_head_dense", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = [f"{name}_head_dense"]
    return g


# ------------------------------------------------------------------- U-Net
# name -> (base, depth, default input, up); tiny: same naming / structure, for fast tests
UNET = {
    "unet": (64, 4, (256, 256, 3), "transpose"),
    "unet_bilinear": (64, 4, (256, 256, 3), "bilinear"),
    "unet_tiny": (16, 2, (32, 32, 3), "transpose"),
}


def build_unet(name: str = "unet", classes: int = 1, input_shape=None, base: int = None, depth: int = None,
               up: str = None) -> Graph:
    """U-Net (Ronneberger et al. 2015) as it is usually written in Keras, with 'same' convolutions so the
    skips need no cropping: encoder level i is two 3x3 ReLU convs of base * 2^i filters and a 2x2 max-pool,
    the bottleneck two convs of base * 2^depth, each decoder level Conv2DTranspose(base * 2^i, 2, strides=2)
    -> Concatenate([skip, up]) -> two 3x3 ReLU convs, the head a 1x1 sigmoid conv.  up="bilinear" /
    "nearest" replaces the transposed conv by UpSampling2D(2) and a 2x2 'same' Conv2D of the same filters
    (the same parameter total).  H and W must be multiples of 2^depth."""
    dbase, ddepth, dshape, dup = UNET.get(name, UNET["unet"])
    base, depth, up = base or dbase, ddepth if depth is None else depth, up or dup
    shape = tuple(input_shape or dshape)
    if up not in ("transpose", "bilinear", "nearest"):
        raise ValueError(f"build_unet: up={up!r} (transpose, bilinear or nearest)")
    if shape[0] % (1 << depth) or shape[1] % (1 << depth):
        raise ValueError(f"build_unet: input {shape} is not a multiple of {1 << depth} in H and W")
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": shape}))

    def double(x: str, nm: str, f: int) -> str:
        x = _conv(g, x, f"{nm}_conv1", f, 3, padding="same", activation="relu")
        return _conv(g, x, f"{nm}_conv2", f, 3, padding="same", activation="relu")

    skips = []
    for i in range(depth):
        x = double(x, f"enc{i + 1}", base << i)
        skips.append(x)
        x = g.add(Layer(f"enc{i + 1}_pool", "maxpool", [x], {"pool": 2, "stride": 2, "padding": "valid"}))
    x = double(x, "bottleneck", base << depth)
    for i in reversed(range(depth)):
        nm, f = f"dec{i + 1}", base << i
        if up == "transpose":
            x = g.add(Layer(f"{nm}_up", "deconv", [x], {"filters": f, "kernel": (2, 2), "stride": 2,
                                                       "padding": "same", "use_bias": True}))
        else:
            x = g.add(Layer(f"{nm}_upsample", "upsample", [x], {"size": (2, 2), "interpolation": up}))
            x = _conv(g, x, f"{nm}_up", f, 2, padding="same")
        x = g.add(Layer(f"{nm}_concat", "concat", [skips[i], x]))
        x = double(x, nm, f)
    x = _conv(g, x, "head", classes, 1, activation="sigmoid")
    g.output_names = [x]
    return g


# ------------------------------------------------- Stable Diffusion VAE decoder
# name -> (widths per level, residual blocks per level, GN groups, latent shape); micro: same naming / structure
VAE_DECODER = {
    "sd_vae_decoder": ((512, 512, 256, 128), 3, 32, (64, 64, 4)),
    "vae_decoder_micro": ((32, 32, 16, 8), 1, 4, (8, 8, 4)),
}
VAE_EPS = 1e-5
VAE_LATENT_SCALE = 0.18215


def build_vae_decoder(name: str = "sd_vae_decoder", input_shape=None) -> Graph:
    """The Stable Diffusion v1 VAE decoder as KerasCV publishes it, as flat layers in its creation order:
    Rescaling(1 / 0.18215), the 1x1 post-quantisation conv, a 3x3 conv to the widest level, the middle (residual
    block, attention block, residual block), then per level its residual blocks and, between levels, nearest
    UpSampling2D(2) and a 3x3 conv; GroupNormalization, swish and a 3x3 conv to RGB close it.  A residual block is
    GN, swish, 3x3 conv, GN, swish, 3x3 conv plus the shortcut (a 1x1 conv where the width changes); the attention
    block is GN, a one-head MultiHeadAttention of key_dim C over the map (the published q / k / v / out 1x1 convs
    are its four projections: the same parameters) and the Add.  Every conv is 'same'."""
    widths, nblocks, groups, default_shape = VAE_DECODER[name]
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": tuple(input_shape or default_shape)}))

    def gn(x: str, nm: str) -> str:
        return g.add(Layer(nm, "groupnorm", [x], {"groups": groups, "epsilon": VAE_EPS}))

    def swish(x: str, nm: str) -> str:
        return g.add(Layer(nm, "act", [x], {"fn": "swish"}))

    def block(x: str, nm: str, f: int) -> str:
        y = _conv(g, swish(gn(x, f"{nm}_norm1"), f"{nm}_swish1"), f"{nm}_conv1", f, 3, padding="same")
        y = _conv(g, swish(gn(y, f"{nm}_norm2"), f"{nm}_swish2"), f"{nm}_conv2", f, 3, padding="same")
        if g.layers[x].out_shape[-1] != f:
            x = _conv(g, x, f"{nm}_shortcut", f, 1)
        return g.add(Layer(f"{nm}_add", "add", [x, y]))

    x = g.add(Layer("rescaling", "rescale", [x], {"scale": 1.0 / VAE_LATENT_SCALE, "offset": 0.0}))
    x = _conv(g, x, "post_quant_conv", g.layers[x].out_shape[-1], 1)
    x = _conv(g, x, "conv_in", widths[0], 3, padding="same")
    x = block(x, "mid_block1", widths[0])
    y = g.add(Layer("mid_attn", "mha", [gn(x, "mid_attn_norm")],
                    {"num_heads": 1, "key_dim": widths[0], "use_bias": True}))
    x = g.add(Layer("mid_attn_add", "add", [x, y]))
    x = block(x, "mid_block2", widths[0])
    for i, f in enumerate(widths):
        for j in range(nblocks):
            x = block(x, f"up{i}_block{j + 1}", f)
        if i + 1 < len(widths):
            x = g.add(Layer(f"up{i}_upsample", "upsample", [x], {"size": (2, 2), "interpolation": "nearest"}))
            x = _conv(g, x, f"up{i}_conv", f, 3, padding="same")
    x = swish(gn(x, "norm_out"), "swish_out")
    x = _conv(g, x, "conv_out", 3, 3, padding="same")
    g.output_names = [x]
    return g


# --------------------------------------------------------------------- ViT
# name -> (patch, width, depth, heads, mlp, default input); micro: same naming / structure, for fast tests
VIT = {
    "vit_ti16": (16, 192, 12, 3, 768, (224, 224, 3)),
    "vit_s16": (16, 384, 12, 6, 1536, (224, 224, 3)),
    "vit_b16": (16, 768, 12, 12, 3072, (224, 224, 3)),
    "vit_l16": (16, 1024, 24, 16, 4096, (224, 224, 3)),
    "vit_micro": (8, 64, 2, 2, 128, (32, 32, 3)),
}
VIT_EPS = 1e-6


def build_vit(name: str = "vit_b16", classes: int = 1000, input_shape=None) -> Graph:
    """Vision Transformer (Dosovitskiy et al. 2021; the published Ti / S / B / L at patch 16) as a flat pre-norm
    graph: a p x p / p patch conv, the class token and position embedding, `depth` blocks of
    LayerNormalization -> MultiHeadAttention -> Add and LayerNormalization -> Dense -> GELU -> Dense -> Add on a
    (1, T, C) token map, a final LayerNormalization, the class token cropped out, and the Dense softmax head."""
    patch, width, depth, heads, mlp, default_shape = VIT[name]
    shape = tuple(input_shape or default_shape)
    if len(shape) != 3 or shape[0] % patch or shape[1] % patch:
        raise ValueError(f"{name}: input {shape} is not (H, W, C) with H and W multiples of the {patch}-pixel patch")
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": shape}))
    x = _conv(g, x, f"{name}_patch_embed", width, patch, stride=patch)
    x = g.add(Layer(f"{name}_pos_embed", "posembed", [x], {"class_token": True}))
    tokens = g.layers[x].out_shape[1]

    def ln(x: str, nm: str) -> str:
        return g.add(Layer(nm, "layernorm", [x], {"epsilon": VIT_EPS}))

    for i in range(depth):
        nm = f"{name}_block_{i}"
        y = g.add(Layer(f"{nm}_attn", "mha", [ln(x, f"{nm}_ln1")],
                        {"num_heads": heads, "key_dim": width // heads, "use_bias": True}))
        x = g.add(Layer(f"{nm}_add1", "add", [x, y]))
        y = g.add(Layer(f"{nm}_mlp_fc1", "dense", [ln(x, f"{nm}_ln2")], {"units": mlp, "use_bias": True}))
        y = g.add(Layer(f"{nm}_mlp_gelu", "act", [y], {"fn": "gelu"}))
        y = g.add(Layer(f"{nm}_mlp_fc2", "dense", [y], {"units": width, "use_bias": True}))
        x = g.add(Layer(f"{nm}_add2", "add", [x, y]))
    x = ln(x, f"{name}_ln")
    x = g.add(Layer(f"{name}_cls", "crop", [x], {"crop": ((0, 0), (0, tokens - 1))}))      # the class token
    x = g.add(Layer(f"{name}_flatten", "flatten", [x]))
    g.add(Layer(f"{name}_head", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = [f"{name}_head"]
    return g


# -------------------------------------------------------------------- Swin
# name -> (patch, window, width C, depths, heads, default input); micro: same naming / structure, for fast tests
SWIN = {
    "swin_tiny": (4, 7, 96, (2, 2, 6, 2), (3, 6, 12, 24), (224, 224, 3)),
    "swin_small": (4, 7, 96, (2, 2, 18, 2), (3, 6, 12, 24), (224, 224, 3)),
    "swin_base": (4, 7, 128, (2, 2, 18, 2), (4, 8, 16, 32), (224, 224, 3)),
    "swin_large": (4, 7, 192, (2, 2, 18, 2), (6, 12, 24, 48), (224, 224, 3)),
    "swin_micro": (4, 4, 32, (2, 2), (2, 4), (32, 32, 3)),
}
SWIN_EPS = 1e-5
SWIN_MLP_RATIO = 4


def build_swin(name: str = "swin_tiny", classes: int = 1000, input_shape=None) -> Graph:
    """Swin Transformer (Liu et al. 2021; the published Tiny / Small / Base / Large at patch 4, window 7) as a
    flat graph on (H, W, C) maps: a 4x4 / 4 patch conv and LayerNormalization; per stage `depth` blocks of
    LayerNormalization -> WindowAttention -> Add and LayerNormalization -> Dense 4C -> GELU -> Dense C -> Add,
    odd blocks shifted by M // 2 (none when the stage's map is a single window, as in the published model);
    between stages SpaceToDepth -> LayerNormalization(4C) -> Dense(2C, no bias); then LayerNormalization,
    GlobalAveragePooling2D and the Dense softmax head."""
    patch, window, width, depths, heads, default_shape = SWIN[name]
    shape = tuple(input_shape or default_shape)
    if len(shape) != 3 or shape[0] % patch or shape[1] % patch:
        raise ValueError(f"{name}: input {shape} is not (H, W, C) with H and W multiples of the {patch}-pixel patch")
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": shape}))
    x = _conv(g, x, f"{name}_patch_embed", width, patch, stride=patch)

    def ln(x: str, nm: str) -> str:
        return g.add(Layer(nm, "layernorm", [x], {"epsilon": SWIN_EPS}))

    x = ln(x, f"{name}_patch_embed_ln")
    for s, (depth, nh) in enumerate(zip(depths, heads)):
        c = width << s
        if s:
            h, w, _ = g.layers[x].out_shape
            if h % 2 or w % 2:
                raise ValueError(f"{name}: stage {s}'s input map {h} x {w} cannot be merged 2 x 2 (input {shape})")
            x = g.add(Layer(f"{name}_stage_{s}_merge", "space_to_depth", [x], {"block": 2}))
            x = ln(x, f"{name}_stage_{s}_merge_ln")
            x = g.add(Layer(f"{name}_stage_{s}_merge_reduction", "dense", [x], {"units": c, "use_bias": False}))
        h, w, _ = g.layers[x].out_shape
        if h % window or w % window:
            raise ValueError(f"{name}: stage {s}'s {h} x {w} map is not a multiple of the {window} x {window} "
                             f"window (input {shape})")
        for i in range(depth):
            nm = f"{name}_stage_{s}_block_{i}"
            shift = window // 2 if i % 2 and (h, w) != (window, window) else 0
            y = g.add(Layer(f"{nm}_attn", "winattn", [ln(x, f"{nm}_ln1")],
                            {"num_heads": nh, "key_dim": c // nh, "window": window, "shift": shift,
                             "use_bias": True}))
            x = g.add(Layer(f"{nm}_add1", "add", [x, y]))
            y = g.add(Layer(f"{nm}_mlp_fc1", "dense", [ln(x, f"{nm}_ln2")],
                            {"units": SWIN_MLP_RATIO * c, "use_bias": True}))
            y = g.add(Layer(f"{nm}_mlp_gelu", "act", [y], {"fn": "gelu"}))
            y = g.add(Layer(f"{nm}_mlp_fc2", "dense", [y], {"units": c, "use_bias": True}))
            x = g.add(Layer(f"{nm}_add2", "add", [x, y]))
    x = ln(x, f"{name}_ln")
    x = g.add(Layer(f"{name}_avg_pool", "gap", [x]))
    g.add(Layer(f"{name}_head", "dense", [x], {"units": classes, "activation": "softmax", "use_bias": True}))
    g.output_names = [f"{name}_head"]
    return g


# -------------------------------------------------------------------- DETR
# name -> (backbone, width, heads, queries, encoder layers, decoder layers, FFN width, default input); micro: same
# naming / structure behind a three-conv backbone, for fast tests
DETR = {
    "detr_resnet50": ("resnet50", 256, 8, 100, 6, 6, 2048, (480, 640, 3)),
    "detr_micro": ((8, 16, 32), 32, 2, 10, 2, 2, 64, (40, 56, 3)),
}
DETR_EPS = 1e-5
DETR_CLASSES = 92          # 91 COCO category ids + "no object"


def build_detr(name: str = "detr_resnet50", classes: int = DETR_CLASSES, input_shape=None) -> Graph:
    """DETR (Carion et al. 2020) as published, post-norm, as a flat graph.  The ResNet-50 layers of `build_resnet`
    through `conv5_block3_out` under their Keras names, a 1x1 `input_proj` to the model width, and the map as
    (1, T, C) tokens.  One position table `pos` (T, C), a LearnedQueries (the published sine values load into it as
    weights).  Encoder layer: MultiHeadAttention(q = k = src + pos, v = src) -> Add -> LayerNormalization ->
    Dense(ffn, relu) -> Dense -> Add -> LayerNormalization.  Decoder layer on `tgt` (a zeros LearnedQueries) with
    `query_embed`: self-attention (q = k = tgt + query_embed, v = tgt), cross-attention (q = tgt + query_embed,
    k = memory + pos, v = memory) and the FFN, each followed by Add and LayerNormalization.  A final
    LayerNormalization, the class head Dense(92), the box head Dense(relu), Dense(relu), Dense(4, sigmoid), and the
    Concatenate of both into one (1, queries, 96) output.  The learned tensors hang off the tensor next to them
    (`pos` off the projected map, `tgt` and `query_embed` off memory + pos), which only gives them the batch size: a
    cut never drags the image along, and one inside the decoder ships the running target, the memory, memory + pos
    and the query embedding."""
    from .resnet import BN_EPS, STACKS, _stack1
    backbone, width, heads, nq, enc, dec, ffn, default_shape = DETR[name]
    shape = tuple(input_shape or default_shape)
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": shape}))
    if isinstance(backbone, str):
        x = g.add(Layer("conv1_pad", "zeropad", [x], {"pad": ((3, 3), (3, 3))}))
        x = _conv(g, x, "conv1_conv", 64, 7, stride=2)
        x = g.add(Layer("conv1_bn", "bn", [x], {"epsilon": BN_EPS}))
        x = g.add(Layer("conv1_relu", "relu", [x]))
        x = g.add(Layer("pool1_pad", "zeropad", [x], {"pad": ((1, 1), (1, 1))}))
        x = g.add(Layer("pool1_pool", "maxpool", [x], {"pool": 3, "stride": 2, "padding": "valid"}))
        for s, (filters, blocks) in enumerate(zip((64, 128, 256, 512), STACKS[backbone])):
            x = _stack1(g, x, filters, blocks, 1 if s == 0 else 2, f"conv{s + 2}")
    else:
        for i, f in enumerate(backbone):
            x = _conv(g, x, f"backbone_conv{i + 1}", f, 3, stride=2, padding="same", activation="relu")
    x = _conv(g, x, "input_proj", width, 1)
    h, w, _ = g.layers[x].out_shape
    tokens = h * w
    src = g.add(Layer("src", "reshape", [x], {"shape": (1, tokens, width)}))
    pos = g.add(Layer("pos", "queries", [src], {"length": tokens, "dim": width, "initializer": "normal"}))

    def add(a: str, b: str, nm: str) -> str:
        return g.add(Layer(nm, "add", [a, b]))

    def ln(x: str, nm: str) -> str:
        return g.add(Layer(nm, "layernorm", [x], {"epsilon": DETR_EPS}))

    def mha(q: str, v: str, k: str, nm: str) -> str:
        return g.add(Layer(nm, "mha", [q, v, k], {"num_heads": heads, "key_dim": width // heads, "use_bias": True}))

    def ffn_block(x: str, nm: str) -> str:
        y = g.add(Layer(f"{nm}_ffn_fc1", "dense", [x], {"units": ffn, "activation": "relu", "use_bias": True}))
        y = g.add(Layer(f"{nm}_ffn_fc2", "dense", [y], {"units": width, "use_bias": True}))
        return ln(add(x, y, f"{nm}_add_ffn"), f"{nm}_ln_ffn")

    x = src
    for i in range(enc):
        nm = f"encoder_{i}"
        qk = add(x, pos, f"{nm}_qk")
        x = ln(add(x, mha(qk, x, qk, f"{nm}_attn"), f"{nm}_add_attn"), f"{nm}_ln_attn")
        x = ffn_block(x, nm)
    memory = x
    memory_pos = add(memory, pos, "memory_pos")
    query_embed = g.add(Layer("query_embed", "queries", [memory_pos], {"length": nq, "dim": width,
                                                                 "initializer": "normal"}))
    x = g.add(Layer("tgt", "queries", [memory_pos], {"length": nq, "dim": width, "initializer": "zeros"}))
    for i in range(dec):
        nm = f"decoder_{i}"
        qk = add(x, query_embed, f"{nm}_self_qk")
        x = ln(add(x, mha(qk, x, qk, f"{nm}_self_attn"), f"{nm}_add_self"), f"{nm}_ln_self")
        q = add(x, query_embed, f"{nm}_cross_q")
        x = ln(add(x, mha(q, memory, memory_pos, f"{nm}_cross_attn"), f"{nm}_add_cross"), f"{nm}_ln_cross")
        x = ffn_block(x, nm)
    x = ln(x, "decoder_ln")
    logits = g.add(Layer("class_head", "dense", [x], {"units": classes, "use_bias": True}))
    y = g.add(Layer("box_head_fc1", "dense", [x], {"units": width, "activation": "relu", "use_bias": True}))
    y = g.add(Layer("box_head_fc2", "dense", [y], {"units": width, "activation": "relu", "use_bias": True}))
    boxes = g.add(Layer("box_head_fc3", "dense", [y], {"units": 4, "activation": "sigmoid", "use_bias": True}))
    g.add(Layer("detections", "concat", [logits, boxes]))
    g.output_names = ["detections"]
    return g


# --------------------------------------------------------------------- GPT
# name -> (depth, width, heads, vocabulary, default tokens); micro: same naming / structure, for fast tests (40
# tokens: one above the attention key tile plus 7, below the query tile)
GPT = {
    "gpt2": (12, 768, 12, 50257, 128),
    "gpt2_medium": (24, 1024, 16, 50257, 128),
    "gpt2_large": (36, 1280, 20, 50257, 128),
    "gpt2_xl": (48, 1600, 25, 50257, 128),
    "gpt_micro": (2, 32, 2, 97, 40),
}
GPT_CONTEXT = 1024         # rows of the published position table
GPT_EPS = 1e-5
GPT_MLP_RATIO = 4


def build_gpt(name: str = "gpt2", classes: Optional[int] = None, input_shape=None,
              all_positions: bool = False) -> Graph:
    """GPT-2 (Radford et al. 2019; the published 124M / medium / large / xl) as a flat pre-norm graph, the
    full-sequence forward pass: the (T,) token ids (carried as float32) through an Embedding, a learned position
    embedding without a class token, `depth` blocks of LayerNormalization -> causal MultiHeadAttention -> Add and
    LayerNormalization -> Dense(4C, gelu_tanh) -> Dense(C) -> Add on a (1, T, C) token map, the last token
    cropped out (`all_positions=True` keeps every token), the final LayerNormalization and `lm_head`, a Dense
    without bias onto the vocabulary: the next-token logits.  `classes` is the vocabulary.  The position table has
    the T rows of the built graph; a loader slices the published 1024-row table.  The IR shares no weights, so
    `lm_head` owns a (C, V) kernel, into which a loader puts the transposed token table: the parameter total
    counts the table once more than the published figure."""
    depth, width, heads, vocab, default_tokens = GPT[name]
    vocab = int(classes or vocab)
    shape = tuple(input_shape or (default_tokens,))
    if len(shape) != 1 or not 1 <= shape[0] <= GPT_CONTEXT:
        raise ValueError(f"{name}: input {shape} is not (T,) token ids with 1 <= T <= {GPT_CONTEXT}")
    tokens = shape[0]
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": shape}))
    x = g.add(Layer(f"{name}_wte", "embedding", [x], {"input_dim": vocab, "output_dim": width}))
    x = g.add(Layer(f"{name}_wpe", "posembed", [x], {"class_token": False}))

    def ln(x: str, nm: str) -> str:
        return g.add(Layer(nm, "layernorm", [x], {"epsilon": GPT_EPS}))

    for i in range(depth):
        nm = f"{name}_block_{i}"
        y = g.add(Layer(f"{nm}_attn", "mha", [ln(x, f"{nm}_ln1")],
                        {"num_heads": heads, "key_dim": width // heads, "use_bias": True, "causal": True}))
        x = g.add(Layer(f"{nm}_add1", "add", [x, y]))
        y = g.add(Layer(f"{nm}_mlp_fc1", "dense", [ln(x, f"{nm}_ln2")],
                        {"units": GPT_MLP_RATIO * width, "activation": "gelu_tanh", "use_bias": True}))
        y = g.add(Layer(f"{nm}_mlp_fc2", "dense", [y], {"units": width, "use_bias": True}))
        x = g.add(Layer(f"{nm}_add2", "add", [x, y]))
    if not all_positions:
        x = g.add(Layer(f"{name}_last", "crop", [x], {"crop": ((0, 0), (tokens - 1, 0))}))      # the last token
    x = ln(x, f"{name}_ln_f")
    g.add(Layer("lm_head", "dense", [x], {"units": vocab, "use_bias": False}))
    g.output_names = ["lm_head"]
    return g


# --------------------------------------------------------------------- DistilBERT
# name -> (depth, width, heads, vocabulary, default tokens); micro: the test size (40 tokens, as gpt_micro)
DISTILBERT = {
    "distilbert_base": (6, 768, 12, 30522, 128),
    "distilbert_micro": (2, 32, 2, 97, 40),
}
DISTILBERT_CONTEXT = 512   # rows of the published position table
DISTILBERT_EPS = 1e-12
DISTILBERT_FFN_RATIO = 4


def build_distilbert(name: str = "distilbert_base", classes: Optional[int] = None, input_shape=None) -> Graph:
    """DistilBERT (Sanh et al. 2019; `distilbert-base-uncased` as published) as a flat post-norm encoder: the (T,)
    token ids (carried as float32, pad id 0) through an Embedding with mask_zero, a learned position embedding
    without a class token and a LayerNormalization; `depth` blocks of MultiHeadAttention -> Add ->
    LayerNormalization -> Dense(4C, exact gelu) -> Dense(C) -> Add -> LayerNormalization; no token-type
    embedding.  The output is the last hidden state, (1, T, C).  The padding mask of the Embedding reaches every
    attention layer by `propagate_masks` (graph/ir.py): each gets `key_mask` and the ids as its last input, and
    attends kept tokens only; hidden states at padded positions are defined but are not Keras' (graph/ir.py
    "mha").  `classes` is the vocabulary.  The position table has the T rows of the built graph; a loader slices
    the published 512-row table, with which the total is the published 66,362,880."""
    depth, width, heads, vocab, default_tokens = DISTILBERT[name]
    vocab = int(classes or vocab)
    shape = tuple(input_shape or (default_tokens,))
    if len(shape) != 1 or not 1 <= shape[0] <= DISTILBERT_CONTEXT:
        raise ValueError(f"{name}: input {shape} is not (T,) token ids with 1 <= T <= {DISTILBERT_CONTEXT}")
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": shape}))
    x = g.add(Layer(f"{name}_word_embeddings", "embedding", [x],
                    {"input_dim": vocab, "output_dim": width, "mask_zero": True}))
    x = g.add(Layer(f"{name}_position_embeddings", "posembed", [x], {"class_token": False}))

    def ln(x: str, nm: str) -> str:
        return g.add(Layer(nm, "layernorm", [x], {"epsilon": DISTILBERT_EPS}))

    x = ln(x, f"{name}_embeddings_ln")
    for i in range(depth):
        nm = f"{name}_layer_{i}"
        y = g.add(Layer(f"{nm}_attention", "mha", [x],
                        {"num_heads": heads, "key_dim": width // heads, "use_bias": True}))
        x = ln(g.add(Layer(f"{nm}_add1", "add", [x, y])), f"{nm}_sa_layer_norm")
        y = g.add(Layer(f"{nm}_ffn_lin1", "dense", [x],
                        {"units": DISTILBERT_FFN_RATIO * width, "activation": "gelu", "use_bias": True}))
        y = g.add(Layer(f"{nm}_ffn_lin2", "dense", [y], {"units": width, "use_bias": True}))
        x = ln(g.add(Layer(f"{nm}_add2", "add", [x, y])), f"{nm}_output_layer_norm")
    g.output_names = [x]
    return with_key_masks(g)


# ------------------------------------------------------------------- Llama
# name -> (depth, width, heads, kv_heads, ffn, vocabulary, default tokens, eps, rope max wavelength); micro: same
# naming / structure, for fast tests (head size 16, so the attention core's MFMA path, with g = 2 query heads per
# key / value head; 40 tokens: one above the attention key tile plus 7, below the query tile)
LLAMA = {
    "tinyllama_1_1b": (22, 2048, 32, 4, 5632, 32000, 128, 1e-5, 10000.0),
    "llama2_7b": (32, 4096, 32, 32, 11008, 32000, 128, 1e-5, 10000.0),
    "llama_micro": (2, 64, 4, 2, 176, 97, 40, 1e-5, 10000.0),
}


def build_llama(name: str = "tinyllama_1_1b", classes: Optional[int] = None, input_shape=None,
                all_positions: bool = False) -> Graph:
    """The Llama family (Touvron et al. 2023; TinyLlama 1.1B and Llama 2 7B as published) as a flat pre-norm
    graph without a bias anywhere, the full-sequence forward pass: the (T,) token ids (carried as float32) through
    an Embedding; `depth` blocks of RMSNormalization -> causal RotaryGroupedQueryAttention -> Add and
    RMSNormalization -> gate = Dense(F) -> swish, up = Dense(F), Multiply -> down = Dense(C) -> Add on a (1, T, C)
    token map; the last token cropped out (`all_positions=True` keeps every token), the final RMSNormalization
    and `lm_head`, a Dense without bias onto the vocabulary: the next-token logits.  There is no position table:
    the attention layers rotate Q and K (`rope`, the max wavelength).  `classes` is the vocabulary.  With
    kv_heads == heads (llama2_7b) the layer is plain multi-head attention behind the rope step.  No KV cache and
    no incremental decoding; frequency scaling (Llama 3) is not built."""
    depth, width, heads, kv_heads, ffn, vocab, default_tokens, eps, wavelength = LLAMA[name]
    vocab = int(classes or vocab)
    shape = tuple(input_shape or (default_tokens,))
    if len(shape) != 1 or shape[0] < 1:
        raise ValueError(f"{name}: input {shape} is not (T,) token ids with T >= 1")
    tokens = shape[0]
    g = Graph(name)
    x = g.add(Layer("input_1", "input", [], {"shape": shape}))
    x = g.add(Layer(f"{name}_embed_tokens", "embedding", [x], {"input_dim": vocab, "output_dim": width}))
    # the (1, T, C) token map every other transformer of the zoo runs on (there a position embedding makes it);
    # the same elements in the same order, so no plan step
    x = g.add(Layer(f"{name}_tokens", "reshape", [x], {"shape": (1, tokens, width)}))

    def norm(x: str, nm: str) -> str:
        return g.add(Layer(nm, "rmsnorm", [x], {"epsilon": eps}))

    for i in range(depth):
        nm = f"{name}_block_{i}"
        attrs = {"num_heads": heads, "key_dim": width // heads, "use_bias": False, "causal": True,
                 "kv_heads": kv_heads, "rope": wavelength}
        y = g.add(Layer(f"{nm}_attn", "mha", [norm(x, f"{nm}_input_norm")], attrs))
        x = g.add(Layer(f"{nm}_add1", "add", [x, y]))
        h = norm(x, f"{nm}_post_attention_norm")
        gate = g.add(Layer(f"{nm}_mlp_gate", "dense", [h], {"units": ffn, "use_bias": False}))
        gate = g.add(Layer(f"{nm}_mlp_swish", "act", [gate], {"fn": "swish"}))
        up = g.add(Layer(f"{nm}_mlp_up", "dense", [h], {"units": ffn, "use_bias": False}))
        y = g.add(Layer(f"{nm}_mlp_mul", "binary", [gate, up], {"fn": "mul"}))
        y = g.add(Layer(f"{nm}_mlp_down", "dense", [y], {"units": width, "use_bias": False}))
        x = g.add(Layer(f"{nm}_add2", "add", [x, y]))
    if not all_positions:
        x = g.add(Layer(f"{name}_last", "crop", [x], {"crop": ((0, 0), (tokens - 1, 0))}))      # the last token
    x = norm(x, f"{name}_norm")
    g.add(Layer("lm_head", "dense", [x], {"units": vocab, "use_bias": False}))
    g.output_names = ["lm_head"]
    return g


BUILDERS: Dict[str, Callable[..., Graph]] = {
    **{n: (lambda n: lambda **kw: build_llama(n, **kw))(n) for n in LLAMA},
    **{n: (lambda n: lambda **kw: build_distilbert(n, **kw))(n) for n in DISTILBERT},
    **{n: (lambda n: lambda **kw: build_gpt(n, **kw))(n) for n in GPT},
    **{n: (lambda n: lambda **kw: build_detr(n, **kw))(n) for n in DETR},
    **{n: (lambda n: lambda **kw: build_swin(n, **kw))(n) for n in SWIN},
    **{n: (lambda n: lambda **kw: build_vit(n, **kw))(n) for n in VIT},
    **{n: (lambda n: lambda **kw: build_vae_decoder(n, **kw))(n) for n in VAE_DECODER},
    **{n: (lambda n: lambda **kw: build_unet(n, **kw))(n) for n in UNET},
    **{n: (lambda n: lambda **kw: build_convnext(n, **kw))(n) for n in CONVNEXT},
    "vgg16": lambda **kw: build_vgg("vgg16", **kw),
    "vgg19": lambda **kw: build_vgg("vgg19", **kw),
    "mobilenet_v2": lambda **kw: build_mobilenet_v2(**kw),
    "densenet121": lambda **kw: build_densenet("densenet121", **kw),
    "densenet169": lambda **kw: build_densenet("densenet169", **kw),
    "densenet201": lambda **kw: build_densenet("densenet201", **kw),
    **{n: (lambda n: lambda **kw: build_efficientnet(n, **kw))(n) for n in EFFNET_SCALE},
    "inception_v3": lambda **kw: build_inception_v3(**kw),
    **{n: (lambda n: lambda **kw: build_resnext(n, **kw))(n) for n in RESNEXT_STACKS},
}


def build_model(name: str, **kw) -> Graph:
    """Any supported family by name: resnet50/101/152 (+ test sizes) or a key of BUILDERS."""
    from .resnet import STACKS, build_resnet
    if name in STACKS:
        return build_resnet(name, **kw)
    if name not in BUILDERS:
        raise KeyError(f"unknown model {name!r}; known: {sorted(STACKS) + sorted(BUILDERS)}")
    return BUILDERS[name](**kw)
