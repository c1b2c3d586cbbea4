"""Cases, inputs, float64 oracles and per-element allowances shared by the layer-kernel tests (PyTorch oracle,
native CPU ops, HIP kernels): depthwise conv, max / average / global pools, activations, Add / BN / binary
element-wise ops, concat, zero pad, casts, `input_pack` and `softmax_rows`.

Oracles are float64 numpy with loops over taps; none calls `F.conv2d`, `F.*_pool2d`, `F.gelu` or ops/reference.py
(those are what tests/test_layer_cases.py checks them against).  Inputs are seeded per case with
``zlib.crc32(repr(case))`` and cached: callers must not modify what they get.  Every ``*_case(c, bf16=True)``
rounds its activations to bf16 first, so the oracle and the allowance follow the values the bf16 kernel is handed.

Allowances are per element and come from the oracle and the inputs alone (u = 2^-24):

* activation of x with oracle y, fp32: ``A(x, y) = 4 (1 + |x|) 2^-23 max(1, |y|)``; the factor (1 + |x|) covers a
  fast exponential whose relative error grows with |x|.
* linear layers (depthwise conv, average pools, GAP, affine, the arithmetic binary ops), fp32:
  ``L = 2 (n + 2) u S`` with n the number of terms summed and S the same oracle run on absolute values
  (sum |x||w| + |bias|; mean |x| for the pools; |a| + |b|, |a||b|, (|a| + |b|) / 2 for add / sub, mul, avg with
  n = 1; max and min are exact, L = 0).  With a fused activation: ``2 L + A(pre, y)`` (every ActMode has slope
  <= 1.76).
* row softmax, fp32: ``2^-23 (4 (1 + |x_i - max|) + log2(N) + 2) p_i + 2^-126``.
* bf16 outputs: the fp32 allowance of the same element plus ``2^-8 |y|`` (one round-to-nearest-even store).
* copies (max pools, pad, concat, bf16 -> fp32 cast, ReLU / ReLU6 on bf16) are bit-exact; fp32 -> bf16 casts
  equal torch's ``.to(torch.bfloat16)`` bit for bit.

No allowance constant had to be changed from these values: torch's fp32 evaluation and the native CPU ops stay
inside them on every case (tests/test_layer_cases.py).

Largest error / allowance seen on an MI355X (tests/test_layers_gpu.py), per kernel family:

    family                      fp32     bf16
    depthwise conv              0.121    0.994  (fp32 scalar kernel 0.103; bf16 register-blocked 3x3 0.995)
    average pool                0.222    0.996
    global average pool         0.184    0.988  (bf16 input, fp32 output 0.132)
    act / affine_act            0.150    0.969
    relu (bf16 kernel)            -      0.980
    add_act, eltwise add / bn   0.166    0.996  (bn_act bf16 0.996)
    binary                      0.167    0.996
    row softmax                 0.844      -

  The bf16 figures sit just under 1 by construction: 2^-8 |y| is half a bf16 ulp bounded from above, and one
  rounding to nearest uses up to all of it.  Every copy and cast was bit-exact.  The fast `__expf` stays inside
  A(x, y) everywhere, SELU / ELU near 0 (exp(v) - 1) and the softmax row with a spread of 160 included.

The grid-stride cases (tests/test_layers_gpu.py `test_second_pass_*`) sit just past 8192 blocks x 256 threads =
2,097,152 work items (`GRID_CAP_ITEMS`), where every capped launcher starts its second loop pass.  `gap_finish*`
(one item per (image, channel) with >= 1024 pixels behind it) cannot cross that count inside 40 MB and has no such
case.
"""
import functools
import math
import types
import zlib

import numpy as np
import torch

U24 = 2.0 ** -24
U23 = 2.0 ** -23
GRID_CAP_ITEMS = 8192 * 256          # work items one pass of a capped grid covers

# index = csrc/kernels/common.h ActMode
ACT_NAMES = ("linear", "relu", "relu6", "swish", "sigmoid", "tanh", "hard_sigmoid", "hard_swish", "gelu", "elu",
             "selu", "softplus", "leaky_relu", "gelu_tanh")
ACT = {n: i for i, n in enumerate(ACT_NAMES)}
BIN_OPS = ("add", "sub", "mul", "max", "min", "avg")
SELU_SCALE, SELU_ALPHA = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def to_bf16(a):
    """fp32 array rounded to bf16 (round to nearest even) and widened back."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _ns(**kw):
    return types.SimpleNamespace(**kw)


# ---------------------------------------------------------------------------------------------------- oracles
_erf = np.vectorize(math.erf, otypes=[np.float64])


def ref_act(x, mode, alpha=0.3):
    """The 13 activations of ActMode (and linear) in float64, Keras definitions."""
    x = np.asarray(x, np.float64)
    m = ACT_NAMES[mode] if isinstance(mode, (int, np.integer)) else mode
    with np.errstate(over="ignore"):              # exp(1e4) = inf gives the right limit
        return _ref_act(x, m, alpha)


def _ref_act(x, m, alpha):
    if m == "linear":
        return x.copy()
    if m == "relu":                               # +0 for -0, as max(x, +0) under IEEE 754 maximum
        return np.where(x > 0, x, 0.0)
    if m == "relu6":
        return np.minimum(np.where(x > 0, x, 0.0), 6.0)
    if m == "swish":
        return x / (1.0 + np.exp(-x))
    if m == "sigmoid":
        return 1.0 / (1.0 + np.exp(-x))
    if m == "tanh":
        return np.tanh(x)
    if m == "hard_sigmoid":
        return np.minimum(np.maximum(0.2 * x + 0.5, 0.0), 1.0)
    if m == "hard_swish":
        return x * np.minimum(np.maximum(x + 3.0, 0.0), 6.0) / 6.0
    if m == "gelu":
        return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
    if m == "elu":
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    if m == "selu":
        return SELU_SCALE * np.where(x > 0, x, SELU_ALPHA * np.expm1(np.minimum(x, 0.0)))
    if m == "softplus":
        return np.logaddexp(0.0, x)
    if m == "leaky_relu":
        return np.where(x > 0, x, alpha * x)
    if m == "gelu_tanh":
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    raise ValueError(m)


def out_hw(H, W, kh, kw, s, pads):
    (pt, pb), (pl, pr) = pads
    return (H + pt + pb - kh) // s + 1, (W + pl + pr - kw) // s + 1


def _padded(x, pads, fill=0.0):
    (pt, pb), (pl, pr) = pads
    B, H, W, C = x.shape
    xp = np.full((B, H + pt + pb, W + pl + pr, C), fill, np.float64)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp


def _taps(xp, kh, kw, s, OH, OW):
    for i in range(kh):
        for j in range(kw):
            yield i, j, xp[:, i:i + (OH - 1) * s + 1:s, j:j + (OW - 1) * s + 1:s]


def ref_dwconv(x, w, bias, s, pads):
    """NHWC depthwise conv (multiplier 1), w [KH, KW, C], explicit ((pt, pb), (pl, pr)) zero padding; no activation."""
    w = np.asarray(w, np.float64)
    KH, KW, C = w.shape
    OH, OW = out_hw(x.shape[1], x.shape[2], KH, KW, s, pads)
    y = np.zeros((x.shape[0], OH, OW, C), np.float64)
    for i, j, v in _taps(_padded(x, pads), KH, KW, s, OH, OW):
        y += v * w[i, j]
    return y + np.asarray(bias, np.float64)


def ref_maxpool(x, k, s, pads, pad_zero):
    """Max pool; padding takes part as zeros (`pad_zero`, a folded ZeroPadding2D) or not at all ('same')."""
    OH, OW = out_hw(x.shape[1], x.shape[2], k, k, s, pads)
    y = np.full((x.shape[0], OH, OW, x.shape[3]), -np.inf, np.float64)
    for _, _, v in _taps(_padded(x, pads, 0.0 if pad_zero else -np.inf), k, k, s, OH, OW):
        y = np.maximum(y, v)
    return y


def ref_avgpool(x, kh, kw, s, pads):
    """(average with padding excluded from the count, the count per output pixel [1, OH, OW, 1])."""
    OH, OW = out_hw(x.shape[1], x.shape[2], kh, kw, s, pads)
    y = np.zeros((x.shape[0], OH, OW, x.shape[3]), np.float64)
    n = np.zeros((1, OH, OW, 1), np.float64)
    ones = _padded(np.ones((1,) + x.shape[1:3] + (1,)), pads)
    for (_, _, v), (_, _, o) in zip(_taps(_padded(x, pads), kh, kw, s, OH, OW), _taps(ones, kh, kw, s, OH, OW)):
        y += v
        n += o
    return y / n, n


def ref_gap(x):
    x = np.asarray(x, np.float64)
    acc = np.zeros((x.shape[0], x.shape[3]), np.float64)
    for h in range(x.shape[1]):
        acc += x[:, h].sum(1)
    return acc / (x.shape[1] * x.shape[2])


def ref_gmp(x):
    x = np.asarray(x, np.float64)
    m = np.full((x.shape[0], x.shape[3]), -np.inf)
    for h in range(x.shape[1]):
        m = np.maximum(m, x[:, h].max(1))
    return m


def ref_pad(x, pt, pl, OH, OW):
    y = np.zeros((x.shape[0], OH, OW, x.shape[3]), np.float64)
    y[:, pt:pt + x.shape[1], pl:pl + x.shape[2]] = x
    return y


def ref_concat(xs):
    y = np.zeros(xs[0].shape[:-1] + (sum(a.shape[-1] for a in xs),), np.float64)
    off = 0
    for a in xs:
        y[..., off:off + a.shape[-1]] = a
        off += a.shape[-1]
    return y


def _bcast(a, b):
    return b if b.shape == a.shape else b.reshape(a.shape[0], *([1] * (a.ndim - 2)), a.shape[-1])


def ref_binary(a, b, op):
    a = np.asarray(a, np.float64)
    b = _bcast(a, np.asarray(b, np.float64))
    return {"add": a + b, "sub": a - b, "mul": a * b, "max": np.maximum(a, b), "min": np.minimum(a, b),
            "avg": 0.5 * (a + b)}[op]


def ref_affine(x, scale, shift):
    return np.asarray(x, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)


def ref_softmax(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


# ------------------------------------------------------------------------------------------------- allowances
def act_allow(x, y):
    return 4.0 * (1.0 + np.abs(x)) * U23 * np.maximum(1.0, np.abs(y))


def lin_allow(n, S):
    return 2.0 * (np.asarray(n, np.float64) + 2.0) * U24 * S


def fused_allow(L, pre, y, mode):
    """Allowance of act(pre) where pre carries the linear allowance L."""
    return L if not mode else 2.0 * L + act_allow(pre, y)


def binary_lin(a, b, op):
    a = np.abs(np.asarray(a, np.float64))
    b = _bcast(a, np.abs(np.asarray(b, np.float64)))
    S = {"add": a + b, "sub": a + b, "mul": a * b, "avg": 0.5 * (a + b), "max": 0.0 * a, "min": 0.0 * a}[op]
    return lin_allow(1, S)


def softmax_allow(x, p):
    x = np.asarray(x, np.float64)
    d = np.abs(x - x.max(-1, keepdims=True))
    return U23 * (4.0 * (1.0 + d) + math.log2(x.shape[-1]) + 2.0) * p + 2.0 ** -126


def bf16_allow(allow, y):
    return allow + 2.0 ** -8 * np.abs(y)


def worst(got, want, allow):
    """(largest error / allowance, its index, error, allowance); any error beyond a zero allowance counts as inf."""
    err = np.abs(np.asarray(got, np.float64) - want)
    allow = np.broadcast_to(np.asarray(allow, np.float64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / allow)
    i = int(np.argmax(ratio))
    return float(ratio.flat[i]), np.unravel_index(i, err.shape), float(err.flat[i]), float(allow.flat[i])


def check(what, got, want, allow):
    """Assert |got - want| <= allow element by element; returns the largest error / allowance."""
    got = np.asarray(got, np.float64)
    assert got.shape == np.shape(want), f"{what}: shape {got.shape}, expected {np.shape(want)}"
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    r, idx, e, a = worst(got, want, allow)
    print(f"{what}: worst error/allowance {r:.3f} at {tuple(int(v) for v in idx)} (error {e:.3e}, allowance {a:.3e})")
    assert r <= 1.0, (f"{what}: element {tuple(int(v) for v in idx)} is off by {e:.3e}, allowance {a:.3e} "
                      f"(got {got[idx]!r}, expected {want[idx]!r})")
    return r


def check_bits(what, got, want):
    """Bit-exact comparison of two arrays of the same dtype through their integer views."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape}"
    iv = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.flatnonzero(got.view(iv).ravel() != want.view(iv).ravel())
    assert bad.size == 0, (f"{what}: {bad.size} elements differ, first at {np.unravel_index(bad[0], got.shape)}: "
                           f"got {got.ravel()[bad[0]]!r}, expected {want.ravel()[bad[0]]!r}")


# ------------------------------------------------------------------------------------------------ activations
ACT_POINTS = [0.0, -0.0, 1e-4, -1e-4, 19.999, -19.999, 20.0, -20.0, 20.001, -20.001, 88.0, -88.0, 100.0, -100.0]
ACT_POINTS_F32 = [1e-30, -1e-30, 1e4, -1e4]
# (mode, alpha, C, affine): every ActMode; fp32 with and without scale / shift at C 4 (vector) and 6 (scalar)
ACT_CASES_F32 = [(m, 0.1 if ACT_NAMES[m] == "leaky_relu" else 0.3, C, aff)
                 for m in range(len(ACT_NAMES)) for C in (4, 6) for aff in (False, True)]
ACT_CASES_BF16 = [(m, 0.1 if ACT_NAMES[m] == "leaky_relu" else 0.3, 8, False) for m in range(len(ACT_NAMES))]
FUSED_MODES = (0, 1, 2, ACT["swish"], ACT["gelu"], ACT["softplus"])     # relu / add_act / bn_act (bf16)
# every mode the fp32 eltwise kernel implements: all but LeakyReLU, whose slope it is not handed
ELTWISE_F32_MODES = tuple(m for m in range(len(ACT_NAMES)) if ACT_NAMES[m] != "leaky_relu")


def act_input(key, shape, bf16):
    """fp32 of `shape`: the special points, then N(0, 3)."""
    pts = ACT_POINTS + ([] if bf16 else ACT_POINTS_F32)
    x = (3.0 * _rng("act", key).standard_normal(int(np.prod(shape)))).astype(np.float32)
    x[:len(pts)] = np.asarray(pts, np.float32)
    x = x.reshape(shape)
    return to_bf16(x) if bf16 else x


@functools.lru_cache(maxsize=None)
def act_case(c, bf16=False):
    """y = act(x * scale + shift) (or act(x)); `pre` is the oracle's pre-activation value."""
    mode, alpha, C, aff = c
    k = _ns(case=c, mode=mode, alpha=alpha, C=C, x=act_input(c, (264 // C, C), bf16), scale=None, shift=None)
    pre, L = k.x.astype(np.float64), 0.0
    if aff:
        r = _rng("aff", c)
        k.scale = r.uniform(0.5, 1.5, C).astype(np.float32)
        k.shift = r.standard_normal(C).astype(np.float32)
        pre = ref_affine(k.x, k.scale, k.shift)
        L = lin_allow(1, ref_affine(np.abs(k.x), np.abs(k.scale), np.abs(k.shift)))
    k.pre, k.want = pre, ref_act(pre, mode, alpha)
    k.allow = (2.0 * L + act_allow(pre, k.want)) if mode else L + 0.0 * k.want
    return k


# ---------------------------------------------------------------------------------------- element-wise add / bn
@functools.lru_cache(maxsize=None)
def eltwise_case(c, bf16=False):
    """c = (op, mode, shape): op 'add' a + b, 'bn' a * scale[c] + shift[c], 'act' a; then ActMode `mode`."""
    op, mode, shape = c
    r = _rng("eltwise", c)
    C = shape[-1]
    k = _ns(case=c, op=op, mode=mode, a=r.standard_normal(shape).astype(np.float32), b=None, scale=None, shift=None)
    if op == "act":
        k.a = act_input(c, shape, bf16)
    if bf16:
        k.a = to_bf16(k.a)
    pre, L = k.a.astype(np.float64), 0.0 * k.a
    if op == "add":
        k.b = r.standard_normal(shape).astype(np.float32)
        if bf16:
            k.b = to_bf16(k.b)
        pre, L = ref_binary(k.a, k.b, "add"), binary_lin(k.a, k.b, "add")
    elif op == "bn":
        k.scale = r.uniform(0.5, 1.5, C).astype(np.float32)
        k.shift = r.standard_normal(C).astype(np.float32)
        pre = ref_affine(k.a, k.scale, k.shift)
        L = lin_allow(1, ref_affine(np.abs(k.a), np.abs(k.scale), np.abs(k.shift)))
    k.pre, k.want = pre, ref_act(pre, mode)
    k.allow = fused_allow(L, pre, k.want, mode)
    return k


ELTWISE_SHAPE_F32 = (2, 3, 5, 20)      # 150 float4 chunks, C a ragged chunk count
ELTWISE_SHAPE_BF16 = (2, 3, 5, 24)
ELTWISE_CASES_F32 = [(op, m, ELTWISE_SHAPE_F32) for op in ("add", "bn", "act") for m in ELTWISE_F32_MODES]
FUSED_CASES_BF16 = [(op, m, ELTWISE_SHAPE_BF16) for op in ("add", "bn", "act") for m in FUSED_MODES]

# (op, broadcast row, fused mode, shape)
BINARY_MODES = (0, 1, ACT["swish"])
BINARY_CASES_F32 = ([(op, bc, m, (2, 3, 5, C)) for op in BIN_OPS for bc in (False, True) for m in BINARY_MODES
                     for C in (8, 6)]
                    + [(op, bc, ACT["swish"], (1, 1, 3, 6)) for op in BIN_OPS for bc in (False, True)]   # n % 4 != 0
                    + [(op, True, 0, (2, 3, 5, 20)) for op in BIN_OPS])
BINARY_CASES_BF16 = [(op, bc, m, (2, 3, 5, 24)) for op in BIN_OPS for bc in (False, True) for m in BINARY_MODES]


@functools.lru_cache(maxsize=None)
def binary_case(c, bf16=False):
    op, bc, mode, shape = c
    r = _rng("binary", c)
    k = _ns(case=c, op=op, mode=mode, a=r.standard_normal(shape).astype(np.float32),
            b=r.standard_normal((shape[0], 1, 1, shape[-1]) if bc else shape).astype(np.float32))
    if bf16:
        k.a, k.b = to_bf16(k.a), to_bf16(k.b)
    k.pre = ref_binary(k.a, k.b, op)
    k.want = ref_act(k.pre, mode)
    k.allow = fused_allow(binary_lin(k.a, k.b, op), k.pre, k.want, mode)
    return k


# -------------------------------------------------------------------------------------------- depthwise conv
P1 = ((1, 1), (1, 1))
# (B, H, W, C, KH, KW, S, pads, act, alpha)
_DW_GEOM = [
    (1, 1, 1, 3, 3, 1, P1, "relu", 0.3),                      # only the centre tap is inside
    (2, 5, 7, 3, 3, 2, ((0, 1), (0, 1)), "relu6", 0.3),       # TF 'same' at stride 2
    (2, 9, 6, 5, 5, 1, ((2, 2), (2, 2)), "swish", 0.3),       # several blocks at C 20
    (1, 4, 4, 7, 7, 1, ((3, 3), (3, 3)), "gelu", 0.3),        # kernel larger than the map
    (2, 3, 10, 1, 7, 1, ((0, 0), (3, 3)), "linear", 0.3),     # KH != KW
    (2, 5, 5, 2, 2, 1, ((0, 1), (0, 1)), "sigmoid", 0.3),
    (2, 9, 11, 5, 5, 2, ((2, 2), (2, 2)), "elu", 0.3),        # 5x5 s2
    (2, 6, 5, 3, 3, 1, P1, "gelu_tanh", 0.3),
]
_DW_GEOM_F32 = _DW_GEOM + [(2, 6, 5, 3, 3, 1, P1, "leaky_relu", 0.1)]


def _with_c(geoms, Cs):
    return [g[:3] + (C,) + g[3:] for g in geoms for C in Cs]


DW_CASES_F32 = _with_c(_DW_GEOM_F32, (4, 6, 8, 20))
DW_CASES_BF16 = _with_c(_DW_GEOM, (8, 24))
# the register-blocked bf16 3x3 kernel at its threshold: 1, 2 or 3 live pixels in the last group of four
DW3_CASES = ([(1, 64, W, 1024, 3, 3, 1, P1, "hard_swish", 0.3) for W in (61, 62, 63)]
             + [(1, 64, W, 1024, 3, 3, 1, ((2, 0), (0, 2)), "relu", 0.3) for W in (61, 62, 63)])
DW3_NEIGHBOURS = [(1, 63, 63, 1024, 3, 3, 1, P1, "hard_swish", 0.3)]       # one row fewer: the generic kernel


def dw3_rule(c):
    """csrc/kernels/layers.hip `dwconv`: the register-blocked kernel serves 3x3 stride 1 from 512 blocks on."""
    B, H, W, C, KH, KW, S, pads = c[:8]
    OH, OW = out_hw(H, W, KH, KW, S, pads)
    return KH == 3 and KW == 3 and S == 1 and B * OH * ((OW + 3) // 4) * (C // 8) >= 512 * 256


@functools.lru_cache(maxsize=16)
def dw_case(c, bf16=False):
    B, H, W, C, KH, KW, S, pads, act, alpha = c
    r = _rng("dw", c)
    k = _ns(case=c, stride=S, pads=pads, mode=ACT[act], alpha=alpha,
            x=r.standard_normal((B, H, W, C)).astype(np.float32),
            w=(0.3 * r.standard_normal((KH, KW, C))).astype(np.float32),
            bias=(0.3 * r.standard_normal(C)).astype(np.float32))
    if bf16:
        k.x = to_bf16(k.x)
    k.pre = ref_dwconv(k.x, k.w, k.bias, S, pads)
    k.want = ref_act(k.pre, k.mode, alpha)
    L = lin_allow(KH * KW, ref_dwconv(np.abs(k.x), np.abs(k.w), np.abs(k.bias), S, pads))
    k.allow = fused_allow(L, k.pre, k.want, k.mode)
    return k


# ------------------------------------------------------------------------------------------------------ pools
# (B, H, W, C, k, s, pads, pad_zero, all negative)
_MAX_GEOM = [
    (2, 7, 7, 3, 2, P1, True, True),                      # folded pad 1, all negative: the border gives 0
    (2, 5, 7, 2, 2, ((0, 1), (0, 1)), False, False),      # 'same' on an odd map
    (2, 6, 5, 3, 1, P1, False, False),                    # 3x3 s1 'same'
    (2, 6, 5, 3, 1, P1, True, False),
]
MAXPOOL_CASES_F32 = _with_c(_MAX_GEOM, (4, 8, 20))
MAXPOOL_CASES_BF16 = _with_c(_MAX_GEOM, (8, 24))


def _some_negative(x):
    """An all-negative top-left 3x3 (and first image's channel 0): a zero-initialised maximum shows."""
    x[:, :3, :3] = -np.abs(x[:, :3, :3]) - 0.1
    x[0, ..., 0] = -np.abs(x[0, ..., 0]) - 0.1
    return x


@functools.lru_cache(maxsize=None)
def maxpool_case(c, bf16=False):
    B, H, W, C, kk, s, pads, pad_zero, neg = c
    x = _rng("maxpool", c).standard_normal((B, H, W, C)).astype(np.float32)
    x = (-np.abs(x) - 0.1).astype(np.float32) if neg else _some_negative(x)
    if bf16:
        x = to_bf16(x)
    return _ns(case=c, x=x, k=kk, s=s, pads=pads, pad_zero=pad_zero, want=ref_maxpool(x, kk, s, pads, pad_zero))


# (B, H, W, C, kh, kw, s, pads)
P0 = ((0, 0), (0, 0))
_AVG_GEOM = [
    (2, 6, 8, 2, 2, 2, P0),                               # 2x2 s2 valid
    (2, 5, 6, 3, 3, 1, P1),                               # 'same': corner count 4, edge count 6
    (2, 6, 6, 3, 3, 2, ((0, 1), (0, 1))),
    (2, 4, 9, 1, 3, 1, ((0, 0), (1, 1))),                 # non-square window
]
AVGPOOL_CASES_F32 = _with_c(_AVG_GEOM, (4, 6, 8, 20))
AVGPOOL_CASES_BF16 = _with_c(_AVG_GEOM, (8, 24))


@functools.lru_cache(maxsize=None)
def avgpool_case(c, bf16=False):
    B, H, W, C, kh, kw, s, pads = c
    x = _rng("avgpool", c).standard_normal((B, H, W, C)).astype(np.float32)
    if bf16:
        x = to_bf16(x)
    want, n = ref_avgpool(x, kh, kw, s, pads)
    return _ns(case=c, x=x, k=(kh, kw), s=s, pads=pads, want=want, count=n,
               allow=lin_allow(n, ref_avgpool(np.abs(x), kh, kw, s, pads)[0]))


# (B, H, W, C); maps of >= 1024 pixels take the sliced two-pass kernels
GAP_LARGE = [(2, 32, 32, 8), (1, 33, 33, 2056), (600, 32, 32, 8)]     # threshold; 257 chunks; one slice
GAP_CASES_BF16 = [(2, h, w, C) for h, w in ((1, 1), (1, 3), (7, 7)) for C in (8, 520)] + GAP_LARGE
GAP_CASES_F32 = [(2, h, w, C) for h, w in ((1, 1), (1, 3), (5, 10)) for C in (4, 260)] + GAP_LARGE
GMP_CASES = [(2, h, w, C) for h, w in ((1, 1), (1, 3), (7, 7)) for C in (8, 1040)]


@functools.lru_cache(maxsize=None)
def gap_case(c, bf16=False):
    x = _rng("gap", c).standard_normal(c).astype(np.float32)
    if bf16:
        x = to_bf16(x)
    want = ref_gap(x)
    return _ns(case=c, x=x, want=want, allow=lin_allow(c[1] * c[2], ref_gap(np.abs(x))))


@functools.lru_cache(maxsize=None)
def gmp_case(c, bf16=False):
    x = _rng("gmp", c).standard_normal(c).astype(np.float32)
    x[0] = -np.abs(x[0]) - 0.1                    # an all-negative image
    if bf16:
        x = to_bf16(x)
    return _ns(case=c, x=x, want=ref_gmp(x))


# ---------------------------------------------------------------------------------------------- concat, pad
CONCAT_CASES_BF16 = [(8, 16), (20, 12, 5), (16, 3)]       # real channels per input; stored padded to 8
CONCAT_CASES_F32 = [(8, 8), (6, 8), (4, 6, 4)]            # (6, 8): an aligned input at offset 6
CONCAT_PIXELS = (2, 3, 5)
SENTINEL = -777.0


@functools.lru_cache(maxsize=None)
def concat_case(c, bf16=False):
    r = _rng("concat", c)
    xs = [r.standard_normal(CONCAT_PIXELS + (ch,)).astype(np.float32) for ch in c]
    if bf16:
        xs = [to_bf16(a) for a in xs]
    return _ns(case=c, xs=xs, want=ref_concat(xs))


# (B, H, W, C, pad_t, pad_l, extra rows and columns after the map)
PAD_CASES_F32 = [(2, 3, 4, C, p[0], p[1], e) for C in (4, 6) for p in ((1, 1), (0, 3)) for e in (0, 2)]
PAD_CASES_BF16 = [(2, 3, 4, 8, p[0], p[1], e) for p in ((1, 1), (0, 3)) for e in (0, 2)]


@functools.lru_cache(maxsize=None)
def pad_case(c, bf16=False):
    B, H, W, C, pt, pl, e = c
    x = _rng("pad", c).standard_normal((B, H, W, C)).astype(np.float32)
    if bf16:
        x = to_bf16(x)
    OH, OW = H + pt + e, W + pl + e
    return _ns(case=c, x=x, pt=pt, pl=pl, OH=OH, OW=OW, want=ref_pad(x, pt, pl, OH, OW))


# ---------------------------------------------------------------------------------------------------- softmax
SOFTMAX_CASES = [(rows, N, False) for N in (1, 10, 255, 256, 257, 1000) for rows in (1, 5)] + [(5, 1000, True)]


@functools.lru_cache(maxsize=None)
def softmax_case(c):
    rows, N, spread = c
    x = (5.0 * _rng("softmax", c).standard_normal((rows, N))).astype(np.float32)
    if spread:                                    # 160 between the largest and the smallest entry of row 0
        x[0] = np.clip(x[0], -60.0, 60.0)
        x[0, 0], x[0, 1] = 80.0, -80.0
    want = ref_softmax(x)
    return _ns(case=c, x=x, want=want, allow=softmax_allow(x, want))


# ------------------------------------------------------------------------------------------------------ casts
def cast_input():
    """fp32 values whose bf16 rounding matters: exact ties (to even both ways), their neighbours, +-0, +-inf, the
    largest finite float (rounds to inf), the largest bf16, denormals, then N(0, 1) at several scales."""
    bits = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0x00000000, 0x80000000,
            0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F0000, 0x7F7F8000, 0x7F7F7FFF, 0x00000001,
            0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0xBF808000, 0xBF818000]
    sp = np.asarray(bits, np.uint32).view(np.float32)
    r = _rng("cast")
    rnd = (r.standard_normal(1002) * np.repeat([1e-20, 1.0, 1e20], 334)).astype(np.float32)
    return np.concatenate([sp, rnd])              # 1024 values


INPUT_PACK_CASES = [(C, Cp) for C in (1, 3, 4, 8, 9, 11) for Cp in (8, 16) if C <= Cp]


def input_pack_input(c):
    C, _ = c
    x = cast_input()
    x = x[np.isfinite(x)]
    n = x.size // C * C
    return np.ascontiguousarray(x[:n].reshape(1, 1, n // C, C))


# ------------------------------------------------------------------------------------- second grid-stride pass
def crop_rows(H, OH, kh, s, pt, first=2, last=4):
    """Input row ranges and pads that reproduce output rows [0, first) and [OH - last, OH) of a map of H rows:
    ((r0, r1, (pt, pb)), ...); the bottom crop's pb pads up to what its last window reads."""
    top = (0, min(H, (first - 1) * s - pt + kh), (pt, max(0, (first - 1) * s - pt + kh - H)))
    r0 = (OH - last) * s - pt
    need = (OH - 1) * s - pt + kh
    bot = (max(r0, 0), H, (max(-r0, 0), max(need - H, 0)))
    return top, bot


# ----------------------------------------------------------------------------------------------- tiny graphs
def addbn_graph():
    """Input(8,8,16) -> Conv2D 1x1 -> Add(conv, input) -> swish ('sg') -> BatchNormalization -> gelu ('out'): the plan
    fuses both activations into the `add` and `bn` steps (modes 3 and 8)."""
    from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
    g = Graph("addbn")
    g.add(Layer("in", "input", [], {"shape": (8, 8, 16)}))
    g.add(Layer("conv", "conv", ["in"], {"filters": 16, "kernel": (1, 1), "stride": 1, "padding": "valid",
                                         "use_bias": True}))
    g.add(Layer("add", "add", ["conv", "in"]))
    g.add(Layer("sg", "act", ["add"], {"fn": "swish"}))
    g.add(Layer("bn", "bn", ["sg"], {"epsilon": 1e-3}))
    g.add(Layer("out", "act", ["bn"], {"fn": "gelu"}))
    return g


def se_graph():
    """Multiply by a broadcast squeeze-excite row, then hard_swish ('out')."""
    from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
    g = Graph("se")
    g.add(Layer("in", "input", [], {"shape": (8, 8, 16)}))
    g.add(Layer("squeeze", "gap", ["in"]))
    g.add(Layer("reshape", "reshape", ["squeeze"], {"shape": (1, 1, 16)}))
    g.add(Layer("se", "conv", ["reshape"], {"filters": 16, "kernel": (1, 1), "stride": 1, "padding": "same",
                                            "use_bias": True, "activation": "sigmoid"}))
    g.add(Layer("excite", "binary", ["in", "se"], {"fn": "mul"}))
    g.add(Layer("out", "act", ["excite"], {"fn": "hard_swish"}))
    return g
