"""Cases, inputs and the float64 oracles shared by the transposed-convolution, upsample and crop tests (CPU ops,
HIP kernels, guard band).

A deconv case is ``(N, H, W, Cin, Cout, k, s, padding, act)``; `k` is one int or ``(kh, kw)``, `act` one of
'none' / 'relu' / 'relu6'.  They are the smallest at which csrc/kernels/deconv_f32.hip can go wrong: k == s on an
odd map with a partial pixel tile, phases of 4 / 2 / 2 / 1 taps, a non-zero start in the frame (pb = 1), a single
phase, unequal phase pixel counts, a phase without taps (k < s), and for the generic path odd channel counts, a
non-square kernel and a 5x5 stride 3 on a narrow map.

Inputs are standard normal, kernels (Keras HWOI: kh, kw, Cout, Cin) scaled by 1 / sqrt(taps per output * Cin) so
outputs are O(1).  The oracle is the issue's definition in float64: the full scatter by
`F.conv_transpose2d`, `out` elements from `pb` per axis, zeros past the end of the frame, then bias and the
activation.  It is computed once per case and cached (callers must not modify it).
"""
import functools
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

MFMA_CASES = [
    (2, 5, 7, 32, 16, 2, 2, "same", "relu"),         # k == s, odd map, partial pixel tile
    (1, 9, 6, 64, 48, 3, 2, "same", "none"),         # phases of 4/2/2/1 taps, pb = 0, Cout not a multiple of 64
    (2, 4, 5, 16, 32, 4, 2, "same", "relu6"),        # pb = 1
    (1, 6, 6, 32, 16, 3, 1, "same", "relu"),         # one phase
    (1, 5, 4, 16, 16, 3, 2, "valid", "none"),        # output 11x9, phases of unequal pixel counts
    (1, 3, 4, 16, 16, 2, 3, "valid", "relu"),        # k < s: a tap-less phase is bias only
]
GENERIC_CASES = [
    (2, 5, 5, 3, 5, 3, 2, "same", "relu"),           # odd channel counts
    (1, 4, 6, 20, 24, (3, 2), 2, "same", "none"),    # non-square kernel
    (1, 7, 3, 8, 8, 5, 3, "same", "relu6"),          # 5x5 stride 3 on a narrow map
]
CASES = MFMA_CASES + GENERIC_CASES
ACT = {"none": 0, "relu": 1, "relu6": 2}

# (size, interpolation, (N, H, W, C))
UPSAMPLE_CASES = [
    (2, "nearest", (2, 5, 7, 24)),
    ((2, 3), "nearest", (1, 3, 4, 6)),
    (2, "bilinear", (1, 4, 5, 16)),
    ((3, 2), "bilinear", (2, 3, 3, 5)),
    (4, "bilinear", (1, 1, 1, 8)),
]
# (crop, (N, H, W, C))
CROP_CASES = [(((1, 2), (0, 3)), (2, 6, 7, 12)), (((1, 2), (0, 3)), (1, 5, 5, 3))]


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_len(size, k, s, padding):
    return size * s if padding == "same" else size * s + max(k - s, 0)


def pad_before(k, s, padding):
    return max(k - s, 0) // 2 if padding == "same" else 0


def ref_deconv(x, kern, bias, s, padding, act):
    """float64 oracle: NHWC x, Keras kernel (kh, kw, Cout, Cin)."""
    kh, kw = kern.shape[:2]
    full = F.conv_transpose2d(torch.from_numpy(x).double().permute(0, 3, 1, 2),
                              torch.from_numpy(kern).double().permute(3, 2, 0, 1), None, stride=s)
    oh, ow = out_len(x.shape[1], kh, s, padding), out_len(x.shape[2], kw, s, padding)
    pt, pl = pad_before(kh, s, padding), pad_before(kw, s, padding)
    full = F.pad(full, (0, max(pl + ow - full.shape[3], 0), 0, max(pt + oh - full.shape[2], 0)))
    y = full[:, :, pt:pt + oh, pl:pl + ow].permute(0, 2, 3, 1) + torch.from_numpy(bias).double()
    if act == 1:
        y = y.clamp_min(0)
    elif act == 2:
        y = y.clamp(0, 6)
    return y.contiguous().numpy()


@functools.lru_cache(maxsize=None)
def case(c):
    N, H, W, Cin, Cout, k, s, padding, act = c
    kh, kw = pair(k)
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    o = types.SimpleNamespace(case=c, N=N, H=H, W=W, Cin=Cin, Cout=Cout, kh=kh, kw=kw, stride=s, padding=padding,
                              act=ACT[act], pads=(pad_before(kh, s, padding), pad_before(kw, s, padding)))
    o.x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    taps = -(-kh // s) * -(-kw // s)
    o.kern = (rng.standard_normal((kh, kw, Cout, Cin)) / np.sqrt(taps * Cin)).astype(np.float32)      # Keras HWOI
    o.bias = rng.standard_normal(Cout).astype(np.float32)
    o.kern_io = np.ascontiguousarray(o.kern.transpose(0, 1, 3, 2))     # (kh, kw, Cin, Cout): what the packers take
    o.want = ref_deconv(o.x, o.kern, o.bias, s, padding, o.act)
    o.out_shape = o.want.shape
    assert o.out_shape == (N, out_len(H, kh, s, padding), out_len(W, kw, s, padding), Cout)
    return o


def zero_stuffed(c):
    """The same layer as a stride-1 dense conv on the zero-stuffed input: (x stuffed and padded, HWIO kernel,
    ((0, 0), (0, 0)) pads).  x is spread with s - 1 zeros between pixels, padded by k - 1 - pb before and as
    much after as the output needs, and correlated with the kernel flipped in both axes."""
    s = c.stride
    pt, pl = c.pads
    OH, OW = c.out_shape[1:3]
    rows, cols = OH + c.kh - 1, OW + c.kw - 1
    z = np.zeros((c.N, rows, cols, c.Cin), np.float32)
    t0, l0 = c.kh - 1 - pt, c.kw - 1 - pl
    for i in range(c.H):
        for j in range(c.W):
            r, q = t0 + i * s, l0 + j * s
            if 0 <= r < rows and 0 <= q < cols:
                z[:, r, q] = c.x[:, i, j]
    return z, np.ascontiguousarray(c.kern_io[::-1, ::-1])


def bilinear_explicit(x, size):
    """The explicit half-pixel formula in float64: fy = max((oy + 0.5) / sh - 0.5, 0), y0 = floor(fy),
    y1 = min(y0 + 1, H - 1), weight fy - y0; the x axis alike."""
    sh, sw = pair(size)
    N, H, W, C = x.shape
    x = x.astype(np.float64)

    def axis(n_out, s, n_in):
        f = np.maximum((np.arange(n_out) + 0.5) / s - 0.5, 0.0)
        i0 = np.floor(f).astype(int)
        return i0, np.minimum(i0 + 1, n_in - 1), f - i0
    y0, y1, wy = axis(H * sh, sh, H)
    x0, x1, wx = axis(W * sw, sw, W)
    wy, wx = wy[None, :, None, None], wx[None, None, :, None]
    top = x[:, y0][:, :, x0] * (1 - wx) + x[:, y0][:, :, x1] * wx
    bot = x[:, y1][:, :, x0] * (1 - wx) + x[:, y1][:, :, x1] * wx
    return top * (1 - wy) + bot * wy


@functools.lru_cache(maxsize=None)
def upsample_case(c):
    size, interp, shape = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    o = types.SimpleNamespace(case=c, size=pair(size), bilinear=interp == "bilinear", shape=shape)
    o.x = rng.standard_normal(shape).astype(np.float32)
    sh, sw = o.size
    if o.bilinear:
        o.want = bilinear_explicit(o.x, o.size)
    else:
        o.want = np.repeat(np.repeat(o.x, sh, axis=1), sw, axis=2).astype(np.float64)
    o.out_shape = o.want.shape
    return o


@functools.lru_cache(maxsize=None)
def crop_case(c):
    crop, shape = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    o = types.SimpleNamespace(case=c, crop=crop, shape=shape)
    o.x = rng.standard_normal(shape).astype(np.float32)
    (t, b), (l, r) = crop
    o.want = np.ascontiguousarray(o.x[:, t:shape[1] - b, l:shape[2] - r])
    o.out_shape = o.want.shape
    return o


def bf16_padded(x):
    """fp32 NHWC -> the executor's bf16 layout: channels padded to a multiple of 8 (zeros), as a torch tensor;
    and the values the bf16 rounding left, as float64."""
    t = torch.from_numpy(x).to(torch.bfloat16)
    cp = -(-x.shape[-1] // 8) * 8
    out = torch.zeros(x.shape[:-1] + (cp,), dtype=torch.bfloat16)
    out[..., :x.shape[-1]] = t
    return out, t.double().numpy()
