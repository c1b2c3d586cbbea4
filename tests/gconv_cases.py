"""Shapes, inputs and the float64 oracle shared by the grouped-convolution tests (CPU op, HIP kernel, guard band).

A shape is ``(B, H, W, Cin, Cout, G, k, stride, pad)``; `pad` is one int (all four sides) or Keras-style
``((top, bottom), (left, right))``.  They are the smallest at which csrc/kernels/gconv_f32.hip can go wrong:
every channels-per-group width of the MFMA path (4, 8, 16, 32: an N tile spanning 4 / 2 / 1 / half a group),
odd maps whose 126 pixels leave a partial pixel tile, stride 2 on an odd map, a 64-channel block that is only
half there (Cout 32), the ResNeXt stage-5 layer itself, and for the generic path a 5x5 with 12 channels per
group, unequal group widths with Cout % 16 != 0, and a grouped 1x1.

Inputs are standard normal, kernels scaled by 1 / sqrt(taps * Cin/G) so outputs are O(1); the oracle is
float64 `F.conv2d(groups=)`, computed once per shape and cached (callers must not modify it).  The
activation mode cycles 0 / 1 / 2 over the list so each is used.
"""
import functools
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

SHAPES = [
    (2, 9, 7, 32, 32, 8, 3, 1, 1),            # CG 4: an N tile spans 4 groups; odd map, 126 pixels
    (2, 9, 7, 128, 128, 32, 3, 2, 1),         # CG 4, stride 2 on an odd map (ResNeXt stage 2 -> 3 form)
    (2, 8, 8, 64, 64, 8, 3, 1, 1),            # CG 8: an N tile spans 2 groups
    (2, 8, 8, 64, 64, 4, 3, 1, 1),            # CG 16: tile == group
    (2, 8, 8, 64, 64, 2, 3, 1, 1),            # CG 32: two N tiles per group
    (2, 7, 7, 1024, 1024, 32, 3, 1, 1),       # the ResNeXt stage-5 layer itself
    (2, 10, 10, 48, 48, 4, 5, 2, 2),          # CG 12, 5x5: generic path
    (1, 6, 5, 24, 36, 3, 3, 1, 1),            # Cin/G != Cout/G, Cout % 16 != 0: generic path
    (2, 5, 5, 20, 30, 10, 1, 1, 0),           # grouped 1x1
    (2, 8, 8, 32, 32, 8, 3, 2, ((0, 1), (0, 1))),     # asymmetric ('same', stride 2) pads
]
MFMA_SHAPES = [s for i, s in enumerate(SHAPES) if i in (0, 1, 2, 3, 4, 5, 9)]


def pads_of(pad):
    return ((pad, pad), (pad, pad)) if isinstance(pad, int) else pad


def ref_gconv(x, kern, bias, groups, stride, pads, act):
    """float64 oracle: NHWC x, Keras grouped kernel (kh, kw, Cin / G, Cout)."""
    (pt, pb), (pl, pr) = pads
    xt = F.pad(torch.from_numpy(x).double().permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xt, torch.from_numpy(kern).double().permute(3, 2, 0, 1), torch.from_numpy(bias).double(),
                 stride=stride, groups=groups).permute(0, 2, 3, 1)
    if act == 1:
        y = y.clamp_min(0)
    elif act == 2:
        y = y.clamp(0, 6)
    return y.contiguous().numpy()


@functools.lru_cache(maxsize=None)
def case(shape):
    B, H, W, Cin, Cout, G, k, s, pad = shape
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    c = types.SimpleNamespace(shape=shape, B=B, H=H, W=W, Cin=Cin, Cout=Cout, G=G, k=k, stride=s,
                              pads=pads_of(pad), act=SHAPES.index(shape) % 3)
    c.x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    c.kern = (rng.standard_normal((k, k, Cin // G, Cout)) / np.sqrt(k * k * (Cin // G))).astype(np.float32)
    c.bias = rng.standard_normal(Cout).astype(np.float32)
    c.want = ref_gconv(c.x, c.kern, c.bias, G, s, c.pads, c.act)
    c.out_shape = c.want.shape
    return c


def dense_kernel(kern, groups):
    """The grouped kernel expanded to a dense block-diagonal HWIO kernel (kh, kw, Cin, Cout)."""
    kh, kw, cgi, cout = kern.shape
    cgo = cout // groups
    d = np.zeros((kh, kw, cgi * groups, cout), np.float32)
    for g in range(groups):
        d[:, :, g * cgi:(g + 1) * cgi, g * cgo:(g + 1) * cgo] = kern[..., g * cgo:(g + 1) * cgo]
    return d
