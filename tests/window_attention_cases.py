"""Cases, inputs, the float64 oracle and the allowance shared by the window attention tests (native CPU op, HIP
kernels, guard band).

A case is ``(B, H, W, M, shift, heads, d, probe)``.  The input is what the `winattn` step is handed: the NHWC map
`qkv` [B * H * W][heads * 3 d], rows of [Q | K | V], head-major inside each part, Q already scaled, N(0, 1), seeded
per case by the crc32 of the case; and the raw relative position bias table [(2M-1)^2][heads], N(0, 1) too, so a
dropped or mis-indexed bias shows.  The cases are the smallest at which csrc/kernels/window_attention.hip can go
wrong, for its 64-query / 32-key tiles (asserted by tests/test_window_attention.py against the kernels module):

* (1,7,7,7,0,1,16): one window, no shift (Swin's last stage);
* (1,14,14,7,3,3,32): all four mask classes; 49 tokens, off both tiles; Swin's head shape;
* (2,14,21,7,3,1,16): non-square, two images: an H / W swap or an image-stride slip;
* (2,16,16,8,4,2,32): M^2 = 64, exactly a query tile and two key tiles;
* (3,4,4,2,1,1,16): four tokens per window;
* (1,24,24,12,6,1,16): 144 tokens, three query tiles and five key tiles (Swin at 384);
* (1,8,8,4,0,1,64) and (1,14,14,7,3,1,128): the other register sizes;
* (2,6,9,3,1,3,6) and (1,12,8,4,2,2,24): the plain kernel; 3 x 6 channels are padded on both sides in bf16.

Probes:

* `ascending` / `descending` on (1,24,24,12,6,1,16): scores of magnitude 100 ramp over the token's index inside
  its window after the roll, so the row maximum sits in the last / the first key tile;
* `masked_dominant` on (2,14,14,7,3,2,32): every query is 100 u; keys at original positions y < s or x < s (the
  strips that wrap around) are u + 0.01 N, all other keys 0.01 N.  A query outside the strips then has raw scores
  of about 100 on keys it must mask, and after the additive -100 they weigh as much as the unmasked ones: a hard
  (-inf) mask moves the result by 1.9, no mask by 1.7, ignoring the shift by 3.0 and ignoring the bias by 1.9,
  against an allowance of 6.7e-5 (tests/test_window_attention.py asserts that each of the four fails).

The oracle is float64 numpy written from the published definition (Liu et al. 2021): roll by (-s, -s), cut into
M x M windows, scores Q K^T + table[index] with index[(i,j),(k,l)] = (i-k+M-1)(2M-1) + (j-l+M-1), -100 between
different regions of the rolled frame (rows [0, H-M), [H-M, H-s), [H-s, H), columns alike, region = 3 x row part +
column part) when s > 0, softmax, P V, un-window, roll back.

Allowance, the project's form: ``max(4 e_ref, 2e-5 max(1, max|want|))``, where e_ref is the error against the
oracle of torch's fp32 CPU path on the same composition: the reference's own error, never the code under test's.
Observed e_ref over the cases: 4.9e-7 .. 2.3e-5; 4 e_ref stays below the floor (3.9e-5 .. 7.8e-5) on all but the
three probes, where 4 e_ref = 9.1e-5, 7.9e-5 and 6.7e-5 decides; the max() form covers that (printed per case by
the tests).

In bf16 the input is the case rounded to bf16, the oracle and the allowance follow the rounded values, and the
bound is ``2^-8 |want| + allowance`` (one rounding of the output).

Cached per case: callers must not modify what they get.
"""
import functools
import types
import zlib

import numpy as np
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.attention import (
    window_attention_path, window_attention_tiles)

QT, KT = window_attention_tiles()          # queries per block, keys per LDS tile of the MFMA path

CASES = [
    (1, 7, 7, 7, 0, 1, 16, None),
    (1, 14, 14, 7, 3, 3, 32, None),
    (2, 14, 21, 7, 3, 1, 16, None),
    (2, 16, 16, 8, 4, 2, 32, None),
    (3, 4, 4, 2, 1, 1, 16, None),
    (1, 24, 24, 12, 6, 1, 16, None),
    (1, 8, 8, 4, 0, 1, 64, None), (1, 14, 14, 7, 3, 1, 128, None),
    (2, 6, 9, 3, 1, 3, 6, None), (1, 12, 8, 4, 2, 2, 24, None),
    (1, 24, 24, 12, 6, 1, 16, "ascending"), (1, 24, 24, 12, 6, 1, 16, "descending"),
    (2, 14, 14, 7, 3, 2, 32, "masked_dominant"),
]
# the 49-token shifted, the one-window, the non-square two-image, the 144-token, the padded plain one
GUARD_CASES = [(1, 14, 14, 7, 3, 3, 32, None), (1, 7, 7, 7, 0, 1, 16, None), (2, 14, 21, 7, 3, 1, 16, None),
               (1, 24, 24, 12, 6, 1, 16, None), (2, 6, 9, 3, 1, 3, 6, None)]


def widths(c):
    """(qkv width, output width) of a case."""
    return 3 * c[5] * c[6], c[5] * c[6]


def split(qkv, B, H, W, h, d):
    x = qkv.reshape(B, H, W, -1)
    return tuple(x[..., i * h * d:(i + 1) * h * d].reshape(B, H, W, h, d) for i in range(3))


def rel_index(M):
    """index[(i, j), (k, l)] = (i - k + M - 1)(2M - 1) + (j - l + M - 1), (M^2, M^2)."""
    i, j = np.divmod(np.arange(M * M), M)
    return (i[:, None] - i[None, :] + M - 1) * (2 * M - 1) + (j[:, None] - j[None, :] + M - 1)


def region_map(H, W, M, s):
    """Region of every position of the rolled frame, (H, W) ints: 3 x row part + column part."""
    def parts(n):
        p = np.zeros(n, np.int64)
        p[n - M:n - s] = 1
        p[n - s:] = 2
        return p
    return 3 * parts(H)[:, None] + parts(W)[None, :]


def _windows(t, M):
    """(B, H, W, ...) -> (B, windows, M^2, ...)."""
    B, H, W = t.shape[:3]
    rest = t.shape[3:]
    t = t.reshape((B, H // M, M, W // M, M) + rest)
    t = np.moveaxis(t, 3, 2)                                        # (B, nwy, nwx, M, M, ...)
    return t.reshape((B, (H // M) * (W // M), M * M) + rest)


def published_mask(H, W, M, s):
    """(windows, M^2, M^2): -100 where the query and the key lie in different regions, else 0."""
    r = _windows(region_map(H, W, M, s)[None], M)[0]                # (windows, M^2)
    return np.where(r[:, :, None] != r[:, None, :], -100.0, 0.0)


def ref_window_attention(qkv, table, B, H, W, M, s, h, d, mask_value=-100.0, use_shift=True, use_bias=True):
    """float64 oracle from the published definition -> [B * H * W][h * d].  The keyword arguments build the wrong
    variants that the probes must tell apart (a hard mask, no mask, no shift, no bias)."""
    q, k, v = split(np.asarray(qkv, np.float64), B, H, W, h, d)
    sh = s if use_shift else 0
    q, k, v = (_windows(np.roll(t, (-sh, -sh), axis=(1, 2)), M) for t in (q, k, v))      # (B, n, T, h, d)
    sc = np.einsum("bnqhd,bnkhd->bnhqk", q, k)
    if use_bias:
        sc = sc + np.asarray(table, np.float64)[rel_index(M)].transpose(2, 0, 1)         # (h, T, T)
    if sh and mask_value != 0.0:
        different = published_mask(H, W, M, sh) != 0
        sc = sc + np.where(different, mask_value, 0.0)[None, :, None]
    p = np.exp(sc - sc.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = np.einsum("bnhqk,bnkhd->bnqhd", p, v)                       # (B, n, T, h, d)
    o = o.reshape(B, H // M, W // M, M, M, h * d)
    o = np.moveaxis(o, 2, 3).reshape(B, H, W, h * d)
    return np.roll(o, (sh, sh), axis=(1, 2)).reshape(B * H * W, h * d)


def library_f32(qkv, table, B, H, W, M, s, h, d):
    """torch's fp32 path on the CPU, the same composition: roll, partition, matmul + bias + mask, softmax, matmul,
    reverse, roll back."""
    x = torch.from_numpy(np.ascontiguousarray(qkv, np.float32)).reshape(B, H, W, 3, h, d)
    x = torch.roll(x, shifts=(-s, -s), dims=(1, 2))
    x = x.reshape(B, H // M, M, W // M, M, 3, h, d).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, -1, h, M * M, d)
    q, k, v = x[0], x[1], x[2]                                      # (B * n, h, T, d)
    bias = torch.from_numpy(np.asarray(table, np.float32))[torch.from_numpy(rel_index(M)).reshape(-1)]
    a = q @ k.transpose(-2, -1) + bias.reshape(M * M, M * M, h).permute(2, 0, 1)
    if s:
        mask = torch.from_numpy(published_mask(H, W, M, s).astype(np.float32))           # (n, T, T)
        a = (a.reshape(B, -1, h, M * M, M * M) + mask[None, :, None]).reshape(-1, h, M * M, M * M)
    o = (torch.softmax(a, dim=-1) @ v).permute(0, 2, 1, 3)          # (B * n, T, h, d)
    o = o.reshape(B, H // M, W // M, M, M, h * d).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, h * d)
    return torch.roll(o, shifts=(s, s), dims=(1, 2)).reshape(B * H * W, h * d).numpy()


def f32_allowance(qkv, table, c, want):
    B, H, W, M, s, h, d, _ = c
    e_ref = float(np.abs(library_f32(qkv, table, B, H, W, M, s, h, d).astype(np.float64) - want).max())
    return e_ref, max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))


def _make(c):
    B, H, W, M, s, h, d, probe = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    q = rng.standard_normal((B, H, W, h, d))
    k = rng.standard_normal((B, H, W, h, d))
    v = rng.standard_normal((B, H, W, h, d))
    table = rng.standard_normal(((2 * M - 1) ** 2, h)).astype(np.float32)
    if probe in ("ascending", "descending"):
        # scores 100 * ramp(token index inside its window, after the roll) + N(0, 1)
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        ry, rx = (np.arange(H) - s) % H, (np.arange(W) - s) % W             # rolled coordinates of a position
        tok = (ry % M)[:, None] * M + (rx % M)[None, :]
        ramp = tok / (M * M - 1)
        ramp = ramp if probe == "ascending" else 1.0 - ramp
        k = ramp[None, :, :, None, None] * u + 0.01 * k          # a step of 0.7 per token under noise of about 1
        q = 100.0 * u + q
    elif probe == "masked_dominant":
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        strip = (np.arange(H) < s)[:, None] | (np.arange(W) < s)[None, :]   # original positions that wrap around
        k = strip[None, :, :, None, None] * u + 0.01 * k
        q = np.broadcast_to(100.0 * u, q.shape)
    qkv = np.concatenate([t.reshape(B * H * W, -1) for t in (q, k, v)], axis=1).astype(np.float32)
    return qkv, table


@functools.lru_cache(maxsize=None)
def case(c):
    B, H, W, M, s, h, d, probe = c
    k = types.SimpleNamespace(case=c, B=B, H=H, W=W, M=M, shift=s, heads=h, d=d, probe=probe,
                              path=window_attention_path(d), rows=B * H * W)
    k.qkv, k.table = _make(c)
    k.want = ref_window_attention(k.qkv, k.table, B, H, W, M, s, h, d)
    k.e_ref, k.allow = f32_allowance(k.qkv, k.table, c, k.want)
    return k


@functools.lru_cache(maxsize=None)
def case_bf16(c):
    """The case rounded to bf16 (oracle and allowance follow the rounded values; the table stays fp32, as the
    packed bias does) with the padded row strides of the bf16 layout: both widths rounded up to 8."""
    k = types.SimpleNamespace(**vars(case(c)))
    k.qkv = torch.from_numpy(k.qkv).to(torch.bfloat16).float().numpy()
    k.want = ref_window_attention(k.qkv, k.table, k.B, k.H, k.W, k.M, k.shift, k.heads, k.d)
    k.e_ref, k.allow = f32_allowance(k.qkv, k.table, c, k.want)
    w_in, w_out = widths(c)
    k.w_in, k.w_out, k.ld_in, k.ld_out = w_in, w_out, (w_in + 7) // 8 * 8, (w_out + 7) // 8 * 8
    return k


# ------------------------------------------------------------ space_to_depth
S2D_CASES = [(B, H, W, C) for (B, H, W) in ((2, 4, 6), (1, 2, 2)) for C in (4, 6, 32)]


@functools.lru_cache(maxsize=None)
def s2d_case(c):
    B, H, W, C = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    return rng.standard_normal((B, H, W, C)).astype(np.float32)


def ref_space_to_depth(x):
    """The four-slice definition: the concatenation of x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2]."""
    return np.concatenate([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], axis=-1)
