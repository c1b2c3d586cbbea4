"""Cases, inputs, the float64 oracle and the allowance shared by the attention tests (native CPU op, HIP kernels,
guard band).

A case is ``(B, T, heads, key_dim, value_dim, probe)``.  The input is what the attention step is handed: `qkv`
[B * T][heads * (2 d + dv)], rows of [Q | K | V], head-major inside each part, Q already scaled.  The cases are the
smallest at which csrc/kernels/attention.hip can go wrong, with the tile sizes read from the kernels module:

* T = 1; T one below, at and one above the key tile and the query tile; T = 197 (ViT at 224 x 224) with two heads;
* B = 2 and 3 with T off both tiles: a read that runs past an image's rows lands in the next image's valid rows,
  which is finite, so only a wrong value can show it;
* heads 1 and 3; (d, dv) = (16, 16), (32, 16), (64, 64), (128, 128) for the MFMA path (all three register sizes,
  d != dv), (24, 24), (8, 40) and (6, 5) for the plain kernel (the last with channel counts that the bf16 layout
  pads on both sides);
* three softmax probes with scores of magnitude about 100 over three key tiles: the row maximum in the last key
  tile (ascending), in the first (descending), and one dominant key per row at a random place.  They fail a
  kernel that omits the maximum (exp(100) overflows fp32) or rescales the running sum wrongly.

Inputs are N(0, 1) (scores then have a standard deviation of sqrt(d)), seeded per case.  The oracle is float64
numpy.  Allowance, the project's layernorm form: ``max(4 e_ref, 2e-5 max(1, max|want|))``, where e_ref is the
error against the oracle of the library's fp32 path on the CPU (torch matmul, softmax, matmul on the same
inputs): the reference's own error, not the code under test's.  The factor 4 covers a different summation order
and the hardware exponent.  Observed e_ref over the cases: 0 (T = 1, and the dominant-key probe, whose rows
reproduce one V row) to 9.4e-6 (the ascending probe; 9.0e-6 at d = 128), so 4 e_ref stays below the floor, which is
2e-5 x max|want| = 3.2e-5 .. 8.5e-5, and the floor decides every case (printed per case by tests/test_attention.py).

In bf16 the input is the case rounded to bf16, the oracle and the allowance follow the rounded values, and the
bound is ``2^-8 |want| + allowance`` (one rounding of the output), as in tests/test_layernorm_gpu.py.

Cached per case: callers must not modify what they get.
"""
import functools
import types
import zlib

import numpy as np
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.attention import (
    attention_path, attention_tiles)

QT, KT = attention_tiles()          # queries per block, keys per LDS tile of the MFMA path

CASES = [
    (1, 1, 1, 16, 16, None),
    (1, KT - 1, 1, 16, 16, None), (1, KT, 1, 16, 16, None), (1, KT + 1, 1, 16, 16, None),
    (1, QT - 1, 1, 32, 16, None), (1, QT, 3, 16, 16, None), (1, QT + 1, 1, 64, 64, None),
    (1, 197, 2, 64, 64, None),
    (2, KT + 1, 1, 16, 16, None), (3, QT + 6, 3, 32, 16, None), (2, KT + 5, 1, 128, 128, None),
    (2, 19, 3, 24, 24, None), (1, QT + 1, 1, 8, 40, None), (2, 19, 3, 6, 5, None),
    (1, 2 * KT + 6, 1, 16, 16, "ascending"), (1, 2 * KT + 6, 1, 16, 16, "descending"),
    (2, 2 * KT + 6, 2, 64, 64, "dominant"),
]
GUARD_CASES = [(2, KT + 1, 1, 16, 16, None), (1, 1, 1, 16, 16, None), (2, 19, 3, 6, 5, None), (1, 197, 2, 64, 64, None),
               (3, QT + 6, 3, 32, 16, None)]


def widths(c):
    """(qkv width, output width) of a case."""
    _, _, h, d, dv, _ = c
    return h * (2 * d + dv), h * dv


def split(qkv, B, T, h, d, dv):
    x = qkv.reshape(B, T, -1)
    q = x[..., :h * d].reshape(B, T, h, d)
    k = x[..., h * d:2 * h * d].reshape(B, T, h, d)
    v = x[..., 2 * h * d:2 * h * d + h * dv].reshape(B, T, h, dv)
    return q, k, v


def ref_attention(qkv, B, T, h, d, dv):
    """float64 oracle: softmax(Q K^T) V per (image, head) -> [B * T][h * dv]."""
    q, k, v = split(np.asarray(qkv, np.float64), B, T, h, d, dv)
    s = np.einsum("bqhd,bkhd->bhqk", q, k)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhqk,bkhd->bqhd", p, v).reshape(B * T, h * dv)


def library_f32(qkv, B, T, h, d, dv):
    """The library's fp32 path on the CPU: torch matmul, softmax, matmul."""
    q, k, v = (torch.from_numpy(np.ascontiguousarray(t)).permute(0, 2, 1, 3) for t in
               split(np.asarray(qkv, np.float32), B, T, h, d, dv))
    p = torch.softmax(torch.matmul(q, k.transpose(-1, -2)), dim=-1)
    return torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B * T, h * dv).numpy()


def f32_allowance(qkv, c, want):
    B, T, h, d, dv, _ = c
    e_ref = float(np.abs(library_f32(qkv, B, T, h, d, dv).astype(np.float64) - want).max())
    return e_ref, max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))


def _make(c):
    B, T, h, d, dv, probe = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    q = rng.standard_normal((B, T, h, d))
    k = rng.standard_normal((B, T, h, d))
    v = rng.standard_normal((B, T, h, dv))
    if probe in ("ascending", "descending"):
        # scores 100 * ramp(key) + N(0, 1): the maximum sits in the last (first) key tile of every row
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        ramp = np.arange(T) / max(T - 1, 1)
        ramp = ramp if probe == "ascending" else 1.0 - ramp
        k = ramp[None, :, None, None] * u + 0.1 * k
        q = 100.0 * u + q
    elif probe == "dominant":
        # unit keys; query r is 100 x the key at a random place: that score is 100, the others about N(0, 100 / sqrt(d))
        k /= np.linalg.norm(k, axis=-1, keepdims=True)
        where = rng.integers(0, T, (B, T, h))
        q = 100.0 * np.take_along_axis(k, where[..., None], axis=1)
    return np.concatenate([t.reshape(B * T, -1) for t in (q, k, v)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(c):
    B, T, h, d, dv, probe = c
    k = types.SimpleNamespace(case=c, B=B, T=T, heads=h, d=d, dv=dv, probe=probe, path=attention_path(d, dv))
    k.qkv = _make(c)
    k.want = ref_attention(k.qkv, B, T, h, d, dv)
    k.e_ref, k.allow = f32_allowance(k.qkv, c, k.want)
    return k


@functools.lru_cache(maxsize=None)
def case_bf16(c):
    """The case rounded to bf16 (oracle and allowance follow the rounded values) with the padded row strides of
    the bf16 layout: both widths rounded up to 8."""
    k = types.SimpleNamespace(**vars(case(c)))
    k.qkv = torch.from_numpy(k.qkv).to(torch.bfloat16).float().numpy()
    k.want = ref_attention(k.qkv, k.B, k.T, k.heads, k.d, k.dv)
    k.e_ref, k.allow = f32_allowance(k.qkv, c, k.want)
    w_in, w_out = widths(c)
    k.w_in, k.w_out, k.ld_in, k.ld_out = w_in, w_out, (w_in + 7) // 8 * 8, (w_out + 7) // 8 * 8
    return k


# ------------------------------------------------------------------ posembed
POSEMBED_CASES = [(2, 3, 3, 64, True), (2, 3, 3, 20, True), (1, 1, 5, 20, False), (3, 4, 4, 64, False)]   # B, H, W, C, ct


@functools.lru_cache(maxsize=None)
def posembed_case(c):
    B, H, W, C, ct = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    k = types.SimpleNamespace(case=c, B=B, T=H * W, C=C, ct=int(ct), Cp=(C + 7) // 8 * 8)
    k.x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    k.cls = rng.standard_normal(C).astype(np.float32) if ct else None
    k.pos = rng.standard_normal((k.T + k.ct, C)).astype(np.float32)
    return k


def ref_posembed(x, cls, pos):
    """numpy in the input's precision: out[:, 0] = cls + pos[0] (with a class token), out[:, ct + t] = x[:, t] +
    pos[ct + t]; one addition per element, so an fp32 kernel must match bit for bit."""
    B, C = x.shape[0], x.shape[-1]
    x = x.reshape(B, -1, C)
    ct = 0 if cls is None else 1
    out = np.empty((B, 1, x.shape[1] + ct, C), x.dtype)
    if ct:
        out[:, 0, 0] = cls + pos[0]
    out[:, 0, ct:] = x + pos[ct:]
    return out
