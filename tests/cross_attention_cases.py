"""Cases, inputs, layouts, the float64 oracle and the allowance shared by the cross-attention tests (native CPU op,
HIP kernels, guard band).

A case is ``(B, Tq, Tk, heads, key_dim, value_dim, layout, probe)``.  The kernel is handed three row pointers; the
layout says which buffers they point into (`views`):

* ``split``: three buffers, each with a row stride wider than its content and NaN in the surplus;
* ``q_kv``:  Q in its own buffer, [K | V] side by side in one (key = value source: `n#q` and `n#kv`);
* ``qk_v``:  [Q | K] side by side in one buffer (Tq = Tk; DETR's encoder: `n#qk` and `n#v`), V in its own.

The cases are the smallest at which csrc/kernels/cross_attention.hip can go wrong, with the tile sizes read from the
kernels module:

* Tk = 1; Tk one below, at and one above the key tile with Tq = 5; Tq = 1 over 2 KT + 6 keys (three of the block's
  four waves hold no query and must still reach every barrier); Tq one below, at and one above the query tile with
  Tk = 5; (Tq, Tk) = (100, 300) with two heads of 32 (DETR's decoder);
* B = 2 and 3 with both lengths off both tiles, once Tq > Tk and once Tq < Tk: a kernel that bases K rows on Tq (or Q
  rows on Tk) lands in a neighbour image's finite rows, so only a wrong value can show it;
* (d, dv) = (16, 16), (32, 16), (64, 64), (128, 128) for the MFMA path (all three register sizes, d != dv), (24, 24),
  (8, 40) and (6, 5) for the plain kernel (the last with widths that the bf16 layout pads);
* one MFMA-sized case whose K pointer is offset by 2 elements (probe ``k_off2``): misaligned for the 4-element
  vectors, it must take the plain kernel;
* the three softmax probes of tests/attention_cases.py with Tq != Tk, scores of magnitude about 100 over three key
  tiles: the row maximum in the last key tile (ascending), in the first (descending), one dominant key per row.

Inputs are N(0, 1), seeded per case.  The oracle is float64 numpy.  Allowance, the form of tests/attention_cases.py,
not a new number: ``max(4 e_ref, 2e-5 max(1, max|want|))``, where e_ref is the error against the oracle of the
library's fp32 path on the CPU (torch matmul, softmax, matmul on the same inputs).  Observed e_ref over the cases: 0
(Tk = 1, and the dominant-key probe, whose rows reproduce one V row) to 6.9e-6 (d = dv = 128; 6.8e-6 on the
ascending probe, 5.9e-6 at 100 x 300), so 4 e_ref, 2.8e-5 at most, stays below each case's own floor, 2e-5 x max(1, max|want|) =
2.0e-5 (Tq = 1, where e_ref is 1.3e-7) .. 7.9e-5 (3.8e-5 on the ascending probe): the floor decides every case
(printed per case by tests/test_cross_attention.py).

In bf16 the input is the case rounded to bf16, the oracle and the allowance follow the rounded values, and the bound
is ``2^-8 |want| + allowance`` (one rounding of the output).

Cached per case: callers must not modify what they get.
"""
import functools
import types
import zlib

import numpy as np
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.attention import (
    attention_path, cross_attention_tiles)

QT, KT = cross_attention_tiles()    # queries per block, keys per LDS tile of the MFMA path

CASES = [
    (1, 5, 1, 1, 16, 16, "split", None),
    (1, 5, KT - 1, 1, 16, 16, "q_kv", None), (1, 5, KT, 1, 16, 16, "split", None), (1, 5, KT + 1, 1, 16, 16, "q_kv", None),
    (1, 1, 2 * KT + 6, 1, 16, 16, "split", None),
    (1, QT - 1, 5, 1, 32, 16, "q_kv", None), (1, QT, 5, 3, 16, 16, "split", None), (1, QT + 1, 5, 1, 64, 64, "q_kv", None),
    (1, 100, 300, 2, 32, 32, "split", None),
    (2, QT + 6, KT + 5, 1, 16, 16, "q_kv", None), (3, 19, QT + KT + 5, 3, 32, 16, "split", None),
    (2, KT + 5, KT + 5, 1, 128, 128, "qk_v", None), (2, 37, 37, 2, 16, 16, "qk_v", None),
    (2, 19, 23, 3, 24, 24, "split", None), (1, QT + 1, 7, 1, 8, 40, "q_kv", None), (2, 19, 19, 3, 6, 5, "qk_v", None),
    (2, 7, 19, 3, 6, 5, "split", None),
    (1, 37, 45, 2, 32, 32, "split", "k_off2"),
    (1, KT + 1, 2 * KT + 6, 1, 16, 16, "split", "ascending"), (1, KT + 1, 2 * KT + 6, 1, 16, 16, "q_kv", "descending"),
    (2, KT + 1, 2 * KT + 6, 2, 64, 64, "split", "dominant"),
]
GUARD_CASES = [(1, 5, 1, 1, 16, 16, "split", None), (2, QT + 6, KT + 5, 1, 16, 16, "q_kv", None),
               (2, 37, 37, 2, 16, 16, "qk_v", None), (2, 19, 23, 3, 24, 24, "split", None),
               (2, 19, 19, 3, 6, 5, "qk_v", None)]


def expected_path(c):
    """What the launcher must choose: the MFMA path for its head sizes unless the K pointer is misaligned."""
    return "mfma" if attention_path(c[4], c[5]) == "mfma" and c[7] != "k_off2" else "plain"


def ref_attention(q, k, v):
    """float64 oracle: softmax(Q K^T) V per (image, head); q (B, Tq, h, d), k (B, Tk, h, d), v (B, Tk, h, dv) ->
    [B * Tq][h * dv]."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    s = np.einsum("bqhd,bkhd->bhqk", q, k)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhqk,bkhd->bqhd", p, v).reshape(q.shape[0] * q.shape[1], -1)


def library_f32(q, k, v):
    """The library's fp32 path on the CPU: torch matmul, softmax, matmul."""
    tq, tk, tv = (torch.from_numpy(np.ascontiguousarray(t, np.float32)).permute(0, 2, 1, 3) for t in (q, k, v))
    p = torch.softmax(torch.matmul(tq, tk.transpose(-1, -2)), dim=-1)
    return torch.matmul(p, tv).permute(0, 2, 1, 3).reshape(q.shape[0] * q.shape[1], -1).numpy()


def f32_allowance(q, k, v, want):
    e_ref = float(np.abs(library_f32(q, k, v).astype(np.float64) - want).max())
    return e_ref, max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))


def _make(c):
    B, Tq, Tk, h, d, dv, _, probe = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    q = rng.standard_normal((B, Tq, h, d))
    k = rng.standard_normal((B, Tk, h, d))
    v = rng.standard_normal((B, Tk, h, dv))
    if probe in ("ascending", "descending"):
        # scores 100 * ramp(key) + N(0, 1): the maximum sits in the last (first) key tile of every row
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        ramp = np.arange(Tk) / max(Tk - 1, 1)
        ramp = ramp if probe == "ascending" else 1.0 - ramp
        k = ramp[None, :, None, None] * u + 0.1 * k
        q = 100.0 * u + q
    elif probe == "dominant":
        # unit keys; query r is 100 x the key at a random place: that score is 100, the others about N(0, 100 / sqrt(d))
        k /= np.linalg.norm(k, axis=-1, keepdims=True)
        where = rng.integers(0, Tk, (B, Tq, h))
        q = 100.0 * np.take_along_axis(k, where[..., None], axis=1)
    return q.astype(np.float32), k.astype(np.float32), v.astype(np.float32)


def _finish(k):
    k.want = ref_attention(k.q, k.k, k.v)
    k.e_ref, k.allow = f32_allowance(k.q, k.k, k.v, k.want)
    k.w_out = k.heads * k.dv
    return k


@functools.lru_cache(maxsize=None)
def case(c):
    B, Tq, Tk, h, d, dv, layout, probe = c
    k = types.SimpleNamespace(case=c, B=B, Tq=Tq, Tk=Tk, heads=h, d=d, dv=dv, layout=layout, probe=probe,
                              path=expected_path(c))
    k.q, k.k, k.v = _make(c)
    return _finish(k)


@functools.lru_cache(maxsize=None)
def case_bf16(c):
    """The case rounded to bf16: the oracle and the allowance follow the rounded values."""
    k = types.SimpleNamespace(**vars(case(c)))
    k.q, k.k, k.v = (torch.from_numpy(t).to(torch.bfloat16).float().numpy() for t in (k.q, k.k, k.v))
    return _finish(k)


def _up8(n):
    return (n + 7) // 8 * 8


def views(k, make, fill=float("nan"), dtype=torch.float32):
    """(q, k, v, buffers) of a case in its layout.  `make(tensor, name)` turns a host tensor into the buffer the
    kernel reads (a device copy, a guarded device copy, or the tensor itself for the CPU op) and is called once per
    buffer; the views are column slices of what it returns.  `fill` is what the surplus of every row holds (never
    read).  A buffer's own row is wider than its content: by 8 more than the width rounded up to 8 where the head
    sizes suit the MFMA path (pointers and strides stay aligned), by 3 elsewhere (odd strides for the plain kernel).
    Probe `k_off2`: K's buffer starts 2 elements into its allocation."""
    rows = {"q": k.q.reshape(k.B * k.Tq, -1), "k": k.k.reshape(k.B * k.Tk, -1), "v": k.v.reshape(k.B * k.Tk, -1)}
    wide = (lambda w: _up8(w) + 8) if attention_path(k.d, k.dv) == "mfma" else (lambda w: w + 3)
    groups = {"split": ("q", "k", "v"), "q_kv": ("q", "kv"), "qk_v": ("qk", "v")}[k.layout]
    out, bufs = {}, []
    for grp in groups:
        parts = [rows[p] for p in grp]
        w = sum(p.shape[1] for p in parts)
        n = parts[0].shape[0]
        off = 2 if (k.probe == "k_off2" and grp == "k") else 0
        host = torch.full((off + n * wide(w),), fill, dtype=dtype)
        body = host[off:].view(n, wide(w))
        col = 0
        for p in parts:
            body[:, col:col + p.shape[1]] = torch.from_numpy(p).to(dtype)
            col += p.shape[1]
        dev = make(host, grp)
        bufs.append(dev)
        body = dev[off:].view(n, wide(w))
        col = 0
        for name, p in zip(grp, parts):
            out[name] = body[:, col:col + p.shape[1]]
            col += p.shape[1]
    return out["q"], out["k"], out["v"], bufs
