"""Causal cases for the attention tests: the cases and inputs of tests/attention_cases.py (imported, not copied)
under Keras' causal mask, query i attends keys j <= i, with a causal float64 oracle and a causal library reference.

Same `CASES` and `GUARD_CASES`, same inputs (`AC.case(c).qkv`).  The cases already sit at T = 1, at the key tile and
the query tile and one to either side of each, at two and three images, on all three register sizes, at d != dv and
on the plain kernel's head sizes; under the mask T = 197 walks every kind of tile: wholly below the diagonal,
straddling it, and above it (skipped).

Allowance, the project's form: ``max(4 e_ref, 2e-5 max(1, max|want|))``.  e_ref is the error against the oracle of
torch's fp32 CPU path on the same inputs (matmul, `masked_fill(-inf)`, softmax, matmul): the reference's own error,
not the code under test's.  Over the 17 cases e_ref is 0 to 9.0e-6 in fp32 and up to 5.6e-6 on the bf16-rounded
inputs; 4 e_ref stays below the floor (3.6e-5 .. 8.4e-5) in every case, so the floor decides, as it does without the
mask.  bf16: the input is the case rounded to bf16, oracle and allowance follow the rounded values, and the bound is
``2^-8 |want| + allowance`` (one rounding of the output).

The probes.  `ascending` puts every row's largest score (about 100) in the last key tile and `dominant` puts it at a
random key, which for most rows is a future one.  A kernel that takes the maximum over all keys and masks the
probabilities afterwards underflows every visible term of such a row (exp(-100 ...) / 0): NaN, which
`late_masking` reproduces on the CPU and tests/test_causal_attention.py asserts.

Cached per case: callers must not modify what they get.
"""
import functools
import types

import numpy as np
import torch

import attention_cases as AC

QT, KT = AC.QT, AC.KT
CASES = AC.CASES
GUARD_CASES = AC.GUARD_CASES
widths = AC.widths


def ref_attention(qkv, B, T, h, d, dv):
    """float64 oracle: softmax over the keys j <= i of (Q K^T) V per (image, head) -> [B * T][h * dv]."""
    q, k, v = AC.split(np.asarray(qkv, np.float64), B, T, h, d, dv)
    s = np.einsum("bqhd,bkhd->bhqk", q, k)
    s = np.where(np.tri(T, dtype=bool), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhqk,bkhd->bqhd", p, v).reshape(B * T, h * dv)


def library_f32(qkv, B, T, h, d, dv):
    """The library's fp32 path on the CPU: torch matmul, masked_fill(-inf), softmax, matmul."""
    q, k, v = (torch.from_numpy(np.ascontiguousarray(t)).permute(0, 2, 1, 3) for t in
               AC.split(np.asarray(qkv, np.float32), B, T, h, d, dv))
    s = torch.matmul(q, k.transpose(-1, -2))
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v).permute(0, 2, 1, 3).reshape(B * T, h * dv).numpy()


def late_masking(qkv, B, T, h, d, dv):
    """What a wrong kernel computes in fp32: the row maximum over all keys, the mask on the probabilities."""
    q, k, v = AC.split(np.asarray(qkv, np.float32), B, T, h, d, dv)
    s = np.einsum("bqhd,bkhd->bhqk", q, k, dtype=np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.exp(s - s.max(-1, keepdims=True)) * np.tri(T, dtype=np.float32)
        p = p / p.sum(-1, keepdims=True)
        return np.einsum("bhqk,bkhd->bqhd", p, v).reshape(B * T, h * dv)


def f32_allowance(qkv, c, want):
    B, T, h, d, dv, _ = c
    e_ref = float(np.abs(library_f32(qkv, B, T, h, d, dv).astype(np.float64) - want).max())
    return e_ref, max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))


@functools.lru_cache(maxsize=None)
def case(c):
    k = types.SimpleNamespace(**vars(AC.case(c)))           # the same inputs; the array is shared, not copied
    k.want = ref_attention(k.qkv, k.B, k.T, k.heads, k.d, k.dv)
    k.e_ref, k.allow = f32_allowance(k.qkv, c, k.want)
    return k


@functools.lru_cache(maxsize=None)
def case_bf16(c):
    """The case rounded to bf16 with the padded row strides of the bf16 layout (`AC.case_bf16`), causal oracle."""
    k = types.SimpleNamespace(**vars(AC.case_bf16(c)))
    k.want = ref_attention(k.qkv, k.B, k.T, k.heads, k.d, k.dv)
    k.e_ref, k.allow = f32_allowance(k.qkv, c, k.want)
    return k
