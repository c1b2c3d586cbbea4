"""Cases, inputs and the float64 oracle shared by the LayerNormalization tests (PyTorch oracle, native CPU op, HIP
kernels, guard band).

A case is ``(rows, C, eps, center, scale, mean, sigma)``.  They are the smallest shapes at which
csrc/kernels/layernorm.hip can go wrong: a single row; C % 4 != 0 (bf16 pads 6 -> 8); rows that are no multiple of
the rows per wave or of the waves per block with C % 8 == 4; the two catastrophic-cancellation probes (mean 100 /
sigma 0.1 at C 768, mean -50 / sigma 0.5 at the widest ConvNeXt C); several rows per wave with a ragged tail; a row
past the register path with an odd C; and the Keras flags center=False, scale=False and the default eps.

Inputs are N(mean, sigma), gamma uniform 0.5..1.5, beta N(0, 1), all seeded per case.  The oracle is written out in
float64 numpy and does not call `F.layer_norm`, so it is independent of ops/reference.py.  Cached per case: callers
must not modify what they get.
"""
import functools
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

CASES = [
    (1, 96, 1e-6, True, True, 0.0, 1.0),          # a single row
    (3, 6, 1e-6, True, True, 0.0, 1.0),           # C % 4 != 0; bf16 pads 6 -> 8
    (65, 100, 1e-6, True, True, 0.0, 1.0),        # rows % rows-per-wave, % waves-per-block != 0; C % 8 == 4
    (98, 768, 1e-6, True, True, 100.0, 0.1),      # 2x7x7 rows; catastrophic-cancellation probe
    (5, 2048, 1e-6, True, True, -50.0, 0.5),      # the widest ConvNeXt C
    (130, 40, 1e-6, True, True, 0.0, 1.0),        # several rows per wave with a ragged tail
    (3, 4099, 1e-6, True, True, 0.0, 1.0),        # past the register path, odd C
    (4, 192, 1e-6, False, True, 0.0, 1.0),        # center=False
    (4, 192, 1e-6, True, False, 0.0, 1.0),        # scale=False
    (2, 24, 1e-3, True, True, 0.0, 1.0),          # Keras' default eps
]
GUARD_CASES = [CASES[i] for i in (1, 2, 5, 6)]


def ref_layernorm(x, gamma, beta, eps):
    """float64 oracle over the last axis; gamma / beta None stand for Keras' scale=False / center=False."""
    x = np.asarray(x, np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    y = (x - mu) / np.sqrt(var + eps)
    if gamma is not None:
        y = y * np.asarray(gamma, np.float64)
    if beta is not None:
        y = y + np.asarray(beta, np.float64)
    return y


@functools.lru_cache(maxsize=None)
def case(c):
    rows, C, eps, center, scale, mean, sigma = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    k = types.SimpleNamespace(case=c, rows=rows, C=C, eps=eps, center=center, scale=scale)
    k.x = (mean + sigma * rng.standard_normal((rows, C))).astype(np.float32)
    k.gamma = rng.uniform(0.5, 1.5, C).astype(np.float32) if scale else None
    k.beta = rng.standard_normal(C).astype(np.float32) if center else None
    # what a kernel is handed: Keras' defaults where the layer has no weight
    k.gamma_k = k.gamma if scale else np.ones(C, np.float32)
    k.beta_k = k.beta if center else np.zeros(C, np.float32)
    k.want = ref_layernorm(k.x, k.gamma, k.beta, eps)
    k.allow = f32_allowance(k.x, k.gamma, k.beta, eps, k.want)
    return k


def f32_allowance(x, gamma, beta, eps, want):
    """max(4 e_ref, 2e-5 max(1, max|want|)): e_ref is the error of the library's fp32 `F.layer_norm` on the CPU
    against the float64 oracle (the reference's own error, not the code under test's); 4x covers a different but
    equally valid summation order; the floor is the project's fp32 bound (tests/test_fp32_gpu.py)."""
    t = F.layer_norm(torch.from_numpy(np.asarray(x, np.float32)), (x.shape[-1],),
                     None if gamma is None else torch.from_numpy(gamma),
                     None if beta is None else torch.from_numpy(beta), eps)
    e_ref = float(np.abs(t.numpy().astype(np.float64) - want).max())
    return max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))


@functools.lru_cache(maxsize=None)
def case_bf16(c):
    """The case with its input rounded to bf16 (the oracle and the fp32 allowance follow the rounded values),
    laid out as the bf16 kernels see it: Cp = C padded to 8, gamma / beta zero-padded to Cp."""
    k0 = case(c)
    k = types.SimpleNamespace(**vars(k0))
    k.x = torch.from_numpy(k0.x).to(torch.bfloat16).float().numpy()
    k.want = ref_layernorm(k.x, k.gamma, k.beta, k.eps)
    k.allow = f32_allowance(k.x, k.gamma, k.beta, k.eps, k.want)
    k.Cp = (k.C + 7) // 8 * 8
    k.gamma_p, k.beta_p = np.zeros(k.Cp, np.float32), np.zeros(k.Cp, np.float32)
    k.gamma_p[:k.C], k.beta_p[:k.C] = k.gamma_k, k.beta_k
    return k
