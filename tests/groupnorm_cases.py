"""Cases, inputs and the float64 oracle shared by the GroupNormalization tests (PyTorch oracle, native CPU op, HIP
kernels, guard band).

A case is ``(B, H, W, C, groups, mean, sigma, eps, center, scale, act)``; groups -1 is Keras' instance norm and act
a Keras activation name folded into the step (None: none).  They are the smallest shapes at which
csrc/kernels/groupnorm.hip can go wrong: one pixel; C % 4 != 0 with two channels per group (the fp32 scalar path;
bf16 pads 6 -> 8); four channels per group with C % 8 == 4 (a bf16 vector straddles two groups and ends in
padding); instance norm; one group; the two catastrophic-cancellation probes (mean 100 / sigma 0.1, and mean -50 /
sigma 0.5 over many pixels and few channels, which is also the smallest case with several slabs); an odd pixel
count with two channels per group and 32 groups (an fp32 vector straddles two groups, a bf16 vector four) on the
split path; batch 3; the Keras flags center=False, scale=False and eps 1e-3; a folded swish; and a case wider than
the vector path (more than 256 16-byte vectors per pixel), the only way to the scalar path in bf16.

Inputs are N(mean, sigma) plus a per-group offset of about 3 sigma, so the groups differ; gamma uniform 0.5..1.5,
beta N(0, 1), all seeded per case.  The oracle is written out in float64 numpy and does not call `F.group_norm`, so
it is independent of ops/reference.py.  Cached per case: callers must not modify what they get.
"""
import functools
import types
import zlib

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
CASES = [
    (1, 1, 1, 8, 2, 0.0, 1.0, EPS, True, True, None),             # one pixel
    (2, 3, 5, 6, 3, 0.0, 1.0, EPS, True, True, None),             # C % 4 != 0, Cg 2; bf16 pads 6 -> 8
    (2, 7, 9, 20, 5, 0.0, 1.0, EPS, True, True, None),            # Cg 4, C % 8 == 4
    (1, 5, 5, 12, -1, 0.0, 1.0, EPS, True, True, None),           # instance norm
    (2, 4, 4, 16, 1, 0.0, 1.0, EPS, True, True, None),            # one group
    (2, 16, 16, 32, 8, 100.0, 0.1, EPS, True, True, None),        # catastrophic-cancellation probe
    (1, 96, 96, 8, 2, -50.0, 0.5, EPS, True, True, None),         # probe with many pixels, few channels; several slabs
    (1, 33, 31, 64, 32, 0.0, 1.0, EPS, True, True, None),         # odd pixel count, Cg 2, G 32; the split path
    (3, 8, 8, 40, 10, 0.0, 1.0, EPS, True, True, None),           # batch 3
    (2, 7, 9, 20, 5, 0.0, 1.0, EPS, False, True, None),           # center=False
    (2, 7, 9, 20, 5, 0.0, 1.0, EPS, True, False, None),           # scale=False
    (3, 8, 8, 40, 10, 0.0, 1.0, 1e-3, True, True, None),          # Keras' default eps
    (1, 33, 31, 64, 32, 0.0, 1.0, EPS, True, True, "swish"),      # swish folded, split path
    (2, 3, 5, 6, 3, 0.0, 1.0, EPS, True, True, "swish"),          # swish folded, scalar (fp32) / single launch (bf16)
    (1, 2, 3, 2056, 8, 0.0, 1.0, EPS, True, True, None),          # 514 fp32 / 257 bf16 vectors per pixel: scalar path
]
# C % 4 != 0; the vector that straddles groups (C % 8 == 4); the odd pixel count on the split path; several slabs
GUARD_CASES = [CASES[i] for i in (1, 2, 7, 6)]


def ref_groupnorm(x, gamma, beta, groups, eps, act=None):
    """float64 oracle on NHWC x; gamma / beta None stand for Keras' scale=False / center=False."""
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    G = C if groups == -1 else groups
    xg = x.reshape(B, H * W, G, C // G)
    mu = xg.mean(axis=(1, 3), keepdims=True)
    var = ((xg - mu) ** 2).mean(axis=(1, 3), keepdims=True)
    y = ((xg - mu) / np.sqrt(var + eps)).reshape(x.shape)
    if gamma is not None:
        y = y * np.asarray(gamma, np.float64)
    if beta is not None:
        y = y + np.asarray(beta, np.float64)
    if act == "swish":
        y = y / (1.0 + np.exp(-y))
    elif act is not None:
        raise ValueError(act)
    return y


def f32_allowance(x, gamma, beta, groups, eps, act, want):
    """max(4 e_ref, 2e-5 max(1, max|want|)): e_ref is the error of the library's fp32 `F.group_norm` (+ `F.silu`)
    on the CPU against the float64 oracle (the reference's own error, not the code under test's); 4x covers a
    different but equally valid summation order; the floor is the project's fp32 bound (tests/test_fp32_gpu.py)."""
    C = x.shape[-1]
    t = F.group_norm(torch.from_numpy(np.asarray(x, np.float32)).permute(0, 3, 1, 2).contiguous(),
                     C if groups == -1 else groups,
                     None if gamma is None else torch.from_numpy(gamma),
                     None if beta is None else torch.from_numpy(beta), eps)
    if act == "swish":
        t = F.silu(t)
    e_ref = float(np.abs(t.permute(0, 2, 3, 1).numpy().astype(np.float64) - want).max())
    return max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))


@functools.lru_cache(maxsize=None)
def case(c):
    B, H, W, C, groups, mean, sigma, eps, center, scale, act = c
    rng = np.random.default_rng(zlib.crc32(repr(c).encode()))
    G = C if groups == -1 else groups
    k = types.SimpleNamespace(case=c, B=B, H=H, W=W, C=C, groups=groups, G=G, eps=eps, center=center, scale=scale,
                              act=act, act_mode={None: 0, "swish": 3}[act])
    offs = np.repeat(3.0 * sigma * rng.standard_normal(G), C // G)                 # per group, about 3 sigma
    k.x = (mean + offs + sigma * rng.standard_normal((B, H, W, C))).astype(np.float32)
    k.gamma = rng.uniform(0.5, 1.5, C).astype(np.float32) if scale else None
    k.beta = rng.standard_normal(C).astype(np.float32) if center else None
    # what a kernel is handed: Keras' defaults where the layer has no weight
    k.gamma_k = k.gamma if scale else np.ones(C, np.float32)
    k.beta_k = k.beta if center else np.zeros(C, np.float32)
    k.want = ref_groupnorm(k.x, k.gamma, k.beta, groups, eps, act)
    k.allow = f32_allowance(k.x, k.gamma, k.beta, groups, eps, act, k.want)
    return k


@functools.lru_cache(maxsize=None)
def case_bf16(c):
    """The case with its input rounded to bf16 (the oracle and the fp32 allowance follow the rounded values),
    laid out as the bf16 kernels see it: Cp = C padded to 8, gamma / beta zero-padded to Cp."""
    k0 = case(c)
    k = types.SimpleNamespace(**vars(k0))
    k.x = torch.from_numpy(k0.x).to(torch.bfloat16).float().numpy()
    k.want = ref_groupnorm(k.x, k.gamma, k.beta, k.groups, k.eps, k.act)
    k.allow = f32_allowance(k.x, k.gamma, k.beta, k.groups, k.eps, k.act, k.want)
    k.Cp = (k.C + 7) // 8 * 8
    k.gamma_p, k.beta_p = np.zeros(k.Cp, np.float32), np.zeros(k.Cp, np.float32)
    k.gamma_p[:k.C], k.beta_p[:k.C] = k.gamma_k, k.beta_k
    return k


def one_pass_f32(x, gamma, beta, groups, eps):
    """The form the kernels must not take, for the record: fp32 E[x^2] - mu^2 with sequential fp32 sums."""
    x = np.asarray(x, np.float32)
    B, H, W, C = x.shape
    G = C if groups == -1 else groups
    xg = x.reshape(B, H * W, G, C // G)
    n = np.float32(H * W * (C // G))
    s1 = np.zeros((B, 1, G, 1), np.float32)
    s2 = np.zeros((B, 1, G, 1), np.float32)
    for p in range(H * W):
        for j in range(C // G):
            v = xg[:, p:p + 1, :, j:j + 1]
            s1 += v
            s2 += v * v
    mu = s1 / n
    var = np.maximum(s2 / n - mu * mu, np.float32(0))
    y = ((xg - mu) / np.sqrt(var + np.float32(eps))).reshape(x.shape)
    return y * (1 if gamma is None else gamma) + (0 if beta is None else beta)
