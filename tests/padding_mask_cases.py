"""What the padding-mask tests share: shapes, mask patterns, the float64 oracles written two ways, the allowance,
and DistilBERT by hand in float64.

A case is ``(head size, tokens)``: B = 3 images (a different pattern per image), 2 heads, d = dv.  The inputs are
those of tests/attention_cases.py for ``(3, T, 2, d, d, None)`` (imported, not copied): N(0, 1), seeded per case.

Head sizes 16, 32, 64, 128 take the MFMA path (all three register sizes), 24 the plain kernel.  Token counts 1, 31,
32, 33, 64, 65, 97, 130: one below, at and one above the 32-key tile and the 64-query tile, and three query tiles.

A mask row holds token ids as float32; token j is padding iff -1 < mask[j] < 1.  The nine patterns, three launches
of three images each (`GROUPS`):

* ``all``: every token kept;
* ``right1``, ``right32``, ``right33``, ``rightT-1``: right padding to that many kept tokens (clamped to T);
* ``left33``: the first 33 tokens padded, so the leading key tile is wholly masked (T <= 33: nothing kept);
* ``hole``: tokens 32 .. 63 padded, one whole interior tile (T <= 32: no hole);
* ``alternate``: every other token padded, and the values walk the edges of the test: padded ones are 0, 0.5,
  -0.99 and -0.0, kept ones 1, -1, 5 and NaN (a NaN is kept, as `NaN != 0` is in Keras);
* ``none``: nothing kept.

Two oracles in float64 numpy.  `ref_masked` is the project's semantics: a padded key has the score -inf, a padded
query's row and every row of an image with no kept key are zeros.  `ref_keras` is Keras': -1e9 added to the scores
under the AND of the query's and the key's mask, softmax over all keys.  At a kept query with a kept key the two
agree (exp(-1e9 - max) is 0); that is what the tests compare, at kept rows only.

Allowance, the project's form (tests/attention_cases.py): ``max(4 e_ref, 2e-5 max(1, max|want|))``, e_ref being the
error against `ref_masked` of torch's fp32 CPU path (matmul, masked_fill(-inf), softmax, matmul) at the kept rows:
the reference's own error, never the code under test's.  bf16: the inputs rounded to bf16, oracle and allowance from
the rounded values, bound ``2^-8 |want| + allowance``.

Cached per case: callers must not modify what they get.
"""
import functools
import types

import numpy as np
import torch

import attention_cases as AC

QT, KT = AC.QT, AC.KT
B, HEADS = 3, 2
HEAD_SIZES = (16, 32, 64, 128, 24)
TOKENS = (1, KT - 1, KT, KT + 1, QT, QT + 1, 97, 130)
CASES = [(d, t) for d in HEAD_SIZES for t in TOKENS]
GUARD_CASES = [(d, t) for d in HEAD_SIZES for t in (1, KT + 1, QT + 1)]
GROUPS = (("all", "right1", "left33"), ("right32", "hole", "none"), ("right33", "rightT-1", "alternate"))
RIGHT = {"all": None, "right1": 1, "right32": 32, "right33": 33, "rightT-1": -1}       # kept length, None: T


def attn_case(c):
    d, t = c
    return (B, t, HEADS, d, d, None)


def kept(mask):
    """The test the kernels, the CPU op and the reference apply: padding iff -1 < x < 1; a NaN is kept."""
    m = np.asarray(mask)
    with np.errstate(invalid="ignore"):
        return ~((m > -1) & (m < 1))


def pattern(name, T, seed=0):
    """(T,) float32 mask row of a pattern: ids in [1, 97) where kept, 0 where padded (but see ``alternate``)."""
    ids = np.random.default_rng(seed + T).integers(1, 97, T).astype(np.float32)
    keep = np.ones(T, bool)
    if name in RIGHT:
        n = RIGHT[name]
        n = T if n is None else (max(T - 1, 0) if n < 0 else min(n, T))
        keep[n:] = False
    elif name == "left33":
        keep[:33] = False
    elif name == "hole":
        keep[KT:2 * KT] = False
    elif name == "none":
        keep[:] = False
    elif name == "alternate":
        pad_vals = np.array([0.0, 0.5, -0.99, -0.0], np.float32)
        keep_vals = np.array([1.0, -1.0, 5.0, np.nan], np.float32)
        j = np.arange(T)
        row = np.where(j % 2 == 0, keep_vals[(j // 2) % 4], pad_vals[(j // 2) % 4]).astype(np.float32)
        assert (kept(row) == (j % 2 == 0)).all()
        return row
    else:
        raise KeyError(name)
    return np.where(keep, ids, np.float32(0.0)).astype(np.float32)


def masks(group, T):
    """(B, T) float32: one pattern per image."""
    return np.stack([pattern(n, T, seed=i) for i, n in enumerate(group)])


def ref_masked(qkv, mask, Bn, T, h, d, dv):
    """float64 oracle, the project's semantics -> [B * T][h * dv]."""
    q, k, v = AC.split(np.asarray(qkv, np.float64), Bn, T, h, d, dv)
    keep = kept(mask).reshape(Bn, T)
    s = np.einsum("bqhd,bkhd->bhqk", q, k)
    s = np.where(keep[:, None, None, :], s, -np.inf)
    with np.errstate(invalid="ignore"):
        p = np.exp(s - s.max(-1, keepdims=True))
        p = p / p.sum(-1, keepdims=True)
    p = np.where(np.isfinite(p), p, 0.0)
    out = np.einsum("bhqk,bkhd->bqhd", p, v)
    out = out * (keep & keep.any(-1, keepdims=True))[:, :, None, None]
    return out.reshape(Bn * T, h * dv)


def ref_keras(qkv, mask, Bn, T, h, d, dv):
    """float64 oracle, Keras' semantics: -1e9 added under the AND of the query's and the key's mask."""
    q, k, v = AC.split(np.asarray(qkv, np.float64), Bn, T, h, d, dv)
    keep = kept(mask).reshape(Bn, T)
    both = keep[:, None, :, None] & keep[:, None, None, :]
    s = np.einsum("bqhd,bkhd->bhqk", q, k) + np.where(both, 0.0, -1e9)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhqk,bkhd->bqhd", p, v).reshape(Bn * T, h * dv)


def library_f32(qkv, mask, Bn, T, h, d, dv):
    """torch's fp32 CPU path: matmul, masked_fill(-inf), softmax, matmul (rows with no kept key come out NaN)."""
    q, k, v = (torch.from_numpy(np.ascontiguousarray(t)).permute(0, 2, 1, 3) for t in
               AC.split(np.asarray(qkv, np.float32), Bn, T, h, d, dv))
    keep = torch.from_numpy(kept(mask).reshape(Bn, T))
    s = torch.matmul(q, k.transpose(-1, -2)).masked_fill(~keep[:, None, None, :], float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v).permute(0, 2, 1, 3).reshape(Bn * T, h * dv).numpy()


def kept_rows(mask):
    """(B * T,) bool: the rows that hold a kept query."""
    return kept(mask).reshape(-1)


def _build(k, group):
    m = masks(group, k.T)
    want = ref_masked(k.qkv, m, k.B, k.T, k.heads, k.d, k.dv)
    rows = kept_rows(m)
    e_ref = 0.0
    if rows.any():
        lib = library_f32(k.qkv, m, k.B, k.T, k.heads, k.d, k.dv).astype(np.float64)
        e_ref = float(np.abs(lib[rows] - want[rows]).max())
    allow = max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))
    return types.SimpleNamespace(group=group, mask=m, want=want, rows=rows, e_ref=e_ref, allow=allow)


@functools.lru_cache(maxsize=None)
def case(c):
    """The fp32 case: AC's inputs plus, per group of patterns, the masks, the oracle and the allowance."""
    k = types.SimpleNamespace(**vars(AC.case(attn_case(c))))
    k.w_in, k.w_out = AC.widths(attn_case(c))
    k.groups = [_build(k, g) for g in GROUPS]
    return k


@functools.lru_cache(maxsize=None)
def case_bf16(c):
    k = types.SimpleNamespace(**vars(AC.case_bf16(attn_case(c))))
    k.groups = [_build(k, g) for g in GROUPS]
    return k


# ------------------------------------------------------------------ DistilBERT by hand
EPS = 1e-12


def _ln(x, w, name):
    mu = x.mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(((x - mu) ** 2).mean(-1, keepdims=True) + EPS) * w[f"{name}/gamma"] + w[f"{name}/beta"]


def _gelu(x):
    from math import erf
    return 0.5 * x * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))


def forward(name, depth, w, ids, keras=False):
    """float64 last hidden state (B, T, C) of `build_distilbert(name)` with weights `w` on `ids` (B, T), written
    out in numpy from the weights' Keras names, independent of the IR, the plan and every executor.  `keras`:
    Keras' masking (-1e9 under the AND of the query's and the key's mask) instead of the project's (a padded key
    -inf, a padded query's context row zeros); the two agree at kept positions."""
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    keep = kept(ids)
    idx = np.asarray(ids).astype(np.int64)
    x = w[f"{name}_word_embeddings/embeddings"][idx] + w[f"{name}_position_embeddings/position_embedding"]
    x = _ln(x, w, f"{name}_embeddings_ln")
    for i in range(depth):
        b = f"{name}_layer_{i}"
        a = f"{b}_attention"
        d = w[f"{a}/query/kernel"].shape[-1]
        q = (np.einsum("btc,chd->bthd", x, w[f"{a}/query/kernel"]) + w[f"{a}/query/bias"]) / np.sqrt(float(d))
        k = np.einsum("btc,chd->bthd", x, w[f"{a}/key/kernel"]) + w[f"{a}/key/bias"]
        v = np.einsum("btc,chd->bthd", x, w[f"{a}/value/kernel"]) + w[f"{a}/value/bias"]
        s = np.einsum("bqhd,bkhd->bhqk", q, k)
        if keras:
            s = s + np.where(keep[:, None, :, None] & keep[:, None, None, :], 0.0, -1e9)
        else:
            s = np.where(keep[:, None, None, :], s, -np.inf)
        with np.errstate(invalid="ignore"):
            p = np.exp(s - s.max(-1, keepdims=True))
            p = p / p.sum(-1, keepdims=True)
        p = np.where(np.isfinite(p), p, 0.0)
        o = np.einsum("bhqk,bkhd->bqhd", p, v)
        if not keras:
            o = o * (keep & keep.any(-1, keepdims=True))[:, :, None, None]
        y = np.einsum("bqhd,hdc->bqc", o, w[f"{a}/attention_output/kernel"]) + w[f"{a}/attention_output/bias"]
        x = _ln(x + y, w, f"{b}_sa_layer_norm")
        y = _gelu(x @ w[f"{b}_ffn_lin1/kernel"] + w[f"{b}_ffn_lin1/bias"])
        x = _ln(x + y @ w[f"{b}_ffn_lin2/kernel"] + w[f"{b}_ffn_lin2/bias"], w, f"{b}_output_layer_norm")
    return x


@functools.lru_cache(maxsize=None)
def micro():
    """(graph, weights, ids (4, T) float32, float64 hidden states) of distilbert_micro.  The four samples: right
    padding to 33 and to 7 kept tokens, no padding, left padding of 33 (a wholly masked leading key tile).  Cached:
    callers must not modify what they get."""
    from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import (
        init_weights)
    from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
        DISTILBERT, build_distilbert)
    import gpt_cases as GC
    g = build_distilbert("distilbert_micro")
    w = GC.noisy(init_weights(g, seed=0))
    T = g.layers[g.input].out_shape[0]
    ids = np.random.default_rng(5).integers(1, 97, (4, T)).astype(np.float32)
    ids[0, 33:] = 0
    ids[1, 7:] = 0
    ids[3, :33] = 0
    return g, w, ids, forward("distilbert_micro", DISTILBERT["distilbert_micro"][0], w, ids)
