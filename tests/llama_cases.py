"""What the Llama tests share: the kernel cases of rmsnorm, rope and the grouped-query attention core with their
float64 numpy oracles written out by hand, the allowance in the project's form, and the model by hand in float64.

`forward` is a Llama written out in numpy from the weights' Keras names, independent of the IR, the plan and every
executor: token table lookup, pre-norm blocks (RMS normalisation, rotary embedding in the rotate-half convention on
Q and K, causal grouped-query attention, Add, RMS normalisation, the SwiGLU MLP, Add), the last token (or every
token), the final RMS normalisation and the head without bias.

The allowance of a kernel case: fp32 `max(4 e_ref, 2e-5 max(1, max|want|))` with e_ref the error of the library's
fp32 evaluation on the CPU against the float64 oracle (never the code under test's); bf16 adds `2^-8 |want|`
elementwise (half a bf16 ulp is 2^-9 relative; the kernels round once, on the store) with the inputs rounded to
bf16 before the oracle sees them.
"""
import functools
import zlib

import numpy as np
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    LLAMA, build_llama)


def seed_of(case) -> int:
    return zlib.crc32(repr(case).encode())


def bf16_round(x: np.ndarray) -> np.ndarray:
    """float32 values rounded to bf16 (nearest even), as float32."""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def allowance(want: np.ndarray, e_ref: float, bf16: bool = False) -> np.ndarray:
    """The elementwise bound on |got - want| (module docstring)."""
    a = max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))
    return a + (np.abs(want) * 2.0 ** -8 if bf16 else 0.0)


# --------------------------------------------------------------------- rmsnorm
# (rows, C, eps, scale, probe): one lane group of every width (8, 16, 32, 64 lanes), C % 4 != 0 and C > 2048 on
# the looped path, rows that are no multiple of the rows per block, the largest register row (2048 fp32 = 512
# vectors), and mean 100 / sigma 0.1, where the mean square is 1e4 and a careless sum loses the digits
RMSNORM_CASES = [
    (1, 96, 1e-6, True, "normal"),
    (3, 6, 1e-6, True, "normal"),
    (65, 100, 1e-5, True, "normal"),
    (130, 40, 1e-6, False, "normal"),
    (3, 4099, 1e-5, True, "normal"),
    (5, 2048, 1e-6, True, "normal"),
    (98, 768, 1e-5, True, "offset"),
    (7, 520, 1e-6, False, "normal"),
]


def rmsnorm_inputs(case, bf16=False):
    rows, C, eps, scale, probe = case
    rng = np.random.default_rng(seed_of(case))
    x = rng.standard_normal((rows, C)) * (0.1 if probe == "offset" else 1.0) + (100.0 if probe == "offset" else 0.0)
    x = x.astype(np.float32)
    if bf16:
        x = bf16_round(x)
    sc = rng.uniform(0.5, 1.5, C).astype(np.float32) if scale else None
    return x, sc


def rmsnorm_oracle(x, sc, eps):
    x = np.asarray(x, np.float64)
    y = x / np.sqrt((x * x).mean(-1, keepdims=True) + np.float64(eps))
    return y if sc is None else y * np.asarray(sc, np.float64)


def rmsnorm_library(x, sc, eps):
    """The library's fp32 evaluation on the CPU, for e_ref."""
    import torch.nn.functional as F
    return F.rms_norm(torch.from_numpy(x), (x.shape[-1],), None if sc is None else torch.from_numpy(sc),
                      float(eps)).numpy()


# ------------------------------------------------------------------------ rope
# (B, T, hq, hkv, d, dv, W): d = 2 and 6 on the scalar path, d = 8 one fp32 vector (scalar in bf16), d = 16, 64,
# 128 on the vector path, dv != d once, T = 1 (position 0: the identity), B = 2 and 3 at T = 33 (row T of the
# buffer is position 0 of image 1), hq != hkv, both wavelengths
ROPE_CASES = [
    (1, 1, 2, 2, 8, 8, 10000.0),
    (1, 5, 3, 1, 2, 2, 10000.0),
    (2, 33, 4, 2, 6, 6, 10000.0),
    (2, 33, 4, 2, 8, 8, 500000.0),
    (3, 33, 4, 2, 16, 16, 10000.0),
    (2, 33, 2, 1, 64, 64, 500000.0),
    (1, 40, 2, 2, 128, 128, 10000.0),
    (2, 7, 6, 2, 16, 24, 10000.0),
    (1, 130, 4, 1, 32, 5, 10000.0),
]


def rope_width(case):
    B, T, hq, hkv, d, dv, W = case
    return (hq + hkv) * d + hkv * dv


def rope_inputs(case, bf16=False):
    B, T = case[:2]
    x = np.random.default_rng(seed_of(case)).standard_normal((B * T, rope_width(case))).astype(np.float32)
    return bf16_round(x) if bf16 else x


def rope_angles(T, d, W):
    """theta(t, i) = t W^(-2i/d) in float64, [T][d/2]."""
    i = np.arange(d // 2, dtype=np.float64)
    return np.arange(T, dtype=np.float64)[:, None] * np.float64(W) ** (-2.0 * i / d)[None, :]


def rope_oracle(x, case, table=None):
    """The rotate-half rotation in float64 on rows of [Q | K | V]; `table` ([2][T][d/2], what the kernels read)
    or the float64 angles themselves."""
    B, T, hq, hkv, d, dv, W = case
    x = np.asarray(x, np.float64)
    if table is None:
        th = rope_angles(T, d, W)
        cs, sn = np.cos(th), np.sin(th)
    else:
        cs, sn = np.asarray(table[0], np.float64), np.asarray(table[1], np.float64)
    y = x.copy()
    t = np.arange(B * T) % T
    for h in range(hq + hkv):
        a, b = x[:, h * d:h * d + d // 2], x[:, h * d + d // 2:(h + 1) * d]
        y[:, h * d:h * d + d // 2] = a * cs[t] - b * sn[t]
        y[:, h * d + d // 2:(h + 1) * d] = b * cs[t] + a * sn[t]
    return y


def rope_library(x, case, table):
    """The same formulas in torch fp32 on the fp32 table, for e_ref."""
    B, T, hq, hkv, d, dv, W = case
    xt = torch.from_numpy(x)
    tb = torch.as_tensor(table, dtype=torch.float32)
    t = torch.arange(B * T) % T
    cs, sn = tb[0][t], tb[1][t]
    y = xt.clone()
    for h in range(hq + hkv):
        a, b = xt[:, h * d:h * d + d // 2], xt[:, h * d + d // 2:(h + 1) * d]
        y[:, h * d:h * d + d // 2] = a * cs - b * sn
        y[:, h * d + d // 2:(h + 1) * d] = b * cs + a * sn
    return y.numpy()


# ------------------------------------------------------------------- GQA core
def gqa_cases(QT, KT):
    """(B, T, hq, hkv, d, dv, probe) for query tile QT and key tile KT of the MFMA path: T at the tile edges and
    at 197, every (hq, hkv) pair, B = 2 and 3, head sizes of the MFMA path at each DMAX (16 and 32 -> 32, 64, 128)
    and of the plain path ((24, 24): not multiples of 16; (6, 5): odd), both softmax probes."""
    return [
        (2, KT - 1, 4, 1, 16, 16, "ascending"),
        (3, KT, 6, 2, 32, 16, "dominant"),
        (2, KT + 1, 4, 2, 64, 64, "ascending"),
        (2, QT - 1, 3, 3, 16, 16, "dominant"),
        (3, QT + 1, 4, 2, 16, 16, "ascending"),
        (2, 197, 6, 2, 64, 64, "dominant"),
        (2, KT + 1, 4, 1, 128, 128, "ascending"),
        (2, QT + 1, 6, 2, 24, 24, "dominant"),
        (3, KT + 1, 4, 2, 6, 5, "ascending"),
        (2, 197, 4, 1, 24, 24, "ascending"),
    ]


def gqa_width(case):
    B, T, hq, hkv, d, dv, probe = case
    return hq * d + hkv * (d + dv)


def gqa_inputs(case, bf16=False):
    """Rows of [Q | K | V] with the softmax probes of tests/attention_cases.py, scores of magnitude about 100:
    "ascending" puts every row's maximum in the last key tile (100 x a ramp over the keys plus N(0, 1)), "dominant"
    gives every query one key, at a random place, whose score is 100 against N(0, 100 / sqrt(d)) for the rest.
    They fail a kernel that omits the maximum or rescales the running sum wrongly."""
    B, T, hq, hkv, d, dv, probe = case
    g = hq // hkv
    rng = np.random.default_rng(seed_of(case))
    q = rng.standard_normal((B, T, hq, d))
    k = rng.standard_normal((B, T, hkv, d))
    v = rng.standard_normal((B, T, hkv, dv))
    if probe == "ascending":
        u = rng.standard_normal(d)
        u /= np.linalg.norm(u)
        k = (np.arange(T) / max(T - 1, 1))[None, :, None, None] * u + 0.1 * k
        q = 100.0 * u + q
    else:
        k /= np.linalg.norm(k, axis=-1, keepdims=True)
        where = rng.integers(0, T, (B, T, hq))
        q = 100.0 * np.take_along_axis(np.repeat(k, g, axis=2), where[..., None], axis=1)
    x = np.concatenate([t.reshape(B * T, -1) for t in (q, k, v)], axis=1).astype(np.float32)
    return bf16_round(x) if bf16 else x


def gqa_split(x, case):
    B, T, hq, hkv, d, dv, probe = case
    q = x[:, :hq * d].reshape(B, T, hq, d)
    k = x[:, hq * d:(hq + hkv) * d].reshape(B, T, hkv, d)
    v = x[:, (hq + hkv) * d:gqa_width(case)].reshape(B, T, hkv, dv)
    return q, k, v


def gqa_oracle(x, case, causal):
    """softmax(Q K^T) V in float64, head h on K / V head h // (hq // hkv): [B * T][hq * dv]."""
    B, T, hq, hkv, d, dv, probe = case
    q, k, v = (np.asarray(t, np.float64) for t in gqa_split(x, case))
    g = hq // hkv
    k, v = np.repeat(k, g, axis=2), np.repeat(v, g, axis=2)
    s = np.einsum("bqhd,bkhd->bhqk", q, k)
    if causal:
        s = np.where(np.tri(T, dtype=bool), s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("bhqk,bkhd->bqhd", p, v).reshape(B * T, hq * dv)


def gqa_library(x, case, causal):
    """The library's fp32 evaluation on the CPU, for e_ref."""
    import torch.nn.functional as F
    B, T, hq, hkv, d, dv, probe = case
    q, k, v = (torch.from_numpy(np.ascontiguousarray(t)).permute(0, 2, 1, 3) for t in gqa_split(x, case))
    g = hq // hkv
    k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    y = F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=1.0)
    return y.permute(0, 2, 1, 3).reshape(B * T, hq * dv).numpy()


def gqa_expanded(x, case):
    """The same rows with each K / V head repeated g times: what the plain multi-head launch reads."""
    B, T, hq, hkv, d, dv, probe = case
    q, k, v = gqa_split(x, case)
    g = hq // hkv
    return np.ascontiguousarray(np.concatenate([q.reshape(B * T, -1), np.repeat(k, g, axis=2).reshape(B * T, -1),
                                                np.repeat(v, g, axis=2).reshape(B * T, -1)], axis=1))


# ----------------------------------------------------------------------- model
def noisy(w, scale=0.5):
    """An embedding table of O(1), so that a misplaced row shows."""
    for n in list(w):
        if n.endswith("/embeddings"):
            w[n] = (np.random.default_rng(len(n)).standard_normal(w[n].shape) * scale).astype(np.float32)
    return w


def _rms(x, w, name, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w[f"{name}/scale"]


def forward(name, w, ids, all_positions=False):
    """float64 logits of `build_llama(name, ...)` with weights `w` on integer `ids` (B, T): (B, V), or (B, T, V)."""
    depth, width, heads, kv_heads, ffn, vocab, _, eps, wavelength = LLAMA[name]
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    ids = np.asarray(ids).astype(np.int64)
    T, d, g = ids.shape[1], width // heads, heads // kv_heads
    th = rope_angles(T, d, wavelength)
    cs, sn = np.cos(th)[None, :, None, :], np.sin(th)[None, :, None, :]

    def rot(t):
        a, b = t[..., :d // 2], t[..., d // 2:]
        return np.concatenate([a * cs - b * sn, b * cs + a * sn], axis=-1)

    x = w[f"{name}_embed_tokens/embeddings"][ids]
    for i in range(depth):
        b = f"{name}_block_{i}"
        a = f"{b}_attn"
        y = _rms(x, w, f"{b}_input_norm", eps)
        q = rot(np.einsum("btc,chd->bthd", y, w[f"{a}/query/kernel"])) / np.sqrt(float(d))
        k = np.repeat(rot(np.einsum("btc,chd->bthd", y, w[f"{a}/key/kernel"])), g, axis=2)
        v = np.repeat(np.einsum("btc,chd->bthd", y, w[f"{a}/value/kernel"]), g, axis=2)
        s = np.where(np.tri(T, dtype=bool), np.einsum("bqhd,bkhd->bhqk", q, k), -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        o = np.einsum("bhqk,bkhd->bqhd", p, v)
        x = x + np.einsum("bqhd,hdc->bqc", o, w[f"{a}/attention_output/kernel"])
        y = _rms(x, w, f"{b}_post_attention_norm", eps)
        gate = y @ w[f"{b}_mlp_gate/kernel"]
        x = x + (gate / (1.0 + np.exp(-gate)) * (y @ w[f"{b}_mlp_up/kernel"])) @ w[f"{b}_mlp_down/kernel"]
    if not all_positions:
        x = x[:, -1]
    return _rms(x, w, f"{name}_norm", eps) @ w["lm_head/kernel"]


@functools.lru_cache(maxsize=None)
def micro(all_positions=False):
    """(graph, weights, ids (4, T) float32, float64 logits) of llama_micro.  Cached: callers must not modify what
    they get."""
    g = build_llama("llama_micro", all_positions=all_positions)
    w = noisy(init_weights(g, seed=0))
    v = g.layers["llama_micro_embed_tokens"].attrs["input_dim"]
    ids = np.random.default_rng(5).integers(0, v, (4,) + tuple(g.layers[g.input].out_shape))
    return g, w, ids.astype(np.float32), forward("llama_micro", w, ids, all_positions)
