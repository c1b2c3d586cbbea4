"""Wrappers for the self-attention core (csrc/kernels/attention.hip; csrc/kernels/attention_core.h holds the
scheme of all three), the attention core with separate query /
key / value sources (csrc/kernels/cross_attention.hip), Swin's window attention core and its bias packer
(csrc/kernels/window_attention.hip), and the ViT class token / position embedding, learned-queries and token
embedding kernels and the rotary position embedding with its host-side table (csrc/kernels/layers.hip).

Shapes, dtypes, strides and the 32-bit index range are checked here before any launch; a shape the kernels do
not take is an error, never a fall-back to torch.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ._lib import kernels, ptr, stream_handle
from .eltwise import _chk


def attention_tiles():
    """(queries per block, keys per LDS tile) of the MFMA path."""
    k = kernels()
    return int(k.attention_query_tile()), int(k.attention_key_tile())


def attention_path(key_dim: int, value_dim: int) -> str:
    """'mfma' (flash-style on the fp32 MFMA) or 'plain' (one wave per query) for a head of this size."""
    return "mfma" if kernels().attention_path(int(key_dim), int(value_dim)) else "plain"


def attention(qkv: torch.Tensor, out: torch.Tensor, batch: int, tokens: int, heads: int, key_dim: int,
              value_dim: Optional[int] = None, stream=None, causal: bool = False,
              key_mask: Optional[torch.Tensor] = None, kv_heads: Optional[int] = None) -> torch.Tensor:
    """out = softmax(Q K^T) V per (image, head); `causal`: query i attends keys j <= i only (Keras'
    use_causal_mask), on the kernels' masked instantiations, which skip the key tiles above the diagonal.  qkv [..., ld_in] holds batch * tokens rows of [Q | K | V]
    (head-major inside each part; Q already scaled by 1/sqrt(key_dim)), out [..., ld_out] gets heads * value_dim
    channels per row and zeros in the rest of the row.  fp32 or bf16 activations (both tensors alike); the
    row strides are the last dimensions, the true widths come from heads / key_dim / value_dim.  `key_mask`: a
    padding mask of batch * tokens fp32 values on the device (never with `causal`); token j of an image is padding
    iff -1 < key_mask[j] < 1, the ids of an Embedding(mask_zero=True).  A padded key is not attended, a padded
    query's row and every row of an image with no kept key are zeros, and the key tiles past an image's last kept
    token are not loaded (the kernels' masked instantiations).  `kv_heads` (grouped-query attention): the `heads`
    query heads share kv_heads key / value heads, head h reads K / V head h // (heads // kv_heads), and a row is
    [Q: heads x key_dim | K: kv_heads x key_dim | V: kv_heads x value_dim]; given and different from `heads` it
    runs the gqa entry points (plain or causal, never with `key_mask`), else the launch is the one it always was."""
    dv = int(value_dim or key_dim)
    B, T, h, d = int(batch), int(tokens), int(heads), int(key_dim)
    hkv = h if kv_heads is None else int(kv_heads)
    if hkv < 1 or h < 1 or h % hkv:
        raise ValueError(f"attention: kv_heads={kv_heads} must be positive and divide the {h} heads")
    if hkv != h and key_mask is not None:
        raise ValueError("attention: a padding mask together with kv_heads is not built")
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"attention: fp32 or bf16 tensors, got {qkv.dtype}")
    _chk(qkv, qkv.dtype, "qkv"); _chk(out, qkv.dtype, "out")
    if min(B, T, h, d, dv) < 1:
        raise ValueError(f"attention: batch, tokens, heads and head sizes must be positive ({B}, {T}, {h}, {d}, {dv})")
    ld_in, ld_out = qkv.shape[-1], out.shape[-1]
    if (qkv.numel() != B * T * ld_in or out.numel() != B * T * ld_out or ld_in < h * d + hkv * (d + dv)
            or ld_out < h * dv):
        raise ValueError(f"attention: qkv{tuple(qkv.shape)} out{tuple(out.shape)} do not hold {B} x {T} rows of "
                         f"{h} heads ({d}, {dv})" + (f" over {hkv} key / value heads" if hkv != h else ""))
    if max(qkv.numel(), out.numel(), B * h * T) >= 2 ** 31:
        raise ValueError("attention: tensors must hold fewer than 2^31 elements (32-bit index math)")
    if key_mask is not None:
        if causal:
            raise ValueError("attention: a padding mask together with the causal mask is not built")
        _chk(key_mask, torch.float32, "key_mask")
        if key_mask.numel() != B * T:
            raise ValueError(f"attention: key_mask{tuple(key_mask.shape)} does not hold {B} x {T} values")
        fn = kernels().attention_masked_f32 if qkv.dtype == torch.float32 else kernels().attention_masked_bf16
        fn(ptr(qkv), ptr(key_mask), ptr(out), B, T, h, d, dv, int(ld_in), int(ld_out), stream_handle(stream))
        return out
    if hkv != h:
        k, f32 = kernels(), qkv.dtype == torch.float32
        if causal:
            fn = k.attention_gqa_causal_f32 if f32 else k.attention_gqa_causal_bf16
        else:
            fn = k.attention_gqa_f32 if f32 else k.attention_gqa_bf16
        fn(ptr(qkv), ptr(out), B, T, h, hkv, d, dv, int(ld_in), int(ld_out), stream_handle(stream))
        return out
    if causal:
        fn = kernels().attention_causal_f32 if qkv.dtype == torch.float32 else kernels().attention_causal_bf16
    else:
        fn = kernels().attention_f32 if qkv.dtype == torch.float32 else kernels().attention_bf16
    fn(ptr(qkv), ptr(out), B, T, h, d, dv, int(ld_in), int(ld_out), stream_handle(stream))
    return out


def rope_table(tokens: int, key_dim: int, max_wavelength: float = 10000.0, device=None) -> torch.Tensor:
    """The cos / sin table of the rotary position embedding, fp32 [2][T][d/2]: table[0, t, i] = cos(theta),
    table[1, t, i] = sin(theta) with theta(t, i) = t * W^(-2i/d).  The angles, their cosines and sines are computed
    in float64 on the host and rounded once to fp32 (an fp32 angle t * freq is already off by 5e-4 rad at
    t = 8192); the table stays fp32 in both precisions.  Frequency scaling (keras_hub's scaling_factor, Llama 3's
    banded scaling) is not built: it would change this function alone."""
    T, d, W = int(tokens), int(key_dim), float(max_wavelength)
    if T < 1 or d < 2 or d % 2 or not W > 0:
        raise ValueError(f"rope_table: tokens >= 1, an even key_dim >= 2 and a positive wavelength "
                         f"(got {tokens}, {key_dim}, {max_wavelength})")
    i = np.arange(d // 2, dtype=np.float64)
    theta = np.arange(T, dtype=np.float64)[:, None] * np.power(np.float64(W), -2.0 * i / d)[None, :]
    t = torch.from_numpy(np.stack([np.cos(theta), np.sin(theta)]).astype(np.float32))
    return t.to(device) if device is not None else t


def rope(x: torch.Tensor, table: torch.Tensor, out: torch.Tensor, tokens: int, heads: int, key_dim: int,
         value_dim: Optional[int] = None, kv_heads: Optional[int] = None, stream=None) -> torch.Tensor:
    """Rotary position embedding on an attention layer's projection buffer, out of place
    (csrc/kernels/layers.hip): x and out [..., ld] hold rows of [Q: heads x key_dim | K: kv_heads x key_dim |
    V: kv_heads x value_dim]; the Q and K heads are rotated by the rotate-half convention with the angles of
    `table` (`rope_table`, fp32 [2][tokens][key_dim / 2]) at position row % tokens, V is copied and the rest of a
    row is written as zeros.  fp32 or bf16 (both tensors alike); key_dim must be even."""
    T, h, d = int(tokens), int(heads), int(key_dim)
    dv = int(value_dim or key_dim)
    hkv = h if kv_heads is None else int(kv_heads)
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"rope: fp32 or bf16 tensors, got {x.dtype}")
    if d < 2 or d % 2:
        raise ValueError(f"rope: key_dim={d} must be even (the rotation pairs channel i with i + key_dim / 2)")
    _chk(x, x.dtype, "x"); _chk(out, x.dtype, "out"); _chk(table, torch.float32, "table")
    if min(T, h, hkv, dv) < 1:
        raise ValueError(f"rope: tokens, heads and head sizes must be positive ({T}, {h}, {hkv}, {d}, {dv})")
    ld = x.shape[-1]
    rows = x.numel() // ld
    if (out.shape[-1] != ld or out.numel() != x.numel() or rows % T or ld < (h + hkv) * d + hkv * dv
            or tuple(table.shape) != (2, T, d // 2)):
        raise ValueError(f"rope: x{tuple(x.shape)} out{tuple(out.shape)} table{tuple(table.shape)} do not hold rows "
                         f"of {h} + {hkv} heads of {d} and {hkv} of {dv} at {T} positions")
    if x.data_ptr() == out.data_ptr():
        raise ValueError("rope: the step is out of place; x and out must differ")
    if max(x.numel(), table.numel()) >= 2 ** 31:
        raise ValueError("rope: tensors must hold fewer than 2^31 elements (32-bit index math)")
    fn = kernels().rope_f32 if x.dtype == torch.float32 else kernels().rope_bf16
    fn(ptr(x), ptr(table), ptr(out), rows, T, h, hkv, d, dv, int(ld), stream_handle(stream))
    return out


def cross_attention_tiles():
    """(queries per block, keys per LDS tile) of the cross-attention kernel's MFMA path."""
    k = kernels()
    return int(k.cross_attention_query_tile()), int(k.cross_attention_key_tile())


def _rows_view(t: torch.Tensor, dtype, name: str):
    """(row stride, width) of a tensor view whose rows are its last dimension: contiguous, or a column slice of a
    contiguous buffer (every leading stride then follows from the row stride)."""
    if t.dtype != dtype:
        raise ValueError(f"cross_attention: {name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"cross_attention: {name}: must be a device tensor")
    if t.dim() < 2 or t.numel() == 0 or t.stride(-1) != 1:
        raise ValueError(f"cross_attention: {name}{tuple(t.shape)}: rows must be the last dimension, unit stride")
    ld = t.stride(-2)
    want = ld
    for i in range(t.dim() - 2, -1, -1):
        if t.shape[i] != 1 and t.stride(i) != want:
            raise ValueError(f"cross_attention: {name}{tuple(t.shape)} strides {t.stride()}: not rows of one stride")
        want *= t.shape[i]
    if ld < t.shape[-1]:
        raise ValueError(f"cross_attention: {name}: row stride {ld} below the width {t.shape[-1]}")
    return int(ld), int(t.shape[-1])


def cross_attention_path(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, key_dim: int,
                         value_dim: Optional[int] = None) -> str:
    """'mfma' or 'plain' for these views: the MFMA path needs head sizes that are multiples of 16 up to 128, the four
    addresses aligned to 4 elements and row strides that are multiples of 4."""
    d, dv = int(key_dim), int(value_dim or key_dim)
    lds = [t.stride(-2) if t.dim() >= 2 else t.shape[-1] for t in (q, k, v, out)]
    return "mfma" if kernels().cross_attention_path(ptr(q), ptr(k), ptr(v), ptr(out), d, dv, *(int(x) for x in lds),
                                                    q.element_size()) else "plain"


def cross_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, batch: int, tokens_q: int,
                    tokens_k: int, heads: int, key_dim: int, value_dim: Optional[int] = None, stream=None) -> torch.Tensor:
    """out = softmax(Q K^T) V per (image, head) with separate sources (csrc/kernels/cross_attention.hip).  q holds
    batch * tokens_q rows of heads * key_dim channels (Q already scaled by 1/sqrt(key_dim)), k batch * tokens_k rows
    of heads * key_dim, v batch * tokens_k rows of heads * value_dim, head-major; each is a tensor view whose row
    stride may exceed its width: a whole buffer, or a column slice of one ([Q | K] or [K | V] side by side).  out
    [..., ld_out] (contiguous) gets heads * value_dim channels per row and zeros in the rest of the row.  fp32 or
    bf16, all four alike."""
    dv = int(value_dim or key_dim)
    B, Tq, Tk, h, d = int(batch), int(tokens_q), int(tokens_k), int(heads), int(key_dim)
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"cross_attention: fp32 or bf16 tensors, got {q.dtype}")
    if min(B, Tq, Tk, h, d, dv) < 1:
        raise ValueError(f"cross_attention: batch, tokens, heads and head sizes must be positive "
                         f"({B}, {Tq}, {Tk}, {h}, {d}, {dv})")
    (ldq, wq), (ldk, wk), (ldv, wv) = (_rows_view(t, q.dtype, n) for t, n in ((q, "q"), (k, "k"), (v, "v")))
    _chk(out, q.dtype, "out")
    ld_out = int(out.shape[-1])
    if (q.numel() != B * Tq * wq or k.numel() != B * Tk * wk or v.numel() != B * Tk * wv
            or out.numel() != B * Tq * ld_out or wq < h * d or wk < h * d or wv < h * dv or ld_out < h * dv):
        raise ValueError(f"cross_attention: q{tuple(q.shape)} k{tuple(k.shape)} v{tuple(v.shape)} out{tuple(out.shape)} "
                         f"do not hold {B} x {Tq} query and {B} x {Tk} key / value rows of {h} heads ({d}, {dv})")
    if max(B * Tq * ldq, B * Tk * ldk, B * Tk * ldv, out.numel(), B * h * Tq) >= 2 ** 31:
        raise ValueError("cross_attention: every tensor must span fewer than 2^31 elements (32-bit index math)")
    fn = kernels().attention_qkv_f32 if q.dtype == torch.float32 else kernels().attention_qkv_bf16
    fn(ptr(q), ptr(k), ptr(v), ptr(out), B, Tq, Tk, h, d, dv, ldq, ldk, ldv, ld_out, stream_handle(stream))
    return out


def queries(emb: torch.Tensor, out: torch.Tensor, C: Optional[int] = None, stream=None) -> torch.Tensor:
    """LearnedQueries: out[b, 0, t] = emb[t] for every image b.  emb [N, C] fp32, out [B, 1, N, Cp] fp32 (Cp = C)
    or bf16 (rows padded to Cp channels with `C` real ones; the padding is written as zeros)."""
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"queries: fp32 or bf16 output, got {out.dtype}")
    _chk(emb, torch.float32, "emb"); _chk(out, out.dtype, "out")
    if emb.dim() != 2 or emb.numel() == 0:
        raise ValueError(f"queries: emb{tuple(emb.shape)} is not [N, C]")
    N, Ce = int(emb.shape[0]), int(emb.shape[1])
    Cp, B = int(out.shape[-1]), int(out.shape[0])
    C = Ce if C is None else int(C)
    if C != Ce or Cp < C or (out.dtype == torch.float32 and Cp != C) or (out.dtype == torch.bfloat16 and Cp % 8):
        raise ValueError(f"queries: emb{tuple(emb.shape)} does not fill rows of {Cp} channels ({C} real, {out.dtype})")
    if B < 1 or out.numel() != B * N * Cp:
        raise ValueError(f"queries: out{tuple(out.shape)} is not [B, 1, {N}, {Cp}]")
    if out.numel() >= 2 ** 31:
        raise ValueError("queries: tensors must hold fewer than 2^31 elements")
    if out.dtype == torch.float32:
        kernels().queries_f32(ptr(emb), ptr(out), B, N, C, stream_handle(stream))
    else:
        kernels().queries_bf16(ptr(emb), ptr(out), B, N, Cp, C, stream_handle(stream))
    return out


def embedding_table(embeddings, dtype, device=None) -> torch.Tensor:
    """A Keras Embedding's (V, C) weight as the table the `embedding` kernel gathers from, prepared once: fp32
    (V, C), or bf16 with rows padded to a multiple of 8 channels and the padding written as zeros."""
    t = np.ascontiguousarray(embeddings.detach().cpu().numpy() if torch.is_tensor(embeddings) else embeddings,
                             np.float32)
    if t.ndim != 2 or t.size == 0:
        raise ValueError(f"embedding_table: embeddings {t.shape} are not (V, C)")
    if dtype == torch.float32:
        res = torch.from_numpy(t)
    elif dtype == torch.bfloat16:
        cp = (t.shape[1] + 7) // 8 * 8
        res = torch.zeros((t.shape[0], cp), dtype=torch.bfloat16)
        res[:, :t.shape[1]] = torch.from_numpy(t).to(torch.bfloat16)
    else:
        raise ValueError(f"embedding_table: fp32 or bf16, got {dtype}")
    return res.to(device) if device is not None else res


def embedding(ids: torch.Tensor, table: torch.Tensor, out: torch.Tensor, stream=None) -> torch.Tensor:
    """Keras Embedding: out[r] = table[int(ids[r])] for every token id.  ids [B, T] are float32 (the transport
    moves float tensors; Keras casts a float input to int32) and truncated toward zero; `table` is what
    `embedding_table` prepared, [V, ld] in the activation dtype with V <= 2**24, so every id is exact; out
    [B, 1, T, ld] has the table's dtype and row length.  An id outside [0, V), an infinity or a NaN yields a zero
    row, TensorFlow's GPU gather behaviour: a kernel cannot raise."""
    if table.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"embedding: fp32 or bf16 table, got {table.dtype}")
    _chk(ids, torch.float32, "ids"); _chk(table, table.dtype, "table"); _chk(out, table.dtype, "out")
    if table.dim() != 2 or table.numel() == 0 or ids.numel() == 0:
        raise ValueError(f"embedding: table{tuple(table.shape)} is not [V, ld], or ids{tuple(ids.shape)} are empty")
    V, ld, rows = int(table.shape[0]), int(table.shape[1]), int(ids.numel())
    if V > 2 ** 24:
        raise ValueError(f"embedding: {V} rows exceed 2**24, beyond which a float32 id is not exact")
    if out.shape[-1] != ld or out.numel() != rows * ld or (table.dtype == torch.bfloat16 and ld % 8):
        raise ValueError(f"embedding: out{tuple(out.shape)} does not hold {rows} rows of the table's {ld} elements "
                         f"(bf16 rows are padded to 8 channels)")
    if max(table.numel(), out.numel()) >= 2 ** 31:
        raise ValueError("embedding: tensors must hold fewer than 2^31 elements (32-bit index math)")
    fn = kernels().embedding_f32 if table.dtype == torch.float32 else kernels().embedding_bf16
    fn(ptr(ids), ptr(table), ptr(out), rows, V, ld, stream_handle(stream))
    return out


def window_attention_tiles():
    """(queries per block, keys per LDS tile) of the window attention's MFMA path; the packed bias' rows are
    padded to the key tile."""
    k = kernels()
    return int(k.window_attention_query_tile()), int(k.window_attention_key_tile())


def window_attention_path(key_dim: int) -> str:
    """'mfma' or 'plain' (one wave per query) for a window attention head of this size."""
    return "mfma" if kernels().window_attention_path(int(key_dim)) else "plain"


def window_bias(table, window: int, shift: int, device=None) -> torch.Tensor:
    """The bias a window attention kernel adds to its scores, packed once per layer: fp32
    [classes][heads][Tp][Tp] with Tp = window^2 rounded up to the key tile and zeros in the padding.
    bias[c, h, q, k] = table[index[q, k], h] + mask_c[q, k]: Swin's relative position bias (`table`
    [(2M-1)^2][heads], numpy or torch) plus, under a shift, the additive -100 between tokens of different
    regions.  Inside one window the regions only depend on whether the window is in the last window row and /
    or the last window column, so there are four classes, c = 2 (last row) + (last column), and one without a
    shift.  Token (i, j) of such a window has row part 1 for i < M - shift, else 2 (0 off the last window row),
    the column part alike, and region 3 x row part + column part."""
    from ..graph.ir import window_index
    M, s = int(window), int(shift)
    t = np.asarray(table.detach().cpu() if torch.is_tensor(table) else table, np.float32)
    if M < 1 or not 0 <= s < M or t.ndim != 2 or t.shape[0] != (2 * M - 1) ** 2:
        raise ValueError(f"window_bias: table {t.shape} is not [(2M-1)^2][heads] for window {M}, or the shift {s} "
                         f"is not in [0, {M})")
    T = M * M
    kt = window_attention_tiles()[1]
    Tp = (T + kt - 1) // kt * kt
    rel = t[window_index(M).reshape(-1)].reshape(T, T, -1).transpose(2, 0, 1)          # (heads, T, T)
    part = np.where(np.arange(M) < M - s, 1, 2)
    out = np.zeros((4 if s else 1, t.shape[1], Tp, Tp), np.float32)
    for c in range(out.shape[0]):
        rows = part if c & 2 else np.zeros(M, np.int64)
        cols = part if c & 1 else np.zeros(M, np.int64)
        region = (3 * rows[:, None] + cols[None, :]).reshape(-1)
        mask = np.where(region[:, None] != region[None, :], np.float32(-100.0), np.float32(0.0))
        out[c, :, :T, :T] = rel + mask
    res = torch.from_numpy(out)
    return res.to(device) if device is not None else res


def window_attention(qkv: torch.Tensor, bias: torch.Tensor, out: torch.Tensor, batch: int, height: int, width: int,
                     window: int, shift: int, heads: int, key_dim: int, stream=None) -> torch.Tensor:
    """Swin window attention core on an NHWC map, nothing rolled or partitioned in memory
    (csrc/kernels/window_attention.hip).  qkv [..., ld_in] holds batch * height * width rows of [Q | K | V]
    (head-major, heads x key_dim each; Q already scaled), `bias` is what `window_bias` packed for this window and
    shift, out [..., ld_out] gets heads * key_dim channels per row and zeros in the rest of the row.  fp32 or
    bf16 activations (both tensors alike, the bias always fp32)."""
    B, H, W, M, s, h, d = (int(v) for v in (batch, height, width, window, shift, heads, key_dim))
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"window_attention: fp32 or bf16 tensors, got {qkv.dtype}")
    _chk(qkv, qkv.dtype, "qkv"); _chk(out, qkv.dtype, "out"); _chk(bias, torch.float32, "bias")
    if min(B, H, W, M, h, d) < 1:
        raise ValueError(f"window_attention: batch, map, window, heads and head size must be positive "
                         f"({B}, {H}, {W}, {M}, {h}, {d})")
    if H % M or W % M:
        raise ValueError(f"window_attention: the {H} x {W} map is not a multiple of the {M} x {M} window")
    if not 0 <= s < M:
        raise ValueError(f"window_attention: shift {s} is not in [0, {M})")
    kt = window_attention_tiles()[1]
    Tp = (M * M + kt - 1) // kt * kt
    if tuple(bias.shape) != (4 if s else 1, h, Tp, Tp):
        raise ValueError(f"window_attention: bias{tuple(bias.shape)} is not {(4 if s else 1, h, Tp, Tp)} "
                         f"(window_bias of window {M}, shift {s}, {h} heads)")
    ld_in, ld_out = qkv.shape[-1], out.shape[-1]
    if qkv.numel() != B * H * W * ld_in or out.numel() != B * H * W * ld_out or ld_in < 3 * h * d or ld_out < h * d:
        raise ValueError(f"window_attention: qkv{tuple(qkv.shape)} out{tuple(out.shape)} do not hold {B} x {H} x {W} "
                         f"rows of {h} heads of {d}")
    if max(qkv.numel(), out.numel(), bias.numel(), B * H * W * h) >= 2 ** 31:
        raise ValueError("window_attention: tensors must hold fewer than 2^31 elements (32-bit index math)")
    fn = kernels().window_attention_f32 if qkv.dtype == torch.float32 else kernels().window_attention_bf16
    fn(ptr(qkv), ptr(bias), ptr(out), B, H, W, M, s, h, d, int(ld_in), int(ld_out), stream_handle(stream))
    return out


def posembed(x: torch.Tensor, cls: Optional[torch.Tensor], pos: torch.Tensor, out: torch.Tensor, C: Optional[int] = None,
             stream=None) -> torch.Tensor:
    """ViT class token + position embedding: out[b, 0] = cls + pos[0] (when `cls` is given),
    out[b, ct + t] = x[b, t] + pos[ct + t].  x [B, ..., Cp] with T positions per image, out [B, 1, T + ct, Cp],
    cls [C] and pos [T + ct, C] fp32.  bf16 rows are padded to Cp channels with `C` real ones; the padding of
    `out` is written as zeros whatever x holds there."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"posembed: fp32 or bf16 tensors, got {x.dtype}")
    _chk(x, x.dtype, "x"); _chk(out, x.dtype, "out"); _chk(pos, torch.float32, "pos")
    ct = 0 if cls is None else 1
    if ct:
        _chk(cls, torch.float32, "cls")
    Cp, B = x.shape[-1], x.shape[0]
    C = Cp if C is None else int(C)
    if x.dtype == torch.float32 and C != Cp:
        raise ValueError(f"posembed: fp32 rows are not padded (C={C}, row {Cp})")
    if x.dtype == torch.bfloat16 and (Cp % 8 or not 0 < C <= Cp):
        raise ValueError(f"posembed: bf16 rows are padded to 8 channels (Cp={Cp}, C={C})")
    if x.numel() == 0 or B < 1:
        raise ValueError("posembed: empty input")
    T = x.numel() // (B * Cp)
    if (out.shape[-1] != Cp or out.numel() != B * (T + ct) * Cp or pos.numel() != (T + ct) * C
            or (ct and cls.numel() != C)):
        raise ValueError(f"posembed: bad shapes x{tuple(x.shape)} out{tuple(out.shape)} pos{tuple(pos.shape)}")
    if out.numel() >= 2 ** 31:
        raise ValueError("posembed: tensors must hold fewer than 2^31 elements")
    if x.dtype == torch.float32:
        kernels().posembed_f32(ptr(x), ptr(cls) if ct else 0, ptr(pos), ptr(out), B, T, C, ct, stream_handle(stream))
    else:
        kernels().posembed_bf16(ptr(x), ptr(cls) if ct else 0, ptr(pos), ptr(out), B, T, Cp, C, ct,
                                stream_handle(stream))
    return out
