"""Wrappers for the self-attention core (csrc/kernels/attention.hip) and the ViT class token / position
embedding kernel (csrc/kernels/layers.hip).

Shapes, dtypes, strides and the 32-bit index range are checked here before any launch; a shape the kernels do
not take is an error, never a fall-back to torch.
"""
from __future__ import annotations

from typing import Optional

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
              value_dim: Optional[int] = None, stream=None) -> torch.Tensor:
    """out = softmax(Q K^T) V per (image, head).  qkv [..., ld_in] holds batch * tokens rows of [Q | K | V]
    (head-major inside each part; Q already scaled by 1/sqrt(key_dim)), out [..., ld_out] gets heads * value_dim
    channels per row and zeros in the rest of the row.  fp32 or bf16 activations (both tensors alike); the
    row strides are the last dimensions, the true widths come from heads / key_dim / value_dim."""
    dv = int(value_dim or key_dim)
    B, T, h, d = int(batch), int(tokens), int(heads), int(key_dim)
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"attention: fp32 or bf16 tensors, got {qkv.dtype}")
    _chk(qkv, qkv.dtype, "qkv"); _chk(out, qkv.dtype, "out")
    if min(B, T, h, d, dv) < 1:
        raise ValueError(f"attention: batch, tokens, heads and head sizes must be positive ({B}, {T}, {h}, {d}, {dv})")
    ld_in, ld_out = qkv.shape[-1], out.shape[-1]
    if (qkv.numel() != B * T * ld_in or out.numel() != B * T * ld_out or ld_in < h * (2 * d + dv)
            or ld_out < h * dv):
        raise ValueError(f"attention: qkv{tuple(qkv.shape)} out{tuple(out.shape)} do not hold {B} x {T} rows of "
                         f"{h} heads ({d}, {dv})")
    if max(qkv.numel(), out.numel(), B * h * T) >= 2 ** 31:
        raise ValueError("attention: tensors must hold fewer than 2^31 elements (32-bit index math)")
    fn = kernels().attention_f32 if qkv.dtype == torch.float32 else kernels().attention_bf16
    fn(ptr(qkv), ptr(out), B, T, h, d, dv, int(ld_in), int(ld_out), stream_handle(stream))
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
