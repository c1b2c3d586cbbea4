"""MXFP4 weights (OCP Microscaling Formats v1.0), on the host in numpy: quantiser, exact dequantiser and the device
layout of csrc/kernels/gemm_skinny_mx.h.

A weight matrix is [N][K] (output channel, input channel).  Every 32 consecutive k of a channel form a block with
one shared exponent e (the e8m0 scale 2^e, stored biased: e + 127) and one e2m1 code per element: a sign bit over
the magnitudes MXFP4_VALUES.  The value is code x 2^e: at most two significant bits, so with |e| <= 64 every one is
a normal bf16 number and `dequantize_mxfp4` of anything is its own bf16 rounding.

On the host the codes are one uint8 (0 .. 15) per element, [N][K], and the exponents int8 [N][ceil(K / 32)] (a
last block may be partial).  `pack_mxfp4` packs them two codes a byte, the lower nibble the lower k, into the
kernel's words; `unpack_mxfp4` is its inverse."""
from __future__ import annotations

import numpy as np

MXFP4_VALUES = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], np.float32)    # e2m1 magnitudes by code & 7
_MIDPOINTS = (MXFP4_VALUES[:-1].astype(np.float64) + MXFP4_VALUES[1:]) / 2        # ties go to the even code
MX_BLOCK = 32                 # k per shared exponent
MX_KC = 128                   # k per chunk of the kernel: rows are padded to it (gemm_skinny_mx.h MX_KC)
MX_N_ALIGN = 128              # channels are padded to the widest channel tile, 16 x 8
MX_EXP_CLAMP = 64             # |e| <= 64: no dequantised value is a bf16 subnormal, and the byte 255 (NaN) never appears
_E2M1_EMAX = 2                # 6 = 1.5 x 2^2


def quantize_mxfp4(w: np.ndarray):
    """(codes uint8 [N][K], exponents int8 [N][ceil(K / 32)]) of float weights w [N][K]: per block the shared
    exponent floor(log2(max |w|)) - 2 clamped to +-64 (0 for an all-zero block), elements rounded to the nearest
    code, ties to the even code, saturating at +-6."""
    w = np.asarray(w)
    if w.dtype != np.float32:                 # float32 stays float32: every step below is exact in either type
        w = w.astype(np.float64)
    if w.ndim != 2:
        raise ValueError(f"quantize_mxfp4 takes a weight matrix [N][K], got shape {w.shape}")
    N, K = w.shape
    nb = -(-K // MX_BLOCK)
    blocks = np.zeros((N, nb * MX_BLOCK), w.dtype)
    blocks[:, :K] = w
    blocks = blocks.reshape(N, nb, MX_BLOCK)
    amax = np.abs(blocks).max(-1)
    exps = np.where(amax > 0, np.frexp(amax)[1] - 1 - _E2M1_EMAX, 0)               # frexp: amax = m 2^e, m in [.5, 1)
    exps = np.clip(exps, -MX_EXP_CLAMP, MX_EXP_CLAMP).astype(np.int8)
    a = np.abs(np.ldexp(blocks, -exps[..., None].astype(np.int32)))                  # exact: a power-of-two scale
    mids = _MIDPOINTS.astype(w.dtype)
    idx = np.searchsorted(mids, a, side="left")                                      # a tie lands on the lower code
    tie = a == mids[np.minimum(idx, len(mids) - 1)]
    idx = idx + (tie & (idx % 2 == 1))                                               # ... and moves up if that is odd
    codes = (idx | (np.signbit(blocks) << 3)).astype(np.uint8)
    return np.ascontiguousarray(codes.reshape(N, -1)[:, :K]), exps


def dequantize_mxfp4(codes: np.ndarray, exponents: np.ndarray) -> np.ndarray:
    """float32 [N][K] values code x 2^e of `quantize_mxfp4`'s pair, exact."""
    codes = np.asarray(codes)
    mag = MXFP4_VALUES[codes & 7] * np.where(codes & 8, np.float32(-1), np.float32(1))
    e = np.repeat(np.asarray(exponents, np.int32), MX_BLOCK, axis=1)[:, :codes.shape[1]]
    return np.ldexp(mag, e).astype(np.float32)


def pack_mxfp4(codes: np.ndarray, exponents: np.ndarray):
    """(words uint32 [Npad][Kpad / 128][q = 4][s = 4], scales uint32 [Npad][Kpad / 128]) of gemm_skinny_mx.h: word
    (q, s) of row n and chunk c holds the codes of k = 128 c + 32 s + 8 q .. + 7, the lowest k in the lowest nibble;
    byte s of a scale dword is e + 127 of block 4 c + s.  Rows are padded with zero codes to a multiple of 128 k,
    channels with zero rows to a multiple of 128; padding blocks carry exponent 0."""
    codes, exponents = np.asarray(codes, np.uint8), np.asarray(exponents, np.int8)
    N, K = codes.shape
    Kpad, Npad = -(-K // MX_KC) * MX_KC, -(-N // MX_N_ALIGN) * MX_N_ALIGN
    nch = Kpad // MX_KC
    c = np.zeros((Npad, Kpad), np.uint32)
    c[:N, :K] = codes
    c = c.reshape(Npad, nch, 4, 4, 8)                                                # [n][chunk][s][q][j]
    words = (c << (4 * np.arange(8, dtype=np.uint32))).sum(-1, dtype=np.uint32).transpose(0, 1, 3, 2)
    e = np.full((Npad, nch * 4), 127, np.uint32)
    e[:N, :exponents.shape[1]] = exponents.astype(np.int32) + 127
    scales = (e.reshape(Npad, nch, 4) << (8 * np.arange(4, dtype=np.uint32))).sum(-1, dtype=np.uint32)
    return np.ascontiguousarray(words), np.ascontiguousarray(scales)


def unpack_mxfp4(words: np.ndarray, scales: np.ndarray, N: int, K: int):
    """`pack_mxfp4`'s inverse: the (codes [N][K], exponents [N][ceil(K / 32)]) the layout holds."""
    words, scales = np.asarray(words, np.uint32), np.asarray(scales, np.uint32)
    Npad, nch = scales.shape
    nib = (words.transpose(0, 1, 3, 2)[..., None] >> (4 * np.arange(8, dtype=np.uint32))) & 15
    e = ((scales[..., None] >> (8 * np.arange(4, dtype=np.uint32))) & 255).astype(np.int32) - 127
    return (np.ascontiguousarray(nib.reshape(Npad, nch * MX_KC)[:N, :K].astype(np.uint8)),
            np.ascontiguousarray(e.reshape(Npad, nch * 4)[:N, :-(-K // MX_BLOCK)].astype(np.int8)))
