"""Cases of the bf16-MFMA attention kernel (csrc/kernels/attention_bf16.h, `math="bf16"`): the inputs, float64 oracles
and allowance of tests/attention_cases.py / tests/causal_attention_cases.py on the bf16-rounded values, plus P|V|.

* T = 1; T one below, at and one above the key tile and the query tile (they coincide at 64);
* B = 2 and 3 with T off both tiles; heads 1 and 3;
* (d, dv) = (16, 16), (32, 16), (48, 80), (64, 64), (128, 128): every register size, d != dv, and d % 32 == 16 (the
  zero half-step of the score product);
* the ascending, the descending and the dominant probe, each over three key tiles;
* one case again with Q scaled by d^-1/2 (scores of N(0, 1): many keys with weight).

Cached per case: callers must not modify what they get.
"""
import functools
import types

import numpy as np
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.attention import (
    attention_bf16_tiles)

import attention_cases as AC
import causal_attention_cases as CC

QT, KT = attention_bf16_tiles()

CASES = sorted({
    (1, 1, 1, 16, 16, None),
    (1, KT - 1, 1, 16, 16, None), (1, KT, 1, 32, 16, None), (1, KT + 1, 1, 48, 80, None),
    (1, QT - 1, 3, 16, 16, None), (1, QT, 1, 64, 64, None), (1, QT + 1, 1, 128, 128, None),
    (2, KT + 5, 1, 128, 128, None), (3, QT + 6, 3, 32, 16, None), (2, 37, 3, 48, 80, None),
    (1, 2 * KT + 6, 1, 16, 16, "ascending"), (1, 2 * KT + 6, 1, 48, 80, "descending"),
    (2, 2 * KT + 6, 2, 64, 64, "dominant"),
}, key=repr)
SCALED = [(2, KT + 5, 1, 128, 128, None)]
GUARD_CASES = [((1, 1, 1, 16, 16, None), False), ((2, KT + 5, 1, 128, 128, None), False),
               ((1, QT + 1, 1, 128, 128, None), True), ((2, 37, 3, 48, 80, None), True)]
# (B, T, hq, hkv, d, dv, probe) of tests/llama_cases.py, off the tiles
GQA_CASES = [(2, KT + 5, 4, 1, 64, 64, "ascending"), (3, 37, 4, 2, 32, 32, "dominant")]


def bound(want, pabsv, allow):
    """The elementwise bound of tests/test_attention_bf16_gpu.py."""
    return 2.0 ** -8 * np.abs(want) + 2.0 ** -8 * pabsv + allow


@functools.lru_cache(maxsize=None)
def case(c, causal=False, scaled=False):
    """The bf16 case of AC / CC; `scaled`: Q multiplied by d^-1/2 and rounded to bf16 again.  `pabsv` is the oracle's
    softmax applied to |V|."""
    M = CC if causal else AC
    k = types.SimpleNamespace(**vars(M.case_bf16(c)))
    if scaled:
        k.qkv = k.qkv.copy()
        k.qkv[:, :k.heads * k.d] *= np.float32(k.d ** -0.5)
        k.qkv = torch.from_numpy(k.qkv).to(torch.bfloat16).float().numpy()
        k.want = M.ref_attention(k.qkv, k.B, k.T, k.heads, k.d, k.dv)
        k.e_ref, k.allow = M.f32_allowance(k.qkv, c, k.want)
    a = k.qkv.copy()
    a[:, 2 * k.heads * k.d:] = np.abs(a[:, 2 * k.heads * k.d:])
    k.pabsv = M.ref_attention(a, k.B, k.T, k.heads, k.d, k.dv)
    return k
