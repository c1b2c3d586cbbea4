"""Cases of the wide attention heads (csrc/kernels/attention_wide.h), shared by the GPU and guard-band tests.  The
inputs, the float64 oracles and the allowance are those of tests/attention_cases.py and, under the causal mask,
tests/causal_attention_cases.py (imported, not copied); this file only lists the shapes, with the tile sizes read
per head size from the kernels module, and rescales Q for the two cases that run a second time.

* T = 1; T one below and one above the key tile at 256; T one above the query tile at 512; two images off both
  tiles at 512;
* (160, 192): uneven slices per wave (3, 3, 2, 2 of d; 3 each of dv), d != dv, two heads, the 256 instantiation;
* (144, 16): three waves own no output slice; (16, 144): three waves own no score slice (they write zero partials);
* the ascending and the descending probe over three key tiles and a bit, at 256 and at 512.

With N(0, 1) inputs the scores of a 512-wide head have a standard deviation of about 23 and the softmax is nearly
one-hot, so `SCALED` cases run again on a copy whose Q columns are multiplied by d^-1/2 (scores of N(0, 1), many
keys with weight), oracle and allowance recomputed on the copy by the same two helpers.

Cached per case: callers must not modify what they get.
"""
import functools
import types

import numpy as np
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.attention import (
    attention_wide_tiles)

import attention_cases as AC
import causal_attention_cases as CC

WQ2, WK2 = attention_wide_tiles(256, 256)
WQ5, WK5 = attention_wide_tiles(512, 512)

CASES = [
    (1, 1, 1, 256, 256, None), (1, WK2 - 1, 1, 256, 256, None), (1, WK2 + 1, 1, 256, 256, None),
    (1, WQ5 + 1, 1, 512, 512, None), (2, WQ5 + WK5 + 5, 1, 512, 512, None),
    (2, 37, 2, 160, 192, None), (1, 38, 3, 144, 16, None), (1, 38, 1, 16, 144, None),
    (1, 3 * WK2 + 6, 1, 256, 256, "ascending"), (1, 3 * WK5 + 6, 1, 512, 512, "descending"),
]
SCALED = [(2, 37, 2, 160, 192, None), (2, WQ5 + WK5 + 5, 1, 512, 512, None)]
GUARD_CASES = [(2, WQ5 + WK5 + 5, 1, 512, 512, None), (1, 38, 3, 144, 16, None), (1, 1, 1, 256, 256, None)]


@functools.lru_cache(maxsize=None)
def case(c, causal=False, bf16=False, scaled=False):
    """The case of AC / CC (`case` or `case_bf16`); `scaled`: a copy with Q multiplied by d^-1/2 (rounded to bf16
    again in bf16), its oracle and allowance from the same module's `ref_attention` and `f32_allowance`."""
    M = CC if causal else AC
    k = types.SimpleNamespace(**vars((M.case_bf16 if bf16 else M.case)(c)))
    if scaled:
        k.qkv = k.qkv.copy()
        k.qkv[:, :k.heads * k.d] *= np.float32(k.d ** -0.5)
        if bf16:
            k.qkv = torch.from_numpy(k.qkv).to(torch.bfloat16).float().numpy()
        k.want = M.ref_attention(k.qkv, k.B, k.T, k.heads, k.d, k.dv)
        k.e_ref, k.allow = M.f32_allowance(k.qkv, c, k.want)
    return k
