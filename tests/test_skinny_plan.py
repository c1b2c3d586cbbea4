"""The host side of the skinny GEMM (ops/conv.py) without a GPU: `skinny_plan` on the one-token GEMMs of
tinyllama_1_1b and llama2_7b (tools/skinny_bench.py's list), `skinny_scratch`, and `skinny_supported` on convs packed
on the CPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from skinny_bench import SHAPES, ROWS  # noqa: E402


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name,K,N", SHAPES, ids=[s[0] for s in SHAPES])
def test_skinny_plan_and_scratch(name, K, N, dtype):
    chunks = C.skinny_chunks(K, dtype)
    for M in ROWS:
        F, KS = C.skinny_plan(M, N, K, dtype)
        assert F in C.SKINNY_F and 1 <= KS <= chunks
        shortest = min((s + 1) * chunks // KS - s * chunks // KS for s in range(KS))
        assert shortest >= 4 or (KS == 1 and shortest >= 1)        # a chunk per wave in every split; none empty
        assert C.skinny_scratch(M, N, K, dtype, F, KS) == ((KS > 1) * KS * M * N, (KS > 1) * math.ceil(N / (16 * F)))
    assert C.skinny_scratch(8, N, K, dtype, 2, 1) == (0, 0)
    assert C.skinny_scratch(8, N, K, dtype, 2, 3) == (3 * 8 * N, math.ceil(N / 32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_skinny_supported(dtype):
    rng = np.random.default_rng(0)
    pack = C.pack_conv_f32 if dtype == torch.float32 else C.pack_conv

    def conv(kh, stride):
        pad = ((kh // 2, kh // 2), (kh // 2, kh // 2))
        return pack(rng.standard_normal((kh, kh, 64, 48)).astype(np.float32), np.zeros(48, np.float32), stride, pad, "cpu")

    pc = conv(1, 1)
    assert C.skinny_supported(pc, 1) and C.skinny_supported(pc, 32)
    assert not C.skinny_supported(pc, 33) and not C.skinny_supported(pc, 0)
    assert not C.skinny_supported(conv(3, 1), 8) and not C.skinny_supported(conv(1, 2), 8)
    pc.n_split = 16
    assert not C.skinny_supported(pc, 8)
