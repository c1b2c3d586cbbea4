"""Guard-band runs of the bf16-MFMA attention kernel (`math="bf16"`), in the form of tests/test_guard_attention_gpu.py:
guards intact, outputs finite, equal between the NaN and +inf poison runs and within the bound of
tests/test_attention_bf16_gpu.py.  Cases: tests/attention_bf16_cases.py `GUARD_CASES`.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import attention_bf16_cases as BC
import guardband as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c,causal", BC.GUARD_CASES, ids=str)
def test_guard_bf16_math_attention(c, causal):
    k = BC.case(c, causal)
    assert A.attention_kernel(k.d, k.dv, math="bf16") == "mfma_bf16"
    outs = {}
    for poison in (G.NAN, G.INF):
        xp = torch.full((k.B * k.T, k.ld_in), float(poison), dtype=torch.bfloat16)      # the pads hold the poison too
        xp[:, :k.w_in] = torch.from_numpy(k.qkv).to(torch.bfloat16)
        x = G.guarded(xp.shape, torch.bfloat16, "cuda", payload=xp, poison=poison, name="qkv")
        out = G.guarded((k.B * k.T, k.ld_out), torch.bfloat16, "cuda", payload=float("nan"), name="out")
        A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, causal=causal, math="bf16")
        torch.cuda.synchronize()
        G.check(x, out, what=f"[bf16 math attention {c} causal={causal}, {poison} poison]")
        outs[poison] = out.cpu()
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all() and torch.isfinite(b).all(), "output not finite under read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    got = a.float().numpy().astype(np.float64)
    assert (got[:, k.w_out:] == 0).all(), "padding channels must come out as exact zeros"
    assert (np.abs(got[:, :k.w_out] - k.want) <= BC.bound(k.want, k.pabsv, k.allow)).all()
