"""Guard-band runs of the padding-mask attention kernels, as tests/test_guard_causal_gpu.py does for the causal
ones: the input, the mask and the output each between 1 MiB guards (tests/guardband.py).

The shapes of tests/padding_mask_cases.py with T in {1, 33, 65}, every head size (both paths), every group of
patterns.  Each launch runs twice, with NaN and with +inf in the guards of everything the kernel reads (a NaN or an
infinity read as a mask value counts as a kept token, so an over-read of the mask moves the key bound or a row),
the output pre-filled with NaN.  Asserted: every guard intact bit for bit; outputs finite, bit-identical between
the two poison runs and within the bound of tests/test_padding_mask_gpu.py.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import guardband as G
import padding_mask_cases as PC

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)


@pytest.mark.parametrize("c", PC.GUARD_CASES, ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_masked_attention(c, dtype):
    k = PC.case(c) if dtype == torch.float32 else PC.case_bf16(c)
    w = k.heads * k.dv
    payload = torch.from_numpy(k.qkv).to(dtype)
    for gr in k.groups:
        outs = {}
        for poison in POISONS:
            x = G.guarded(payload.shape, dtype, "cuda", payload=payload, poison=poison, name="qkv")
            m = G.guarded(gr.mask.shape, torch.float32, "cuda", payload=gr.mask, poison=poison, name="mask")
            out = G.guarded((k.B * k.T, w), dtype, "cuda", payload=float("nan"), name="out")
            A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, key_mask=m)
            torch.cuda.synchronize()
            G.check(x, m, out, what=f"[masked attention {dtype} {c} {gr.group}, {poison} poison]")
            outs[poison] = out.cpu()
        a, b = outs[G.NAN], outs[G.INF]
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
        got = a.float().numpy().astype(np.float64)
        bound = gr.allow if dtype == torch.float32 else 2.0 ** -8 * np.abs(gr.want) + gr.allow
        assert (np.abs(got - gr.want) <= bound).all()
        assert (got[~gr.rows] == 0).all()
