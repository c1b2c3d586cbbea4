"""Guard-band runs of the head-split attention kernel for wide heads (csrc/kernels/attention_wide.h), in the form of
tests/test_guard_attention_gpu.py: `qkv` and `out` between 1 MiB guards (tests/guardband.py), each case launched
with NaN and with +inf in the guards and, in bf16, in the input's padding channels, the output pre-filled with NaN.
Asserted: every guard intact bit for bit; outputs finite, bit-identical between the two poison runs and within the
bound of tests/test_attention_wide_gpu.py.  Cases: two images off both tiles at 512, three heads of (144, 16) (three
waves without an output slice), and one token at 256.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import attention_wide_cases as WC
import guardband as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", WC.GUARD_CASES, ids=str)
def test_guard_wide_attention(c, dtype):
    bf16 = dtype == torch.bfloat16
    k = WC.case(c, False, bf16)
    w_in, w_out = WC.AC.widths(c)
    ld_in, ld_out = ((w_in + 7) // 8 * 8, (w_out + 7) // 8 * 8) if bf16 else (w_in, w_out)
    outs = {}
    for poison in (G.NAN, G.INF):
        xp = torch.full((k.B * k.T, ld_in), float(poison), dtype=dtype)                # the pads hold the poison too
        xp[:, :w_in] = torch.from_numpy(k.qkv).to(dtype)
        x = G.guarded(xp.shape, dtype, "cuda", payload=xp, poison=poison, name="qkv")
        out = G.guarded((k.B * k.T, ld_out), dtype, "cuda", payload=float("nan"), name="out")
        A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv)
        torch.cuda.synchronize()
        G.check(x, out, what=f"[wide attention {dtype} {c}, {poison} poison]")
        outs[poison] = out.cpu()
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all() and torch.isfinite(b).all(), "output not finite under read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    got = a.float().numpy().astype(np.float64)
    assert (got[:, w_out:] == 0).all(), "padding channels must come out as exact zeros"
    bound = k.allow + (2.0 ** -8 * np.abs(k.want) if bf16 else 0.0)
    assert (np.abs(got[:, :w_out] - k.want) <= bound).all()
