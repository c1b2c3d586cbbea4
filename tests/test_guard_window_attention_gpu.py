"""Guard-band runs of the window attention kernels (csrc/kernels/window_attention.hip) and the space-to-depth
kernels (csrc/kernels/resize.hip), as the other test_guard_*_gpu.py files do for theirs: `qkv`, the packed bias
and `out` between 1 MiB guards (tests/guardband.py).

Each case is launched twice, with NaN and with +inf in the guards of everything the kernel reads, the output
pre-filled with NaN.  Asserted: every guard intact bit for bit; outputs finite, bit-identical between the two
poison runs and within the bound of tests/test_window_attention_gpu.py.  Cases
(tests/window_attention_cases.py): the 49-token shifted one, one window, the non-square two-image one, 144 tokens,
and the plain kernel with padded widths.  The bf16 input's padding channels hold the read poison too.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E

import guardband as G
import window_attention_cases as WC

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)


def _same_and_finite(outs):
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    return a


def _bias(k, poison):
    b = A.window_bias(k.table, k.M, k.shift)
    return G.guarded(b.shape, torch.float32, "cuda", payload=b, poison=poison, name="bias")


@pytest.mark.parametrize("c", WC.GUARD_CASES, ids=str)
def test_guard_window_attention_f32(c):
    k = WC.case(c)
    outs = {}
    for poison in POISONS:
        x = G.guarded(k.qkv.shape, torch.float32, "cuda", payload=k.qkv, poison=poison, name="qkv")
        bias = _bias(k, poison)
        out = G.guarded(k.want.shape, torch.float32, "cuda", payload=float("nan"), name="out")
        A.window_attention(x, bias, out, k.B, k.H, k.W, k.M, k.shift, k.heads, k.d)
        torch.cuda.synchronize()
        G.check(x, bias, out, what=f"[window_attention_f32 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    a = _same_and_finite(outs)
    assert np.abs(a.numpy().astype(np.float64) - k.want).max() <= k.allow


@pytest.mark.parametrize("c", WC.GUARD_CASES, ids=str)
def test_guard_window_attention_bf16(c):
    k = WC.case_bf16(c)
    outs = {}
    for poison in POISONS:
        xp = torch.full((k.rows, k.ld_in), float(poison), dtype=torch.bfloat16)        # the pads hold the poison too
        xp[:, :k.w_in] = torch.from_numpy(k.qkv).to(torch.bfloat16)
        x = G.guarded(xp.shape, torch.bfloat16, "cuda", payload=xp, poison=poison, name="qkv")
        bias = _bias(k, poison)
        out = G.guarded((k.rows, k.ld_out), torch.bfloat16, "cuda", payload=float("nan"), name="out")
        A.window_attention(x, bias, out, k.B, k.H, k.W, k.M, k.shift, k.heads, k.d)
        torch.cuda.synchronize()
        G.check(x, bias, out, what=f"[window_attention bf16 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs).float().numpy().astype(np.float64)
    assert (got[:, k.w_out:] == 0).all(), "padding channels must come out as exact zeros"
    assert (np.abs(got[:, :k.w_out] - k.want) <= 2.0 ** -8 * np.abs(k.want) + k.allow).all()


@pytest.mark.parametrize("C", [6, 32])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_space_to_depth(C, dtype):
    c = (2, 4, 6, C)
    B, H, W, _ = c
    bf = dtype == torch.bfloat16
    Cpx, Cpy = ((C + 7) // 8 * 8, (4 * C + 7) // 8 * 8) if bf else (C, 4 * C)
    xv = torch.from_numpy(WC.s2d_case(c)).to(dtype)
    want = WC.ref_space_to_depth(xv.float().numpy())
    outs = {}
    for poison in POISONS:
        xp = torch.full((B, H, W, Cpx), float(poison), dtype=dtype)                    # bf16 pads hold the poison
        xp[..., :C] = xv
        x = G.guarded(xp.shape, dtype, "cuda", payload=xp, poison=poison, name="x")
        out = G.guarded((B, H // 2, W // 2, Cpy), dtype, "cuda", payload=float("nan"), name="out")
        E.space_to_depth(x, out, C=C)
        torch.cuda.synchronize()
        G.check(x, out, what=f"[space_to_depth {c} {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs).float().numpy()
    np.testing.assert_array_equal(got[..., :4 * C], want)
    assert (got[..., 4 * C:] == 0).all()
