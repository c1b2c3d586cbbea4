"""Guard-band runs of the attention kernels (csrc/kernels/attention.hip) and the position-embedding kernel, as the
other test_guard_*_gpu.py files do for theirs: `qkv` and `out` between 1 MiB guards (tests/guardband.py).

Each case is launched twice, with NaN and with +inf in the guards of everything the kernel reads, the output
pre-filled with NaN.  Asserted: every guard intact bit for bit; outputs finite, bit-identical between the two
poison runs and within the bound of tests/test_attention_gpu.py.  Cases (tests/attention_cases.py): T off the key
tile with two images, T = 1, the plain kernel with padded widths, 197 tokens, and three images with T off both
tiles.  The bf16 input's padding channels hold the read poison too.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import attention_cases as AC
import guardband as G

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)


def _same_and_finite(outs):
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    return a


@pytest.mark.parametrize("c", AC.GUARD_CASES, ids=str)
def test_guard_attention_f32(c):
    k = AC.case(c)
    outs = {}
    for poison in POISONS:
        x = G.guarded(k.qkv.shape, torch.float32, "cuda", payload=k.qkv, poison=poison, name="qkv")
        out = G.guarded(k.want.shape, torch.float32, "cuda", payload=float("nan"), name="out")
        A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv)
        torch.cuda.synchronize()
        G.check(x, out, what=f"[attention_f32 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    a = _same_and_finite(outs)
    assert np.abs(a.numpy().astype(np.float64) - k.want).max() <= k.allow


@pytest.mark.parametrize("c", AC.GUARD_CASES, ids=str)
def test_guard_attention_bf16(c):
    k = AC.case_bf16(c)
    outs = {}
    for poison in POISONS:
        xp = torch.full((k.B * k.T, k.ld_in), float(poison), dtype=torch.bfloat16)     # the pads hold the poison too
        xp[:, :k.w_in] = torch.from_numpy(k.qkv).to(torch.bfloat16)
        x = G.guarded(xp.shape, torch.bfloat16, "cuda", payload=xp, poison=poison, name="qkv")
        out = G.guarded((k.B * k.T, k.ld_out), torch.bfloat16, "cuda", payload=float("nan"), name="out")
        A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv)
        torch.cuda.synchronize()
        G.check(x, out, what=f"[attention bf16 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs).float().numpy().astype(np.float64)
    assert (got[:, k.w_out:] == 0).all(), "padding channels must come out as exact zeros"
    assert (np.abs(got[:, :k.w_out] - k.want) <= 2.0 ** -8 * np.abs(k.want) + k.allow).all()


@pytest.mark.parametrize("c", AC.POSEMBED_CASES[:3], ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_posembed(c, dtype):
    k = AC.posembed_case(c)
    bf = dtype == torch.bfloat16
    Cs = k.Cp if bf else k.C
    xv = torch.from_numpy(k.x).to(dtype)
    want = AC.ref_posembed(xv.float().numpy().astype(np.float64), None if k.cls is None else k.cls.astype(np.float64),
                           k.pos.astype(np.float64))
    outs = {}
    for poison in POISONS:
        xp = torch.full(k.x.shape[:3] + (Cs,), float(poison), dtype=dtype)             # bf16 pads hold the poison
        xp[..., :k.C] = xv
        x = G.guarded(xp.shape, dtype, "cuda", payload=xp, poison=poison, name="x")
        cls = None if k.cls is None else G.guarded(k.C, torch.float32, "cuda", payload=k.cls, poison=poison, name="cls")
        pos = G.guarded(k.pos.shape, torch.float32, "cuda", payload=k.pos, poison=poison, name="pos")
        out = G.guarded((k.B, 1, k.T + k.ct, Cs), dtype, "cuda", payload=float("nan"), name="out")
        A.posembed(x, cls, pos, out, C=k.C)
        torch.cuda.synchronize()
        G.check(x, cls, pos, out, what=f"[posembed {c} {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs).float().numpy().astype(np.float64)
    assert (got[..., k.C:] == 0).all()
    if bf:
        assert (np.abs(got[..., :k.C] - want) <= 2.0 ** -8 * np.abs(want) + 1e-30).all()
    else:
        np.testing.assert_array_equal(got[..., :k.C], AC.ref_posembed(k.x, k.cls, k.pos).astype(np.float64))
