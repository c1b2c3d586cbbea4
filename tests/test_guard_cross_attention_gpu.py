"""Guard-band runs of the cross-attention kernels (csrc/kernels/cross_attention.hip) and the learned-queries kernel,
as tests/test_guard_attention_gpu.py does for self-attention: every buffer the kernel reads and `out` between 1 MiB
guards (tests/guardband.py).

Each case is launched twice, with NaN and with +inf in the guards and in the surplus of every row of what the kernel
reads, the output pre-filled with NaN.  Asserted: every guard intact bit for bit; outputs finite, bit-identical
between the two poison runs and within the bound of tests/test_cross_attention_gpu.py.  Cases
(tests/cross_attention_cases.py): Tk = 1 in three buffers, two images with both lengths off both tiles and [K | V]
side by side, [Q | K] side by side on the MFMA path and on the plain kernel, and the plain kernel on three buffers
with odd strides.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import cross_attention_cases as XC
import guardband as G

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)


def _same_and_finite(outs):
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    return a


def _run(k, dtype, ld_out):
    outs = {}
    for poison in POISONS:
        make = lambda t, name: G.guarded(t.shape, dtype, "cuda", payload=t, poison=poison, name=name)  # noqa: E731
        q, kk, v, bufs = XC.views(k, make, fill=float(poison), dtype=dtype)     # the rows' surplus holds the poison too
        out = G.guarded((k.B * k.Tq, ld_out), dtype, "cuda", payload=float("nan"), name="out")
        assert A.cross_attention_path(q, kk, v, out, k.d, k.dv) == k.path
        A.cross_attention(q, kk, v, out, k.B, k.Tq, k.Tk, k.heads, k.d, k.dv)
        torch.cuda.synchronize()
        G.check(*bufs, out, what=f"[cross_attention {dtype} {k.case}, {poison} poison]")
        outs[poison] = out.cpu()
    return _same_and_finite(outs)


@pytest.mark.parametrize("c", XC.GUARD_CASES, ids=str)
def test_guard_cross_attention_f32(c):
    k = XC.case(c)
    a = _run(k, torch.float32, k.w_out)
    assert np.abs(a.numpy().astype(np.float64) - k.want).max() <= k.allow


@pytest.mark.parametrize("c", XC.GUARD_CASES, ids=str)
def test_guard_cross_attention_bf16(c):
    k = XC.case_bf16(c)
    got = _run(k, torch.bfloat16, (k.w_out + 7) // 8 * 8).float().numpy().astype(np.float64)
    assert (got[:, k.w_out:] == 0).all(), "padding channels must come out as exact zeros"
    assert (np.abs(got[:, :k.w_out] - k.want) <= 2.0 ** -8 * np.abs(k.want) + k.allow).all()


@pytest.mark.parametrize("c", [(2, 5, 64), (3, 7, 20), (1, 1, 6)], ids=str)              # B, N, C
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_queries(c, dtype):
    B, N, C = c
    Cs = (C + 7) // 8 * 8 if dtype == torch.bfloat16 else C
    table = np.random.default_rng(N * C).standard_normal((N, C)).astype(np.float32)
    outs = {}
    for poison in POISONS:
        emb = G.guarded(table.shape, torch.float32, "cuda", payload=table, poison=poison, name="emb")
        out = G.guarded((B, 1, N, Cs), dtype, "cuda", payload=float("nan"), name="out")
        A.queries(emb, out, C=C)
        torch.cuda.synchronize()
        G.check(emb, out, what=f"[queries {c} {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs)
    assert (got[..., C:] == 0).all()
    assert torch.equal(got[..., :C], torch.from_numpy(table).to(dtype).expand(B, 1, N, C))
