"""Guard-band runs of the LayerNormalization kernels (csrc/kernels/layernorm.hip), as the other
test_guard_*_gpu.py files do for theirs: x, gamma, beta and the output between 1 MiB guards (tests/guardband.py).

Each case is launched twice, with NaN and with +inf in the guards of everything the kernel reads, the output
pre-filled with NaN.  Asserted: every guard intact bit for bit; outputs finite, bit-identical between the two
poison runs and within the bound of tests/test_layernorm_gpu.py.  Cases (tests/layernorm_cases.py): C % 4 != 0 (the
fp32 looped path; one bf16 vector with two padding channels), rows that end inside a wave and inside a block with
C % 8 == 4, several rows per wave with a ragged tail, and the looped path with an odd C on both kernels.  The bf16
input's padding channels hold the read poison too.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E

import guardband as G
import layernorm_cases as LC

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)


@pytest.mark.parametrize("c", LC.GUARD_CASES, ids=str)
def test_guard_layernorm_f32(c):
    k = LC.case(c)
    outs = {}
    for poison in POISONS:
        x = G.guarded(k.x.shape, torch.float32, "cuda", payload=k.x, poison=poison, name="x")
        gm = G.guarded(k.C, torch.float32, "cuda", payload=k.gamma_k, poison=poison, name="gamma")
        bt = G.guarded(k.C, torch.float32, "cuda", payload=k.beta_k, poison=poison, name="beta")
        out = G.guarded(k.x.shape, torch.float32, "cuda", payload=float("nan"), name="out")
        E.layernorm_f32(x, gm, bt, out, k.eps)
        torch.cuda.synchronize()
        G.check(x, gm, bt, out, what=f"[layernorm_f32 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    assert np.abs(a.numpy().astype(np.float64) - k.want).max() <= k.allow


@pytest.mark.parametrize("c", LC.GUARD_CASES, ids=str)
def test_guard_layernorm_bf16(c):
    k = LC.case_bf16(c)
    outs = {}
    for poison in POISONS:
        xp = torch.full((k.rows, k.Cp), float(poison), dtype=torch.bfloat16)      # the pads hold the poison too
        xp[:, :k.C] = torch.from_numpy(k.x).to(torch.bfloat16)
        x = G.guarded(xp.shape, torch.bfloat16, "cuda", payload=xp, poison=poison, name="x")
        gm = G.guarded(k.Cp, torch.float32, "cuda", payload=k.gamma_p, poison=poison, name="gamma")
        bt = G.guarded(k.Cp, torch.float32, "cuda", payload=k.beta_p, poison=poison, name="beta")
        out = G.guarded(xp.shape, torch.bfloat16, "cuda", payload=float("nan"), name="out")
        E.layernorm(x, gm, bt, out, k.C, k.eps)
        torch.cuda.synchronize()
        G.check(x, gm, bt, out, what=f"[layernorm bf16 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    got = a.float().numpy().astype(np.float64)
    assert (got[:, k.C:] == 0).all(), "padding channels must come out as exact zeros"
    assert (np.abs(got[:, :k.C] - k.want) <= 2.0 ** -8 * np.abs(k.want) + k.allow).all()
