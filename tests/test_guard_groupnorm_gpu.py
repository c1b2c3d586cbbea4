"""Guard-band runs of the GroupNormalization kernels (csrc/kernels/groupnorm.hip), as the other
test_guard_*_gpu.py files do for theirs: x, gamma, beta, the output and the workspace between 1 MiB guards
(tests/guardband.py).

Each case is launched twice, with NaN and with +inf in the guards of everything the kernel reads, the output and
the exactly sized workspace pre-filled with NaN (a partial read before it was written would show).  Asserted: every
guard intact bit for bit; outputs finite, bit-identical between the two poison runs and within the bound of
tests/test_groupnorm_gpu.py.  Cases (tests/groupnorm_cases.py): C % 4 != 0 (the fp32 scalar path; one bf16 vector
with two padding channels, single launch); the vector that straddles two groups with C % 8 == 4; the odd pixel
count on the split path; and the split path with several slabs.  The bf16 input's padding channels hold the read
poison too.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E

import guardband as G
import groupnorm_cases as GN

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)


def _workspace(k, bf16):
    """The workspace exactly as large as the host function says, or None where the single launch needs none."""
    need = E.groupnorm_workspace(k.B, k.H * k.W, k.C, k.groups, bf16)
    return G.guarded(need, torch.float32, "cuda", payload=float("nan"), name="workspace") if need else None


def test_the_guard_cases_reach_the_split_path_with_a_workspace():
    for bf16 in (False, True):
        paths = [E.groupnorm_path(c[0], c[1] * c[2], c[3], c[4], bf16) for c in GN.GUARD_CASES]
        assert paths == ([2, 2, 1, 1] if bf16 else [0, 2, 1, 1])
        assert E.groupnorm_slabs(1, 96 * 96, 8, 2, bf16) > 1
        assert [E.groupnorm_workspace(c[0], c[1] * c[2], c[3], c[4], bf16) > 0 for c in GN.GUARD_CASES] == \
            [not bf16, False, True, True]


@pytest.mark.parametrize("c", GN.GUARD_CASES, ids=str)
def test_guard_groupnorm_f32(c):
    k = GN.case(c)
    outs = {}
    for poison in POISONS:
        x = G.guarded(k.x.shape, torch.float32, "cuda", payload=k.x, poison=poison, name="x")
        gm = G.guarded(k.C, torch.float32, "cuda", payload=k.gamma_k, poison=poison, name="gamma")
        bt = G.guarded(k.C, torch.float32, "cuda", payload=k.beta_k, poison=poison, name="beta")
        out = G.guarded(k.x.shape, torch.float32, "cuda", payload=float("nan"), name="out")
        ws = _workspace(k, False)
        E.groupnorm_f32(x, gm, bt, out, k.groups, k.eps, act=k.act_mode, workspace=ws)
        torch.cuda.synchronize()
        G.check(x, gm, bt, out, ws, what=f"[groupnorm_f32 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    assert np.abs(a.numpy().astype(np.float64) - k.want).max() <= k.allow


@pytest.mark.parametrize("c", GN.GUARD_CASES, ids=str)
def test_guard_groupnorm_bf16(c):
    k = GN.case_bf16(c)
    outs = {}
    for poison in POISONS:
        xp = torch.full((k.B, k.H, k.W, k.Cp), float(poison), dtype=torch.bfloat16)    # the pads hold the poison too
        xp[..., :k.C] = torch.from_numpy(k.x).to(torch.bfloat16)
        x = G.guarded(xp.shape, torch.bfloat16, "cuda", payload=xp, poison=poison, name="x")
        gm = G.guarded(k.Cp, torch.float32, "cuda", payload=k.gamma_p, poison=poison, name="gamma")
        bt = G.guarded(k.Cp, torch.float32, "cuda", payload=k.beta_p, poison=poison, name="beta")
        out = G.guarded(xp.shape, torch.bfloat16, "cuda", payload=float("nan"), name="out")
        ws = _workspace(k, True)
        E.groupnorm(x, gm, bt, out, k.C, k.groups, k.eps, act=k.act_mode, workspace=ws)
        torch.cuda.synchronize()
        G.check(x, gm, bt, out, ws, what=f"[groupnorm bf16 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    got = a.float().numpy().astype(np.float64)
    assert (got[..., k.C:] == 0).all(), "padding channels must come out as exact zeros"
    assert (np.abs(got[..., :k.C] - k.want) <= 2.0 ** -8 * np.abs(k.want) + k.allow).all()
