"""The causal instantiations of the attention kernels (csrc/kernels/attention_core.h, attention.hip) on the GPU,
against the causal float64 oracle and the allowance of tests/causal_attention_cases.py.

Every case runs in fp32 and in bf16 with the output pre-filled with NaN: all finite, within the allowance (bf16:
2^-8 |want| + allowance), the bf16 layout's padding channels exact zeros whatever the input's padding holds.  Under
the mask query 0 attends key 0 alone (p = 1, l = 1), so in fp32 its row reproduces V's row 0 bit for bit on both
paths; row q agrees with an unmasked launch over the first q + 1 tokens; and `causal=False` is the launch as it
was.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import attention_cases as AC
import causal_attention_cases as CC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", CC.CASES, ids=str)
def test_causal_attention_f32(c):
    k = CC.case(c)
    out = torch.full(k.want.shape, float("nan"), dtype=torch.float32, device="cuda")
    A.attention(torch.from_numpy(k.qkv).cuda(), out, k.B, k.T, k.heads, k.d, k.dv, causal=True)
    torch.cuda.synchronize()
    got32 = out.cpu().numpy()
    got = got32.astype(np.float64)
    err = np.abs(got - k.want).max()
    print(f"causal attention fp32 {c} [{k.path}]: e_ref {k.e_ref:.3e}, max err {err:.3e}, allowance {k.allow:.3e}")
    assert np.isfinite(got).all() and err <= k.allow
    v0 = AC.split(k.qkv, k.B, k.T, k.heads, k.d, k.dv)[2][:, 0].reshape(k.B, -1)
    np.testing.assert_array_equal(got32.reshape(k.B, k.T, -1)[:, 0], v0)


@pytest.mark.parametrize("c", CC.CASES, ids=str)
def test_causal_attention_bf16(c):
    k = CC.case_bf16(c)
    x = torch.full((k.B * k.T, k.ld_in), float("nan"), dtype=torch.bfloat16)
    x[:, :k.w_in] = torch.from_numpy(k.qkv).to(torch.bfloat16)
    out = torch.full((k.B * k.T, k.ld_out), float("nan"), dtype=torch.bfloat16, device="cuda")
    A.attention(x.cuda(), out, k.B, k.T, k.heads, k.d, k.dv, causal=True)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[:, k.w_out:] == 0).all(), "padding channels must come out as exact zeros"
    over = np.abs(got[:, :k.w_out] - k.want) - (2.0 ** -8 * np.abs(k.want) + k.allow)
    print(f"causal attention bf16 {c} [{k.path}]: max err {np.abs(got[:, :k.w_out] - k.want).max():.3e}, "
          f"worst excess {over.max():.3e}")
    assert (over <= 0).all()


def test_a_causal_row_is_the_unmasked_launch_over_its_prefix():
    c = (1, 197, 2, 64, 64, None)
    k = CC.case(c)
    x = torch.from_numpy(k.qkv).cuda()
    out = torch.full(k.want.shape, float("nan"), dtype=torch.float32, device="cuda")
    A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, causal=True)
    for q in (0, CC.KT - 1, CC.KT, k.T - 1):
        part = torch.full((q + 1, k.want.shape[1]), float("nan"), dtype=torch.float32, device="cuda")
        A.attention(x[:q + 1].contiguous(), part, 1, q + 1, k.heads, k.d, k.dv)
        torch.cuda.synchronize()
        err = (out[q].double() - part[q].double()).abs().max().item()
        print(f"row {q}: causal vs unmasked prefix {err:.3e}, allowance {k.allow:.3e}")
        assert err <= k.allow


@pytest.mark.parametrize("c", [(1, 197, 2, 64, 64, None), (2, 19, 3, 6, 5, None)], ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_causal_false_is_the_launch_as_it_was(c, dtype):
    k = AC.case(c)
    x = torch.from_numpy(k.qkv).to(dtype)
    if dtype == torch.bfloat16:
        kb = AC.case_bf16(c)
        xp = torch.zeros((k.B * k.T, kb.ld_in), dtype=dtype)
        xp[:, :kb.w_in] = x
        x, shape = xp, (k.B * k.T, kb.ld_out)
    else:
        shape = k.want.shape
    x = x.cuda()
    a = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    b = torch.full(shape, float("nan"), dtype=dtype, device="cuda")
    A.attention(x, a, k.B, k.T, k.heads, k.d, k.dv)
    A.attention(x, b, k.B, k.T, k.heads, k.d, k.dv, causal=False)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
