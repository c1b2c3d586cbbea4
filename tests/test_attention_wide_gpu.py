"""The head-split attention kernel for wide heads (csrc/kernels/attention_wide.h) on the GPU, through
`ops.attention.attention`, against the float64 oracles and the allowance of tests/attention_cases.py and
tests/causal_attention_cases.py: ``max(4 e_ref, 2e-5 max(1, max|want|))``, bf16 ``2^-8 |want| + allowance``.

Every case of tests/attention_wide_cases.py runs plain and causal, in fp32 and in bf16 (padded row strides, the pads
of the input hold NaN), with the output pre-filled with NaN: all finite, within the bound, padding channels exact
zeros.  Two cases run again with Q scaled by d^-1/2.  An fp32 emulation of the kernel's summation order (four slice
groups added in wave order, 16-key online softmax) sat at 0.05 - 0.16 of the allowance on these cases (e_ref 0 to
3.0e-5, allowance 6.5e-5 to 1.2e-4) and at 0.02 of 2.9e-5 on the scaled copies.

Then: grouped-query rows on the wide kernel, bit-equal to the multi-head launch on the expanded rows; a row stride
of width + 1 and the padding-mask entry point, both on the plain kernel at these head sizes and right as before;
and `vae_decoder_wide_micro` captured and replayed against the fp32 CPU oracle in the form and with the budgets of
tests/test_groupnorm_gpu.py.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import attention_wide_cases as WC
import llama_cases as LC
import padding_mask_cases as PC

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
CAUSAL = pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])


def _rows(a, dtype, ld):
    """`a` as device rows of stride `ld`; the channels beyond its width hold NaN."""
    x = torch.full((a.shape[0], ld), float("nan"), dtype=dtype)
    x[:, :a.shape[1]] = torch.from_numpy(a).to(dtype)
    return x.cuda()


def _pad(w, dtype, extra=0):
    return (w + 7) // 8 * 8 if dtype == torch.bfloat16 else w + extra


def _check(out, want, allow, dtype, what):
    got = out.float().cpu().numpy().astype(np.float64)
    w = want.shape[1]
    assert np.isfinite(got).all(), what
    assert (got[:, w:] == 0).all(), f"{what}: padding channels must come out as exact zeros"
    err = np.abs(got[:, :w] - want)
    bound = allow + (2.0 ** -8 * np.abs(want) if dtype == torch.bfloat16 else 0.0)
    print(f"{what}: max err {err.max():.3e}, allowance {allow:.3e}, worst err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), what


@DTYPES
@CAUSAL
@pytest.mark.parametrize("c,scaled", [(c, False) for c in WC.CASES] + [(c, True) for c in WC.SCALED], ids=str)
def test_wide_attention(c, scaled, causal, dtype):
    k = WC.case(c, causal, dtype == torch.bfloat16, scaled)
    assert A.attention_kernel(k.d, k.dv) == "wide"
    w_in, w_out = WC.AC.widths(c)
    out = torch.full((k.B * k.T, _pad(w_out, dtype)), float("nan"), dtype=dtype, device="cuda")
    A.attention(_rows(k.qkv, dtype, _pad(w_in, dtype)), out, k.B, k.T, k.heads, k.d, k.dv, causal=causal)
    torch.cuda.synchronize()
    _check(out, k.want, k.allow, dtype, f"wide attention {c} scaled={scaled} causal={causal} {dtype}")


@DTYPES
@CAUSAL
@pytest.mark.parametrize("c", [(2, WC.WK2 + 1, 4, 1, 256, 256, "ascending"), (2, WC.WQ2 + 1, 4, 2, 160, 160, "dominant")],
                         ids=str)
def test_wide_gqa_attention(c, causal, dtype):
    B, T, hq, hkv, d, dv, probe = c
    x = LC.gqa_inputs(c, bf16=dtype == torch.bfloat16)
    want = LC.gqa_oracle(x, c, causal)
    e_ref = float(np.abs(LC.gqa_library(x, c, causal) - want).max())
    out = torch.full((B * T, _pad(hq * dv, dtype)), float("nan"), dtype=dtype, device="cuda")
    A.attention(_rows(x, dtype, _pad(x.shape[1], dtype)), out, B, T, hq, d, dv, causal=causal, kv_heads=hkv)
    xe = LC.gqa_expanded(x, c)
    full = torch.full_like(out, float("nan"))
    A.attention(_rows(xe, dtype, _pad(xe.shape[1], dtype)), full, B, T, hq, d, dv, causal=causal)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().astype(np.float64)
    assert (got[:, hq * dv:] == 0).all()
    err = np.abs(got[:, :hq * dv] - want)
    allow = LC.allowance(want, e_ref, bf16=dtype == torch.bfloat16)
    print(f"wide gqa {c} causal={causal} {dtype}: e_ref {e_ref:.3e} err {err.max():.3e} allowance {np.max(allow):.3e}")
    assert (err <= allow).all()
    assert torch.equal(out, full), "a GQA launch must equal the plain launch on the expanded rows bit for bit"


@CAUSAL
def test_a_row_stride_off_the_vector_grid_takes_the_plain_kernel_and_is_right(causal):
    c = (2, 37, 2, 160, 192, None)
    k = WC.case(c, causal)
    w_in, w_out = WC.AC.widths(c)
    out = torch.full((k.B * k.T, w_out + 1), float("nan"), device="cuda")
    A.attention(_rows(k.qkv, torch.float32, w_in + 1), out, k.B, k.T, k.heads, k.d, k.dv, causal=causal)
    torch.cuda.synchronize()
    _check(out, k.want, k.allow, torch.float32, f"row stride width + 1 {c} causal={causal}")


@DTYPES
def test_the_padding_mask_at_a_wide_head_takes_the_plain_kernel_and_is_right(dtype):
    k = PC.case((256, 33)) if dtype == torch.float32 else PC.case_bf16((256, 33))
    w_in, w_out = k.heads * (2 * k.d + k.dv), k.heads * k.dv
    x = _rows(k.qkv, dtype, w_in + 8)
    for gr in k.groups:
        out = torch.full((k.B * k.T, w_out + 8), float("nan"), dtype=dtype, device="cuda")
        A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, key_mask=torch.from_numpy(gr.mask).cuda())
        torch.cuda.synchronize()
        _check(out, gr.want, gr.allow, dtype, f"padding mask at (256, 256) {gr.group} {dtype}")


@pytest.fixture(scope="module")
def wide_micro():
    g = build_model("vae_decoder_wide_micro")
    w = init_weights(g, seed=0)
    x = (np.random.default_rng(3).standard_normal((4, 8, 8, 4)) * 0.18215 * 4.0).astype(np.float32)
    want = ReferenceExecutor(g, w, device="cpu")(torch.from_numpy(x)).double().numpy()
    return g, w, x, want


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_vae_decoder_wide_micro_matches_oracle_captured_and_replayed(wide_micro, precision, budget):
    g, w, x, want = wide_micro
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    attn = [st for st in ex.steps if st.kind == "attention"]
    assert len(attn) == 1 and A.attention_kernel(g.layers["mid_attn"].attrs["key_dim"], 160) == "wide"
    ex.capture()
    assert ex.captured
    seen = []
    for half in (slice(0, 2), slice(2, 4)):
        out = ex(torch.from_numpy(x[half]).cuda())
        torch.cuda.synchronize()
        got = out.double().cpu().numpy()
        assert got.shape == (2, 64, 64, 3 if precision == "fp32" else 8) and np.isfinite(got).all()
        rel = np.abs(got[..., :3] - want[half]).max() / np.abs(want[half]).max()
        print(f"vae_decoder_wide_micro {precision} rel err {rel:.3e}")
        assert rel <= budget, f"vae_decoder_wide_micro {precision} rel err {rel}"
        seen.append(got[..., :3])
    # the two inputs' outputs are further apart than the budget, so a stale replay could not have passed above
    assert np.abs(seen[0] - seen[1]).max() > 2 * budget * np.abs(want).max(), "the replay returned the first input's result"
