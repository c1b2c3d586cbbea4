"""The bf16-MFMA attention kernel (csrc/kernels/attention_bf16.h) on the GPU, through
`ops.attention.attention(..., math="bf16")`, against the float64 oracles of tests/attention_cases.py and
tests/causal_attention_cases.py on the bf16-rounded inputs.

Bound, elementwise: ``err <= 2^-8 |want| + 2^-8 (P|V|) + allowance``.  `P|V|` is the oracle's softmax applied to |V|
and `allowance` the existing ``max(4 e_ref, 2e-5 max(1, max|want|))`` from the library's fp32 path on the CPU.
Derivation: one rounding of the output is 2^-9 |want| relative, bounded by 2^-8 |want|.  Each probability is rounded
to bf16 once, off by at most 2^-9 relative; that is scale-free, so the online rescale does not matter, and gives
2^-9 P|V| in the numerator (and 2^-9 |want| more where the row sum is taken from the rounded values; this kernel sums
the unrounded ones).  A CPU emulation of the scheme (32-key online softmax, P rounded to bf16, either choice of sum)
sat at 0.46 to 0.75 of this bound on these generators at comparable shapes, plain and causal.

Every case runs plain and causal with NaN in the row pads and in the output before the launch.  Then grouped-query
rows (bit-equal to the expanded multi-head launch), the three fall-backs by the existing bf16 bound, and `llama_micro`
and `vit_micro` with the switch, captured and replayed, within the budget of their existing bf16 tests.
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

import attention_bf16_cases as BC
import attention_wide_cases as WC
import llama_cases as LC
import padding_mask_cases as PC

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
CAUSAL = pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])


def _rows(a, ld):
    """`a` as bf16 device rows of stride `ld`; the channels beyond its width hold NaN."""
    x = torch.full((a.shape[0], ld), float("nan"), dtype=BF)
    x[:, :a.shape[1]] = torch.from_numpy(a).to(BF)
    return x.cuda()


def _check(out, want, bound, what):
    got = out.float().cpu().numpy().astype(np.float64)
    w = want.shape[1]
    assert np.isfinite(got).all(), what
    assert (got[:, w:] == 0).all(), f"{what}: padding channels must come out as exact zeros"
    err = np.abs(got[:, :w] - want)
    print(f"{what}: max err {err.max():.3e}, worst err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), what


@CAUSAL
@pytest.mark.parametrize("c,scaled", [(c, False) for c in BC.CASES] + [(c, True) for c in BC.SCALED], ids=str)
def test_bf16_math_attention(c, scaled, causal):
    k = BC.case(c, causal, scaled)
    assert A.attention_kernel(k.d, k.dv, math="bf16") == "mfma_bf16"
    out = torch.full((k.B * k.T, k.ld_out + 8), float("nan"), dtype=BF, device="cuda")
    A.attention(_rows(k.qkv, k.ld_in + 8), out, k.B, k.T, k.heads, k.d, k.dv, causal=causal, math="bf16")
    torch.cuda.synchronize()
    _check(out, k.want, BC.bound(k.want, k.pabsv, k.allow), f"bf16 math {c} scaled={scaled} causal={causal}")


@CAUSAL
@pytest.mark.parametrize("c", BC.GQA_CASES, ids=str)
def test_bf16_math_gqa_attention(c, causal):
    B, T, hq, hkv, d, dv, probe = c
    x = LC.gqa_inputs(c, bf16=True)
    want = LC.gqa_oracle(x, c, causal)
    xa = x.copy()
    xa[:, (hq + hkv) * d:] = np.abs(xa[:, (hq + hkv) * d:])
    e_ref = float(np.abs(LC.gqa_library(x, c, causal) - want).max())
    allow = max(4.0 * e_ref, 2e-5 * max(1.0, float(np.abs(want).max())))
    out = torch.full((B * T, hq * dv + 8), float("nan"), dtype=BF, device="cuda")
    A.attention(_rows(x, x.shape[1] + 8), out, B, T, hq, d, dv, causal=causal, kv_heads=hkv, math="bf16")
    xe = LC.gqa_expanded(x, c)
    full = torch.full_like(out, float("nan"))
    A.attention(_rows(xe, xe.shape[1] + 8), full, B, T, hq, d, dv, causal=causal, math="bf16")
    torch.cuda.synchronize()
    _check(out, want, BC.bound(want, LC.gqa_oracle(xa, c, causal), allow), f"bf16 math gqa {c} causal={causal}")
    assert torch.equal(out, full), "a GQA launch must equal the plain launch on the expanded rows bit for bit"


def test_bf16_math_falls_back_under_a_padding_mask():
    k = PC.case_bf16((64, 33))
    w_in, w_out = k.heads * (2 * k.d + k.dv), k.heads * k.dv
    assert A.attention_kernel(k.d, k.dv, math="bf16", key_mask=True) == A.attention_kernel(k.d, k.dv)
    gr = k.groups[0]
    out = torch.full((k.B * k.T, w_out + 8), float("nan"), dtype=BF, device="cuda")
    A.attention(_rows(k.qkv, w_in + 8), out, k.B, k.T, k.heads, k.d, k.dv, key_mask=torch.from_numpy(gr.mask).cuda(),
                math="bf16")
    torch.cuda.synchronize()
    _check(out, gr.want, gr.allow + 2.0 ** -8 * np.abs(gr.want), f"bf16 math under a padding mask {gr.group}")


@pytest.mark.parametrize("c,extra", [((2, 37, 3, 48, 80, None), 4), ((2, 37, 2, 160, 160, None), 0)], ids=str)
def test_bf16_math_falls_back_off_the_grid_and_at_a_wide_head(c, extra):
    k = WC.case(c, False, True)
    w_in, w_out = WC.AC.widths(c)
    ld_in, ld_out = (w_in + 7) // 8 * 8 + extra, (w_out + 7) // 8 * 8 + extra
    assert A.attention_kernel(k.d, k.dv, math="bf16", strides=(ld_in, ld_out)) == A.attention_kernel(k.d, k.dv)
    out = torch.full((k.B * k.T, ld_out), float("nan"), dtype=BF, device="cuda")
    A.attention(_rows(k.qkv, ld_in), out, k.B, k.T, k.heads, k.d, k.dv, math="bf16")
    torch.cuda.synchronize()
    _check(out, k.want, k.allow + 2.0 ** -8 * np.abs(k.want), f"bf16 math fall-back {c} stride + {extra}")


def test_bf16_math_on_fp32_tensors_is_refused():
    x, out = torch.zeros(4, 48, device="cuda"), torch.zeros(4, 16, device="cuda")
    with pytest.raises(ValueError):
        A.attention(x, out, 1, 4, 1, 16, 16, math="bf16")


def _llama():
    return LC.micro() + (lambda ex, out: out.double().cpu().numpy().reshape(2, -1)[:, :97],)


def _vit():                                 # the fixture of tests/test_vit_gpu.py
    g = build_model("vit_micro", classes=10)
    w = init_weights(g, seed=0)
    for n in list(w):
        if n.endswith("/bias") or "pos_embed" in n:
            w[n] = np.random.default_rng(len(n)).standard_normal(w[n].shape).astype(np.float32) * 0.5
    x = np.random.default_rng(5).standard_normal((4, 32, 32, 3)).astype(np.float32)
    feat_name = g.layers[g.output].inputs[0]
    feat = ReferenceExecutor(g, w, device="cpu").run({g.input: torch.from_numpy(x)}, outputs=[feat_name])[feat_name]
    want = feat.double().numpy() @ w[f"{g.output}/kernel"].astype(np.float64) + w[f"{g.output}/bias"]
    return g, w, x, want, lambda ex, out: ex.logits().double().cpu().numpy()


@pytest.mark.parametrize("model", [_llama, _vit], ids=["llama_micro", "vit_micro"])
def test_models_with_bf16_attention_math_captured_and_replayed(model, monkeypatch, budget=5e-2):
    g, w, x, want, logits_of = model()
    monkeypatch.delenv("ADAPT_ATTENTION_MATH", raising=False)
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision="bf16", attention_math="bf16")
    base = SliceExecutor(g, w, batch=2, device="cuda:0", precision="bf16")
    assert [s.kind for s in ex.steps] == [s.kind for s in base.steps]                    # the plan is the same
    ex.capture()
    assert ex.captured
    seen = []
    for half in (slice(0, 2), slice(2, 4)):
        xd = torch.from_numpy(x[half]).cuda()
        out = ex(xd)
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        logits = logits_of(ex, out)
        rel = np.abs(logits - want[half]).max() / np.abs(want[half]).max()
        print(f"{g.name} bf16, attention_math bf16: logits rel err {rel:.3e}")
        assert rel <= budget
        assert not torch.equal(out, base(xd)), "the switch did not reach the kernel"
        seen.append(logits)
    assert np.abs(seen[0] - seen[1]).max() > 2 * budget * np.abs(want).max(), "the replay returned the first input's result"
