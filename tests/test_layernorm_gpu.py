"""csrc/kernels/layernorm.hip on the MI355X, the depthwise routing of Conv2D(groups=C), and ConvNeXt through
`SliceExecutor` in both precisions.

Cases, the float64 oracle and the fp32 allowance max(4 e_ref, 2e-5 max(1, max|want|)): tests/layernorm_cases.py
(e_ref is the error of the library's fp32 `F.layer_norm` on the CPU; the one-pass E[x^2] - mu^2 form misses the
allowance by 280x - 2000x on the two cancellation probes).  bf16: the input is the case rounded to bf16, the
oracle follows the rounded values, and an output element may be off by one bf16 rounding step on top of the fp32
term: |got - want| <= 2^-8 |want| + allowance.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops._lib import kernels
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import gconv_cases as GC
import layernorm_cases as LC

pytestmark = pytest.mark.gpu

CUT = "convnext_micro_stage_2_block_0_layernorm"


# ------------------------------------------------------------------ the kernels
def test_the_cases_meet_every_path_of_the_kernel():
    """Lanes per row of the register path by 16-byte vectors per row; 0 is the looped path."""
    lanes = kernels().layernorm_lanes
    assert [lanes(n) for n in (1, 16, 17, 32, 33, 64, 65, 128, 256, 512, 513)] == [8, 8, 16, 16, 32, 32, 64, 64, 64,
                                                                                  64, 0]
    f32 = {lanes(c[1] // 4) if c[1] % 4 == 0 else 0 for c in LC.CASES}
    bf16 = {lanes((c[1] + 7) // 8) for c in LC.CASES}
    assert f32 == {0, 8, 16, 32, 64} and bf16 == {0, 8, 16, 64}


@pytest.mark.parametrize("c", LC.CASES, ids=str)
def test_layernorm_f32_matches_float64_oracle(c):
    k = LC.case(c)
    x = torch.from_numpy(k.x).cuda()
    out = torch.full(k.x.shape, float("nan"), dtype=torch.float32, device="cuda")
    E.layernorm_f32(x, torch.from_numpy(k.gamma_k).cuda(), torch.from_numpy(k.beta_k).cuda(), out, k.eps)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "an output element was not written (NaN pre-fill) or is not finite"
    err = np.abs(got - k.want).max()
    print(f"layernorm_f32 {c}: max err {err:.3e}, allowance {k.allow:.3e}")
    assert err <= k.allow


@pytest.mark.parametrize("c", LC.CASES, ids=str)
def test_layernorm_bf16_matches_float64_oracle_and_zeroes_the_pads(c):
    k = LC.case_bf16(c)
    xp = torch.full((k.rows, k.Cp), float("inf"), dtype=torch.bfloat16)       # +inf in the padding channels
    xp[:, :k.C] = torch.from_numpy(k.x).to(torch.bfloat16)
    out = torch.full((k.rows, k.Cp), float("nan"), dtype=torch.bfloat16, device="cuda")
    E.layernorm(xp.cuda(), torch.from_numpy(k.gamma_p).cuda(), torch.from_numpy(k.beta_p).cuda(), out, k.C, k.eps)
    torch.cuda.synchronize()
    got = out.cpu().float().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "an output element was not written (NaN pre-fill) or is not finite"
    assert (got[:, k.C:] == 0).all(), "padding channels must come out as exact zeros"
    over = np.abs(got[:, :k.C] - k.want) - (2.0 ** -8 * np.abs(k.want) + k.allow)
    print(f"layernorm bf16 {c}: max err {np.abs(got[:, :k.C] - k.want).max():.3e}, worst excess {over.max():.3e}")
    assert (over <= 0).all()


# ------------------------------------------------------------------ Conv2D(groups=C) on the depthwise kernel
def test_one_channel_per_group_conv_runs_on_dwconv_f32():
    rng = np.random.default_rng(7)
    B, H, W, C = 2, 9, 7, 24
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    kern = (rng.standard_normal((7, 7, 1, C)) / 7.0).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (H, W, C)}))
    g.add(Layer("dw", "conv", ["in"], {"filters": C, "kernel": (7, 7), "stride": 1, "padding": "same",
                                       "use_bias": True, "groups": C}))
    g.output_names = ["dw"]
    ex = SliceExecutor(g, {"dw/kernel": kern, "dw/bias": bias}, batch=B, device="cuda:0", precision="fp32")
    assert [st.kind for st in ex.steps] == ["dwconv"]
    ex.output_buf("dw").fill_(float("nan"))
    got = ex(torch.from_numpy(x).cuda()).double().cpu().numpy()
    want = GC.ref_gconv(x, kern, bias, C, 1, ((3, 3), (3, 3)), 0)
    assert np.isfinite(got).all()
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    print(f"groups == C 7x7 on dwconv_f32: rel err {err:.3e}")
    assert err < 2e-5


# ------------------------------------------------------------------ ConvNeXt through SliceExecutor
@pytest.fixture(scope="module")
def micro():
    g = build_model("convnext_micro", classes=10)
    w = init_weights(g, seed=0)
    x = np.random.default_rng(5).standard_normal((4, 64, 64, 3)).astype(np.float32)
    feat_name = g.layers[g.output].inputs[0]
    feat = ReferenceExecutor(g, w, device="cpu").run({g.input: torch.from_numpy(x)}, outputs=[feat_name])[feat_name]
    want = feat.double().numpy() @ w[f"{g.output}/kernel"].astype(np.float64) + w[f"{g.output}/bias"]
    return g, w, x, want


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_convnext_micro_logits_match_oracle_captured_and_replayed(micro, precision, budget):
    g, w, x, want = micro
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    kinds = [st.kind for st in ex.steps]
    assert kinds.count("dwconv") == 5 and kinds.count("layernorm") == 10 and "gconv" not in kinds
    ex.capture()
    assert ex.captured
    seen = []
    for half in (slice(0, 2), slice(2, 4)):
        probs = ex(torch.from_numpy(x[half]).cuda())
        torch.cuda.synchronize()
        logits = ex.logits().double().cpu().numpy()
        rel = np.abs(logits - want[half]).max() / np.abs(want[half]).max()
        print(f"convnext_micro {precision} logits rel err {rel:.3e}")
        assert rel <= budget, f"convnext_micro {precision} logits rel err {rel}"
        assert torch.isfinite(probs).all()
        seen.append(logits)
    # the two inputs' logits are further apart than the budget, so a stale replay could not have passed above
    assert np.abs(want[:2] - want[2:]).max() > 4 * budget * np.abs(want).max()
    assert np.abs(seen[0] - seen[1]).max() > 2 * budget * np.abs(want).max(), "the replay returned the first input's result"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_stage_slice_equals_unsliced(micro, precision):
    """The cut falls between two steps of the unsliced plan, so the stages run the same kernels on the same
    values: bit-identical."""
    g, w, x, _ = micro
    xd = torch.from_numpy(x[:2]).cuda()
    full = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)(xd).clone()
    parts = slicer.partition(g, [CUT])
    assert set(parts[1].inputs) == {CUT, "convnext_micro_downsampling_conv_1"}
    vals = {g.input: xd}
    for s in parts:
        sg = slicer.subgraph(g, s)
        ex = SliceExecutor(sg, w, batch=2, device="cuda:0", precision=precision)
        out = ex.run({k: vals[k] for k in sg.input_names})
        vals.update({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert torch.equal(vals[g.output], full)


def test_bf16_layernorm_dense_layerscale_with_channels_off_the_vector_width():
    """input (8, 8, 20) -> layernorm -> dense 12 -> layerscale: C % 8 != 0 on both sides of the dense."""
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (8, 8, 20)}))
    g.add(Layer("ln", "layernorm", ["in"], {"epsilon": 1e-6}))
    g.add(Layer("fc", "dense", ["ln"], {"units": 12, "use_bias": True}))
    g.add(Layer("ls", "layerscale", ["fc"], {"init_values": 1e-6}))
    g.output_names = ["ls"]
    w = init_weights(g, 1)
    w["fc/bias"] = np.random.default_rng(3).standard_normal(12).astype(np.float32)
    x = np.random.default_rng(2).standard_normal((2, 8, 8, 20)).astype(np.float32)
    want = ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision="bf16")
    assert [st.kind for st in ex.steps] == ["pack", "layernorm", "conv"] and ex.steps[2].p["scale"] == "ls"
    ex.output_buf("ls").fill_(float("nan"))
    out = ex(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert tuple(out.shape) == (2, 8, 8, 16) and out.dtype == torch.bfloat16
    got = out.float().cpu().numpy()
    assert np.isfinite(got).all() and (got[..., 12:] == 0).all()
    rel = np.abs(got[..., :12] - want).max() / np.abs(want).max()
    print(f"bf16 layernorm -> dense -> layerscale: rel err {rel:.3e}")
    assert rel <= 5e-2
