"""csrc/kernels/gconv_f32.hip on the GPU: the grouped-convolution kernel against the float64 CPU oracle, against
the dense block-diagonal expansion on the existing fp32 conv kernels, and ResNeXt-50 end to end.

Metric and bound are tests/test_fp32_gpu.py's: max|got - want| / max(1, max|want|) < 2e-5, the project's fp32-conv
bound (fp32 `F.conv2d` itself lands at 0.5e-7 .. 3.5e-7 on these inputs).  Shapes: tests/gconv_cases.py.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import gconv_cases as GC

pytestmark = pytest.mark.gpu

BOUND = 2e-5


def _rel1(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def _run(c):
    pg = C.pack_gconv_f32(c.kern, c.bias, c.G, c.stride, c.pads, "cuda")
    out = torch.full(c.out_shape, float("nan"), dtype=torch.float32, device="cuda")
    C.gconv_forward_f32(torch.from_numpy(c.x).cuda(), pg, out, relu=c.act)
    torch.cuda.synchronize()
    return pg, out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("shape", GC.SHAPES, ids=str)
def test_gconv_f32_matches_float64_oracle(shape):
    c = GC.case(shape)
    pg, got = _run(c)
    want_path = "mfma" if shape in GC.MFMA_SHAPES else "generic"
    assert C.gconv_path(c.Cin, c.Cout, c.G, c.k, c.k) == want_path and pg.path == want_path
    if want_path == "mfma":          # fragment-packed weights: the generic kernel could not have read them
        nj = 2 if c.Cin // c.G == 32 else 1
        assert tuple(pg.w.shape) == (c.Cout // 16, c.k * c.k, nj, 64, 4)
    assert np.isfinite(got).all(), "an output element was not written (NaN pre-fill) or is not finite"
    err = _rel1(got, c.want)
    print(f"gconv {shape} path {pg.path} act {c.act}: rel err {err:.3e}")
    assert err < BOUND


def test_activation_modes_are_all_used():
    assert {GC.case(s).act for s in GC.SHAPES} == {0, 1, 2}
    assert {GC.case(s).act for s in GC.MFMA_SHAPES} == {0, 1, 2}


@pytest.mark.parametrize("shape", [GC.SHAPES[0], GC.SHAPES[1], GC.SHAPES[4]], ids=str)
def test_gconv_f32_agrees_with_dense_block_diagonal_conv(shape):
    """CG 4 (stride 1 and 2) and CG 32: the same layer as a dense HWIO kernel on conv_forward_f32."""
    c = GC.case(shape)
    _, got = _run(c)
    pc = C.pack_conv_f32(GC.dense_kernel(c.kern, c.G), c.bias, c.stride, c.pads, "cuda")
    dense = torch.full(c.out_shape, float("nan"), dtype=torch.float32, device="cuda")
    C.conv_forward_f32(torch.from_numpy(c.x).cuda(), pc, dense, relu=c.act)
    torch.cuda.synchronize()
    err = _rel1(got, dense.cpu().numpy().astype(np.float64))
    print(f"gconv vs dense expansion {shape}: rel diff {err:.3e}")
    assert err < BOUND


def test_launcher_rejects_a_path_the_shape_does_not_fit():
    """Weights packed for the generic path are never handed to the MFMA kernel (no silent fall-through either way)."""
    c = GC.case(GC.SHAPES[7])
    pg = C.pack_gconv_f32(c.kern, c.bias, c.G, c.stride, c.pads, "cuda")
    pg.path = "mfma"
    out = torch.empty(c.out_shape, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="gconv_f32_forward"):
        C.gconv_forward_f32(torch.from_numpy(c.x).cuda(), pg, out)


# ------------------------------------------------------------------ whole model
def test_resnext50_fp32_logits_match_oracle_captured_and_replayed():
    """As test_other_families_fp32_logits_match_oracle (tests/test_fp32_gpu.py), on the captured graph; a replay
    on a second input gives that input's logits."""
    g = build_model("resnext50_32x4d")
    w = init_weights(g, seed=0)
    shape = tuple(g.layers[g.input].out_shape)
    x = np.random.default_rng(5).uniform(0, 255, (4,) + shape).astype(np.float32)
    feat_name = g.layers[g.output].inputs[0]
    feat = ReferenceExecutor(g, w, device="cpu").run({g.input: torch.from_numpy(x)}, outputs=[feat_name])[feat_name]
    want = feat.double().reshape(4, -1).numpy() @ w[f"{g.output}/kernel"].astype(np.float64) + w[f"{g.output}/bias"]
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision="fp32")
    assert [st.kind for st in ex.steps].count("gconv") == 16
    assert {ex.packed[i].path for i, st in enumerate(ex.steps) if st.kind == "gconv"} == {"mfma"}
    ex.capture()
    assert ex.captured
    seen = []
    for half in (slice(0, 2), slice(2, 4)):
        probs = ex(torch.from_numpy(x[half]).cuda())
        torch.cuda.synchronize()
        logits = ex.logits().double().cpu().numpy()
        rel = np.abs(logits - want[half]).max() / np.abs(want[half]).max()
        print(f"resnext50_32x4d fp32 logits rel err {rel:.3e}")
        assert rel <= 1e-3, f"resnext50_32x4d fp32 logits rel err {rel}"
        assert (logits.argmax(-1) == want[half].argmax(-1)).all()
        assert torch.isfinite(probs).all()
        seen.append(logits)
    # the two inputs' logits are further apart than the budget, so a stale replay could not have passed above
    assert np.abs(want[:2] - want[2:]).max() > 4e-3 * np.abs(want).max()
    assert np.abs(seen[0] - seen[1]).max() > 2e-3 * np.abs(want).max(), "the replay returned the first input's result"


def test_bf16_refuses_grouped_conv_at_construction():
    g = build_model("resnext_tiny", input_shape=(64, 64, 3), classes=10)
    w = init_weights(g, seed=0)
    with pytest.raises(NotImplementedError, match=r"conv2_block1_2_conv.*fp32"):
        SliceExecutor(g, w, batch=2, device="cuda:0", precision="bf16")
