"""U-Net end to end on SliceExecutor: the transposed-convolution, upsample and concat steps inside the captured
hipGraph, in both precisions, against the fp32 CPU oracle.

Budgets are the whole-model ones the other families use (tests/test_gconv_gpu.py, tests/test_layernorm_gpu.py):
fp32 rel <= 1e-3 of max|want|, bf16 rel <= 5e-2 on the first `classes` channels of the padded output.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    build_model, build_unet)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    g = build_model("unet_tiny")
    w = init_weights(g, seed=0)
    x = np.random.default_rng(5).standard_normal((4, 32, 32, 3)).astype(np.float32)
    want = ReferenceExecutor(g, w, device="cpu")(torch.from_numpy(x)).double().numpy()
    return g, w, x, want


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_unet_tiny_matches_oracle_captured_and_replayed(tiny, precision, budget):
    g, w, x, want = tiny
    assert want.shape == (4, 32, 32, 1) and want.min() > 0 and want.max() < 1
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    kinds = [st.kind for st in ex.steps]
    assert kinds.count("deconv") == 2 and kinds.count("concat") == 2
    paths = [ex.packed[i].path for i, st in enumerate(ex.steps) if st.kind == "deconv"]
    assert paths == (["mfma", "mfma"] if precision == "fp32" else ["bf16", "bf16"])      # 64 -> 32 and 32 -> 16
    ex.capture()
    assert ex.captured
    seen = []
    for half in (slice(0, 2), slice(2, 4)):
        out = ex(torch.from_numpy(x[half]).cuda())
        torch.cuda.synchronize()
        got = out.double().cpu().numpy()
        assert got.shape == (2, 32, 32, 1 if precision == "fp32" else 8) and np.isfinite(got).all()
        rel = np.abs(got[..., :1] - want[half]).max() / np.abs(want[half]).max()
        print(f"unet_tiny {precision} rel err {rel:.3e}")
        assert rel <= budget, f"unet_tiny {precision} rel err {rel}"
        seen.append(got[..., :1])
    # the two inputs' outputs are further apart than the budget, so a stale replay could not have passed above
    assert np.abs(want[:2] - want[2:]).max() > 4 * budget * np.abs(want).max()
    assert np.abs(seen[0] - seen[1]).max() > 2 * budget * np.abs(want).max(), "the replay returned the first input's result"


def test_unet_tiny_bilinear_fp32(tiny):
    _, _, x, _ = tiny
    g = build_unet("unet_tiny", up="bilinear")
    w = init_weights(g, seed=0)
    want = ReferenceExecutor(g, w, device="cpu")(torch.from_numpy(x[:2])).double().numpy()
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision="fp32")
    kinds = [st.kind for st in ex.steps]
    assert kinds.count("upsample") == 2 and "deconv" not in kinds
    ex.capture()
    out = ex(torch.from_numpy(x[:2]).cuda())
    torch.cuda.synchronize()
    got = out.double().cpu().numpy()
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"unet_tiny bilinear fp32 rel err {rel:.3e}")
    assert got.shape == (2, 32, 32, 1) and np.isfinite(got).all() and rel <= 1e-3
