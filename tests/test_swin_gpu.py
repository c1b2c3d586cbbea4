"""Swin through SliceExecutor on the GPU: `swin_micro` (an 8 x 8 map of four 4 x 4 windows with one shifted block,
then a single 4 x 4 window; heads of 16) in both precisions, captured and replayed, sliced inside the shifted
block, and a single WindowAttention layer on the plain kernel with channel counts that the bf16 layout pads.

Budgets are the project's model budgets (tests/test_layernorm_gpu.py): logits within 1e-3 (fp32) and 5e-2 (bf16)
of the oracle, relative to the largest logit.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

pytestmark = pytest.mark.gpu

CUT = "swin_micro_stage_0_block_1_ln2"
BLOCK_KINDS = ["layernorm", "conv", "winattn", "conv", "layernorm", "conv", "act", "conv"]
MERGE_KINDS = ["space_to_depth", "layernorm", "conv"]


def _noisy(w):
    for n in list(w):                       # biases and tables of O(1): a dropped or misplaced one must show
        if n.endswith("/bias") or n.endswith("bias_table"):
            w[n] = np.random.default_rng(len(n)).standard_normal(w[n].shape).astype(np.float32) * 0.5
    return w


@pytest.fixture(scope="module")
def micro():
    g = build_model("swin_micro", classes=10)
    w = _noisy(init_weights(g, seed=0))
    x = np.random.default_rng(5).standard_normal((4, 32, 32, 3)).astype(np.float32)
    # the second pair carries a strong pattern on top (two opposite quadrants; two opposite colours): the average
    # pool makes pure-noise images' logits too alike for the stale-replay assertion below to mean anything
    x[2, :16, :16] += 5
    x[2, 16:, 16:] -= 5
    x[3, :, :, 0] += 5
    x[3, :, :, 1] -= 5
    feat_name = g.layers[g.output].inputs[0]
    feat = ReferenceExecutor(g, w, device="cpu").run({g.input: torch.from_numpy(x)}, outputs=[feat_name])[feat_name]
    want = feat.double().numpy() @ w[f"{g.output}/kernel"].astype(np.float64) + w[f"{g.output}/bias"]
    return g, w, x, want


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_swin_micro_logits_match_oracle_captured_and_replayed(micro, precision, budget):
    g, w, x, want = micro
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    kinds = [st.kind for st in ex.steps if st.kind != "pack"]
    assert [k for k in kinds if k in ("winattn", "space_to_depth")] == ["winattn"] * 2 + ["space_to_depth"] + ["winattn"] * 2
    assert kinds[-(len(BLOCK_KINDS) * 2 + 3):-3] == BLOCK_KINDS * 2 and kinds[-3:] == ["layernorm", "gap", "dense"]
    i = kinds.index("space_to_depth")
    assert kinds[i:i + 3] == MERGE_KINDS and kinds[i - 2 * len(BLOCK_KINDS):i] == BLOCK_KINDS * 2
    ex.capture()
    assert ex.captured
    seen = []
    for half in (slice(0, 2), slice(2, 4)):
        probs = ex(torch.from_numpy(x[half]).cuda())
        torch.cuda.synchronize()
        logits = ex.logits().double().cpu().numpy()
        rel = np.abs(logits - want[half]).max() / np.abs(want[half]).max()
        print(f"swin_micro {precision} logits rel err {rel:.3e}")
        assert rel <= budget, f"swin_micro {precision} logits rel err {rel}"
        assert torch.isfinite(probs).all()
        seen.append(logits)
    # the two inputs' logits are further apart than the budget, so a stale replay could not have passed above
    assert np.abs(want[:2] - want[2:]).max() > 4 * budget * np.abs(want).max()
    assert np.abs(seen[0] - seen[1]).max() > 2 * budget * np.abs(want).max(), "the replay returned the first input's result"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_stage_slice_inside_a_shifted_block_equals_unsliced(micro, precision):
    """The cut falls between two steps of the unsliced plan (the layernorm and the Dense after it) of the shifted
    block; the block's residual crosses beside it.  Both stages run the same kernels on the same values:
    bit-identical."""
    g, w, x, _ = micro
    assert g.layers["swin_micro_stage_0_block_1_attn"].attrs["shift"] == 2
    xd = torch.from_numpy(x[:2]).cuda()
    full = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)(xd).clone()
    parts = slicer.partition(g, [CUT])
    assert set(parts[1].inputs) == {CUT, "swin_micro_stage_0_block_1_add1"}
    vals = {g.input: xd}
    for s in parts:
        sg = slicer.subgraph(g, s)
        ex = SliceExecutor(sg, w, batch=2, device="cuda:0", precision=precision)
        out = ex.run({k: vals[k] for k in sg.input_names})
        vals.update({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert torch.equal(vals[g.output], full)


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
@pytest.mark.parametrize("shift", [0, 1])
def test_one_window_attention_layer_on_the_plain_kernel_with_padded_channels(precision, budget, shift):
    """C = 20 (bf16 stores 24), heads 2 x 10, M = 3 on a 6 x 9 map: the plain kernel, qkv rows 60 wide (64 stored)
    and context rows 20 wide (24 stored)."""
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (6, 9, 20)}))
    g.add(Layer("attn", "winattn", ["in"], {"num_heads": 2, "key_dim": 10, "window": 3, "shift": shift,
                                            "use_bias": True}))
    g.output_names = ["attn"]
    w = _noisy(init_weights(g, 3))
    x = np.random.default_rng(2).standard_normal((2, 6, 9, 20)).astype(np.float32)
    want = ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    assert [st.kind for st in ex.steps if st.kind != "pack"] == ["conv", "winattn", "conv"]
    ex.output_buf("attn").fill_(float("nan"))
    out = ex(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    got = out.float().cpu().numpy()
    assert np.isfinite(got).all()
    if precision == "bf16":
        assert tuple(out.shape) == (2, 6, 9, 24) and (got[..., 20:] == 0).all()
    rel = np.abs(got[..., :20] - want).max() / np.abs(want).max()
    print(f"one winattn layer shift {shift} {precision}: rel err {rel:.3e}")
    assert rel <= budget
