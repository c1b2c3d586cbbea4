"""Llama through SliceExecutor on the GPU: `llama_micro` (40 tokens, 2 blocks, 4 query heads of 16 over 2 key /
value heads: the attention core's MFMA path with g = 2) in both precisions, captured and replayed, sliced inside a
block, and the token ids kept fp32 in the bf16 plan.

Budgets are those of tests/test_gpt_gpu.py: logits within 1e-3 (fp32) and 5e-2 (bf16) of the model by hand in
float64 (tests/llama_cases.py), relative to the largest logit.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import llama_cases as LC

pytestmark = pytest.mark.gpu

CUT = "llama_micro_block_0_post_attention_norm"
BLOCK_KINDS = ["rmsnorm", "conv", "rope", "attention", "conv", "rmsnorm", "conv", "act", "conv", "binary", "conv"]


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_llama_micro_logits_match_the_model_by_hand_captured_and_replayed(precision, budget):
    g, w, ids, want = LC.micro()
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    assert [st.kind for st in ex.steps] == ["embedding"] + BLOCK_KINDS * 2 + ["crop", "rmsnorm", "conv"]  # no pack step
    cores = [st for st in ex.steps if st.kind == "attention"]
    assert [(st.p.get("causal"), st.p.get("kv_heads"), st.p.get("rope")) for st in cores] == [(True, 2, 10000.0)] * 2
    tables = [ex.packed[i] for i, st in enumerate(ex.steps) if st.kind == "rope"]
    assert len(tables) == 2 and tables[0] is tables[1]               # one table, prepared once, for both layers
    assert tables[0].dtype == torch.float32 and tuple(tables[0].shape) == (2, 40, 8)      # fp32 in both precisions
    # the ids stay fp32 in the bf16 plan too
    assert ex.input_buf(g.input).dtype == torch.float32 and tuple(ex.input_buf(g.input).shape) == (2, 40)
    ex.capture()
    assert ex.captured
    seen = []
    for half in (slice(0, 2), slice(2, 4)):
        out = ex(torch.from_numpy(ids[half]).cuda())
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        logits = out.double().cpu().numpy().reshape(2, -1)[:, :97]
        rel = np.abs(logits - want[half]).max() / np.abs(want[half]).max()
        print(f"llama_micro {precision} logits rel err {rel:.3e}")
        assert rel <= budget, f"llama_micro {precision} logits rel err {rel}"
        seen.append(logits)
    # the two inputs' logits are further apart than the budget, so a stale replay could not have passed above
    assert np.abs(want[:2] - want[2:]).max() > 4 * budget * np.abs(want).max()
    assert np.abs(seen[0] - seen[1]).max() > 2 * budget * np.abs(want).max(), "the replay returned the first input's result"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_stage_slice_inside_a_block_equals_unsliced(precision):
    """The cut falls between the second RMS normalisation and the gate / up projections; the block's residual crosses
    beside it.  Both stages run the same kernels on the same values: bit-identical."""
    g, w, ids, _ = LC.micro()
    xd = torch.from_numpy(ids[:2]).cuda()
    full = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)(xd).clone()
    parts = slicer.partition(g, [CUT])
    assert set(parts[1].inputs) == {CUT, "llama_micro_block_0_add1"}
    vals = {g.input: xd}
    for s in parts:
        sg = slicer.subgraph(g, s)
        ex = SliceExecutor(sg, w, batch=2, device="cuda:0", precision=precision)
        if g.input in sg.input_names:
            assert ex.input_buf(g.input).dtype == torch.float32
        out = ex.run({k: vals[k] for k in sg.input_names})
        vals.update({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert torch.equal(vals[g.output], full)
