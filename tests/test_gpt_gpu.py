"""GPT through SliceExecutor on the GPU: `gpt_micro` (40 tokens, 2 blocks, 2 heads of 16) in both precisions,
captured and replayed, sliced inside a block, and the token ids kept fp32 in the bf16 plan.

Budgets are the project's model budgets (tests/test_vit_gpu.py): logits within 1e-3 (fp32) and 5e-2 (bf16) of the
model by hand in float64 (tests/gpt_cases.py), relative to the largest logit.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import gpt_cases as GC

pytestmark = pytest.mark.gpu

CUT = "gpt_micro_block_0_ln2"
BLOCK_KINDS = ["layernorm", "conv", "attention", "conv", "layernorm", "conv", "act", "conv"]


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_gpt_micro_logits_match_the_model_by_hand_captured_and_replayed(precision, budget):
    g, w, ids, want = GC.micro()
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    kinds = [st.kind for st in ex.steps]
    assert kinds == ["embedding", "posembed"] + BLOCK_KINDS * 2 + ["crop", "layernorm", "conv"]     # no pack step
    assert [st.p.get("causal") for st in ex.steps if st.kind == "attention"] == [True, True]
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
        print(f"gpt_micro {precision} logits rel err {rel:.3e}")
        assert rel <= budget, f"gpt_micro {precision} logits rel err {rel}"
        seen.append(logits)
    # the two inputs' logits are further apart than the budget, so a stale replay could not have passed above
    assert np.abs(want[:2] - want[2:]).max() > 4 * budget * np.abs(want).max()
    assert np.abs(seen[0] - seen[1]).max() > 2 * budget * np.abs(want).max(), "the replay returned the first input's result"


def test_the_bf16_plan_keeps_the_token_ids_fp32():
    """Vocabulary 1000 with odd ids above 256, none of which bf16 holds: the bf16 run's embedding rows are the fp32
    run's rows after one rounding, so the ids were never rounded; and the logits stay within the budget."""
    g, w, ids, want = GC.micro(vocab=1000)
    assert (ids > 256).sum() > ids.size // 3
    assert (torch.from_numpy(ids).to(torch.bfloat16).float().numpy() != ids)[ids > 256].all()
    x = torch.from_numpy(ids[:2]).cuda()
    rows = {}
    for precision in ("fp32", "bf16"):
        ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision, outputs=["gpt_micro_wte", g.output])
        assert ex.input_buf(g.input).dtype == torch.float32
        out = ex.run({g.input: x})
        torch.cuda.synchronize()
        rows[precision] = out["gpt_micro_wte"].clone()
        logits = out[g.output].double().cpu().numpy().reshape(2, -1)[:, :1000]
        rel = np.abs(logits - want[:2]).max() / np.abs(want[:2]).max()
        print(f"gpt_micro vocabulary 1000 {precision} logits rel err {rel:.3e}")
        assert rel <= (1e-3 if precision == "fp32" else 5e-2)
    table = torch.from_numpy(w["gpt_micro_wte/embeddings"])
    assert torch.equal(rows["fp32"].cpu().reshape(2, 40, 32), table[torch.from_numpy(ids[:2]).long()])
    assert rows["bf16"].dtype == torch.bfloat16
    assert torch.equal(rows["bf16"].cpu(), rows["fp32"].to(torch.bfloat16).cpu())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_stage_slice_inside_a_block_equals_unsliced(precision):
    """The cut falls between the layernorm and the Dense after it; the block's residual crosses beside it.  Both
    stages run the same kernels on the same values: bit-identical."""
    g, w, ids, _ = GC.micro()
    xd = torch.from_numpy(ids[:2]).cuda()
    full = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)(xd).clone()
    parts = slicer.partition(g, [CUT])
    assert set(parts[1].inputs) == {CUT, "gpt_micro_block_0_add1"}
    vals = {g.input: xd}
    for s in parts:
        sg = slicer.subgraph(g, s)
        ex = SliceExecutor(sg, w, batch=2, device="cuda:0", precision=precision)
        out = ex.run({k: vals[k] for k in sg.input_names})
        vals.update({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert torch.equal(vals[g.output], full)
