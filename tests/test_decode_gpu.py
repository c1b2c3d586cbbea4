"""Incremental decoding through the executor and `Model.generate`: llama_micro with LC.micro's weights and ids,
teacher-forced (a prompt of P tokens, then the next N ids of the same row fed one per step, not the argmax, so a tie
cannot fork the run) against the model by hand in float64 at every position, captured and replayed."""
import copy

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    build_gpt, build_llama)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import llama_cases as LC

pytestmark = pytest.mark.gpu
P, N = 7, 12


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_llama_micro_decodes_token_by_token(precision, budget):
    _, w, ids, want = LC.micro(all_positions=True)
    g = build_llama("llama_micro", input_shape=(P,))
    ex = SliceExecutor(g, w, 2, precision=precision, kv_cache=P + N)
    plain = SliceExecutor(g, w, 2, precision=precision)
    assert [(s.kind, s.out) for s in ex.steps] == [(s.kind, s.out) for s in plain.steps]
    dec = ex.decoder()
    ex.capture()
    dec.capture()
    scale, V = np.abs(want).max(), want.shape[-1]   # a bf16 logits row is padded to 8 channels
    seen = []
    for half in (slice(0, 2), slice(2, 4)):             # two prompts through the same captured graphs
        x = torch.from_numpy(ids[half]).cuda()
        first = ex(x[:, :P]).clone()
        assert torch.equal(first, plain(x[:, :P])), "the prefill output changed with kv_cache set"
        assert ex.positions.tolist() == [P, P]
        got = [first.float().cpu().numpy().reshape(2, -1)[:, :V]]
        for t in range(P, P + N):
            got.append(dec(x[:, t:t + 1]).float().cpu().numpy().reshape(2, -1)[:, :V])
        assert ex.positions.tolist() == [P + N, P + N]
        got = np.stack(got, axis=1)                     # positions P - 1 .. P + N - 1
        rel = np.abs(got - want[half, P - 1:P + N]).max(axis=(0, 2)) / scale
        print(f"llama_micro {precision} decode rel err per position {np.array2string(rel, precision=2)}")
        assert rel.max() <= budget
        seen.append(got)
    assert np.abs(seen[0] - seen[1]).max() > 2 * budget * scale, "the replay returned the first prompt's result"


def test_generate_is_the_argmax_chain_of_its_logits():
    g, w, ids, _ = LC.micro(all_positions=True)
    m = Model(g, w)
    toks, logits = m.generate(ids[:2, :P], N, return_logits=True)
    assert toks.shape == (2, N) and toks.dtype == np.int64 and logits.shape[:2] == (2, N)
    np.testing.assert_array_equal(toks, logits.argmax(-1))
    # its first logits are the full forward pass's at the prompt's last position
    want = LC.forward("llama_micro", w, ids[:2, :P])
    assert np.abs(logits[:, 0] - want).max() <= 1e-3 * np.abs(want).max()
    with pytest.raises(ValueError, match="max_tokens"):
        m.generate(ids[:2, :P], N, max_tokens=P + N - 1)
    with pytest.raises(ValueError, match="zoo"):
        other = copy.copy(g)                            # the same layers under a name no builder knows
        other.name = "elsewhere"
        Model(other, w).generate(ids[:2, :P], N)


def test_gpt_decoder_is_refused_by_layer():
    g = build_gpt("gpt_micro")
    ex = SliceExecutor(g, init_weights(g, seed=0), 1, kv_cache=64)
    with pytest.raises(ValueError, match="gpt_micro_wpe.*posembed"):
        ex.decoder()
