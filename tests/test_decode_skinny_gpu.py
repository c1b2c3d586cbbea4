"""Incremental decoding with the projection and MLP steps on the skinny GEMM (`SliceExecutor.decoder(gemm="skinny")`,
csrc/kernels/gemm_skinny.h): llama_micro teacher-forced as in tests/test_decode_gpu.py, captured and replayed, against
the model by hand in float64 at every position with that file's budgets."""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_llama
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import llama_cases as LC

pytestmark = pytest.mark.gpu
P, N = 7, 12


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_llama_micro_decodes_on_the_skinny_gemm(precision, budget):
    _, w, ids, want = LC.micro(all_positions=True)
    ex = SliceExecutor(build_llama("llama_micro", input_shape=(P,)), w, 2, precision=precision, kv_cache=P + N)
    dec = ex.decoder(gemm="skinny")
    assert ex.decoder().skinny_steps == [] and ex.skinny_steps == []
    routed = [dec.steps[i] for i in dec.skinny_steps]
    assert len(routed) == 10 and all(st.kind == "conv" for st in routed)       # qkv, out, gate, up, down x 2 blocks
    assert sum(len(st.ins) > 1 for st in routed) == 4                           # out and down carry their residual
    assert all(f"skinny={dec._skinny[i]}" in dec.describe().splitlines()[i] for i in dec.skinny_steps)
    dec.capture()
    scale, V = np.abs(want).max(), want.shape[-1]
    x = torch.from_numpy(ids[:2]).cuda()
    got = [ex(x[:, :P]).float().cpu().numpy().reshape(2, -1)[:, :V]]
    for t in range(P, P + N):
        got.append(dec(x[:, t:t + 1]).float().cpu().numpy().reshape(2, -1)[:, :V])
    rel = np.abs(np.stack(got, axis=1) - want[:2, P - 1:P + N]).max(axis=(0, 2)) / scale
    print(f"llama_micro {precision} skinny decode rel err per position {np.array2string(rel, precision=2)}")
    assert rel.max() <= budget


def test_generate_with_the_skinny_gemm():
    g, w, ids, _ = LC.micro(all_positions=True)
    m = Model(g, w)
    toks, logits = m.generate(ids[:2, :P], N, return_logits=True, decode_gemm="skinny")
    np.testing.assert_array_equal(toks, logits.argmax(-1))
    m.generate(ids[:2, :P], N)
    keys = [k for k in m._executors if k[0] == "generate"]
    assert sorted(k[-1] for k in keys) == ["skinny", "tiles"]                   # an executor pair per path
    assert all(len(m._executors[k][1].skinny_steps) == (10 if k[-1] == "skinny" else 0) for k in keys)
