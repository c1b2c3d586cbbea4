"""MXFP4 weights without a bf16 copy (`SliceExecutor(..., weight_quant="mxfp4_only")`): llama_micro at batch 2 and a
prompt of 20 tokens, so the prefill's 40 rows run csrc/kernels/gemm_tile_mx.h, then 8 teacher-forced decode steps on
the skinny kernel, against the float64 model on the dequantised weights at every position (the `quantised` fixture
and the 5e-2 budget of tests/test_decode_mx_gpu.py)."""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_llama
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import llama_cases as LC
from test_decode_mx_gpu import quantised  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
P, N = 20, 8


def test_llama_micro_runs_on_the_codes_alone(quantised):  # noqa: F811
    _, w, _, _ = LC.micro(all_positions=True)
    _, ids, want = quantised
    ex = SliceExecutor(build_llama("llama_micro", input_shape=(P,)), w, 2, precision="bf16", kv_cache=P + N,
                       weight_quant="mxfp4_only")
    assert len(ex.mx_tile_steps) == 10 and ex.mx_steps == []                       # qkv, out, gate, up, down x 2 blocks
    assert sorted(ex.packed[i].cin for i in ex.mx_tile_steps) == [64] * 8 + [176] * 2
    assert all(ex.packed[i].w.shape[0] == 0 and ex.packed[i].mx is not None for i in ex.mx_tile_steps)
    assert all(f"mxt={ex._mx_tile[i]}" in ex.describe().splitlines()[i] for i in ex.mx_tile_steps)
    scale, V = np.abs(want).max(), want.shape[-1]
    x = torch.from_numpy(ids[:2]).cuda()
    for gemm in ("skinny", "tiles"):
        dec = ex.decoder(gemm=gemm)
        assert dec.mx_steps == ex.mx_tile_steps and dec.skinny_steps == [] and dec.mx_tile_steps == []
        dec.capture()
        got = [ex(x[:, :P]).float().cpu().numpy().reshape(2, -1)[:, :V]]
        for t in range(P, P + N):
            got.append(dec(x[:, t:t + 1]).float().cpu().numpy().reshape(2, -1)[:, :V])
        rel = np.abs(np.stack(got, axis=1) - want[:2, P - 1:P + N]).max(axis=(0, 2)) / scale
        print(f"llama_micro mxfp4_only {gemm} decode rel err per position {np.array2string(rel, precision=2)}")
        assert rel.max() <= 5e-2


def test_generate_on_the_codes_alone():
    g, w, ids, _ = LC.micro(all_positions=True)
    m = Model(g, w)
    toks, logits = m.generate(ids[:2, :P], N, precision="bf16", return_logits=True, weight_quant="mxfp4_only")
    np.testing.assert_array_equal(toks, logits.argmax(-1))
    (key,) = [k for k in m._executors if k[0] == "generate"]
    assert "mxfp4_only" in key and len(m._executors[key][0].mx_tile_steps) == 10
    with pytest.raises(ValueError, match="weight_quant"):
        SliceExecutor(build_llama("llama_micro", input_shape=(P,)), w, 2, precision="fp32", weight_quant="mxfp4_only")
