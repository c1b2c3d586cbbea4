"""Incremental decoding on MXFP4 weights (`SliceExecutor(..., weight_quant="mxfp4")`, csrc/kernels/gemm_skinny_mx.h):
llama_micro teacher-forced as in tests/test_decode_skinny_gpu.py, captured and replayed, against the model by hand
in float64 on the dequantised weights at every position, with that file's bf16 budget."""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_llama
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import mx as MX
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import llama_cases as LC

pytestmark = pytest.mark.gpu
P, N = 7, 12


@pytest.fixture(scope="module")
def quantised():
    """(weights with every projection / MLP kernel replaced by its dequantised MXFP4 form, ids, float64 logits).
    Blocks run along a kernel's input axes: all but the last of query / key / value and the MLP, the first two
    (heads, head size) of attention_output.  The 1 / sqrt(16) query scale the packer folds in is a power of two."""
    _, w, ids, _ = LC.micro(all_positions=True)
    wq = dict(w)
    for name, k in w.items():
        if name.endswith("/kernel") and name != "lm_head/kernel":
            out_proj = name.endswith("attention_output/kernel")
            m = k.reshape(-1, k.shape[-1]) if out_proj else k.reshape(k.shape[0], -1)          # [K][N]
            wq[name] = MX.dequantize_mxfp4(*MX.quantize_mxfp4(m.T)).T.reshape(k.shape)
    return wq, ids, LC.forward("llama_micro", wq, ids, all_positions=True)


def test_llama_micro_decodes_on_mxfp4_weights(quantised):
    _, w, _, _ = LC.micro(all_positions=True)
    _, ids, want = quantised
    ex = SliceExecutor(build_llama("llama_micro", input_shape=(P,)), w, 2, precision="bf16", kv_cache=P + N,
                       weight_quant="mxfp4")
    scale, V = np.abs(want).max(), want.shape[-1]
    x = torch.from_numpy(ids[:2]).cuda()
    for gemm in ("skinny", "tiles"):
        dec = ex.decoder(gemm=gemm)
        routed = [dec.steps[i] for i in dec.mx_steps]
        if gemm == "tiles":
            assert routed == [] and dec.skinny_steps == []
        else:
            assert len(routed) == 10 and dec.skinny_steps == []                    # qkv, out, gate, up, down x 2 blocks
            assert sorted(dec.packed[i].cin for i in dec.mx_steps) == [64] * 8 + [176] * 2
            assert all(f"mx={dec._mx[i]}" in dec.describe().splitlines()[i] for i in dec.mx_steps)
        dec.capture()
        got = [ex(x[:, :P]).float().cpu().numpy().reshape(2, -1)[:, :V]]
        for t in range(P, P + N):
            got.append(dec(x[:, t:t + 1]).float().cpu().numpy().reshape(2, -1)[:, :V])
        rel = np.abs(np.stack(got, axis=1) - want[:2, P - 1:P + N]).max(axis=(0, 2)) / scale
        print(f"llama_micro mxfp4 {gemm} decode rel err per position {np.array2string(rel, precision=2)}")
        assert rel.max() <= 5e-2


def test_weight_quant_is_opt_in_and_bf16_only():
    _, w, _, _ = LC.micro(all_positions=True)
    g = build_llama("llama_micro", input_shape=(P,))
    ex = SliceExecutor(g, w, 2, precision="bf16", kv_cache=P + N)
    assert ex.decoder(gemm="skinny").mx_steps == [] and all(getattr(pc, "mx", None) is None for pc in ex.packed.values())
    with pytest.raises(ValueError, match="weight_quant"):
        SliceExecutor(g, w, 2, precision="fp32", kv_cache=P + N, weight_quant="mxfp4")


def test_generate_on_mxfp4_weights():
    g, w, ids, _ = LC.micro(all_positions=True)
    m = Model(g, w)
    toks, logits = m.generate(ids[:2, :P], N, precision="bf16", return_logits=True, weight_quant="mxfp4",
                              decode_gemm="skinny")
    np.testing.assert_array_equal(toks, logits.argmax(-1))
    (key,) = [k for k in m._executors if k[0] == "generate"]
    assert "mxfp4" in key and len(m._executors[key][1].mx_steps) == 10
