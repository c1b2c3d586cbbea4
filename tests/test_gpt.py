"""GPT-2 (models/zoo.py `build_gpt`) without a GPU: names and structure, parameter totals in closed form, the
`gelu_tanh` activation, `gpt_micro` through the PyTorch oracle and the native CPU path against the model by hand in
float64 (tests/gpt_cases.py), causality as a property of the logits, slicing inside a block, and the command line.

On the GPU: tests/test_gpt_gpu.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import (
    ACT_MODE, ACTIVATIONS, Graph, Layer)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    BUILDERS, GPT, GPT_CONTEXT, build_gpt, build_model)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor

import gpt_cases as GC
from test_vit import _k2, _k3, _rel

PKG = "adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = "gpt_micro_block_0_ln2"
BLOCK_KINDS = ["layernorm", "conv", "attention", "conv", "layernorm", "conv", "act", "conv"]


# ------------------------------------------------------------------ zoo
def test_gpt_names_and_structure():
    assert {"gpt2", "gpt2_medium", "gpt2_large", "gpt2_xl", "gpt_micro"} <= set(BUILDERS)
    assert GPT["gpt_micro"] == (2, 32, 2, 97, 40)
    g = build_model("gpt_micro")
    assert g.order[:3] == ["input_1", "gpt_micro_wte", "gpt_micro_wpe"]
    b = "gpt_micro_block_0"
    assert g.order[3:10] == [f"{b}_{s}" for s in ("ln1", "attn", "add1", "ln2", "mlp_fc1", "mlp_fc2", "add2")]
    assert [g.layers[n].op for n in g.order[3:10]] == ["layernorm", "mha", "add", "layernorm", "dense", "dense", "add"]
    assert g.order[-3:] == ["gpt_micro_last", "gpt_micro_ln_f", "lm_head"] and g.output_names == ["lm_head"]
    assert g.layers[g.input].out_shape == (40,) and g.layers["gpt_micro_wte"].out_shape == (40, 32)
    assert g.layers["gpt_micro_wpe"].out_shape == (1, 40, 32) and not g.layers["gpt_micro_wpe"].attrs["class_token"]
    assert g.layers[f"{b}_attn"].attrs == {"num_heads": 2, "key_dim": 16, "use_bias": True, "causal": True}
    assert g.layers[f"{b}_ln1"].attrs["epsilon"] == 1e-5
    assert g.layers[f"{b}_mlp_fc1"].attrs == {"units": 128, "activation": "gelu_tanh", "use_bias": True}
    assert g.layers["gpt_micro_last"].op == "crop" and g.layers["gpt_micro_last"].out_shape == (1, 1, 32)
    assert g.layers["lm_head"].attrs == {"units": 97, "use_bias": False} and g.layers["lm_head"].out_shape == (1, 1, 97)
    every = build_gpt("gpt_micro", all_positions=True)
    assert "gpt_micro_last" not in every.layers and every.layers["lm_head"].out_shape == (1, 40, 97)
    assert build_gpt("gpt_micro", classes=1000, input_shape=(7,)).layers["lm_head"].out_shape == (1, 1, 1000)
    assert build_model("gpt2").layers["input_1"].out_shape == (128,)
    for shape in ((0,), (GPT_CONTEXT + 1,), (4, 4)):
        with pytest.raises(ValueError, match="gpt_micro"):
            build_gpt("gpt_micro", input_shape=shape)
    assert json.loads(from_keras_json(to_keras_json(g), causal_attention=True).to_json()) == json.loads(g.to_json())


@pytest.mark.parametrize("name,depth,width,heads", [("gpt2", 12, 768, 12), ("gpt2_medium", 24, 1024, 16),
                                                    ("gpt2_large", 36, 1280, 20), ("gpt2_xl", 48, 1600, 25)])
def test_gpt_parameter_totals_in_closed_form(name, depth, width, heads):
    V, ctx, T, C = 50257, 1024, 128, width
    assert GPT[name] == (depth, width, heads, V, T) and width % heads == 0 and width // heads == 64
    # per block: two LayerNormalizations, Q K V and output projections with biases, the two FFN layers
    block = 2 * 2 * C + 4 * (C * C + C) + (C * 4 * C + 4 * C) + (4 * C * C + C)
    published = V * C + ctx * C + depth * block + 2 * C             # the head tied to the token table
    if name == "gpt2":
        assert published == 124_439_808
    g = build_model(name)
    # here the position table has the graph's T rows, and `lm_head` owns a (C, V) kernel of its own
    assert g.count_params() == published - (ctx - T) * C + C * V
    assert build_gpt(name, input_shape=(ctx,)).count_params() == published + C * V
    assert g.layers[f"{name}_block_0_attn"].attrs["num_heads"] == heads
    assert g.layers["lm_head"].out_shape == (1, 1, V)


# ------------------------------------------------------------------ gelu_tanh
def test_gelu_tanh_against_the_formula():
    assert "gelu_tanh" in ACTIVATIONS and ACT_MODE["gelu_tanh"] == 13 and ACT_MODE["gelu"] == 8
    x = np.concatenate([np.linspace(-6, 6, 241), [-20.0, 20.0, 0.0]]).astype(np.float32)
    want = GC.gelu_tanh(x)
    y = np.empty_like(x)
    cpu_executor.native().activation(x, y, ACT_MODE["gelu_tanh"], 0.3)
    assert np.abs(y - want).max() < 2e-6
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (x.size,)}))
    g.add(Layer("act", "act", ["in"], {"fn": "gelu_tanh"}))
    g.output_names = ["act"]
    assert np.abs(ReferenceExecutor(g, {})(torch.from_numpy(x[None])).numpy()[0] - want).max() < 2e-6
    assert np.abs(want - 0.5 * x * (1 + np.vectorize(__import__("math").erf)(x / np.sqrt(2)))).max() > 1e-4


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_keras_json_maps_the_tanh_gelu_names(L, keras3):
    shape = {"batch_shape": [None, 4, 8]} if keras3 else {"batch_input_shape": [None, 4, 8]}

    def doc(dense_cfg, act_cfg):
        layers = [L("InputLayer", "in", [], dtype="float32", **shape),
                  L("Dense", "fc", ["in"], units=6, use_bias=True, **dense_cfg),
                  L("Activation", "act", ["fc"], **act_cfg)]
        return json.dumps({"class_name": "Functional", "config": {"name": "m", "layers": layers,
                                                                  "input_layers": [["in", 0, 0]],
                                                                  "output_layers": [["act", 0, 0]]}})
    for nm in ("gelu_tanh", "gelu_new", "gelu_approximate"):
        g = from_keras_json(doc({"activation": nm}, {"activation": nm}))
        assert g.layers["fc"].attrs["activation"] == "gelu_tanh" and g.layers["act"].attrs == {"fn": "gelu_tanh"}
        assert json.loads(from_keras_json(to_keras_json(g)).to_json()) == json.loads(g.to_json())
    g = from_keras_json(doc({"activation": "gelu", "approximate": True}, {"activation": "gelu", "approximate": True}))
    assert g.layers["fc"].attrs["activation"] == "gelu_tanh" and g.layers["act"].attrs == {"fn": "gelu_tanh"}
    g = from_keras_json(doc({"activation": "gelu"}, {"activation": "gelu", "approximate": False}))
    assert g.layers["fc"].attrs["activation"] == "gelu" and g.layers["act"].attrs == {"fn": "gelu"}


# ------------------------------------------------------------------ numerics
@pytest.mark.parametrize("all_positions", [False, True], ids=["last", "all"])
def test_gpt_micro_matches_the_model_by_hand(all_positions):
    g, w, ids, want = GC.micro(all_positions)
    got = ReferenceExecutor(g, w)(torch.from_numpy(ids)).numpy()
    assert got.shape == (4, 1, 40 if all_positions else 1, 97)
    assert _rel(got.reshape(want.shape), want) < 1e-5
    ex = cpu_executor.CpuExecutor(g, w)
    kinds = [st.kind for st in ex.steps]
    assert kinds == ["embedding", "posembed"] + BLOCK_KINDS * 2 + ([] if all_positions else ["crop"]) + [
        "layernorm", "conv"]
    assert [st.p.get("causal") for st in ex.steps if st.kind == "attention"] == [True, True]
    assert _rel(ex(ids).reshape(want.shape), want) < 1e-5


def test_changing_a_token_leaves_the_logits_before_it_unchanged():
    g, w, ids, _ = GC.micro(True)
    ex = cpu_executor.CpuExecutor(g, w)
    base = ex(ids[:1])[0, 0]
    scale = np.abs(base).max()
    for t in (0, 1, 31, 32, 39):
        other = ids[:1].copy()
        other[0, t] = (other[0, t] + 1) % 97
        got = ex(other)[0, 0]
        assert np.abs(got[:t] - base[:t]).max(initial=0.0) <= 1e-6 * scale, t
        assert np.abs(got[t] - base[t]).max() > 1e-3 * scale, t


def test_two_stage_slice_inside_a_block_equals_unsliced_on_the_cpu_path():
    g, w, ids, _ = GC.micro()
    full = cpu_executor.CpuExecutor(g, w)(ids[:2])
    parts = slicer.partition(g, [CUT])
    assert set(parts[1].inputs) == {CUT, "gpt_micro_block_0_add1"}  # the same two-tensor frontier as in ViT
    vals = {g.input: ids[:2]}
    for s in parts:
        sg = slicer.subgraph(g, s)
        vals.update(cpu_executor.CpuExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
    np.testing.assert_array_equal(vals[g.output], full)


def test_cli_plans_and_runs_gpt_micro_by_name():
    from test_vit import _cli
    r = _cli("plan", "--model", "gpt_micro", "--stages", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "gpt_micro" in r.stdout
    r = _cli("local-infer", "--model", "gpt_micro", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-2000:]
