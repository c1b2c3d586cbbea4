"""Swin Transformer without a GPU: the zoo builder (published parameter totals, the shift rule, refusals), the
Keras JSON round trip with the project's `WindowAttention` / `SpaceToDepth` classes, the compiled plan, the native
CPU path against a float64 forward, slicing inside a block and planning.

The HIP kernels and the GPU executor: tests/test_window_attention_gpu.py, tests/test_swin_gpu.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import planner, slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    BUILDERS, SWIN, build_model, build_swin)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.utils.config import AdaptConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd"
BLOCK_KINDS = ["layernorm", "conv", "winattn", "conv", "layernorm", "conv", "act", "conv"]
MERGE_KINDS = ["space_to_depth", "layernorm", "conv"]
CUT = "swin_micro_stage_0_block_1_ln2"          # inside the shifted block of stage 1


def _params(g):
    """Parameter total from `weight_specs` alone: nothing is allocated."""
    return sum(int(np.prod(shp, dtype=np.int64)) for _, shp in g.weight_specs())


@pytest.mark.parametrize("name,params", [("swin_tiny", 28_288_354), ("swin_small", 49_606_258),
                                         ("swin_base", 87_768_224), ("swin_large", 196_532_476)])
def test_swin_parameter_totals_are_the_published_ones(name, params):
    assert name in BUILDERS and _params(build_model(name)) == params


def test_shapes_weight_specs_and_macs_of_the_two_ops():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (8, 12, 6)}))
    g.add(Layer("attn", "winattn", ["in"], {"num_heads": 2, "key_dim": 3, "window": 4, "shift": 2, "use_bias": True}))
    g.add(Layer("s2d", "space_to_depth", ["attn"], {"block": 2}))
    assert g.layers["attn"].out_shape == (8, 12, 6) and g.layers["s2d"].out_shape == (4, 6, 24)
    assert dict(g.weight_specs(["attn"])) == {
        "attn/query/kernel": (6, 2, 3), "attn/query/bias": (2, 3), "attn/key/kernel": (6, 2, 3),
        "attn/key/bias": (2, 3), "attn/value/kernel": (6, 2, 3), "attn/value/bias": (2, 3),
        "attn/attention_output/kernel": (2, 3, 6), "attn/attention_output/bias": (6,),
        "attn/relative_position_bias_table": (49, 2)}
    assert g.weight_specs(["s2d"]) == []
    # 4 H W C^2 + 2 H W M^2 C with C = heads x key_dim = 6
    assert g.layer_macs("attn") == 4 * 8 * 12 * 36 + 2 * 8 * 12 * 16 * 6 and g.layer_macs("s2d") == 0
    costs = planner.layer_costs(g, batch=4)
    assert costs["attn"] > 0 and costs["s2d"] > 0
    w = init_weights(g, 0)
    assert w["attn/relative_position_bias_table"].shape == (49, 2)
    assert 0.005 < w["attn/relative_position_bias_table"].std() < 0.05          # N(0, 0.02)


@pytest.mark.parametrize("op,shape,attrs,word", [
    ("winattn", (8, 10, 6), {"num_heads": 2, "key_dim": 3, "window": 4, "shift": 0}, "multiple"),
    ("winattn", (8, 8, 6), {"num_heads": 2, "key_dim": 3, "window": 4, "shift": 4}, "shift"),
    ("winattn", (8, 8, 6), {"num_heads": 0, "key_dim": 3, "window": 4, "shift": 0}, "num_heads"),
    ("space_to_depth", (7, 8, 6), {"block": 2}, "even"),
    ("space_to_depth", (8, 8, 6), {"block": 3}, "block"),
])
def test_graph_add_refuses_a_bad_layer_by_name(op, shape, attrs, word):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": shape}))
    with pytest.raises(ValueError, match=f"(?s)'bad'.*{word}"):
        g.add(Layer("bad", op, ["in"], attrs))


def test_swin_micro_structure_and_the_shift_rule():
    g = build_model("swin_micro", classes=10)
    attn = [g.layers[n] for n in g.order if g.layers[n].op == "winattn"]
    assert [(L.out_shape, L.attrs["window"], L.attrs["shift"], L.attrs["num_heads"], L.attrs["key_dim"])
            for L in attn] == [((8, 8, 32), 4, 0, 2, 16), ((8, 8, 32), 4, 2, 2, 16),
                               ((4, 4, 64), 4, 0, 4, 16), ((4, 4, 64), 4, 0, 4, 16)]   # a single window: no shift
    assert g.layers["swin_micro_stage_1_merge"].out_shape == (4, 4, 128)
    assert g.layers["swin_micro_stage_1_merge_reduction"].attrs == {"units": 64, "use_bias": False}
    assert all(g.layers[n].attrs["epsilon"] == 1e-5 for n in g.order if g.layers[n].op == "layernorm")
    assert g.layers[g.output].out_shape == (10,)
    # the published sizes: odd blocks shifted by 7 // 2 in the first three stages, none on the 7 x 7 map
    for name in ("swin_tiny", "swin_base"):
        t = build_model(name)
        for n in t.order:
            L = t.layers[n]
            if L.op == "winattn":
                stage, block = (int(v) for v in n.split("_stage_")[1].replace("_attn", "").split("_block_"))
                assert L.attrs["window"] == 7 and L.attrs["key_dim"] == 32
                assert L.attrs["shift"] == (3 if block % 2 and stage < 3 else 0), n
        assert [t.layers[n].out_shape[:2] for n in t.order if t.layers[n].op == "space_to_depth"] == [
            (28, 28), (14, 14), (7, 7)]


def test_a_bad_input_size_is_refused_by_stage_name():
    with pytest.raises(ValueError, match="stage 0"):
        build_swin("swin_tiny", input_shape=(200, 200, 3))          # 50 x 50 is no multiple of 7
    with pytest.raises(ValueError, match="stage 1"):
        build_swin("swin_micro", input_shape=(48, 48, 3))           # 12 x 12 is, 6 x 6 is not a multiple of 4
    with pytest.raises(ValueError, match="patch"):
        build_swin("swin_micro", input_shape=(30, 32, 3))
    assert set(SWIN) == {"swin_tiny", "swin_small", "swin_base", "swin_large", "swin_micro"}


def test_keras_json_round_trips_swin_micro_with_its_own_classes():
    g = build_model("swin_micro")
    s = to_keras_json(g)
    layers = {ld["name"]: ld for ld in json.loads(s)["config"]["layers"]}
    assert layers["swin_micro_stage_0_block_1_attn"]["class_name"] == "WindowAttention"
    assert layers["swin_micro_stage_0_block_1_attn"]["config"]["window_size"] == 4
    assert layers["swin_micro_stage_0_block_1_attn"]["config"]["shift_size"] == 2
    assert layers["swin_micro_stage_1_merge"]["class_name"] == "SpaceToDepth"
    assert json.loads(from_keras_json(s).to_json()) == json.loads(g.to_json())


def test_keras_json_refuses_a_window_that_does_not_divide_the_map_by_layer_name():
    g = build_model("swin_micro")
    d = json.loads(to_keras_json(g))
    for ld in d["config"]["layers"]:
        if ld["name"] == "swin_micro_stage_0_block_0_attn":
            ld["config"]["window_size"] = 3
    with pytest.raises(ValueError, match="swin_micro_stage_0_block_0_attn"):
        from_keras_json(json.dumps(d))


# ------------------------------------------------------------------ native CPU path and slicing
def _noisy(w):
    """Biases and tables of O(1), as tests/test_vit_gpu.py does: a dropped or misplaced one must show."""
    for n in list(w):
        if n.endswith("/bias") or n.endswith("bias_table"):
            w[n] = np.random.default_rng(len(n)).standard_normal(w[n].shape).astype(np.float32) * 0.5
    return w


def _float64_logits(g, w, x):
    """The oracle in float64 up to the classifier's input, and the classifier in numpy float64."""
    w64 = {k: np.asarray(v, np.float64) for k, v in w.items()}
    feat_name = g.layers[g.output].inputs[0]
    ref = ReferenceExecutor(g, w64, device="cpu", dtype=torch.float64)
    feat = ref.run({g.input: torch.from_numpy(x).double()}, outputs=[feat_name])[feat_name]
    return feat.numpy() @ w64[f"{g.output}/kernel"] + w64[f"{g.output}/bias"]


@pytest.fixture(scope="module")
def micro():
    g = build_model("swin_micro", classes=10)
    w = _noisy(init_weights(g, 0))
    x = np.random.default_rng(1).standard_normal((2, 32, 32, 3)).astype(np.float32)
    return g, w, x, _float64_logits(g, w, x)


def test_cpu_executor_runs_the_plan_of_section_3_within_1e_5_of_float64(micro):
    g, w, x, want = micro
    ex = cpu_executor.CpuExecutor(g, w)
    kinds = [st.kind for st in ex.steps]
    assert kinds == (["conv", "layernorm"] + BLOCK_KINDS * 2 + MERGE_KINDS + BLOCK_KINDS * 2
                     + ["layernorm", "gap", "dense"])
    qkv = next(st for st in ex.steps if st.out == "swin_micro_stage_0_block_1_attn#qkv")
    core = next(st for st in ex.steps if st.kind == "winattn" and st.ins == [qkv.out])
    proj = next(st for st in ex.steps if st.ins[0] == core.out)
    assert core.out == "swin_micro_stage_0_block_1_attn#ctx" and core.p["window"] == 4 and core.p["shift"] == 2
    assert proj.out == "swin_micro_stage_0_block_1_add1" and proj.p["residual"] == "swin_micro_stage_0_block_0_add2"
    probs = ex(x)
    rel = np.abs(ex.logits() - want).max() / np.abs(want).max()
    print(f"swin_micro CpuExecutor logits rel err vs float64 {rel:.3e}")
    assert rel <= 1e-5 and np.allclose(probs.sum(1), 1.0, atol=1e-5)


def test_a_cut_inside_a_block_is_the_two_tensor_frontier(micro):
    g, w, x, _ = micro
    parts = slicer.partition(g, [CUT])
    assert len(parts) == 2 and set(parts[1].inputs) == {CUT, "swin_micro_stage_0_block_1_add1"}
    full = cpu_executor.CpuExecutor(g, w)(x)
    vals = {g.input_names[0]: x}
    for s in parts:
        sg = slicer.subgraph(g, s)
        vals.update(cpu_executor.CpuExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
    np.testing.assert_array_equal(vals[g.output], full)


def test_auto_2_plans_swin_tiny():
    g = build_model("swin_tiny")
    cuts = AdaptConfig(part_at="auto:2", batch=32).cuts(g)
    assert len(cuts) == 1 and cuts[0] in g.layers
    parts = slicer.partition(g, cuts)
    assert len(parts) == 2 and all(p.layers for p in parts)


def test_cli_local_infer_runs_swin_micro_on_the_cpu():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", PKG, "local-infer", "--model", "swin_micro", "--device", "cpu"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
