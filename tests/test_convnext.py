"""ConvNeXt and its three layers (LayerNormalization, Dense on (H, W, C), LayerScale / StochasticDepth), the parts
that need no GPU: IR, zoo, Keras JSON, the PyTorch oracle, the launch plan, the native CPU path and slicing.

Cases and the float64 layernorm oracle: tests/layernorm_cases.py.  The HIP kernels: tests/test_layernorm_gpu.py.
"""
import itertools
import json

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import planner, slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

import layernorm_cases as LC

CUT = "convnext_micro_stage_2_block_0_layernorm"
BLOCK = "convnext_micro_stage_2_block_1"


def _rel(a, b):
    """tests/test_gconv.py's (and tests/test_cpu_native.py's) metric."""
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------ IR
def _three_layer_graph():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (8, 8, 20)}))
    g.add(Layer("ln", "layernorm", ["in"], {"epsilon": 1e-6}))
    g.add(Layer("fc", "dense", ["ln"], {"units": 12, "use_bias": True}))
    g.add(Layer("ls", "layerscale", ["fc"], {"init_values": 1e-6}))
    g.output_names = ["ls"]
    return g


def test_shapes_and_weight_specs_of_the_new_ops():
    g = _three_layer_graph()
    assert [g.layers[n].out_shape for n in g.order] == [(8, 8, 20), (8, 8, 20), (8, 8, 12), (8, 8, 12)]
    assert g.weight_specs() == [("ln/gamma", (20,)), ("ln/beta", (20,)), ("fc/kernel", (20, 12)), ("fc/bias", (12,)),
                                ("ls/gamma", (12,))]
    assert g.layer_macs("fc") == 8 * 8 * 20 * 12 and g.layer_macs("ln") == 0 and g.layer_macs("ls") == 0
    # a (C,) layernorm, the Keras flags, and the rank-1 dense, which is as it was
    h = Graph("h")
    h.add(Layer("in", "input", [], {"shape": (4, 4, 10)}))
    h.add(Layer("gap", "gap", ["in"]))
    h.add(Layer("ln", "layernorm", ["gap"], {"epsilon": 1e-3, "center": False}))
    h.add(Layer("ln2", "layernorm", ["ln"], {"epsilon": 1e-3, "scale": False}))
    h.add(Layer("fc", "dense", ["ln2"], {"units": 7, "use_bias": False}))
    assert h.layers["ln"].out_shape == (10,) and h.layers["fc"].out_shape == (7,)
    assert h.weight_specs() == [("ln/gamma", (10,)), ("ln2/beta", (10,)), ("fc/kernel", (10, 7))]
    assert h.layer_macs("fc") == 70
    w = init_weights(g, 0)
    assert 0.8 <= w["ln/gamma"].min() and w["ln/gamma"].max() <= 1.2
    assert 0.1 <= w["ls/gamma"].min() and w["ls/gamma"].max() <= 0.3            # O(1), not Keras' 1e-6
    costs = planner.layer_costs(g, batch=2)
    assert costs["ls"] == 0.0 and costs["ln"] > 0.0


# ------------------------------------------------------------------ zoo
@pytest.mark.parametrize("name,params", [("convnext_tiny", 28_589_128), ("convnext_small", 50_223_688),
                                         ("convnext_base", 88_591_464), ("convnext_large", 197_767_336),
                                         ("convnext_xlarge", 350_196_968)])
def test_convnext_parameter_totals(name, params):
    g = build_model(name)
    assert g.count_params() == params
    assert g.layers[g.input].out_shape == (224, 224, 3) and g.layers[g.output].out_shape == (1000,)


def test_convnext_tiny_first_block_names_and_weight_order():
    g = build_model("convnext_tiny")
    assert g.order[:3] == ["input_1", "convnext_tiny_stem_conv", "convnext_tiny_stem_layernorm"]
    b = "convnext_tiny_stage_0_block_0"
    block = [f"{b}_{s}" for s in ("depthwise_conv", "layernorm", "pointwise_conv_1", "gelu", "pointwise_conv_2",
                                  "layer_scale", "identity")]
    assert g.order[3:10] == block
    assert g.layers[g.order[10]].op == "add" and g.layers[g.order[10]].inputs == ["convnext_tiny_stem_layernorm",
                                                                                 f"{b}_identity"]
    assert [g.layers[n].op for n in block] == ["conv", "layernorm", "dense", "act", "dense", "layerscale", "identity"]
    assert g.weight_specs(block) == [
        (f"{b}_depthwise_conv/kernel", (7, 7, 1, 96)), (f"{b}_depthwise_conv/bias", (96,)),
        (f"{b}_layernorm/gamma", (96,)), (f"{b}_layernorm/beta", (96,)),
        (f"{b}_pointwise_conv_1/kernel", (96, 384)), (f"{b}_pointwise_conv_1/bias", (384,)),
        (f"{b}_pointwise_conv_2/kernel", (384, 96)), (f"{b}_pointwise_conv_2/bias", (96,)),
        (f"{b}_layer_scale/gamma", (96,))]
    assert g.layers[f"{b}_pointwise_conv_1"].out_shape == (56, 56, 384)
    assert g.layers[f"{b}_layernorm"].attrs["epsilon"] == 1e-6 and g.layers[f"{b}_gelu"].attrs["fn"] == "gelu"
    assert "convnext_tiny_downsampling_layernorm_0" in g.layers and "convnext_tiny_downsampling_conv_2" in g.layers
    assert g.order[-3:] == ["avg_pool", "convnext_tiny_head_layernorm", "convnext_tiny_head_dense"]
    m = build_model("convnext_micro")
    assert m.layers[m.input].out_shape == (64, 64, 3)
    assert [m.layers[f"convnext_micro_stage_{i}_block_0_depthwise_conv"].attrs["filters"] for i in range(4)] == \
        [24, 48, 96, 192]
    assert "convnext_micro_stage_2_block_1_add" in m.layers and "convnext_micro_stage_2_block_2_add" not in m.layers


# ------------------------------------------------------------------ Keras JSON
def _k2(cls, name, inbound, **cfg):
    return {"class_name": cls, "name": name, "config": dict(cfg, name=name),
            "inbound_nodes": [[[i, 0, 0, {}] for i in inbound]] if inbound else []}


def _k3(cls, name, inbound, **cfg):
    args = [{"class_name": "__keras_tensor__", "config": {"shape": [None], "dtype": "float32",
                                                         "keras_history": [i, 0, 0]}} for i in inbound]
    return {"module": "keras.layers", "class_name": cls, "name": name, "config": dict(cfg, name=name),
            "inbound_nodes": [{"args": args, "kwargs": {}}] if inbound else []}


def _keras_block(L, axis4, axis2, keras3=False):
    shape = {"batch_shape": [None, 6, 6, 8]} if keras3 else {"batch_input_shape": [None, 6, 6, 8]}
    layers = [
        L("InputLayer", "in", [], dtype="float32", **shape),
        L("LayerNormalization", "ln", ["in"], axis=axis4, epsilon=1e-6, center=True, scale=True),
        L("Dense", "pw", ["ln"], units=16, activation="linear", use_bias=True),
        L("LayerScale", "ls", ["pw"], init_values=1e-6, projection_dim=16),
        L("StochasticDepth", "sd", ["ls"], drop_path_rate=0.1),
        L("GlobalAveragePooling2D", "gap", ["sd"]),
        L("LayerNormalization", "hln", ["gap"], axis=axis2, epsilon=1e-3, center=False, scale=True),
    ]
    return json.dumps({"class_name": "Functional", "config": {"name": "blk", "layers": layers,
                                                              "input_layers": [["in", 0, 0]],
                                                              "output_layers": [["hln", 0, 0]]}})


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
@pytest.mark.parametrize("axis4,axis2", [(-1, -1), ([-1], [-1]), ([3], [1]), (3, 1)])
def test_keras_json_imports_the_convnext_classes(L, keras3, axis4, axis2):
    g = from_keras_json(_keras_block(L, axis4, axis2, keras3))
    assert [g.layers[n].op for n in g.order] == ["input", "layernorm", "dense", "layerscale", "identity", "gap",
                                                 "layernorm"]
    assert g.layers["ln"].attrs == {"epsilon": 1e-6} and g.layers["hln"].attrs == {"epsilon": 1e-3, "center": False}
    assert g.layers["pw"].out_shape == (6, 6, 16) and g.layers["hln"].out_shape == (16,)
    assert g.weight_specs() == [("ln/gamma", (8,)), ("ln/beta", (8,)), ("pw/kernel", (8, 16)), ("pw/bias", (16,)),
                                ("ls/gamma", (16,)), ("hln/gamma", (16,))]
    m = Model.from_keras_json(_keras_block(L, axis4, axis2, keras3), seed=2)
    x = np.random.default_rng(0).standard_normal((2, 6, 6, 8)).astype(np.float32)
    want = ReferenceExecutor(m.graph, m.weights)(torch.from_numpy(x)).numpy()
    assert _rel(m.predict(x, device="cpu"), want) < 1e-4


@pytest.mark.parametrize("axis", [[1], 2, [1, 2, 3], [-2]])
def test_keras_json_rejects_layernorm_over_another_axis(axis):
    with pytest.raises(NotImplementedError, match="'?ln'?.*LayerNormalization|LayerNormalization.*ln"):
        from_keras_json(_keras_block(_k2, axis, -1))


def test_keras_json_round_trips_convnext_micro():
    g = build_model("convnext_micro")
    s = to_keras_json(g)
    classes = {ld["name"]: ld["class_name"] for ld in json.loads(s)["config"]["layers"]}
    b = "convnext_micro_stage_0_block_0"
    assert classes[f"{b}_layernorm"] == "LayerNormalization" and classes[f"{b}_layer_scale"] == "LayerScale"
    assert classes[f"{b}_pointwise_conv_1"] == "Dense" and classes[f"{b}_depthwise_conv"] == "Conv2D"
    assert json.loads(from_keras_json(s).to_json()) == json.loads(g.to_json())


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("c", LC.CASES, ids=str)
def test_reference_executor_layernorm_matches_float64_oracle(c):
    k = LC.case(c)
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (k.C,)}))
    a = {"epsilon": k.eps}
    if not k.center:
        a["center"] = False
    if not k.scale:
        a["scale"] = False
    g.add(Layer("ln", "layernorm", ["in"], a))
    g.output_names = ["ln"]
    w = {n: v for n, v in (("ln/gamma", k.gamma), ("ln/beta", k.beta)) if v is not None}
    assert [n for n, _ in g.weight_specs()] == list(w)
    got = ReferenceExecutor(g, w)(torch.from_numpy(k.x)).numpy().astype(np.float64)
    err = np.abs(got - k.want).max()
    print(f"reference layernorm {c}: max err {err:.3e}, allowance {k.allow:.3e}")
    assert err <= k.allow


def test_one_pass_variance_would_fail_the_allowance():
    """The allowance separates the two-pass form from E[x^2] - mu^2 on the cancellation probes."""
    for c in (LC.CASES[3], LC.CASES[4]):
        k = LC.case(c)
        x = k.x.astype(np.float32)
        mu = x.mean(-1, keepdims=True, dtype=np.float32)
        var = (x * x).mean(-1, keepdims=True, dtype=np.float32) - mu * mu
        y = (x - mu) / np.sqrt(np.maximum(var, 0) + np.float32(k.eps)) * k.gamma + k.beta
        assert np.abs(y.astype(np.float64) - k.want).max() > 4 * k.allow


# ------------------------------------------------------------------ plan
@pytest.fixture(scope="module")
def micro():
    g = build_model("convnext_micro", classes=10)
    w = init_weights(g, 0)
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(1))
    return g, w, x, ReferenceExecutor(g, w)(x)


@pytest.mark.parametrize("fp32,device_fusions", [(True, True), (True, False), (False, True)])
def test_convnext_block_is_five_steps(fp32, device_fusions):
    g = build_model("convnext_micro")
    steps = compile_plan(g, fp32=fp32, device_fusions=device_fusions)
    i = next(j for j, st in enumerate(steps) if st.p.get("conv") == f"{BLOCK}_depthwise_conv")
    blk = steps[i:i + 5]
    assert [st.kind for st in blk] == ["dwconv", "layernorm", "conv", "act", "conv"]
    assert blk[0].p["kernel"] == (7, 7) and blk[0].p["pads"] == ((3, 3), (3, 3)) and blk[0].p["relu"] == 0
    assert blk[1].p == {"layer": f"{BLOCK}_layernorm", "eps": 1e-6} and blk[1].covers == [f"{BLOCK}_layernorm"]
    assert blk[2].p["dense"] and blk[2].p["kernel"] == (1, 1) and blk[2].p["filters"] == 384 and not blk[2].p["residual"]
    assert blk[3].p["mode"] == 8 and blk[3].covers == [f"{BLOCK}_gelu"]
    last = blk[4]
    assert last.covers == [f"{BLOCK}_pointwise_conv_2", f"{BLOCK}_layer_scale", f"{BLOCK}_identity", f"{BLOCK}_add"]
    assert last.p["residual"] == "convnext_micro_stage_2_block_0_add" and last.p["scale"] == f"{BLOCK}_layer_scale"
    assert last.out == f"{BLOCK}_add" and last.ins == [f"{BLOCK}_gelu", "convnext_micro_stage_2_block_0_add"]
    kinds = [st.kind for st in steps if st.kind != "pack"]
    # stem conv + layernorm, 5 blocks of 5, 3 x (layernorm, conv) downsampling, gap, head layernorm, dense
    assert kinds == (["conv", "layernorm"] + ["dwconv", "layernorm", "conv", "act", "conv"]
                     + (["layernorm", "conv"] + ["dwconv", "layernorm", "conv", "act", "conv"]) * 2
                     + ["dwconv", "layernorm", "conv", "act", "conv"]
                     + ["layernorm", "conv"] + ["dwconv", "layernorm", "conv", "act", "conv"]
                     + ["gap", "layernorm", "dense"])
    assert not any(st.p.get("sibling") for st in steps)


def test_layerscale_is_not_folded_past_a_cut_that_exposes_it():
    g = build_model("convnext_micro")
    ls = f"{BLOCK}_layer_scale"
    steps = compile_plan(g, outputs=[ls, g.output], fp32=True)
    by_out = {st.out: st for st in steps}
    assert ls in by_out                                     # the step list still produces it
    cv = by_out[ls]
    assert cv.kind == "conv" and cv.covers == [f"{BLOCK}_pointwise_conv_2", ls] and not cv.p["residual"]
    add = by_out[f"{BLOCK}_add"]
    assert add.kind == "add" and set(add.ins) == {ls, "convnext_micro_stage_2_block_0_add"}
    # a cut that exposes the raw conv output leaves the scale as an affine step
    steps = compile_plan(g, outputs=[f"{BLOCK}_pointwise_conv_2", g.output], fp32=True)
    by_out = {st.out: st for st in steps}
    assert by_out[f"{BLOCK}_pointwise_conv_2"].kind == "conv" and "scale" not in by_out[f"{BLOCK}_pointwise_conv_2"].p
    assert by_out[ls].kind == "affine" and by_out[ls].p == {"layer": ls}


def _dw_graph(groups, cin=24, filters=24):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (9, 7, cin)}))
    g.add(Layer("dw", "conv", ["in"], {"filters": filters, "kernel": (7, 7), "stride": 1, "padding": "same",
                                       "use_bias": True, "groups": groups}))
    g.output_names = ["dw"]
    return g


@pytest.mark.parametrize("fp32", [True, False])
def test_one_channel_per_group_conv_is_a_dwconv_step(fp32):
    st = [s for s in compile_plan(_dw_graph(24), fp32=fp32) if s.kind != "pack"]
    assert [s.kind for s in st] == ["dwconv"]
    assert st[0].p == {"conv": "dw", "bn": None, "relu": 0, "pads": ((3, 3), (3, 3)), "stride": 1, "kernel": (7, 7)}
    st = [s for s in compile_plan(_dw_graph(12), fp32=fp32) if s.kind != "pack"]
    assert [s.kind for s in st] == ["gconv"] and st[0].p["groups"] == 12
    # groups == cin but two filters per group (a depth multiplier) is a grouped conv, not a depthwise one
    st = [s for s in compile_plan(_dw_graph(24, filters=48), fp32=fp32) if s.kind != "pack"]
    assert [s.kind for s in st] == ["gconv"]


def test_rank3_dense_softmax_raises_by_name():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (4, 4, 8)}))
    g.add(Layer("pix_probs", "dense", ["in"], {"units": 8, "activation": "softmax"}))
    with pytest.raises(NotImplementedError, match="pix_probs"):
        compile_plan(g)


def test_resnet50_plan_is_unchanged():
    from test_gconv import R50_FP32_KINDS      # the list recorded on the parent commit of the grouped-conv change
    kinds = [s.kind for s in compile_plan(build_model("resnet50"), fp32=True)]
    assert [(k, len(list(v))) for k, v in itertools.groupby(kinds)] == R50_FP32_KINDS


# ------------------------------------------------------------------ native CPU path
@pytest.mark.parametrize("c", LC.CASES, ids=str)
def test_cpu_layernorm_matches_float64_oracle(c):
    k = LC.case(c)
    y = np.full(k.x.shape, np.nan, np.float32)
    cpu_executor.native().layernorm(k.x, k.gamma_k, k.beta_k, y, k.eps)
    err = np.abs(y.astype(np.float64) - k.want).max()
    print(f"cpu layernorm {c}: max err {err:.3e}, allowance {k.allow:.3e}")
    assert np.isfinite(y).all() and err <= k.allow


def test_cpu_executor_runs_convnext_micro(micro):
    g, w, x, want = micro
    ex = cpu_executor.CpuExecutor(g, w)
    kinds = [s.kind for s in ex.steps]
    assert kinds.count("dwconv") == 5 and kinds.count("layernorm") == 10 and "gconv" not in kinds
    assert _rel(ex(x.numpy()), want.numpy()) < 1e-4
    assert _rel(Model(g, w).predict(x.numpy(), device="cpu"), want.numpy()) < 1e-4


def test_three_layer_graph_on_cpu_with_odd_channels():
    g = _three_layer_graph()
    w = init_weights(g, 1)
    x = np.random.default_rng(2).standard_normal((2, 8, 8, 20)).astype(np.float32)
    ex = cpu_executor.CpuExecutor(g, w)
    assert [s.kind for s in ex.steps] == ["layernorm", "conv"] and ex.steps[1].p["scale"] == "ls"
    assert _rel(ex(x), ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()) < 1e-4


def test_sliced_equals_unsliced_with_a_two_tensor_frontier(micro):
    """Cut at stage 2 block 0's layernorm: the block input (the residual) crosses the cut beside it.  The cut
    falls between two steps of the unsliced plan (the layernorm and the Dense-as-conv after it), so both stages
    run the very steps of the unsliced plan on the same values and the result is bit-identical."""
    g, w, x, _ = micro
    parts = slicer.partition(g, [CUT])
    assert len(parts) == 2 and set(parts[1].inputs) == {CUT, "convnext_micro_downsampling_conv_1"}
    full = cpu_executor.CpuExecutor(g, w)(x.numpy())
    vals = {g.input_names[0]: x.numpy()}
    for s in parts:
        sg = slicer.subgraph(g, s)
        vals.update(cpu_executor.CpuExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
    np.testing.assert_array_equal(vals[g.output], full)


def test_depthwise_route_equals_the_grouped_cpu_op():
    g = _dw_graph(24)
    w = init_weights(g, 4)
    x = np.random.default_rng(3).standard_normal((2, 9, 7, 24)).astype(np.float32)
    ex = cpu_executor.CpuExecutor(g, w)
    assert [s.kind for s in ex.steps] == ["dwconv"]
    got = ex(x)
    want = np.full_like(got, np.nan)
    cpu_executor.native().gconv2d(x, w["dw/kernel"], w["dw/bias"], want, 1, 3, 3, 24, 0, 0.3)
    assert np.isfinite(want).all() and _rel(got, want) < 2e-5
