"""Vision Transformers and their two ops (`mha`: Keras MultiHeadAttention as self-attention; `posembed`: class token
+ position embedding), the parts that need no GPU: IR, zoo, Keras JSON, the PyTorch oracle, the launch plan, the
native CPU path, slicing and the command line.

The attention core itself: tests/attention_cases.py, tests/test_attention.py; on the GPU tests/test_attention_gpu.py,
tests/test_vit_gpu.py.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import planner, slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import (
    Graph, Layer, mha_projection)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    BUILDERS, build_model, build_vit)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import (
    compile_plan, tensor_shape)

PKG = "adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = "vit_micro_block_0_ln2"
BLOCK_KINDS = ["layernorm", "conv", "attention", "conv", "layernorm", "conv", "act", "conv"]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _noisy(w, scale=0.5):
    """Biases and embeddings of O(1), so that a dropped or misplaced one shows."""
    for n in list(w):
        if n.endswith("/bias") or n.endswith("/class_token") or n.endswith("/position_embedding"):
            w[n] = (np.random.default_rng(len(n)).standard_normal(w[n].shape) * scale).astype(np.float32)
    return w


# ------------------------------------------------------------------ IR
def _mha_graph(shape=(4, 4, 8), heads=2, key_dim=4, value_dim=None, use_bias=True):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": shape}))
    a = {"num_heads": heads, "key_dim": key_dim, "use_bias": use_bias}
    if value_dim:
        a["value_dim"] = value_dim
    g.add(Layer("attn", "mha", ["in"], a))
    g.output_names = ["attn"]
    return g


def test_shapes_weight_specs_and_macs_of_mha():
    g = _mha_graph((4, 4, 8), 2, 4, 3)
    assert g.layers["attn"].out_shape == (4, 4, 8)
    assert g.weight_specs() == [
        ("attn/query/kernel", (8, 2, 4)), ("attn/query/bias", (2, 4)), ("attn/key/kernel", (8, 2, 4)),
        ("attn/key/bias", (2, 4)), ("attn/value/kernel", (8, 2, 3)), ("attn/value/bias", (2, 3)),
        ("attn/attention_output/kernel", (2, 3, 8)), ("attn/attention_output/bias", (8,))]
    T, C, h, d, dv = 16, 8, 2, 4, 3
    assert g.layer_macs("attn") == T * C * h * (2 * d + dv) + T * T * h * (d + dv) + T * h * dv * C
    nb = _mha_graph((10, 8), 2, 4, use_bias=False)                  # rank-2 tokens, no biases, value_dim = key_dim
    assert nb.layers["attn"].out_shape == (10, 8)
    assert [n for n, _ in nb.weight_specs()] == [f"attn/{p}/kernel" for p in ("query", "key", "value", "attention_output")]
    assert nb.weight_specs()[2][1] == (8, 2, 4) and nb.weight_specs()[3][1] == (2, 4, 8)
    assert json.loads(Graph.from_json(g.to_json()).to_json()) == json.loads(g.to_json())
    assert planner.layer_costs(g, batch=2)["attn"] > 0.0
    w = init_weights(g, 0)
    assert all((w[n] == 0).all() for n in w if n.endswith("/bias")) and w["attn/query/kernel"].std() > 0.1


@pytest.mark.parametrize("shape,attrs", [((4, 4, 8), {"num_heads": 0, "key_dim": 4}), ((4, 4, 8), {"num_heads": 2, "key_dim": 0}),
                                         ((8,), {"num_heads": 2, "key_dim": 4})])
def test_graph_add_refuses_a_bad_mha_by_name(shape, attrs):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": shape}))
    with pytest.raises(ValueError, match="bad_attn"):
        g.add(Layer("bad_attn", "mha", ["in"], attrs))


def test_shapes_and_weight_specs_of_posembed():
    for shape in ((3, 5, 8), (1, 15, 8)):
        g = Graph("t")
        g.add(Layer("in", "input", [], {"shape": shape}))
        g.add(Layer("pe", "posembed", ["in"], {"class_token": True}))
        g.add(Layer("pn", "posembed", ["pe"], {"class_token": False}))
        assert g.layers["pe"].out_shape == (1, 16, 8) and g.layers["pn"].out_shape == (1, 16, 8)
        assert g.weight_specs() == [("pe/class_token", (1, 1, 8)), ("pe/position_embedding", (16, 8)),
                                    ("pn/position_embedding", (16, 8))]
        assert g.layer_macs("pe") == 0
    w = init_weights(g, 0)
    assert 0.01 < w["pe/position_embedding"].std() < 0.03 and w["pe/class_token"].shape == (1, 1, 8)
    x = np.random.default_rng(0).standard_normal((2, 1, 15, 8)).astype(np.float32)
    got = ReferenceExecutor(g, w).run({"in": torch.from_numpy(x)}, outputs=["pe"])["pe"].numpy()
    np.testing.assert_array_equal(got[:, 0, 0], np.broadcast_to(w["pe/class_token"][0, 0] + w["pe/position_embedding"][0],
                                                               (2, 8)))
    np.testing.assert_array_equal(got[:, 0, 1:], x[:, 0] + w["pe/position_embedding"][1:])


# ------------------------------------------------------------------ zoo
@pytest.mark.parametrize("name,params", [("vit_ti16", 5_717_416), ("vit_s16", 22_050_664), ("vit_b16", 86_567_656),
                                         ("vit_l16", 304_326_632)])
def test_vit_parameter_totals(name, params):
    g = build_model(name)
    assert g.count_params() == params
    assert g.layers[g.input].out_shape == (224, 224, 3) and g.layers[g.output].out_shape == (1000,)
    assert g.layers[f"{name}_pos_embed"].out_shape[:2] == (1, 197)


def test_vit_micro_names_and_structure():
    assert {"vit_ti16", "vit_s16", "vit_b16", "vit_l16", "vit_micro"} <= set(BUILDERS)
    g = build_model("vit_micro")
    assert g.order[:3] == ["input_1", "vit_micro_patch_embed", "vit_micro_pos_embed"]
    b = "vit_micro_block_0"
    assert g.order[3:11] == [f"{b}_{s}" for s in ("ln1", "attn", "add1", "ln2", "mlp_fc1", "mlp_gelu", "mlp_fc2", "add2")]
    assert [g.layers[n].op for n in g.order[3:11]] == ["layernorm", "mha", "add", "layernorm", "dense", "act", "dense", "add"]
    assert g.order[-4:] == ["vit_micro_ln", "vit_micro_cls", "vit_micro_flatten", "vit_micro_head"]
    assert g.layers["vit_micro_pos_embed"].out_shape == (1, 17, 64) and g.layers["vit_micro_cls"].out_shape == (1, 1, 64)
    assert g.layers[f"{b}_attn"].attrs == {"num_heads": 2, "key_dim": 32, "use_bias": True}
    assert g.layers[f"{b}_ln1"].attrs["epsilon"] == 1e-6 and g.layers[f"{b}_mlp_fc1"].out_shape == (1, 17, 128)
    assert g.layers["vit_micro_patch_embed"].attrs["kernel"] == (8, 8) and g.layers[g.input].out_shape == (32, 32, 3)
    assert build_vit("vit_micro", input_shape=(16, 24, 3)).layers["vit_micro_pos_embed"].out_shape == (1, 7, 64)
    with pytest.raises(ValueError, match="patch"):
        build_vit("vit_micro", input_shape=(30, 32, 3))


# ------------------------------------------------------------------ Keras JSON
def _kt(name):
    return {"class_name": "__keras_tensor__", "config": {"shape": [None], "dtype": "float32",
                                                          "keras_history": [name, 0, 0]}}


def _k2(cls, name, inbound, call=None, **cfg):
    """Keras 2: tensors given by keyword sit in the first inbound entry's kwargs as ["name", 0, 0]."""
    kw = {k: ([v, 0, 0] if isinstance(v, str) else v) for k, v in (call or {}).items()}
    nodes = [[[i, 0, 0, dict(kw) if j == 0 else {}] for j, i in enumerate(inbound)]] if inbound else []
    return {"class_name": cls, "name": name, "config": dict(cfg, name=name), "inbound_nodes": nodes}


def _k3(cls, name, inbound, call=None, **cfg):
    """Keras 3: tensors given by keyword sit in "kwargs" as __keras_tensor__."""
    kw = {k: (_kt(v) if isinstance(v, str) else v) for k, v in (call or {}).items()}
    return {"module": "keras.layers", "class_name": cls, "name": name, "config": dict(cfg, name=name),
            "inbound_nodes": [{"args": [_kt(i) for i in inbound], "kwargs": kw}] if inbound else []}


def _keras_attention(L, keras3=False, inbound=("ln",), call=None, **mha_cfg):
    shape = {"batch_shape": [None, 4, 4, 8]} if keras3 else {"batch_input_shape": [None, 4, 4, 8]}
    cfg = dict(num_heads=2, key_dim=4, value_dim=4, dropout=0.0, use_bias=True, output_shape=None, attention_axes=None)
    cfg.update(mha_cfg)
    layers = [
        L("InputLayer", "in", [], dtype="float32", **shape),
        L("Reshape", "tok", ["in"], target_shape=[16, 8]),
        L("LayerNormalization", "ln", ["tok"], axis=[-1], epsilon=1e-6, center=True, scale=True),
        L("LayerNormalization", "other", ["tok"], axis=[-1], epsilon=1e-3, center=True, scale=True),
        L("MultiHeadAttention", "attn", list(inbound), call=call if call is not None else {"value": "ln"}, **cfg),
        L("Add", "add", ["tok", "attn"]),
        L("Dense", "fc", ["add"], units=6, activation="linear", use_bias=True),
    ]
    return json.dumps({"class_name": "Functional", "config": {"name": "blk", "layers": layers,
                                                              "input_layers": [["in", 0, 0]],
                                                              "output_layers": [["fc", 0, 0]]}})


def _numpy_forward(w, x):
    """The block by hand in float64: LayerNormalization, Keras MultiHeadAttention(2, 4)(x, x), Add, Dense."""
    t = x.reshape(x.shape[0], 16, 8).astype(np.float64)
    mu = t.mean(-1, keepdims=True)
    y = (t - mu) / np.sqrt(((t - mu) ** 2).mean(-1, keepdims=True) + 1e-6) * w["ln/gamma"] + w["ln/beta"]
    q = (np.einsum("btc,chd->bthd", y, w["attn/query/kernel"]) + w["attn/query/bias"]) / np.sqrt(4.0)
    k = np.einsum("btc,chd->bthd", y, w["attn/key/kernel"]) + w["attn/key/bias"]
    v = np.einsum("btc,chd->bthd", y, w["attn/value/kernel"]) + w["attn/value/bias"]
    s = np.einsum("bqhd,bkhd->bhqk", q, k)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = np.einsum("bhqk,bkhd->bqhd", p, v)
    o = np.einsum("bqhd,hdc->bqc", o, w["attn/attention_output/kernel"]) + w["attn/attention_output/bias"]
    return (t + o) @ w["fc/kernel"] + w["fc/bias"]


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
@pytest.mark.parametrize("form", ["value_kw", "value_key_kw", "positional"])
def test_keras_json_imports_self_attention_on_rank2_tokens(L, keras3, form):
    inbound, call = {"value_kw": (("ln",), {"value": "ln"}),
                     "value_key_kw": (("ln",), {"value": "ln", "key": "ln", "attention_mask": None,
                                                "use_causal_mask": False, "return_attention_scores": False}),
                     "positional": (("ln", "ln"), {})}[form]
    doc = _keras_attention(L, keras3, inbound, call)
    g = from_keras_json(doc)
    assert [g.layers[n].op for n in g.order] == ["input", "reshape", "layernorm", "layernorm", "mha", "add", "dense"]
    assert g.layers["attn"].inputs == ["ln"] and g.layers["attn"].attrs == {"num_heads": 2, "key_dim": 4, "use_bias": True}
    assert g.layers["attn"].out_shape == (16, 8) and g.layers["fc"].out_shape == (16, 6)
    # the Keras 2 writer exports it, and reading that back gives the same graph
    s = to_keras_json(g)
    classes = {ld["name"]: ld["class_name"] for ld in json.loads(s)["config"]["layers"]}
    assert classes["attn"] == "MultiHeadAttention"
    assert json.loads(from_keras_json(s).to_json()) == json.loads(g.to_json())
    w = _noisy(init_weights(g, 2))
    x = np.random.default_rng(0).standard_normal((2, 4, 4, 8)).astype(np.float32)
    want = _numpy_forward(w, x)
    got = ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()
    assert got.shape == (2, 16, 6) and _rel(got, want) < 1e-5
    # the same (T, C) tensors through the plan: Dense and the projections are 1x1 conv steps, the Add a residual
    ex = cpu_executor.CpuExecutor(g, w, outputs=["fc"])
    assert [st.kind for st in ex.steps] == ["layernorm", "layernorm", "conv", "attention", "conv", "conv"]
    assert ex.steps[4].p["residual"] == "in" and ex.steps[5].p["dense"]
    assert _rel(ex(x), want) < 1e-5


def test_keras_json_round_trips_vit_micro_with_its_own_class():
    g = build_model("vit_micro")
    s = to_keras_json(g)
    classes = {ld["name"]: ld["class_name"] for ld in json.loads(s)["config"]["layers"]}
    assert classes["vit_micro_pos_embed"] == "ClassTokenPositionEmbedding"
    assert classes["vit_micro_block_1_attn"] == "MultiHeadAttention" and classes["vit_micro_cls"] == "Cropping2D"
    assert json.loads(from_keras_json(s).to_json()) == json.loads(g.to_json())


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
@pytest.mark.parametrize("why,inbound,call,cfg", [
    ("cross-attention", ("ln",), {"value": "other"}, {}),
    ("cross-attention", ("ln",), {"value": "ln", "key": "other"}, {}),
    ("cross-attention", ("ln", "other"), {}, {}),
    ("attention_mask", ("ln",), {"value": "ln", "attention_mask": "other"}, {}),
    ("use_causal_mask", ("ln",), {"value": "ln", "use_causal_mask": True}, {}),
    ("return_attention_scores", ("ln",), {"value": "ln", "return_attention_scores": True}, {}),
    ("attention_axes", ("ln",), {"value": "ln"}, {"attention_axes": [2]}),
    ("output_shape", ("ln",), {"value": "ln"}, {"output_shape": [12]}),
])
def test_keras_json_refuses_what_is_not_plain_self_attention(L, keras3, why, inbound, call, cfg):
    with pytest.raises(NotImplementedError, match=f"attn.*{why}"):
        from_keras_json(_keras_attention(L, keras3, inbound, call, **cfg))


@pytest.mark.parametrize("cfg", [{"attention_axes": [1]}, {"attention_axes": [-2]}, {"attention_axes": 1},
                                 {"output_shape": 8}, {"output_shape": [8]}])
def test_keras_json_takes_the_defaults_written_out(cfg):
    assert from_keras_json(_keras_attention(_k2, False, **cfg)).layers["attn"].op == "mha"


# ------------------------------------------------------------------ oracle and packing
def test_packed_projections_reproduce_the_reference_layer():
    """[Q | K | V] side by side with 1/sqrt(d) folded into Q, the float64 core, then the output projection."""
    import attention_cases as AC
    g = _mha_graph((3, 5, 20), 3, 6, 5)
    w = _noisy(init_weights(g, 1))
    x = np.random.default_rng(1).standard_normal((2, 3, 5, 20)).astype(np.float32)
    head = {"heads": 3, "key_dim": 6, "value_dim": 5}
    kq, bq = mha_projection(w, "attn", head, "qkv")
    ko, bo = mha_projection(w, "attn", head, "out")
    assert kq.shape == (20, 51) and bq.shape == (51,) and ko.shape == (15, 20) and bo.shape == (20,)
    qkv = x.reshape(30, 20).astype(np.float64) @ kq + bq
    ctx = AC.ref_attention(qkv, 2, 15, 3, 6, 5)
    got = (ctx @ ko + bo).reshape(2, 3, 5, 20)
    assert _rel(got, ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()) < 1e-5
    nb = _mha_graph((3, 5, 20), 3, 6, 5, use_bias=False)
    assert mha_projection(init_weights(nb, 1), "attn", head, "qkv")[1] is None


# ------------------------------------------------------------------ plan
@pytest.mark.parametrize("fp32,device_fusions", [(True, True), (True, False), (False, True)])
def test_vit_micro_plan(fp32, device_fusions):
    g = build_model("vit_micro")
    steps = [s for s in compile_plan(g, fp32=fp32, device_fusions=device_fusions) if s.kind != "pack"]
    assert [s.kind for s in steps] == ["conv", "posembed"] + BLOCK_KINDS * 2 + ["layernorm", "crop", "dense"]
    b = "vit_micro_block_1"
    i = next(j for j, s in enumerate(steps) if s.out == f"{b}_attn#qkv")
    qkv, att, proj = steps[i:i + 3]
    assert qkv.ins == [f"{b}_ln1"] and qkv.covers == [] and qkv.p["mha"] == "qkv" and qkv.p["filters"] == 2 * 3 * 32
    assert qkv.p["dense"] and qkv.p["kernel"] == (1, 1) and not qkv.p["residual"]
    assert att.kind == "attention" and att.ins == [f"{b}_attn#qkv"] and att.out == f"{b}_attn#ctx"
    assert att.p == {"layer": f"{b}_attn", "tokens": 17, "heads": 2, "key_dim": 32, "value_dim": 32}
    assert proj.out == f"{b}_add1" and proj.ins == [f"{b}_attn#ctx", "vit_micro_block_0_add2"]
    assert proj.covers == [f"{b}_attn", f"{b}_add1"] and proj.p["residual"] == "vit_micro_block_0_add2"
    assert proj.p["mha"] == "out" and proj.p["filters"] == 64
    fc2 = steps[i + 6]
    assert fc2.covers == [f"{b}_mlp_fc2", f"{b}_add2"] and fc2.p["residual"] == f"{b}_add1" and fc2.out == f"{b}_add2"
    assert not any(s.kind == "add" or s.p.get("sibling") for s in steps)
    assert tensor_shape(g, f"{b}_attn#qkv") == (1, 17, 192) and tensor_shape(g, f"{b}_attn#ctx") == (1, 17, 64)
    assert tensor_shape(g, f"{b}_attn") == (1, 17, 64)


def test_a_cut_that_exposes_the_attention_output_keeps_the_add_a_step():
    g = build_model("vit_micro")
    a = "vit_micro_block_0_attn"
    steps = compile_plan(g, outputs=[a, g.output], fp32=True)
    by_out = {s.out: s for s in steps}
    assert by_out[a].kind == "conv" and by_out[a].covers == [a] and not by_out[a].p["residual"]
    add = by_out["vit_micro_block_0_add1"]
    assert add.kind == "add" and set(add.ins) == {a, "vit_micro_pos_embed"}


def test_existing_models_plan_as_before():
    """No Dense of an existing family gained a residual, and none of their steps is of a new kind."""
    for name in ("resnet50", "convnext_micro", "unet_tiny"):
        for fp32 in (True, False):
            if name == "unet_tiny" and not fp32:
                continue
            steps = compile_plan(build_model(name), fp32=fp32)
            assert not any(s.kind in ("attention", "posembed") or s.p.get("mha") for s in steps)
    cn = compile_plan(build_model("convnext_micro"), fp32=True)
    assert all(s.p.get("scale") for s in cn if s.kind == "conv" and s.p.get("dense") and s.p.get("residual"))


# ------------------------------------------------------------------ native CPU path and slicing
@pytest.fixture(scope="module")
def micro():
    g = build_model("vit_micro", classes=10)
    w = _noisy(init_weights(g, 0))
    x = torch.randn(2, 32, 32, 3, generator=torch.Generator().manual_seed(1))
    ref = ReferenceExecutor(g, w)
    feat_name = g.layers[g.output].inputs[0]
    feat = ref.run({g.input: x}, outputs=[feat_name])[feat_name]
    return g, w, x, ref(x), feat.numpy() @ w[f"{g.output}/kernel"] + w[f"{g.output}/bias"]


def test_cpu_executor_logits_of_vit_micro_match_the_oracle(micro):
    """The README's bound for the native CPU path: logits within 1.3e-5 of the PyTorch oracle, relative to the
    largest logit."""
    g, w, x, want, want_logits = micro
    ex = cpu_executor.CpuExecutor(g, w)
    probs = ex(x.numpy())
    rel = _rel(ex.logits(), want_logits)
    print(f"vit_micro CpuExecutor logits rel err {rel:.3e}")
    assert rel <= 1.3e-5
    assert _rel(probs, want.numpy()) < 1e-4 and np.allclose(probs.sum(1), 1.0, atol=1e-5)


def test_sliced_equals_unsliced_with_a_two_tensor_frontier(micro):
    g, w, x, _, _ = micro
    parts = slicer.partition(g, [CUT])
    assert len(parts) == 2 and set(parts[1].inputs) == {CUT, "vit_micro_block_0_add1"}
    full = cpu_executor.CpuExecutor(g, w)(x.numpy())
    vals = {g.input_names[0]: x.numpy()}
    for s in parts:
        sg = slicer.subgraph(g, s)
        vals.update(cpu_executor.CpuExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
    np.testing.assert_array_equal(vals[g.output], full)


# ------------------------------------------------------------------ command line
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", PKG, *args], cwd=ROOT, env=env, capture_output=True, text=True,
                          timeout=300)


def test_cli_plans_vit_micro_in_two_stages():
    r = _cli("plan", "--model", "vit_micro", "--stages", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "vit_micro" in r.stdout


def test_cli_local_infer_runs_vit_micro_on_the_cpu():
    r = _cli("local-infer", "--model", "vit_micro", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-2000:]
