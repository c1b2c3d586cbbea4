"""Cross-attention and learned queries, the parts that need no GPU: the `mha` op with separate query / value / key
sources and the `queries` op in the IR, Keras JSON (Keras 2 and Keras 3) in and out, weight specs, the launch plan of
every source pattern, the native CPU ops against the float64 oracle of tests/cross_attention_cases.py, DETR in the
zoo (detr_micro through the CPU executor, slicing and the planner; detr_resnet50's parameter total), and the plans of
the older families unchanged.

The HIP kernels: tests/test_cross_attention_gpu.py, tests/test_guard_cross_attention_gpu.py.
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
    DETR, DETR_CLASSES, build_model)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import (
    compile_plan, tensor_shape)

import cross_attention_cases as XC

PKG = "adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_steps_before_cross_attention.json")
ENC_CUT, DEC_CUT = "encoder_0_ln_attn", "decoder_0_ln_self"


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _noisy(w, scale=0.5):
    """Biases of O(1), so that a dropped or misplaced one shows."""
    for n in list(w):
        if n.endswith("/bias"):
            w[n] = (np.random.default_rng(len(n)).standard_normal(w[n].shape) * scale).astype(np.float32)
    return w


def _graph(inputs=("q", "v", "k"), q=(10, 8), v=(7, 12), k=(7, 6), **attrs):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (4, 4, 3)}))
    for n, shp in (("q", q), ("v", v), ("k", k)):
        g.add(Layer(n, "input", [], {"shape": shp}))
    g.add(Layer("attn", "mha", list(inputs), dict({"num_heads": 2, "key_dim": 4, "value_dim": 3}, **attrs)))
    g.output_names = ["attn"]
    return g


# ------------------------------------------------------------------ IR
def test_shapes_weight_specs_and_macs_follow_each_source():
    g = _graph()
    assert g.layers["attn"].out_shape == (10, 8)
    assert g.weight_specs(["attn"]) == [
        ("attn/query/kernel", (8, 2, 4)), ("attn/query/bias", (2, 4)), ("attn/key/kernel", (6, 2, 4)),
        ("attn/key/bias", (2, 4)), ("attn/value/kernel", (12, 2, 3)), ("attn/value/bias", (2, 3)),
        ("attn/attention_output/kernel", (2, 3, 8)), ("attn/attention_output/bias", (8,))]
    Tq, Tk, h, d, dv = 10, 7, 2, 4, 3
    assert g.layer_macs("attn") == (Tq * 8 * h * d + Tk * 6 * h * d + Tk * 12 * h * dv + Tq * Tk * h * (d + dv)
                                    + Tq * h * dv * 8)
    # a missing key is the value: its kernel follows the value's channels
    kv = _graph(("q", "v"))
    assert dict(kv.weight_specs(["attn"]))["attn/key/kernel"] == (12, 2, 4)
    w = init_weights(g, 0)
    assert w["attn/key/kernel"].shape == (6, 2, 4) and w["attn/value/kernel"].shape == (12, 2, 3)
    assert planner.layer_costs(g, batch=2)["attn"] > 0.0
    assert json.loads(Graph.from_json(g.to_json()).to_json()) == json.loads(g.to_json())
    # rank-3 maps count all positions
    m = _graph(q=(2, 5, 8), v=(7, 1, 12), k=(1, 7, 6))
    assert m.layers["attn"].out_shape == (2, 5, 8)


@pytest.mark.parametrize("kw,word", [
    (dict(v=(7, 12), k=(6, 6)), "tokens"),                          # value and key token counts differ
    (dict(v=(12,)), "rank"),                                        # ranks other than 2 / 3
    (dict(q=(2, 2, 5, 8)), "rank"),
    (dict(output_shape=[12]), "output_shape"),                      # not the query's channel count
    (dict(inputs=("q", "v", "k", "q")), "rank"),                    # more than three inputs
])
def test_graph_add_refuses_a_bad_cross_attention_by_name(kw, word):
    with pytest.raises(ValueError, match=f"attn.*{word}"):
        _graph(**kw)
    assert _graph(output_shape=[8]).layers["attn"].out_shape == (10, 8)


def test_projection_parts_stand_side_by_side_with_the_scale_in_q():
    g = _graph(("q", "q", "q"), q=(10, 8))
    w = _noisy(init_weights(g, 1))
    head = {"heads": 2, "key_dim": 4, "value_dim": 3}
    full, bias = mha_projection(w, "attn", head, "qkv")
    cols = {"q": (0, 8), "k": (8, 16), "v": (16, 22), "qk": (0, 16), "kv": (8, 22), "qkv": (0, 22)}
    for part, (a, b) in cols.items():
        kern, bs = mha_projection(w, "attn", head, part)
        np.testing.assert_array_equal(kern, full[:, a:b])
        np.testing.assert_array_equal(bs, bias[a:b])
    np.testing.assert_allclose(full[:, :8], w["attn/query/kernel"].reshape(8, 8) / 2.0, rtol=1e-6)


def test_queries_op():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (4, 4, 3)}))
    g.add(Layer("qe", "queries", ["in"], {"length": 5, "dim": 6, "initializer": "normal"}))
    g.add(Layer("z", "queries", ["in"], {"length": 5, "dim": 6, "initializer": "zeros"}))
    g.add(Layer("sum", "add", ["qe", "z"]))
    g.output_names = ["sum"]
    assert g.layers["qe"].out_shape == (1, 5, 6) and g.weight_specs(["qe"]) == [("qe/embeddings", (5, 6))]
    w = init_weights(g, 0)
    assert (w["z/embeddings"] == 0).all() and 0.5 < w["qe/embeddings"].std() < 1.5
    assert planner.layer_costs(g, batch=2)["qe"] > 0.0
    for bad in ({"length": 0, "dim": 6}, {"length": 5, "dim": 6, "initializer": "ones"}):
        with pytest.raises(ValueError, match="bad_q"):
            g.add(Layer("bad_q", "queries", ["in"], bad))
    steps = compile_plan(g, fp32=True, device_fusions=False)
    assert [s.kind for s in steps] == ["queries", "queries", "add"]
    x = np.zeros((3, 4, 4, 3), np.float32)
    want = ReferenceExecutor(g, w).run({"in": torch.from_numpy(x)}, outputs=["qe", "sum"])
    got = cpu_executor.CpuExecutor(g, w, outputs=["qe", "sum"]).run({"in": x})
    assert got["qe"].shape == (3, 1, 5, 6)
    for n in ("qe", "sum"):                                 # a copy: bit-exact, the same for every image
        np.testing.assert_array_equal(got[n], want[n].numpy())
        np.testing.assert_array_equal(got[n], np.broadcast_to(w["qe/embeddings"], (3, 1, 5, 6)))
    s = to_keras_json(g)
    assert {ld["name"]: ld["class_name"] for ld in json.loads(s)["config"]["layers"]}["qe"] == "LearnedQueries"
    assert json.loads(from_keras_json(s, cross_attention=True).to_json()) == json.loads(g.to_json())


# ------------------------------------------------------------------ Keras JSON
def _k2(cls, name, inbound, call=None, **cfg):
    first = dict((k, [v, 0, 0] if isinstance(v, str) else v) for k, v in (call or {}).items())
    nodes = [[[i, 0, 0, first if j == 0 else {}] for j, i in enumerate(inbound)]] if inbound else []
    return {"class_name": cls, "name": name, "config": dict(cfg, name=name), "inbound_nodes": nodes}


def _kt(name):
    return {"class_name": "__keras_tensor__", "config": {"shape": [None], "dtype": "float32",
                                                         "keras_history": [name, 0, 0]}}


def _k3(cls, name, inbound, call=None, **cfg):
    kw = {k: (_kt(v) if isinstance(v, str) else v) for k, v in (call or {}).items()}
    return {"module": "keras.layers", "class_name": cls, "name": name, "config": dict(cfg, name=name),
            "inbound_nodes": [{"args": [_kt(i) for i in inbound], "kwargs": kw}] if inbound else []}


def _keras_block(L, keras3, inbound, call, **mha_cfg):
    """tok (16, 8) is the query; mem (16, 6) and memk (16, 8) are other tensors of the same 16 positions."""
    shape = {"batch_shape": [None, 4, 4, 8]} if keras3 else {"batch_input_shape": [None, 4, 4, 8]}
    cfg = dict(num_heads=2, key_dim=4, value_dim=4, dropout=0.0, use_bias=True, output_shape=None, attention_axes=None)
    cfg.update(mha_cfg)
    layers = [
        L("InputLayer", "in", [], dtype="float32", **shape),
        L("Reshape", "tok", ["in"], target_shape=[16, 8]),
        L("Dense", "mem", ["tok"], units=6, activation="linear", use_bias=True),
        L("LayerNormalization", "memk", ["tok"], axis=[-1], epsilon=1e-3, center=True, scale=True),
        L("MultiHeadAttention", "attn", list(inbound), call=call, **cfg),
        L("Add", "add", ["tok", "attn"]),
    ]
    return json.dumps({"class_name": "Functional", "config": {"name": "blk", "layers": layers,
                                                              "input_layers": [["in", 0, 0]],
                                                              "output_layers": [["add", 0, 0]]}})


def _numpy_block(w, x):
    """The block by hand in float64: MultiHeadAttention(2, 4)(tok, mem, key=memk), Add."""
    t = x.reshape(x.shape[0], 16, 8).astype(np.float64)
    mem = t @ w["mem/kernel"] + w["mem/bias"]
    mu = t.mean(-1, keepdims=True)
    memk = (t - mu) / np.sqrt(((t - mu) ** 2).mean(-1, keepdims=True) + 1e-3) * w["memk/gamma"] + w["memk/beta"]
    q = (np.einsum("btc,chd->bthd", t, w["attn/query/kernel"]) + w["attn/query/bias"]) / np.sqrt(4.0)
    k = np.einsum("btc,chd->bthd", memk, w["attn/key/kernel"]) + w["attn/key/bias"]
    v = np.einsum("btc,chd->bthd", mem, w["attn/value/kernel"]) + w["attn/value/bias"]
    s = np.einsum("bqhd,bkhd->bhqk", q, k)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = np.einsum("bhqk,bkhd->bqhd", p, v)
    return t + np.einsum("bqhd,hdc->bqc", o, w["attn/attention_output/kernel"]) + w["attn/attention_output/bias"]


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
@pytest.mark.parametrize("form", ["kwargs", "positional"])
def test_keras_json_imports_a_cross_attention_call_and_round_trips(L, keras3, form):
    """The parent refuses this call with NotImplementedError ("cross-attention ... only self-attention")."""
    inbound, call = {"kwargs": (("tok",), {"value": "mem", "key": "memk", "attention_mask": None}),
                     "positional": (("tok", "mem", "memk"), {})}[form]
    g = from_keras_json(_keras_block(L, keras3, inbound, call), cross_attention=True)
    assert g.layers["attn"].inputs == ["tok", "mem", "memk"] and g.layers["attn"].out_shape == (16, 8)
    assert dict(g.weight_specs(["attn"]))["attn/value/kernel"] == (6, 2, 4)
    s = to_keras_json(g)
    entry = json.loads(s)["config"]["layers"][4]["inbound_nodes"][0][0]
    assert entry[0] == "tok" and entry[3] == {"value": ["mem", 0, 0], "key": ["memk", 0, 0]}
    assert json.loads(from_keras_json(s, cross_attention=True).to_json()) == json.loads(g.to_json())
    w = _noisy(init_weights(g, 2))
    x = np.random.default_rng(0).standard_normal((2, 4, 4, 8)).astype(np.float32)
    want = _numpy_block(w, x)
    assert _rel(ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy(), want) < 1e-5
    ex = cpu_executor.CpuExecutor(g, w)
    assert [st.out for st in ex.steps if "#" in st.out] == ["attn#q", "attn#k", "attn#v", "attn#ctx"]
    assert _rel(ex(x), want) < 1e-5


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_keras_json_key_defaults_to_the_value_and_both_forms_are_written_back(L, keras3):
    g = from_keras_json(_keras_block(L, keras3, ("tok",), {"value": "mem"}), cross_attention=True)
    assert g.layers["attn"].inputs == ["tok", "mem"]
    s = to_keras_json(g)
    assert json.loads(s)["config"]["layers"][4]["inbound_nodes"][0][0][3] == {"value": ["mem", 0, 0]}
    assert json.loads(from_keras_json(s, cross_attention=True).to_json()) == json.loads(g.to_json())
    # a key written out as the value, and a call whose three tensors are one, stay what they were
    same_key = from_keras_json(_keras_block(L, keras3, ("tok",), {"value": "mem", "key": "mem"}), cross_attention=True)
    assert same_key.layers["attn"].inputs == ["tok", "mem"]
    one = from_keras_json(_keras_block(L, keras3, ("tok",), {"value": "tok", "key": "tok"}), cross_attention=True)
    assert one.layers["attn"].inputs == ["tok"]


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_the_importer_reads_cross_attention_on_request_and_the_model_loader_requests_it(L, keras3):
    """`from_keras_json` keeps refusing such a call by layer name unless asked (its contract before the `mha` op
    took separate sources); `Model.from_keras_json`, which the command line uses, asks."""
    from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
    doc = _keras_block(L, keras3, ("tok",), {"value": "mem", "key": "memk"})
    with pytest.raises(NotImplementedError, match="attn.*cross-attention.*cross_attention=True"):
        from_keras_json(doc)
    m = Model.from_keras_json(doc, seed=2)
    assert m.graph.layers["attn"].inputs == ["tok", "mem", "memk"]
    x = np.random.default_rng(0).standard_normal((2, 4, 4, 8)).astype(np.float32)
    assert _rel(m.predict(x, device="cpu"), _numpy_block(m.weights, x)) < 1e-5


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
@pytest.mark.parametrize("why,call,cfg", [
    ("attention_mask", {"value": "mem", "attention_mask": "memk"}, {}),
    ("use_causal_mask", {"value": "mem", "use_causal_mask": True}, {}),
    ("return_attention_scores", {"value": "mem", "return_attention_scores": True}, {}),
    ("attention_axes", {"value": "mem"}, {"attention_axes": [2]}),
    ("output_shape", {"value": "mem"}, {"output_shape": [6]}),          # the value's width is not the query's
])
def test_keras_json_still_refuses_masks_scores_and_partial_axes(L, keras3, why, call, cfg):
    with pytest.raises(NotImplementedError, match=f"attn.*{why}"):
        from_keras_json(_keras_block(L, keras3, ("tok",), call, **cfg), cross_attention=True)


# ------------------------------------------------------------------ plan
def _pattern_graph(pattern):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (1, 6, 8)}))
    g.add(Layer("a", "layernorm", ["in"], {"epsilon": 1e-5}))
    g.add(Layer("b", "dense", ["in"], {"units": 12, "use_bias": True}))
    g.add(Layer("c", "dense", ["in"], {"units": 8, "use_bias": True}))
    ins = {"qkv": ["a", "a", "a"], "qk_v": ["a", "b", "a"], "q_kv": ["a", "b"], "q_k_v": ["a", "b", "c"]}[pattern]
    g.add(Layer("attn", "mha", ins, {"num_heads": 2, "key_dim": 4, "value_dim": 3, "use_bias": True}))
    g.add(Layer("sum", "add", ["in", "attn"]))
    g.output_names = ["sum"]
    return g


@pytest.mark.parametrize("fp32,device_fusions", [(True, True), (True, False), (False, True)])
@pytest.mark.parametrize("pattern,parts", [("qkv", ["qkv"]), ("qk_v", ["qk", "v"]), ("q_kv", ["q", "kv"]),
                                           ("q_k_v", ["q", "k", "v"])])
def test_the_step_list_of_each_source_pattern(pattern, parts, fp32, device_fusions):
    g = _pattern_graph(pattern)
    steps = [s for s in compile_plan(g, fp32=fp32, device_fusions=device_fusions) if "attn" in s.out or s.out == "sum"]
    assert [s.out for s in steps] == [f"attn#{p}" for p in parts] + ["attn#ctx", "sum"]
    h, d, dv = 2, 4, 3
    width = {"q": h * d, "k": h * d, "v": h * dv}
    # (query, key, value) sources; the layer's inputs are in Keras' order, [query, value, key]
    src = dict(zip("qkv", {"qkv": "aaa", "qk_v": "aab", "q_kv": "abb", "q_k_v": "acb"}[pattern]))
    for s, part in zip(steps, parts):
        assert s.kind == "conv" and s.p["mha"] == part and s.p["dense"] and s.covers == [] and not s.p["residual"]
        assert s.ins == [src[part[0]]] and s.p["filters"] == sum(width[c] for c in part)
        assert tensor_shape(g, s.out) == (1, 6, s.p["filters"])
    att, out = steps[-2:]
    assert att.kind == "attention" and att.ins == [f"attn#{p}" for p in parts] and att.covers == []
    if pattern == "qkv":                                    # one source: exactly the self-attention step
        assert att.p == {"layer": "attn", "tokens": 6, "heads": h, "key_dim": d, "value_dim": dv}
    else:
        assert att.p["tokens_q"] == 6 and att.p["tokens_k"] == 6
        where = {}
        for j, part in enumerate(parts):
            col = 0
            for c in part:
                where[c] = (j, col)
                col += width[c]
        assert {c: tuple(att.p[c]) for c in "qkv"} == where
    assert out.kind == "conv" and out.p["mha"] == "out" and out.p["residual"] == "in" and out.covers == ["attn", "sum"]
    assert tensor_shape(g, "attn#ctx") == (1, 6, h * dv)
    # and it computes what the oracle computes
    if fp32 and not device_fusions:
        w = _noisy(init_weights(g, 3))
        x = np.random.default_rng(1).standard_normal((2, 1, 6, 8)).astype(np.float32)
        assert _rel(cpu_executor.CpuExecutor(g, w)(x), ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()) < 1e-5


def test_key_tokens_come_from_the_key_source():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (1, 5, 8)}))
    g.add(Layer("mem", "input", [], {"shape": (3, 3, 6)}))
    g.add(Layer("attn", "mha", ["in", "mem"], {"num_heads": 2, "key_dim": 4}))
    g.output_names = ["attn"]
    steps = compile_plan(g, fp32=True, device_fusions=False)
    assert [s.out for s in steps] == ["attn#q", "attn#kv", "attn#ctx", "attn"]
    assert steps[2].p["tokens_q"] == 5 and steps[2].p["tokens_k"] == 9
    assert tensor_shape(g, "attn#kv") == (1, 9, 16) and tensor_shape(g, "attn#q") == (1, 5, 8)
    w = _noisy(init_weights(g, 0))
    rng = np.random.default_rng(0)
    x = {"in": rng.standard_normal((2, 1, 5, 8)).astype(np.float32), "mem": rng.standard_normal((2, 3, 3, 6)).astype(np.float32)}
    want = ReferenceExecutor(g, w).run({n: torch.from_numpy(v) for n, v in x.items()})["attn"].numpy()
    assert _rel(cpu_executor.CpuExecutor(g, w).run(x)["attn"], want) < 1e-5


# ------------------------------------------------------------------ the native CPU op
def test_the_cases_meet_every_path_layout_and_tail():
    QT, KT = XC.QT, XC.KT
    assert QT % 16 == 0 and KT % 16 == 0
    mfma = [c for c in XC.CASES if XC.expected_path(c) == "mfma"]
    plain = [c for c in XC.CASES if XC.expected_path(c) == "plain"]
    assert {(c[4], c[5]) for c in mfma} >= {(16, 16), (32, 16), (64, 64), (128, 128)}
    assert {(c[4], c[5]) for c in plain} >= {(24, 24), (8, 40), (6, 5)}
    assert any(c[7] == "k_off2" and c[4] % 16 == 0 and c[5] % 16 == 0 for c in plain)
    assert {c[6] for c in mfma} == {"split", "q_kv", "qk_v"} == {c[6] for c in plain}
    assert all(c[1] == c[2] for c in XC.CASES if c[6] == "qk_v")
    assert any(c[2] == 1 for c in mfma) and any(c[1] == 1 and c[2] == 2 * KT + 6 for c in mfma)
    assert {c[2] for c in mfma if c[1] == 5} >= {KT - 1, KT, KT + 1}
    assert {c[1] for c in mfma if c[2] == 5} >= {QT - 1, QT, QT + 1}
    assert (1, 100, 300, 2, 32, 32, "split", None) in XC.CASES
    off = [c for c in mfma if c[0] > 1 and c[1] % QT and c[1] % KT and c[2] % QT and c[2] % KT and c[1] != c[2]]
    assert {c[0] for c in off} >= {2, 3} and any(c[1] > c[2] for c in off) and any(c[1] < c[2] for c in off)
    probes = [c for c in XC.CASES if c[7] in ("ascending", "descending", "dominant")]
    assert {c[7] for c in probes} == {"ascending", "descending", "dominant"}
    for c in probes:
        k = XC.case(c)
        s = np.einsum("bqhd,bkhd->bhqk", k.q.astype(np.float64), k.k.astype(np.float64))
        assert k.Tq != k.Tk and k.Tk > 2 * KT and 80 < s.max() < 130
        arg = s.argmax(-1)
        if c[7] == "ascending":
            assert (arg >= 2 * KT).all()
        elif c[7] == "descending":
            assert (arg < KT).all()
        else:
            assert len(np.unique(arg // KT)) == 3
    g = XC.GUARD_CASES
    assert set(g) <= set(XC.CASES) and {c[6] for c in g} == {"split", "q_kv", "qk_v"}
    assert {XC.expected_path(c) for c in g} == {"mfma", "plain"} and any(c[0] > 1 for c in g) and any(c[2] == 1 for c in g)


@pytest.mark.parametrize("c", XC.CASES, ids=str)
def test_cpu_cross_attention_matches_float64_oracle(c):
    k = XC.case(c)
    q, kk, v, _ = XC.views(k, lambda t, name: t)                    # the layout's views, NaN in every surplus
    y = np.full((k.B * k.Tq, k.w_out + 3), np.nan, np.float32)
    cpu_executor.native().cross_attention(q.numpy(), kk.numpy(), v.numpy(), y, k.B, k.Tq, k.Tk, k.heads, k.d, k.dv)
    err = np.abs(y[:, :k.w_out].astype(np.float64) - k.want).max()
    print(f"cpu cross_attention {c} [{k.path}]: e_ref {k.e_ref:.3e}, max err {err:.3e}, allowance {k.allow:.3e}")
    assert np.isfinite(y).all() and (y[:, k.w_out:] == 0).all() and err <= k.allow


def test_cpu_cross_attention_refuses_rows_that_do_not_fit():
    k = XC.case(XC.CASES[0])
    q, kk, v = (t.reshape(t.shape[0] * t.shape[1], -1) for t in (k.q, k.k, k.v))
    y = np.empty((k.B * k.Tq, k.w_out), np.float32)
    with pytest.raises(Exception):
        cpu_executor.native().cross_attention(q[:, :-1].copy(), kk, v, y, k.B, k.Tq, k.Tk, k.heads, k.d, k.dv)
    with pytest.raises(Exception):
        cpu_executor.native().cross_attention(q, kk, v, y, k.B, k.Tq, k.Tk + 1, k.heads, k.d, k.dv)


# ------------------------------------------------------------------ DETR
@pytest.fixture(scope="module")
def micro():
    g = build_model("detr_micro")
    w = _noisy(init_weights(g, 0))
    x = torch.randn(2, 40, 56, 3, generator=torch.Generator().manual_seed(1))
    return g, w, x, ReferenceExecutor(g, w)(x).numpy()


def test_detr_micro_graph():
    g = build_model("detr_micro")
    assert g.layers["src"].out_shape == (1, 35, 32) and g.layers["pos"].out_shape == (1, 35, 32)
    assert g.layers["query_embed"].out_shape == (1, 10, 32) and g.layers["tgt"].attrs["initializer"] == "zeros"
    assert g.layers["encoder_1_attn"].inputs == ["encoder_1_qk", "encoder_0_ln_ffn", "encoder_1_qk"]
    assert g.layers["decoder_1_cross_attn"].inputs == ["decoder_1_cross_q", "encoder_1_ln_ffn", "memory_pos"]
    assert g.layers["detections"].out_shape == (1, 10, DETR_CLASSES + 4) and g.output_names == ["detections"]
    outs = [s.out for s in compile_plan(g, fp32=True)]
    assert [o for o in outs if o.startswith("encoder_0_attn#")] == [f"encoder_0_attn#{p}" for p in ("qk", "v", "ctx")]
    assert [o for o in outs if o.startswith("decoder_0_cross_attn#")] == [
        f"decoder_0_cross_attn#{p}" for p in ("q", "k", "v", "ctx")]
    s = to_keras_json(g)
    assert json.loads(from_keras_json(s, cross_attention=True).to_json()) == json.loads(g.to_json())


def test_cpu_executor_runs_detr_micro_within_the_vit_micro_bound(micro):
    """The native CPU path's model-level bound (tests/test_vit.py): within 1.3e-5 of the PyTorch oracle, relative to
    the largest output."""
    g, w, x, want = micro
    got = cpu_executor.CpuExecutor(g, w)(x.numpy())
    rel = _rel(got, want)
    print(f"detr_micro CpuExecutor rel err {rel:.3e}")
    assert got.shape == (2, 1, 10, 96) and np.isfinite(got).all() and rel <= 1.3e-5
    assert (got[..., 92:] > 0).all() and (got[..., 92:] < 1).all()          # the sigmoid boxes


@pytest.mark.parametrize("cut,frontier", [
    (ENC_CUT, {ENC_CUT, "pos"}),
    (DEC_CUT, {DEC_CUT, "encoder_1_ln_ffn", "memory_pos", "query_embed"}),
])
def test_sliced_equals_unsliced_inside_an_encoder_and_a_decoder_layer(micro, cut, frontier):
    """The decoder cut's frontier is the running target, the memory, memory + pos and the query embedding."""
    g, w, x, _ = micro
    parts = slicer.partition(g, [cut])
    assert len(parts) == 2 and set(parts[1].inputs) == frontier
    full = cpu_executor.CpuExecutor(g, w)(x.numpy())
    vals = {g.input_names[0]: x.numpy()}
    for s in parts:
        sg = slicer.subgraph(g, s)
        vals.update(cpu_executor.CpuExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
    np.testing.assert_array_equal(vals[g.output], full)


@pytest.mark.parametrize("stages", [2, 3])
def test_planner_cuts_detr_micro(micro, stages):
    g, w, x, want = micro
    cuts, _ = planner.plan_cuts(g, stages, batch=2, precision="fp32", calibrated=False)
    assert len(cuts) == stages - 1
    parts = slicer.partition(g, cuts)
    vals = {g.input_names[0]: x.numpy()}
    for s in parts:
        sg = slicer.subgraph(g, s)
        vals.update(cpu_executor.CpuExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
    assert _rel(vals[g.output], want) <= 1.3e-5


def test_planner_costs_the_two_new_kinds():
    g = build_model("detr_micro")
    hw = planner.HwModel()
    cost = planner.layer_costs(g, batch=4, hw=hw)
    assert cost["pos"] == pytest.approx(g.tensor_bytes("pos", hw.act_bytes) * 4 / hw.hbm_bw + hw.launch_s)
    # q = k from one tensor: two projections, the core, the output projection
    assert cost["encoder_0_attn"] >= 4 * hw.launch_s and cost["decoder_0_cross_attn"] >= 5 * hw.launch_s


def test_parameter_total_of_detr_resnet50_by_closed_form():
    """From the hyper-parameters alone.  The published PyTorch figure, about 41.3 M, leaves out the frozen
    BatchNormalization statistics (which Keras counts as weights), has no position or zeros-target table (its sine
    encoding is computed, its target starts as a constant) and no conv biases in the backbone; it is not the
    number asserted here."""
    _, width, heads, nq, enc, dec, ffn, shape = DETR["detr_resnet50"]

    def conv(k, cin, cout):
        return k * k * cin * cout + cout

    bn = lambda c: 4 * c                                            # noqa: E731
    backbone = conv(7, 3, 64) + bn(64)
    cin = 64
    for filters, blocks in zip((64, 128, 256, 512), (3, 4, 6, 3)):
        for b in range(blocks):
            if b == 0:
                backbone += conv(1, cin, 4 * filters) + bn(4 * filters)
            backbone += (conv(1, cin, filters) + bn(filters) + conv(3, filters, filters) + bn(filters)
                         + conv(1, filters, 4 * filters) + bn(4 * filters))
            cin = 4 * filters
    assert backbone == 23_587_712                                   # Keras ResNet50(include_top=False)
    tokens = (shape[0] // 32) * (shape[1] // 32)
    assert tokens == 300
    mha = 4 * (width * width + width)
    ln = 2 * width
    ffn_p = width * ffn + ffn + ffn * width + width
    total = (backbone + conv(1, 2048, width) + tokens * width
             + enc * (mha + ffn_p + 2 * ln) + 2 * nq * width + dec * (2 * mha + ffn_p + 3 * ln) + ln
             + width * DETR_CLASSES + DETR_CLASSES + 2 * (width * width + width) + width * 4 + 4)
    g = build_model("detr_resnet50")
    assert g.count_params() == total == 41_759_968
    assert g.layers["src"].out_shape == (1, 300, 256) and g.layers["detections"].out_shape == (1, 100, 96)
    assert g.layers["conv5_block3_out"].out_shape == (15, 20, 2048)
    # above 224 wide the fused stem does not apply: the plain conv path takes the 7x7
    for fp32 in (True, False):
        kinds = [s.kind for s in compile_plan(g, fp32=fp32)]
        assert "stem" not in kinds and "stem_f32" not in kinds


# ------------------------------------------------------------------ command line
def _cli(*args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", PKG, *args], cwd=root, env=env, capture_output=True, text=True,
                          timeout=300)


def test_cli_plans_detr_micro_in_three_stages():
    r = _cli("plan", "--model", "detr_micro", "--stages", "3")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "detections" in r.stdout and "part3" in r.stdout


def test_cli_local_infer_runs_detr_micro_on_the_cpu():
    r = _cli("local-infer", "--model", "detr_micro", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-2000:]


# ------------------------------------------------------------------ nothing else moves
@pytest.mark.parametrize("model", ["resnet50", "convnext_tiny", "unet", "vit_b16", "swin_tiny", "sd_vae_decoder"])
def test_the_plans_of_the_older_families_are_unchanged(model):
    """tests/golden/plan_steps_before_cross_attention.json: "kind output" of every step, fp32 and bf16, recorded from
    the commit before cross-attention."""
    with open(GOLDEN) as f:
        before = json.load(f)[model]
    g = build_model(model)
    for precision in ("fp32", "bf16"):
        now = [f"{s.kind} {s.out}" for s in compile_plan(g, fp32=precision == "fp32")]
        assert now == before[precision], f"{model} {precision}"
