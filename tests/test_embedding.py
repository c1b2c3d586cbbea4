"""The `embedding` op (Keras Embedding over float32 token ids) without a GPU: the native CPU op, the PyTorch oracle,
the IR and Keras JSON in both serialisations.

A gather moves values and computes nothing, so every comparison is bit for bit.  The HIP kernel:
tests/test_guard_causal_gpu.py, tests/test_gpt_gpu.py.
"""
import json

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import planner
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

from test_vit import _k2, _k3

V, C, T = 300, 12, 9


def _graph(v=V, c=C, t=T):
    g = Graph("t")
    g.add(Layer("ids", "input", [], {"shape": (t,)}))
    g.add(Layer("emb", "embedding", ["ids"], {"input_dim": v, "output_dim": c}))
    g.output_names = ["emb"]
    return g


def _table():
    return np.random.default_rng(0).standard_normal((V, C)).astype(np.float32)


def test_native_op_is_bit_exact_against_indexing():
    table = _table()
    ids = np.random.default_rng(1).integers(0, V, (3, T))
    ids[0, :3] = (0, V - 1, 257)                                    # both ends, and an id bf16 would not hold
    y = np.full((3, T, C), np.nan, np.float32)
    cpu_executor.native().embedding(ids.astype(np.float32), table, y)
    np.testing.assert_array_equal(y, table[ids])


def test_ids_out_of_range_give_zero_rows_and_fractions_truncate_toward_zero():
    table = _table()
    ids = np.array([[0.0, V - 1.0, V, -1.0, 1e9, -7.0, 2.9, 0.999, -0.5, np.nan, np.inf, -np.inf, V - 0.25]],
                   np.float32)
    want = np.zeros((1, ids.shape[1], C), np.float32)
    for j, i in enumerate((0, V - 1, None, None, None, None, 2, 0, 0, None, None, None, V - 1)):
        if i is not None:
            want[0, j] = table[i]
    y = np.full(want.shape, np.nan, np.float32)
    cpu_executor.native().embedding(ids, table, y)
    np.testing.assert_array_equal(y, want)
    g = _graph(t=ids.shape[1])
    got = ReferenceExecutor(g, {"emb/embeddings": table})(torch.from_numpy(ids)).numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cpu_executor.CpuExecutor(g, {"emb/embeddings": table})(ids), want)


def test_ir_shapes_weights_plan_and_refusals():
    g = _graph()
    assert g.layers["emb"].out_shape == (T, C) and g.weight_specs() == [("emb/embeddings", (V, C))]
    assert g.layer_macs("emb") == 0 and planner.layer_costs(g, batch=2)["emb"] > 0.0
    assert json.loads(Graph.from_json(g.to_json()).to_json()) == json.loads(g.to_json())
    assert 0.01 < init_weights(g, 0)["emb/embeddings"].std() < 0.03
    for kw in ({"fp32": True, "device_fusions": False}, {"fp32": True}, {"fp32": False}):
        steps = compile_plan(g, **kw)                               # no pack step in front of the ids
        assert [(st.kind, st.out, st.ins) for st in steps] == [("embedding", "emb", ["ids"])]
    big = Graph("t")
    big.add(Layer("ids", "input", [], {"shape": (T,)}))
    big.add(Layer("ok", "embedding", ["ids"], {"input_dim": 2 ** 24, "output_dim": 2}))
    with pytest.raises(ValueError, match=r"too_big.*2\*\*24"):
        big.add(Layer("too_big", "embedding", ["ids"], {"input_dim": 2 ** 24 + 1, "output_dim": 2}))
    with pytest.raises(ValueError, match="on_a_map"):
        big.add(Layer("on_a_map", "embedding", ["ok"], {"input_dim": 4, "output_dim": 2}))
    with pytest.raises(ValueError, match="empty"):
        big.add(Layer("empty", "embedding", ["ids"], {"input_dim": 0, "output_dim": 2}))


def _keras_model(L, keras3, **cfg):
    shape = {"batch_shape": [None, T]} if keras3 else {"batch_input_shape": [None, T]}
    c = dict(input_dim=V, output_dim=C, mask_zero=False, input_length=None if keras3 else T)
    c.update(cfg)
    layers = [L("InputLayer", "ids", [], dtype="int32", **shape),
              L("Embedding", "emb", ["ids"], **c),
              L("Dense", "fc", ["emb"], units=5, activation="linear", use_bias=True)]
    return json.dumps({"class_name": "Functional", "config": {"name": "m", "layers": layers,
                                                              "input_layers": [["ids", 0, 0]],
                                                              "output_layers": [["fc", 0, 0]]}})


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_keras_json_imports_embedding_and_round_trips(L, keras3):
    g = from_keras_json(_keras_model(L, keras3))
    assert [g.layers[n].op for n in g.order] == ["input", "embedding", "dense"]
    assert g.layers["emb"].attrs == {"input_dim": V, "output_dim": C}
    assert g.layers["emb"].out_shape == (T, C) and g.layers["fc"].out_shape == (T, 5)
    s = to_keras_json(g)
    assert {ld["name"]: ld["class_name"] for ld in json.loads(s)["config"]["layers"]}["emb"] == "Embedding"
    assert json.loads(from_keras_json(s).to_json()) == json.loads(g.to_json())
    w = init_weights(g, 1)
    ids = np.random.default_rng(2).integers(0, V, (2, T)).astype(np.float32)
    want = w["emb/embeddings"].astype(np.float64)[ids.astype(int)] @ w["fc/kernel"].astype(np.float64) + w["fc/bias"]
    assert np.abs(ReferenceExecutor(g, w)(torch.from_numpy(ids)).numpy() - want).max() < 1e-6
    assert np.abs(cpu_executor.CpuExecutor(g, w)(ids) - want).max() < 1e-6


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_keras_json_refuses_mask_zero_and_a_wrong_input_length_by_name(L, keras3):
    with pytest.raises(NotImplementedError, match="emb.*mask_zero"):
        from_keras_json(_keras_model(L, keras3, mask_zero=True))
    with pytest.raises(NotImplementedError, match="emb.*input_length"):
        from_keras_json(_keras_model(L, keras3, input_length=T + 1))
