"""Causal self-attention without a GPU: the native CPU op against the causal oracle of
tests/causal_attention_cases.py, the `causal` attribute through the IR, the Keras JSON importer and the launch plan,
and a block by hand in float64 through the PyTorch oracle and the native CPU path.

The HIP kernels: tests/test_causal_attention_gpu.py, tests/test_guard_causal_gpu.py.
"""
import json

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

import attention_cases as AC
import causal_attention_cases as CC
from test_vit import _k2, _k3, _keras_attention, _kt, _noisy, _rel

CAUSAL_CALL = {"value": "ln", "use_causal_mask": True}


# ------------------------------------------------------------------ the core
@pytest.mark.parametrize("c", CC.CASES, ids=str)
def test_cpu_causal_attention_matches_float64_oracle(c):
    k = CC.case(c)
    y = np.full(k.want.shape, np.nan, np.float32)
    cpu_executor.native().attention(k.qkv, y, k.B, k.T, k.heads, k.d, k.dv, causal=True)
    err = np.abs(y.astype(np.float64) - k.want).max()
    print(f"cpu causal attention {c} [{k.path}]: e_ref {k.e_ref:.3e}, max err {err:.3e}, allowance {k.allow:.3e}")
    assert np.isfinite(y).all() and err <= k.allow
    # query 0 attends key 0 alone: p = 1, so the row is V's row 0 bit for bit
    v0 = AC.split(k.qkv, k.B, k.T, k.heads, k.d, k.dv)[2][:, 0].reshape(k.B, -1)
    np.testing.assert_array_equal(y.reshape(k.B, k.T, -1)[:, 0], v0)


def test_cpu_attention_default_is_not_causal():
    c = CC.CASES[3]
    k, kn = CC.case(c), AC.case(c)
    y, z = np.empty(k.want.shape, np.float32), np.empty(k.want.shape, np.float32)
    cpu_executor.native().attention(k.qkv, y, k.B, k.T, k.heads, k.d, k.dv)
    cpu_executor.native().attention(k.qkv, z, k.B, k.T, k.heads, k.d, k.dv, causal=False)
    np.testing.assert_array_equal(y, z)
    assert np.abs(y.astype(np.float64) - kn.want).max() <= kn.allow
    assert np.abs(kn.want - k.want).max() > 100 * k.allow           # the mask matters on this case


def test_the_causal_oracle_and_its_allowance():
    for c in CC.CASES:
        k, kn = CC.case(c), AC.case(c)
        assert k.qkv is kn.qkv                                      # the same inputs, shared
        np.testing.assert_allclose(k.want[(k.T - 1)::k.T], kn.want[(k.T - 1)::k.T], rtol=1e-12, atol=1e-12)
        assert k.e_ref <= 1e-5 and k.allow == 2e-5 * max(1.0, float(np.abs(k.want).max())), (c, k.e_ref)
        assert CC.case_bf16(c).e_ref <= 1e-5
        # row q of the causal result is the unmasked result over the first q + 1 tokens
        q = min(k.T - 1, CC.KT)
        x = k.qkv.reshape(k.B, k.T, -1)[:, :q + 1].reshape(k.B * (q + 1), -1)
        part = AC.ref_attention(x, k.B, q + 1, k.heads, k.d, k.dv).reshape(k.B, q + 1, -1)[:, q]
        np.testing.assert_allclose(k.want.reshape(k.B, k.T, -1)[:, q], part, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("probe", ["ascending", "dominant"])
def test_masking_after_the_maximum_would_fail_the_probes(probe):
    """A large future score underflows every visible term when the maximum is taken before the mask: NaN."""
    c = next(c for c in CC.CASES if c[5] == probe)
    k = CC.case(c)
    y = CC.late_masking(k.qkv, k.B, k.T, k.heads, k.d, k.dv)
    assert np.isnan(y).any()


# ------------------------------------------------------------------ IR
def _graph(causal, inputs=("in",), shape=(16, 8)):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": shape}))
    g.add(Layer("other", "layernorm", ["in"], {"epsilon": 1e-3}))
    a = {"num_heads": 2, "key_dim": 4, "use_bias": True}
    if causal:
        a["causal"] = True
    g.add(Layer("attn", "mha", list(inputs), a))
    g.output_names = ["attn"]
    return g


def test_ir_takes_causal_only_as_true_and_only_on_self_attention():
    g, gn = _graph(True), _graph(False)
    assert g.layers["attn"].attrs["causal"] is True and "causal" not in gn.layers["attn"].attrs
    T, C, h, d = 16, 8, 2, 4
    assert gn.layer_macs("attn") == 3 * T * C * h * d + T * T * h * 2 * d + T * h * d * C
    assert g.layer_macs("attn") == 3 * T * C * h * d + T * (T + 1) // 2 * h * 2 * d + T * h * d * C
    assert json.loads(Graph.from_json(g.to_json()).to_json()) == json.loads(g.to_json())
    with pytest.raises(ValueError, match="attn.*causal"):
        _graph(True, ("in", "other"))
    with pytest.raises(ValueError, match="attn.*causal"):
        _graph(True, ("in", "other", "other"))
    bad = Graph("t")
    bad.add(Layer("in", "input", [], {"shape": (16, 8)}))
    with pytest.raises(ValueError, match="attn.*causal"):
        bad.add(Layer("attn", "mha", ["in"], {"num_heads": 2, "key_dim": 4, "causal": False}))


# ------------------------------------------------------------------ Keras JSON
def _keras3_positional():
    """Keras 3 with every call argument in "args": (query, value, key, attention_mask, return_attention_scores,
    training, use_causal_mask)."""
    d = json.loads(_keras_attention(_k3, True, ("ln",), {"value": "ln"}))
    for ld in d["config"]["layers"]:
        if ld["name"] == "attn":
            ld["inbound_nodes"] = [{"args": [_kt("ln"), _kt("ln"), None, None, False, False, True], "kwargs": {}}]
    return json.dumps(d)


@pytest.mark.parametrize("doc", [lambda: _keras_attention(_k2, False, ("ln",), CAUSAL_CALL),
                                 lambda: _keras_attention(_k3, True, ("ln",), CAUSAL_CALL),
                                 _keras3_positional], ids=["keras2", "keras3", "keras3_args"])
def test_keras_json_reads_use_causal_mask_on_request_and_round_trips(doc):
    doc = doc()
    g = from_keras_json(doc, causal_attention=True)
    assert g.layers["attn"].inputs == ["ln"]
    assert g.layers["attn"].attrs == {"num_heads": 2, "key_dim": 4, "use_bias": True, "causal": True}
    s = to_keras_json(g)
    node = next(ld for ld in json.loads(s)["config"]["layers"] if ld["name"] == "attn")["inbound_nodes"][0]
    assert node[0][3]["use_causal_mask"] is True                    # the Keras 2 call kwarg
    assert json.loads(from_keras_json(s, causal_attention=True).to_json()) == json.loads(g.to_json())
    # by default, and with cross_attention alone, the call is refused by layer name, with the hint
    for kw in ({}, {"cross_attention": True}):
        with pytest.raises(NotImplementedError, match=r"attn.*use_causal_mask.*causal_attention=True\) reads it"):
            from_keras_json(doc, **kw)
        with pytest.raises(NotImplementedError, match="attn.*use_causal_mask"):
            from_keras_json(s, **kw)
    m = Model.from_keras_json(doc, seed=2)                          # what the command line uses asks for it
    assert m.graph.layers["attn"].attrs.get("causal") is True


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_keras_json_without_the_mask_stores_no_attribute(L, keras3):
    for call in ({"value": "ln"}, {"value": "ln", "use_causal_mask": False}):
        g = from_keras_json(_keras_attention(L, keras3, ("ln",), call), causal_attention=True)
        assert g.layers["attn"].attrs == {"num_heads": 2, "key_dim": 4, "use_bias": True}


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
@pytest.mark.parametrize("call", [{"value": "other", "use_causal_mask": True},
                                  {"value": "ln", "key": "other", "use_causal_mask": True}])
def test_keras_json_refuses_a_causal_mask_on_separate_sources_by_name(L, keras3, call):
    with pytest.raises(NotImplementedError, match="attn.*use_causal_mask.*separate"):
        from_keras_json(_keras_attention(L, keras3, ("ln",), call), cross_attention=True, causal_attention=True)


# ------------------------------------------------------------------ plan
def test_plan_marks_only_the_causal_attention_step():
    for kw in ({"fp32": True, "device_fusions": False}, {"fp32": True}, {"fp32": False}):
        causal = compile_plan(_graph(True), **kw)
        plain = compile_plan(_graph(False), **kw)
        assert [st.kind for st in causal] == [st.kind for st in plain]
        for a, b in zip(causal, plain):
            assert (a.out, a.ins, a.covers) == (b.out, b.ins, b.covers)
            if a.kind == "attention":
                assert a.p == dict(b.p, causal=True) and "causal" not in b.p
            else:
                assert a.p == b.p and "causal" not in a.p
        assert sum(st.kind == "attention" for st in causal) == 1


# ------------------------------------------------------------------ a block by hand
def _numpy_forward(w, x):
    """The block of tests/test_vit.py by hand in float64 with the causal mask on the scores."""
    t = x.reshape(x.shape[0], 16, 8).astype(np.float64)
    mu = t.mean(-1, keepdims=True)
    y = (t - mu) / np.sqrt(((t - mu) ** 2).mean(-1, keepdims=True) + 1e-6) * w["ln/gamma"] + w["ln/beta"]
    q = (np.einsum("btc,chd->bthd", y, w["attn/query/kernel"]) + w["attn/query/bias"]) / np.sqrt(4.0)
    k = np.einsum("btc,chd->bthd", y, w["attn/key/kernel"]) + w["attn/key/bias"]
    v = np.einsum("btc,chd->bthd", y, w["attn/value/kernel"]) + w["attn/value/bias"]
    s = np.where(np.tri(16, dtype=bool), np.einsum("bqhd,bkhd->bhqk", q, k), -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    o = np.einsum("bhqk,bkhd->bqhd", p, v)
    o = np.einsum("bqhd,hdc->bqc", o, w["attn/attention_output/kernel"]) + w["attn/attention_output/bias"]
    return (t + o) @ w["fc/kernel"] + w["fc/bias"]


def test_a_causal_block_by_hand_through_the_oracle_and_the_native_cpu_path():
    g = from_keras_json(_keras_attention(_k2, False, ("ln",), CAUSAL_CALL), causal_attention=True)
    w = _noisy(init_weights(g, 2))
    x = np.random.default_rng(0).standard_normal((2, 4, 4, 8)).astype(np.float32)
    want = _numpy_forward(w, x)
    got = ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()
    assert got.shape == (2, 16, 6) and _rel(got, want) < 1e-5
    ex = cpu_executor.CpuExecutor(g, w, outputs=["fc"])
    assert [st.kind for st in ex.steps] == ["layernorm", "layernorm", "conv", "attention", "conv", "conv"]
    assert ex.steps[3].p["causal"] is True
    assert _rel(ex(x), want) < 1e-5
    # and the mask is not a no-op on these values
    plain = from_keras_json(_keras_attention(_k2, False, ("ln",), {"value": "ln"}))
    assert _rel(cpu_executor.CpuExecutor(plain, w, outputs=["fc"])(x), want) > 1e-3
