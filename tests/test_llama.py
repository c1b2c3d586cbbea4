"""Llama (models/zoo.py `build_llama`) without a GPU: the three new layers (rmsnorm, the rope step, grouped-query
attention) on the native CPU ops against the float64 oracles of tests/llama_cases.py, the host-side rope table, the
IR and Keras JSON (round trips and every refusal by layer name), the plan (the golden step-list pin of the models
that existed before, and llama_micro's steps), `llama_micro` through the CPU path and the PyTorch oracle against
the model by hand, the model by hand against `transformers`' LlamaForCausalLM, sliced runs, parameter totals in
closed form and the command line.

On the GPU: tests/test_llama_kernels_gpu.py, tests/test_guard_llama_gpu.py, tests/test_llama_gpu.py.
"""
import json
import os

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.utils.config import AdaptConfig
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import (
    Graph, Layer, mha_projection, propagate_masks)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.planner import layer_costs
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    BUILDERS, LLAMA, build_llama, build_model)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

import llama_cases as LC
from test_vit import _k2, _k3, _rel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_steps_before_llama.json")
QT, KT = A.attention_tiles()
GQA_CASES = LC.gqa_cases(QT, KT)
CUT = "llama_micro_block_0_post_attention_norm"
BLOCK_KINDS = ["rmsnorm", "conv", "rope", "attention", "conv", "rmsnorm", "conv", "act", "conv", "binary", "conv"]


# ------------------------------------------------------------------ kernel cases on the native CPU ops
@pytest.mark.parametrize("c", LC.RMSNORM_CASES, ids=str)
def test_cpu_rmsnorm_against_the_oracle(c):
    rows, C, eps, scale, probe = c
    x, sc = LC.rmsnorm_inputs(c)
    want = LC.rmsnorm_oracle(x, sc, eps)
    e_ref = float(np.abs(LC.rmsnorm_library(x, sc, eps) - want).max())
    y = np.full_like(x, np.nan)
    cpu_executor.native().rmsnorm(x, sc if scale else np.ones(C, np.float32), y, eps)
    err, allow = float(np.abs(y - want).max()), LC.allowance(want, e_ref)
    print(f"rmsnorm cpu {c}: e_ref {e_ref:.3e} err {err:.3e} allowance {allow:.3e}")
    assert err <= allow


@pytest.mark.parametrize("c", LC.ROPE_CASES, ids=str)
def test_cpu_rope_against_the_oracle(c):
    B, T, hq, hkv, d, dv, W = c
    x = LC.rope_inputs(c)
    x = np.concatenate([x, np.full((B * T, 3), 7.0, np.float32)], axis=1)      # three columns past the true width
    table = A.rope_table(T, d, W).numpy()
    wd, rotw = LC.rope_width(c), (hq + hkv) * d
    want = LC.rope_oracle(x[:, :wd], c, table)
    e_ref = float(np.abs(LC.rope_library(x[:, :wd], c, table) - want).max())
    y = np.full_like(x, np.nan)
    cpu_executor.native().rope(x, table, y, T, hq, hkv, d, dv)
    err, allow = float(np.abs(y[:, :wd] - want).max()), LC.allowance(want, e_ref)
    print(f"rope cpu {c}: e_ref {e_ref:.3e} err {err:.3e} allowance {allow:.3e}")
    assert err <= allow
    np.testing.assert_array_equal(y[:, rotw:wd], x[:, rotw:wd])     # V: a copy, bit for bit
    assert (y[:, wd:] == 0).all()                                    # the rest of a row: zeros
    np.testing.assert_array_equal(y[::T, :wd], x[::T, :wd])         # position 0 of every image: the identity
    # against the float64 angles themselves: the table's one rounding is all that separates the two
    assert np.abs(want - LC.rope_oracle(x[:, :wd], c)).max() <= 2.0 ** -23 * np.abs(x).max() * 2


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("c", GQA_CASES, ids=str)
def test_cpu_gqa_attention_against_the_oracle(c, causal):
    B, T, hq, hkv, d, dv, probe = c
    x = LC.gqa_inputs(c)
    want = LC.gqa_oracle(x, c, causal)
    e_ref = float(np.abs(LC.gqa_library(x, c, causal) - want).max())
    m = cpu_executor.native()
    y = np.full((B * T, hq * dv), np.nan, np.float32)
    m.attention(x, y, B, T, hq, d, dv, causal, None, hkv)
    err, allow = float(np.abs(y - want).max()), LC.allowance(want, e_ref)
    print(f"gqa cpu {c} causal={causal}: e_ref {e_ref:.3e} err {err:.3e} allowance {allow:.3e}")
    assert err <= allow
    # the same op on rows with each K / V head repeated g times: the same arithmetic per (image, head)
    z = np.full_like(y, np.nan)
    m.attention(LC.gqa_expanded(x, c), z, B, T, hq, d, dv, causal)
    np.testing.assert_array_equal(y, z)
    if hq == hkv:                                                    # kv_heads == heads is the op as it was
        m.attention(x, z, B, T, hq, d, dv, causal, None, 0)
        np.testing.assert_array_equal(y, z)


def test_cpu_ops_refuse_what_they_cannot_hold():
    m = cpu_executor.native()
    x = np.zeros((4, 24), np.float32)
    with pytest.raises(Exception, match="kv_heads"):
        m.attention(x, np.zeros((4, 8), np.float32), 1, 4, 4, 2, 2, False, None, 3)        # 4 % 3
    with pytest.raises(Exception, match="key_mask"):
        m.attention(x, np.zeros((4, 8), np.float32), 1, 4, 4, 2, 2, False, np.ones(4, np.float32), 2)
    with pytest.raises(Exception, match="rope"):
        m.rope(np.zeros((4, 9), np.float32), np.zeros((2, 4, 1), np.float32), np.zeros((4, 9), np.float32), 4, 1, 1,
               3, 3)                                                                       # odd d


def test_rope_table_is_float64_angles_rounded_once():
    """4096 positions: an angle computed in fp32 is off by up to 2.4e-4 rad there, far above one rounding of the
    cosine.  Fails a table built from fp32 angles."""
    T, d, W = 4096, 64, 10000.0
    t = A.rope_table(T, d, W)
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, T, d // 2)
    th = LC.rope_angles(T, d, W)
    np.testing.assert_array_equal(t[0].numpy(), np.cos(th).astype(np.float32))
    np.testing.assert_array_equal(t[1].numpy(), np.sin(th).astype(np.float32))
    th32 = (np.arange(T, dtype=np.float32)[:, None] * (np.float32(W) ** (-2.0 * np.arange(d // 2, dtype=np.float32)
                                                                       / np.float32(d)))[None, :])
    assert np.abs(np.cos(th32).astype(np.float32) - t[0].numpy()).max() > 1e-5           # what is being ruled out
    for bad in ((0, 64, W), (8, 7, W), (8, 0, W), (8, 64, 0.0)):
        with pytest.raises(ValueError, match="rope_table"):
            A.rope_table(*bad)


def test_wrappers_refuse_before_any_launch():
    x = torch.zeros((4, 9))
    with pytest.raises(ValueError, match="even"):
        A.rope(x, torch.zeros((2, 4, 1)), torch.zeros((4, 9)), 4, 1, 3, 3, kv_heads=1)
    with pytest.raises(ValueError, match="kv_heads"):
        A.attention(x, x, 1, 4, 4, 2, 2, kv_heads=3)
    with pytest.raises(ValueError, match="padding mask together with kv_heads"):
        A.attention(x, x, 1, 4, 4, 2, 2, kv_heads=2, key_mask=torch.ones(4))


# ------------------------------------------------------------------ IR
def _attn_graph(inputs=("in",), shape=(6, 8), op="mha", **attrs):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": shape}))
    g.add(Layer("other", "input", [], {"shape": shape}))
    a = dict({"num_heads": 4, "key_dim": 4, "use_bias": False}, **attrs)
    g.add(Layer("attn_7", op, list(inputs), a))
    return g


@pytest.mark.parametrize("attrs,inputs,word", [
    ({"kv_heads": 3}, ("in",), "divides"),
    ({"kv_heads": 0}, ("in",), "divides"),
    ({"kv_heads": 2}, ("in", "other"), "one input"),
    ({"rope": 10000.0}, ("in", "other"), "one input"),
    ({"rope": 10000.0, "key_dim": 3}, ("in",), "even key_dim"),
    ({"rope": 0.0}, ("in",), "max wavelength"),
    ({"rope": True}, ("in",), "max wavelength"),
])
def test_graph_add_refuses_a_bad_grouped_or_rotary_layer_by_name(attrs, inputs, word):
    with pytest.raises(ValueError, match=f"'attn_7'.*{word}"):
        _attn_graph(inputs, **attrs)


def test_graph_add_refuses_rope_on_window_attention_and_masks_with_gqa_by_name():
    with pytest.raises(ValueError, match="'attn_7'.*window attention"):
        _attn_graph(shape=(4, 4, 8), op="winattn", window=2, shift=0, rope=10000.0, key_dim=2)
    g = Graph("t")
    g.add(Layer("ids", "input", [], {"shape": (6,)}))
    g.add(Layer("emb", "embedding", ["ids"], {"input_dim": 9, "output_dim": 8}))
    for extra in ({"kv_heads": 2}, {"rope": 10000.0}):
        with pytest.raises(ValueError, match="'attn_7'.*key_mask"):
            g.add(Layer("attn_7", "mha", ["emb", "ids"], dict({"num_heads": 4, "key_dim": 4, "key_mask": True}, **extra)))
    with pytest.raises(ValueError, match="'norm_3'.*\\(T, C\\)"):
        g.add(Layer("norm_3", "rmsnorm", ["ids"], {"epsilon": 1e-6}))


@pytest.mark.parametrize("extra", [{"kv_heads": 2}, {"rope": 10000.0}, {"kv_heads": 4}], ids=str)
def test_propagate_masks_refuses_a_mask_into_grouped_or_rotary_attention_and_passes_rmsnorm(extra):
    g = Graph("t")
    g.add(Layer("ids", "input", [], {"shape": (6,)}))
    g.add(Layer("emb", "embedding", ["ids"], {"input_dim": 9, "output_dim": 8, "mask_zero": True}))
    g.add(Layer("norm", "rmsnorm", ["emb"], {"epsilon": 1e-6}))
    g.add(Layer("plain", "mha", ["norm"], {"num_heads": 4, "key_dim": 4}))
    assert propagate_masks(g) == {"plain": "ids"}                    # through rmsnorm as through layernorm
    g.add(Layer("attn_7", "mha", ["norm"], dict({"num_heads": 4, "key_dim": 4}, **extra)))
    with pytest.raises(NotImplementedError, match="'attn_7'.*kv_heads / rope"):
        propagate_masks(g)


def test_weight_shapes_projection_and_macs_follow_kv_heads():
    g = _attn_graph(kv_heads=2, rope=10000.0, key_dim=6, value_dim=5)
    L = g.layers["attn_7"]
    shapes = dict(L.weight_shapes([(6, 8)]))
    assert shapes == {"attn_7/query/kernel": (8, 4, 6), "attn_7/key/kernel": (8, 2, 6), "attn_7/value/kernel": (8, 2, 5),
                      "attn_7/attention_output/kernel": (4, 5, 8)}
    rng = np.random.default_rng(0)
    w = {n: rng.standard_normal(s).astype(np.float32) for n, s in shapes.items()}
    k, b = mha_projection(w, "attn_7", {"heads": 4, "key_dim": 6, "value_dim": 5, "kv_heads": 2}, "qkv")
    assert b is None and k.shape == (8, 4 * 6 + 2 * 6 + 2 * 5)
    np.testing.assert_allclose(k[:, :24], w["attn_7/query/kernel"].reshape(8, 24) / np.sqrt(6.0), rtol=1e-6)
    np.testing.assert_array_equal(k[:, 24:36], w["attn_7/key/kernel"].reshape(8, 12))
    np.testing.assert_array_equal(k[:, 36:], w["attn_7/value/kernel"].reshape(8, 10))
    plain = _attn_graph(key_dim=6, value_dim=5).layers["attn_7"]
    assert plain.macs([(6, 8)]) - L.macs([(6, 8)]) == 6 * 8 * 2 * (6 + 5)      # two K / V heads fewer to project
    g2 = _attn_graph(shape=(3, 2, 8))
    g2.add(Layer("n", "rmsnorm", ["attn_7"], {"epsilon": 1e-6, "scale": False}))
    assert g2.layers["n"].out_shape == (3, 2, 8) and g2.layers["n"].weight_shapes([(3, 2, 8)]) == []
    g2.add(Layer("m", "rmsnorm", ["attn_7"], {"epsilon": 1e-6}))
    assert g2.layers["m"].weight_shapes([(3, 2, 8)]) == [("m/scale", (8,))]


# ------------------------------------------------------------------ Keras JSON
def _doc(L, keras3, cls, attn_inbound=("norm",), call=None, norm_cfg=None, **cfg):
    shape = {"batch_shape": [None, 6, 8]} if keras3 else {"batch_input_shape": [None, 6, 8]}
    ncfg = dict(axis=-1, epsilon=1e-5, scale=True)
    ncfg.update(norm_cfg or {})
    layers = [L("InputLayer", "in", [], dtype="float32", **shape),
              L("RMSNormalization", "norm", ["in"], **ncfg),
              L("RMSNormalization", "other", ["in"], axis=-1, epsilon=1e-6, scale=False),
              L(cls, "attn_7", list(attn_inbound), call=call if call is not None else {"value": "norm"}, **cfg),
              L("Add", "add", ["in", "attn_7"])]
    return json.dumps({"class_name": "Functional", "config": {"name": "blk", "layers": layers,
                                                              "input_layers": [["in", 0, 0]],
                                                              "output_layers": [["add", 0, 0]]}})


GQA_CFG = dict(head_dim=4, num_query_heads=4, num_key_value_heads=2, dropout=0.0, use_bias=False)


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_keras_json_reads_and_writes_the_new_classes(L, keras3):
    g = from_keras_json(_doc(L, keras3, "GroupedQueryAttention", **GQA_CFG))
    assert g.layers["norm"].op == "rmsnorm" and g.layers["norm"].attrs == {"epsilon": 1e-5}
    assert g.layers["other"].attrs == {"epsilon": 1e-6, "scale": False}
    assert g.layers["attn_7"].attrs == {"num_heads": 4, "key_dim": 4, "kv_heads": 2, "use_bias": False}
    assert json.loads(from_keras_json(to_keras_json(g)).to_json()) == json.loads(g.to_json())
    assert json.loads(to_keras_json(g))["config"]["layers"][3]["class_name"] == "GroupedQueryAttention"
    # hq == hkv stays a GroupedQueryAttention: kv_heads is stored all the same
    g = from_keras_json(_doc(L, keras3, "GroupedQueryAttention", **dict(GQA_CFG, num_key_value_heads=4)))
    assert g.layers["attn_7"].attrs["kv_heads"] == 4
    doc = to_keras_json(g)
    assert json.loads(doc)["config"]["layers"][3]["class_name"] == "GroupedQueryAttention"
    assert json.loads(from_keras_json(doc).to_json()) == json.loads(g.to_json()) and to_keras_json(from_keras_json(doc)) == doc
    # the project's own rotary class, causal under causal_attention=True only
    src = _doc(L, keras3, "RotaryGroupedQueryAttention", call={"value": "norm", "use_causal_mask": True},
               rope_max_wavelength=500000.0, **GQA_CFG)
    with pytest.raises(NotImplementedError, match="attn_7.*use_causal_mask"):
        from_keras_json(src)
    g = from_keras_json(src, causal_attention=True)
    assert g.layers["attn_7"].attrs == {"num_heads": 4, "key_dim": 4, "kv_heads": 2, "use_bias": False,
                                        "rope": 500000.0, "causal": True}
    doc = to_keras_json(g)
    assert json.loads(doc)["config"]["layers"][3]["class_name"] == "RotaryGroupedQueryAttention"
    assert json.loads(from_keras_json(doc, causal_attention=True).to_json()) == json.loads(g.to_json())
    assert to_keras_json(from_keras_json(doc, causal_attention=True)) == doc
    g = from_keras_json(_doc(L, keras3, "RotaryGroupedQueryAttention", **GQA_CFG))
    assert g.layers["attn_7"].attrs["rope"] == 10000.0                                  # the default wavelength


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_keras_json_refuses_by_layer_name(L, keras3):
    def refused(match, cls="GroupedQueryAttention", exc=(NotImplementedError, ValueError), **kw):
        cfg = dict(GQA_CFG)
        cfg.update(kw.pop("cfg", {}))
        with pytest.raises(exc, match=match):
            from_keras_json(_doc(L, keras3, cls, **kw, **cfg), cross_attention=True, causal_attention=True)
    refused("attn_7.*separate sources", call={"value": "other"})
    refused("attn_7.*separate sources", cls="RotaryGroupedQueryAttention", call={"value": "norm", "key": "other"})
    refused("attn_7.*attention_mask", call={"value": "norm", "attention_mask": "other"})
    refused("attn_7.*return_attention_scores", call={"value": "norm", "return_attention_scores": True})
    refused("attn_7.*multiple", cfg={"num_key_value_heads": 3})
    refused("attn_7.*odd head_dim", cls="RotaryGroupedQueryAttention", cfg={"head_dim": 3})
    refused("attn_7.*frequency scaling", cls="RotaryGroupedQueryAttention", cfg={"rope_scaling_factor": 2.0})
    refused("norm.*RMSNormalization over axis", norm_cfg={"axis": 1})
    g = from_keras_json(_doc(L, keras3, "GroupedQueryAttention", norm_cfg={"axis": [2]}, **GQA_CFG))     # the last, positively
    assert g.layers["norm"].op == "rmsnorm"


# ------------------------------------------------------------------ plan
def _js(v):
    if isinstance(v, dict):
        return {str(k): _js(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
    if isinstance(v, (list, tuple)):
        return [_js(x) for x in v]
    return v if isinstance(v, (str, int, float, bool)) or v is None else repr(v)


@pytest.mark.parametrize("model", ["gpt_micro", "distilbert_micro", "vit_micro", "detr_micro", "swin_micro"])
def test_existing_models_compile_to_the_steps_they_compiled_to(model):
    """tests/golden/plan_steps_before_llama.json: kind, output, inputs and parameters of every step, fp32 and bf16,
    recorded from the commit before this one."""
    with open(GOLDEN) as f:
        before = json.load(f)[model]
    g = build_model(model)
    for precision in ("fp32", "bf16"):
        now = [{"kind": s.kind, "out": s.out, "ins": list(s.ins), "p": _js(s.p)}
               for s in compile_plan(g, fp32=precision == "fp32")]
        assert now == before[precision], f"{model} {precision}"
        assert not any("kv_heads" in s["p"] or "rope" in s["p"] or s["kind"] in ("rope", "rmsnorm") for s in now)


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "bf16"])
def test_llama_micro_compiles_to_rmsnorm_rope_and_gqa_steps(fp32):
    g = build_model("llama_micro")
    steps = compile_plan(g, fp32=fp32)
    assert [s.kind for s in steps] == ["embedding"] + BLOCK_KINDS * 2 + ["crop", "rmsnorm", "conv"]
    b = "llama_micro_block_0_attn"
    qkv, rope, core = steps[2], steps[3], steps[4]
    assert qkv.out == b + "#qkv" and qkv.p["filters"] == 4 * 16 + 2 * 16 + 2 * 16 and qkv.p["kv_heads"] == 2
    assert rope.out == b + "#rot" and rope.ins == [b + "#qkv"] and rope.p["rope"] == 10000.0
    assert (rope.p["heads"], rope.p["kv_heads"], rope.p["key_dim"], rope.p["tokens"]) == (4, 2, 16, 40)
    assert core.ins == [b + "#rot"] and core.out == b + "#ctx"
    assert core.p["causal"] is True and core.p["kv_heads"] == 2 and core.p["rope"] == 10000.0
    assert steps[1].p == {"layer": "llama_micro_block_0_input_norm", "eps": 1e-5}
    # no step writes the tensor it reads: the rope step is out of place
    assert all(s.out not in s.ins for s in steps)
    # plain multi-head attention behind the rope step carries no kv_heads
    mha = build_llama("llama_micro")
    for L in mha.layers.values():
        if L.op == "mha":
            L.attrs["kv_heads"] = 4
    cores = [s for s in compile_plan(mha, fp32=fp32) if s.kind == "attention"]
    assert all("kv_heads" not in s.p and s.p["rope"] == 10000.0 for s in cores)


def test_planner_costs_the_new_layers():
    g = build_model("llama_micro")
    cost = layer_costs(g, batch=2)
    assert cost["llama_micro_block_0_input_norm"] > 0
    plain = build_llama("llama_micro")
    for L in plain.layers.values():
        if L.op == "mha":
            del L.attrs["rope"]
    assert cost["llama_micro_block_0_attn"] > layer_costs(plain, batch=2)["llama_micro_block_0_attn"]


# ------------------------------------------------------------------ zoo
def test_llama_names_and_structure():
    assert {"tinyllama_1_1b", "llama2_7b", "llama_micro"} <= set(BUILDERS)
    assert LLAMA["llama_micro"] == (2, 64, 4, 2, 176, 97, 40, 1e-5, 10000.0)
    assert LLAMA["tinyllama_1_1b"] == (22, 2048, 32, 4, 5632, 32000, 128, 1e-5, 10000.0)
    assert LLAMA["llama2_7b"] == (32, 4096, 32, 32, 11008, 32000, 128, 1e-5, 10000.0)
    g = build_model("llama_micro")
    b = "llama_micro_block_0"
    assert g.order[:3] == ["input_1", "llama_micro_embed_tokens", "llama_micro_tokens"]
    names = ("input_norm", "attn", "add1", "post_attention_norm", "mlp_gate", "mlp_swish", "mlp_up", "mlp_mul",
             "mlp_down", "add2")
    assert g.order[3:13] == [f"{b}_{s}" for s in names]
    assert [g.layers[n].op for n in g.order[3:13]] == ["rmsnorm", "mha", "add", "rmsnorm", "dense", "act", "dense",
                                                       "binary", "dense", "add"]
    assert g.layers[f"{b}_attn"].attrs == {"num_heads": 4, "key_dim": 16, "use_bias": False, "causal": True,
                                           "kv_heads": 2, "rope": 10000.0}
    assert g.layers[f"{b}_mlp_swish"].attrs == {"fn": "swish"} and g.layers[f"{b}_mlp_mul"].attrs == {"fn": "mul"}
    assert not any(n.endswith("/bias") for L in g.layers.values() for n, _ in L.weight_shapes(g.in_shapes(L.name)))
    assert g.order[-3:] == ["llama_micro_last", "llama_micro_norm", "lm_head"] and g.output_names == ["lm_head"]
    assert g.layers["lm_head"].out_shape == (1, 1, 97)
    every = build_llama("llama_micro", all_positions=True)
    assert "llama_micro_last" not in every.layers and every.layers["lm_head"].out_shape == (1, 40, 97)
    assert build_llama("llama_micro", classes=1000, input_shape=(7,)).layers["lm_head"].out_shape == (1, 1, 1000)
    assert build_model("tinyllama_1_1b").layers["input_1"].out_shape == (128,)
    for shape in ((0,), (4, 4)):
        with pytest.raises(ValueError, match="llama_micro"):
            build_llama("llama_micro", input_shape=shape)
    assert json.loads(from_keras_json(to_keras_json(g), causal_attention=True).to_json()) == json.loads(g.to_json())


@pytest.mark.parametrize("name,published", [("tinyllama_1_1b", 1_100_048_384), ("llama2_7b", 6_738_415_616)])
def test_llama_parameter_totals_in_closed_form(name, published):
    depth, C, h, hkv, F, V, T, eps, wavelength = LLAMA[name]
    d = C // h
    # per block: Q and output projections (C x C), K and V (C x hkv d), gate, up and down, two norms; then the token
    # table, the final norm and the untied head
    block = 2 * C * C + 2 * C * hkv * d + 3 * C * F + 2 * C
    assert V * C + depth * block + C + C * V == published
    g = build_model(name)                                            # counted from shapes: no weight is allocated
    assert g.count_params() == published
    assert g.layers[f"{name}_block_0_attn"].attrs["kv_heads"] == hkv and g.layers["lm_head"].out_shape == (1, 1, V)


# ------------------------------------------------------------------ numerics
@pytest.mark.parametrize("all_positions", [False, True], ids=["last", "all"])
def test_llama_micro_matches_the_model_by_hand(all_positions):
    g, w, ids, want = LC.micro(all_positions)
    got = ReferenceExecutor(g, w)(torch.from_numpy(ids)).numpy()
    assert got.shape == (4, 1, 40 if all_positions else 1, 97)
    print(f"llama_micro reference rel err {_rel(got.reshape(want.shape), want):.3e}")
    assert _rel(got.reshape(want.shape), want) < 1e-5
    ex = cpu_executor.CpuExecutor(g, w)
    assert [st.kind for st in ex.steps] == ["embedding"] + BLOCK_KINDS * 2 + ([] if all_positions else ["crop"]) + [
        "rmsnorm", "conv"]
    tables = [ex.packed[i][0] for i, st in enumerate(ex.steps) if st.kind == "rope"]
    assert len(tables) == 2 and tables[0] is tables[1]               # one table for both layers
    print(f"llama_micro cpu rel err {_rel(ex(ids).reshape(want.shape), want):.3e}")
    assert _rel(ex(ids).reshape(want.shape), want) < 1e-5


def test_changing_a_token_leaves_the_logits_before_it_unchanged():
    g, w, ids, _ = LC.micro(True)
    ex = cpu_executor.CpuExecutor(g, w)
    base = ex(ids[:1])[0, 0]
    scale = np.abs(base).max()
    for t in (0, 1, 31, 32, 39):
        other = ids[:1].copy()
        other[0, t] = (other[0, t] + 1) % 97
        got = ex(other)[0, 0]
        assert np.abs(got[:t] - base[:t]).max(initial=0.0) <= 1e-6 * scale, t
        assert np.abs(got[t] - base[t]).max() > 1e-3 * scale, t


def test_the_model_by_hand_agrees_with_transformers_llama():
    """The by-hand oracle against Hugging Face's LlamaForCausalLM in float64 with llama_micro's weights loaded: pins
    the RoPE convention, the head grouping and the weight layout to the outside world.  Bound 1e-6 max|logits|; the
    residue is HF's fp32 `inv_freq` buffer.  Measured for llama_micro (4 query heads over 2, head 16, 40 tokens):
    6.5e-7 absolute at max|logit| 3.34, 2.0e-7 relative (transformers 5.15)."""
    transformers = pytest.importorskip("transformers")
    depth, C, h, hkv, F, V, T, eps, wavelength = LLAMA["llama_micro"]
    g, w, ids, want = LC.micro(True)
    kw = dict(vocab_size=V, hidden_size=C, intermediate_size=F, num_hidden_layers=depth, num_attention_heads=h,
              num_key_value_heads=hkv, head_dim=C // h, max_position_embeddings=T, rms_norm_eps=eps,
              hidden_act="silu", attention_bias=False, mlp_bias=False, tie_word_embeddings=False,
              attention_dropout=0.0)
    try:
        cfg = transformers.LlamaConfig(rope_theta=wavelength, **kw)
    except TypeError:
        cfg = transformers.LlamaConfig(rope_parameters={"rope_type": "default", "rope_theta": wavelength}, **kw)
    cfg._attn_implementation = "eager"
    model = transformers.LlamaForCausalLM(cfg).eval()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    sd = {"model.embed_tokens.weight": t(w["llama_micro_embed_tokens/embeddings"]),
          "model.norm.weight": t(w["llama_micro_norm/scale"]), "lm_head.weight": t(w["lm_head/kernel"].T)}
    for i in range(depth):
        b, p = f"llama_micro_block_{i}", f"model.layers.{i}."
        a = f"{b}_attn"
        sd[p + "input_layernorm.weight"] = t(w[f"{b}_input_norm/scale"])
        sd[p + "post_attention_layernorm.weight"] = t(w[f"{b}_post_attention_norm/scale"])
        for ours, theirs in (("query", "q_proj"), ("key", "k_proj"), ("value", "v_proj")):
            sd[p + f"self_attn.{theirs}.weight"] = t(w[f"{a}/{ours}/kernel"].reshape(C, -1).T)
        sd[p + "self_attn.o_proj.weight"] = t(w[f"{a}/attention_output/kernel"].reshape(-1, C).T)
        for ours, theirs in (("gate", "gate_proj"), ("up", "up_proj"), ("down", "down_proj")):
            sd[p + f"mlp.{theirs}.weight"] = t(w[f"{b}_mlp_{ours}/kernel"].T)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    model = model.double()
    with torch.no_grad():
        logits = model(input_ids=torch.from_numpy(ids).long()).logits.numpy()
    err, top = float(np.abs(logits - want).max()), float(np.abs(want).max())
    print(f"by hand vs transformers {transformers.__version__}: abs err {err:.3e} at max|logit| {top:.3e}")
    assert err <= 1e-6 * top


# ------------------------------------------------------------------ sliced runs
@pytest.mark.parametrize("cuts", [[CUT], "auto:3"], ids=["in_block", "auto3"])
def test_llama_micro_sliced_equals_unsliced_on_the_cpu_path(cuts):
    g, w, ids, _ = LC.micro()
    full = cpu_executor.CpuExecutor(g, w)(ids[:2])
    cut_names = AdaptConfig(part_at=cuts, batch=2).cuts(g) if isinstance(cuts, str) else cuts
    parts = slicer.partition(g, cut_names)
    assert len(parts) == len(cut_names) + 1
    slicer.validate_slices(g, parts)
    if cuts == [CUT]:                   # the norm's output and, beside it, the block's residual
        assert set(parts[1].inputs) == {CUT, "llama_micro_block_0_add1"}
    vals = {g.input: ids[:2]}
    for s in parts:
        sg = slicer.subgraph(g, s)
        vals.update(cpu_executor.CpuExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
    np.testing.assert_array_equal(vals[g.output], full)


# ------------------------------------------------------------------ command line
def test_cli_plans_and_runs_llama_micro_by_name():
    from test_vit import _cli
    r = _cli("plan", "--model", "llama_micro", "--stages", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "llama_micro" in r.stdout
    r = _cli("local-infer", "--model", "llama_micro", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-2000:]
