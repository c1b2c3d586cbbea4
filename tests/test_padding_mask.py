"""Padding masks from Embedding(mask_zero=True) without a GPU: the Keras importer and writer, `propagate_masks`,
the plan, the native CPU op against the float64 oracles of tests/padding_mask_cases.py, DistilBERT sliced against
unsliced on the CPU path, and its parameter totals.
"""
import json
import os

import numpy as np
import pytest

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import (
    Graph, Layer, holds_token_ids, mha_sources, propagate_masks, with_key_masks)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    DISTILBERT, DISTILBERT_FFN_RATIO, build_distilbert, build_model)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.utils.config import AdaptConfig

import padding_mask_cases as PC
from test_vit import _k2, _k3

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_steps_before_padding_mask.json")
T, V, C = 12, 50, 8


# ------------------------------------------------------------------ Keras JSON
def _doc(L, keras3=False, mask_zero=True, attn_inbound=("ln",), attn_call=None, tail=(), cfg=None):
    """Embedding -> LayerNormalization -> MultiHeadAttention -> Add -> LayerNormalization -> MultiHeadAttention,
    plus `tail` layers."""
    shape = {"batch_shape": [None, T]} if keras3 else {"batch_input_shape": [None, T]}
    mha = dict(num_heads=2, key_dim=4, value_dim=4, dropout=0.0, use_bias=True, output_shape=None, attention_axes=None)
    mha.update(cfg or {})
    layers = [
        L("InputLayer", "ids", [], dtype="float32", **shape),
        L("Embedding", "emb", ["ids"], input_dim=V, output_dim=C, mask_zero=mask_zero, input_length=T),
        L("LayerNormalization", "ln", ["emb"], axis=[-1], epsilon=1e-6, center=True, scale=True),
        L("MultiHeadAttention", "attn", list(attn_inbound), call=attn_call if attn_call is not None else {"value": "ln"},
          **mha),
        L("Add", "add", ["emb", "attn"]),
        L("LayerNormalization", "ln2", ["add"], axis=[-1], epsilon=1e-6, center=True, scale=True),
        L("MultiHeadAttention", "attn2", ["ln2"], call={"value": "ln2"}, **mha),
    ] + list(tail)
    out = tail[-1]["name"] if tail else "attn2"
    return json.dumps({"class_name": "Functional", "config": {"name": "blk", "layers": layers,
                                                              "input_layers": [["ids", 0, 0]],
                                                              "output_layers": [[out, 0, 0]]}})


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_default_import_still_refuses_mask_zero_by_layer_name_with_the_hint(L, keras3):
    with pytest.raises(NotImplementedError, match=r"emb.*mask_zero.*padding_mask=True"):
        from_keras_json(_doc(L, keras3))
    for kw in ({"cross_attention": True}, {"causal_attention": True}):
        with pytest.raises(NotImplementedError, match=r"emb.*mask_zero"):
            from_keras_json(_doc(L, keras3), **kw)
    g = from_keras_json(_doc(L, keras3, mask_zero=False))           # without the mask nothing changes
    assert g.layers["attn"].inputs == ["ln"] and "key_mask" not in g.layers["attn"].attrs
    assert "mask_zero" not in g.layers["emb"].attrs


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_flagged_import_sets_key_mask_on_every_reached_mha_and_round_trips(L, keras3):
    doc = _doc(L, keras3)
    g = from_keras_json(doc, padding_mask=True)
    assert g.layers["emb"].attrs["mask_zero"] is True
    for n, src in (("attn", "ln"), ("attn2", "ln2")):
        assert g.layers[n].inputs == [src, "ids"], n
        assert g.layers[n].attrs["key_mask"] is True
        assert mha_sources(g.layers[n].inputs, True) == (src, src, src)
    assert propagate_masks(g) == {"attn": "ids", "attn2": "ids"}
    assert holds_token_ids(g, "ids") and not holds_token_ids(g, "ln")
    assert set(g.consumers()["ids"]) == {"emb", "attn", "attn2"}    # a real edge
    assert "ids" in g.ancestors("attn2")
    s = to_keras_json(g)
    written = {ld["name"]: ld for ld in json.loads(s)["config"]["layers"]}
    assert written["emb"]["config"]["mask_zero"] is True
    assert [e[0] for e in written["attn"]["inbound_nodes"][0]] == ["ln"]        # the call without the extra input
    assert written["attn"]["inbound_nodes"][0][0][3] == {"value": ["ln", 0, 0]}
    assert json.loads(from_keras_json(s, padding_mask=True).to_json()) == json.loads(g.to_json())
    with pytest.raises(NotImplementedError, match=r"emb.*mask_zero.*padding_mask=True"):
        from_keras_json(s)
    m = Model.from_keras_json(doc, seed=2)                          # what the command line uses asks for it
    assert m.graph.layers["attn2"].attrs.get("key_mask") is True
    # Graph JSON keeps the edge and the attribute
    assert json.loads(Graph.from_json(g.to_json()).to_json()) == json.loads(g.to_json())


def test_refusals_by_layer_name():
    with pytest.raises(NotImplementedError, match="attn.*causal"):
        from_keras_json(_doc(_k2, attn_call={"value": "ln", "use_causal_mask": True}), padding_mask=True,
                        causal_attention=True)
    with pytest.raises(NotImplementedError, match="attn.*separate sources"):
        from_keras_json(_doc(_k2, attn_inbound=("ln",), attn_call={"value": "emb"}), padding_mask=True,
                        cross_attention=True)
    gap = _k2("GlobalAveragePooling2D", "pool", ["attn2"], data_format="channels_last", keepdims=False)
    with pytest.raises(NotImplementedError, match="pool.*padding mask"):
        from_keras_json(_doc(_k2, tail=[gap]), padding_mask=True)
    with pytest.raises(NotImplementedError, match="attn.*attention_mask"):
        from_keras_json(_doc(_k2, attn_call={"value": "ln", "attention_mask": "ids"}), padding_mask=True)
    pos = _k2("ClassTokenPositionEmbedding", "pos", ["attn2"], class_token=True)
    with pytest.raises(NotImplementedError, match="pos.*class token"):
        from_keras_json(_doc(_k2, tail=[pos]), padding_mask=True)
    pos = _k2("ClassTokenPositionEmbedding", "pos", ["attn2"], class_token=False)
    assert from_keras_json(_doc(_k2, tail=[pos]), padding_mask=True).layers["pos"].out_shape == (1, T, C)


def _hand(mask_edges=("attn",), second_ids=False):
    g = Graph("t")
    g.add(Layer("ids", "input", [], {"shape": (T,)}))
    if second_ids:
        g.add(Layer("ids2", "input", [], {"shape": (T,)}))
    g.add(Layer("emb", "embedding", ["ids"], {"input_dim": V, "output_dim": C, "mask_zero": True}))
    g.add(Layer("emb2", "embedding", ["ids2" if second_ids else "ids"], {"input_dim": V, "output_dim": C}))
    a = {"num_heads": 2, "key_dim": 4, "use_bias": True}
    for n, src in (("attn", "emb"), ("plain", "emb2")):
        if n in mask_edges:
            g.add(Layer(n, "mha", [src, "ids"], dict(a, key_mask=True)))
        else:
            g.add(Layer(n, "mha", [src], dict(a)))
    g.output_names = ["attn"]
    return g


def test_the_writer_refuses_a_key_mask_edge_the_propagation_would_not_derive():
    assert json.loads(from_keras_json(to_keras_json(_hand()), padding_mask=True).to_json())["layers"]
    with pytest.raises(NotImplementedError, match="plain.*key_mask"):          # emb2 has no mask_zero
        to_keras_json(_hand(mask_edges=("attn", "plain")))
    with pytest.raises(NotImplementedError, match="attn.*key_mask"):           # the mask reaches attn: edge missing
        to_keras_json(_hand(mask_edges=()))
    g = _hand(second_ids=True)
    g.layers["attn"].inputs[-1] = "ids2"                                       # hand-edited to another tensor
    with pytest.raises(NotImplementedError, match="attn.*key_mask"):
        to_keras_json(g)
    assert with_key_masks(_hand(mask_edges=())).layers["attn"].inputs == ["emb", "ids"]


def test_ir_validation_of_key_mask():
    def g(inputs, shape=(T,), **attrs):
        g = Graph("t")
        g.add(Layer("ids", "input", [], {"shape": shape}))
        g.add(Layer("x", "input", [], {"shape": (T, C)}))
        g.add(Layer("y", "input", [], {"shape": (T, C)}))
        g.add(Layer("attn", "mha", list(inputs), dict({"num_heads": 2, "key_dim": 4}, **attrs)))
        return g
    ok = g(["x", "ids"], key_mask=True)
    plain = g(["x"])
    assert ok.layer_macs("attn") == plain.layer_macs("attn")        # costs what the unmasked one costs
    assert ok.layers["attn"].weight_shapes(ok.in_shapes("attn")) == plain.layers["attn"].weight_shapes(
        plain.in_shapes("attn"))
    assert ok.layers["attn"].out_shape == (T, C)
    with pytest.raises(ValueError, match="attn.*key_mask"):
        g(["x", "ids"], key_mask=False)
    with pytest.raises(ValueError, match="attn.*key_mask"):
        g(["x", "ids"], key_mask=1)
    with pytest.raises(ValueError, match="attn.*causal"):
        g(["x", "ids"], key_mask=True, causal=True)
    with pytest.raises(ValueError, match="attn.*one source"):
        g(["x", "y", "ids"], key_mask=True)
    with pytest.raises(ValueError, match="attn.*one source"):
        g(["x"], key_mask=True)
    with pytest.raises(ValueError, match="attn.*token count"):
        g(["x", "ids"], shape=(T + 1,), key_mask=True)
    two = Graph("t")
    two.add(Layer("a", "input", [], {"shape": (T,)}))
    two.add(Layer("b", "input", [], {"shape": (T,)}))
    two.add(Layer("ea", "embedding", ["a"], {"input_dim": V, "output_dim": C, "mask_zero": True}))
    two.add(Layer("eb", "embedding", ["b"], {"input_dim": V, "output_dim": C, "mask_zero": True}))
    two.add(Layer("sum", "add", ["ea", "eb"]))
    with pytest.raises(NotImplementedError, match="sum.*two different"):
        propagate_masks(two)


# ------------------------------------------------------------------ plan
@pytest.mark.parametrize("model", ["gpt_micro", "vit_micro", "detr_micro"])
def test_the_step_lists_of_the_other_attention_families_are_unchanged(model):
    """tests/golden/plan_steps_before_padding_mask.json: kind, output, inputs and parameters of every step, fp32
    and bf16, recorded from the commit before padding masks."""
    def js(v):
        if isinstance(v, dict):
            return {str(k): js(x) for k, x in sorted(v.items(), key=lambda kv: str(kv[0]))}
        if isinstance(v, (list, tuple)):
            return [js(x) for x in v]
        return v if isinstance(v, (str, int, float, bool)) or v is None else repr(v)
    with open(GOLDEN) as f:
        before = json.load(f)[model]
    g = build_model(model)
    for precision in ("fp32", "bf16"):
        now = [{"kind": s.kind, "out": s.out, "ins": list(s.ins), "p": js(s.p)}
               for s in compile_plan(g, fp32=precision == "fp32")]
        assert now == before[precision], f"{model} {precision}"
        assert not any("key_mask" in s["p"] for s in now)


BLOCK_KINDS = ["conv", "attention", "conv", "layernorm", "conv", "act", "conv", "layernorm"]


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32", "bf16"])
def test_distilbert_micro_compiles_to_masked_attention_steps(fp32):
    g = build_model("distilbert_micro")
    steps = compile_plan(g, fp32=fp32)
    assert [s.kind for s in steps] == ["embedding", "posembed", "layernorm"] + BLOCK_KINDS * 2     # no pack step
    att = [s for s in steps if s.kind == "attention"]
    assert [s.p.get("key_mask") for s in att] == [True, True]
    assert all(s.ins == [s.p["layer"] + "#qkv", g.input] for s in att)
    assert all("causal" not in s.p for s in att)


# ------------------------------------------------------------------ native CPU op
@pytest.mark.parametrize("c", PC.CASES, ids=str)
def test_cpu_attention_with_key_mask_against_both_oracles(c):
    k = PC.case(c)
    for gr in k.groups:
        y = np.full(gr.want.shape, np.nan, np.float32)
        cpu_executor.native().attention(k.qkv, y, k.B, k.T, k.heads, k.d, k.dv, key_mask=gr.mask.reshape(-1))
        got = y.astype(np.float64)
        err = np.abs(got - gr.want).max()
        print(f"cpu masked attention {c} {gr.group}: e_ref {gr.e_ref:.3e}, max err {err:.3e}, allowance {gr.allow:.3e}")
        assert np.isfinite(got).all() and err <= gr.allow           # the project's semantics, all rows
        assert (y[~gr.rows] == 0).all()                             # padded rows and no-key images: exact zeros
        if gr.rows.any():                                           # Keras' semantics, kept rows: the equivalence
            keras = PC.ref_keras(k.qkv, gr.mask, k.B, k.T, k.heads, k.d, k.dv)
            np.testing.assert_allclose(gr.want[gr.rows], keras[gr.rows], rtol=1e-12, atol=1e-12)
            assert np.abs(got[gr.rows] - keras[gr.rows]).max() <= gr.allow


def test_cpu_attention_default_has_no_mask_and_an_all_kept_mask_changes_nothing():
    c = (16, PC.KT + 1)
    k = PC.case(c)
    y, z, m = (np.empty(k.want.shape, np.float32) for _ in range(3))
    cpu_executor.native().attention(k.qkv, y, k.B, k.T, k.heads, k.d, k.dv)
    cpu_executor.native().attention(k.qkv, z, k.B, k.T, k.heads, k.d, k.dv, key_mask=None)
    cpu_executor.native().attention(k.qkv, m, k.B, k.T, k.heads, k.d, k.dv,
                                    key_mask=np.ones(k.B * k.T, np.float32))
    np.testing.assert_array_equal(y, z)
    np.testing.assert_array_equal(y, m)
    assert np.abs(y.astype(np.float64) - k.want).max() <= k.allow
    with pytest.raises(Exception):
        cpu_executor.native().attention(k.qkv, y, k.B, k.T, k.heads, k.d, k.dv, causal=True,
                                        key_mask=np.ones(k.B * k.T, np.float32))
    with pytest.raises(Exception):
        cpu_executor.native().attention(k.qkv, y, k.B, k.T, k.heads, k.d, k.dv, key_mask=np.ones(5, np.float32))


def test_the_oracles_and_the_allowance():
    for c in PC.CASES:
        k = PC.case(c)
        for gr in k.groups:
            floor = 2e-5 * max(1.0, float(np.abs(gr.want).max()))
            assert gr.e_ref <= 5e-5 and gr.allow == max(4.0 * gr.e_ref, floor), (c, gr.e_ref)
        allk = k.groups[0]
        np.testing.assert_allclose(allk.want[:k.T], k.want[:k.T], rtol=1e-12, atol=1e-12)      # image 0: all kept


# ------------------------------------------------------------------ DistilBERT
def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_distilbert_micro_on_the_cpu_path_and_the_reference_match_the_model_by_hand():
    g, w, ids, want = PC.micro()
    keep = PC.kept(ids)
    got = cpu_executor.CpuExecutor(g, w)(ids).reshape(want.shape)
    ref = ReferenceExecutor(g, w, device="cpu").run({g.input: __import__("torch").from_numpy(ids)})[g.output]
    ref = ref.numpy().reshape(want.shape)
    print(f"distilbert_micro cpu rel err {_rel(got, want):.3e}, reference {_rel(ref, want):.3e}")
    assert _rel(got, want) <= 1e-3 and _rel(ref, want) <= 1e-3      # every position, the project's semantics
    keras = PC.forward("distilbert_micro", 2, w, ids, keras=True)
    assert _rel(keras[keep], want[keep]) <= 1e-9                    # kept positions are Keras'
    assert _rel(got[keep], keras[keep]) <= 1e-3
    assert np.abs(keras[~keep] - want[~keep]).max() > 1e-2          # padded positions are not, by design


@pytest.mark.parametrize("cuts", [["distilbert_micro_layer_0_ffn_lin1"], "auto:3"], ids=["ffn", "auto3"])
def test_distilbert_micro_sliced_equals_unsliced_and_the_ids_cross_every_cut(cuts):
    g, w, ids, _ = PC.micro()
    full = cpu_executor.CpuExecutor(g, w)(ids[:2])
    cut_names = AdaptConfig(part_at=cuts, batch=2).cuts(g) if isinstance(cuts, str) else cuts
    parts = slicer.partition(g, cut_names)
    assert len(parts) == len(cut_names) + 1
    slicer.validate_slices(g, parts)
    assert parts[0].relay == [g.input]                              # stage 0 relays the graph input itself
    masked = [n for n in g.order if g.layers[n].attrs.get("key_mask")]
    for s in parts[:-1]:
        # the ids cross every cut that has a masked attention layer behind it (the planner may put its last cut
        # behind the last one, where nothing reads them any more)
        later = any(n in p.layers for p in parts[s.index + 1:] for n in masked)
        assert (g.input in s.outputs) == later, s.name
    assert g.input in parts[0].outputs
    vals = {g.input: ids[:2]}
    for s in parts:
        sg = slicer.subgraph(g, s)
        assert g.input not in sg.input_names or holds_token_ids(sg, g.input)
        vals.update(cpu_executor.CpuExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
    np.testing.assert_array_equal(vals[g.output], full)


def _closed_form(depth, width, vocab, tokens):
    attn = 4 * (width * width + width)
    ffn = 2 * DISTILBERT_FFN_RATIO * width * width + DISTILBERT_FFN_RATIO * width + width
    return vocab * width + tokens * width + 2 * width + depth * (attn + ffn + 4 * width)


@pytest.mark.parametrize("name,tokens", [("distilbert_base", 512), ("distilbert_base", 128), ("distilbert_micro", 40),
                                         ("distilbert_micro", 7)])
def test_parameter_totals_in_closed_form(name, tokens):
    depth, width, heads, vocab, default = DISTILBERT[name]
    g = build_distilbert(name, input_shape=(tokens,))
    assert g.count_params() == _closed_form(depth, width, vocab, tokens)
    if (name, tokens) == ("distilbert_base", 512):
        assert g.count_params() == 66_362_880                       # the published figure
    assert g.layers[g.output].out_shape == (1, tokens, width)
    assert build_model(name).layers["input_1"].out_shape == (default,)
    eps = {L.attrs["epsilon"] for L in g.layers.values() if L.op == "layernorm"}
    assert eps == {1e-12}
    assert {L.attrs.get("activation") for L in g.layers.values() if L.op == "dense"} == {"gelu", None}


def test_cli_plans_and_runs_distilbert_micro_by_name():
    from test_vit import _cli
    r = _cli("plan", "--model", "distilbert_micro", "--stages", "2")
    assert r.returncode == 0, r.stderr[-2000:]
    assert "distilbert_micro" in r.stdout
    r = _cli("local-infer", "--model", "distilbert_micro", "--device", "cpu")
    assert r.returncode == 0, r.stderr[-2000:]
