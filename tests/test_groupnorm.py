"""GroupNormalization without a GPU: the IR op and its refusals, Keras JSON in both serialisations, the PyTorch
oracle and the native CPU op against the float64 oracle of tests/groupnorm_cases.py, the plan's activation fold,
the Stable Diffusion VAE decoder of the zoo, and the plans of the older families, which must not move.
"""
import json
import os

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import planner
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    BUILDERS, VAE_DECODER, build_model)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

import groupnorm_cases as GN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_steps_before_groupnorm.json")


def _graph(shape=(4, 4, 8), **attrs):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": shape}))
    g.add(Layer("gn", "groupnorm", ["in"], dict({"groups": 2, "epsilon": 1e-5}, **attrs)))
    return g


# ------------------------------------------------------------------ IR
@pytest.mark.parametrize("shape,groups,word", [
    ((8,), 2, r"\(H, W, C\)"),            # not a map
    ((4, 8), 2, r"\(H, W, C\)"),
    ((4, 4, 8), 0, "groups"),
    ((4, 4, 8), -2, "groups"),
    ((4, 4, 8), 3, "divide"),             # C % G != 0
])
def test_graph_add_refuses_a_bad_groupnorm_by_name(shape, groups, word):
    with pytest.raises(ValueError, match=f"'norm_7'.*{word}"):
        g = Graph("t")
        g.add(Layer("in", "input", [], {"shape": shape}))
        g.add(Layer("norm_7", "groupnorm", ["in"], {"groups": groups, "epsilon": 1e-5}))


def test_graph_add_stores_the_resolved_group_count():
    assert _graph(groups=-1).layers["gn"].attrs["groups"] == 8          # instance norm: one group per channel
    g = _graph(groups=4)
    assert g.layers["gn"].attrs["groups"] == 4 and g.layers["gn"].out_shape == (4, 4, 8)
    assert g.layer_macs("gn") == 0


def test_weight_specs_follow_the_center_and_scale_flags():
    assert _graph().weight_specs() == [("gn/gamma", (8,)), ("gn/beta", (8,))]               # Keras order
    assert _graph(center=False).weight_specs() == [("gn/gamma", (8,))]
    assert _graph(scale=False).weight_specs() == [("gn/beta", (8,))]
    assert _graph(center=False, scale=False).weight_specs() == []
    w = init_weights(_graph(scale=False), 0)
    assert set(w) == {"gn/beta"} and w["gn/beta"].shape == (8,)


# ------------------------------------------------------------------ Keras JSON
def _k2(cls, name, inbound, **cfg):
    return {"class_name": cls, "name": name, "config": dict(cfg, name=name),
            "inbound_nodes": [[[i, 0, 0, {}] for i in inbound]] if inbound else []}


def _k3(cls, name, inbound, **cfg):
    args = [{"class_name": "__keras_tensor__", "config": {"shape": [None], "dtype": "float32",
                                                         "keras_history": [i, 0, 0]}} for i in inbound]
    return {"module": "keras.layers", "class_name": cls, "name": name, "config": dict(cfg, name=name),
            "inbound_nodes": [{"args": args, "kwargs": {}}] if inbound else []}


def _keras_model(L, keras3, axis=-1, groups=4, **flags):
    shape = {"batch_shape": [None, 6, 6, 8]} if keras3 else {"batch_input_shape": [None, 6, 6, 8]}
    layers = [
        L("InputLayer", "in", [], dtype="float32", **shape),
        L("GroupNormalization", "gn", ["in"], groups=groups, axis=axis, epsilon=1e-5, **flags),
        L("Activation", "sw", ["gn"], activation="swish"),
        L("GroupNormalization", "inst", ["sw"], groups=-1, axis=axis, epsilon=1e-3, center=True, scale=True),
    ]
    return json.dumps({"class_name": "Functional",
                       "config": {"name": "m", "layers": layers, "input_layers": [["in", 0, 0]],
                                  "output_layers": [["inst", 0, 0]]}})


@pytest.mark.parametrize("keras3", [False, True], ids=["keras2", "keras3"])
@pytest.mark.parametrize("axis", [-1, 3, [3]])
def test_keras_json_imports_groupnorm_and_round_trips(keras3, axis):
    g = from_keras_json(_keras_model(_k3 if keras3 else _k2, keras3, axis=axis, center=False, scale=True))
    gn, inst = g.layers["gn"], g.layers["inst"]
    assert gn.op == "groupnorm" and gn.attrs == {"groups": 4, "epsilon": 1e-5, "center": False}
    assert inst.attrs == {"groups": 8, "epsilon": 1e-3}                 # -1 resolved; flags stored only when False
    assert g.weight_specs() == [("gn/gamma", (8,)), ("inst/gamma", (8,)), ("inst/beta", (8,))]
    s = to_keras_json(g)
    layers = {ld["name"]: ld for ld in json.loads(s)["config"]["layers"]}
    assert layers["gn"]["class_name"] == "GroupNormalization" and layers["gn"]["config"]["groups"] == 4
    assert layers["gn"]["config"]["center"] is False and layers["gn"]["config"]["scale"] is True
    assert json.loads(from_keras_json(s).to_json()) == json.loads(g.to_json())


@pytest.mark.parametrize("keras3", [False, True], ids=["keras2", "keras3"])
def test_keras_json_refuses_another_axis_by_layer_name(keras3):
    with pytest.raises(NotImplementedError, match="gn.*axis"):
        from_keras_json(_keras_model(_k3 if keras3 else _k2, keras3, axis=1))


def test_keras_json_refuses_groups_that_do_not_divide_by_layer_name():
    with pytest.raises(ValueError, match="'gn'"):
        from_keras_json(_keras_model(_k2, False, groups=3))


def test_the_decoder_round_trips_through_keras_json():
    g = build_model("vae_decoder_micro")
    assert json.loads(from_keras_json(to_keras_json(g)).to_json()) == json.loads(g.to_json())


# ------------------------------------------------------------------ the two CPU implementations
def _layer_graph(k):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (k.H, k.W, k.C)}))
    a = {"groups": k.groups, "epsilon": k.eps}
    if not k.center:
        a["center"] = False
    if not k.scale:
        a["scale"] = False
    g.add(Layer("gn", "groupnorm", ["in"], a))
    if k.act:
        g.add(Layer("act", "act", ["gn"], {"fn": k.act}))
    g.output_names = [g.order[-1]]
    w = {}
    if k.scale:
        w["gn/gamma"] = k.gamma
    if k.center:
        w["gn/beta"] = k.beta
    return g, w


@pytest.mark.parametrize("c", GN.CASES, ids=str)
def test_pytorch_oracle_is_within_the_allowance(c):
    k = GN.case(c)
    g, w = _layer_graph(k)
    got = ReferenceExecutor(g, w)(torch.from_numpy(k.x)).numpy().astype(np.float64)
    err = np.abs(got - k.want).max()
    print(f"ReferenceExecutor {c}: max err {err:.3e}, allowance {k.allow:.3e}")
    assert got.shape == k.want.shape and err <= k.allow


@pytest.mark.parametrize("c", GN.CASES, ids=str)
def test_native_cpu_op_is_within_the_allowance(c):
    k = GN.case(c)
    y = np.full(k.x.shape, np.nan, np.float32)
    cpu_executor.native().groupnorm(k.x, k.gamma_k, k.beta_k, y, k.G, k.eps, k.act_mode, 0.3)
    err = np.abs(y.astype(np.float64) - k.want).max()
    print(f"_cpu.groupnorm {c}: max err {err:.3e}, allowance {k.allow:.3e}")
    assert np.isfinite(y).all() and err <= k.allow


def test_native_cpu_op_checks_its_arguments():
    k = GN.case(GN.CASES[2])
    y = np.empty(k.x.shape, np.float32)
    for args in ((k.x, k.gamma_k, k.beta_k, y, 3, k.eps),                     # C % G != 0
                 (k.x, k.gamma_k[:-1], k.beta_k, y, k.G, k.eps),              # gamma too short
                 (k.x, k.gamma_k, k.beta_k, y[:, :-1], k.G, k.eps),           # output of another shape
                 (k.x.reshape(-1, k.C), k.gamma_k, k.beta_k, y, k.G, k.eps)):  # not a map
        with pytest.raises(Exception, match="groupnorm"):
            cpu_executor.native().groupnorm(*args)


@pytest.mark.parametrize("i", [5, 6])
def test_the_one_pass_form_fails_the_cancellation_probes(i):
    """Why the kernels never form E[x^2] - mu^2: in fp32 it misses the allowance by orders of magnitude here."""
    k = GN.case(GN.CASES[i])
    err = np.abs(GN.one_pass_f32(k.x, k.gamma, k.beta, k.groups, k.eps).astype(np.float64) - k.want).max()
    print(f"one-pass fp32 {GN.CASES[i]}: max err {err:.3e} = {err / k.allow:.0f}x the allowance {k.allow:.3e}")
    assert err > 100 * k.allow


# ------------------------------------------------------------------ the plan
def _gn_swish(extra=None):
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (8, 8, 16)}))
    g.add(Layer("gn", "groupnorm", ["in"], {"groups": 4, "epsilon": 1e-5}))
    g.add(Layer("sw", "act", ["gn"], {"fn": "swish"}))
    g.add(Layer("cv", "conv", ["sw"], {"filters": 16, "kernel": (3, 3), "stride": 1, "padding": "same",
                                       "use_bias": True}))
    g.output_names = ["cv"]
    if extra:
        g.add(Layer("sum", "add", ["gn", "cv"]))
        g.output_names = ["sum"]
    return g


@pytest.mark.parametrize("fp32", [True, False])
def test_groupnorm_then_swish_is_one_step(fp32):
    steps = [s for s in compile_plan(_gn_swish(), fp32=fp32) if s.kind != "pack"]
    assert [s.kind for s in steps] == ["groupnorm", "conv"]
    assert steps[0].out == "sw" and steps[0].covers == ["gn", "sw"]
    assert steps[0].p == {"layer": "gn", "groups": 4, "eps": 1e-5, "act": 3}


@pytest.mark.parametrize("fp32", [True, False])
def test_a_cut_or_a_second_consumer_keeps_the_activation_apart(fp32):
    cut = [s for s in compile_plan(_gn_swish(), outputs=["gn", "cv"], fp32=fp32) if s.kind != "pack"]
    assert [s.kind for s in cut] == ["groupnorm", "act", "conv"] and cut[0].out == "gn" and cut[0].p["act"] == 0
    two = [s for s in compile_plan(_gn_swish(extra=True), fp32=fp32) if s.kind != "pack"]
    assert [s.kind for s in two][:2] == ["groupnorm", "act"] and two[0].out == "gn" and two[0].p["act"] == 0


def test_relu_folds_and_leaky_relu_does_not():
    g = _gn_swish()
    g.layers["sw"].op, g.layers["sw"].attrs = "relu", {"max_value": 6.0}
    assert compile_plan(g, fp32=True)[0].p["act"] == 2
    g.layers["sw"].op, g.layers["sw"].attrs = "act", {"fn": "leaky_relu", "alpha": 0.1}
    assert [s.kind for s in compile_plan(g, fp32=True)][:2] == ["groupnorm", "act"]


def test_planner_costs_groupnorm_by_its_bytes_and_passes():
    g = _gn_swish()
    hw = planner.HwModel()
    cost = planner.layer_costs(g, batch=4, hw=hw)
    byts = 2 * g.tensor_bytes("gn", hw.act_bytes) * 4                  # read once, written once
    assert cost["gn"] == pytest.approx(1.5 * byts / hw.hbm_bw + 3 * hw.launch_s)


# ------------------------------------------------------------------ the decoder
def _decoder_params(widths, nblocks, latent_c):
    """Closed formula from the widths: GN has 2 C, a k x k conv k^2 cin cout + cout, the attention block a GN and
    four C x C projections with biases."""
    def conv(k, cin, cout):
        return k * k * cin * cout + cout

    def block(cin, cout):
        return 2 * cin + conv(3, cin, cout) + 2 * cout + conv(3, cout, cout) + (conv(1, cin, cout) if cin != cout else 0)

    w0 = widths[0]
    total = conv(1, latent_c, latent_c) + conv(3, latent_c, w0)
    total += 2 * block(w0, w0) + 2 * w0 + 4 * (w0 * w0 + w0)
    cin = w0
    for i, f in enumerate(widths):
        total += block(cin, f) + (nblocks - 1) * block(f, f)
        if i + 1 < len(widths):
            total += conv(3, f, f)
        cin = f
    return total + 2 * cin + conv(3, cin, 3)


def test_sd_vae_decoder_has_the_published_parameter_total():
    g = build_model("sd_vae_decoder")
    assert _decoder_params((512, 512, 256, 128), 3, 4) == 49_490_199
    assert g.count_params() == 49_490_199
    assert g.layers[g.input].out_shape == (64, 64, 4) and g.layers[g.output].out_shape == (512, 512, 3)
    assert 2 * 512 + 2 * (9 * 512 * 512 + 512) + 2 * 512 == 4_721_664                 # one 512 block
    gns = [n for n in g.order if g.layers[n].op == "groupnorm"]
    assert len(gns) == 30 and all(g.layers[n].attrs == {"groups": 32, "epsilon": 1e-5} for n in gns)
    assert g.layers["rescaling"].attrs["scale"] == pytest.approx(1 / 0.18215)
    assert g.layers["mid_attn"].attrs == {"num_heads": 1, "key_dim": 512, "use_bias": True}
    assert [g.layers[n].attrs["size"] for n in g.order if g.layers[n].op == "upsample"] == [(2, 2)] * 3


def test_vae_decoder_micro_structure_and_plan():
    g = build_model("vae_decoder_micro")
    widths, nblocks, groups, latent = VAE_DECODER["vae_decoder_micro"]
    assert (widths, nblocks, groups, latent) == ((32, 32, 16, 8), 1, 4, (8, 8, 4))
    assert g.count_params() == _decoder_params(widths, nblocks, 4)
    assert g.layers[g.output].out_shape == (64, 64, 3) and g.layers["mid_attn"].attrs["key_dim"] == 32
    assert {"sd_vae_decoder", "vae_decoder_micro"} <= set(BUILDERS)
    for fp32 in (True, False):
        steps = compile_plan(g, fp32=fp32)
        gn = [s for s in steps if s.kind == "groupnorm"]
        assert len(gn) == 14 and [s.p["act"] for s in gn].count(3) == 13           # all but the attention block's
        for i, s in enumerate(steps[:-1]):
            assert not (s.kind == "groupnorm" and steps[i + 1].kind == "act")
        attn = next(i for i, s in enumerate(steps) if s.kind == "attention")
        assert steps[attn - 2].kind == "groupnorm" and steps[attn - 2].p["act"] == 0
        assert steps[attn + 1].kind == "conv" and steps[attn + 1].p["residual"] == "mid_block1_add"


@pytest.fixture(scope="module")
def micro():
    g = build_model("vae_decoder_micro")
    w = init_weights(g, seed=0)
    x = np.random.default_rng(3).standard_normal((2, 8, 8, 4)).astype(np.float32) * 0.18215 * 4.0
    want = ReferenceExecutor(g, w, device="cpu")(torch.from_numpy(x)).numpy()
    return g, w, x, want


def test_cpu_executor_runs_vae_decoder_micro_within_the_family_budget(micro):
    g, w, x, want = micro
    ex = cpu_executor.CpuExecutor(g, w)
    assert [s.kind for s in ex.steps].count("groupnorm") == 14
    got = ex(x)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"vae_decoder_micro CpuExecutor rel err {rel:.3e}")
    assert got.shape == (2, 64, 64, 3) and np.isfinite(got).all() and rel <= 1e-3


# ------------------------------------------------------------------ nothing else moves
@pytest.mark.parametrize("model", ["resnet50", "convnext_tiny", "unet", "vit_b16", "swin_tiny"])
def test_the_plans_of_the_older_families_are_unchanged(model):
    """tests/golden/plan_steps_before_groupnorm.json: "kind output" of every step, fp32 and bf16, recorded from the
    commit before GroupNormalization."""
    with open(GOLDEN) as f:
        before = json.load(f)[model]
    g = build_model(model)
    for precision in ("fp32", "bf16"):
        now = [f"{s.kind} {s.out}" for s in compile_plan(g, fp32=precision == "fp32")]
        assert now == before[precision], f"{model} {precision}"
