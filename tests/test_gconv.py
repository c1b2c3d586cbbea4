"""Grouped convolution (Keras Conv2D(groups > 1)) and ResNeXt, the parts that need no GPU: IR, Keras JSON,
launch plan, weight packing of the MFMA path, the native CPU op, slicing and DEFER serving.

Shapes and the float64 oracle: tests/gconv_cases.py.  The HIP kernel itself: tests/test_gconv_gpu.py.
"""
import itertools
import json
import queue
import threading

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.dispatcher import DEFER
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.node import Node
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

import gconv_cases as GC

TINY_SHAPE = (64, 64, 3)


def _rel(a, b):
    """tests/test_cpu_native.py's metric."""
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


# ------------------------------------------------------------------ IR, zoo
@pytest.mark.parametrize("name,params", [("resnext50_32x4d", 25_097_128), ("resnext101_32x4d", 44_315_560)])
def test_resnext_parameter_totals(name, params):
    g = build_model(name)
    assert g.count_params() == params
    assert g.layers[g.output].out_shape == (1000,)
    for stage, w in zip((2, 3, 4, 5), (128, 256, 512, 1024)):
        n = f"conv{stage}_block1_2_conv"
        assert g.layers[n].weight_shapes(g.in_shapes(n)) == [(f"{n}/kernel", (3, 3, w // 32, w))]
        assert g.layers[n].attrs["groups"] == 32 and g.layers[n].attrs["stride"] == (1 if stage == 2 else 2)
        assert g.layers[f"conv{stage}_block1_3_conv"].attrs["filters"] == 2 * w


def test_groups_attr_is_absent_from_existing_graphs_and_checked_on_add():
    assert '"groups"' not in build_model("resnet50").to_json()
    assert '"groups"' not in build_model("mobilenet_v2").to_json()
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (8, 8, 12)}))
    for groups, filters in ((5, 20), (4, 18)):          # not a divisor of the input channels / of filters
        with pytest.raises(ValueError, match="groups"):
            g.add(Layer("c", "conv", ["in"], {"filters": filters, "kernel": (3, 3), "groups": groups}))
    g.add(Layer("c", "conv", ["in"], {"filters": 18, "kernel": (3, 3), "groups": 3}))
    assert g.weight_specs(["c"])[0] == ("c/kernel", (3, 3, 4, 18))
    assert g.layer_macs("c") == 6 * 6 * 18 * 9 * 4


def test_macs_divide_by_groups_and_init_is_he_normal_over_the_group_fan_in():
    g = build_model("resnext_tiny", input_shape=TINY_SHAPE)
    n = "conv3_block1_2_conv"
    oh, ow, co = g.layers[n].out_shape
    assert g.layer_macs(n) == oh * ow * co * 9 * (256 // 32)
    k = init_weights(g, 0, layers=[n])[f"{n}/kernel"]
    assert k.shape == (3, 3, 8, 256)
    assert abs(k.std() / np.sqrt(2.0 / (9 * 8)) - 1.0) < 0.02          # 18432 samples: sigma of the estimate 0.5 %


# ------------------------------------------------------------------ Keras JSON
def _keras_conv(groups=1, dilation=1):
    def L(cls, name, cfg, inbound):
        return {"class_name": cls, "name": name, "config": dict(cfg, name=name),
                "inbound_nodes": [[[i, 0, 0, {}] for i in inbound]] if inbound else []}
    layers = [
        L("InputLayer", "in", {"batch_input_shape": [None, 8, 8, 8], "dtype": "float32"}, []),
        L("Conv2D", "gc", {"filters": 16, "kernel_size": [3, 3], "strides": [1, 1], "padding": "same",
                           "data_format": "channels_last", "dilation_rate": [dilation, dilation], "groups": groups,
                           "activation": "relu", "use_bias": True}, ["in"]),
    ]
    return json.dumps({"class_name": "Functional", "keras_version": "2.15.0", "backend": "tensorflow",
                       "config": {"name": "m", "layers": layers, "input_layers": [["in", 0, 0]],
                                  "output_layers": [["gc", 0, 0]]}})


def test_keras_json_imports_groups_and_still_rejects_dilation():
    g = from_keras_json(_keras_conv(groups=4))
    assert g.layers["gc"].attrs["groups"] == 4
    assert g.weight_specs(["gc"]) == [("gc/kernel", (3, 3, 2, 16)), ("gc/bias", (16,))]
    assert "groups" not in from_keras_json(_keras_conv(groups=1)).layers["gc"].attrs
    with pytest.raises(NotImplementedError, match="dilat"):
        from_keras_json(_keras_conv(groups=1, dilation=2))
    with pytest.raises(NotImplementedError, match="dilat"):
        from_keras_json(_keras_conv(groups=4, dilation=2))
    # the imported layer runs: oracle vs the dense block-diagonal expansion
    w = init_weights(g, 3)
    x = torch.randn(2, 8, 8, 8, generator=torch.Generator().manual_seed(0))
    got = ReferenceExecutor(g, w)(x)
    gd = from_keras_json(_keras_conv(groups=1))
    wd = {"gc/kernel": GC.dense_kernel(w["gc/kernel"], 4), "gc/bias": w["gc/bias"]}
    torch.testing.assert_close(got, ReferenceExecutor(gd, wd)(x), rtol=1e-5, atol=1e-6)


def test_keras_json_round_trips_resnext_tiny():
    g = build_model("resnext_tiny")
    s = to_keras_json(g)
    convs = {ld["name"]: ld["config"] for ld in json.loads(s)["config"]["layers"] if ld["class_name"] == "Conv2D"}
    assert convs["conv4_block1_2_conv"]["groups"] == 32 and convs["conv4_block1_1_conv"]["groups"] == 1
    assert json.loads(from_keras_json(s).to_json()) == json.loads(g.to_json())


# ------------------------------------------------------------------ plan
@pytest.mark.parametrize("fp32,device_fusions", [(True, True), (True, False), (False, True)])
def test_resnext_tiny_plan_has_four_gconv_steps_nothing_else_touches(fp32, device_fusions):
    g = build_model("resnext_tiny")
    steps = compile_plan(g, fp32=fp32, device_fusions=device_fusions)
    gc = [s for s in steps if s.kind == "gconv"]
    assert len(gc) == 4
    for stage, st in zip((2, 3, 4, 5), gc):
        b = f"conv{stage}_block1_2"
        assert st.covers == [f"{b}_pad", f"{b}_conv", f"{b}_bn", f"{b}_relu"]
        assert st.out == f"{b}_relu" and st.ins == [f"conv{stage}_block1_1_relu"]
        assert st.p == {"conv": f"{b}_conv", "bn": f"{b}_bn", "relu": 1, "pads": ((1, 1), (1, 1)),
                        "stride": 1 if stage == 2 else 2, "kernel": (3, 3), "filters": 64 << (stage - 1), "groups": 32}
    # no pair / stem / sibling / bottleneck step consumed or merged a grouped layer
    grouped = {c for st in gc for c in st.covers}
    for st in steps:
        if st.kind != "gconv":
            assert not grouped & set(st.covers), (st.kind, st.covers)
            assert "groups" not in st.p and "groups" not in (st.p.get("sibling") or {})
    # the Add after the block is a conv's residual (the 1x1 _3_conv), never the grouped conv's
    assert all("residual" not in st.p for st in gc)


def test_grouped_conv_own_activation_and_post_activation():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (8, 8, 16)}))
    g.add(Layer("a", "conv", ["in"], {"filters": 16, "kernel": (3, 3), "padding": "same", "groups": 4,
                                     "activation": "relu6"}))
    g.add(Layer("b", "conv", ["a"], {"filters": 32, "kernel": (1, 1), "groups": 2, "activation": "swish"}))
    g.add(Layer("c", "conv", ["b"], {"filters": 32, "kernel": (3, 3), "stride": 2, "padding": "same", "groups": 8}))
    g.add(Layer("c_add", "add", ["c", "c"]))
    g.output_names = ["c_add"]
    steps = compile_plan(g, fp32=True)
    assert [s.kind for s in steps] == ["gconv", "gconv", "act", "gconv", "add"]
    assert steps[0].p["relu"] == 2 and steps[0].p["pads"] == ((1, 1), (1, 1))
    assert steps[1].out == "b#preact" and steps[2].p["mode"] == 3 and steps[2].out == "b"
    assert steps[3].p["pads"] == ((0, 1), (0, 1)) and steps[3].covers == ["c"]
    w = init_weights(g, 0)
    x = np.random.default_rng(0).standard_normal((2, 8, 8, 16)).astype(np.float32)
    y = cpu_executor.CpuExecutor(g, w)(x)
    assert _rel(y, ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()) < 1e-4


# run-length encoded step kinds of compile_plan(resnet50, fp32=True) on the parent commit
R50_FP32_KINDS = [("stem_f32", 1), ("conv", 2), ("pair", 1), ("conv", 1), ("pair", 1), ("conv", 41), ("gap", 1),
                  ("dense", 1)]


def test_resnet50_plan_is_unchanged():
    kinds = [s.kind for s in compile_plan(build_model("resnet50"), fp32=True)]
    assert [(k, len(list(v))) for k, v in itertools.groupby(kinds)] == R50_FP32_KINDS


# ------------------------------------------------------------------ MFMA weight packing
@pytest.mark.parametrize("shape", GC.MFMA_SHAPES[:5], ids=str)
def test_mfma_fragment_packing_reproduces_the_conv(shape):
    """The packed A fragments, multiplied the way gconv_f32.hip indexes them (N tile t, tap, 16-channel chunk j,
    lane (fr, fq), k-step s <-> input channel cbase(t) + 16 j + 4 fq + s, output channel 16 t + fr), give the
    grouped convolution."""
    c = GC.case(shape)
    cg = c.Cin // c.G
    assert C.gconv_path(c.Cin, c.Cout, c.G, c.k, c.k) == "mfma"
    frag = C.gconv_fragments_np(c.kern, c.G)
    nj = 2 if cg == 32 else 1
    assert frag.shape == (c.Cout // 16, c.k * c.k, nj, 64, 4)
    dense = np.zeros((c.k * c.k, c.Cin, c.Cout), np.float32)
    for t, j, lane, s in itertools.product(range(c.Cout // 16), range(nj), range(64), range(4)):
        fr, fq = lane & 15, lane >> 4
        cbase = 16 * t if nj == 1 else (16 * t) // 32 * 32
        dense[:, cbase + 16 * j + 4 * fq + s, 16 * t + fr] = frag[t, :, j, lane, s]
    np.testing.assert_array_equal(dense.reshape(c.k, c.k, c.Cin, c.Cout), GC.dense_kernel(c.kern, c.G))


def test_gconv_path_rule():
    assert [C.gconv_path(s[3], s[4], s[5], s[6], s[6]) for s in GC.SHAPES] == \
        ["mfma"] * 6 + ["generic"] * 3 + ["mfma"]
    assert C.gconv_path(64, 64, 32) == "generic" and C.gconv_path(64, 64, 64) == "generic"      # CG 2, 1
    assert C.gconv_path(64, 128, 4) == "generic"                                                # 16 -> 32 per group
    with pytest.raises(ValueError):
        C.gconv_path(30, 32, 4)


# ------------------------------------------------------------------ native CPU op, executors
@pytest.mark.parametrize("shape", GC.SHAPES, ids=str)
def test_cpu_gconv2d_matches_float64_oracle(shape):
    c = GC.case(shape)
    y = np.full(c.out_shape, np.nan, np.float32)
    (pt, _), (pl, _) = c.pads
    cpu_executor.native().gconv2d(c.x, c.kern, c.bias, y, c.stride, pt, pl, c.G, c.act, 0.3)
    assert _rel(y.astype(np.float64), c.want) < 1e-4


@pytest.fixture(scope="module")
def tiny():
    g = build_model("resnext_tiny", input_shape=TINY_SHAPE, classes=10)
    w = init_weights(g, 0)
    x = torch.randn(2, *TINY_SHAPE, generator=torch.Generator().manual_seed(1))
    return g, w, x, ReferenceExecutor(g, w)(x)


def test_cpu_executor_runs_resnext_tiny(tiny):
    g, w, x, want = tiny
    ex = cpu_executor.CpuExecutor(g, w)
    assert [s.kind for s in ex.steps].count("gconv") == 4
    assert _rel(ex(x.numpy()), want.numpy()) < 1e-4
    assert _rel(Model(g, w).predict(x.numpy(), device="cpu"), want.numpy()) < 1e-4


def test_sliced_equals_unsliced_cut_inside_a_block(tiny):
    """Cut at conv3_block1_2_relu: the block input (the shortcut's source) crosses the cut beside it."""
    g, w, x, full = tiny
    parts = slicer.partition(g, ["conv3_block1_2_relu"])
    assert len(parts) == 2 and set(parts[1].inputs) == {"conv3_block1_2_relu", "conv2_block1_out"}
    vals = {g.input_names[0]: x}
    cpu_vals = {g.input_names[0]: x.numpy()}
    for s in parts:
        sg = slicer.subgraph(g, s)
        compile_plan(sg, sg.output_names)
        vals.update(ReferenceExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
        cpu_vals.update(cpu_executor.CpuExecutor(sg, w).run({k: cpu_vals[k] for k in sg.input_names}))
    torch.testing.assert_close(vals[g.output], full, rtol=1e-5, atol=1e-6)
    assert _rel(cpu_vals[g.output], full.numpy()) < 1e-4


def test_defer_serves_resnext_tiny_on_two_cpu_workers(tiny):
    g, w, _, _ = tiny
    m = Model(g, w)
    d = DEFER(membership_port=0, result_port=0, worker_wait=10, ordered=True, batch=2)
    d.membership_server.start()
    nodes = [Node(membership_port=d.membership_port, data_port=0, config_port=0, device="cpu", node_id=f"x{i}",
                  heartbeat_ttl=0.5) for i in range(2)]
    for n in nodes:
        n.run(block=False)
    try:
        inq, outq = queue.Queue(), queue.Queue()
        threading.Thread(target=d.run_defer, args=(m, ["conv3_block1_2_relu"], inq, outq), daemon=True).start()
        xs = [np.random.default_rng(i).standard_normal((2,) + TINY_SHAPE).astype(np.float32) for i in range(3)]
        for x in xs:
            inq.put(x)
        got = np.concatenate([outq.get(timeout=60) for _ in xs])
        np.testing.assert_allclose(got, m.predict(np.concatenate(xs), device="cpu"), rtol=1e-4, atol=1e-6)
    finally:
        d.shutdown(stop_workers=True)
        for n in nodes:
            n.stop()
