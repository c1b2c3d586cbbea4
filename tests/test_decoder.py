"""Conv2DTranspose, UpSampling2D, Cropping2D and U-Net, the parts that need no GPU: IR, Keras JSON, the PyTorch
oracle, the launch plan, weight packing, the native CPU ops, slicing and DEFER serving.

Cases and the float64 oracles: tests/deconv_cases.py.  The HIP kernels: tests/test_deconv_gpu.py,
tests/test_resize_gpu.py, tests/test_guard_deconv_gpu.py, tests/test_unet_gpu.py.

The fp32 bound of the native CPU ops is the project's fp32-conv one (tests/test_fp32_gpu.py):
max|got - want| / max(1, max|want|) < 2e-5; nearest and crop are exact.
"""
import json
import queue
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.dispatcher import DEFER
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import planner, slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.keras_json import (
    from_keras_json, to_keras_json)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    build_model, build_unet)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.node import Node
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

import deconv_cases as DC

BOUND = 2e-5


def _rel1(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


# ------------------------------------------------------------------ IR
def _decoder_graph():
    g = Graph("dec")
    g.add(Layer("in", "input", [], {"shape": (5, 6, 8)}))
    g.add(Layer("up", "deconv", ["in"], {"filters": 12, "kernel": (3, 2), "stride": 2, "padding": "valid",
                                         "use_bias": True, "activation": "relu"}))
    g.add(Layer("us", "upsample", ["up"], {"size": (2, 3), "interpolation": "bilinear"}))
    g.add(Layer("cr", "crop", ["us"], {"crop": ((1, 2), (0, 3))}))
    g.output_names = ["cr"]
    return g


def test_shapes_weight_specs_and_macs_of_the_new_ops():
    g = _decoder_graph()
    # valid: in * s + max(k - s, 0) -> (5*2 + 1, 6*2 + 0); upsample x(2, 3); crop
    assert [g.layers[n].out_shape for n in g.order] == [(5, 6, 8), (11, 12, 12), (22, 36, 12), (19, 33, 12)]
    assert g.weight_specs() == [("up/kernel", (3, 2, 12, 8)), ("up/bias", (12,))]          # Keras HWOI
    assert g.layer_macs("up") == 5 * 6 * 3 * 2 * 8 * 12 and g.layer_macs("us") == 0 and g.layer_macs("cr") == 0
    assert g.count_params() == 3 * 2 * 12 * 8 + 12
    h = Graph("h")
    h.add(Layer("in", "input", [], {"shape": (4, 7, 3)}))
    h.add(Layer("a", "deconv", ["in"], {"filters": 5, "kernel": (4, 4), "stride": 2, "padding": "same",
                                        "use_bias": False}))
    h.add(Layer("b", "deconv", ["a"], {"filters": 2, "kernel": (2, 2), "stride": 3, "padding": "valid"}))
    assert h.layers["a"].out_shape == (8, 14, 5) and h.layers["b"].out_shape == (24, 42, 2)
    assert h.weight_specs() == [("a/kernel", (4, 4, 5, 3)), ("b/kernel", (2, 2, 2, 5)), ("b/bias", (2,))]
    w = init_weights(g, 0)
    assert w["up/kernel"].shape == (3, 2, 12, 8) and abs(w["up/kernel"].std() - np.sqrt(2 / (3 * 2 * 8))) < 0.05
    costs = planner.layer_costs(g, batch=2)
    assert costs["up"] > 0 and costs["us"] > 0 and costs["cr"] > 0
    # the JSON form of the IR keeps size / crop as tuples
    g2 = Graph.from_json(g.to_json())
    assert g2.layers["us"].attrs["size"] == (2, 3) and g2.layers["cr"].attrs["crop"] == ((1, 2), (0, 3))
    assert g2.layers["up"].attrs["kernel"] == (3, 2)


def test_an_empty_crop_and_a_bad_upsample_raise_at_add():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (4, 4, 2)}))
    with pytest.raises(ValueError, match="crop 'c'"):
        g.add(Layer("c", "crop", ["in"], {"crop": ((2, 2), (0, 0))}))
    with pytest.raises(ValueError, match="crop 'c'"):
        g.add(Layer("c", "crop", ["in"], {"crop": ((0, 0), (1, 3))}))
    with pytest.raises(ValueError, match="upsample 'u'"):
        g.add(Layer("u", "upsample", ["in"], {"size": (2, 0), "interpolation": "nearest"}))
    with pytest.raises(ValueError, match="upsample 'u'"):
        g.add(Layer("u", "upsample", ["in"], {"size": (2, 2), "interpolation": "bicubic"}))
    g.add(Layer("c", "crop", ["in"], {"crop": ((1, 2), (0, 3))}))
    assert g.layers["c"].out_shape == (1, 1, 2)


# ------------------------------------------------------------------ Keras JSON
def _k2(cls, name, inbound, **cfg):
    return {"class_name": cls, "name": name, "config": dict(cfg, name=name),
            "inbound_nodes": [[[i, 0, 0, {}] for i in inbound]] if inbound else []}


def _k3(cls, name, inbound, **cfg):
    args = [{"class_name": "__keras_tensor__", "config": {"shape": [None], "dtype": "float32",
                                                         "keras_history": [i, 0, 0]}} for i in inbound]
    return {"module": "keras.layers", "class_name": cls, "name": name, "config": dict(cfg, name=name),
            "inbound_nodes": [{"args": args, "kwargs": {}}] if inbound else []}


def _keras_encoder_decoder(L, keras3=False, **override):
    """Conv2D stride 2 -> Conv2DTranspose -> UpSampling2D -> Cropping2D -> Concatenate with the input."""
    shape = {"batch_shape": [None, 8, 8, 4]} if keras3 else {"batch_input_shape": [None, 8, 8, 4]}
    up = dict(filters=6, kernel_size=[3, 3], strides=[2, 2], padding="same", data_format="channels_last",
              dilation_rate=[1, 1], output_padding=None, activation="relu", use_bias=True)
    us = dict(size=[2, 2], data_format="channels_last", interpolation="bilinear")
    up.update(override.get("up", {}))
    us.update(override.get("us", {}))
    layers = [
        L("InputLayer", "in", [], dtype="float32", **shape),
        L("Conv2D", "down", ["in"], filters=8, kernel_size=[3, 3], strides=[2, 2], padding="same",
          data_format="channels_last", dilation_rate=[1, 1], groups=1, activation="relu", use_bias=True),
        L("Conv2DTranspose", "up", ["down"], **up),
        L("UpSampling2D", "us", ["up"], **us),
        L("Cropping2D", "cr", ["us"], cropping=[[4, 4], [3, 5]], data_format="channels_last"),
        L("Concatenate", "cat", ["in", "cr"], axis=-1),
    ]
    return json.dumps({"class_name": "Functional", "config": {"name": "encdec", "layers": layers,
                                                              "input_layers": [["in", 0, 0]],
                                                              "output_layers": [["cat", 0, 0]]}})


@pytest.mark.parametrize("L,keras3", [(_k2, False), (_k3, True)], ids=["keras2", "keras3"])
def test_keras_json_imports_the_three_classes(L, keras3):
    g = from_keras_json(_keras_encoder_decoder(L, keras3))
    assert [g.layers[n].op for n in g.order] == ["input", "conv", "deconv", "upsample", "crop", "concat"]
    assert g.layers["up"].attrs == {"filters": 6, "kernel": (3, 3), "stride": 2, "padding": "same", "use_bias": True,
                                    "activation": "relu"}
    assert g.layers["us"].attrs == {"size": (2, 2), "interpolation": "bilinear"}
    assert g.layers["cr"].attrs == {"crop": ((4, 4), (3, 5))}
    assert [g.layers[n].out_shape for n in g.order] == [(8, 8, 4), (4, 4, 8), (8, 8, 6), (16, 16, 6), (8, 8, 6),
                                                        (8, 8, 10)]
    assert g.weight_specs()[2:] == [("up/kernel", (3, 3, 6, 8)), ("up/bias", (6,))]
    # round trip through our writer (Keras 2 layout) and through the IR's own JSON
    s = to_keras_json(g)
    classes = {ld["name"]: ld["class_name"] for ld in json.loads(s)["config"]["layers"]}
    assert (classes["up"], classes["us"], classes["cr"]) == ("Conv2DTranspose", "UpSampling2D", "Cropping2D")
    assert json.loads(from_keras_json(s).to_json()) == json.loads(g.to_json())
    # get_weights() order and the CPU path
    m = Model.from_keras_json(_keras_encoder_decoder(L, keras3), seed=3)
    x = np.random.default_rng(0).standard_normal((2, 8, 8, 4)).astype(np.float32)
    want = ReferenceExecutor(m.graph, m.weights)(torch.from_numpy(x)).numpy()
    assert _rel1(m.predict(x, device="cpu"), want) < BOUND


@pytest.mark.parametrize("override,match", [
    ({"up": {"output_padding": [1, 1]}}, r"up.*output_padding"),
    ({"up": {"dilation_rate": [2, 2]}}, r"up.*dilat"),
    ({"up": {"strides": [2, 1]}}, r"up.*strides"),
    ({"us": {"interpolation": "bicubic"}}, r"us.*bicubic"),
    ({"us": {"interpolation": "lanczos3"}}, r"us.*lanczos3"),
])
def test_keras_json_rejections_name_the_layer(override, match):
    with pytest.raises(NotImplementedError, match=match):
        from_keras_json(_keras_encoder_decoder(_k2, **override))


# ------------------------------------------------------------------ oracle
@pytest.mark.parametrize("k,s,n", [(2, 2, 5), (3, 2, 5), (4, 2, 3), (3, 1, 4), (1, 2, 3), (5, 3, 4), (2, 3, 3)])
def test_deconv_oracle_is_the_vjp_of_a_same_strided_conv(k, s, n):
    """Keras defines Conv2DTranspose('same') as the gradient of a stride-s 'same' Conv2D from size n*s with
    respect to its input.  In float64 the oracle equals that vector-Jacobian product to 0.0."""
    rng = np.random.default_rng(k * 100 + s * 10 + n)
    cin, cout = 3, 2                      # of the transposed conv: it maps cin -> cout
    # small integers: every product and sum is exact in float64 (and in the fp32 arrays the executor keeps its
    # weights in), so the two sides agree to 0.0 whatever order either sums its taps and channels in
    x = rng.integers(-8, 9, (2, n, n, cin)).astype(np.float64)
    kern = rng.integers(-8, 9, (k, k, cout, cin)).astype(np.float64)        # Keras HWOI = the forward conv's HWIO
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (n, n, cin)}))
    g.add(Layer("up", "deconv", ["in"], {"filters": cout, "kernel": (k, k), "stride": s, "padding": "same",
                                         "use_bias": False}))
    g.output_names = ["up"]
    got = ReferenceExecutor(g, {"up/kernel": kern}, dtype=torch.float64)(torch.from_numpy(x))
    assert got.shape == (2, n * s, n * s, cout)
    # forward conv: (n*s, n*s, cout) -> (n, n, cin), TF 'same' pads, kernel HWIO = (k, k, cout, cin)
    size = n * s
    total = max((n - 1) * s + k - size, 0)
    lo, hi = total // 2, total - total // 2
    z = torch.zeros(2, cout, size, size, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(z, (lo, hi, lo, hi)), torch.from_numpy(kern).permute(3, 2, 0, 1), stride=s)
    assert y.shape == (2, cin, n, n)
    (vjp,) = torch.autograd.grad(y, z, torch.from_numpy(x).permute(0, 3, 1, 2))
    assert float((got - vjp.permute(0, 2, 3, 1)).abs().max()) == 0.0
    # and the shared float64 oracle of the kernel tests is the same function
    want = DC.ref_deconv(x.astype(np.float32), kern.astype(np.float32), np.zeros(cout, np.float32), s, "same", 0)
    got32 = ReferenceExecutor(g, {"up/kernel": kern.astype(np.float32)}, dtype=torch.float64)(
        torch.from_numpy(x.astype(np.float32)))
    assert float(np.abs(got32.numpy() - want).max()) == 0.0


@pytest.mark.parametrize("c", [u for u in DC.UPSAMPLE_CASES if u[1] == "bilinear"], ids=str)
def test_bilinear_oracle_matches_the_explicit_formula(c):
    u = DC.upsample_case(c)
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": u.shape[1:]}))
    g.add(Layer("us", "upsample", ["in"], {"size": u.size, "interpolation": "bilinear"}))
    g.output_names = ["us"]
    got = ReferenceExecutor(g, {}, dtype=torch.float64)(torch.from_numpy(u.x)).numpy()
    err = np.abs(got - u.want).max()
    print(f"bilinear oracle {c}: max err against the explicit formula {err:.3e}")
    assert got.shape == u.out_shape and err < 1e-14


def test_zero_stuffed_expansion_is_the_same_layer():
    """The expansion the GPU tests and tools/deconv_bench.py run on conv_forward_f32, checked here in float64."""
    for c in DC.MFMA_CASES[:3]:
        k = DC.case(c)
        z, kern = DC.zero_stuffed(k)
        y = F.conv2d(torch.from_numpy(z).double().permute(0, 3, 1, 2), torch.from_numpy(kern).double().permute(3, 2, 0, 1),
                     torch.from_numpy(k.bias).double()).permute(0, 2, 3, 1)
        y = y.clamp_min(0) if k.act == 1 else y.clamp(0, 6) if k.act == 2 else y
        assert y.shape == k.out_shape and float(np.abs(y.numpy() - k.want).max()) < 1e-12


# ------------------------------------------------------------------ weight packing
def test_deconv_path_and_fragment_packing():
    for c in DC.CASES:
        k = DC.case(c)
        assert C.deconv_path(k.Cin, k.Cout, k.kh, k.kw, k.stride) == ("mfma" if c in DC.MFMA_CASES else "generic")
    assert C.deconv_path(1024, 512, 2, 2, 2) == "mfma" and C.deconv_path(128, 64, 2, 2, 2) == "mfma"
    assert C.deconv_path(16, 8, 2, 2, 2) == "generic" and C.deconv_path(24, 16, 2, 2, 2) == "generic"
    with pytest.raises(ValueError):
        C.deconv_path(16, 16, 2, 2, 0)
    k = DC.case(DC.MFMA_CASES[1])                                   # 3x3 stride 2, 64 -> 48
    f = C.deconv_fragments_np(k.kern_io, 2)
    assert f.shape == (4, 3, 4, 4, 64, 4)
    # phase (1, 0), N tile 2, slot (0, 1) = tap (1, 2), chunk 3, lane (fq 2, o 5), k-step 3 -> cin 59, cout 37
    assert f[2, 2, 1, 3, 2 * 16 + 5, 3] == k.kern_io[1, 2, 48 + 11, 37]
    # slots past the kernel stay zero: phase (1, 1) has the one tap (1, 1), phase (0, 1) the taps (0, 1) and (2, 1)
    assert not f[3, :, 1:].any() and not f[1, :, [1, 3]].any() and f[1, :, 0].any() and f[1, :, 2].any()
    assert np.count_nonzero(f) == np.count_nonzero(k.kern_io)


# ------------------------------------------------------------------ native CPU ops
@pytest.mark.parametrize("c", DC.CASES, ids=str)
def test_cpu_deconv2d_matches_float64_oracle(c):
    k = DC.case(c)
    y = np.full(k.out_shape, np.nan, np.float32)
    cpu_executor.native().deconv2d(k.x, k.kern_io, k.bias, y, k.stride, k.pads[0], k.pads[1], k.act, 0.3)
    err = _rel1(y.astype(np.float64), k.want)
    print(f"cpu deconv {c}: rel err {err:.3e}")
    assert np.isfinite(y).all() and err < BOUND


@pytest.mark.parametrize("c", DC.UPSAMPLE_CASES, ids=str)
def test_cpu_upsample2d_matches_oracle(c):
    u = DC.upsample_case(c)
    y = np.full(u.out_shape, np.nan, np.float32)
    cpu_executor.native().upsample2d(u.x, y, u.size[0], u.size[1], u.bilinear)
    if u.bilinear:
        assert np.isfinite(y).all() and _rel1(y.astype(np.float64), u.want) < BOUND
    else:
        np.testing.assert_array_equal(y.astype(np.float64), u.want)


@pytest.mark.parametrize("c", DC.CROP_CASES, ids=str)
def test_cpu_crop2d_is_exact(c):
    k = DC.crop_case(c)
    y = np.full(k.out_shape, np.nan, np.float32)
    cpu_executor.native().crop2d(k.x, y, k.crop[0][0], k.crop[1][0])
    np.testing.assert_array_equal(y, k.want)


def test_cpu_ops_refuse_mismatched_outputs():
    m = cpu_executor.native()
    k = DC.case(DC.GENERIC_CASES[0])
    with pytest.raises(ValueError, match="deconv2d"):
        m.deconv2d(k.x, k.kern_io, k.bias, np.empty(k.out_shape[:3] + (k.Cout + 1,), np.float32), k.stride, 0, 0, 0, 0.3)
    with pytest.raises(ValueError, match="upsample2d"):
        m.upsample2d(np.zeros((1, 2, 2, 3), np.float32), np.empty((1, 4, 5, 3), np.float32), 2, 2, False)
    with pytest.raises(ValueError, match="crop2d"):
        m.crop2d(np.zeros((1, 4, 4, 3), np.float32), np.empty((1, 3, 3, 3), np.float32), 2, 0)


def test_cpu_executor_runs_the_decoder_graph_with_bn_folded():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (5, 6, 8)}))
    g.add(Layer("up", "deconv", ["in"], {"filters": 12, "kernel": (3, 3), "stride": 2, "padding": "same",
                                         "use_bias": True}))
    g.add(Layer("bn", "bn", ["up"], {"epsilon": 1e-3}))
    g.add(Layer("act", "relu", ["bn"], {"max_value": 6.0}))
    g.add(Layer("up2", "deconv", ["act"], {"filters": 4, "kernel": (2, 2), "stride": 2, "padding": "valid",
                                           "use_bias": False, "activation": "sigmoid"}))
    g.add(Layer("us", "upsample", ["up2"], {"size": (1, 2), "interpolation": "nearest"}))
    g.add(Layer("cr", "crop", ["us"], {"crop": ((0, 1), (2, 0))}))
    g.output_names = ["cr"]
    w = init_weights(g, 5)
    for fp32, fusions in ((True, True), (True, False), (False, True)):
        st = [s for s in compile_plan(g, fp32=fp32, device_fusions=fusions) if s.kind != "pack"]
        assert [s.kind for s in st] == ["deconv", "deconv", "act", "upsample", "crop"]
        assert st[0].covers == ["up", "bn", "act"] and st[0].out == "act"
        assert st[0].p == {"conv": "up", "deconv": True, "bn": "bn", "relu": 2, "stride": 2, "kernel": (3, 3),
                           "filters": 12, "pads": (0, 0)}
        assert st[1].p["relu"] == 0 and st[1].out == "up2#preact" and st[2].p["mode"] == 4 and st[2].out == "up2"
        assert st[3].p == {"size": (1, 2), "bilinear": False} and st[4].p == {"crop": ((0, 1), (2, 0))}
    x = np.random.default_rng(1).standard_normal((2, 5, 6, 8)).astype(np.float32)
    want = ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()
    assert _rel1(cpu_executor.CpuExecutor(g, w)(x), want) < BOUND


def test_a_4x4_same_deconv_starts_one_into_the_frame():
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (4, 5, 16)}))
    g.add(Layer("up", "deconv", ["in"], {"filters": 32, "kernel": (4, 4), "stride": 2, "padding": "same"}))
    (st,) = compile_plan(g, fp32=True)
    assert st.kind == "deconv" and st.p["pads"] == (1, 1) and st.p["relu"] == 0


# ------------------------------------------------------------------ zoo
@pytest.mark.parametrize("name,kw,params", [("unet", {}, 31_031_745), ("unet", {"input_shape": (256, 256, 1)}, 31_030_593),
                                            ("unet_bilinear", {}, 31_031_745), ("unet_tiny", {}, 117_041)])
def test_unet_parameter_totals(name, kw, params):
    g = build_model(name, **kw)
    assert g.count_params() == params
    assert g.layers[g.output].out_shape == tuple(g.layers[g.input].out_shape[:2]) + (1,)


def test_unet_structure():
    g = build_model("unet")
    assert g.layers[g.input].out_shape == (256, 256, 3)
    ups = [n for n in g.order if g.layers[n].op == "deconv"]
    assert ups == ["dec4_up", "dec3_up", "dec2_up", "dec1_up"]
    assert [(g.in_shapes(n)[0], g.layers[n].out_shape) for n in ups] == [
        ((16, 16, 1024), (32, 32, 512)), ((32, 32, 512), (64, 64, 256)), ((64, 64, 256), (128, 128, 128)),
        ((128, 128, 128), (256, 256, 64))]
    assert g.layers["dec4_concat"].inputs == ["enc4_conv2", "dec4_up"] and g.layers["dec4_concat"].out_shape[-1] == 1024
    assert g.layers["head"].attrs["activation"] == "sigmoid" and g.layers["head"].attrs["kernel"] == (1, 1)
    b = build_model("unet_bilinear")
    assert not any(L.op == "deconv" for L in b.layers.values())
    assert [b.layers[n].attrs["interpolation"] for n in b.order if b.layers[n].op == "upsample"] == ["bilinear"] * 4
    assert b.layers["dec4_up"].op == "conv" and b.layers["dec4_up"].attrs["kernel"] == (2, 2)
    t = build_unet("unet_tiny", up="nearest", classes=3, input_shape=(16, 24, 1))
    assert t.layers[t.output].out_shape == (16, 24, 3)
    with pytest.raises(ValueError, match="multiple of 4"):
        build_model("unet_tiny", input_shape=(30, 32, 3))


@pytest.fixture(scope="module")
def tiny():
    g = build_model("unet_tiny")
    w = init_weights(g, 0)
    x = torch.randn(2, 32, 32, 3, generator=torch.Generator().manual_seed(1))
    return g, w, x, ReferenceExecutor(g, w)(x)


@pytest.mark.parametrize("fp32,device_fusions", [(True, True), (True, False), (False, True)])
def test_unet_tiny_plan_step_kinds(fp32, device_fusions):
    g = build_model("unet_tiny")
    steps = [s for s in compile_plan(g, fp32=fp32, device_fusions=device_fusions) if s.kind != "pack"]
    assert [s.kind for s in steps] == (["conv", "conv", "maxpool"] * 2 + ["conv", "conv"]
                                       + ["deconv", "concat", "conv", "conv"] * 2 + ["conv", "act"])
    dec = [s for s in steps if s.kind == "deconv"]
    assert [s.p["conv"] for s in dec] == ["dec2_up", "dec1_up"]
    assert all(s.p["relu"] == 0 and s.p["pads"] == (0, 0) and s.p["kernel"] == (2, 2) and s.p["stride"] == 2
               for s in dec)
    # a Conv2DTranspose(activation='relu') folds the ReLU into the step
    g.layers["dec2_up"].attrs["activation"] = "relu"
    dec = [s for s in compile_plan(g, fp32=fp32, device_fusions=device_fusions) if s.kind == "deconv"]
    assert [s.p["relu"] for s in dec] == [1, 0]


def test_model_predict_cpu_on_unet_tiny_from_keras_json(tiny):
    g, w, x, want = tiny
    m = Model.from_keras_json(to_keras_json(g), weights=[w[n] for n, _ in g.weight_specs()])
    got = m.predict(x.numpy(), device="cpu")
    assert got.shape == (2, 32, 32, 1) and got.min() > 0.0 and got.max() < 1.0
    assert _rel1(got, want.numpy()) < BOUND
    gb = build_unet("unet_tiny", up="bilinear")
    wb = init_weights(gb, 0)
    assert _rel1(Model(gb, wb).predict(x.numpy(), device="cpu"), ReferenceExecutor(gb, wb)(x).numpy()) < BOUND


def test_plan_cuts_and_sliced_equals_unsliced(tiny):
    """Three stages: two cuts, each with a skip connection in flight beside the cut tensor."""
    g, w, x, full = tiny
    cuts, _ = planner.plan_cuts(g, 3, batch=2, precision="fp32", calibrated=False)
    assert len(cuts) == 2
    parts = slicer.partition(g, cuts)
    assert len(parts) == 3 and any(len(p.inputs) > 1 for p in parts[1:])
    vals = {g.input_names[0]: x}
    cpu_vals = {g.input_names[0]: x.numpy()}
    for s in parts:
        sg = slicer.subgraph(g, s)
        compile_plan(sg, sg.output_names)
        vals.update(ReferenceExecutor(sg, w).run({k: vals[k] for k in sg.input_names}))
        cpu_vals.update(cpu_executor.CpuExecutor(sg, w).run({k: cpu_vals[k] for k in sg.input_names}))
    torch.testing.assert_close(vals[g.output], full, rtol=1e-5, atol=1e-6)
    assert _rel1(cpu_vals[g.output], full.numpy()) < BOUND
    # a cut right after a transposed conv: the skip crosses beside it
    parts = slicer.partition(g, ["dec2_up"])
    assert set(parts[1].inputs) == {"dec2_up", "enc2_conv2", "enc1_conv2"}


def test_defer_serves_unet_tiny_on_two_cpu_workers(tiny):
    g, w, _, _ = tiny
    m = Model(g, w)
    d = DEFER(membership_port=0, result_port=0, worker_wait=10, ordered=True, batch=2)
    d.membership_server.start()
    nodes = [Node(membership_port=d.membership_port, data_port=0, config_port=0, device="cpu", node_id=f"u{i}",
                  heartbeat_ttl=0.5) for i in range(2)]
    for n in nodes:
        n.run(block=False)
    try:
        inq, outq = queue.Queue(), queue.Queue()
        threading.Thread(target=d.run_defer, args=(m, ["dec2_up"], inq, outq), daemon=True).start()
        xs = [np.random.default_rng(i).standard_normal((2, 32, 32, 3)).astype(np.float32) for i in range(3)]
        for x in xs:
            inq.put(x)
        got = np.concatenate([outq.get(timeout=60) for _ in xs])
        np.testing.assert_allclose(got, m.predict(np.concatenate(xs), device="cpu"), rtol=1e-4, atol=1e-6)
    finally:
        d.shutdown(stop_workers=True)
        for n in nodes:
            n.stop()
