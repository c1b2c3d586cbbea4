"""csrc/kernels/deconv_f32.hip on the GPU: the transposed-convolution kernel against the float64 CPU oracle and
against the zero-stuffed expansion on the existing fp32 conv kernels, and the bf16 instantiation of its
bounds-checked path.

Metric and bound are tests/test_fp32_gpu.py's: max|got - want| / max(1, max|want|) < 2e-5, the project's fp32-conv
bound (fp32 `F.conv_transpose2d` itself lands at 1.9e-7 .. 2.1e-7 on these inputs).  The bf16 kernel is held to
the bf16 kernel bound of tests/test_kernels_gpu.py, err <= 2e-2 * scale + 1e-2, against the oracle on the
bf16-rounded input.  Cases: tests/deconv_cases.py.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

import deconv_cases as DC

pytestmark = pytest.mark.gpu

BOUND = 2e-5


def _rel1(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def _run(c):
    pd = C.pack_deconv_f32(c.kern_io, c.bias, c.stride, c.padding, "cuda")
    out = torch.full(c.out_shape, float("nan"), dtype=torch.float32, device="cuda")
    C.deconv_forward_f32(torch.from_numpy(c.x).cuda(), pd, out, relu=c.act)
    torch.cuda.synchronize()
    return pd, out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("case", DC.CASES, ids=str)
def test_deconv_f32_matches_float64_oracle(case):
    c = DC.case(case)
    pd, got = _run(c)
    want_path = "mfma" if case in DC.MFMA_CASES else "generic"
    assert C.deconv_path(c.Cin, c.Cout, c.kh, c.kw, c.stride) == want_path and pd.path == want_path
    assert (pd.pad_t, pd.pad_l) == c.pads
    if want_path == "mfma":          # fragment-packed weights: the generic kernel could not have read them
        s = c.stride
        assert tuple(pd.w.shape) == (s * s, c.Cout // 16, -(-c.kh // s) * -(-c.kw // s), c.Cin // 16, 64, 4)
    else:
        assert tuple(pd.w.shape) == (c.kh, c.kw, c.Cin, c.Cout)
    assert np.isfinite(got).all(), "an output element was not written (NaN pre-fill) or is not finite"
    err = _rel1(got, c.want)
    print(f"deconv {case} path {pd.path}: rel err {err:.3e}")
    assert err < BOUND


def test_activation_modes_are_all_used():
    assert {DC.case(c).act for c in DC.MFMA_CASES} == {0, 1, 2}
    assert {DC.case(c).act for c in DC.GENERIC_CASES} == {0, 1, 2}


@pytest.mark.parametrize("case", DC.MFMA_CASES[:3], ids=str)
def test_deconv_f32_agrees_with_the_zero_stuffed_conv(case):
    """k == s, 3x3 stride 2 and 4x4 stride 2 (pb = 1): the same layer as a stride-1 conv of the zero-stuffed,
    padded input with the flipped kernel, on conv_forward_f32."""
    c = DC.case(case)
    _, got = _run(c)
    z, kern = DC.zero_stuffed(c)
    pc = C.pack_conv_f32(kern, c.bias, 1, ((0, 0), (0, 0)), "cuda")
    dense = torch.full(c.out_shape, float("nan"), dtype=torch.float32, device="cuda")
    C.conv_forward_f32(torch.from_numpy(z).cuda(), pc, dense, relu=c.act)
    torch.cuda.synchronize()
    err = _rel1(got, dense.cpu().numpy().astype(np.float64))
    print(f"deconv vs zero-stuffed expansion {case}: rel diff {err:.3e}")
    assert err < BOUND


def test_launcher_rejects_a_path_the_shape_does_not_fit():
    """Weights packed for the generic path are never handed to the MFMA kernel (no silent fall-through either
    way).  The launcher refuses on the host, before any launch."""
    c = DC.case(DC.GENERIC_CASES[1])
    pd = C.pack_deconv_f32(c.kern_io, c.bias, c.stride, c.padding, "cuda")
    assert pd.path == "generic"
    pd.path = "mfma"
    out = torch.empty(c.out_shape, dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="deconv_f32_forward"):
        C.deconv_forward_f32(torch.from_numpy(c.x).cuda(), pd, out)
    # fragment-packed weights labelled generic: the wrapper sees the shape
    m = DC.case(DC.MFMA_CASES[0])
    pm = C.pack_deconv_f32(m.kern_io, m.bias, m.stride, m.padding, "cuda")
    pm.path = "generic"
    with pytest.raises(ValueError, match="generic"):
        C.deconv_forward_f32(torch.from_numpy(m.x).cuda(), pm, torch.empty(m.out_shape, device="cuda"))
    # and bf16-packed weights are refused on fp32 activations by the wrapper
    pb = C.pack_deconv_bf16(c.kern_io, c.bias, c.stride, c.padding, "cuda")
    with pytest.raises(ValueError, match="bf16"):
        C.deconv_forward_f32(torch.from_numpy(c.x).cuda(), pb, out)


@pytest.mark.parametrize("case", [DC.MFMA_CASES[1], DC.GENERIC_CASES[0], DC.GENERIC_CASES[1]], ids=str)
def test_deconv_bf16_generic_kernel(case):
    """bf16 in / out, fp32 weights and accumulate, channels padded to 8: 64 -> 48, 3 -> 5 (8 -> 8 stored) and
    20 -> 24 (24 -> 24 stored).  The padding channels of x hold NaN and must not reach a real channel; those of
    the output must come out as zeros."""
    c = DC.case(case)
    xb, xr = DC.bf16_padded(c.x)
    xb[..., c.Cin:] = float("nan")
    want = DC.ref_deconv(xr.astype(np.float32), c.kern, c.bias, c.stride, c.padding, c.act)
    cop = -(-c.Cout // 8) * 8
    pd = C.pack_deconv_bf16(c.kern_io, c.bias, c.stride, c.padding, "cuda")
    out = torch.full(c.out_shape[:3] + (cop,), float("nan"), dtype=torch.bfloat16, device="cuda")
    C.deconv_forward_bf16(xb.cuda(), pd, out, relu=c.act)
    torch.cuda.synchronize()
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    assert (got[..., c.Cout:] == 0).all(), "a padding channel of the output is not zero"
    err, scale = np.abs(got[..., :c.Cout] - want).max(), np.abs(want).max() + 1e-6
    print(f"deconv bf16 {case}: max err {err:.3e} (scale {scale:.3f})")
    assert err <= 2e-2 * scale + 1e-2
