"""Guard-band runs of the transposed convolution (csrc/kernels/deconv_f32.hip) and of upsample / crop
(csrc/kernels/resize.hip), as tests/test_guard_gconv_gpu.py does for the grouped convolution: every buffer a
kernel is given lies between 1 MiB guards (tests/guardband.py).

Each case is launched twice, with NaN and with +inf in the guards of everything the kernel reads, the output
pre-filled with NaN.  Asserted: every guard intact bit for bit; outputs finite, bit-identical between the two
poison runs, and within the kernel's bound of the float64 oracle.  Cases (tests/deconv_cases.py): the MFMA path at
k == s on an odd map with a partial pixel tile, 3x3 stride 2 'same' (halo rows and columns outside the image, a
partial N block), k < s (a phase without taps); the generic path's non-square kernel; the bf16 generic kernel;
and each resize kernel on its odd-shape case (vector and scalar fp32, bf16).
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E

import deconv_cases as DC
import guardband as G

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)
GUARD_CASES = [DC.MFMA_CASES[0], DC.MFMA_CASES[1], DC.MFMA_CASES[5], DC.GENERIC_CASES[1]]


def _rel1(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def _same_finite(outs):
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a.float()).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b.float()).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    return a


@pytest.mark.parametrize("case", GUARD_CASES, ids=str)
def test_guard_deconv_f32(case):
    c = DC.case(case)
    outs = {}
    for poison in POISONS:
        pd = C.pack_deconv_f32(c.kern_io, c.bias, c.stride, c.padding, "cuda")
        assert pd.path == ("mfma" if case in DC.MFMA_CASES else "generic")
        pd.w, pd.bias = G.rehome(pd.w, poison, "pd.w"), G.rehome(pd.bias, poison, "pd.bias")
        x = G.guarded(c.x.shape, torch.float32, "cuda", payload=c.x, poison=poison, name="x")
        out = G.guarded(c.out_shape, torch.float32, "cuda", payload=float("nan"), name="out")
        C.deconv_forward_f32(x, pd, out, relu=c.act)
        torch.cuda.synchronize()
        G.check(x, pd.w, pd.bias, out, what=f"[deconv {case} {pd.path}, {poison} poison]")
        outs[poison] = out.cpu()
    a = _same_finite(outs)
    err = _rel1(a.numpy().astype(np.float64), c.want)
    assert err < 2e-5, f"deconv {case}: rel err {err:.3e}"


def test_guard_deconv_bf16():
    case = DC.GENERIC_CASES[0]                      # 3 -> 5 channels: rows of 8 with 5 and 3 padding channels
    c = DC.case(case)
    xb, xr = DC.bf16_padded(c.x)
    xb[..., c.Cin:] = float("nan")
    want = DC.ref_deconv(xr.astype(np.float32), c.kern, c.bias, c.stride, c.padding, c.act)
    outs = {}
    for poison in POISONS:
        pd = C.pack_deconv_bf16(c.kern_io, c.bias, c.stride, c.padding, "cuda")
        pd.w, pd.bias = G.rehome(pd.w, poison, "pd.w"), G.rehome(pd.bias, poison, "pd.bias")
        x = G.guarded(xb.shape, torch.bfloat16, "cuda", payload=xb, poison=poison, name="x")
        out = G.guarded(c.out_shape[:3] + (8,), torch.bfloat16, "cuda", payload=float("nan"), name="out")
        C.deconv_forward_bf16(x, pd, out, relu=c.act)
        torch.cuda.synchronize()
        G.check(x, pd.w, pd.bias, out, what=f"[deconv bf16 {case}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_finite(outs).double().numpy()
    assert (got[..., c.Cout:] == 0).all()
    err, scale = np.abs(got[..., :c.Cout] - want).max(), np.abs(want).max() + 1e-6
    assert err <= 2e-2 * scale + 1e-2, f"deconv bf16 {case}: max err {err:.3e} (scale {scale:.3f})"


# nearest (2, 3) on 6 channels: the scalar fp32 kernel; bilinear (3, 2) on 5 channels: scalar, clamped taps;
# bilinear 2 on 16 channels: the vector kernel
@pytest.mark.parametrize("case", [DC.UPSAMPLE_CASES[1], DC.UPSAMPLE_CASES[3], DC.UPSAMPLE_CASES[2]], ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_upsample(case, dtype):
    u = DC.upsample_case(case)
    Cc = u.shape[-1]
    xb, xr = DC.bf16_padded(u.x)
    xb[..., Cc:] = float("nan")
    src = torch.from_numpy(u.x) if dtype == torch.float32 else xb
    outs = {}
    for poison in POISONS:
        x = G.guarded(src.shape, dtype, "cuda", payload=src, poison=poison, name="x")
        out = G.guarded(u.out_shape[:3] + (src.shape[-1],), dtype, "cuda", payload=float("nan"), name="out")
        E.upsample(x, out, u.size, u.bilinear, C=Cc)
        torch.cuda.synchronize()
        G.check(x, out, what=f"[upsample {case} {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_finite(outs).double().numpy()
    if dtype == torch.float32:
        want = u.want
        assert (_rel1(got, want) < 2e-5) if u.bilinear else np.array_equal(got, want)
    else:
        sh, sw = u.size
        want = DC.bilinear_explicit(xr, u.size) if u.bilinear else np.repeat(np.repeat(xr, sh, axis=1), sw, axis=2)
        assert (got[..., Cc:] == 0).all()
        err, scale = np.abs(got[..., :Cc] - want).max(), np.abs(want).max() + 1e-6
        assert (err <= 2e-2 * scale + 1e-2) if u.bilinear else err == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_crop(dtype):
    k = DC.crop_case(DC.CROP_CASES[1])              # 5x5x3 -> 2x2x3: the scalar fp32 kernel, 5 padding channels in bf16
    (t, _), (l, _) = k.crop
    Cc = k.shape[-1]
    xb, xr = DC.bf16_padded(k.x)
    xb[..., Cc:] = float("nan")
    src = torch.from_numpy(k.x) if dtype == torch.float32 else xb
    ref = (k.x if dtype == torch.float32 else xr)[:, t:t + k.out_shape[1], l:l + k.out_shape[2]]
    outs = {}
    for poison in POISONS:
        x = G.guarded(src.shape, dtype, "cuda", payload=src, poison=poison, name="x")
        out = G.guarded(k.out_shape[:3] + (src.shape[-1],), dtype, "cuda", payload=float("nan"), name="out")
        E.crop(x, out, t, l, C=Cc)
        torch.cuda.synchronize()
        G.check(x, out, what=f"[crop {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_finite(outs).double().numpy()
    assert np.array_equal(got[..., :Cc], ref) and (got[..., Cc:] == 0).all()
