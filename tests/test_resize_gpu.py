"""csrc/kernels/resize.hip on the GPU: UpSampling2D (nearest / bilinear) and Cropping2D in fp32 and bf16.

Nearest and crop are bit-exact copies in both precisions.  Bilinear fp32 is held to the project's fp32 bound,
max|got - want| / max(1, max|want|) < 2e-5, against the explicit half-pixel formula in float64; bilinear bf16 to
the bf16 kernel bound of tests/test_kernels_gpu.py, err <= 2e-2 * scale + 1e-2, against the same formula on the
bf16-rounded input.  bf16 rows are padded to 8 channels: the input's padding holds NaN here and the output's
padding must be zero.  Cases: tests/deconv_cases.py.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E

import deconv_cases as DC

pytestmark = pytest.mark.gpu


def _rel1(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


@pytest.mark.parametrize("case", DC.UPSAMPLE_CASES, ids=str)
def test_upsample_f32(case):
    u = DC.upsample_case(case)
    out = torch.full(u.out_shape, float("nan"), dtype=torch.float32, device="cuda")
    E.upsample(torch.from_numpy(u.x).cuda(), out, u.size, u.bilinear)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "an output element was not written (NaN pre-fill)"
    if u.bilinear:
        err = _rel1(got, u.want)
        print(f"bilinear fp32 {case}: rel err {err:.3e}")
        assert err < 2e-5
    else:
        np.testing.assert_array_equal(got, u.want)


@pytest.mark.parametrize("case", DC.UPSAMPLE_CASES, ids=str)
def test_upsample_bf16(case):
    u = DC.upsample_case(case)
    C = u.shape[-1]
    xb, xr = DC.bf16_padded(u.x)
    xb[..., C:] = float("nan")
    out = torch.full(u.out_shape[:3] + (xb.shape[-1],), float("nan"), dtype=torch.bfloat16, device="cuda")
    E.upsample(xb.cuda(), out, u.size, u.bilinear, C=C)
    torch.cuda.synchronize()
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    assert (got[..., C:] == 0).all(), "a padding channel of the output is not zero"
    if u.bilinear:
        want = DC.bilinear_explicit(xr, u.size)
        err, scale = np.abs(got[..., :C] - want).max(), np.abs(want).max() + 1e-6
        print(f"bilinear bf16 {case}: max err {err:.3e} (scale {scale:.3f})")
        assert err <= 2e-2 * scale + 1e-2
    else:
        sh, sw = u.size
        np.testing.assert_array_equal(got[..., :C], np.repeat(np.repeat(xr, sh, axis=1), sw, axis=2))


@pytest.mark.parametrize("case", DC.CROP_CASES, ids=str)
def test_crop_f32_and_bf16_are_exact(case):
    k = DC.crop_case(case)
    (t, _), (l, _) = k.crop
    out = torch.full(k.out_shape, float("nan"), dtype=torch.float32, device="cuda")
    E.crop(torch.from_numpy(k.x).cuda(), out, t, l)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), k.want)
    C = k.shape[-1]
    xb, xr = DC.bf16_padded(k.x)
    xb[..., C:] = float("nan")
    outb = torch.full(k.out_shape[:3] + (xb.shape[-1],), float("nan"), dtype=torch.bfloat16, device="cuda")
    E.crop(xb.cuda(), outb, t, l, C=C)
    torch.cuda.synchronize()
    got = outb.cpu().double().numpy()
    assert (got[..., C:] == 0).all(), "a padding channel of the output is not zero"
    np.testing.assert_array_equal(got[..., :C], xr[:, t:t + k.out_shape[1], l:l + k.out_shape[2]])


def test_wrappers_refuse_bad_shapes_on_the_host():
    x = torch.zeros(1, 4, 4, 8, device="cuda")
    with pytest.raises(ValueError, match="upsample"):
        E.upsample(x, torch.empty(1, 8, 9, 8, device="cuda"), 2)
    with pytest.raises(ValueError, match="crop"):
        E.crop(x, torch.empty(1, 3, 3, 8, device="cuda"), 2, 0)
    with pytest.raises(ValueError, match="bf16"):
        E.upsample(x.to(torch.bfloat16), torch.empty(1, 8, 8, 8, device="cuda", dtype=torch.bfloat16), 2)
