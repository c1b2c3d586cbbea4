"""The three attention entry points run one scheme (csrc/kernels/attention_core.h; cross_attention.hip and
window_attention.hip in kernels of their own): where two of them are handed the same rows they give the same bits,
in fp32 and in bf16, on the MFMA and on the plain kernel.

* `attention` on a [Q | K | V] buffer against `cross_attention` on the three column slices of that buffer;
* `window_attention` with H = W = M, no shift and an all-zero bias table against `attention` with T = M^2 on the
  same rows (token t of the only window is map row t, and a score accumulator that starts from a loaded 0.0 is the
  one that starts from 0.0).

Inputs are N(0, 1) with a fixed seed, in rows with 8 surplus columns of NaN (never read); the outputs are
pre-filled with NaN and have 8 padding channels, which both sides write as zeros, so the whole tensors compare.
Each output is also held to the float64 oracle and the allowance of tests/attention_cases.py (bf16: the input
rounded to bf16, 2^-8 |want| + allowance), so that two equally wrong outputs cannot pass.
"""
import functools

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import attention_cases as AC

pytestmark = pytest.mark.gpu

# (B, T, heads, d, dv), path.  100 tokens: two query tiles, the second partly empty, four key tiles with a tail,
# d != dv in the 64-wide registers; 37 tokens of 24: the plain kernel
SELF_CROSS = [((2, 100, 2, 32, 48), "mfma"), ((2, 37, 3, 24, 24), "plain")]
# (B, M, heads, d), path.  49 tokens: two key tiles with a tail, one query tile in which one wave holds no query;
# 81 tokens: two query tiles, three key tiles
WINDOW_SELF = [((2, 7, 2, 32), "mfma"), ((2, 7, 2, 24), "plain"), ((1, 9, 1, 16), "mfma")]
DTYPES = [torch.float32, torch.bfloat16]
PAD = 8     # surplus columns of the input rows and padding channels of the output rows: slices stay 4-element aligned


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """The [Q | K | V] rows (a CPU tensor of `dtype` with NaN in the surplus columns), the oracle on the values
    the kernels see, and the allowance."""
    B, T, h, d, dv = shape
    w = h * (2 * d + dv)
    vals = torch.randn((B * T, w), generator=torch.Generator().manual_seed(16)).to(dtype)
    qkv = torch.full((B * T, w + PAD), float("nan"), dtype=dtype)
    qkv[:, :w] = vals
    seen = vals.float().numpy()
    want = AC.ref_attention(seen, B, T, h, d, dv)
    _, allow = AC.f32_allowance(seen, shape + (None,), want)
    return qkv, want, allow


def _check_oracle(out, shape, dtype, what):
    _, want, allow = _inputs(shape, dtype)
    w_out = shape[2] * shape[4]
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[:, w_out:] == 0).all(), "padding channels must come out as exact zeros"
    err = np.abs(got[:, :w_out] - want)
    bound = allow + (2.0 ** -8 * np.abs(want) if dtype == torch.bfloat16 else 0.0)
    print(f"{what} {shape} {dtype}: max err {err.max():.3e}, allowance {allow:.3e}, worst excess {(err - bound).max():.3e}")
    assert (err <= bound).all()


def _empty_out(shape, dtype):
    B, T, h, _, dv = shape
    return torch.full((B * T, h * dv + PAD), float("nan"), dtype=dtype, device="cuda")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("shape,path", SELF_CROSS, ids=str)
def test_attention_equals_cross_attention_on_its_column_slices(shape, path, dtype):
    B, T, h, d, dv = shape
    qkv = _inputs(shape, dtype)[0].cuda()
    q, k, v = qkv[:, :h * d], qkv[:, h * d:2 * h * d], qkv[:, 2 * h * d:2 * h * d + h * dv]
    one, three = _empty_out(shape, dtype), _empty_out(shape, dtype)
    assert A.attention_path(d, dv) == path and A.cross_attention_path(q, k, v, three, d, dv) == path
    A.attention(qkv, one, B, T, h, d, dv)
    A.cross_attention(q, k, v, three, B, T, T, h, d, dv)
    torch.cuda.synchronize()
    _check_oracle(one, shape, dtype, "attention")
    assert torch.equal(one, three)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case,path", WINDOW_SELF, ids=str)
def test_one_unshifted_window_without_bias_equals_attention(case, path, dtype):
    B, M, h, d = case
    shape = (B, M * M, h, d, d)
    qkv = _inputs(shape, dtype)[0].cuda()
    bias = A.window_bias(np.zeros(((2 * M - 1) ** 2, h), np.float32), M, 0, device="cuda")
    assert not bias.any()
    win, one = _empty_out(shape, dtype), _empty_out(shape, dtype)
    assert A.window_attention_path(d) == path and A.attention_path(d, d) == path
    A.window_attention(qkv, bias, win, B, M, M, M, 0, h, d)
    A.attention(qkv, one, B, M * M, h, d, d)
    torch.cuda.synchronize()
    _check_oracle(win, shape, dtype, "window_attention")
    assert torch.equal(win, one)
