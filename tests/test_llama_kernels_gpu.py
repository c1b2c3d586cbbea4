"""The three Llama kernels on the GPU against the float64 oracles of tests/llama_cases.py, fp32 and bf16: rmsnorm
(csrc/kernels/layernorm.hip), the rope step (csrc/kernels/layers.hip) and the grouped-query instantiations of the
attention core (csrc/kernels/attention.hip).  The same cases as on the native CPU ops (tests/test_llama.py), the
allowance of the case module, every output pre-filled with NaN.

Beyond the allowance, the exact checks: rope's V columns are copies bit for bit, its padding and rmsnorm's are
zeros, position 0 is the identity bit for bit in fp32; a grouped-query launch equals, bit for bit, the existing
launch on rows in which each K / V head stands g times (the same template, the same arithmetic per (image, head)),
in both precisions, on the MFMA and the plain path, causal and not; and `kv_heads` equal to `heads`, or None, is
the launch as it was.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E

import llama_cases as LC

pytestmark = pytest.mark.gpu

QT, KT = A.attention_tiles()
GQA_CASES = LC.gqa_cases(QT, KT)


def _pad8(n):
    return (n + 7) // 8 * 8


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


# --------------------------------------------------------------------- rmsnorm
@pytest.mark.parametrize("c", LC.RMSNORM_CASES, ids=str)
def test_rmsnorm_f32(c):
    rows, C, eps, scale, probe = c
    x, sc = LC.rmsnorm_inputs(c)
    want = LC.rmsnorm_oracle(x, sc, eps)
    e_ref = float(np.abs(LC.rmsnorm_library(x, sc, eps) - want).max())
    out = torch.full((rows, C), float("nan"), device="cuda")
    E.rmsnorm_f32(_dev(x), _dev(sc if scale else np.ones(C, np.float32)), out, eps)
    torch.cuda.synchronize()
    err, allow = float(np.abs(out.double().cpu().numpy() - want).max()), LC.allowance(want, e_ref)
    print(f"rmsnorm_f32 {c}: e_ref {e_ref:.3e} err {err:.3e} allowance {allow:.3e}")
    assert err <= allow


@pytest.mark.parametrize("c", LC.RMSNORM_CASES, ids=str)
def test_rmsnorm_bf16(c):
    rows, C, eps, scale, probe = c
    x, sc = LC.rmsnorm_inputs(c, bf16=True)
    want = LC.rmsnorm_oracle(x, sc, eps)
    e_ref = float(np.abs(LC.rmsnorm_library(x, sc, eps) - want).max())
    Cp = _pad8(C)
    xp = torch.full((rows, Cp), float("nan"), dtype=torch.bfloat16)              # the pads hold NaN
    xp[:, :C] = torch.from_numpy(x).to(torch.bfloat16)
    scp = np.zeros(Cp, np.float32)
    scp[:C] = sc if scale else 1.0
    out = torch.full((rows, Cp), float("nan"), dtype=torch.bfloat16, device="cuda")
    E.rmsnorm(xp.cuda(), _dev(scp), out, C, eps)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().astype(np.float64)
    assert (got[:, C:] == 0).all(), "padding channels must come out as exact zeros"
    err = np.abs(got[:, :C] - want)
    allow = LC.allowance(want, e_ref, bf16=True)
    print(f"rmsnorm_bf16 {c}: e_ref {e_ref:.3e} err {err.max():.3e} allowance {np.max(allow):.3e}")
    assert (err <= allow).all()


# ------------------------------------------------------------------------ rope
@pytest.mark.parametrize("c", LC.ROPE_CASES, ids=str)
def test_rope_f32(c):
    B, T, hq, hkv, d, dv, W = c
    x = LC.rope_inputs(c)
    table = A.rope_table(T, d, W)
    wd, rotw = LC.rope_width(c), (hq + hkv) * d
    want = LC.rope_oracle(x, c, table.numpy())
    e_ref = float(np.abs(LC.rope_library(x, c, table.numpy()) - want).max())
    out = torch.full((B * T, wd), float("nan"), device="cuda")
    A.rope(_dev(x), table.cuda(), out, T, hq, d, dv, kv_heads=hkv)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    err, allow = float(np.abs(got.astype(np.float64) - want).max()), LC.allowance(want, e_ref)
    print(f"rope_f32 {c}: e_ref {e_ref:.3e} err {err:.3e} allowance {allow:.3e}")
    assert err <= allow
    np.testing.assert_array_equal(got[:, rotw:], x[:, rotw:])       # V: a copy, bit for bit
    np.testing.assert_array_equal(got[::T], x[::T])                 # position 0 of every image: the identity
    if B > 1:                           # row T is position 0 of image 1; a kernel on the global row rotates it
        assert np.abs(LC.rope_oracle(x, (1, B * T) + c[2:])[T, :rotw] - x[T, :rotw]).max() > 1e-2


@pytest.mark.parametrize("c", LC.ROPE_CASES, ids=str)
def test_rope_bf16(c):
    B, T, hq, hkv, d, dv, W = c
    x = LC.rope_inputs(c, bf16=True)
    table = A.rope_table(T, d, W)
    wd, rotw = LC.rope_width(c), (hq + hkv) * d
    ld = _pad8(wd)
    want = LC.rope_oracle(x, c, table.numpy())
    e_ref = float(np.abs(LC.rope_library(x, c, table.numpy()) - want).max())
    xp = torch.full((B * T, ld), float("nan"), dtype=torch.bfloat16)             # the pads hold NaN
    xp[:, :wd] = torch.from_numpy(x).to(torch.bfloat16)
    out = torch.full((B * T, ld), float("nan"), dtype=torch.bfloat16, device="cuda")
    A.rope(xp.cuda(), table.cuda(), out, T, hq, d, dv, kv_heads=hkv)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy()
    assert (got[:, wd:] == 0).all(), "padding channels must come out as exact zeros"
    np.testing.assert_array_equal(got[:, rotw:wd], x[:, rotw:wd])   # V: a copy, bit for bit
    np.testing.assert_array_equal(got[::T, :wd], x[::T])            # position 0: exact also after the one rounding
    err = np.abs(got[:, :wd].astype(np.float64) - want)
    allow = LC.allowance(want, e_ref, bf16=True)
    print(f"rope_bf16 {c}: e_ref {e_ref:.3e} err {err.max():.3e} allowance {np.max(allow):.3e}")
    assert (err <= allow).all()


def test_rope_refuses_what_it_cannot_rotate():
    x = torch.zeros((4, 24), device="cuda")
    table = A.rope_table(4, 4, 10000.0, device="cuda")
    A.rope(x, table, torch.empty_like(x), 4, 2, 4, 4, kv_heads=2)
    with pytest.raises(ValueError, match="out of place"):
        A.rope(x, table, x, 4, 2, 4, 4, kv_heads=2)
    with pytest.raises(ValueError, match="even"):
        A.rope(x, table, torch.empty_like(x), 4, 2, 3, 3, kv_heads=2)
    with pytest.raises(ValueError):
        A.rope(x, table, torch.empty_like(x), 4, 4, 4, 4, kv_heads=2)               # 32 columns do not fit 24
    with pytest.raises(ValueError):
        A.rope(x, table[:, :3].contiguous(), torch.empty_like(x), 4, 2, 4, 4, kv_heads=2)
    with pytest.raises(ValueError):
        A.rope(x, table.to(torch.bfloat16), torch.empty_like(x), 4, 2, 4, 4, kv_heads=2)   # the table stays fp32


# ------------------------------------------------------------------- GQA core
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("c", GQA_CASES, ids=str)
def test_gqa_attention_f32(c, causal):
    B, T, hq, hkv, d, dv, probe = c
    x = LC.gqa_inputs(c)
    want = LC.gqa_oracle(x, c, causal)
    e_ref = float(np.abs(LC.gqa_library(x, c, causal) - want).max())
    out = torch.full((B * T, hq * dv), float("nan"), device="cuda")
    A.attention(_dev(x), out, B, T, hq, d, dv, causal=causal, kv_heads=hkv)
    wide = torch.full((B * T, hq * dv), float("nan"), device="cuda")
    A.attention(_dev(LC.gqa_expanded(x, c)), wide, B, T, hq, d, dv, causal=causal)
    torch.cuda.synchronize()
    err, allow = float(np.abs(out.double().cpu().numpy() - want).max()), LC.allowance(want, e_ref)
    print(f"gqa f32 {c} causal={causal} [{A.attention_path(d, dv)}]: e_ref {e_ref:.3e} err {err:.3e} "
          f"allowance {allow:.3e}")
    assert err <= allow
    assert torch.equal(out, wide), "a GQA launch must equal the plain launch on the expanded rows bit for bit"


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("c", GQA_CASES, ids=str)
def test_gqa_attention_bf16(c, causal):
    B, T, hq, hkv, d, dv, probe = c
    x = LC.gqa_inputs(c, bf16=True)
    want = LC.gqa_oracle(x, c, causal)
    e_ref = float(np.abs(LC.gqa_library(x, c, causal) - want).max())
    w_in, w_out = LC.gqa_width(c), hq * dv

    def rows(a):
        p = torch.full((B * T, _pad8(a.shape[1])), float("nan"), dtype=torch.bfloat16)     # the pads hold NaN
        p[:, :a.shape[1]] = torch.from_numpy(a).to(torch.bfloat16)
        return p.cuda()
    out = torch.full((B * T, _pad8(w_out)), float("nan"), dtype=torch.bfloat16, device="cuda")
    A.attention(rows(x), out, B, T, hq, d, dv, causal=causal, kv_heads=hkv)
    wide = torch.full_like(out, float("nan"))
    A.attention(rows(LC.gqa_expanded(x, c)), wide, B, T, hq, d, dv, causal=causal)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().astype(np.float64)
    assert (got[:, w_out:] == 0).all(), "padding channels must come out as exact zeros"
    err = np.abs(got[:, :w_out] - want)
    allow = LC.allowance(want, e_ref, bf16=True)
    print(f"gqa bf16 {c} causal={causal}: e_ref {e_ref:.3e} err {err.max():.3e} allowance {np.max(allow):.3e}")
    assert (err <= allow).all()
    assert torch.equal(out, wide), "a GQA launch must equal the plain launch on the expanded rows bit for bit"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("c", [GQA_CASES[0], GQA_CASES[3], GQA_CASES[5], GQA_CASES[8]], ids=str)
def test_kv_heads_equal_to_heads_or_none_is_the_launch_as_it_was(c, causal, dtype):
    """Multi-head rows (each K / V head standing once per query head) through the wrapper with `kv_heads=heads` and
    with `kv_heads=None` against the existing entry point called directly, not through the wrapper's dispatch: the
    same bits, MFMA and plain path, both precisions."""
    from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops._lib import (
        kernels, ptr, stream_handle)
    B, T, hq, hkv, d, dv, probe = c
    x = LC.gqa_expanded(LC.gqa_inputs(c, bf16=dtype == torch.bfloat16), c)
    bf16 = dtype == torch.bfloat16
    ld_in, ld_out = (_pad8(x.shape[1]), _pad8(hq * dv)) if bf16 else (x.shape[1], hq * dv)
    rows = torch.zeros((B * T, ld_in), dtype=dtype)
    rows[:, :x.shape[1]] = torch.from_numpy(x).to(dtype)
    rows = rows.cuda()
    outs = [torch.full((B * T, ld_out), float("nan"), dtype=dtype, device="cuda") for _ in range(3)]
    A.attention(rows, outs[0], B, T, hq, d, dv, causal=causal, kv_heads=hq)
    A.attention(rows, outs[1], B, T, hq, d, dv, causal=causal, kv_heads=None)
    name = "attention" + ("_causal" if causal else "") + ("_bf16" if bf16 else "_f32")
    getattr(kernels(), name)(ptr(rows), ptr(outs[2]), B, T, hq, d, dv, ld_in, ld_out, stream_handle(None))
    torch.cuda.synchronize()
    assert torch.isfinite(outs[2]).all()
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[2])


def test_gqa_attention_refuses_what_it_cannot_hold():
    x = torch.zeros((8, 4 * 16 + 2 * 32), device="cuda")
    out = torch.zeros((8, 64), device="cuda")
    A.attention(x, out, 2, 4, 4, 16, 16, kv_heads=2)
    with pytest.raises(ValueError, match="kv_heads"):
        A.attention(x, out, 2, 4, 4, 16, 16, kv_heads=3)
    with pytest.raises(ValueError):
        A.attention(x, out, 2, 4, 4, 16, 16, kv_heads=4)                # plain rows need 192 columns, not 128
    with pytest.raises(ValueError, match="padding mask"):
        A.attention(x, out, 2, 4, 4, 16, 16, kv_heads=2, key_mask=torch.ones(8, device="cuda"))
