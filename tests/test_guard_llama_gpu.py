"""Guard-band runs of the Llama kernels, as tests/test_guard_causal_gpu.py does for the causal ones: rmsnorm, the
rope step and both paths of the grouped-query attention core, each at its ragged cases, every buffer between 1 MiB
guards (tests/guardband.py).

Each case is launched twice, with NaN and with +inf in the guards of everything the kernel reads (inputs, scale,
the rope table), the output pre-filled with NaN between pattern guards.  Asserted: every guard intact bit for bit;
outputs finite, bit-identical between the two poison runs and within the bound of
tests/test_llama_kernels_gpu.py.  A bf16 input's padding channels hold the read poison too.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E

import guardband as G
import llama_cases as LC

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)
QT, KT = A.attention_tiles()
DTYPES = [torch.float32, torch.bfloat16]

# rows off the rows-per-block of every lane split, C off the vector on both looped paths, the widest register row
RMSNORM_GUARD = [c for c in LC.RMSNORM_CASES if c[:2] in ((3, 6), (65, 100), (130, 40), (3, 4099), (5, 2048))]
# the scalar path, one fp32 vector, the vector path with T = 33 rows per image, dv != d, a V tail of 5 columns
ROPE_GUARD = [c for c in LC.ROPE_CASES if (c[1], c[4], c[5]) in ((33, 6, 6), (33, 8, 8), (33, 16, 16), (7, 16, 24),
                                                                  (130, 32, 5))]
# MFMA path one key past a tile and at 197 tokens, plain path with odd head sizes
GQA_GUARD = [c for c in LC.gqa_cases(QT, KT) if (c[1], c[4], c[5]) in ((KT + 1, 64, 64), (197, 64, 64), (KT + 1, 6, 5),
                                                                        (QT + 1, 24, 24))]


def _pad8(n):
    return (n + 7) // 8 * 8


def _same_and_finite(outs):
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    return a.float().numpy().astype(np.float64)


def _rows(a, dtype, poison):
    """[rows][width] values as the dtype's layout: bf16 rows padded to 8 channels, the pads holding the poison."""
    if dtype == torch.float32:
        return torch.from_numpy(np.ascontiguousarray(a))
    p = torch.full((a.shape[0], _pad8(a.shape[1])), float(poison), dtype=torch.bfloat16)
    p[:, :a.shape[1]] = torch.from_numpy(a).to(torch.bfloat16)
    return p


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", RMSNORM_GUARD, ids=str)
def test_guard_rmsnorm(c, dtype):
    rows, C, eps, scale, probe = c
    bf16 = dtype == torch.bfloat16
    x, sc = LC.rmsnorm_inputs(c, bf16=bf16)
    want = LC.rmsnorm_oracle(x, sc, eps)
    e_ref = float(np.abs(LC.rmsnorm_library(x, sc, eps) - want).max())
    ld = _pad8(C) if bf16 else C
    scp = np.zeros(ld, np.float32)
    scp[:C] = sc if scale else 1.0
    outs = {}
    for poison in POISONS:
        xs = _rows(x, dtype, poison)
        xg = G.guarded(xs.shape, dtype, "cuda", payload=xs, poison=poison, name="x")
        sg = G.guarded((ld,), torch.float32, "cuda", payload=scp, poison=poison, name="scale")
        out = G.guarded((rows, ld), dtype, "cuda", payload=float("nan"), name="out")
        if bf16:
            E.rmsnorm(xg, sg, out, C, eps)
        else:
            E.rmsnorm_f32(xg, sg, out, eps)
        torch.cuda.synchronize()
        G.check(xg, sg, out, what=f"[rmsnorm {c} {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs)
    assert (got[:, C:] == 0).all()
    assert (np.abs(got[:, :C] - want) <= LC.allowance(want, e_ref, bf16=bf16)).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", ROPE_GUARD, ids=str)
def test_guard_rope(c, dtype):
    B, T, hq, hkv, d, dv, W = c
    bf16 = dtype == torch.bfloat16
    x = LC.rope_inputs(c, bf16=bf16)
    table = A.rope_table(T, d, W)
    wd, rotw = LC.rope_width(c), (hq + hkv) * d
    want = LC.rope_oracle(x, c, table.numpy())
    e_ref = float(np.abs(LC.rope_library(x, c, table.numpy()) - want).max())
    outs = {}
    for poison in POISONS:
        xs = _rows(x, dtype, poison)
        xg = G.guarded(xs.shape, dtype, "cuda", payload=xs, poison=poison, name="qkv")
        tg = G.guarded(table.shape, torch.float32, "cuda", payload=table, poison=poison, name="table")
        out = G.guarded(xs.shape, dtype, "cuda", payload=float("nan"), name="rot")
        A.rope(xg, tg, out, T, hq, d, dv, kv_heads=hkv)
        torch.cuda.synchronize()
        G.check(xg, tg, out, what=f"[rope {c} {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs)
    assert (got[:, wd:] == 0).all()
    np.testing.assert_array_equal(got[:, rotw:wd], x[:, rotw:wd].astype(np.float64))
    assert (np.abs(got[:, :wd] - want) <= LC.allowance(want, e_ref, bf16=bf16)).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("c", GQA_GUARD, ids=str)
def test_guard_gqa_attention(c, causal, dtype):
    B, T, hq, hkv, d, dv, probe = c
    bf16 = dtype == torch.bfloat16
    x = LC.gqa_inputs(c, bf16=bf16)
    want = LC.gqa_oracle(x, c, causal)
    e_ref = float(np.abs(LC.gqa_library(x, c, causal) - want).max())
    w_out = hq * dv
    ld_out = _pad8(w_out) if bf16 else w_out
    outs = {}
    for poison in POISONS:
        xs = _rows(x, dtype, poison)
        xg = G.guarded(xs.shape, dtype, "cuda", payload=xs, poison=poison, name="qkv")
        out = G.guarded((B * T, ld_out), dtype, "cuda", payload=float("nan"), name="out")
        A.attention(xg, out, B, T, hq, d, dv, causal=causal, kv_heads=hkv)
        torch.cuda.synchronize()
        G.check(xg, out, what=f"[gqa attention {c} causal={causal} {dtype} {A.attention_path(d, dv)}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs)
    assert (got[:, w_out:] == 0).all()
    assert (np.abs(got[:, :w_out] - want) <= LC.allowance(want, e_ref, bf16=bf16)).all()
