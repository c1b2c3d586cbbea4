"""Guard-band runs of the causal attention kernels and the embedding kernel (csrc/kernels/layers.hip), exactly as
tests/test_guard_attention_gpu.py does for the unmasked kernels: every buffer between 1 MiB guards
(tests/guardband.py).

Each case is launched twice, with NaN and with +inf in the guards of everything the kernel reads, the output
pre-filled with NaN.  Asserted: every guard intact bit for bit; outputs finite, bit-identical between the two
poison runs and within the bound of tests/test_causal_attention_gpu.py.  The bf16 input's padding channels hold the
read poison too.  For the embedding the table and the ids are guarded, and the ids include 0, V - 1, V and -1: the
last two must give zero rows without their table rows, which would lie in a guard, being read.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import causal_attention_cases as CC
import guardband as G

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)


def _same_and_finite(outs):
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    return a


@pytest.mark.parametrize("c", CC.GUARD_CASES, ids=str)
def test_guard_causal_attention_f32(c):
    k = CC.case(c)
    outs = {}
    for poison in POISONS:
        x = G.guarded(k.qkv.shape, torch.float32, "cuda", payload=k.qkv, poison=poison, name="qkv")
        out = G.guarded(k.want.shape, torch.float32, "cuda", payload=float("nan"), name="out")
        A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, causal=True)
        torch.cuda.synchronize()
        G.check(x, out, what=f"[causal attention_f32 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    a = _same_and_finite(outs)
    assert np.abs(a.numpy().astype(np.float64) - k.want).max() <= k.allow


@pytest.mark.parametrize("c", CC.GUARD_CASES, ids=str)
def test_guard_causal_attention_bf16(c):
    k = CC.case_bf16(c)
    outs = {}
    for poison in POISONS:
        xp = torch.full((k.B * k.T, k.ld_in), float(poison), dtype=torch.bfloat16)     # the pads hold the poison too
        xp[:, :k.w_in] = torch.from_numpy(k.qkv).to(torch.bfloat16)
        x = G.guarded(xp.shape, torch.bfloat16, "cuda", payload=xp, poison=poison, name="qkv")
        out = G.guarded((k.B * k.T, k.ld_out), torch.bfloat16, "cuda", payload=float("nan"), name="out")
        A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, causal=True)
        torch.cuda.synchronize()
        G.check(x, out, what=f"[causal attention bf16 {c}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs).float().numpy().astype(np.float64)
    assert (got[:, k.w_out:] == 0).all(), "padding channels must come out as exact zeros"
    assert (np.abs(got[:, :k.w_out] - k.want) <= 2.0 ** -8 * np.abs(k.want) + k.allow).all()


# (V, C, B, T): a vector row in both types; a row that is scalar in bf16 only; a scalar row in both (C = 5)
EMBEDDING_CASES = [(300, 64, 2, 9), (300, 20, 2, 9), (7, 5, 1, 6)]


@pytest.mark.parametrize("c", EMBEDDING_CASES, ids=str)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_embedding(c, dtype):
    V, C, B, T = c
    rng = np.random.default_rng(V + C)
    emb = rng.standard_normal((V, C)).astype(np.float32)
    ids = rng.integers(0, V, (B, T)).astype(np.float32)
    ids[0, :6] = (0, V - 1, V, -1, V - 1 + 0.75, 0.5)               # both ends, both sides out, two fractions
    table = A.embedding_table(emb, dtype)
    ld = table.shape[1]
    assert ld == (C if dtype == torch.float32 else (C + 7) // 8 * 8)
    want = table.float().numpy()[np.clip(ids.astype(np.int64), 0, V - 1)]
    want[(ids <= -1) | (ids >= V)] = 0.0
    outs = {}
    for poison in POISONS:
        tb = G.guarded(table.shape, dtype, "cuda", payload=table, poison=poison, name="table")
        ix = G.guarded(ids.shape, torch.float32, "cuda", payload=ids, poison=poison, name="ids")
        out = G.guarded((B, 1, T, ld), dtype, "cuda", payload=float("nan"), name="out")
        A.embedding(ix, tb, out)
        torch.cuda.synchronize()
        G.check(tb, ix, out, what=f"[embedding {c} {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    got = _same_and_finite(outs).float().numpy()
    np.testing.assert_array_equal(got[:, 0], want)                  # a gather: bit for bit, padding zeros included
    assert (got[0, 0, 2] == 0).all() and (got[0, 0, 3] == 0).all() and (got[..., C:] == 0).all()


def test_embedding_refuses_what_it_cannot_index_or_hold():
    table = torch.zeros((8, 16), dtype=torch.float32, device="cuda")
    ids = torch.zeros((2, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 1, 3, 16), dtype=torch.float32, device="cuda")
    A.embedding(ids, table, out)
    with pytest.raises(ValueError):
        A.embedding(ids.to(torch.int32), table, out)                # ids travel as float32
    with pytest.raises(ValueError):
        A.embedding(ids, table, out.to(torch.bfloat16))
    with pytest.raises(ValueError):
        A.embedding(ids, table, out[:, :, :2].contiguous())
    with pytest.raises(ValueError):
        A.embedding(ids, table.to(torch.bfloat16)[:, :12].contiguous(), out.to(torch.bfloat16)[..., :12].contiguous())
    with pytest.raises(ValueError):
        A.embedding_table(np.zeros((4,), np.float32), torch.float32)
