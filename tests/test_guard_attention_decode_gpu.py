"""Guard-band runs of the decoding kernels, in the form of tests/test_guard_llama_gpu.py: `kv_append` and
`attention_decode` with its combine kernel at two ragged cases each, every buffer between 1 MiB guards
(tests/guardband.py), the caches and the split workspace included.

Each case runs twice, with NaN and with +inf in the guards of everything a kernel reads (rows, table, caches,
query) and in the cache rows beyond every length; outputs and the workspace are pre-filled with NaN between pattern
guards.  Asserted: every guard intact bit for bit; outputs finite, bit-identical between the two poison runs and
within the bound of tests/test_attention_decode_gpu.py."""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A

import decode_cases as DC
import guardband as G
import llama_cases as LC
pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16]
# (B, T, hq, hkv, d, dv, probe), the lengths of the launch, the least KS: three splits with an empty one, group sizes
# 3 and 8; and 16 sequences on 8 kv heads, where KS = 128 and a wave walks two fragments of a split
DECODE_GUARD = [((3, 129, 6, 2, 64, 64, "dominant"), [1, 65, 129], 64),
                ((2, 150, 8, 1, 128, 128, "ascending"), [17, 150], 64),
                ((16, 257, 16, 8, 32, 16, "ascending"), DC.long_lengths(128), 128)]
# (B, Tn, hq, hkv, d, dv, W), Tmax, pos: the scalar path and the vector path with dv != d; tokens past the cache
APPEND_GUARD = [((2, 5, 4, 2, 6, 6, 10000.0), 9, [2, 7]), ((3, 3, 6, 2, 16, 24, 10000.0), 7, [0, 4, 6])]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c,lengths,ks", DECODE_GUARD, ids=str)
def test_guard_attention_decode(c, lengths, ks, dtype):
    B, T, hq, hkv, d, dv, probe = c
    bf16 = dtype == torch.bfloat16
    x = LC.gqa_inputs(c, bf16=bf16)
    full = LC.gqa_oracle(x, c, True)
    e_ref = float(np.abs(LC.gqa_library(x, c, True) - full).max())
    want = np.stack([full[b * T + L - 1] for b, L in enumerate(lengths)])
    xt = torch.from_numpy(x).to(dtype)
    q, k, v = LC.gqa_split(xt, c)
    S, KS, wsn = A.attention_decode_plan(B, hkv, T, hq, dv)
    assert S > 1 and KS >= ks
    outs = {}
    for poison in (G.NAN, G.INF):
        kp = torch.full((B, hkv, T, d), float(poison), dtype=dtype)
        vp = torch.full((B, hkv, T, dv), float(poison), dtype=dtype)
        for b, L in enumerate(lengths):                 # the rows beyond a length hold the poison
            kp[b, :, :L] = k[b, :L].transpose(0, 1)
            vp[b, :, :L] = v[b, :L].transpose(0, 1)
        kc = G.guarded(kp.shape, dtype, "cuda", payload=kp, poison=poison, name="kcache")
        vc = G.guarded(vp.shape, dtype, "cuda", payload=vp, poison=poison, name="vcache")
        qp = torch.stack([q[b, L - 1].reshape(-1) for b, L in enumerate(lengths)])
        qg = G.guarded(qp.shape, dtype, "cuda", payload=qp, poison=poison, name="q")
        pos = G.guarded((B,), torch.int32, "cuda", payload=torch.tensor(lengths, dtype=torch.int32) - 1, poison=0x7F,
                        name="pos")
        ws = G.guarded((wsn,), torch.float32, "cuda", payload=float("nan"), name="workspace")
        out = G.guarded((B, hq * dv + 8), dtype, "cuda", payload=float("nan"), name="out")
        A.attention_decode(qg, kc, vc, pos, out, hq, d, dv, kv_heads=hkv, workspace=ws)
        torch.cuda.synchronize()
        G.check(kc, vc, qg, pos, ws, out, what=f"[attention_decode {c} {dtype}, {poison} poison]")
        outs[poison] = out.cpu()
    assert torch.isfinite(outs[G.NAN]).all() and torch.equal(outs[G.NAN], outs[G.INF])
    got = outs[G.NAN].float().numpy().astype(np.float64)
    assert (got[:, hq * dv:] == 0).all()
    assert (np.abs(got[:, :hq * dv] - want) <= LC.allowance(want, e_ref, bf16=bf16)).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("rotate", [False, True], ids=["copy", "rope"])
@pytest.mark.parametrize("c,Tmax,posv", APPEND_GUARD, ids=str)
def test_guard_kv_append(c, Tmax, posv, rotate, dtype):
    B, Tn, hq, hkv, d, dv, W = c
    bf16 = dtype == torch.bfloat16
    wd = LC.rope_width(c)
    ld = (wd + 7) // 8 * 8 if bf16 else wd
    x = LC.rope_inputs(c, bf16=bf16)
    table = A.rope_table(Tmax, d, W)
    res = {}
    for poison in (G.NAN, G.INF):
        xs = torch.full((B * Tn, ld), float(poison), dtype=dtype)       # the row padding holds the poison too
        xs[:, :wd] = torch.from_numpy(x).to(dtype)
        xg = G.guarded(xs.shape, dtype, "cuda", payload=xs, poison=poison, name="x")
        tg = G.guarded(table.shape, torch.float32, "cuda", payload=table, poison=poison, name="table")
        kc = G.guarded((B, hkv, Tmax, d), dtype, "cuda", payload=0.0, name="kcache")
        vc = G.guarded((B, hkv, Tmax, dv), dtype, "cuda", payload=0.0, name="vcache")
        pos = G.guarded((B,), torch.int32, "cuda", payload=torch.tensor(posv, dtype=torch.int32), poison=0x7F, name="pos")
        qo = G.guarded((B * Tn, hq * d + 8), dtype, "cuda", payload=0.0, name="q_out") if rotate else None
        A.kv_append(xg, kc, vc, pos, Tn, hq, d, dv, kv_heads=hkv, table=tg if rotate else None, q_out=qo)
        torch.cuda.synchronize()
        G.check(xg, tg, kc, vc, pos, qo, what=f"[kv_append {c} rope={rotate} {dtype}, {poison} poison]")
        res[poison] = [t.cpu() for t in (kc, vc) + ((qo,) if rotate else ())]
    for a, b in zip(res[G.NAN], res[G.INF]):             # the values are checked in tests/test_attention_decode_gpu.py
        assert torch.isfinite(a).all() and torch.equal(a, b)
