"""Guard-band runs of the skinny GEMM (csrc/kernels/gemm_skinny.h), in the form of
tests/test_guard_attention_decode_gpu.py: x, the packed weights, bias, residual, out, workspace and counters between
1 MiB guards (tests/guardband.py), the scratch sized exactly by `skinny_scratch`, at F = 4 (the widest channel tile:
the most rows read past N) and the largest ksplit the case allows (its chunk count: one chunk per split).

What a kernel reads carries NaN in its guards; out and the workspace are pre-filled with NaN between pattern guards.
Asserted: every guard intact bit for bit, the counters zero, the output finite and within the bound of
tests/test_skinny_gemm_gpu.py."""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

import guardband as G
import llama_cases as LC
from test_skinny_gemm_gpu import skinny_case

pytestmark = pytest.mark.gpu
GUARD_CASES = [(3, 176, 128, True, 1), (8, 704, 176, False, 2), (17, 128, 64, False, 0)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", GUARD_CASES, ids=str)
def test_guard_skinny_gemm(case, dtype):
    M, K, N, has_res, act = case
    F, ks = 4, C.skinny_chunks(K, dtype)
    x, pc, res, want = skinny_case(*case, dtype)
    xg = G.rehome(x, poison=G.NAN, name="x")
    pc.w = G.rehome(pc.w, poison=G.NAN, name="w")
    pc.bias = G.rehome(pc.bias, poison=G.NAN, name="bias")
    rg = None if res is None else G.rehome(res, poison=G.NAN, name="residual")
    ws_n, ctr_n = C.skinny_scratch(M, N, K, dtype, F, ks)
    ws = G.guarded((ws_n,), torch.float32, "cuda", payload=float("nan"), name="workspace") if ws_n else None
    ctr = G.guarded((ctr_n,), torch.int32, "cuda", payload=0, name="counters") if ctr_n else None
    out = G.guarded((M, N), dtype, "cuda", payload=float("nan"), name="out")
    C.skinny_forward(xg, pc, out, rg, relu=act, F=F, ksplit=ks, workspace=ws, counters=ctr)
    torch.cuda.synchronize()
    G.check(xg, pc.w, pc.bias, rg, ws, ctr, out, what=f"[skinny {case} {dtype} F {F} ksplit {ks}]")
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all() and (ctr is None or int(ctr.abs().sum()) == 0)
    if dtype == torch.float32:
        assert np.abs(got - want).max() / max(1.0, np.abs(want).max()) < 2e-5
    else:
        assert (np.abs(got - want) <= LC.allowance(want, 0.0, bf16=True)).all()
