"""Guard-band runs of the MXFP4 tile GEMM (csrc/kernels/gemm_tile_mx.h), in the form of
tests/test_guard_skinny_mx_gpu.py: x, codes, scales, bias, residual, out, workspace and counters between 1 MiB guards
(tests/guardband.py), the scratch sized exactly by `mx_tile_scratch`, at the widest tile (the most rows and
channels a block covers past M and N) and the largest ksplit the case allows (one chunk per split).

Asserted: every guard intact bit for bit, the counters zero, the output finite and within the bound of
tests/test_tile_mx_gpu.py."""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

import guardband as G
import llama_cases as LC
from test_skinny_mx_gpu import mx_case

pytestmark = pytest.mark.gpu
GUARD_CASES = [(33, 176, 128, True, 1), (65, 704, 176, False, 2), (130, 1152, 40, True, 0)]


@pytest.mark.parametrize("case", GUARD_CASES, ids=str)
def test_guard_tile_mx(case):
    M, K, N, has_res, act = case
    (F, MT), ks = C.MX_TILES[0], C.mx_chunks(K)
    x, pc, res, want = mx_case(*case)
    xg = G.rehome(x, poison=G.NAN, name="x")
    # integer tensors: guards of 0xFF bytes, the scale byte 255 (NaN in e8m0, infinity as the fp32 pattern) over
    # codes of -6, so a read outside shows as a non-finite output
    pc.mx = C.MxWeights(G.rehome(pc.mx.codes, poison=0xFF, name="codes"),
                        G.rehome(pc.mx.scales, poison=0xFF, name="scales"))
    pc.bias = G.rehome(pc.bias, poison=G.NAN, name="bias")
    rg = None if res is None else G.rehome(res, poison=G.NAN, name="residual")
    ws_n, ctr_n = C.mx_tile_scratch(M, N, K, F, MT, ks)
    ws = G.guarded((ws_n,), torch.float32, "cuda", payload=float("nan"), name="workspace")
    ctr = G.guarded((ctr_n,), torch.int32, "cuda", payload=0, name="counters")
    out = G.guarded((M, N), torch.bfloat16, "cuda", payload=float("nan"), name="out")
    C.mx_tile_forward(xg, pc, out, rg, relu=act, F=F, MT=MT, ksplit=ks, workspace=ws, counters=ctr)
    torch.cuda.synchronize()
    G.check(xg, pc.mx.codes, pc.mx.scales, pc.bias, rg, ws, ctr, out, what=f"[tile mx {case} ksplit {ks}]")
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all() and int(ctr.abs().sum()) == 0
    assert (np.abs(got - want) <= LC.allowance(want, 0.0, bf16=True)).all()
