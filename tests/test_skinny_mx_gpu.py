"""`ops.conv.mx_forward` (csrc/kernels/gemm_skinny_mx.h) against float64 numpy: x (bf16) . dequantize(quantize(W))^T
+ bias (+ residual), then the activation.  The bound is tests/test_skinny_gemm_gpu.py's for bf16,
`llama_cases.allowance(want, 0, bf16=True)`: the same instruction, fp32 sums and one output rounding, and the
operands are exact (a dequantised weight is a bf16 number).  The weights are normal / sqrt(K) times 2^j per block of
32 k, j uniform in -6 .. 6: a kernel that picks the wrong scale byte is off by a power of two.

Cases (M, K, N, residual, act, ksplits), for the chunk of 128 k:
  (1, 32, 64)      one row, one block of 32 k: three MFMA steps of the only vector are padding, three waves bring zeros
  (3, 176, 128)    a partial last block (K % 32 == 16), a chunk tail
  (8, 704, 176)    11 channel fragments (a partial channel tile at F = 2, 4, 8), ksplit 1, 2, 3 (3: uneven splits)
  (16, 1152, 40)   9 chunks: two for every wave and a tail, so both register sets run; a partial channel fragment
  (17, 128, 64), (32, 320, 96)   the second row fragment, partial and full
A ksplit above the case's chunk count is asserted to be refused."""
import math

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import mx as MX

import llama_cases as LC

pytestmark = pytest.mark.gpu
CASES = [(1, 32, 64, False, 0, (1, 2)), (3, 176, 128, True, 1, (1, 2)), (8, 704, 176, False, 2, (1, 2, 3)),
         (16, 8 * C.MX_KC + 128, 40, True, 0, (1, 2)), (17, 128, 64, False, 0, (1, 2)), (32, 320, 96, True, 1, (1, 2))]


def mx_case(M, K, N, has_res, act):
    """(x, pc, residual, float64 result) of one case."""
    rng = np.random.default_rng(1000 * M + K + N)
    x = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float32)).bfloat16()
    blocks = 2.0 ** rng.integers(-6, 7, (N, math.ceil(K / 32)))
    w = (rng.standard_normal((N, K)) / np.sqrt(K) * np.repeat(blocks, 32, axis=1)[:, :K]).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    res = torch.from_numpy(rng.standard_normal((M, N)).astype(np.float32)).bfloat16() if has_res else None
    pc = C.pack_conv_mxfp4(np.ascontiguousarray(w.T).reshape(1, 1, K, N), bias, "cuda")
    want = x.double().numpy() @ MX.dequantize_mxfp4(*MX.quantize_mxfp4(w)).astype(np.float64).T + bias
    if has_res:
        want = want + res.double().numpy()
    want = want if act == 0 else np.clip(want, 0, 6.0 if act == 2 else None)
    return x.cuda(), pc, None if res is None else res.cuda(), want


@pytest.mark.parametrize("F", C.MX_F)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_skinny_mx_matches_fp64(case, F):
    M, K, N, has_res, act, splits = case
    x, pc, res, want = mx_case(M, K, N, has_res, act)
    for ks in splits:
        ws_n, ctr_n = C.mx_scratch(M, N, K, F, ks)
        ctr = torch.zeros(max(ctr_n, 1), dtype=torch.int32, device="cuda")
        if ks > C.mx_chunks(K):
            with pytest.raises(ValueError, match="ksplit"):
                C.mx_forward(x, pc, torch.empty((M, N), dtype=torch.bfloat16, device="cuda"), res, relu=act, F=F,
                             ksplit=ks, counters=ctr)
            continue
        outs = []
        for _ in range(2 if ks > 1 else 1):             # twice on the same counters: they came back zero
            out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
            C.mx_forward(x, pc, out, res, relu=act, F=F, ksplit=ks, counters=ctr)
            outs.append(out.cpu())
        got = outs[0].double().numpy()
        err = np.abs(got - want)
        print(f"{case} F {F} ks {ks}: max err {err.max():.3e}, rel {err.max() / max(1, np.abs(want).max()):.3e}")
        assert np.isfinite(got).all()
        assert (err <= LC.allowance(want, 0.0, bf16=True)).all()
        assert torch.equal(outs[0], outs[-1]) and int(ctr.abs().sum()) == 0
        assert ws_n == (ks > 1) * ks * M * N and ctr_n == (ks > 1) * math.ceil(N / (16 * F))


def test_skinny_mx_refusals():
    out = torch.empty((33, 64), dtype=torch.bfloat16, device="cuda")
    x, pc, _, _ = mx_case(33, 64, 64, False, 0)
    with pytest.raises(ValueError, match="MXFP4"):                       # M = 33
        C.mx_forward(x, pc, out)
    with pytest.raises(ValueError, match="bf16"):                        # an fp32 x
        C.mx_forward(x[:4].float(), pc, out[:4])
    pc.mx = None
    assert not C.mx_supported(pc, 4)
    with pytest.raises(ValueError, match="no MXFP4 codes"):              # a PackedConv without codes
        C.mx_forward(x[:4], pc, out[:4])
