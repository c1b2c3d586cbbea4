"""`ops.conv.skinny_forward` (csrc/kernels/gemm_skinny.h) against float64 numpy on the same inputs (bf16: rounded to
bf16 first).  fp32 bound: the one of tests/test_gemm_f32s_gpu.py (same instruction and accumulation); bf16:
`llama_cases.allowance(want, 0, bf16=True)`, one rounding of the output.

Cases (M, K, N, residual, act), chosen for the chunk of 64 (fp32) / 128 (bf16) k:
  (1, 64, 64)     one row; one chunk or less, so three waves bring zero partials through the LDS merge
  (3, 176, 128)   llama_micro's MLP: a chunk tail, in bf16 a half-masked last MFMA step (K % 32 == 16)
  (8, 704, 176)   11 channel fragments (a partial channel tile at F = 2 and 4), several chunks per wave,
                  ksplit 1, 2, 3 (3: uneven splits)
  (16, 256, 40)   a full row fragment with a partial channel fragment; fp32 also at N = 36
  (17, 128, 64), (32, 320, 96)   the second row fragment, partial and full
A case without ksplit values of its own runs 1 and 2.  A ksplit above the case's chunk count (2 on one chunk:
(1, 64, 64), and bf16 (17, 128, 64)) is what `skinny_forward` refuses, and is asserted to be refused."""
import math

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

import llama_cases as LC

pytestmark = pytest.mark.gpu
CASES = [(1, 64, 64, False, 0, (1, 2)), (3, 176, 128, True, 1, (1, 2)), (8, 704, 176, False, 2, (1, 2, 3)),
         (16, 256, 40, True, 0, (1, 2)), (16, 256, 36, True, 0, (1, 2)), (17, 128, 64, False, 0, (1, 2)),
         (32, 320, 96, True, 1, (1, 2))]
# N = 36 is the fp32 case: bf16 rows are multiples of 8 channels
PARAMS = [(c, d) for c in CASES for d in (torch.float32, torch.bfloat16) if d == torch.float32 or c[2] % 8 == 0]


def skinny_case(M, K, N, has_res, act, dtype, kh=1):
    """(x, pc, residual, float64 result) of one case, inputs rounded to `dtype`."""
    rng = np.random.default_rng(1000 * M + K + N)
    rnd = lambda a: torch.from_numpy(a.astype(np.float32)).to(dtype)      # noqa: E731
    x = rnd(rng.standard_normal((M, K)))
    kern = rnd(rng.standard_normal((kh, kh, K, N)) / np.sqrt(K))
    bias = rng.standard_normal(N).astype(np.float32)
    res = rnd(rng.standard_normal((M, N))) if has_res else None
    pack = C.pack_conv_f32 if dtype == torch.float32 else C.pack_conv
    pc = pack(kern.float().numpy(), bias, 1, ((0, 0), (0, 0)), "cuda")
    want = x.double().numpy() @ kern.double().numpy()[0, 0] + bias
    if has_res:
        want = want + res.double().numpy()
    want = want if act == 0 else np.clip(want, 0, 6.0 if act == 2 else None)
    return x.cuda(), pc, None if res is None else res.cuda(), want


@pytest.mark.parametrize("F", C.SKINNY_F)
@pytest.mark.parametrize("case,dtype", PARAMS, ids=str)
def test_skinny_gemm_matches_fp64(case, dtype, F):
    M, K, N, has_res, act, splits = case
    x, pc, res, want = skinny_case(M, K, N, has_res, act, dtype)
    for ks in splits:
        ws_n, ctr_n = C.skinny_scratch(M, N, K, dtype, F, ks)
        ctr = torch.zeros(max(ctr_n, 1), dtype=torch.int32, device="cuda")
        if ks > C.skinny_chunks(K, dtype):
            with pytest.raises(ValueError, match="ksplit"):
                C.skinny_forward(x, pc, torch.empty((M, N), dtype=dtype, device="cuda"), res, relu=act, F=F, ksplit=ks,
                                 counters=ctr)
            continue
        outs = []
        for _ in range(2 if ks > 1 else 1):             # twice on the same counters: they came back zero
            out = torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
            C.skinny_forward(x, pc, out, res, relu=act, F=F, ksplit=ks, counters=ctr)
            outs.append(out.cpu())
        got = outs[0].double().numpy()
        err = np.abs(got - want)
        print(f"{case} F {F} ks {ks} {dtype}: max err {err.max():.3e}, rel {err.max() / max(1, np.abs(want).max()):.3e}")
        assert np.isfinite(got).all()
        if dtype == torch.float32:
            assert err.max() / max(1.0, np.abs(want).max()) < 2e-5
        else:
            assert (err <= LC.allowance(want, 0.0, bf16=True)).all()
        assert torch.equal(outs[0], outs[-1]) and int(ctr.abs().sum()) == 0
        assert ws_n == (ks > 1) * ks * M * N and ctr_n == (ks > 1) * math.ceil(N / (16 * F))


def test_skinny_gemm_refusals():
    out = torch.empty((33, 64), device="cuda")
    x, pc, _, _ = skinny_case(33, 64, 64, False, 0, torch.float32)
    with pytest.raises(ValueError, match="skinny"):                      # M = 33
        C.skinny_forward(x, pc, out)
    x, pc3, _, _ = skinny_case(4, 64, 64, False, 0, torch.float32, kh=3)
    with pytest.raises(ValueError, match="skinny"):                      # a 3x3 conv
        C.skinny_forward(x, pc3, out[:4])
    x, pc, _, _ = skinny_case(4, 64, 64, False, 0, torch.float32)
    with pytest.raises(ValueError, match="ksplit"):                      # one chunk, two splits
        C.skinny_forward(x, pc, out[:4], ksplit=2, counters=torch.zeros(4, dtype=torch.int32, device="cuda"))
    pc.n_split = 32
    with pytest.raises(ValueError, match="skinny"):                      # merged siblings
        C.skinny_forward(x, pc, out[:4])
