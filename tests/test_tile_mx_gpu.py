"""`ops.conv.mx_tile_forward` (csrc/kernels/gemm_tile_mx.h) against float64 numpy on dequantize(quantize(W)), with
the cases of tests/test_skinny_mx_gpu.py's `mx_case` (per-block power-of-two scales: a wrong scale byte is off by
2x) and that file's bound, `llama_cases.allowance(want, 0, bf16=True)`: the same instruction on exact operands,
fp32 sums, one output rounding.

Cases (M, K, N, residual, act, ksplits), on every (F, MT) tile:
  (1, 32, 64)        one row, one block; its ksplit 2 is above the one chunk
  (33, 176, 128)     a partial last block of 32 k, a partial row fragment
  (65, 704, 176)     a second row tile at BM = 64, 11 channel fragments, ksplit 3: uneven splits
  (130, 1152, 40)    two row tiles at BM = 128; 9 chunks: both LDS buffers and both code sets; a partial fragment
  (257, 256, 264)    a second channel tile at the widest tile, three row tiles
Every ksplit > 1 runs twice on the same counters: bit-equal outputs, counters zero.  A ksplit above the chunk
count is asserted to be refused."""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

import llama_cases as LC
from test_skinny_mx_gpu import mx_case

pytestmark = pytest.mark.gpu
CASES = [(1, 32, 64, False, 0, (1, 2)), (33, 176, 128, True, 1, (1, 2)), (65, 704, 176, False, 2, (1, 2, 3)),
         (130, 1152, 40, True, 0, (1, 2)), (257, 256, 264, False, 0, (1,))]


@pytest.mark.parametrize("tile", C.MX_TILES, ids=str)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_tile_mx_matches_fp64(case, tile):
    M, K, N, has_res, act, splits = case
    F, MT = tile
    x, pc, res, want = mx_case(M, K, N, has_res, act)
    for ks in splits:
        ws_n, ctr_n = C.mx_tile_scratch(M, N, K, F, MT, ks)
        ctr = torch.zeros(max(ctr_n, 1), dtype=torch.int32, device="cuda")
        if ks > C.mx_chunks(K):
            with pytest.raises(ValueError, match="ksplit"):
                C.mx_tile_forward(x, pc, torch.empty((M, N), dtype=torch.bfloat16, device="cuda"), res, relu=act, F=F,
                                  MT=MT, ksplit=ks, counters=ctr)
            continue
        outs = []
        for _ in range(2 if ks > 1 else 1):             # twice on the same counters: they came back zero
            out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
            C.mx_tile_forward(x, pc, out, res, relu=act, F=F, MT=MT, ksplit=ks, counters=ctr)
            outs.append(out.cpu())
        got = outs[0].double().numpy()
        err = np.abs(got - want)
        print(f"{case} tile {tile} ks {ks}: max err {err.max():.3e}, rel {err.max() / max(1, np.abs(want).max()):.3e}")
        assert np.isfinite(got).all()
        assert (err <= LC.allowance(want, 0.0, bf16=True)).all()
        assert torch.equal(outs[0], outs[-1]) and int(ctr.abs().sum()) == 0
        assert ws_n == (ks > 1) * ks * M * N and ctr_n == (ks > 1) * -(-M // (16 * MT)) * -(-N // (64 * F))


def test_tile_mx_refusals():
    out = torch.empty((40, 64), dtype=torch.bfloat16, device="cuda")
    x, pc, _, _ = mx_case(40, 64, 64, False, 0)
    with pytest.raises(ValueError, match="bf16"):                        # an fp32 x
        C.mx_tile_forward(x.float(), pc, out)
    rng = np.random.default_rng(0)
    only = C.pack_conv_mxfp4(rng.standard_normal((1, 1, 64, 64)).astype(np.float32), np.zeros(64, np.float32), "cuda",
                             keep_bf16=False)
    assert tuple(only.w.shape) == (0, pc.Kpad) and only.w.dtype == torch.bfloat16 and C.mx_tile_supported(only, 40)
    with pytest.raises(ValueError, match="codes alone"):                 # no weight rows: no tile config, no skinny GEMM
        C.conv_forward(x, only, out)
    with pytest.raises(ValueError, match="codes alone"):
        C.skinny_forward(x[:4], only, out[:4])
    pc.mx = None
    assert not C.mx_tile_supported(pc, 40)
    with pytest.raises(ValueError, match="no MXFP4 codes"):              # a PackedConv without codes
        C.mx_tile_forward(x, pc, out)
