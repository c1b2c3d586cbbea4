"""CPU checks of the row-split F(4x4, 3x3) Winograd (csrc/kernels/wino4s_f32.hip, cfg ids 238+), in numpy
float64: the separable output transform the GEMM epilogue and wino4s_finish_kernel share between them, and the
workspace layout tr[6][tiles][4][N] behind V against the size the contract function reports."""
import numpy as np
import pytest

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

SHAPES = [(1, 4, 4, 16, 32), (3, 13, 10, 32, 48), (5, 5, 6, 16, 16), (2, 14, 14, 256, 256), (4, 7, 7, 512, 512),
          (2, 28, 28, 128, 128)]


def test_rows_then_columns_is_the_output_transform():
    """tr[a][j] = sum_b A^T[j][b] M[a][b] per row a (a block sees only its own rows), then y[i][j] =
    sum_a A^T[i][a] tr[a][j]: equal to A^T M A for random M, whichever rows a block holds."""
    rng = np.random.default_rng(0)
    AT = C.WINO4_AT
    for rg in (1, 2, 3):
        M = rng.standard_normal((6, 6, 5, 7))                  # [a][b][tile][channel]
        tr = np.zeros((6, 4, 5, 7))
        for a0 in range(0, 6, rg):                             # one block per row group
            rows = M[a0:a0 + rg]
            tr[a0:a0 + rg] = np.einsum("jb,abtn->ajtn", AT, rows)
        y = np.einsum("ia,ajtn->ijtn", AT, tr)
        want = np.einsum("ia,abtn,jb->ijtn", AT, M, AT)
        assert np.allclose(y, want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("B,H,W,Cin,N", SHAPES)
def test_workspace_size_is_the_layouts_last_index_plus_one(B, H, W, Cin, N):
    T = B * ((H + 3) // 4) * ((W + 3) // 4)
    v = ((T + 15) // 16) * 16 * Cin * 36                       # V: 36 positions x 16-tile groups x Cin
    last = v + (((5 * T + (T - 1)) * 4 + 3) * N + (N - 1))    # tr[a = 5][tile T - 1][j = 3][channel N - 1]
    for cfg in sorted(C.WINO4S_ROW_CFGS):
        assert C.wino4s_ws_elems(B, H, W, Cin, N, 1, cfg) == last + 1
    # without a config: enough for every config; the split-K configs keep their own sizes
    assert C.wino4s_ws_elems(B, H, W, Cin, N, 1) == last + 1
    assert C.wino4s_ws_elems(B, H, W, Cin, N, 1, 221) == v
    if (Cin // 16) % 2 == 0:
        assert C.wino4s_ws_elems(B, H, W, Cin, N, 2, 221) == C.wino4s_ws_elems(B, H, W, Cin, N, 2) > v


def test_row_cfgs_take_whole_k_only():
    k = C.kernels()
    for cfg in sorted(C.WINO4S_ROW_CFGS):
        wn = C.WINO4S_F32_CFGS[cfg][1]
        assert k.wino4s_ok(cfg, 64, 16 * wn, 1)
        assert not any(k.wino4s_ok(cfg, 64, 16 * wn, ks) for ks in (2, 4, -2, -4, -1, 0))
        assert not k.wino4s_ok(cfg, 64, 16 * wn + 16, 1) or wn == 1
        assert not k.wino4s_ok(cfg, 24, 16 * wn, 1)


def test_range_check_covers_rows_and_fused_slabs():
    """32-bit byte offsets: the row split's tr[6][T][4][N] and the fused split-K slabs must stay below 2^31
    bytes even where V and U do (wino4s_forward refuses the launch otherwise)."""
    k = C.kernels()
    for cfg in (221, 238, 241):
        assert k.wino4s_range_ok(cfg, 32, 14, 14, 256, 256, 1) and k.wino4s_range_ok(cfg, 32, 7, 7, 512, 512, 1)
    # T = 32 x 16 x 16 = 8192 tiles, C = 16: V is 18.9 MB; N = 4096: tr = 24 T N floats = 3.2 GB
    assert k.wino4s_range_ok(221, 32, 64, 64, 16, 4096, 1)
    assert not k.wino4s_range_ok(238, 32, 64, 64, 16, 4096, 1)
    T, N = 8192, 2752                                   # the first N (a multiple of 32) at which 96 T N reaches 2^31 - 1
    assert 96 * T * (N - 32) < 2 ** 31 - 1 <= 96 * T * N
    assert k.wino4s_range_ok(238, 32, 64, 64, 16, N - 32, 1) and not k.wino4s_range_ok(238, 32, 64, 64, 16, N, 1)
    # fused split-K, cfg 221 (2 x 2 waves): ks x ceil(TG / 2) x N / 32 blocks x 4 waves x 16 KiB
    assert k.wino4s_range_ok(221, 32, 64, 64, 64, 512, -4) == (4 * 256 * 16 * 4 * 16384 < 2 ** 31 - 1)
    assert k.wino4s_range_ok(221, 32, 64, 64, 64, 512, 4)                # the slab + reduce path uses 64-bit offsets
    assert k.wino4s_range_ok(221, 32, 64, 64, 64, 256, -2) and not k.wino4s_range_ok(221, 32, 64, 64, 64, 2048, -4)
