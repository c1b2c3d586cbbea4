"""Row-split F(4x4, 3x3) Winograd (csrc/kernels/wino4s_f32.hip, cfg ids 238+): a block owns rows of the 6x6
position grid and all of K, leaves them half-transformed, and wino4s_finish_kernel completes the output.

Every row-split config against a float64 `F.conv2d` of the same fp32 data, at the bound of the kernel family
(max abs error over max abs reference < 3e-5), with and without ReLU.  Shapes (B, H, W, C, N):

* (1, 4, 4, 16, 32): one tile, one chunk;
* (3, 13, 10, 32, 48): edge tiles, 36 tiles (not a multiple of 16), N not a power of two;
* (5, 5, 6, 16, 16): 20 tiles, a partial tile group with WT = 2;
* (2, 14, 14, 256, 256) and (4, 7, 7, 512, 512): the two target layer shapes at a small batch (16 / 32 chunks);
* (2, 28, 28, 128, 128): the stage-3 shape;
* (3, 13, 10, 32, 64): the edge-tile map again with an N that every config's channel block divides (N = 48 and
  N = 16 run on the configs with one channel group per block and must raise ValueError on the others).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C_

pytestmark = pytest.mark.gpu

CFGS = sorted(C_.WINO4S_ROW_CFGS)
SHAPES = [(1, 4, 4, 16, 32), (3, 13, 10, 32, 48), (5, 5, 6, 16, 16), (2, 14, 14, 256, 256), (4, 7, 7, 512, 512),
          (2, 28, 28, 128, 128), (3, 13, 10, 32, 64)]
BOUND = 3e-5


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Host data, the packed conv and the float64 reference (before ReLU) of one shape, shared by every config."""
    B, H, W, C, N = shape
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    x = torch.randn((B, H, W, C), generator=g)
    k = torch.randn((3, 3, C, N), generator=g) / (3.0 * C ** 0.5)
    b = torch.randn(N, generator=g) * 0.1
    want = F.conv2d(x.double().permute(0, 3, 1, 2), k.double().permute(3, 2, 0, 1), b.double(), padding=1)
    pc = C_.pack_conv_f32(k.numpy(), b.numpy(), 1, ((1, 1), (1, 1)), "cuda")
    return x.cuda(), pc, want.permute(0, 2, 3, 1).contiguous()


def _forward(shape, cfg, relu):
    x, pc, _ = _case(shape)
    B, H, W, C, N = shape
    out = torch.full((B, H, W, N), float("nan"), device="cuda")
    C_.conv_forward_f32(x, pc, out, relu=relu, cfg=cfg, ksplit=1)
    torch.cuda.synchronize()
    return out.cpu()


def test_row_cfgs_are_registered():
    assert CFGS and min(CFGS) == 238
    for cfg in CFGS:
        wt, wn, pg, r, order, rg = C_.WINO4S_F32_CFGS[cfg]
        assert rg in (1, 2, 3) and (6 * rg) % pg == 0 and r >= 2


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cfg", CFGS)
def test_rows_match_float64_conv(cfg, shape):
    B, H, W, C, N = shape
    if N % (16 * C_.WINO4S_F32_CFGS[cfg][1]):
        with pytest.raises(ValueError):
            _forward(shape, cfg, 1)
        return
    want = _case(shape)[2]
    for relu in (1, 0):
        got = _forward(shape, cfg, relu).double()
        ref = torch.relu(want) if relu else want
        assert torch.isfinite(got).all(), (cfg, shape, relu)
        rel = ((got - ref).abs().max() / ref.abs().max()).item()
        print(f"cfg {cfg} shape {shape} relu {relu}: rel {rel:.3e}")
        assert rel < BOUND, (cfg, shape, relu, rel)


@pytest.mark.parametrize("cfg,shape", [(c, s) for c in CFGS for s in ((3, 13, 10, 32, 48), (3, 13, 10, 32, 64),
                                                                      (4, 7, 7, 512, 512))
                                       if s[4] % (16 * C_.WINO4S_F32_CFGS[c][1]) == 0])
def test_two_runs_give_identical_bits(cfg, shape):
    a, b = _forward(shape, cfg, 1), _forward(shape, cfg, 1)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize("cfg", CFGS)
def test_rejects_split_residual_and_channel_block(cfg):
    pc = C_.pack_conv_f32(np.zeros((3, 3, 32, 64), np.float32), np.zeros(64, np.float32), 1, ((1, 1), (1, 1)),
                          "cuda")
    x = torch.zeros((1, 8, 8, 32), device="cuda")
    out = torch.zeros((1, 8, 8, 64), device="cuda")
    ctr = torch.zeros(64, dtype=torch.int32, device="cuda")
    for ks in (2, -2, -1, 4):
        with pytest.raises(ValueError):
            C_.conv_forward_f32(x, pc, out, cfg=cfg, ksplit=ks, counters=ctr)
    with pytest.raises(ValueError):
        C_.conv_forward_f32(x, pc, out, residual=torch.zeros_like(out), cfg=cfg, ksplit=1)
    assert not C_.f32_cfg_supported(cfg, 32, 64, pc, residual=True)
    assert C_.f32_cfg_supported(cfg, 32, 64, pc)
    wn = C_.WINO4S_F32_CFGS[cfg][1]
    pc16 = C_.pack_conv_f32(np.zeros((3, 3, 32, 16), np.float32), np.zeros(16, np.float32), 1, ((1, 1), (1, 1)),
                            "cuda")
    out16 = torch.zeros((1, 8, 8, 16), device="cuda")
    if 16 % (16 * wn):
        with pytest.raises(ValueError):
            C_.conv_forward_f32(x, pc16, out16, cfg=cfg, ksplit=1)
    with pytest.raises(ValueError):                      # a workspace one float short of the contract
        need = C_.wino4s_ws_elems(1, 8, 8, 32, 64, 1, cfg)
        C_.conv_forward_f32(x, pc, out, cfg=cfg, ksplit=1, workspace=torch.empty(need - 1, device="cuda"))
