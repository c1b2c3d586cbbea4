"""Even-lattice launches of the split F(4x4, 3x3) Winograd (csrc/kernels/wino4s_f32.hip, `lattice == 2`;
`PackedConv.out_lattice`): the conv whose only reader samples output pixels (2i, 2j) computes 25 of the 36
positions and writes those pixels alone, at their places in the full-size NHWC map.

Every config with an even-lattice build (`wino4s_lattice_ok`) on every shape, ReLU on and off, output prefilled
with NaN:
  (a) the pixels (2i, 2j) are bit-equal to the full launch of the same config;
  (b) every other pixel is still NaN;
  (c) the pixels (2i, 2j) are within 3e-5 of a float64 `F.conv2d`, relative to the largest of them (the family's
      bound, tests/test_wino4s_gpu.py);
  (d) a config without such a build, or a split-K launch, writes the whole correct map.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C_

pytestmark = pytest.mark.gpu

# single tile, odd maps, partial tile groups; the two ResNet-50 shapes at batch 2
SHAPES = [(1, 4, 4, 16, 32), (5, 5, 6, 16, 16), (3, 7, 7, 32, 64), (3, 13, 10, 32, 64), (2, 9, 17, 48, 64),
          (2, 14, 14, 256, 256), (2, 56, 56, 64, 64)]
PADS = ((1, 1), (1, 1))
BOUND = 3e-5


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Host data, the float64 oracle before the activation, and the conv packed without / with the lattice."""
    B, H, W, C, N = shape
    g = torch.Generator().manual_seed(B * 1000 + H * 31 + W)
    x = torch.randn((B, H, W, C), generator=g)
    k = torch.randn((3, 3, C, N), generator=g) / (3.0 * C ** 0.5)
    b = torch.randn(N, generator=g) * 0.1
    want = F.conv2d(x.double().permute(0, 3, 1, 2), k.double().permute(3, 2, 0, 1), b.double(), padding=1)
    want = want.permute(0, 2, 3, 1).contiguous()
    full = C_.pack_conv_f32(k.numpy(), b.numpy(), 1, PADS, "cuda")
    lat = C_.pack_conv_f32(k.numpy(), b.numpy(), 1, PADS, "cuda", out_lattice=2)
    assert full.out_lattice == 0 and lat.out_lattice == 2 and lat.wino4s is not None
    return x.cuda(), want, full, lat


def _launch(x, pc, cfg, relu, ks=1):
    out = torch.full(x.shape[:3] + (pc.cout,), float("nan"), device="cuda")
    ctr = torch.zeros(1 << 12, dtype=torch.int32, device="cuda") if ks < 0 else None
    C_.conv_forward_f32(x, pc, out, relu=relu, cfg=cfg, ksplit=ks, counters=ctr)
    torch.cuda.synchronize()
    return out.cpu()


def _lattice_cfgs(C, N):
    return [cfg for cfg in sorted(C_.WINO4S_F32_CFGS) if C_.kernels().wino4s_lattice_ok(cfg, C, N)]


def test_lattice_configs_are_whole_k_configs_of_the_family():
    k = C_.kernels()
    assert {221, 225, 238, 240, 241, 242} <= set(_lattice_cfgs(64, 64))
    for cfg in _lattice_cfgs(64, 64):
        assert cfg in C_.WINO4S_F32_CFGS and k.wino4s_ok(cfg, 64, 64, 1)
        assert not k.wino4s_lattice_ok(cfg, 24, 64) and not k.wino4s_lattice_ok(cfg, 64, 24)
    assert not k.wino4s_lattice_ok(220, 64, 64) and not k.wino4s_lattice_ok(244, 64, 64)
    assert not k.wino4s_lattice_ok(156, 64, 64)


@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("shape", SHAPES)
def test_sampled_pixels_bit_equal_the_full_launch_and_the_rest_is_untouched(shape, relu):
    B, H, W, C, N = shape
    x, want, full, lat = _case(shape)
    want = torch.relu(want) if relu else want
    ws = want[:, ::2, ::2]
    rest = torch.ones((H, W), dtype=torch.bool)
    rest[::2, ::2] = False
    ran = []
    for cfg in _lattice_cfgs(C, N):
        ref = _launch(x, full, cfg, relu)
        got = _launch(x, lat, cfg, relu)
        assert torch.isfinite(ref).all(), (cfg, "full launch")
        gs = got[:, ::2, ::2]
        assert torch.isfinite(gs).all(), (cfg, "sampled pixels not all written")
        assert torch.equal(gs, ref[:, ::2, ::2]), (cfg, "(a)", (gs - ref[:, ::2, ::2]).abs().max().item())
        assert torch.isnan(got[:, rest]).all(), (cfg, "(b)", int((~torch.isnan(got[:, rest])).sum()))
        rel = ((gs.double() - ws).abs().max() / ws.abs().max()).item()
        print(f"shape {shape} relu {relu} cfg {cfg}: rel err {rel:.3e}")
        assert rel < BOUND, (cfg, "(c)", rel)
        ran.append(cfg)
    assert ran, "no config has an even-lattice build for this shape"
    assert 225 in ran and 242 in ran                   # one wave along N: every N % 16 == 0
    if N % 32 == 0:
        assert 221 in ran and 238 in ran, ran          # whole K and row split


@pytest.mark.parametrize("shape", [(3, 7, 7, 32, 64), (3, 13, 10, 32, 64)])
def test_launches_without_a_lattice_build_write_the_whole_map(shape):
    B, H, W, C, N = shape
    x, want, full, lat = _case(shape)
    want = torch.relu(want)
    ran = 0
    for cfg, ks in [(220, 1), (222, 1), (227, 1), (233, 1), (239, 1), (244, 1), (246, 1), (221, 2), (221, -2),
                    (225, 2)]:
        assert C_.kernels().wino4s_ok(cfg, C, N, ks), (cfg, ks)
        assert ks != 1 or not C_.kernels().wino4s_lattice_ok(cfg, C, N)
        got = _launch(x, lat, cfg, 1, ks)
        assert torch.isfinite(got).all(), (cfg, ks, "pixels left unwritten")
        rel = ((got.double() - want).abs().max() / want.abs().max()).item()
        assert rel < BOUND, (cfg, ks, rel)
        assert torch.equal(got, _launch(x, full, cfg, 1, ks)), (cfg, ks)
        ran += 1
    assert ran == 10
