"""Guard-band runs of the fp32 path: every kernel family and config between 1 MiB guards (tests/guardband.py).

Each (family, config, split mode, shape) is launched twice, once with NaN and once with +inf in the guards of
everything it reads (activations, residuals, packed weights, biases, and the workspace, which is also written),
with outputs pre-filled with NaN and scratch of exactly the size the project's contract functions promise
(`f32_scratch`: workspace floats and arrival counters of the config and split launched; `dense_small_f32_scratch`,
`gap_scratch_elems`).  Asserted per launch:

1. every guard of every buffer handed to the launch is intact, bit for bit;
2. the outputs are finite and bit-identical between the two poison runs;
3. they match the float64 reference within the family's existing budget (2e-5; F(4x4) Winograd 3e-5);
4. stream-K / fused-split arrival counters are back to zero.

Shapes are the smallest at which a tail can go wrong: non-square maps, M below every tile, N not a tile
multiple, K not a multiple of 32, asymmetric ("same", stride 2) padding.  Where a launcher rejects such
a shape, the smallest one it accepts runs instead:

* F32S stream-K (cfgs 300 / 302, ksplit -1) needs >= 256 (tile, K chunk) units and <= 16 blocks per tile, so
  it runs on Cin = 256, N = 48, M = 23 x 151 = 3473 (31 tiles of 112 rows + one row); the whole-K launches use
  Cin = 64, N = 48, M = 15 / 113.
* The whole-row stem variants 2 / 5 / 6 fall back to variant 1 unless the conv row is 112 wide, so (1, 18, 224)
  joins (1, 64, 64) and (2, 40, 64).
* Tail config 125 needs two or more fragments per wave, which K = 512 does not give it, so it skips the
  (5, 30, 31, 512, 128) map: (1, 23, 23, 256, 2048, res) (M = 529, two tiles in the partial last round) is there
  for it.
* The pooling / depthwise asymmetric-pad case also runs on an even map (2, 12, 10, C), where the bottom / right
  padding is actually met (on 13 x 11 no 3x3 / s2 window reaches it).

Known limit (tests/guardband.py): an over-read whose value a select discards is invisible here.
"""
import types
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops._lib import kernels

import guardband as G
from test_fp32_gpu import _ref_conv

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)
F32 = torch.float32
RAN = set()              # config ids that ran guarded (test_every_config_ran_guarded)


def _pads(p):
    return ((p, p), (p, p)) if isinstance(p, int) else p


def _rd(a, poison, name):
    """A read-only operand (numpy array or tensor) between poisoned guards on the GPU."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return G.guarded(t.shape, t.dtype, "cuda", payload=t, poison=poison, name=name)


def _out(shape, name="out"):
    return G.guarded(shape, F32, "cuda", payload=float("nan"), name=name)


def _scratch(n, poison, name="workspace"):
    """fp32 scratch of exactly `n` elements: NaN payload, guards that poison reads and are checked for writes."""
    return G.guarded(n, F32, "cuda", payload=float("nan"), poison=poison, name=name) if n else None


def _counters(n):
    return G.guarded(n, torch.int32, "cuda", payload=0, name="counters") if n else None


def _rehome_pc(pc, poison):
    for f in ("w", "bias", "wino", "wino4s", "pwf"):
        t = getattr(pc, f, None)
        if t is not None:
            setattr(pc, f, G.rehome(t, poison=poison, name=f"pc.{f}"))
    return pc


def _pc_bufs(pc):
    return [t for t in (getattr(pc, f, None) for f in ("w", "bias", "wino", "wino4s", "pwf")) if t is not None]


def _rel1(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


def _rel_max(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def _verify(label, outs, wants, budget, rel=_rel1):
    """outs: {poison: [cpu tensors]}; wants: float64 arrays in the same order."""
    for i, want in enumerate(wants):
        a, b = outs[G.NAN][i], outs[G.INF][i]
        got = a.numpy().reshape(want.shape)
        assert np.isfinite(got).all(), f"{label}: output {i} not finite under NaN read-poison"
        assert np.isfinite(b.numpy()).all(), f"{label}: output {i} not finite under +inf read-poison"
        assert torch.equal(a, b), f"{label}: output {i} differs between the NaN and +inf poison runs"
        err = rel(got.astype(np.float64), want)
        assert err < budget, f"{label}: output {i} rel err {err:.3e} >= {budget}"


# ------------------------------------------------------------------ conv_forward_f32 families
def _conv_case(shape, n_split=0):
    """Host data, float64 reference and the guarded device operands (per poison) of one conv shape:
    (B, H, W, Cin, Cout, k, stride, pads, residual, act)."""
    B, H, W, Cin, Cout, k, s, pads, has_res, relu = shape
    pads = _pads(pads)
    rng = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    c = types.SimpleNamespace(shape=shape, B=B, H=H, W=W, Cin=Cin, Cout=Cout, relu=relu, n_split=n_split)
    c.x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    c.kern = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    c.bias = rng.standard_normal(Cout).astype(np.float32)
    (pt, pb), (pl, pr) = pads
    c.OH, c.OW = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
    c.M = B * c.OH * c.OW
    c.res = rng.standard_normal((B, c.OH, c.OW, Cout)).astype(np.float32) if has_res else None
    c.want = _ref_conv(c.x, c.kern, c.bias, s, pads, c.res, 0 if n_split else relu)
    c.dev = {}
    for poison in POISONS:
        pc = _rehome_pc(C.pack_conv_f32(c.kern, c.bias, s, pads, "cuda"), poison)
        pc.n_split = n_split
        assert pc.out_hw(H, W) == (c.OH, c.OW)
        c.dev[poison] = (_rd(c.x, poison, "x"), None if c.res is None else _rd(c.res, poison, "residual"), pc)
    c.Kpad = c.dev[G.NAN][2].Kpad
    return c


def _guarded_conv(c, cfg, ksplit, budget=2e-5, rel=_rel1, relu2=1):
    """One config / split mode on one case, under both poisons; the four assertions of the module docstring."""
    label = f"cfg {cfg} ksplit {ksplit} shape {c.shape}"
    outs = {}
    ns = c.n_split
    for poison in POISONS:
        x, res, pc = c.dev[poison]
        out = _out((c.B, c.OH, c.OW, ns or c.Cout))
        out2 = _out((c.B, c.OH, c.OW, c.Cout - ns), "out2") if ns else None
        nws, nctr = C.f32_scratch(cfg, ksplit, c.B, c.H, c.W, pc)
        ws, ctr = _scratch(nws, poison), _counters(nctr)
        for _rep in range(2 if ctr is not None else 1):      # the second launch meets the first one's counters
            C.conv_forward_f32(x, pc, out, res, relu=c.relu, cfg=cfg, ksplit=ksplit, workspace=ws, counters=ctr,
                               out2=out2, relu2=relu2)
        torch.cuda.synchronize()
        G.check(x, res, *_pc_bufs(pc), out, out2, ws, ctr, what=f"[{label}, {poison} poison]")
        if ctr is not None:
            assert int(ctr.abs().sum()) == 0, f"{label}: arrival counters not back to zero"
        outs[poison] = [out.cpu()] + ([out2.cpu()] if ns else [])
    if ns:
        w0 = c.want[..., :ns]
        w0 = np.maximum(w0, 0) if c.relu == 1 else w0
        w1 = c.want[..., ns:]
        w1 = np.maximum(w1, 0) if relu2 == 1 else w1
        wants = [w0, w1]
    else:
        wants = [c.want]
    _verify(label, outs, wants, budget, rel)
    RAN.add(cfg)


GEMM_SHAPES = [  # (B, H, W, Cin, Cout, k, stride, pads, residual, act)
    (2, 11, 9, 3, 64, 7, 2, 3, False, 1),                        # K = 147 -> Kpad 160, 3-channel gather
    (1, 5, 3, 32, 36, 1, 1, 0, True, 1),                         # M = 15: below every tile
    (1, 9, 12, 32, 48, 3, 2, ((0, 1), (0, 1)), False, 0),        # asymmetric "same" padding, H != W
    (3, 7, 5, 64, 96, 3, 1, 1, True, 2),                         # ReLU6, N not a tile multiple
    (2, 7, 9, 64, 128, 1, 2, 0, False, 0),                       # strided 1x1
]


# stream-K runs on the v2 configs only, and they need Cin % 32 == 0
@pytest.mark.parametrize("shape,ksplit", [(s, k) for s in GEMM_SHAPES for k in (1, 4, -1) if k > 0 or s[3] % 32 == 0])
def test_guard_conv_f32_tiles(shape, ksplit):
    """Every id in F32_TILES (v1 register-staged and v2 LDS-DMA); ksplit 4 split-K slabs, -1 stream-K (v2)."""
    c = _conv_case(shape)
    ran = 0
    for cfg in C.F32_TILES:
        if not C.f32_cfg_supported(cfg, c.Cin, c.Cout) or (ksplit < 0 and cfg not in C.F32G_CFGS):
            continue
        _guarded_conv(c, cfg, ksplit)
        ran += 1
    assert ran > 0


WINO_SHAPES = [  # (B, H, W, Cin, Cout, residual, act)
    (1, 5, 3, 16, 96, False, 1),
    (2, 9, 7, 32, 96, True, 2),
    (1, 4, 4, 48, 96, False, 0),
]


def _wino_case(shape):
    B, H, W, Cin, Cout, has_res, relu = shape
    return _conv_case((B, H, W, Cin, Cout, 3, 1, 1, has_res, relu))


def _wino_mode_ok(shape, ksplit):
    """Split-K within the 16-channel chunks; stream-K only where the v2 configs map (rows of >= 4 tiles)."""
    return abs(ksplit) <= shape[3] // 16 if ksplit > C.WINO_SK_BASE else (shape[2] + 1) // 2 >= 4


@pytest.mark.parametrize("shape,ksplit", [(s, k) for s in WINO_SHAPES for k in (1, 2, -2, -101) if _wino_mode_ok(s, k)])
def test_guard_wino_f32(shape, ksplit):
    """F(2x2, 3x3): whole K, split-K slabs, fused split-K, stream-K, gated as in test_wino_gpu.py."""
    c = _wino_case(shape)
    pc = c.dev[G.NAN][2]
    ran = 0
    for cfg in C.WINO_F32_CFGS:
        if cfg in C.WINO_MEASURE_CFGS:
            continue
        if not C.f32_cfg_supported(cfg, c.Cin, c.Cout, pc) or not C.wino_map_ok(cfg, c.H, c.W):
            continue
        if (ksplit <= C.WINO_SK_BASE) != (cfg in C.WINO_SK_CFGS):
            continue
        if cfg in C.WINO_PU_CFGS and ksplit != 1:
            continue
        if ksplit <= C.WINO_SK_BASE and not C.wino_sk_feasible(cfg, c.B, c.H, c.W, c.Cout, c.Cin, ksplit):
            continue
        _guarded_conv(c, cfg, ksplit)
        ran += 1
    assert ran > 0


WINO4S_SHAPES = [(1, 5, 6, 16, 64), (3, 7, 7, 32, 64), (1, 4, 4, 16, 64)]     # (B, H, W, Cin, Cout)


# a split must divide the 16-channel chunks
@pytest.mark.parametrize("shape,ksplit",
                         [(s, k) for s in WINO4S_SHAPES for k in (1, 2, -2) if (s[3] // 16) % abs(k) == 0])
def test_guard_wino4s_f32(shape, ksplit):
    """F(4x4, 3x3) transform + GEMM: V and the split slabs in exactly wino4s_ws_elems floats, wino4s_blocks
    counters (the existing test hands it 1 << 14)."""
    B, H, W, Cin, Cout = shape
    c = _conv_case((B, H, W, Cin, Cout, 3, 1, 1, False, 1))
    ran = 0
    for cfg in C.WINO4S_F32_CFGS:
        if not kernels().wino4s_ok(cfg, Cin, Cout, ksplit):
            continue
        _guarded_conv(c, cfg, ksplit, budget=3e-5, rel=_rel_max)
        ran += 1
    assert ran > 0


PW_SHAPES = [  # (B, H, W, K, N, residual, act)
    (1, 5, 3, 256, 512, False, 0),
    (1, 3, 5, 1024, 192, True, 0),
    (1, 3, 3, 64, 256, True, 1),
    (5, 30, 31, 512, 128, True, 0),          # a partial last tile round: tail config 126 (125 needs FPW >= 2)
    (1, 23, 23, 256, 2048, True, 1),         # ... and the smallest round map whose last round both 125 and 126 split
]


def _pw_ok(cfg, c, pc):
    if not C.f32_cfg_supported(cfg, c.Cin, c.Cout, pc):
        return False
    if cfg in C.PW_F32_TAIL:
        return bool(kernels().pw_f32_tail_plan(c.M, c.Cin, c.Cout, int(c.n_split), C.PW_F32_CFGS[cfg])[0])
    return True


@pytest.mark.parametrize("shape", PW_SHAPES)
def test_guard_pw_f32(shape):
    """Persistent / streaming pointwise configs (pw_f32.hip)."""
    B, H, W, K, N, has_res, relu = shape
    c = _conv_case((B, H, W, K, N, 1, 1, 0, has_res, relu))
    ran = 0
    for cfg in sorted(C.PW_F32_CFGS):
        if _pw_ok(cfg, c, c.dev[G.NAN][2]):
            _guarded_conv(c, cfg, 1)
            ran += 1
    assert ran > 0


def test_guard_pw_f32_strided_dual_output():
    """Merged sibling stride-2 1x1 convs: (B, H, K, N0, N1) = (1, 9, 256, 512, 128), two guarded outputs."""
    c = _conv_case((1, 9, 9, 256, 512 + 128, 1, 2, 0, False, 0), n_split=512)
    ran = 0
    for cfg in sorted(C.PW_F32_CFGS):
        if _pw_ok(cfg, c, c.dev[G.NAN][2]):
            _guarded_conv(c, cfg, 1)
            ran += 1
    assert ran > 0


def _f32s_sk_ok(cfg, c):
    """What gemm_f32s.hip asks of a stream-K launch (as test_gemm_f32s_gpu.py gates it)."""
    if cfg in C.F32S_TM:
        return False
    per = C.f32s_tiles(cfg, c.M, c.Cout) * (c.Cin // 32) // 256
    return per >= 1 and -(-(c.Cin // 32) // per) + 1 <= 16


F32S_CASES = [  # ((B, H, W, Cin, Cout, stride), ksplit): M = 15, 113 (one row past a 112-row tile); the stream-K shape
    ((1, 5, 3, 64, 48, 1), 1), ((1, 113, 1, 64, 48, 1), 1), ((1, 9, 5, 64, 48, 2), 1), ((1, 225, 1, 64, 48, 2), 1),
    ((1, 23, 151, 256, 48, 1), -1),
]


@pytest.mark.parametrize("shape,ksplit", F32S_CASES)
def test_guard_gemm_f32s(shape, ksplit):
    """Big-tile 1x1 GEMM: whole K per tile, and stream-K with exactly f32s_ws_elems / f32s_tiles scratch."""
    B, H, W, Cin, Cout, s = shape
    c = _conv_case((B, H, W, Cin, Cout, 1, s, 0, True, 1))
    assert c.M in (15, 113, 3473)
    ran = 0
    for cfg in sorted(C.F32S_CFGS):
        if not C.f32_cfg_supported(cfg, Cin, Cout, c.dev[G.NAN][2]) or (ksplit < 0 and not _f32s_sk_ok(cfg, c)):
            continue
        _guarded_conv(c, cfg, ksplit)
        ran += 1
    assert ran > 0


# ------------------------------------------------------------------ stem, pair
@pytest.mark.parametrize("variant", [0, 1, 2, 5, 6])
@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (2, 40, 64), (1, 18, 224)])
def test_guard_stem_f32(B, H, W, variant):
    rng = np.random.default_rng(H + W + B)
    x = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    kern = (rng.standard_normal((7, 7, 3, 64)) / np.sqrt(147)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(64)).astype(np.float32)
    pads = ((3, 3), (3, 3))
    conv = _ref_conv(x, kern, bias, 2, pads, None, 1)
    want = F.max_pool2d(F.pad(torch.from_numpy(conv).permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2)
    want = want.permute(0, 2, 3, 1).numpy()
    outs = {}
    for poison in POISONS:
        ps = C.pack_stem_f32(kern, bias, pads, "cuda")
        ps.w, ps.bias = G.rehome(ps.w, poison, "ps.w"), G.rehome(ps.bias, poison, "ps.bias")
        xd, out = _rd(x, poison, "x"), _out(want.shape)
        C.stem_f32_forward(xd, ps, out, variant=variant)
        torch.cuda.synchronize()
        G.check(xd, ps.w, ps.bias, out, what=f"[stem_f32 variant {variant}, {poison} poison]")
        outs[poison] = [out.cpu()]
    _verify(f"stem_f32 variant {variant} {(B, H, W)}", outs, [want], 2e-5)


@pytest.mark.parametrize("bm", C.PAIR_F32_BM)
@pytest.mark.parametrize("B,H,W", [(1, 5, 3), (2, 7, 7)])
def test_guard_pair_f32(bm, B, H, W):
    rng = np.random.default_rng(B * 100 + H + bm)
    x = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    res = rng.standard_normal((B, H, W, 256)).astype(np.float32)
    k3 = (rng.standard_normal((1, 1, 64, 256)) / 8).astype(np.float32)
    b3 = rng.standard_normal(256).astype(np.float32) * 0.1
    k1 = (rng.standard_normal((1, 1, 256, 64)) / 16).astype(np.float32)
    b1 = rng.standard_normal(64).astype(np.float32) * 0.1
    yw = np.maximum(x.astype(np.float64) @ k3[0, 0].astype(np.float64) + b3 + res, 0)
    zw = np.maximum(yw @ k1[0, 0].astype(np.float64) + b1, 0)
    outs = {}
    for poison in POISONS:
        pp = C.pack_pair_f32(k3, b3, k1, b1, "cuda")
        for f in ("w3", "b3", "w1", "b1"):
            setattr(pp, f, G.rehome(getattr(pp, f), poison, f"pp.{f}"))
        xd, rd = _rd(x, poison, "x"), _rd(res, poison, "residual")
        y, z = _out((B, H, W, 256), "y"), _out((B, H, W, 64), "z")
        C.pair_f32_forward(xd, rd, pp, y, z, bm=bm)
        torch.cuda.synchronize()
        G.check(xd, rd, pp.w3, pp.b3, pp.w1, pp.b1, y, z, what=f"[pair_f32 bm {bm}, {poison} poison]")
        outs[poison] = [y.cpu(), z.cpu()]
    _verify(f"pair_f32 bm {bm} {(B, H, W)}", outs, [yw, zw], 2e-5)


# ------------------------------------------------------------------ head
@pytest.mark.parametrize("M,K,N", [(1, 96, 130), (5, 1280, 1000), (17, 4096, 10)])
def test_guard_dense_small_f32(M, K, N):
    rng = np.random.default_rng(M * 7 + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    want = x.astype(np.float64) @ w.astype(np.float64) + b
    e = np.exp(want - want.max(1, keepdims=True))
    sm = e / e.sum(1, keepdims=True)
    outs = {}
    for poison in POISONS:
        pc = _rehome_pc(C.pack_conv_f32(w.reshape(1, 1, K, N), b, 1, ((0, 0), (0, 0)), "cuda"), poison)
        xd = _rd(x, poison, "x")
        part = _scratch(E.dense_small_f32_scratch(M, N, pc.Kpad), poison, "part")
        logits, probs = _out((M, N), "logits"), _out((M, N), "probs")
        E.dense_small_f32(xd, pc, part, logits=logits, probs=probs)
        torch.cuda.synchronize()
        G.check(xd, *_pc_bufs(pc), part, logits, probs, what=f"[dense_small_f32 {(M, K, N)}, {poison} poison]")
        outs[poison] = [logits.cpu(), probs.cpu()]
    _verify(f"dense_small_f32 {(M, K, N)}", outs, [want], 2e-5, _rel_max)
    assert torch.equal(outs[G.NAN][1], outs[G.INF][1])
    assert np.abs(outs[G.NAN][1].numpy() - sm).max() < 1e-5


@pytest.mark.parametrize("shape", [(2, 7, 7, 36), (1, 33, 40, 36)])
def test_guard_gap_f32(shape):
    """One-pass GAP, and the sliced two-pass kernel (>= GAP_LARGE_HW pixels) with exactly gap_scratch_elems."""
    B, H, W, Cc = shape
    x = torch.from_numpy(np.random.default_rng(4).standard_normal(shape).astype(np.float32))
    want = x.double().mean(dim=(1, 2)).numpy()
    need = E.gap_scratch_elems(B, H * W, Cc)
    assert (need > 0) == (H * W >= E.GAP_LARGE_HW)
    outs = {}
    for poison in POISONS:
        xd, g, sc = _rd(x, poison, "x"), _out((B, Cc)), _scratch(need, poison, "scratch")
        E.gap_f32(xd, g, scratch=sc)
        torch.cuda.synchronize()
        G.check(xd, g, sc, what=f"[gap_f32 {shape}, {poison} poison]")
        outs[poison] = [g.cpu()]
    _verify(f"gap_f32 {shape}", outs, [want], 1e-5)
    assert np.allclose(outs[G.NAN][0].double().numpy(), want, rtol=1e-5, atol=1e-6)      # test_fp32_gpu.py's bound


# ------------------------------------------------------------------ fp32 layers (conv_f32.hip)
def _run_layer(label, reads, out_shapes, launch, check):
    """reads: {name: cpu tensor}; launch(dev reads, outs); check(list of cpu outputs) asserts against the
    oracle.  Guards, finiteness and bit-identity across the two poisons are asserted here."""
    outs = {}
    for poison in POISONS:
        dev = {k: _rd(v, poison, k) for k, v in reads.items()}
        o = [_out(s, f"out{i}") for i, s in enumerate(out_shapes)]
        launch(dev, o)
        torch.cuda.synchronize()
        G.check(*dev.values(), *o, what=f"[{label}, {poison} poison]")
        outs[poison] = [t.cpu() for t in o]
    for a, b in zip(outs[G.NAN], outs[G.INF]):
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), f"{label}: non-finite output"
        assert torch.equal(a, b), f"{label}: outputs differ between the NaN and +inf poison runs"
    check(outs[G.NAN])


LAYER_MAPS = [  # (H, W, k, stride, pads)
    (13, 11, 3, 1, ((1, 1), (1, 1))), (13, 11, 5, 2, ((2, 2), (2, 2))), (13, 11, 2, 1, ((1, 1), (1, 1))),
    (13, 11, 3, 2, ((0, 1), (0, 1))), (12, 10, 3, 2, ((0, 1), (0, 1))),
]


@pytest.mark.parametrize("Cc", [8, 6])             # 4-channel vector kernels / scalar fallback
@pytest.mark.parametrize("H,W,k,stride,pads", LAYER_MAPS)
def test_guard_f32_dwconv_avgpool(Cc, H, W, k, stride, pads):
    rng = np.random.default_rng(7 + k)
    x = torch.from_numpy(rng.standard_normal((2, H, W, Cc)).astype(np.float32))
    w = torch.from_numpy(rng.standard_normal((k, k, Cc)).astype(np.float32))
    bias = torch.from_numpy(rng.standard_normal(Cc).astype(np.float32))
    (pt, pb), (pl, pr) = pads
    OH, OW = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
    xt = F.pad(x.permute(0, 3, 1, 2).double(), (pl, pr, pt, pb))
    conv = F.conv2d(xt, w.double().permute(2, 0, 1).unsqueeze(1), bias.double(), stride=stride, groups=Cc)
    for act, fn in ((1, lambda t: t.clamp_min(0)), (3, lambda t: t * torch.sigmoid(t))):
        want = fn(conv).permute(0, 2, 3, 1)
        _run_layer(f"dwconv_f32 C {Cc} k {k} s {stride} act {act}", {"x": x, "w": w, "bias": bias},
                   [(2, OH, OW, Cc)],
                   lambda d, o: E.dwconv_f32(d["x"], d["w"], d["bias"], o[0], stride, pads, act=act),
                   lambda got: torch.testing.assert_close(got[0].double(), want, rtol=1e-5, atol=1e-5))
    ones = F.pad(torch.ones((1, 1, H, W), dtype=torch.float64), (pl, pr, pt, pb))
    want = (F.avg_pool2d(xt, k, stride) / F.avg_pool2d(ones, k, stride)).permute(0, 2, 3, 1)     # padding not counted
    _run_layer(f"avgpool_f32 C {Cc} k {k} s {stride}", {"x": x}, [(2, OH, OW, Cc)],
               lambda d, o: E.avgpool_f32(d["x"], o[0], k, stride, pads),
               lambda got: torch.testing.assert_close(got[0].double(), want, rtol=1e-5, atol=1e-6))


@pytest.mark.parametrize("Cc", [8, 4])
@pytest.mark.parametrize("H,W,k,stride,pads", LAYER_MAPS)
def test_guard_f32_maxpool(Cc, H, W, k, stride, pads):
    """+inf in the guards is what shows a max-pool over-read (max drops NaN)."""
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, H, W, Cc)).astype(np.float32))
    (pt, pb), (pl, pr) = pads
    OH, OW = (H + pt + pb - k) // stride + 1, (W + pl + pr - k) // stride + 1
    for pad_zero, value in ((False, float("-inf")), (True, 0.0)):
        want = F.max_pool2d(F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb), value=value), k, stride).permute(0, 2, 3, 1)
        _run_layer(f"maxpool_f32 C {Cc} k {k} s {stride} pad_zero {pad_zero}", {"x": x}, [(2, OH, OW, Cc)],
                   lambda d, o: E.maxpool_f32(d["x"], o[0], k, stride, pt, pl, pad_zero=pad_zero),
                   lambda got: torch.testing.assert_close(got[0], want.contiguous(), rtol=0, atol=0))


@pytest.mark.parametrize("Cc", [8, 6])
def test_guard_f32_elementwise_layers(Cc):
    """concat_f32, binary_f32 (full and per-image broadcast), affine_act_f32, eltwise_f32 (C % 4 == 0), pad_f32."""
    rng = np.random.default_rng(11)
    shape = (2, 13, 11, Cc)
    a = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    se = torch.from_numpy(rng.standard_normal((2, Cc)).astype(np.float32))
    sc = torch.rand(Cc, generator=torch.Generator().manual_seed(1))
    sh = torch.rand(Cc, generator=torch.Generator().manual_seed(2))
    close = torch.testing.assert_close
    _run_layer("binary_f32 mul bcast", {"a": a, "b": se}, [shape],
               lambda d, o: E.binary_f32(d["a"], d["b"], o[0], "mul"),
               lambda got: close(got[0], a * se[:, None, None, :], rtol=1e-6, atol=1e-6))
    _run_layer("binary_f32 add", {"a": a, "b": b}, [shape],
               lambda d, o: E.binary_f32(d["a"], d["b"], o[0], "add", act_mode=1),
               lambda got: close(got[0], (a + b).clamp_min(0), rtol=1e-6, atol=1e-6))
    t = a.double() * sc.double() + sh.double()
    _run_layer("affine_act_f32 swish", {"x": a, "scale": sc, "shift": sh}, [shape],
               lambda d, o: E.affine_act_f32(d["x"], o[0], d["scale"], d["shift"], act=3),
               lambda got: close(got[0].double(), t * torch.sigmoid(t), rtol=1e-5, atol=1e-5))
    _run_layer("concat_f32", {"a": a, "b": b}, [(2, 13, 11, 2 * Cc)],
               lambda d, o: E.concat_f32([d["a"], d["b"]], o[0]),
               lambda got: close(got[0], torch.cat([a, b], dim=-1), rtol=0, atol=0))
    want = F.pad(a.permute(0, 3, 1, 2), (2, 1, 1, 2)).permute(0, 2, 3, 1).contiguous()
    _run_layer("pad_f32", {"x": a}, [(2, 16, 14, Cc)],
               lambda d, o: E.pad_f32(d["x"], o[0], 1, 2),
               lambda got: close(got[0], want, rtol=0, atol=0))
    if Cc % 4 == 0:
        _run_layer("eltwise_f32 add relu", {"a": a, "b": b}, [shape],
                   lambda d, o: E.eltwise_f32(d["a"], o[0], b=d["b"], relu=1),
                   lambda got: close(got[0], (a + b).clamp_min(0), rtol=1e-6, atol=1e-6))
        _run_layer("eltwise_f32 affine", {"a": a, "scale": sc, "shift": sh}, [shape],
                   lambda d, o: E.eltwise_f32(d["a"], o[0], scale=d["scale"], shift=d["shift"]),
                   lambda got: close(got[0], a * sc + sh, rtol=1e-6, atol=1e-6))


# ------------------------------------------------------------------ coverage
def test_every_config_ran_guarded():
    """Skipping must not hide a config: every non-measurement id of every fp32 config table ran guarded on at
    least one shape above (this test runs last in the file)."""
    tables = {
        "F32_TILES": set(C.F32_TILES),
        "WINO_F32_CFGS": set(C.WINO_F32_CFGS) - set(C.WINO_MEASURE_CFGS),
        "WINO4S_F32_CFGS": set(C.WINO4S_F32_CFGS),
        "PW_F32_CFGS": set(C.PW_F32_CFGS),
        "F32S_CFGS": set(C.F32S_CFGS),
    }
    missing = {name: sorted(ids - RAN) for name, ids in tables.items() if ids - RAN}
    assert not missing, f"configs that never ran guarded: {missing}"
