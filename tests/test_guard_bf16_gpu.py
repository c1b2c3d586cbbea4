"""Guard-band runs of the bf16 path: every kernel family and config between 1 MiB guards (tests/guardband.py).

Same harness and the same four assertions as tests/test_guard_f32_gpu.py: each launch runs once with NaN and once
with +inf in the guards of everything it reads (uint8 inputs: 0xFF bytes), outputs pre-filled with NaN, scratch of
exactly `bf16_scratch` (workspace floats, `sk_plan` tile counters) / `dense_small_scratch` / `gap_scratch_elems`; all guards intact,
outputs finite and bit-identical between the two runs, stream-K counters back to zero, and the result within the
family's existing budget of a float64 reference computed from the bf16-rounded inputs and weights.

Per family: the smallest shape of its existing test file plus a ragged one (B = 1, odd H != W, N at the smallest
multiple the family takes).  rr3 / cs3 / the fused bottleneck, pair and pointwise kernels only exist for fixed
channel counts (and rr3 / cs3 for fixed maps), so only their pixel count is ragged.

Known limit (tests/guardband.py): an over-read whose value a select discards is invisible here.
"""
import math
import types
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E

import guardband as G

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)
BF16, F32 = torch.bfloat16, torch.float32
RAN = set()              # config ids that ran guarded (test_every_config_ran_guarded)


def _rd(t, poison, name):
    """A read-only operand (CPU tensor) between poisoned guards on the GPU (integer data: 0xFF bytes)."""
    t = torch.from_numpy(np.ascontiguousarray(t)) if isinstance(t, np.ndarray) else t
    return G.guarded(t.shape, t.dtype, "cuda", payload=t, poison=poison if t.dtype.is_floating_point else 0xFF,
                     name=name)


def _out(shape, dtype=BF16, name="out"):
    return G.guarded(shape, dtype, "cuda", payload=float("nan"), name=name)


def _scratch(n, poison, name="workspace"):
    return G.guarded(n, F32, "cuda", payload=float("nan"), poison=poison, name=name) if n else None


def _bf(a):
    """numpy / tensor -> CPU bf16 tensor (the rounding the kernels' inputs carry)."""
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
    return t.to(BF16)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _rehome_fields(obj, fields, poison):
    bufs = []
    for f in fields:
        t = getattr(obj, f, None)
        if t is not None:
            setattr(obj, f, G.rehome(t, poison=poison, name=f"{type(obj).__name__}.{f}"))
            bufs.append(getattr(obj, f))
    return bufs


def _run(label, reads, out_specs, launch, check):
    """reads: {name: CPU tensor}; out_specs: [(shape, dtype)]; launch(dev reads, outs, poison) -> extra guarded
    buffers it used (weights, scratch, counters); check(list of CPU outputs) compares with the oracle.  Guards,
    counters, finiteness and bit-identity across the two poisons are asserted here."""
    got = {}
    for poison in POISONS:
        dev = {k: _rd(v, poison, k) for k, v in reads.items()}
        outs = [_out(s, d, f"out{i}") for i, (s, d) in enumerate(out_specs)]
        extra = launch(dev, outs, poison)
        extra = extra if isinstance(extra, list) else []        # (the wrappers themselves return their output)
        torch.cuda.synchronize()
        G.check(*dev.values(), *outs, *extra, what=f"[{label}, {poison} poison]")
        for t in extra:
            if t is not None and t.dtype == torch.int32:
                assert int(t.abs().sum()) == 0, f"{label}: stream-K counters not back to zero"
        got[poison] = [t.cpu() for t in outs]
    for i, (a, b) in enumerate(zip(got[G.NAN], got[G.INF])):
        assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all(), f"{label}: output {i} not finite"
        assert torch.equal(a, b), f"{label}: output {i} differs between the NaN and +inf poison runs"
    check(got[G.NAN])


def _close(got, want, rel, abs_, label):
    """The conv families' budget: max |got - want| <= rel x max |want| + abs."""
    err = (got.double() - want).abs().max().item()
    lim = rel * want.abs().max().item() + abs_
    assert err <= lim, f"{label}: max err {err:.4g} > {lim:.4g}"


# ------------------------------------------------------------------ conv_forward, every id in CFG_TILES
def _ref_conv64(x, kern, bias, stride, pads, res=None, relu=0):
    """float64 CPU conv of bf16-rounded NHWC x / HWIO weights (+ fp32 bias, bf16 residual, activation)."""
    (pt, pb), (pl, pr) = pads
    xt = F.pad(x.double().permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xt, _bf(kern).double().permute(3, 2, 0, 1), torch.from_numpy(bias).double(), stride=stride)
    y = y.permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0) if relu == 1 else y.clamp(0, 6) if relu == 2 else y


def _conv_case(shape, n_split=0):
    """(B, H, W, Cin, Cout, k, stride, pads, residual, act): host data, reference, guarded operands per poison."""
    B, H, W, Cin, Cout, k, s, pads, has_res, relu = shape
    pads = ((pads, pads), (pads, pads)) if isinstance(pads, int) else pads
    rng = _rng(shape)
    c = types.SimpleNamespace(shape=shape, B=B, H=H, W=W, Cin=Cin, Cout=Cout, relu=relu, n_split=n_split, k=k, s=s)
    c.x = _bf(rng.standard_normal((B, H, W, Cin)).astype(np.float32))
    c.kern = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    c.bias = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    (pt, pb), (pl, pr) = pads
    c.OH, c.OW = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
    c.M = B * c.OH * c.OW
    c.res = _bf(rng.standard_normal((B, c.OH, c.OW, Cout)).astype(np.float32)) if has_res else None
    c.want = _ref_conv64(c.x, c.kern, c.bias, s, pads, c.res, 0 if n_split else relu)
    c.pc, c.pcbufs = {}, {}
    for poison in POISONS:
        pc = C.pack_conv(c.kern, c.bias, s, pads, "cuda")
        c.pcbufs[poison] = _rehome_fields(pc, ("w", "bias"), poison)
        pc.n_split = n_split
        c.pc[poison] = pc
    c.Kpad = c.pc[G.NAN].Kpad
    c.pure = k == 1 and s == 1 and pads == ((0, 0), (0, 0))
    return c


def _guarded_conv(c, cfg, ksplit, relu2=1):
    label = f"cfg {cfg} ksplit {ksplit} shape {c.shape}"
    ns = c.n_split
    reads = {"x": c.x}
    if c.res is not None:
        reads["residual"] = c.res
    specs = [((c.B, c.OH, c.OW, ns or c.Cout), BF16)] + ([((c.B, c.OH, c.OW, c.Cout - ns), BF16)] if ns else [])

    def launch(dev, outs, poison):
        nws, nctr = C.bf16_scratch(cfg, ksplit, c.B, c.H, c.W, c.pc[poison])
        ws = _scratch(nws, poison)
        ctr = None
        if ksplit < 0:
            ctr = G.guarded(nctr, torch.int32, "cuda", payload=0, name="counters")
        for _rep in range(2 if ctr is not None else 1):      # the second launch meets the first one's counters
            C.conv_forward(dev["x"], c.pc[poison], outs[0], dev.get("residual"), relu=c.relu, cfg=cfg, ksplit=ksplit,
                           workspace=ws, counters=ctr, out2=outs[1] if ns else None, relu2=relu2)
        return c.pcbufs[poison] + [ws, ctr]

    def check(got):
        if ns:
            _close(got[0], c.want[..., :ns], 2e-2, 1e-2, label + " out")
            w1 = c.want[..., ns:]
            _close(got[1], w1.clamp_min(0) if relu2 else w1, 2e-2, 1e-2, label + " out2")
        else:
            _close(got[0], c.want, 2e-2, 1e-2, label)

    _run(label, reads, specs, launch, check)
    RAN.add(cfg)


def _conv_ok(c, cfg, ksplit):
    pc = c.pc[G.NAN]
    if not C.cfg_supported(cfg, pc, c.pure):
        return False
    halo = cfg in C.HALO_PATCH
    if halo and (ksplit != 1 or C.halo_rows(cfg, pc, c.H, c.W) < 1):
        return False
    if ksplit < 0 and cfg in C.V1_CFGS:
        return False
    if ksplit > 1 and c.Kpad // C.BK < 4:         # as test_kernels_gpu.py: split only K of 4+ tiles
        return False
    return True


CONV_SHAPES = [  # (B, H, W, Cin, Cout, k, stride, pads, residual, act)
    (3, 9, 11, 24, 40, 3, 2, 1, True, 1),                        # the smallest of test_kernels_gpu.py (v1 only)
    (1, 7, 5, 64, 40, 3, 1, 1, True, 1),                         # ragged; 3x3 / s1 / p1: the halo configs too
    (1, 5, 3, 64, 72, 1, 1, 0, False, 2),                        # pure 1x1 GEMM path, M = 15, ReLU6
    (2, 9, 12, 64, 48, 3, 2, ((0, 1), (0, 1)), False, 0),        # asymmetric "same" padding
]


def _mode_ok(shape, ksplit):
    """Stream-K is a v2 mode (Cin % 64 == 0); split-K only for K of 4+ tiles (as test_kernels_gpu.py)."""
    ktiles = -(-shape[5] ** 2 * shape[3] // C.BK)
    return ksplit == 1 or (shape[3] % 64 == 0 if ksplit < 0 else ktiles >= 4)


@pytest.mark.parametrize("shape,ksplit", [(s, k) for s in CONV_SHAPES for k in (1, 2, -1) if _mode_ok(s, k)])
def test_guard_conv_bf16_tiles(shape, ksplit):
    """Every id in CFG_TILES (v1, the LDS-DMA v2 families incl. 62-70, the halo kernel); ksplit 2: split-K
    slabs; -1: stream-K with exactly the `bf16_scratch` floats and `sk_plan` tile counters."""
    c = _conv_case(shape)
    ran = 0
    for cfg in sorted(C.CFG_TILES):
        if _conv_ok(c, cfg, ksplit):
            _guarded_conv(c, cfg, ksplit)
            ran += 1
    assert ran > 0


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("ksplit", [1, -1])
def test_guard_conv_bf16_dual_output(stride, ksplit):
    """Sibling 1x1 convs packed along N: columns [0, 256) -> out, the rest -> out2 (ReLU), two guarded outputs."""
    c = _conv_case((1, 9, 11, 64, 256 + 64, 1, stride, 0, False, 0), n_split=256)
    ran = 0
    for cfg in sorted(C.CFG_TILES):
        if cfg not in C.HALO_PATCH and _conv_ok(c, cfg, ksplit):
            _guarded_conv(c, cfg, ksplit)
            ran += 1
    assert ran > 0


# ------------------------------------------------------------------ pointwise / register-resident families
def _pw_case(M, K, N, has_res, relu):
    rng = _rng(M, K, N)
    kern = (rng.standard_normal((1, 1, K, N)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    x = _bf(rng.standard_normal((M, K)).astype(np.float32))
    r = _bf(rng.standard_normal((M, N)).astype(np.float32)) if has_res else None
    want = x.double() @ _bf(kern[0, 0]).double() + torch.from_numpy(bias).double()
    if r is not None:
        want = want + r.double()
    if relu:
        want = want.clamp_min(0)
    pcs = {}
    for poison in POISONS:
        pc = C.pack_conv(kern, bias, 1, ((0, 0), (0, 0)), "cuda")
        bufs = _rehome_fields(pc, ("w", "bias"), poison)
        pc._pw_frag = G.rehome(C.pw_fragments(pc), poison=poison, name="pw fragments")
        pcs[poison] = (pc, bufs + [pc._pw_frag])
    return x, r, want, pcs


def _guarded_pw(fwd, cfg, M, K, N, has_res, relu, blocks, case):
    x, r, want, pcs = case
    label = f"{fwd.__name__} cfg {cfg} M {M} K {K} N {N} blocks {blocks}"
    reads = {"x": x, **({"residual": r} if r is not None else {})}

    def launch(dev, outs, poison):
        pc, bufs = pcs[poison]
        fwd(dev["x"], pc, outs[0], dev.get("residual"), relu=relu, cfg=cfg, blocks=blocks)
        return bufs

    def check(got):
        err = (got[0].double() - want).abs().max().item() / want.abs().max().item()
        assert err < 1e-2, f"{label}: rel err {err}"

    _run(label, reads, [((M, N), BF16)], launch, check)
    RAN.add(cfg)


@pytest.mark.parametrize("K,N,M", [(64, 256, 777), (128, 512, 15), (64, 256, 15)])
def test_guard_pw_wide(K, N, M):
    """pw_wide.hip (cfgs 60 / 61): M = 15 is below both tile sizes."""
    for has_res, relu in ((True, 1), (False, 0)):
        case = _pw_case(M, K, N, has_res, relu)
        assert C.pw_supported(case[3][G.NAN][0])
        for cfg in sorted(C.PW_CFGS):
            _guarded_pw(C.pw_forward, cfg, M, K, N, has_res, relu, 64, case)


@pytest.mark.parametrize("M,K,N,has_res", [(100, 1024, 128, False), (777, 256, 512, True), (15, 128, 512, True),
                                           (15, 512, 128, False), (15, 256, 1024, True)])
def test_guard_pw_slice(M, K, N, has_res):
    """pw_slice.hip (cfgs 74-79) on the grids the tuner uses (1 and 2 blocks per CU)."""
    case = _pw_case(M, K, N, has_res, 1)
    ran = 0
    for cfg in sorted(C.PS_CFGS):
        if not C.ps_supported(case[3][G.NAN][0], cfg):
            continue
        for blocks in (C.NUM_CUS, 2 * C.NUM_CUS):
            _guarded_pw(C.ps_forward, cfg, M, K, N, has_res, 1, blocks, case)
        ran += 1
    assert ran > 0


@pytest.mark.parametrize("cfg,H,W,Cc", [(71, 28, 28, 128), (72, 28, 28, 128), (73, 14, 14, 256), (73, 7, 7, 512)])
def test_guard_rr3_cs3(cfg, H, W, Cc):
    """The register-resident 3x3 kernels on their fixed maps at B = 1 (conv3x3_rr.hip, conv3x3_cs.hip)."""
    c = _conv_case((1, H, W, Cc, Cc, 3, 1, 1, False, 1))
    for poison in POISONS:
        pc = c.pc[poison]
        pc._pw_frag = G.rehome(C.pw_fragments(pc), poison=poison, name="filter fragments")
        c.pcbufs[poison] = c.pcbufs[poison] + [pc._pw_frag]
    assert C.cfg_supported(cfg, c.pc[G.NAN], False)
    label = f"cfg {cfg} {(1, H, W, Cc)}"

    def launch(dev, outs, poison):
        C.conv_forward(dev["x"], c.pc[poison], outs[0], relu=True, cfg=cfg)
        return c.pcbufs[poison]

    _run(label, {"x": c.x}, [((1, H, W, Cc), BF16)], launch, lambda got: _close(got[0], c.want, 1e-2, 1e-2, label))
    RAN.add(cfg)


# ------------------------------------------------------------------ fused bottleneck, pair, stem
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("B,H,W", [(2, 8, 8), (1, 8, 24)])
def test_guard_bottleneck(proj, B, H, W):
    rng = _rng("bottleneck", proj, H, W)
    cin = 64 if proj else 256

    def w(*s):
        return (rng.standard_normal(s) / np.sqrt(np.prod(s[:3]))).astype(np.float32)
    k1, k2, k3 = w(1, 1, cin, 64), w(3, 3, 64, 64), w(1, 1, 64, 256)
    b1, b2, b3 = (rng.standard_normal(n).astype(np.float32) * 0.1 for n in (64, 64, 256))
    kp, bp = (w(1, 1, 64, 256), rng.standard_normal(256).astype(np.float32) * 0.1) if proj else (None, None)
    x = _bf(rng.standard_normal((B, H, W, cin)).astype(np.float32))
    p0, p1 = ((0, 0), (0, 0)), ((1, 1), (1, 1))
    y1 = _ref_conv64(x, k1, b1, 1, p0, None, 1).to(BF16)              # intermediates rounded like the kernel's
    y2 = _ref_conv64(y1, k2, b2, 1, p1, None, 1).to(BF16)
    sc = x.double() if kp is None else _ref_conv64(x, kp, bp, 1, p0)
    want = (_ref_conv64(y2, k3, b3, 1, p0) + sc).clamp_min(0)
    label = f"bottleneck proj {proj} {(B, H, W)}"

    def launch(dev, outs, poison):
        pb = C.pack_bottleneck(k1, b1, k2, b2, k3, b3, kp, bp)
        bufs = _rehome_fields(pb, ("w1", "w2", "w3", "b1", "b2", "b3"), poison)
        C.bottleneck_forward(dev["x"], pb, outs[0])
        return bufs

    def check(got):
        err = (got[0].double() - want).abs().max().item() / max(1.0, want.abs().max().item())
        assert err < 1.5e-2, f"{label}: rel err {err}"

    _run(label, {"x": x}, [((B, H, W, 256), BF16)], launch, check)


@pytest.mark.parametrize("cin,co,cm,bm", sorted(C.PAIR_CFGS))
@pytest.mark.parametrize("M", [17, 35])
def test_guard_pair(cin, co, cm, bm, M):
    rng = _rng("pair", cin, M)
    k3 = (rng.standard_normal((1, 1, cin, co)) / cin ** 0.5).astype(np.float32)
    k1 = (rng.standard_normal((1, 1, co, cm)) / co ** 0.5).astype(np.float32)
    b3, b1 = (0.1 * rng.standard_normal(co)).astype(np.float32), (0.1 * rng.standard_normal(cm)).astype(np.float32)
    x = _bf(rng.standard_normal((M, cin)).astype(np.float32))
    res = _bf(rng.standard_normal((M, co)).astype(np.float32))
    y_ref = (x.double() @ _bf(k3[0, 0]).double() + torch.from_numpy(b3).double() + res.double()).clamp_min(0)
    label = f"pair {(cin, co, cm, bm)} M {M}"

    def launch(dev, outs, poison):
        pp = C.pack_pair(k3, b3, k1, b1, device="cuda")
        bufs = _rehome_fields(pp, ("w3", "b3", "w1", "b1"), poison)
        C.pair_forward(dev["x"], dev["res"], pp, outs[0], outs[1], bm=bm)
        return bufs

    def check(got):
        _close(got[0], y_ref, 2e-2, 1e-2, label + " y")
        # z from the kernel's own (bf16-rounded) y: the second GEMM's numerics alone
        z_ref = (got[0].double() @ _bf(k1[0, 0]).double() + torch.from_numpy(b1).double()).clamp_min(0)
        _close(got[1], z_ref, 2e-2, 1e-2, label + " z")

    _run(label, {"x": x, "res": res}, [((M, co), BF16), ((M, cm), BF16)], launch, check)


@pytest.mark.parametrize("B,H,W,pool", [(2, 37, 29, True), (1, 21, 30, False), (1, 13, 19, True)])
@pytest.mark.parametrize("version", ["v1", "v2", "v3", "v4", "v6"])
def test_guard_stem(B, H, W, pool, version, monkeypatch):
    monkeypatch.setenv("ADAPT_STEM_V1", {"v1": "1", "v2": "0", "v3": "3", "v4": "4", "v6": "6"}[version])
    rng = _rng("stem", B, H, W)
    x = torch.from_numpy((rng.standard_normal((B, H, W, 3)) * 40.0).astype(np.float32))      # caffe pixel scale
    kern = (rng.standard_normal((7, 7, 3, 64)) / math.sqrt(147) / 40.0).astype(np.float32)
    bias = (0.1 * rng.standard_normal(64)).astype(np.float32)
    pads = ((3, 3), (3, 3))
    want = _ref_conv64(_bf(x), kern, bias, 2, pads, None, 1)         # the kernel stages the image as bf16
    if pool:
        want = F.max_pool2d(F.pad(want.permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, 2).permute(0, 2, 3, 1)
    label = f"stem {version} {(B, H, W)} pool {pool}"

    def launch(dev, outs, poison):
        ps = C.pack_stem(kern, bias, pads, "cuda")
        bufs = _rehome_fields(ps, ("w", "bias"), poison)
        C.stem_forward(dev["x"], ps, outs[0], pool=pool)
        return bufs

    _run(label, {"x": x}, [(tuple(want.shape), BF16)], launch, lambda got: _close(got[0], want, 2e-2, 1e-2, label))


# ------------------------------------------------------------------ head and layers
@pytest.mark.parametrize("M,K,N", [(7, 512, 10), (20, 1000, 37), (1, 96, 130)])
def test_guard_dense_small(M, K, N):
    rng = _rng("dense", M, K, N)
    x = _bf(rng.standard_normal((M, K)).astype(np.float32))
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    want = x.double() @ _bf(w).double() + torch.from_numpy(b).double()
    label = f"dense_small {(M, K, N)}"

    def launch(dev, outs, poison):
        pc = C.pack_conv(w.reshape(1, 1, K, N), b, 1, ((0, 0), (0, 0)), "cuda")
        bufs = _rehome_fields(pc, ("w", "bias"), poison)
        part = _scratch(E.dense_small_scratch(M, N, K), poison, "part")
        E.dense_small(dev["x"], pc, part, logits=outs[0], probs=outs[1])
        return bufs + [part]

    def check(got):
        torch.testing.assert_close(got[0].double(), want, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(got[1].double(), torch.softmax(want, -1), atol=1e-3, rtol=2e-2)

    _run(label, {"x": x}, [((M, N), F32), ((M, N), F32)], launch, check)


@pytest.mark.parametrize("shape", [(3, 5, 9, 64), (2, 1, 1, 520), (1, 33, 40, 40)])
def test_guard_gap(shape):
    """One-pass GAP and the sliced two-pass kernel (>= GAP_LARGE_HW pixels) with exactly gap_scratch_elems."""
    B, H, W, Cc = shape
    x = _bf(_rng("gap", shape).standard_normal(shape).astype(np.float32))
    want = x.double().mean(dim=(1, 2))
    need = E.gap_scratch_elems(B, H * W, Cc)
    assert (need > 0) == (H * W >= E.GAP_LARGE_HW)

    def launch(dev, outs, poison):
        sc = _scratch(need, poison, "scratch")
        E.gap(dev["x"], out=outs[0], out32=outs[1], scratch=sc)
        return [sc]

    def check(got):
        torch.testing.assert_close(got[1].double(), want, atol=1e-3, rtol=1e-3)
        torch.testing.assert_close(got[0].double(), want, atol=1e-2, rtol=1e-2)

    _run(f"gap {shape}", {"x": x}, [((B, Cc), BF16), ((B, Cc), F32)], launch, check)


POOL_MAPS = [  # (B, H, W, C, k, stride, pads)
    (2, 13, 11, 8, 3, 2, ((1, 1), (1, 1))), (1, 12, 10, 16, 3, 2, ((0, 1), (0, 1))),
    (1, 7, 5, 8, 2, 2, ((0, 0), (0, 0))), (1, 9, 7, 24, 3, 1, ((1, 1), (1, 1))),
]


@pytest.mark.parametrize("B,H,W,Cc,k,s,pads", POOL_MAPS)
def test_guard_maxpool_avgpool(B, H, W, Cc, k, s, pads):
    """+inf in the guards is what shows a max-pool over-read (max drops NaN)."""
    x = _bf(_rng("pool", H, W, Cc).standard_normal((B, H, W, Cc)).astype(np.float32))
    (pt, pb), (pl, pr) = pads
    OH, OW = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
    xt = x.double().permute(0, 3, 1, 2)
    for pad_zero, value in ((True, 0.0), (False, float("-inf"))):
        want = F.max_pool2d(F.pad(xt, (pl, pr, pt, pb), value=value), k, s).permute(0, 2, 3, 1)
        _run(f"maxpool k {k} s {s} pad_zero {pad_zero} {(B, H, W, Cc)}", {"x": x}, [((B, OH, OW, Cc), BF16)],
             lambda dev, outs, poison: E.maxpool(dev["x"], outs[0], k, s, pt, pl, pad_zero),
             lambda got: torch.testing.assert_close(got[0].double(), want.contiguous(), rtol=0, atol=0))
    num = F.avg_pool2d(F.pad(xt, (pl, pr, pt, pb)), k, s, divisor_override=1)
    den = F.avg_pool2d(F.pad(torch.ones_like(xt[:, :1]), (pl, pr, pt, pb)), k, s, divisor_override=1)
    want = (num / den).permute(0, 2, 3, 1)
    _run(f"avgpool k {k} s {s} {(B, H, W, Cc)}", {"x": x}, [((B, OH, OW, Cc), BF16)],
         lambda dev, outs, poison: E.avgpool(dev["x"], outs[0], k, s, pads),
         lambda got: torch.testing.assert_close(got[0].double(), want.contiguous(), rtol=1e-2, atol=1e-2))


@pytest.mark.parametrize("B,H,W,Cc,k,s,pads,act", [
    (1, 7, 9, 40, 3, 2, ((1, 1), (1, 1)), 1), (2, 10, 10, 16, 5, 1, ((2, 2), (2, 2)), 2),
    (1, 8, 10, 8, 3, 2, ((0, 1), (0, 1)), 0), (1, 5, 3, 8, 3, 1, ((1, 1), (1, 1)), 2)])
def test_guard_dwconv(B, H, W, Cc, k, s, pads, act):
    rng = _rng("dw", H, W, Cc, k)
    x = _bf(rng.standard_normal((B, H, W, Cc)).astype(np.float32))
    w = torch.from_numpy((0.3 * rng.standard_normal((k, k, Cc))).astype(np.float32))
    b = torch.from_numpy((0.1 * rng.standard_normal(Cc)).astype(np.float32))
    (pt, pb), (pl, pr) = pads
    OH, OW = (H + pt + pb - k) // s + 1, (W + pl + pr - k) // s + 1
    xr = F.pad(x.double().permute(0, 3, 1, 2), (pl, pr, pt, pb))
    want = F.conv2d(xr, w.double().permute(2, 0, 1).unsqueeze(1), b.double(), stride=s, groups=Cc).permute(0, 2, 3, 1)
    want = want.clamp_min(0) if act else want
    want = want.clamp(max=6.0) if act == 2 else want
    _run(f"dwconv {(B, H, W, Cc)} k {k} s {s} act {act}", {"x": x, "w": w, "bias": b}, [((B, OH, OW, Cc), BF16)],
         lambda dev, outs, poison: E.dwconv(dev["x"], dev["w"], dev["bias"], outs[0], s, pads, act=act),
         lambda got: torch.testing.assert_close(got[0].double(), want.contiguous(), rtol=2e-2, atol=2e-2))


@pytest.mark.parametrize("chans", [(16, 24), (20, 12, 5)])
def test_guard_concat(chans):
    rng = _rng("concat", chans)
    pad8 = lambda c: (c + 7) // 8 * 8  # noqa: E731
    real = [_bf(rng.standard_normal((1, 7, 5, c)).astype(np.float32)) for c in chans]
    xs = {f"x{i}": F.pad(t, (0, pad8(t.shape[-1]) - t.shape[-1])).contiguous() for i, t in enumerate(real)}
    total = sum(chans)

    def check(got):
        assert torch.equal(got[0][..., :total], torch.cat(real, -1))
        assert bool((got[0][..., total:] == 0).all())

    _run(f"concat {chans}", xs, [((1, 7, 5, pad8(total)), BF16)],
         lambda dev, outs, poison: E.concat([dev[f"x{i}"] for i in range(len(chans))], list(chans), outs[0], total),
         check)


@pytest.mark.parametrize("shape", [(3, 5, 6, 32), (1, 5, 3, 8)])
def test_guard_elementwise(shape):
    """binary (full / per-image broadcast), act, bn_act, add_act, gmp, pad."""
    rng = _rng("eltwise", shape)
    B, H, W, Cc = shape
    a = _bf((3 * rng.standard_normal(shape)).astype(np.float32))
    b = _bf(rng.standard_normal(shape).astype(np.float32))
    se = _bf(rng.standard_normal((B, 1, 1, Cc)).astype(np.float32))
    sc = torch.from_numpy((rng.random(Cc) + 0.5).astype(np.float32))
    sh = torch.from_numpy(rng.standard_normal(Cc).astype(np.float32))
    close = torch.testing.assert_close
    ad, bd = a.double(), b.double()
    for fn, bb, ref in (("add", b, ad + bd), ("max", b, torch.maximum(ad, bd)), ("mul", se, ad * se.double())):
        want = ref * torch.sigmoid(ref) if fn == "mul" else ref
        _run(f"binary {fn} {shape}", {"a": a, "b": bb}, [(shape, BF16)],
             lambda dev, outs, poison: E.binary(dev["a"], dev["b"], outs[0], fn,
                                                act_mode=E.ACT_MODES["swish"] if fn == "mul" else 0),
             lambda got: close(got[0].double(), want, rtol=2e-2, atol=2e-2))
    for name, want in (("relu", ad.clamp_min(0)), ("swish", ad * torch.sigmoid(ad))):
        _run(f"act {name} {shape}", {"x": a}, [(shape, BF16)],
             lambda dev, outs, poison: E.act(dev["x"], outs[0], E.ACT_MODES[name], alpha=0.2),
             lambda got: close(got[0].double(), want, rtol=2e-2, atol=2e-2))
    _run(f"bn_act {shape}", {"x": a, "scale": sc, "shift": sh}, [(shape, BF16)],
         lambda dev, outs, poison: E.bn_act(dev["x"], dev["scale"], dev["shift"], outs[0], relu=False),
         lambda got: close(got[0].double(), ad * sc.double() + sh.double(), rtol=1e-2, atol=2e-2))
    _run(f"add_act {shape}", {"a": a, "b": b}, [(shape, BF16)],
         lambda dev, outs, poison: E.add_act(dev["a"], dev["b"], outs[0], relu=True),
         lambda got: close(got[0].double(), (ad + bd).clamp_min(0), rtol=1e-2, atol=1e-2))
    _run(f"gmp {shape}", {"x": a}, [((B, Cc), BF16)],
         lambda dev, outs, poison: E.gmp(dev["x"], outs[0]),
         lambda got: close(got[0], a.amax(dim=(1, 2)), rtol=0, atol=0))
    _run(f"pad {shape}", {"x": a}, [((B, H + 3, W + 2, Cc), BF16)],
         lambda dev, outs, poison: E.pad(dev["x"], outs[0], 1, 2),
         lambda got: close(got[0], F.pad(a, (0, 0, 2, 0, 1, 2)), rtol=0, atol=0))


@pytest.mark.parametrize("mode", ["none", "caffe", "tf", "torch"])
@pytest.mark.parametrize("shape", [(3, 17, 5, 3), (1, 1, 1, 3)])
def test_guard_ingest_u8(mode, shape):
    """uint8 images between guards of 0xFF bytes."""
    x = np.random.default_rng(0).integers(0, 256, shape, dtype=np.uint8)
    want = E.preprocess_ref(x, mode)
    _run(f"ingest_u8 {mode} {shape}", {"x": torch.from_numpy(x)}, [(shape, F32)],
         lambda dev, outs, poison: E.ingest_u8(dev["x"], outs[0], mode),
         lambda got: np.testing.assert_allclose(got[0].numpy(), want, rtol=1e-6, atol=1e-5))


# ------------------------------------------------------------------ coverage
def test_every_config_ran_guarded():
    """Skipping must not hide a config: every id of every bf16 config table ran guarded on at least one shape
    above (this test runs last in the file)."""
    tables = {"CFG_TILES": set(C.CFG_TILES), "PW_CFGS": set(C.PW_CFGS), "PS_CFGS": set(C.PS_CFGS),
              "RR3_CFGS": set(C.RR3_CFGS), "CS3_CFGS": set(C.CS3_CFGS)}
    missing = {name: sorted(ids - RAN) for name, ids in tables.items() if ids - RAN}
    assert not missing, f"configs that never ran guarded: {missing}"
