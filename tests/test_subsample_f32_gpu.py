"""fp32 1x1 convs whose fused residual is sampled from a larger map (PackedConv.res_stride, `res_row` in
csrc/kernels/kernels.h): every family that claims support, in both forms the plan's lattice pass produces

* ``strided``: x is the full B x H x W map read with the conv's own stride s, the residual the full map
  sampled with the same s (the `_out` conv of a stage once its stride-s readers are its only readers);
* ``dense``:   x is already the compact ceil(H / s) x ceil(W / s) map (stride 1), the residual still the
  full map sampled every s pixels (res_stride independent of the conv's stride).

Each launch is compared two ways: against the float64 oracle within the 2e-5 allowance of
tests/test_pw_f32_gpu.py / tests/test_gemm_f32s_gpu.py, and bit for bit (`torch.equal`) against the same
config's full stride-1 launch sliced ``[:, ::s, ::s, :]``: an output element is one k-ordered chain of fp32
MFMA fmas plus bias and residual, whatever tile it lands in.  Two kinds of launch have no such fixed order and
are exempt from the bit comparison (not from the oracle): stream-K (ksplit < 0), and the rows of a streaming
tail round (cfgs 125 / 126), whose fragments run on four accumulator chains (pw_f32.hip `pw_tail_frag`)
where the main loop uses 4 / FPW: a pixel that sits in the tail round of one launch and in the main loop of
the other differs in the last bit.  Those rows are compared bit for bit between the two forms instead, which
share one tile schedule.

Shapes: B = 2; maps 7x7, 9x5, 8x8 with s = 2 and 3 (M = 32, 30, 18, 12: partial 16-, 32-, 64-row tiles);
K in {64, 128, 256}; N one and two channel slices of the persistent kernel; ReLU on and off.  The three
`TAIL` cases are the smallest maps whose sampled M leaves the streaming kernels a partial last tile round.

Guard bands (tests/guardband.py): x, residual, compact output and workspace between 1 MiB guards, and the
unsampled pixels of x and of the residual poisoned with NaN in one run and +inf in the other: finite,
bit-identical outputs prove that no dead pixel reaches a result.
"""
import functools

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops._lib import kernels

import guardband as G

pytestmark = pytest.mark.gpu

B = 2
BUDGET = 2e-5
NO_PADS = ((0, 0), (0, 0))
MAPS = [(7, 7), (9, 5), (8, 8)]
KNR = [(64, 256, 1), (64, 512, 0), (128, 512, 0), (128, 1024, 1), (256, 256, 1), (256, 512, 0)]   # K, N, ReLU
TAIL = [(95, 95, 128, 512, 1), (47, 47, 256, 1024, 1), (129, 129, 64, 256, 0)]                    # H, W, K, N, ReLU


@functools.lru_cache(maxsize=None)
def _problem(H, W, K, N, relu):
    """Host data and the float64 oracle of the full stride-1 conv, computed once per shape and left unchanged."""
    rng = np.random.default_rng([H, W, K, N])
    x = rng.standard_normal((B, H, W, K)).astype(np.float32)
    kern = (rng.standard_normal((1, 1, K, N)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    res = rng.standard_normal((B, H, W, N)).astype(np.float32)
    want = x.astype(np.float64) @ kern[0, 0].astype(np.float64) + bias + res
    if relu:
        want = np.maximum(want, 0)
    for a in (x, kern, res, want):
        a.setflags(write=False)
    return x, kern, bias, res, want


def _modes(pc, B_, H, W):
    """(cfg, ksplit) of every family that takes this conv with a fused residual: whole K; split-K slabs on the
    tile families (their reduce kernel adds the residual); stream-K where the family has it and accepts the
    shape."""
    OH, OW = pc.out_hw(H, W)
    M = B_ * OH * OW
    for fam in C.F32_FAMILIES:
        for cfg in fam.cfgs:
            if not fam.supported(cfg, pc, True):
                continue
            if cfg in C.PW_F32_TAIL:
                if kernels().pw_f32_tail_plan(M, pc.cin, pc.cout, 0, C.PW_F32_CFGS[cfg])[0]:
                    yield cfg, 1
                continue
            yield cfg, 1
            if fam in (C.F32_V1, C.F32_V2) and pc.Kpad // C.F32_BK >= 4:
                yield cfg, 2
            if fam is C.F32_V2:
                yield cfg, -1
            if fam is C.F32_GEMM_S and cfg not in C.F32S_TM:
                per = C.f32s_tiles(cfg, M, pc.cout) * (pc.cin // 32) // 256
                if per >= 1 and -(-(pc.cin // 32) // per) + 1 <= 16:
                    yield cfg, -1


def _launch(x, pc, res, relu, cfg, ks, shape):
    out = torch.full(shape, float("nan"), device="cuda")
    nws, nctr = C.f32_scratch(cfg, ks, x.shape[0], x.shape[1], x.shape[2], pc)
    ctr = torch.zeros(nctr, dtype=torch.int32, device="cuda") if nctr else None
    C.conv_forward_f32(x, pc, out, res, relu=relu, cfg=cfg, ksplit=ks, counters=ctr)
    return out


def _tail_rows(cfg, M, K, N):
    """First row of the streaming kernels' tail round (M: none)."""
    if cfg not in C.PW_F32_TAIL:
        return M
    tail = kernels().pw_f32_tail_plan(M, K, N, 0, C.PW_F32_CFGS[cfg])[0]
    return (-(-M // 16) - tail) * 16


def _check_case(H, W, K, N, relu, s):
    x, kern, bias, res, want_full = _problem(H, W, K, N, relu)
    OH, OW = -(-H // s), -(-W // s)
    M = B * OH * OW
    want = want_full[:, ::s, ::s, :]
    xd = torch.tensor(x).cuda()
    resd = torch.tensor(res).cuda()
    xc = xd[:, ::s, ::s, :].contiguous()
    full_pc = C.pack_conv_f32(kern, bias, 1, NO_PADS, "cuda")
    forms = {"strided": (xd, C.pack_conv_f32(kern, bias, s, NO_PADS, "cuda", res_stride=s)),
             "dense": (xc, C.pack_conv_f32(kern, bias, 1, NO_PADS, "cuda", res_stride=s))}
    ran = {f: set() for f in forms}
    got, fulls = {}, {}
    for form, (xin, pc) in forms.items():
        assert pc.out_hw(xin.shape[1], xin.shape[2]) == (OH, OW)
        for cfg, ks in _modes(pc, B, xin.shape[1], xin.shape[2]):
            label = f"{form} s={s} {H}x{W} K={K} N={N} relu={relu} cfg {cfg} ksplit {ks}"
            out = _launch(xin, pc, resd, relu, cfg, ks, (B, OH, OW, N))
            g = out.cpu().numpy()
            assert np.isfinite(g).all(), label
            err = np.abs(g - want).max() / max(1.0, np.abs(want).max())
            assert err < BUDGET, f"{label}: rel err {err:.3e}"
            ran[form].add(cfg)
            got[form, cfg, ks] = out
            if ks < 0:
                continue                              # stream-K: partials meet in arrival order
            if not C.f32_family(cfg).supported(cfg, full_pc, True):
                continue
            if cfg in C.PW_F32_TAIL and not kernels().pw_f32_tail_plan(B * H * W, K, N, 0, C.PW_F32_CFGS[cfg])[0]:
                continue                              # the full map leaves this config no tail round to launch
            if (cfg, ks) not in fulls:
                fulls[cfg, ks] = _launch(xd, full_pc, resd, relu, cfg, ks, (B, H, W, N))
            full = fulls[cfg, ks]
            a = out.reshape(M, N)
            b = full[:, ::s, ::s, :].reshape(M, N)
            if cfg in C.PW_F32_TAIL:
                # rows in the main loop of both launches (module docstring)
                r0 = _tail_rows(cfg, M, K, N)
                rows = torch.arange(M, device="cuda")
                img, r = rows // (OH * OW), rows % (OH * OW)
                mfull = (img * H + (r // OW) * s) * W + (r % OW) * s
                keep = (rows < r0) & (mfull < _tail_rows(cfg, B * H * W, K, N))
                a, b = a[keep], b[keep]
            assert torch.equal(a, b), f"{label}: differs from the full stride-1 launch sliced [::{s}, ::{s}]"
    for (form, cfg, ks), out in got.items():          # the two forms share M and the tile schedule
        if form == "dense" and ks > 0 and ("strided", cfg, ks) in got:
            assert torch.equal(out, got["strided", cfg, ks]), f"cfg {cfg} ksplit {ks}: dense and strided forms differ"
    return ran


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("hw", MAPS, ids=lambda m: f"{m[0]}x{m[1]}")
@pytest.mark.parametrize("knr", KNR, ids=lambda t: f"K{t[0]}N{t[1]}r{t[2]}")
def test_sampled_residual_every_family(knr, hw, s):
    K, N, relu = knr
    ran = {form: {C.f32_family(cfg) for cfg in cfgs} for form, cfgs in _check_case(hw[0], hw[1], K, N, relu, s).items()}
    # the dense form is a plain stride-1 1x1: all four 1x1 families take it; the pointwise and big-tile GEMM
    # kernels read x with stride 1 or 2 only, so at s = 3 the strided form is the tile families'
    assert ran["dense"] == {C.F32_V1, C.F32_V2, C.F32_PW, C.F32_GEMM_S}
    assert ran["strided"] == ({C.F32_V1, C.F32_V2, C.F32_PW, C.F32_GEMM_S} if s == 2 else {C.F32_V1, C.F32_V2})


@pytest.mark.parametrize("case", TAIL, ids=lambda t: f"{t[0]}x{t[1]}K{t[2]}N{t[3]}")
def test_sampled_residual_streaming_tail_round(case):
    """Sampled M with a partial last tile round: the tail-fragment path reads the residual through the same
    mapping (cfgs 125 / 126 launch only when there is such a round)."""
    H, W, K, N, relu = case
    M = B * (-(-H // 2)) * (-(-W // 2))
    tails = [cfg for cfg in sorted(C.PW_F32_TAIL) if kernels().pw_f32_tail_plan(M, K, N, 0, C.PW_F32_CFGS[cfg])[0]]
    assert tails, "no tail config launches on this case"
    ran = _check_case(H, W, K, N, relu, 2)
    assert set(tails) <= ran["dense"] and set(tails) <= ran["strided"]


def test_wino_and_mismatched_geometry_are_refused():
    """A family without the sampled residual reports the conv unsupported; a residual whose lattice is not the
    output map is an error, never a wrong launch."""
    x, kern, bias, res, _ = _problem(7, 7, 64, 256, 1)
    k3 = np.zeros((3, 3, 64, 256), np.float32)
    pc3 = C.pack_conv_f32(k3, bias, 1, ((1, 1), (1, 1)), "cuda", res_stride=2)
    for cfg in C.WINO_F32_CFGS:
        assert not C.f32_family(cfg).supported(cfg, pc3, True)
        assert not any(c == cfg for c, _ in C.f32_candidates(2, 7, 7, pc3, True))
    pc = C.pack_conv_f32(kern, bias, 1, NO_PADS, "cuda", res_stride=2)
    xc = torch.from_numpy(np.ascontiguousarray(x[:, ::2, ::2, :])).cuda()
    out = torch.empty((B, 4, 4, 256), device="cuda")
    for bad in (torch.zeros((B, 9, 7, 256), device="cuda"), torch.zeros((B, 4, 4, 256), device="cuda"),
                torch.zeros((B * 7 * 7, 256), device="cuda"), torch.zeros((B, 7, 7, 128), device="cuda")):
        with pytest.raises(ValueError):
            C.conv_forward_f32(xc, pc, out, bad, relu=1, cfg=122)


# ------------------------------------------------------------------ guard bands
def _poisoned(a, s, value):
    """`a` [B, H, W, C] with every pixel off the (s i, s j) lattice set to `value`."""
    p = np.full_like(a, value)
    p[:, ::s, ::s, :] = a[:, ::s, ::s, :]
    return p


@pytest.mark.parametrize("form", ["strided", "dense"])
@pytest.mark.parametrize("hw,s,K,N", [((7, 7), 2, 64, 256), ((9, 5), 2, 128, 512), ((9, 5), 3, 256, 512),
                                      ((47, 47), 2, 256, 1024)], ids=lambda v: str(v).replace(" ", ""))
def test_guard_sampled_residual(form, hw, s, K, N):
    H, W = hw
    x, kern, bias, res, want_full = _problem(H, W, K, N, 1)
    OH, OW = -(-H // s), -(-W // s)
    want = want_full[:, ::s, ::s, :]
    outs = {}
    modes = None
    for poison, value in ((G.NAN, np.nan), (G.INF, np.inf)):
        # unsampled pixels poisoned: a dead pixel that reaches a result makes it non-finite
        resd = G.guarded(res.shape, torch.float32, "cuda", payload=_poisoned(res, s, value), poison=poison,
                         name="residual")
        if form == "strided":
            xin = G.guarded(x.shape, torch.float32, "cuda", payload=_poisoned(x, s, value), poison=poison, name="x")
            pc = C.pack_conv_f32(kern, bias, s, NO_PADS, "cuda", res_stride=s)
        else:
            xc = np.ascontiguousarray(x[:, ::s, ::s, :])
            xin = G.guarded(xc.shape, torch.float32, "cuda", payload=xc, poison=poison, name="x")
            pc = C.pack_conv_f32(kern, bias, 1, NO_PADS, "cuda", res_stride=s)
        for f in ("w", "bias", "pwf"):
            if getattr(pc, f, None) is not None:
                setattr(pc, f, G.rehome(getattr(pc, f), poison=poison, name=f"pc.{f}"))
        modes = list(_modes(pc, B, xin.shape[1], xin.shape[2]))
        for cfg, ks in modes:
            label = f"{form} cfg {cfg} ksplit {ks} [{poison} poison]"
            out = G.guarded((B, OH, OW, N), torch.float32, "cuda", payload=float("nan"), name="out")
            nws, nctr = C.f32_scratch(cfg, ks, B, xin.shape[1], xin.shape[2], pc)
            ws = G.guarded(nws, torch.float32, "cuda", payload=float("nan"), poison=poison, name="workspace") \
                if nws else None
            ctr = G.guarded(nctr, torch.int32, "cuda", payload=0, name="counters") if nctr else None
            C.conv_forward_f32(xin, pc, out, resd, relu=1, cfg=cfg, ksplit=ks, workspace=ws, counters=ctr)
            torch.cuda.synchronize()
            G.check(xin, resd, out, ws, ctr, pc.w, pc.bias, pc.pwf, what=label)
            if ctr is not None:
                assert int(ctr.abs().sum()) == 0, f"{label}: arrival counters not back to zero"
            outs[poison, cfg, ks] = out.cpu()
    assert modes
    for cfg, ks in modes:
        a, b = outs[G.NAN, cfg, ks], outs[G.INF, cfg, ks]
        label = f"{form} cfg {cfg} ksplit {ks}"
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), f"{label}: a dead pixel reached the output"
        assert torch.equal(a, b), f"{label}: outputs differ between the NaN and +inf runs"
        err = np.abs(a.numpy() - want).max() / max(1.0, np.abs(want).max())
        assert err < BUDGET, f"{label}: rel err {err:.3e}"
