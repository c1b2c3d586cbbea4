"""The layer kernels of csrc/kernels/{layers,eltwise,conv_f32,head}.hip on the MI355X against the float64 oracles
of tests/layer_cases.py: depthwise conv, max / average / global pools, activations, Add / BN / binary ops, concat,
zero pad, casts, `input_pack`, `softmax_rows`, in bf16 and fp32, through the ops/eltwise.py wrappers.

Every element is held to its own allowance (module docstring of layer_cases.py: derived from the oracle and the
inputs, checked against torch's fp32 evaluation in tests/test_layer_cases.py, never fitted to a kernel); copies are
compared bit for bit.  Besides the small shapes that reach each path there is one case per capped launcher just
past 2,097,152 work items (the second pass of its grid-stride loop), the fp32 scalar fallbacks through a base that
is 4 bytes off 16-byte alignment, and two tiny graphs through `SliceExecutor` whose plans fuse a non-ReLU
activation into `add`, `bn` and `binary` steps.
"""
import functools

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import layer_cases as LC

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for key in sorted(RATIOS):
        print(f"\nRATIO {key}: {RATIOS[key]:.3f}", end="")
    print()


def note(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), ratio)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().to(dtype)


def off16(a):
    """`a` on the device as a contiguous fp32 tensor whose base is 4 bytes past 16-byte alignment."""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def blank(shape, dtype=torch.float32, fill=float("nan")):
    return torch.full(tuple(shape), fill, dtype=dtype, device="cuda")


def blank_off16(shape):
    buf = torch.full((int(np.prod(shape)) + 1,), float("nan"), dtype=torch.float32, device="cuda")
    return buf[1:].view(tuple(shape))


def host(t):
    torch.cuda.synchronize()
    return t.float().cpu().numpy()


def same_bits(what, got, want):
    """A copy: the fp32 widening of both sides must agree bit for bit (bf16 -> fp32 is exact)."""
    LC.check_bits(what, host(got), np.ascontiguousarray(want, np.float32))


# ------------------------------------------------------------------ depthwise conv
def run_dw_f32(k, mis=False):
    put = off16 if mis else dev
    out = blank_off16(k.want.shape) if mis else blank(k.want.shape)
    E.dwconv_f32(put(k.x), dev(k.w), dev(k.bias), out, k.stride, k.pads, act=k.mode, alpha=k.alpha)
    return host(out)


@pytest.mark.parametrize("c", LC.DW_CASES_F32, ids=repr)
def test_dwconv_f32(c):
    k = LC.dw_case(c)
    note("dwconv fp32", LC.check(f"dwconv_f32 {c}", run_dw_f32(k), k.want, k.allow))


@pytest.mark.parametrize("c", [c for c in LC.DW_CASES_F32 if c[3] == 8], ids=repr)
def test_dwconv_f32_scalar_kernel_through_a_misaligned_base(c):
    k = LC.dw_case(c)
    note("dwconv fp32 scalar", LC.check(f"dwconv_f32 misaligned {c}", run_dw_f32(k, True), k.want, k.allow))


def run_dw_bf16(k):
    out = blank(k.want.shape, BF16)
    E.dwconv(dev(k.x, BF16), dev(k.w), dev(k.bias), out, k.stride, k.pads, act=k.mode)
    return host(out)


@pytest.mark.parametrize("c", LC.DW_CASES_BF16, ids=repr)
def test_dwconv_bf16_generic(c):
    assert not LC.dw3_rule(c)
    k = LC.dw_case(c, True)
    note("dwconv bf16", LC.check(f"dwconv {c}", run_dw_bf16(k), k.want, LC.bf16_allow(k.allow, k.want)))


@pytest.mark.parametrize("c", LC.DW3_CASES + LC.DW3_NEIGHBOURS, ids=repr)
def test_dwconv_bf16_register_blocked_3x3_and_its_neighbour(c):
    assert LC.dw3_rule(c) == (c in LC.DW3_CASES)
    k = LC.dw_case(c, True)
    note("dwconv bf16 3x3 blocked" if LC.dw3_rule(c) else "dwconv bf16",
         LC.check(f"dwconv {c}", run_dw_bf16(k), k.want, LC.bf16_allow(k.allow, k.want)))


# ------------------------------------------------------------------ pools
@pytest.mark.parametrize("c", LC.MAXPOOL_CASES_F32, ids=repr)
def test_maxpool_f32(c):
    k = LC.maxpool_case(c)
    out = blank(k.want.shape)
    E.maxpool_f32(dev(k.x), out, k.k, k.s, k.pads[0][0], k.pads[1][0], k.pad_zero)
    same_bits(f"maxpool_f32 {c}", out, k.want)


@pytest.mark.parametrize("c", LC.MAXPOOL_CASES_BF16, ids=repr)
def test_maxpool_bf16(c):
    k = LC.maxpool_case(c, True)
    out = blank(k.want.shape, BF16)
    E.maxpool(dev(k.x, BF16), out, k.k, k.s, k.pads[0][0], k.pads[1][0], k.pad_zero)
    same_bits(f"maxpool {c}", out, k.want)


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("c", LC.AVGPOOL_CASES_F32, ids=repr)
def test_avgpool_f32(c, mis):
    k = LC.avgpool_case(c)
    out = blank_off16(k.want.shape) if mis else blank(k.want.shape)
    E.avgpool_f32((off16 if mis else dev)(k.x), out, k.k, k.s, k.pads)
    note("avgpool fp32", LC.check(f"avgpool_f32 {c} misaligned={mis}", host(out), k.want, k.allow))


@pytest.mark.parametrize("c", LC.AVGPOOL_CASES_BF16, ids=repr)
def test_avgpool_bf16(c):
    k = LC.avgpool_case(c, True)
    out = blank(k.want.shape, BF16)
    E.avgpool(dev(k.x, BF16), out, k.k, k.s, k.pads)
    note("avgpool bf16", LC.check(f"avgpool {c}", host(out), k.want, LC.bf16_allow(k.allow, k.want)))


@pytest.mark.parametrize("c", LC.GAP_CASES_F32, ids=repr)
def test_gap_f32(c):
    k = LC.gap_case(c)
    assert (E.gap_scratch_elems(c[0], c[1] * c[2], c[3]) > 0) == (c in LC.GAP_LARGE)
    if c[0] == 600:
        assert E.kernels().gap_large_slices(c[0], c[1] * c[2]) == 1
    out = blank(k.want.shape)
    E.gap_f32(dev(k.x), out)
    note("gap fp32", LC.check(f"gap_f32 {c}", host(out), k.want, k.allow))


@pytest.mark.parametrize("c", LC.GAP_CASES_BF16, ids=repr)
def test_gap_bf16_both_outputs(c):
    k = LC.gap_case(c, True)
    assert (E.gap_scratch_elems(c[0], c[1] * c[2], c[3]) > 0) == (c in LC.GAP_LARGE)
    out, out32 = blank(k.want.shape, BF16), blank(k.want.shape)
    E.gap(dev(k.x, BF16), out, out32)
    note("gap bf16 (fp32 output)", LC.check(f"gap {c} fp32 output", host(out32), k.want, k.allow))
    note("gap bf16", LC.check(f"gap {c} bf16 output", host(out), k.want, LC.bf16_allow(k.allow, k.want)))


@pytest.mark.parametrize("c", LC.GMP_CASES, ids=repr)
def test_global_max_pool_bf16(c):
    k = LC.gmp_case(c, True)
    out = blank(k.want.shape, BF16)
    E.gmp(dev(k.x, BF16), out)
    same_bits(f"gmp {c}", out, k.want)


# ------------------------------------------------------------------ activations, Add, BN, binary
@pytest.mark.parametrize("c", LC.ACT_CASES_BF16, ids=repr)
def test_act_bf16_every_mode(c):
    k = LC.act_case(c, True)
    out = blank(k.x.shape, BF16)
    E.act(dev(k.x, BF16), out, k.mode, k.alpha)
    if k.mode <= 2:
        same_bits(f"act {c}", out, k.want)
    note("act bf16", LC.check(f"act {c}", host(out), k.want, LC.bf16_allow(k.allow, k.want)))


# C = 6 takes the scalar kernel as it is; C = 4 also through a misaligned base
@pytest.mark.parametrize("c,mis", [(c, m) for c in LC.ACT_CASES_F32 for m in (False, True) if not m or c[2] == 4],
                         ids=repr)
def test_affine_act_f32_every_mode(c, mis):
    k = LC.act_case(c)
    out = blank_off16(k.x.shape) if mis else blank(k.x.shape)
    sc, sh = (None, None) if k.scale is None else (dev(k.scale), dev(k.shift))
    E.affine_act_f32((off16 if mis else dev)(k.x), out, sc, sh, act=k.mode, alpha=k.alpha)
    note("affine_act fp32", LC.check(f"affine_act_f32 {c} misaligned={mis}", host(out), k.want, k.allow))


@pytest.mark.parametrize("c", LC.FUSED_CASES_BF16, ids=repr)
def test_relu_add_act_bn_act_bf16(c):
    k = LC.eltwise_case(c, True)
    out = blank(k.a.shape, BF16)
    if k.op == "add":
        E.add_act(dev(k.a, BF16), dev(k.b, BF16), out, relu=k.mode)
    elif k.op == "bn":
        E.bn_act(dev(k.a, BF16), dev(k.scale), dev(k.shift), out, relu=k.mode)
    else:
        E.relu(dev(k.a, BF16), out, mode=k.mode)
        if k.mode <= 2:
            same_bits(f"relu {c}", out, k.want)
    note({"add": "add_act", "bn": "bn_act", "act": "relu"}[k.op] + " bf16",
         LC.check(f"bf16 {c}", host(out), k.want, LC.bf16_allow(k.allow, k.want)))


@pytest.mark.parametrize("c", LC.ELTWISE_CASES_F32, ids=repr)
def test_eltwise_f32_every_op_and_mode(c):
    k = LC.eltwise_case(c)
    out = blank(k.a.shape)
    if k.op == "add":
        E.eltwise_f32(dev(k.a), out, b=dev(k.b), relu=k.mode)
    elif k.op == "bn":
        E.eltwise_f32(dev(k.a), out, scale=dev(k.scale), shift=dev(k.shift), relu=k.mode)
    else:
        E.eltwise_f32(dev(k.a), out, relu=k.mode)
    note("eltwise fp32", LC.check(f"eltwise_f32 {c}", host(out), k.want, k.allow))


def test_eltwise_f32_refuses_leaky_relu():
    a = dev(np.zeros((1, 1, 1, 4)))
    with pytest.raises(ValueError, match="ActMode"):
        E.eltwise_f32(a, torch.empty_like(a), relu=LC.ACT["leaky_relu"])


@pytest.mark.parametrize("c,mis", [(c, m) for c in LC.BINARY_CASES_F32 for m in (False, True)
                                   if not m or c[3][-1] % 4 == 0], ids=repr)
def test_binary_f32(c, mis):
    k = LC.binary_case(c)
    put = off16 if mis else dev
    out = blank_off16(k.a.shape) if mis else blank(k.a.shape)
    E.binary_f32(put(k.a), dev(k.b), out, k.op, k.mode)
    note("binary fp32", LC.check(f"binary_f32 {c} misaligned={mis}", host(out), k.want, k.allow))


@pytest.mark.parametrize("c", LC.BINARY_CASES_BF16, ids=repr)
def test_binary_bf16(c):
    k = LC.binary_case(c, True)
    out = blank(k.a.shape, BF16)
    E.binary(dev(k.a, BF16), dev(k.b, BF16), out, k.op, k.mode)
    note("binary bf16", LC.check(f"binary {c}", host(out), k.want, LC.bf16_allow(k.allow, k.want)))


# ------------------------------------------------------------------ concat, pad
def pad8(c):
    return (c + 7) // 8 * 8


@pytest.mark.parametrize("c", LC.CONCAT_CASES_BF16, ids=repr)
def test_concat_bf16_writes_every_channel_and_zeroes_the_padding(c):
    k = LC.concat_case(c, True)
    xs = []
    for a in k.xs:                                  # the inputs' own padding holds a sentinel: it must not travel
        p = np.full(a.shape[:-1] + (pad8(a.shape[-1]),), 55.0, np.float32)
        p[..., :a.shape[-1]] = a
        xs.append(dev(p, BF16))
    total = sum(c)
    out = blank(LC.CONCAT_PIXELS + (pad8(total),), BF16, LC.SENTINEL)
    E.concat(xs, list(c), out, total)
    got = host(out)
    LC.check_bits(f"concat {c}", got[..., :total], k.want.astype(np.float32))
    assert (got[..., total:] == 0).all(), f"concat {c}: padding channels are not zero"


@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("c", LC.CONCAT_CASES_F32, ids=repr)
def test_concat_f32(c, mis):
    k = LC.concat_case(c)
    out = blank(k.want.shape, fill=LC.SENTINEL)
    E.concat_f32([(off16 if mis else dev)(a) for a in k.xs], out)
    same_bits(f"concat_f32 {c} misaligned={mis}", out, k.want)


@pytest.mark.parametrize("c", LC.PAD_CASES_F32, ids=repr)
def test_pad_f32(c):
    k = LC.pad_case(c)
    out = blank(k.want.shape, fill=LC.SENTINEL)
    E.pad_f32(dev(k.x), out, k.pt, k.pl)
    same_bits(f"pad_f32 {c}", out, k.want)


@pytest.mark.parametrize("c", LC.PAD_CASES_BF16, ids=repr)
def test_pad_bf16(c):
    k = LC.pad_case(c, True)
    out = blank(k.want.shape, BF16, LC.SENTINEL)
    E.pad(dev(k.x, BF16), out, k.pt, k.pl)
    same_bits(f"pad {c}", out, k.want)


# ------------------------------------------------------------------ softmax, casts, input_pack
@pytest.mark.parametrize("c", LC.SOFTMAX_CASES, ids=repr)
def test_softmax_rows(c):
    k = LC.softmax_case(c)
    out = blank(k.x.shape)
    E.softmax_rows(dev(k.x), out)
    note("softmax fp32", LC.check(f"softmax_rows {c}", host(out), k.want, k.allow))


def bits16(t):
    torch.cuda.synchronize()
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def test_casts_match_torch_bit_for_bit():
    x = LC.cast_input()
    want = torch.from_numpy(x).to(BF16)                                  # the CPU's round to nearest even
    out = blank((x.size,), BF16, 1.0)
    E.cast_f32_bf16(dev(x), out)
    got = bits16(out)
    bad = np.flatnonzero(got != bits16(want))
    assert bad.size == 0, f"cast_f32_bf16: {x[bad[0]]!r} -> {got[bad[0]]:#06x}, torch gives {bits16(want)[bad[0]]:#06x}"
    back = blank((x.size,), fill=1.0)
    E.cast_bf16_f32(want.cuda(), back)
    torch.cuda.synchronize()
    LC.check_bits("cast_bf16_f32", back.cpu().numpy(), want.float().numpy())


@pytest.mark.parametrize("c", LC.INPUT_PACK_CASES, ids=repr)
def test_input_pack_rounds_as_torch_and_zeroes_the_padding(c):
    C, Cp = c
    x = LC.input_pack_input(c)
    out = blank(x.shape[:3] + (Cp,), BF16, LC.SENTINEL)
    E.input_pack(dev(x), out)
    got = bits16(out)
    want = bits16(torch.from_numpy(x).to(BF16))
    assert (got[..., :C] == want).all(), f"input_pack {c}: real channels differ from torch's rounding"
    assert (got[..., C:] == 0).all(), f"input_pack {c}: padding channels are not +0"


# ------------------------------------------------------------------ second pass of the grid-stride loops
N1 = LC.GRID_CAP_ITEMS + 257          # elements of a kernel whose work item is 1 element
N4, N8 = 4 * N1, 8 * N1


@functools.lru_cache(maxsize=None)
def noise():
    return np.random.default_rng(20).standard_normal(17_100_000, dtype=np.float32)     # the largest case and a bit


def big(n, shape=None, bf16=False, seed=0):
    """(host fp32 values, device tensor) of n N(0, 1) elements; bf16: rounded on the way."""
    x = np.roll(noise(), 7919 * seed)[:n].reshape(shape or (n,))
    d = torch.from_numpy(x).cuda()
    if bf16:
        d = d.to(BF16)
        x = host(d)
    return x, d


def test_second_pass_act_and_relu_bf16():
    x, d = big(N8, bf16=True)
    out = blank((N8,), BF16)
    E.act(d, out, LC.ACT["swish"])
    want = LC.ref_act(x, "swish")
    note("act bf16", LC.check("act second pass", host(out), want, LC.bf16_allow(LC.act_allow(x, want), want)))
    E.relu(d, out, mode=1)
    same_bits("relu second pass", out, LC.ref_act(x, "relu"))


def test_second_pass_add_act_and_binary_bf16():
    a, da = big(N8, (N1, 8), bf16=True)
    b, db = big(N8, (N1, 8), bf16=True, seed=1)
    out = blank((N1, 8), BF16)
    E.add_act(da, db, out, relu=0)
    want = LC.ref_binary(a, b, "add")
    note("add_act bf16", LC.check("add_act second pass", host(out), want,
                                  LC.bf16_allow(LC.binary_lin(a, b, "add"), want)))
    E.binary(da, db, out, "mul", 1)
    pre = LC.ref_binary(a, b, "mul")
    want = LC.ref_act(pre, "relu")
    note("binary bf16", LC.check("binary second pass", host(out), want, LC.bf16_allow(
        LC.fused_allow(LC.binary_lin(a, b, "mul"), pre, want, 1), want)))


def test_second_pass_bn_act_bf16():
    x, d = big(N8, (N1, 8), bf16=True)
    sc, sh = np.linspace(0.5, 1.5, 8, dtype=np.float32), np.linspace(-1, 1, 8, dtype=np.float32)
    out = blank((N1, 8), BF16)
    E.bn_act(d, dev(sc), dev(sh), out, relu=1)
    pre = LC.ref_affine(x, sc, sh)
    want = LC.ref_act(pre, "relu")
    L = LC.lin_allow(1, LC.ref_affine(np.abs(x), sc, np.abs(sh)))
    note("bn_act bf16", LC.check("bn_act second pass", host(out), want,
                                 LC.bf16_allow(LC.fused_allow(L, pre, want, 1), want)))


def test_second_pass_casts_and_input_pack():
    x, d = big(N1)
    out = blank((N1,), BF16, 1.0)
    E.cast_f32_bf16(d, out)
    assert torch.equal(out.cpu().view(torch.int16), torch.from_numpy(x).to(BF16).view(torch.int16))
    back = blank((N1,), fill=1.0)
    E.cast_bf16_f32(out, back)
    same_bits("cast_bf16_f32 second pass", back, LC.to_bf16(x))
    x3, d3 = big(3 * N1, (1, 1, N1, 3))
    packed = blank((1, 1, N1, 8), BF16, LC.SENTINEL)
    E.input_pack(d3, packed)
    got = host(packed)
    LC.check_bits("input_pack second pass", got[..., :3], LC.to_bf16(x3))
    assert (got[..., 3:] == 0).all()


@pytest.mark.parametrize("C,n", [(4, N4), (1, N1)], ids=["vector", "scalar"])
def test_second_pass_affine_binary_eltwise_f32(C, n):
    a, da = big(n, (n // C, C))
    b, db = big(n, (n // C, C), seed=1)
    sc, sh = np.linspace(0.5, 1.5, C, dtype=np.float32), np.linspace(-1, 1, C, dtype=np.float32)
    out = blank((n // C, C))
    E.affine_act_f32(da, out, dev(sc), dev(sh), act=LC.ACT["swish"])
    pre = LC.ref_affine(a, sc, sh)
    want = LC.ref_act(pre, "swish")
    L = LC.lin_allow(1, LC.ref_affine(np.abs(a), sc, np.abs(sh)))
    note("affine_act fp32", LC.check("affine_act_f32 second pass", host(out), want, LC.fused_allow(L, pre, want, 3)))
    E.binary_f32(da, db, out, "sub", 1)
    pre = LC.ref_binary(a, b, "sub")
    want = LC.ref_act(pre, "relu")
    note("binary fp32", LC.check("binary_f32 second pass", host(out), want,
                                 LC.fused_allow(LC.binary_lin(a, b, "sub"), pre, want, 1)))
    if C == 4:                                      # eltwise_f32 has no scalar kernel
        E.eltwise_f32(da, out, b=db, relu=LC.ACT["swish"])
        pre = LC.ref_binary(a, b, "add")
        want = LC.ref_act(pre, "swish")
        note("eltwise fp32", LC.check("eltwise_f32 second pass", host(out), want,
                                      LC.fused_allow(LC.binary_lin(a, b, "add"), pre, want, 3)))


# (name, bf16, x shape, kh, kw, pads): stride 1; the smallest maps whose work items cross the cap
SPATIAL = [
    ("dwconv", True, (2, 130, 128, 512), 5, 5, ((2, 2), (2, 2))),          # generic kernel, item = 8 channels
    ("dwconv", True, (2, 1025, 1, 8200), 3, 3, LC.P1),                      # register-blocked: item = 4 px x 8 ch
    ("dwconv", False, (2, 130, 128, 256), 3, 3, LC.P1),                     # dwconv_f32v, item = 4 channels
    ("dwconv", False, (1, 131, 128, 126), 3, 3, LC.P1),                     # dwconv_f32, item = 1 element
    ("maxpool", True, (2, 130, 128, 512), 3, 3, LC.P1),
    ("maxpool", False, (2, 130, 128, 256), 3, 3, LC.P1),
    ("avgpool", True, (2, 130, 128, 512), 3, 3, LC.P1),
    ("avgpool", False, (2, 130, 128, 256), 3, 3, LC.P1),
    ("avgpool", False, (1, 131, 128, 126), 3, 3, LC.P1),
]


def spatial_items(name, bf16, shape, kh, kw, pads):
    B, H, W, C = shape
    OH, OW = LC.out_hw(H, W, kh, kw, 1, pads)
    if name == "dwconv" and bf16 and LC.dw3_rule((B, H, W, C, kh, kw, 1, pads)):
        return B * OH * ((OW + 3) // 4) * (C // 8)
    per = 8 if bf16 else (4 if C % 4 == 0 else 1)
    return B * OH * OW * C // per


@pytest.mark.parametrize("name,bf16,shape,kh,kw,pads", SPATIAL, ids=lambda v: repr(v).replace(" ", ""))
def test_second_pass_spatial(name, bf16, shape, kh, kw, pads):
    """The first two output rows of the first image and the last four of the last one (written by the second pass)
    against the oracle run on the matching input rows."""
    B, H, W, C = shape
    n = B * H * W * C
    assert LC.GRID_CAP_ITEMS < spatial_items(name, bf16, shape, kh, kw, pads) and n * (2 if bf16 else 4) <= 40e6
    x, d = big(n, shape, bf16=bf16)
    OH, OW = LC.out_hw(H, W, kh, kw, 1, pads)
    out = blank((B, OH, OW, C), BF16 if bf16 else torch.float32)
    r = np.random.default_rng(3)
    w, bias = (0.3 * r.standard_normal((kh, kw, C))).astype(np.float32), (0.3 * r.standard_normal(C)).astype(np.float32)
    mode = LC.ACT["swish"]
    if name == "dwconv":
        (E.dwconv if bf16 else E.dwconv_f32)(d, dev(w), dev(bias), out, 1, pads, act=mode)
    elif name == "maxpool":
        (E.maxpool if bf16 else E.maxpool_f32)(d, out, kh, 1, pads[0][0], pads[1][0], False)
    else:
        (E.avgpool if bf16 else E.avgpool_f32)(d, out, (kh, kw), 1, pads)
    got = host(out)
    top, bot = LC.crop_rows(H, OH, kh, 1, pads[0][0])
    for img, rows, (r0, r1, hp) in ((0, slice(0, 2), top), (B - 1, slice(OH - 4, OH), bot)):
        xc, cp, g = x[img:img + 1, r0:r1], (hp, pads[1]), got[img:img + 1, rows]
        what = f"{name} {'bf16' if bf16 else 'fp32'} {shape} second pass, image {img} rows {rows}"
        if name == "maxpool":
            LC.check_bits(what, g, LC.ref_maxpool(xc, kh, 1, cp, False).astype(np.float32))
            continue
        if name == "dwconv":
            pre = LC.ref_dwconv(xc, w, bias, 1, cp)
            want = LC.ref_act(pre, mode)
            L = LC.lin_allow(kh * kw, LC.ref_dwconv(np.abs(xc), np.abs(w), np.abs(bias), 1, cp))
            allow = LC.fused_allow(L, pre, want, mode)
        else:
            want, cnt = LC.ref_avgpool(xc, kh, kw, 1, cp)
            allow = LC.lin_allow(cnt, LC.ref_avgpool(np.abs(xc), kh, kw, 1, cp)[0])
        note(f"{name} {'bf16' if bf16 else 'fp32'}",
             LC.check(what, g, want, LC.bf16_allow(allow, want) if bf16 else allow))


@pytest.mark.parametrize("bf16,shape", [(True, (2, 128, 128, 512)), (False, (1, 129, 128, 126))], ids=["bf16", "fp32"])
def test_second_pass_pad(bf16, shape):
    B, H, W, C = shape
    x, d = big(B * H * W * C, shape, bf16=bf16)
    out = blank((B, H + 2, W, C), BF16 if bf16 else torch.float32, LC.SENTINEL)
    assert out.numel() // (8 if bf16 else 1) > LC.GRID_CAP_ITEMS
    (E.pad if bf16 else E.pad_f32)(d, out, 1, 0)
    got = host(out)
    for img in (0, B - 1):
        LC.check_bits(f"pad second pass image {img}", got[img:img + 1],
                      LC.ref_pad(x[img:img + 1], 1, 0, H + 2, W).astype(np.float32))


P_BIG = LC.GRID_CAP_ITEMS // 8 + 33      # pixels: 8 chunks (or 9 scalars) per pixel cross the cap


@pytest.mark.parametrize("chans", [(64, 8), (9, 7)], ids=["vector", "scalar"])
def test_second_pass_concat_bf16(chans):
    assert P_BIG * (chans[0] // 8 if chans[0] % 8 == 0 else chans[0]) > LC.GRID_CAP_ITEMS
    xs, ds = zip(*(big(P_BIG * pad8(c), (1, 1, P_BIG, pad8(c)), bf16=True, seed=i) for i, c in enumerate(chans)))
    total = sum(chans)
    out = blank((1, 1, P_BIG, pad8(total)), BF16, LC.SENTINEL)
    E.concat(list(ds), list(chans), out, total)
    got = host(out)
    LC.check_bits("concat second pass", got[..., :total],
                  LC.ref_concat([a[..., :c] for a, c in zip(xs, chans)]).astype(np.float32))
    assert (got[..., total:] == 0).all()


@pytest.mark.parametrize("chans", [(32, 4), (9, 3)], ids=["vector", "scalar"])
def test_second_pass_concat_f32(chans):
    assert P_BIG * (chans[0] // 4 if chans[0] % 4 == 0 else chans[0]) > LC.GRID_CAP_ITEMS
    xs, ds = zip(*(big(P_BIG * c, (1, 1, P_BIG, c), seed=i) for i, c in enumerate(chans)))
    out = blank((1, 1, P_BIG, sum(chans)), fill=LC.SENTINEL)
    E.concat_f32(list(ds), out)
    same_bits("concat_f32 second pass", out, LC.ref_concat(xs))


# ------------------------------------------------------------------ the tiny graphs through SliceExecutor
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("graph", [LC.addbn_graph, LC.se_graph], ids=["addbn", "se"])
def test_fused_activations_through_the_executor(graph, precision):
    """fp32: max |got - want| / max |want| <= 1e-4 (tests/test_fp32_gpu.py); bf16: ||got - want|| / ||want|| < 5e-2
    (the feature bound of tests/test_zoo_gpu.py)."""
    g = graph()
    w = init_weights(g, seed=3)
    x = torch.randn(2, 8, 8, 16, generator=torch.Generator().manual_seed(5))
    outs = [n for n in ("sg", "out") if n in g.layers]
    want = ReferenceExecutor(g, w, device="cpu").run({g.input: x}, outputs=outs)
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", outputs=outs, precision=precision)
    kinds = {st.kind: st.p for st in ex.steps}
    if graph is LC.addbn_graph:
        assert kinds["add"]["relu"] == LC.ACT["swish"] and kinds["bn"]["relu"] == LC.ACT["gelu"]
    else:
        assert kinds["binary"]["act"] == LC.ACT["hard_swish"]
    ex.capture()
    assert ex.captured
    got = ex.run({g.input: x.cuda()})
    torch.cuda.synchronize()
    for n in outs:
        a, b = got[n].float().cpu().reshape(2, 8, 8, -1)[..., :16].double(), want[n].double()
        if precision == "fp32":
            rel = float((a - b).abs().max() / b.abs().max())
            print(f"{g.name} {n} fp32: max error / max |want| {rel:.3e}")
            assert rel <= 1e-4, f"{g.name} {n}: fp32 relative error {rel:.3e} > 1e-4"
        else:
            rel = float((a - b).norm() / b.norm())
            print(f"{g.name} {n} bf16: relative error {rel:.3e}")
            assert rel < 5e-2, f"{g.name} {n}: bf16 relative error {rel:.3e}"
