"""The layer cases of tests/layer_cases.py without a GPU: every hand-written float64 oracle against torch's float64
functional op (two independent references, 1e-12), torch's fp32 evaluation and the native CPU ops inside the
per-element allowances (the check that the allowances are sound: none is fitted to a kernel), and the fp32
executor's activation dispatch: the plan fuses any ActMode but LeakyReLU into `add` and `bn` steps, so the op those
steps run must implement it.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import ACT_MODE
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor, _act)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import executor as X
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

import layer_cases as LC

F64, F32 = torch.float64, torch.float32


def T(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def tpad(t, pads, value=0.0):
    (pt, pb), (pl, pr) = pads
    return F.pad(t, (pl, pr, pt, pb), value=value)


def t_act(t, mode, alpha=0.3):
    if LC.ACT_NAMES[mode] == "softplus" and t.dtype == F64:
        return F.softplus(t, threshold=1e3)       # the default returns x above 20: 2e-9 off, fine in fp32 only
    return _act(t, LC.ACT_NAMES[mode], alpha)


def t_dwconv(k, dt, act=True):
    C = k.x.shape[-1]
    w = T(k.w, dt).permute(2, 0, 1).unsqueeze(1)
    y = F.conv2d(tpad(nchw(T(k.x, dt)), k.pads), w, T(k.bias, dt), stride=k.stride, groups=C)
    return nhwc(t_act(y, k.mode, k.alpha) if act else y)


def t_maxpool(k, dt):
    xp = tpad(nchw(T(k.x, dt)), k.pads, 0.0 if k.pad_zero else float("-inf"))
    return nhwc(F.max_pool2d(xp, k.k, k.s))


def t_avgpool(k, dt):
    xp = tpad(nchw(T(k.x, dt)), k.pads)
    ones = tpad(torch.ones(1, 1, *k.x.shape[1:3], dtype=dt), k.pads)
    return nhwc(F.avg_pool2d(xp, k.k, k.s) / F.avg_pool2d(ones, k.k, k.s))


def t_binary(k, dt):
    a, b = T(k.a, dt), T(k.b, dt)
    r = {"add": a + b, "sub": a - b, "mul": a * b, "max": torch.maximum(a, b.expand_as(a)),
         "min": torch.minimum(a, b.expand_as(a)), "avg": 0.5 * (a + b)}[k.op]
    return t_act(r, k.mode).numpy()


def t_eltwise(k, dt):
    a = T(k.a, dt)
    if k.op == "add":
        a = a + T(k.b, dt)
    elif k.op == "bn":
        a = a * T(k.scale, dt) + T(k.shift, dt)
    return t_act(a, k.mode).numpy()


def t_actcase(k, dt):
    x = T(k.x, dt)
    if k.scale is not None:
        x = x * T(k.scale, dt) + T(k.shift, dt)
    return t_act(x, k.mode, k.alpha).numpy()


def close64(what, got, want):
    """Two float64 evaluations of the same formula: 1e-12, relative to max(1, |want|)."""
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert got.shape == want.shape and err.max() <= 1e-12, f"{what}: oracle and torch float64 differ by {err.max():.3e}"


# (family, cases, case builder, torch evaluation); max pool, pad and concat are copies: bit-exact
LINEAR = [
    ("dwconv", LC.DW_CASES_F32, LC.dw_case, t_dwconv),
    ("avgpool", LC.AVGPOOL_CASES_F32, LC.avgpool_case, t_avgpool),
    ("gap", LC.GAP_CASES_F32, LC.gap_case, lambda k, dt: T(k.x, dt).mean((1, 2)).numpy()),
    ("act", LC.ACT_CASES_F32, LC.act_case, t_actcase),
    ("eltwise", LC.ELTWISE_CASES_F32, LC.eltwise_case, t_eltwise),
    ("binary", LC.BINARY_CASES_F32, LC.binary_case, t_binary),
    ("softmax", LC.SOFTMAX_CASES, LC.softmax_case, lambda k, dt: torch.softmax(T(k.x, dt), -1).numpy()),
]
IDS = [f[0] for f in LINEAR]


@pytest.mark.parametrize("name,cases,build,teval", LINEAR, ids=IDS)
def test_oracles_agree_with_torch_float64(name, cases, build, teval):
    for c in cases:
        k = build(c)
        close64(f"{name} {c}", teval(k, F64), k.want)


@pytest.mark.parametrize("name,cases,build,teval", LINEAR, ids=IDS)
def test_torch_fp32_stays_inside_the_allowances(name, cases, build, teval):
    top = max(LC.check(f"{name} {c}", teval(build(c), F32), build(c).want, build(c).allow) for c in cases)
    print(f"{name}: torch fp32 uses at most {top:.3f} of the allowance")


def test_copy_oracles_agree_with_torch():
    for c in LC.MAXPOOL_CASES_F32:
        k = LC.maxpool_case(c)
        LC.check_bits(f"maxpool {c}", t_maxpool(k, F64), k.want)
        assert (k.want[0, 0, 0] <= 0).all() and np.isfinite(k.want).all()       # the all-negative window is there
    for c in LC.GMP_CASES:
        k = LC.gmp_case(c)
        LC.check_bits(f"gmp {c}", T(k.x, F64).amax((1, 2)).numpy(), k.want)
        assert (k.want[0] < 0).all()
    for c in LC.PAD_CASES_F32:
        k = LC.pad_case(c)
        B, H, W, C, pt, pl, e = c
        LC.check_bits(f"pad {c}", F.pad(T(k.x, F64), (0, 0, pl, e, pt, e)).numpy(), k.want)
    for c in LC.CONCAT_CASES_F32 + LC.CONCAT_CASES_BF16:
        k = LC.concat_case(c)
        LC.check_bits(f"concat {c}", torch.cat([T(a, F64) for a in k.xs], -1).numpy(), k.want)


def test_all_negative_maxpool_border_is_zero_under_pad_zero():
    k = LC.maxpool_case(LC.MAXPOOL_CASES_F32[0])
    assert k.pad_zero and (k.x < 0).all()
    assert (k.want[:, 0] == 0).all() and (k.want[:, :, 0] == 0).all() and (k.want[:, 1:-1, 1:-1] < 0).all()


def test_bf16_register_blocked_cases_sit_on_their_side_of_the_rule():
    assert all(LC.dw3_rule(c) for c in LC.DW3_CASES)
    assert not any(LC.dw3_rule(c) for c in LC.DW3_NEIGHBOURS + LC.DW_CASES_BF16)


def test_dw3_oracle_agrees_with_torch_float64_and_fp32_fits():
    for c in (LC.DW3_CASES[0], LC.DW3_CASES[-1]):
        k = LC.dw_case(c, True)
        close64(f"dw3 {c}", t_dwconv(k, F64), k.want)
        LC.check(f"dw3 {c} fp32", t_dwconv(k, F32), k.want, k.allow)


def test_bf16_rounding_of_the_fp32_value_fits_the_bf16_allowance():
    """One round-to-nearest-even of torch's fp32 value: the bound is tight on purpose (2^-8 |y| is half a bf16 ulp
    bounded from above)."""
    top = 0.0
    for c in LC.ACT_CASES_BF16:
        k = LC.act_case(c, True)
        got = T(t_actcase(k, F32), torch.bfloat16).float().numpy()
        top = max(top, LC.check(f"act bf16 {c}", got, k.want, LC.bf16_allow(k.allow, k.want)))
    print(f"bf16 rounding uses at most {top:.3f}")


def test_cast_inputs_hold_ties_zeros_infinities_and_the_largest_float():
    x = LC.cast_input()
    bits = x.view(np.uint32)
    assert x.size == 1024 and np.isinf(x).sum() == 2 and (bits == 0x80000000).any() and (bits == 0).any()
    assert (bits == 0x7F7FFFFF).any() and ((bits & 0xFFFF) == 0x8000).sum() >= 6 and not np.isnan(x).any()
    r = T(x, torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert r[0] == 0x3F80 and r[1] == 0x3F82                 # ties go to even, down and up
    assert r[10] == 0x7F80                                   # the largest finite float rounds to +inf


# ------------------------------------------------------------------ native CPU ops
@pytest.fixture(scope="module")
def cpu():
    return cpu_executor.native()


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def test_native_dwconv_and_pools(cpu):
    for c in LC.DW_CASES_F32:
        k = LC.dw_case(c)
        y = np.full(k.want.shape, np.nan, np.float32)
        cpu.dwconv2d(k.x, k.w, k.bias, y, k.stride, k.pads[0][0], k.pads[1][0], k.mode, k.alpha)
        LC.check(f"cpu dwconv {c}", y, k.want, k.allow)
    for c in LC.AVGPOOL_CASES_F32:
        k = LC.avgpool_case(c)
        y = np.full(k.want.shape, np.nan, np.float32)
        cpu.pool2d(k.x, y, 1, k.k[0], k.k[1], k.s, k.pads[0][0], k.pads[1][0], False)
        LC.check(f"cpu avgpool {c}", y, k.want, k.allow)
    for c in LC.MAXPOOL_CASES_F32:
        k = LC.maxpool_case(c)
        y = np.full(k.want.shape, np.nan, np.float32)
        cpu.pool2d(k.x, y, 0, k.k, k.k, k.s, k.pads[0][0], k.pads[1][0], k.pad_zero)
        LC.check_bits(f"cpu maxpool {c}", y, f32(k.want))
    for c in LC.GAP_CASES_F32:
        k = LC.gap_case(c)
        y = np.full(k.want.shape, np.nan, np.float32)
        cpu.global_pool(k.x, y, 0)
        LC.check(f"cpu gap {c}", y, k.want, k.allow)
    for c in LC.GMP_CASES:
        k = LC.gmp_case(c)
        y = np.full(k.want.shape, np.nan, np.float32)
        cpu.global_pool(k.x, y, 1)
        LC.check_bits(f"cpu gmp {c}", y, f32(k.want))


def test_native_elementwise(cpu):
    for c in LC.ACT_CASES_F32:
        k = LC.act_case(c)
        y = np.full(k.x.shape, np.nan, np.float32)
        if k.scale is None:
            cpu.activation(k.x, y, k.mode, k.alpha)
        else:
            cpu.affine(k.x, k.scale, k.shift, y, k.mode, k.alpha)
        LC.check(f"cpu act {c}", y, k.want, k.allow)
    for c in LC.BINARY_CASES_F32:
        k = LC.binary_case(c)
        y = np.full(k.a.shape, np.nan, np.float32)
        cpu.binary(k.a, f32(k.b.reshape(k.b.shape[0], -1)) if k.b.shape != k.a.shape else k.b, y,
                   cpu_executor._BINARY[k.op], k.mode, 0.3)
        LC.check(f"cpu binary {c}", y, k.want, k.allow)
    for c in LC.SOFTMAX_CASES:
        k = LC.softmax_case(c)
        y = np.full(k.x.shape, np.nan, np.float32)
        cpu.softmax(k.x, y)
        LC.check(f"cpu softmax {c}", y, k.want, k.allow)


def test_native_copies(cpu):
    for c in LC.CONCAT_CASES_F32:
        k = LC.concat_case(c)
        y = np.full(k.want.shape, LC.SENTINEL, np.float32)
        cpu.concat(list(k.xs), y)
        LC.check_bits(f"cpu concat {c}", y, f32(k.want))
    for c in LC.PAD_CASES_F32:
        k = LC.pad_case(c)
        y = np.full(k.want.shape, LC.SENTINEL, np.float32)
        cpu.zero_pad(k.x, y, k.pt, k.pl)
        LC.check_bits(f"cpu pad {c}", y, f32(k.want))


# ------------------------------------------------------------------ the fp32 executor's activation dispatch
def test_plan_fuses_swish_into_add_and_gelu_into_bn():
    g = LC.addbn_graph()
    for fp32 in (True, False):
        steps = {st.kind: st for st in compile_plan(g, fp32=fp32)}
        assert steps["add"].p["relu"] == ACT_MODE["swish"] and steps["add"].out == "sg"
        assert steps["bn"].p["relu"] == ACT_MODE["gelu"] and steps["bn"].out == "out"
    se = {st.kind: st for st in compile_plan(LC.se_graph(), fp32=True)}
    assert se["binary"].p == {"fn": "mul", "act": ACT_MODE["hard_swish"]}


@pytest.mark.parametrize("graph", [LC.addbn_graph, LC.se_graph], ids=["addbn", "se"])
def test_cpu_executor_matches_the_reference_on_the_tiny_graphs(graph):
    g = graph()
    w = init_weights(g, seed=3)
    x = torch.randn(2, 8, 8, 16, generator=torch.Generator().manual_seed(5))
    outs = [n for n in ("sg", "out") if n in g.layers]
    want = ReferenceExecutor(g, w, device="cpu").run({g.input: x}, outputs=outs)
    got = cpu_executor.CpuExecutor(g, w, outputs=outs).run({g.input: x.numpy()}, outputs=outs)
    for n in outs:
        err = np.abs(got[n] - want[n].numpy()).max()
        assert err <= 1e-5, f"{graph.__name__} {n}: native CPU differs from the reference by {err:.3e}"


def planner_modes(kind):
    """Every ActMode runtime/plan.py can put into a step of `kind` (its `act_mode` fuses all but LeakyReLU; a
    `relu` step is ReLU or ReLU6; an `act` step is any activation layer)."""
    fusible = {m for n, m in ACT_MODE.items() if n != "leaky_relu"}
    return {"relu": {1, 2}, "act": set(ACT_MODE.values())}.get(kind, fusible)


@pytest.mark.parametrize("kind", sorted(X.F32_ACT_STEPS))
def test_fp32_steps_dispatch_to_an_op_that_implements_every_mode_the_plan_can_give(kind):
    op, key = X.F32_ACT_STEPS[kind]
    missing = planner_modes(kind) - E.f32_act_modes(op)
    assert not missing, f"fp32 step {kind!r} runs {op}, which lacks ActModes {sorted(missing)} of p[{key!r}]"


def test_eltwise_f32_refuses_a_mode_its_kernel_lacks():
    a = torch.zeros(1, 1, 1, 4)
    for bad in (ACT_MODE["leaky_relu"], -1, 14):
        with pytest.raises(ValueError, match="ActMode"):
            E.eltwise_f32(a, torch.empty_like(a), relu=bad)
