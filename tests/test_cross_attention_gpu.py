"""The cross-attention kernels (csrc/kernels/cross_attention.hip) and the learned-queries kernel
(csrc/kernels/layers.hip) on the GPU, against the float64 oracle and the allowance of tests/cross_attention_cases.py,
and DETR's test size through SliceExecutor.

Every case runs in fp32 and in bf16, in its layout (three buffers, [K | V] or [Q | K] side by side, NaN in every
row's surplus: the kernels never read it), with the output pre-filled with NaN: all finite, within the allowance
(bf16: 2^-8 |want| + allowance), and the bf16 layout's padding channels exact zeros.

`detr_micro` (35 memory tokens, 10 queries, 2 + 2 layers, 2 heads of 16) with the budgets of tests/test_vit_gpu.py:
within 1e-3 (fp32) and 5e-2 (bf16) of the oracle, relative to the largest output.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_model
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import cross_attention_cases as XC

pytestmark = pytest.mark.gpu

ENC_CUT, DEC_CUT = "encoder_0_ln_attn", "decoder_0_ln_self"


def _device(t, name):
    return t.cuda()


@pytest.mark.parametrize("c", XC.CASES, ids=str)
def test_cross_attention_f32(c):
    k = XC.case(c)
    q, kk, v, _ = XC.views(k, _device)
    out = torch.full(k.want.shape, float("nan"), dtype=torch.float32, device="cuda")
    assert A.cross_attention_path(q, kk, v, out, k.d, k.dv) == k.path
    A.cross_attention(q, kk, v, out, k.B, k.Tq, k.Tk, k.heads, k.d, k.dv)
    torch.cuda.synchronize()
    got = out.double().cpu().numpy()
    err = np.abs(got - k.want).max()
    print(f"cross_attention fp32 {c} [{k.path}]: e_ref {k.e_ref:.3e}, max err {err:.3e}, allowance {k.allow:.3e}")
    assert np.isfinite(got).all() and err <= k.allow


@pytest.mark.parametrize("c", XC.CASES, ids=str)
def test_cross_attention_bf16(c):
    k = XC.case_bf16(c)
    q, kk, v, _ = XC.views(k, _device, dtype=torch.bfloat16)
    ld_out = (k.w_out + 7) // 8 * 8
    out = torch.full((k.B * k.Tq, ld_out), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert A.cross_attention_path(q, kk, v, out, k.d, k.dv) == k.path
    A.cross_attention(q, kk, v, out, k.B, k.Tq, k.Tk, k.heads, k.d, k.dv)
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[:, k.w_out:] == 0).all(), "padding channels must come out as exact zeros"
    over = np.abs(got[:, :k.w_out] - k.want) - (2.0 ** -8 * np.abs(k.want) + k.allow)
    print(f"cross_attention bf16 {c} [{k.path}]: max err {np.abs(got[:, :k.w_out] - k.want).max():.3e}, "
          f"worst excess {over.max():.3e}")
    assert (over <= 0).all()


def test_cross_attention_refuses_what_it_cannot_index_or_hold():
    q = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    kv = torch.zeros((6, 48), dtype=torch.float32, device="cuda")
    y = torch.zeros((4, 16), dtype=torch.float32, device="cuda")
    k, v = kv[:, :16], kv[:, 16:32]
    A.cross_attention(q, k, v, y, 1, 4, 6, 1, 16, 16)                           # what the refusals below vary
    with pytest.raises(ValueError):
        A.cross_attention(q, k, v, y, 1, 4, 6, 1, 16, 32)                       # v and out too narrow for dv = 32
    with pytest.raises(ValueError):
        A.cross_attention(q, k, v, y, 1, 4, 5, 1, 16, 16)                       # not 5 key rows
    with pytest.raises(ValueError):
        A.cross_attention(q, k, v, y, 2, 4, 6, 1, 16, 16)                       # not 2 images
    with pytest.raises(ValueError):
        A.cross_attention(q, k.to(torch.bfloat16), v, y, 1, 4, 6, 1, 16, 16)    # mixed dtypes
    with pytest.raises(ValueError):
        A.cross_attention(q, k, v, y, 1, 4, 0, 1, 16, 16)
    big = torch.zeros((2, 4, 48), dtype=torch.float32, device="cuda")
    q2, y2 = torch.zeros((8, 16), dtype=torch.float32, device="cuda"), torch.zeros((8, 16), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):                                             # 3 of every 4 rows: two strides
        A.cross_attention(q2, big[:, :3, :16], big[:, :3, 16:32], y2, 2, 4, 3, 1, 16, 16)
    A.cross_attention(q2, big[:, :, :16], big[:, :, 16:32], y2, 2, 4, 4, 1, 16, 16)     # all rows: one stride
    with pytest.raises(ValueError):
        A.cross_attention(q, k, v, y[:, :8], 1, 4, 6, 1, 16, 16)                # the output is not contiguous
    with pytest.raises(ValueError):
        A.cross_attention(q.cpu(), k, v, y, 1, 4, 6, 1, 16, 16)
    torch.cuda.synchronize()
    assert A.cross_attention_path(q, k, v, y, 16, 16) == "mfma" and A.cross_attention_path(q, k, v, y, 24, 24) == "plain"
    assert A.cross_attention_path(q, kv[:, 2:18], v, y, 16, 16) == "plain"      # K 8 bytes off the 16-byte grid


QUERY_CASES = [(2, 5, 64), (3, 7, 20), (1, 1, 6), (2, 100, 256)]          # B, N, C


@pytest.mark.parametrize("c", QUERY_CASES, ids=str)
def test_queries_f32_is_bit_exact(c):
    B, N, C = c
    emb = np.random.default_rng(N * C).standard_normal((N, C)).astype(np.float32)
    out = torch.full((B, 1, N, C), float("nan"), dtype=torch.float32, device="cuda")
    A.queries(torch.from_numpy(emb).cuda(), out)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), np.broadcast_to(emb, (B, 1, N, C)))


@pytest.mark.parametrize("c", QUERY_CASES, ids=str)
def test_queries_bf16(c):
    B, N, C = c
    Cp = (C + 7) // 8 * 8
    emb = torch.from_numpy(np.random.default_rng(N * C).standard_normal((N, C)).astype(np.float32))
    out = torch.full((B, 1, N, Cp), float("nan"), dtype=torch.bfloat16, device="cuda")
    A.queries(emb.cuda(), out, C=C)
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[..., C:] == 0).all()
    # one rounding to bf16, the library's own
    assert torch.equal(got[..., :C], emb.to(torch.bfloat16).expand(B, 1, N, C))
    with pytest.raises(ValueError):
        A.queries(emb.cuda(), out, C=C + 1)                                     # not the table's width


# ------------------------------------------------------------------ DETR
@pytest.fixture(scope="module")
def micro():
    g = build_model("detr_micro")
    w = init_weights(g, seed=0)
    for n in list(w):                       # biases of O(1): a dropped or misplaced one must show
        if n.endswith("/bias"):
            w[n] = np.random.default_rng(len(n)).standard_normal(w[n].shape).astype(np.float32) * 0.5
    x = np.random.default_rng(5).standard_normal((4, 40, 56, 3)).astype(np.float32)
    x[2:] += 3.0        # a brighter second pair: the queries dominate the output, so like images give like outputs
    want = ReferenceExecutor(g, w, device="cpu")(torch.from_numpy(x)).double().numpy()
    return g, w, x, want


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_detr_micro_matches_oracle_and_replays(micro, precision, budget):
    """Eager, then captured: the replay of the first input is bit-identical to its eager run, and a second input
    gives its own result."""
    g, w, x, want = micro
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    kinds = [st.kind for st in ex.steps]
    assert kinds.count("queries") == 3 and kinds.count("attention") == 6
    xa, xb = torch.from_numpy(x[:2]).cuda(), torch.from_numpy(x[2:]).cuda()
    first = ex(xa).clone()
    torch.cuda.synchronize()
    got = first.double().cpu().numpy()
    rel = np.abs(got - want[:2]).max() / np.abs(want[:2]).max()
    print(f"detr_micro {precision} rel err {rel:.3e}")
    assert got.shape == (2, 1, 10, 96) and np.isfinite(got).all() and rel <= budget
    ex.capture()
    assert ex.captured
    other = ex(xb).clone()
    again = ex(xa).clone()
    torch.cuda.synchronize()
    assert torch.equal(again, first), "the hipGraph replay differs from the first run"
    rel = np.abs(other.double().cpu().numpy() - want[2:]).max() / np.abs(want[2:]).max()
    assert rel <= budget
    # the two inputs' outputs are further apart than the budget, so a stale replay could not have passed above
    assert np.abs(want[:2] - want[2:]).max() > 4 * budget * np.abs(want).max()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("cut", [ENC_CUT, DEC_CUT])
def test_detr_micro_sliced_equals_unsliced(micro, precision, cut):
    """A cut inside an encoder layer (the position table crosses beside it) and one inside a decoder layer (the
    running target, the memory, memory + pos and the query embedding): both stages run the same kernels on the same
    values, bit-identical."""
    g, w, x, _ = micro
    xd = torch.from_numpy(x[:2]).cuda()
    full = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)(xd).clone()
    parts = slicer.partition(g, [cut])
    assert len(parts[1].inputs) == (2 if cut == ENC_CUT else 4)
    vals = {g.input: xd}
    for s in parts:
        sg = slicer.subgraph(g, s)
        ex = SliceExecutor(sg, w, batch=2, device="cuda:0", precision=precision)
        out = ex.run({k: vals[k] for k in sg.input_names})
        vals.update({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert torch.equal(vals[g.output], full)
