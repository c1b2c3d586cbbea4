"""The padding-mask instantiations of the attention kernels (csrc/kernels/attention_core.h, attention.hip) on the
GPU, and DistilBERT through SliceExecutor.

Every case of tests/padding_mask_cases.py (head sizes 16 .. 128 on the MFMA path and 24 on the plain kernel, the
token counts around both tiles, three images with a pattern each, 2 heads) runs in fp32 and bf16 with rows wider
than the heads need (the input's extra channels hold NaN, the output is pre-filled with NaN):

* within the allowance of the float64 oracle (bf16: 2^-8 |want| + allowance); padded rows, every row of an image
  with no kept key, and every layout-padding channel are exact zeros;
* an all-kept mask gives the bits of the unmasked entry point;
* right padding to L gives, at the kept rows, the bits of the unmasked entry point run on the first L tokens
  alone (the tile order is the same and a masked term is an exact 0);
* NaN in every row past an image's last kept token changes no bit at a kept row: nothing past it is read.

A NaN at an interior masked key is not required to be harmless (0 x NaN is NaN in Keras too) and is not tested.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph import slicer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import (
    SliceExecutor)

import padding_mask_cases as PC

pytestmark = pytest.mark.gpu

EXTRA = 8           # layout padding per row, both buffers: keeps the 4-element alignment of the MFMA path
DTYPES = [torch.float32, torch.bfloat16]


def _k(c, dtype):
    return PC.case(c) if dtype == torch.float32 else PC.case_bf16(c)


def _padded_input(k, dtype, qkv=None):
    w_in = k.heads * (2 * k.d + k.dv)
    x = torch.full((k.B * k.T, w_in + EXTRA), float("nan"), dtype=dtype)
    x[:, :w_in] = torch.from_numpy(k.qkv if qkv is None else qkv).to(dtype)
    return x.cuda()


def _run(k, x, dtype, mask=None, B=None, T=None):
    B, T = B or k.B, T or k.T
    out = torch.full((B * T, k.heads * k.dv + EXTRA), float("nan"), dtype=dtype, device="cuda")
    A.attention(x, out, B, T, k.heads, k.d, k.dv,
                key_mask=None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda())
    torch.cuda.synchronize()
    return out.cpu()


def _bound(want, allow, dtype):
    return allow if dtype == torch.float32 else 2.0 ** -8 * np.abs(want) + allow


@pytest.mark.parametrize("c", PC.CASES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_masked_attention_against_the_oracle(c, dtype):
    k = _k(c, dtype)
    x = _padded_input(k, dtype)
    w = k.heads * k.dv
    for gr in k.groups:
        out = _run(k, x, dtype, gr.mask)
        got = out.float().numpy().astype(np.float64)
        err = np.abs(got[:, :w] - gr.want)
        print(f"masked attention {dtype} {c} {gr.group} [{k.path}]: max err {err.max():.3e}, "
              f"allowance {gr.allow:.3e}")
        assert np.isfinite(got).all()
        assert (err <= _bound(gr.want, gr.allow, dtype)).all()
        assert (got[~gr.rows] == 0).all(), "padded rows and images with no kept key must be exact zeros"
        assert (got[:, w:] == 0).all(), "layout padding must be exact zeros"


@pytest.mark.parametrize("c", PC.CASES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_an_all_kept_mask_gives_the_bits_of_the_unmasked_entry_point(c, dtype):
    k = _k(c, dtype)
    x = _padded_input(k, dtype)
    ids = np.random.default_rng(k.T).integers(1, 97, (k.B, k.T)).astype(np.float32)
    assert torch.equal(_run(k, x, dtype, ids), _run(k, x, dtype))


@pytest.mark.parametrize("c", PC.CASES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_right_padding_gives_the_bits_of_the_unmasked_launch_on_the_prefix(c, dtype):
    """Also: NaN in every row past the last kept token (Q, K and V) changes no bit at a kept row."""
    k = _k(c, dtype)
    lengths = sorted({min(n, k.T) for n in (1, 32, 33, max(k.T - 1, 1))})
    x = _padded_input(k, dtype)
    for first in range(0, len(lengths), k.B):
        ls = (lengths[first:first + k.B] * k.B)[:k.B]               # one length per image
        mask = np.stack([PC.pattern("all", k.T, seed=b) for b in range(k.B)])
        for b, n in enumerate(ls):
            mask[b, n:] = 0.0
        out = _run(k, x, dtype, mask).reshape(k.B, k.T, -1)
        poisoned = x.clone().reshape(k.B, k.T, -1)
        for b, n in enumerate(ls):
            poisoned[b, n:] = float("nan")
        out_p = _run(k, poisoned.reshape(k.B * k.T, -1), dtype, mask).reshape(k.B, k.T, -1)
        for b, n in enumerate(ls):
            alone = _run(k, x.reshape(k.B, k.T, -1)[b, :n].contiguous(), dtype, B=1, T=n)
            assert torch.equal(out[b, :n], alone), f"image {b}, length {n}: bits differ from the prefix alone"
            assert torch.equal(out_p[b, :n], out[b, :n]), f"image {b}, length {n}: a row past the bound was read"
            assert (out[b, n:] == 0).all() and (out_p[b, n:] == 0).all()


def test_the_wrapper_checks_the_mask():
    k = PC.case((16, 33))
    x = torch.from_numpy(k.qkv).cuda()
    out = torch.empty((k.B * k.T, k.heads * k.dv), dtype=torch.float32, device="cuda")
    ok = torch.ones((k.B, k.T), dtype=torch.float32, device="cuda")
    A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, key_mask=ok)
    for bad in (ok.cpu(), ok.to(torch.bfloat16), ok[:, :-1].contiguous(), ok.t()):
        with pytest.raises(ValueError):
            A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, key_mask=bad)
    with pytest.raises(ValueError):
        A.attention(x, out, k.B, k.T, k.heads, k.d, k.dv, key_mask=ok, causal=True)


# ------------------------------------------------------------------ DistilBERT
# three stages; the middle one (the first layer's FFN) holds no attention layer and only relays the ids
RELAY_CUTS = ["distilbert_micro_layer_0_sa_layer_norm", "distilbert_micro_layer_0_output_layer_norm"]
BLOCK_KINDS = ["conv", "attention", "conv", "layernorm", "conv", "act", "conv", "layernorm"]
CUT = "distilbert_micro_layer_0_ffn_lin1"


@pytest.mark.parametrize("precision,budget", [("fp32", 1e-3), ("bf16", 5e-2)])
def test_distilbert_micro_matches_the_model_by_hand_and_the_cpu_path(precision, budget):
    """The model budgets of tests/test_gpt_gpu.py: within 1e-3 (fp32) and 5e-2 (bf16) of the model by hand in
    float64, relative to the largest value; every position, padded ones included (the project's semantics)."""
    g, w, ids, want = PC.micro()
    ex = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)
    assert [st.kind for st in ex.steps] == ["embedding", "posembed", "layernorm"] + BLOCK_KINDS * 2     # no pack step
    assert [st.p.get("key_mask") for st in ex.steps if st.kind == "attention"] == [True, True]
    assert ex.input_buf(g.input).dtype == torch.float32 and tuple(ex.input_buf(g.input).shape) == (2, 40)
    cpu = cpu_executor.CpuExecutor(g, w)(ids).reshape(want.shape)
    for half in (slice(0, 2), slice(2, 4)):
        out = ex(torch.from_numpy(ids[half]).cuda())
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        got = out.double().cpu().numpy().reshape(2, 40, -1)[..., :32]
        rel = np.abs(got - want[half]).max() / np.abs(want[half]).max()
        rel_cpu = np.abs(got - cpu[half]).max() / np.abs(cpu[half]).max()
        print(f"distilbert_micro {precision} rel err {rel:.3e} (against the cpu path {rel_cpu:.3e})")
        assert rel <= budget and rel_cpu <= budget


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_stage_slice_equals_unsliced_and_the_ids_stay_fp32(precision):
    g, w, ids, _ = PC.micro()
    xd = torch.from_numpy(ids[:2]).cuda()
    full = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)(xd).clone()
    parts = slicer.partition(g, [CUT])
    assert g.input in parts[1].inputs and parts[0].relay == [g.input]
    vals = {g.input: xd}
    for s in parts:
        sg = slicer.subgraph(g, s)
        ex = SliceExecutor(sg, w, batch=2, device="cuda:0", precision=precision)
        assert ex.input_buf(g.input).dtype == torch.float32         # the ids: never packed, never rounded
        out = ex.run({k: vals[k] for k in sg.input_names})
        vals.update({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert torch.equal(vals[g.input].cpu(), xd.cpu())
    assert torch.equal(vals[g.output], full)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_a_stage_that_only_relays_the_ids_keeps_them_fp32(precision):
    """Three stages, the middle one without an attention layer: it reads the ids nowhere and hands them on.  Its
    input and output buffers of the ids are float32 like every other stage's, so the buffers on both sides of each
    link agree; two odd ids above 256, which bf16 does not hold, arrive unchanged, and the result is the unsliced
    run's bit for bit."""
    g, w, ids, _ = PC.micro()
    big = ids[:2].copy()
    big[0, 1], big[1, 2] = 301.0, 511.0                             # out of the 97-row table: zero rows, still kept
    assert (torch.from_numpy(big).to(torch.bfloat16).float().numpy() != big).any()
    xd = torch.from_numpy(big).cuda()
    full = SliceExecutor(g, w, batch=2, device="cuda:0", precision=precision)(xd).clone()
    parts = slicer.partition(g, RELAY_CUTS)
    assert [any(g.layers[n].op == "mha" for n in s.layers) for s in parts] == [True, False, True]
    assert parts[1].relay == [g.input] and g.input in parts[2].inputs
    vals = {g.input: xd}
    for s in parts:
        sg = slicer.subgraph(g, s)
        ex = SliceExecutor(sg, w, batch=2, device="cuda:0", precision=precision)
        assert ex.input_buf(g.input).dtype == torch.float32, s.name
        if g.input in s.outputs:
            assert ex.output_buf(g.input).dtype == torch.float32, s.name
        out = ex.run({k: vals[k] for k in sg.input_names})
        vals.update({k: v.clone() for k, v in out.items()})
        assert vals[g.input].dtype == torch.float32 and torch.equal(vals[g.input], xd), s.name
    torch.cuda.synchronize()
    assert torch.isfinite(full).all() and torch.equal(vals[g.output], full)
