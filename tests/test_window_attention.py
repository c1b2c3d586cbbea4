"""Window attention and space-to-depth without a GPU: the case list against the kernel's paths and tiles, the
probes' power to tell wrong variants apart, the native CPU ops on every case within the allowance of
tests/window_attention_cases.py, the `ReferenceExecutor` layer against a by-hand float64 forward, and the bias
packer against the published index and mask.

The HIP kernels: tests/test_window_attention_gpu.py, tests/test_guard_window_attention_gpu.py.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.attention import window_bias
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor

import window_attention_cases as WC


def test_the_cases_meet_every_path_and_tile():
    assert (WC.QT, WC.KT) == (64, 32), "the case list is written for 64-query / 32-key tiles: add M^2 around new ones"
    mfma = [c for c in WC.CASES if WC.case(c).path == "mfma"]
    plain = [c for c in WC.CASES if WC.case(c).path == "plain"]
    assert {c[6] for c in plain} == {6, 24} and {c[6] for c in mfma} == {16, 32, 64, 128}
    ts = {c[3] ** 2 for c in mfma}
    assert ts >= {4, 16, 49, 64, 144}                   # below a key tile, off both tiles, exactly a query tile, 3 / 5 tiles
    assert any(c[4] == 0 for c in mfma) and any(c[4] > 0 and c[1] // c[3] > 1 and c[2] // c[3] > 1 for c in mfma)
    assert any(c[1] != c[2] and c[0] > 1 for c in WC.CASES)
    assert any(WC.widths(c)[0] % 8 and WC.widths(c)[1] % 8 for c in plain)
    assert {c[7] for c in WC.CASES if c[7]} == {"ascending", "descending", "masked_dominant"}
    for c in (c for c in WC.CASES if c[7] in ("ascending", "descending")):
        k = WC.case(c)
        q, kk, _ = WC.split(k.qkv.astype(np.float64), k.B, k.H, k.W, k.heads, k.d)
        q, kk = (WC._windows(np.roll(t, (-k.shift, -k.shift), axis=(1, 2)), k.M) for t in (q, kk))
        s = np.einsum("bnqhd,bnkhd->bnhqk", q, kk)
        arg = s.argmax(-1)
        assert 80 < s.max() < 130
        last = (k.M ** 2 - 1) // WC.KT * WC.KT             # first key of the last key tile
        assert k.M ** 2 > 2 * WC.KT and ((arg >= last).all() if c[7] == "ascending" else (arg < WC.KT).all())
    assert set(WC.GUARD_CASES) <= set(WC.CASES) and len(WC.GUARD_CASES) == 5


def test_masked_dominant_tells_the_wrong_variants_apart():
    """A hard mask, no mask, an ignored shift and an ignored bias each move the result far beyond the allowance."""
    c = (2, 14, 14, 7, 3, 2, 32, "masked_dominant")
    k = WC.case(c)
    args = (k.qkv, k.table, k.B, k.H, k.W, k.M, k.shift, k.heads, k.d)
    for name, kw in (("hard mask", {"mask_value": -np.inf}), ("no mask", {"mask_value": 0.0}),
                     ("no shift", {"use_shift": False}), ("no bias", {"use_bias": False})):
        moved = np.abs(WC.ref_window_attention(*args, **kw) - k.want).max()
        print(f"masked_dominant, {name}: moves the result by {moved:.2f} (allowance {k.allow:.1e})")
        assert moved > 1.0 > 1000 * k.allow


@pytest.mark.parametrize("c", WC.CASES, ids=str)
def test_cpu_window_attention_matches_float64_oracle(c):
    k = WC.case(c)
    y = np.full(k.want.shape, np.nan, np.float32)
    cpu_executor.native().window_attention(k.qkv, k.table, y, k.B, k.H, k.W, k.M, k.shift, k.heads, k.d)
    err = np.abs(y.astype(np.float64) - k.want).max()
    print(f"cpu window attention {c} [{k.path}]: e_ref {k.e_ref:.3e}, max err {err:.3e}, allowance {k.allow:.3e}")
    assert np.isfinite(y).all() and err <= k.allow


def test_cpu_window_attention_takes_padded_rows_and_refuses_bad_shapes():
    c = (2, 6, 9, 3, 1, 3, 6, None)
    k = WC.case(c)
    w_in, w_out = WC.widths(c)
    x = np.full((k.rows, w_in + 6), np.nan, np.float32)            # the padding is never read
    x[:, :w_in] = k.qkv
    y = np.full((k.rows, w_out + 6), np.nan, np.float32)
    op = cpu_executor.native().window_attention
    op(x, k.table, y, k.B, k.H, k.W, k.M, k.shift, k.heads, k.d)
    assert (y[:, w_out:] == 0).all() and np.abs(y[:, :w_out].astype(np.float64) - k.want).max() <= k.allow
    with pytest.raises(Exception):
        op(x, k.table, y, k.B, k.H, k.W, 4, k.shift, k.heads, k.d)             # 6 x 9 is no multiple of 4
    with pytest.raises(Exception):
        op(x, k.table, y, k.B, k.H, k.W, k.M, 3, k.heads, k.d)                 # shift >= window
    with pytest.raises(Exception):
        op(x, k.table[:-1].copy(), y, k.B, k.H, k.W, k.M, k.shift, k.heads, k.d)


@pytest.mark.parametrize("M,s,H,W", [(7, 3, 14, 21), (4, 2, 8, 8), (3, 1, 6, 9), (7, 0, 7, 7), (12, 6, 24, 24)])
def test_window_bias_is_the_published_index_and_mask(M, s, H, W):
    heads = 3
    table = np.random.default_rng(M * 10 + s).standard_normal(((2 * M - 1) ** 2, heads)).astype(np.float32)
    bias = window_bias(table, M, s).numpy()
    T = M * M
    Tp = (T + WC.KT - 1) // WC.KT * WC.KT
    assert bias.shape == (4 if s else 1, heads, Tp, Tp) and bias.dtype == np.float32
    # written out pair by pair, not with the packer's vectorised index
    want = np.empty((heads, T, T), np.float32)
    for a in range(T):
        for b in range(T):
            want[:, a, b] = table[(a // M - b // M + M - 1) * (2 * M - 1) + (a % M - b % M + M - 1)]
    np.testing.assert_array_equal(bias[0, :, :T, :T], want)
    assert (bias[:, :, T:, :] == 0).all() and (bias[:, :, :, T:] == 0).all()
    if s:
        mask = WC.published_mask(H, W, M, s).astype(np.float32)          # per window of the H x W map
        nwy, nwx = H // M, W // M
        seen = set()
        for wy in range(nwy):
            for wx in range(nwx):
                cls = 2 * (wy == nwy - 1) + (wx == nwx - 1)
                seen.add(cls)
                np.testing.assert_array_equal(bias[cls, :, :T, :T], want + mask[wy * nwx + wx])
        assert seen == {0, 1, 2, 3}
    with pytest.raises(ValueError):
        window_bias(table, M, M)
    with pytest.raises(ValueError):
        window_bias(table[:-1], M, s)


def _block_by_hand(x, w, n, M, s, h, d):
    """float64 forward of one `winattn` layer `n` on x (B, H, W, C), token by token inside each window."""
    B, H, W, C = x.shape
    x = x.astype(np.float64)
    f = lambda p: w[f"{n}/{p}"].astype(np.float64)
    q = (np.einsum("bhwc,ckd->bhwkd", x, f("query/kernel")) + f("query/bias")) / np.sqrt(d)
    k = np.einsum("bhwc,ckd->bhwkd", x, f("key/kernel")) + f("key/bias")
    v = np.einsum("bhwc,ckd->bhwkd", x, f("value/kernel")) + f("value/bias")
    table = f("relative_position_bias_table")
    region = WC.region_map(H, W, M, s)
    ctx = np.zeros((B, H, W, h, d))
    for wy in range(H // M):
        for wx in range(W // M):
            # rolled-frame positions of the window and the original positions they come from
            pos = [(wy * M + i, wx * M + j) for i in range(M) for j in range(M)]
            org = [((y + s) % H, (x_ + s) % W) for y, x_ in pos]
            for a, (ya, xa) in enumerate(org):
                sc = np.empty((B, h, M * M))
                for b, (yb, xb) in enumerate(org):
                    sc[:, :, b] = (np.einsum("bkd,bkd->bk", q[:, ya, xa], k[:, yb, xb])
                                   + table[(a // M - b // M + M - 1) * (2 * M - 1) + (a % M - b % M + M - 1)])
                    if s and region[pos[a]] != region[pos[b]]:
                        sc[:, :, b] += -100.0
                p = np.exp(sc - sc.max(-1, keepdims=True))
                p /= p.sum(-1, keepdims=True)
                ctx[:, ya, xa] = sum(p[:, :, b, None] * v[:, yb, xb] for b, (yb, xb) in enumerate(org))
    return np.einsum("bhwkd,kdc->bhwc", ctx, f("attention_output/kernel")) + f("attention_output/bias")


@pytest.mark.parametrize("shift", [0, 1])
def test_reference_executor_layer_matches_a_by_hand_forward(shift):
    H, W, C, M, h, d = 6, 9, 8, 3, 2, 4
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (H, W, C)}))
    g.add(Layer("attn", "winattn", ["in"], {"num_heads": h, "key_dim": d, "window": M, "shift": shift,
                                            "use_bias": True}))
    g.output_names = ["attn"]
    w = init_weights(g, 1)
    for n in w:                               # biases and the table of O(1): a dropped one must show
        if n.endswith("/bias") or n.endswith("bias_table"):
            w[n] = np.random.default_rng(len(n)).standard_normal(w[n].shape).astype(np.float32)
    x = np.random.default_rng(3).standard_normal((2, H, W, C)).astype(np.float32)
    got = ReferenceExecutor(g, w)(torch.from_numpy(x)).numpy()
    want = _block_by_hand(x, w, "attn", M, shift, h, d)
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("c", WC.S2D_CASES, ids=str)
def test_space_to_depth_cpu_op_and_reference_are_the_four_slices(c):
    x = WC.s2d_case(c)
    want = WC.ref_space_to_depth(x)
    B, H, W, C = c
    for dy in range(2):                       # the channel block order, spelled out
        for dx in range(2):
            np.testing.assert_array_equal(want[..., (2 * dx + dy) * C:(2 * dx + dy + 1) * C], x[:, dy::2, dx::2])
    y = np.full(want.shape, np.nan, np.float32)
    cpu_executor.native().space_to_depth(x, y)
    np.testing.assert_array_equal(y, want)
    g = Graph("t")
    g.add(Layer("in", "input", [], {"shape": (H, W, C)}))
    g.add(Layer("s2d", "space_to_depth", ["in"], {"block": 2}))
    g.output_names = ["s2d"]
    assert g.layers["s2d"].out_shape == (H // 2, W // 2, 4 * C)
    np.testing.assert_array_equal(ReferenceExecutor(g, {})(torch.from_numpy(x)).numpy(), want)
    with pytest.raises(Exception):
        cpu_executor.native().space_to_depth(x[:, :, :-1].copy(), y)
