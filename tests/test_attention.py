"""The attention core without a GPU: the case list against the kernel's paths, the oracle's own sanity, and the
native CPU op `attention` on every case within the allowance of tests/attention_cases.py.

The HIP kernels: tests/test_attention_gpu.py, tests/test_guard_attention_gpu.py.
"""
import numpy as np
import pytest

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor

import attention_cases as AC


def test_the_cases_meet_every_path():
    QT, KT = AC.QT, AC.KT
    assert QT % 16 == 0 and KT % 16 == 0 and QT >= 16 and KT >= 16
    plain = [c for c in AC.CASES if AC.case(c).path == "plain"]
    mfma = [c for c in AC.CASES if AC.case(c).path == "mfma"]
    assert len(plain) >= 3 and len(mfma) >= 10
    assert {(c[3], c[4]) for c in mfma} >= {(16, 16), (32, 16), (64, 64), (128, 128)}
    assert {(c[3], c[4]) for c in plain} >= {(24, 24), (8, 40)}
    ts = {c[1] for c in mfma}
    assert ts >= {1, KT - 1, KT, KT + 1, QT - 1, QT, QT + 1, 197}
    # every tail kind: less than one key tile; whole tiles; a ragged last key tile after whole ones; a ragged
    # last query tile after a whole one; a last query tile whose trailing waves hold no query at all
    assert any(t < KT for t in ts) and any(t % KT == 0 for t in ts) and any(t > KT and t % KT for t in ts)
    assert any(t > QT and t % QT for t in ts) and any(t > QT and t % QT and t % QT <= QT - 16 for t in ts)
    # more than one image with T off both tiles, on both paths; one head and several; d != dv
    assert any(c[0] == 2 and c[1] % KT and c[1] % QT for c in mfma) and any(c[0] == 3 and c[1] % KT for c in mfma)
    assert any(c[0] > 1 and c[1] % 64 for c in plain)
    assert {c[2] for c in AC.CASES} >= {1, 3} and any(c[3] != c[4] for c in mfma) and any(c[3] != c[4] for c in plain)
    # the three register sizes of the MFMA kernel
    assert {32 if max(c[3], c[4]) <= 32 else 64 if max(c[3], c[4]) <= 64 else 128 for c in mfma} == {32, 64, 128}
    # widths that the bf16 layout pads on both sides
    assert any(AC.widths(c)[0] % 8 and AC.widths(c)[1] % 8 for c in plain)
    # the softmax probes span more than two key tiles and really reach scores near 100
    probes = [c for c in AC.CASES if c[5]]
    assert {c[5] for c in probes} == {"ascending", "descending", "dominant"}
    for c in probes:
        k = AC.case(c)
        q, kk, _ = AC.split(k.qkv.astype(np.float64), k.B, k.T, k.heads, k.d, k.dv)
        s = np.einsum("bqhd,bkhd->bhqk", q, kk)
        assert k.T > 2 * KT and 80 < s.max() < 130
        arg = s.argmax(-1)
        if c[5] == "ascending":
            assert (arg >= 2 * KT).all()
        elif c[5] == "descending":
            assert (arg < KT).all()
        else:
            assert len(np.unique(arg // KT)) == 3 and (np.sort(s, -1)[..., -1] - np.sort(s, -1)[..., -2]).min() > 20
    assert set(AC.GUARD_CASES) <= set(AC.CASES) and 4 <= len(AC.GUARD_CASES) <= 6


def test_a_softmax_without_the_maximum_would_fail_the_probes():
    """exp(100) overflows fp32: the probes separate a kernel that subtracts the row maximum from one that does not."""
    for c in (c for c in AC.CASES if c[5]):
        k = AC.case(c)
        q, kk, v = AC.split(k.qkv, k.B, k.T, k.heads, k.d, k.dv)
        with np.errstate(over="ignore", invalid="ignore"):
            p = np.exp(np.einsum("bqhd,bkhd->bhqk", q, kk, dtype=np.float32))
            y = np.einsum("bhqk,bkhd->bqhd", p / p.sum(-1, keepdims=True), v).reshape(k.want.shape)
        assert not (np.abs(y - k.want) <= k.allow).all()


@pytest.mark.parametrize("c", AC.CASES, ids=str)
def test_cpu_attention_matches_float64_oracle(c):
    k = AC.case(c)
    y = np.full(k.want.shape, np.nan, np.float32)
    cpu_executor.native().attention(k.qkv, y, k.B, k.T, k.heads, k.d, k.dv)
    err = np.abs(y.astype(np.float64) - k.want).max()
    print(f"cpu attention {c} [{k.path}]: e_ref {k.e_ref:.3e}, max err {err:.3e}, allowance {k.allow:.3e}")
    assert np.isfinite(y).all() and err <= k.allow


def test_cpu_attention_takes_padded_rows_and_zeroes_the_output_padding():
    c = (2, 19, 3, 6, 5, None)
    k = AC.case(c)
    w_in, w_out = AC.widths(c)
    x = np.full((k.B * k.T, w_in + 5), np.nan, np.float32)          # the padding is never read
    x[:, :w_in] = k.qkv
    y = np.full((k.B * k.T, w_out + 1), np.nan, np.float32)
    cpu_executor.native().attention(x, y, k.B, k.T, k.heads, k.d, k.dv)
    assert (y[:, w_out:] == 0).all() and np.abs(y[:, :w_out].astype(np.float64) - k.want).max() <= k.allow
    with pytest.raises(Exception):
        cpu_executor.native().attention(k.qkv[:, :-1].copy(), y, k.B, k.T, k.heads, k.d, k.dv)


@pytest.mark.parametrize("c", AC.POSEMBED_CASES, ids=str)
def test_posembed_oracle_shapes(c):
    k = AC.posembed_case(c)
    out = AC.ref_posembed(k.x, k.cls, k.pos)
    assert out.shape == (k.B, 1, k.T + k.ct, k.C)
    np.testing.assert_array_equal(out[:, 0, k.ct], k.x.reshape(k.B, -1, k.C)[:, 0] + k.pos[k.ct])
