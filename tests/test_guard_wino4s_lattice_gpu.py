"""Guard-band runs of the even-lattice launches of the split F(4x4) Winograd (wino4s_f32.hip, `lattice == 2`;
tests/guardband.py).

Input, packed weights, output and a workspace of exactly `f32_scratch` floats (NaN payload: the launch leaves
the position-5 units of V and part of the row split's tr area unwritten, and must not read them) sit between
1 MiB guards, once with NaN and once with +inf in the guards of everything read.  Asserted: guards intact bit for
bit; the sampled pixels (2i, 2j) finite, bit-identical between the two poisons and within 3e-5 of the float64
reference; every other output pixel still the NaN it was prefilled with.  Shapes: edge tiles with 4 tiles,
3 x 4 tiles over two chunks, and a single tile.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops._lib import kernels

import guardband as G
from test_guard_f32_gpu import POISONS, _conv_case, _out, _pc_bufs, _rel_max, _scratch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(1, 5, 6, 16, 64), (3, 7, 7, 32, 64), (1, 4, 4, 16, 64)])
def test_guard_wino4s_lattice(shape):
    B, H, W, Cin, Cout = shape
    c = _conv_case((B, H, W, Cin, Cout, 3, 1, 1, False, 1))
    want = c.want.reshape(B, H, W, Cout)[:, ::2, ::2]
    rest = np.ones((H, W), bool)
    rest[::2, ::2] = False
    ran = []
    for cfg in sorted(C.WINO4S_F32_CFGS):
        if not kernels().wino4s_lattice_ok(cfg, Cin, Cout):
            continue
        label = f"cfg {cfg} shape {shape}"
        outs = {}
        for poison in POISONS:
            x, _, pc = c.dev[poison]
            pc.out_lattice = 2
            need, nctr = C.f32_scratch(cfg, 1, B, H, W, pc)
            assert need == C.wino4s_ws_elems(B, H, W, Cin, Cout, 1, cfg) and nctr == 0
            out, ws = _out((B, H, W, Cout)), _scratch(need, poison)
            C.conv_forward_f32(x, pc, out, relu=1, cfg=cfg, ksplit=1, workspace=ws)
            torch.cuda.synchronize()
            G.check(x, *_pc_bufs(pc), out, ws, what=f"[{label}, {poison} poison]")
            outs[poison] = out.cpu().numpy()
        a, b = outs[G.NAN], outs[G.INF]
        assert np.isfinite(a[:, ::2, ::2]).all() and np.isfinite(b[:, ::2, ::2]).all(), label
        assert np.array_equal(a[:, ::2, ::2], b[:, ::2, ::2]), f"{label}: differs between the poisons"
        assert np.isnan(a[:, rest]).all() and np.isnan(b[:, rest]).all(), f"{label}: a pixel off the lattice written"
        err = _rel_max(a[:, ::2, ::2].astype(np.float64), want)
        assert err < 3e-5, f"{label}: rel err {err:.3e}"
        ran.append(cfg)
    assert {221, 238} <= set(ran), ran
