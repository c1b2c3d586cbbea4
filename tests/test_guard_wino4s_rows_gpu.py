"""Guard-band runs of the row-split F(4x4) Winograd (wino4s_f32.hip cfg ids 238+; tests/guardband.py).

The GEMM writes its half-transformed rows tr[6][tiles][4][N] behind V and wino4s_finish_kernel writes the
output: both between 1 MiB guards, with a workspace of exactly `wino4s_ws_elems(..., cfg)` floats (NaN
payload), once with NaN and once with +inf in the guards of everything read.  Asserted as in
test_guard_f32_gpu.py: guards intact bit for bit, outputs finite and bit-identical between the two poisons,
and within 3e-5 of the float64 reference.  Shapes: (3, 13, 10, 32, 48) (edge tiles, 36 tiles, N = 48: the
configs whose channel block divides it) and (4, 7, 7, 512, 512) (a target layer shape, 32 chunks).
"""
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops._lib import kernels

import guardband as G
from test_guard_f32_gpu import POISONS, _conv_case, _out, _pc_bufs, _rel_max, _scratch, _verify

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(3, 13, 10, 32, 48), (4, 7, 7, 512, 512)])
def test_guard_wino4s_rows(shape):
    B, H, W, Cin, Cout = shape
    c = _conv_case((B, H, W, Cin, Cout, 3, 1, 1, False, 1))
    T = B * ((H + 3) // 4) * ((W + 3) // 4)
    ran = 0
    for cfg in sorted(C.WINO4S_ROW_CFGS):
        if not kernels().wino4s_ok(cfg, Cin, Cout, 1):
            continue
        need = C.wino4s_ws_elems(B, H, W, Cin, Cout, 1, cfg)
        assert need == ((T + 15) // 16) * 16 * Cin * 36 + 24 * T * Cout          # V, then tr[6][T][4][N]
        label = f"cfg {cfg} shape {shape}"
        outs = {}
        for poison in POISONS:
            x, _, pc = c.dev[poison]
            out, ws = _out((B, H, W, Cout)), _scratch(need, poison)
            C.conv_forward_f32(x, pc, out, relu=1, cfg=cfg, ksplit=1, workspace=ws)
            torch.cuda.synchronize()
            G.check(x, *_pc_bufs(pc), out, ws, what=f"[{label}, {poison} poison]")
            outs[poison] = [out.cpu()]
        _verify(label, outs, [c.want], 3e-5, _rel_max)
        ran += 1
    assert ran > 0
