"""Guard-band runs of the grouped convolution (csrc/kernels/gconv_f32.hip), as tests/test_guard_f32_gpu.py does
for the other fp32 kernels: x, packed weights, bias and output between 1 MiB guards (tests/guardband.py).

Each shape is launched twice, with NaN and with +inf in the guards of everything the kernel reads, the output
pre-filled with NaN.  Asserted: every guard intact bit for bit; outputs finite, bit-identical between the two
poison runs, and within 2e-5 of the float64 oracle.  Shapes (tests/gconv_cases.py): the MFMA path on an odd map
with a partial pixel tile and a half-empty channel block (stride 1 and 2), and the generic path's 5x5 / CG 12
and unequal-width cases, so pad rows, partial tiles and partial channel blocks of both paths are met.
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

import gconv_cases as GC
import guardband as G

pytestmark = pytest.mark.gpu

POISONS = (G.NAN, G.INF)
GUARD_SHAPES = [GC.SHAPES[i] for i in (0, 1, 6, 7)]


def _rel1(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


@pytest.mark.parametrize("shape", GUARD_SHAPES, ids=str)
def test_guard_gconv_f32(shape):
    c = GC.case(shape)
    outs = {}
    for poison in POISONS:
        pg = C.pack_gconv_f32(c.kern, c.bias, c.G, c.stride, c.pads, "cuda")
        assert pg.path == ("mfma" if shape in GC.MFMA_SHAPES else "generic")
        pg.w, pg.bias = G.rehome(pg.w, poison, "pg.w"), G.rehome(pg.bias, poison, "pg.bias")
        x = G.guarded(c.x.shape, torch.float32, "cuda", payload=c.x, poison=poison, name="x")
        out = G.guarded(c.out_shape, torch.float32, "cuda", payload=float("nan"), name="out")
        C.gconv_forward_f32(x, pg, out, relu=c.act)
        torch.cuda.synchronize()
        G.check(x, pg.w, pg.bias, out, what=f"[gconv {shape} {pg.path}, {poison} poison]")
        outs[poison] = out.cpu()
    a, b = outs[G.NAN], outs[G.INF]
    assert torch.isfinite(a).all(), "output not finite under NaN read-poison"
    assert torch.isfinite(b).all(), "output not finite under +inf read-poison"
    assert torch.equal(a, b), "output differs between the NaN and +inf poison runs"
    err = _rel1(a.numpy().astype(np.float64), c.want)
    assert err < 2e-5, f"gconv {shape}: rel err {err:.3e}"
