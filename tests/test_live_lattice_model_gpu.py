"""The live-lattice mark in whole models (runtime/plan.py `_mark_live_lattice`, PackedConv.out_lattice): the 3x3
in front of each subsampled 1x1 runs the even-lattice launch of the split F(4x4) Winograd and leaves 3/4 of its
full-size buffer as it was, and the model's logits do not notice.

The zoo's small ResNet on a 100 x 100 image at batch 3 (odd maps 25 / 13 / 7, as in test_subsample_model_gpu.py)
with the marked steps forced onto the whole-K config 221 and the row-split config 238, and ResNet-50 at batch 32
with the configs of the tuning table."""
import pytest
import torch

from bench import PP_LOGIT_RTOL

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import build_resnet, init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C_
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import SliceExecutor

pytestmark = pytest.mark.gpu

RTOL = PP_LOGIT_RTOL["fp32"]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def _marked(ex):
    return [i for i, st in enumerate(ex.steps) if st.p.get("live_lattice")]


def _executor(g, w, batch, off=False):
    mp = pytest.MonkeyPatch()
    mp.delenv("ADAPT_LIVE_LATTICE", raising=False)
    mp.setenv("ADAPT_NO_LIVE_LATTICE", "1" if off else "0")
    try:
        return SliceExecutor(g, w, batch, precision="fp32")
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def tiny():
    g = build_resnet("resnet_tiny", classes=10, input_shape=(100, 100, 3))
    w = init_weights(g, seed=4)
    x = torch.randn(3, 100, 100, 3, generator=torch.Generator().manual_seed(1)).cuda()
    off = _executor(g, w, 3, off=True)
    assert not _marked(off)
    off(x)
    torch.cuda.synchronize()
    return g, w, x, off.logits().clone()


@pytest.mark.parametrize("cfg", [221, 238])
def test_tiny_resnet_odd_maps(tiny, cfg):
    g, w, x, want = tiny
    ex = _executor(g, w, 3)
    marked = _marked(ex)
    assert [ex.steps[i].out for i in marked] == ["conv2_block1_2_relu", "conv3_block1_2_relu", "conv4_block1_2_relu"]
    forced = 0
    for i in marked:
        pc = ex.packed[i]
        assert pc.out_lattice == 2 and ex.steps[i].p["stride"] == 1
        assert tuple(ex.bufs(0)[ex.steps[i].out].shape[1:3]) == tuple(g.layers[ex.steps[i].out].out_shape[:2])
        if C_.kernels().wino4s_lattice_ok(cfg, pc.cin, pc.cout):
            ex.cfg[i] = (cfg, 1)
            forced += 1
    assert forced == len(marked)
    ex._ensure_ws()
    ex(x)
    torch.cuda.synchronize()
    eager = ex.logits().clone()
    assert torch.isfinite(eager).all()
    rel = _rel(eager, want)
    print(f"cfg {cfg}: logits mark on vs off: rel {rel:.3e}, bit-identical {torch.equal(eager, want)}")
    assert rel <= RTOL
    assert torch.equal(eager.argmax(-1), want.argmax(-1))
    ex.capture()
    ex(x)
    torch.cuda.synchronize()
    assert torch.equal(ex.logits(), eager), "graph replay differs from eager"


def test_resnet50_bs32_runs_the_lattice_launch_on_stages_2_and_4():
    g = build_resnet("resnet50")
    w = init_weights(g, seed=0)
    x = torch.randn(32, 224, 224, 3, generator=torch.Generator().manual_seed(0)).cuda()
    off = _executor(g, w, 32, off=True)
    off(x)
    torch.cuda.synchronize()
    want = off.logits().clone()
    ex = _executor(g, w, 32)
    by_out = {ex.steps[i].out: i for i in _marked(ex)}
    assert sorted(by_out) == ["conv2_block3_2_relu", "conv3_block4_2_relu", "conv4_block6_2_relu"]
    for t in ("conv2_block3_2_relu", "conv4_block6_2_relu"):
        i = by_out[t]
        pc, (cfg, ks) = ex.packed[i], ex.cfg[i]
        assert pc.out_lattice == 2
        assert cfg in C_.WINO4S_F32_CFGS and ks == 1, (t, cfg, ks)
        assert C_.kernels().wino4s_lattice_ok(cfg, pc.cin, pc.cout), (t, cfg)
        print(f"{t}: cfg {cfg}, the full launch runs {off.cfg[i]}")
    ex(x)
    torch.cuda.synchronize()
    got = ex.logits()
    rel = _rel(got, want)
    print(f"ResNet-50 bs 32: logits mark on vs off: rel {rel:.3e}, bit-identical {torch.equal(got, want)}")
    assert torch.isfinite(got).all() and rel <= RTOL
    assert torch.equal(got.argmax(-1), want.argmax(-1))
