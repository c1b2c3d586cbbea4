"""The lattice pass in a whole model: the zoo's small ResNet (one block per stage) in fp32 on a 100 x 100 image, so
the stage boundaries are odd maps (25 -> 13 -> 7 -> 4) and every compact tensor drops a last row and column.
Run twice: the 1x1 pass alone (ADAPT_SUBSAMPLE_3X3=0) and with the 3x3 in front of each subsampled 1x1 strided
too (=1; on these odd maps it keeps its bottom / right pad)."""
import numpy as np
import pytest
import torch

from bench import PP_LOGIT_RTOL

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.slicer import partition, subgraph
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import build_resnet, init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import SliceExecutor

pytestmark = pytest.mark.gpu

BATCH = 3
RTOL = PP_LOGIT_RTOL["fp32"]
SAMPLED = {"conv2_block1_out": (13, 13), "conv3_block1_out": (7, 7), "conv4_block1_out": (4, 4)}
FRONT = {"conv2_block1_2_relu": (13, 13), "conv3_block1_2_relu": (7, 7), "conv4_block1_2_relu": (4, 4)}


@pytest.fixture(scope="module")
def model():
    g = build_resnet("resnet_tiny", classes=10, input_shape=(100, 100, 3))
    w = init_weights(g, seed=4)
    x = torch.randn(BATCH, 100, 100, 3, generator=torch.Generator().manual_seed(1)).cuda()
    return g, w, x


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.fixture(scope="module", params=["0", "1"], ids=["1x1", "1x1+3x3"])
def unsliced(model, request):
    """Logits of the unsliced model with the pass on: eager, then replayed from the hipGraph."""
    g, w, x = model
    mp = pytest.MonkeyPatch()
    mp.setenv("ADAPT_SUBSAMPLE_3X3", request.param)
    try:
        ex = SliceExecutor(g, w, BATCH, precision="fp32")
    finally:
        mp.undo()
    want = {**SAMPLED, **(FRONT if request.param == "1" else {})}
    assert ex._compact == want
    for t, hw in want.items():
        assert tuple(ex.bufs(0)[t].shape) == (BATCH,) + hw + (g.layers[t].out_shape[-1],)
    ex(x)
    torch.cuda.synchronize()
    eager = ex.logits().clone()
    probs = ex.output_buf(ex.outputs[0]).clone()
    ex.capture()
    ex(x)
    torch.cuda.synchronize()
    return ex, eager, probs, ex.logits().clone(), ex.output_buf(ex.outputs[0]).clone()


def test_pass_on_matches_pass_off(model, unsliced, monkeypatch):
    g, w, x = model
    _, eager, probs, _, _ = unsliced
    monkeypatch.setenv("ADAPT_NO_SUBSAMPLE", "1")
    off = SliceExecutor(g, w, BATCH, precision="fp32")
    assert not off._compact and [f"{s.kind} {s.out}" for s in off.steps] == [f"{s.kind} {s.out}" for s in unsliced[0].steps]
    off(x)
    torch.cuda.synchronize()
    want = off.logits()
    assert torch.isfinite(eager).all()
    rel = _rel(eager, want)
    print(f"logits pass on vs off: rel {rel:.3e}, bit-identical {torch.equal(eager, want)}")
    assert rel <= RTOL
    assert torch.equal(eager.argmax(-1), want.argmax(-1))
    assert _rel(probs, off.output_buf(off.outputs[0])) <= RTOL


def test_graph_replay_is_bit_identical_to_eager(unsliced):
    _, eager, probs, replay, replay_probs = unsliced
    assert torch.equal(eager, replay) and torch.equal(probs, replay_probs)


@pytest.mark.parametrize("cut", ["conv2_block1_out", "conv3_block1_1_conv"])
def test_sliced_model_matches_unsliced(model, unsliced, cut, monkeypatch):
    """A cut at a subsampled tensor's name, and the multi-tensor frontier beside it: the tensor crosses the cut
    at full size, and the slices (compiled with both steps of the pass) give the unsliced model's logits."""
    g, w, x = model
    monkeypatch.setenv("ADAPT_SUBSAMPLE_3X3", "1")
    _, eager, _, _, _ = unsliced
    feed = {g.input: x}
    last = None
    for sl in partition(g, [cut]):
        sg = subgraph(g, sl)
        ex = SliceExecutor(sg, w, BATCH, outputs=sg.output_names, precision="fp32")
        assert "conv2_block1_out" not in ex._compact
        for t in sl.inputs + sl.outputs:
            if t in g.layers and len(g.layers[t].out_shape) == 3:
                assert tuple(ex.shape_of(t)[1:3]) == tuple(g.layers[t].out_shape[:2])
        out = ex.run({n: feed[n] for n in sg.input_names})
        torch.cuda.synchronize()
        feed.update({n: t.clone() for n, t in out.items()})
        last = ex
    got = last.logits()
    rel = _rel(got, eager)
    print(f"cut {cut}: logits vs unsliced rel {rel:.3e}")
    assert torch.isfinite(got).all() and rel <= RTOL
    assert np.array_equal(got.argmax(-1).cpu().numpy(), eager.argmax(-1).cpu().numpy())
