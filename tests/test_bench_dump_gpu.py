"""`bench.py --dump-outputs` on the MI355X: a plain run (no `--full`) times
exactly `--steps` steps, reports `ms_per_step`, skips the bf16 companion and
leaves the outputs of its last timed step as float32 .npy files that match the
fp32 PyTorch oracle on the same seeded input."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models import resnet, zoo
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import ReferenceExecutor

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL, BATCH = "resnet_tiny", 4
# the fp32 path's budget against the fp32 oracle (the smoke run's: logits within 1e-4 of their scale)
LOGIT_BUDGET = 1e-4


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_plain_run_dumps_the_last_step_outputs(tmp_path, capsys):
    b = _bench()
    out = tmp_path / "dump"
    b.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--model", MODEL, "--batch", str(BATCH),
            "--dump-outputs", str(out)])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["dtype"] == "fp32" and rec["unit"] == "images/s"
    assert rec["ms_per_step"] > 0 and rec["higher_is_better"] is True
    assert rec["value"] == pytest.approx(BATCH / (rec["ms_per_step"] * 1e-3), rel=1e-3)
    assert "value_bf16" not in rec                       # the companion timing needs --full

    g = zoo.build_model(MODEL)
    w = resnet.init_weights(g, seed=0)
    assert sorted(p.name for p in out.iterdir()) == sorted([f"{o}.npy" for o in g.output_names] + ["logits.npy"])
    probs = np.load(out / f"{g.output_names[0]}.npy")
    logits = np.load(out / "logits.npy")
    assert probs.dtype == np.float32 and logits.dtype == np.float32
    assert probs.shape == logits.shape == (BATCH, 1000)
    assert np.isfinite(probs).all() and np.allclose(probs.sum(-1), 1.0, atol=1e-4)

    x = b.synthetic_input(BATCH, g.layers[g.input].out_shape, 0, torch.device("cuda", 0))
    feat = ReferenceExecutor(g, w, device="cpu").run({g.input: x.cpu()}, outputs=["avg_pool"])["avg_pool"]
    want = feat.double().numpy() @ w["predictions/kernel"].astype(np.float64) + w["predictions/bias"]
    rel = np.abs(logits - want).max() / np.abs(want).max()
    print(f"dumped logits vs fp32 oracle: rel err {rel:.3e} (budget {LOGIT_BUDGET:.0e})")
    assert rel <= LOGIT_BUDGET
    assert (logits.argmax(-1) == probs.argmax(-1)).all()
