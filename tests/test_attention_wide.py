"""Routing of the wide attention heads (csrc/kernels/attention_wide.h) and the zoo's smallest model that takes
them, without a GPU: `attention_kernel` names the kernel per head size, `attention_path` keeps its values, and
`vae_decoder_wide_micro` (a mid-block head of 160 over 64 tokens) compiles to the plan of `vae_decoder_micro` and
runs on the CPU executor within the family's budget (tests/test_groupnorm.py).
"""
import numpy as np
import pytest
import torch

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import (
    BUILDERS, VAE_DECODER, build_model)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops.reference import (
    ReferenceExecutor)
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime import cpu_executor
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.plan import compile_plan

KERNEL = {(64, 64): "mfma", (128, 128): "mfma",
          (144, 16): "wide", (16, 144): "wide", (160, 192): "wide", (256, 256): "wide", (512, 512): "wide",
          (528, 16): "plain", (136, 136): "plain", (24, 24): "plain"}


@pytest.mark.parametrize("head", KERNEL, ids=str)
def test_kernel_per_head_size(head):
    assert A.attention_kernel(*head) == KERNEL[head]
    assert A.attention_path(*head) == ("mfma" if KERNEL[head] == "mfma" else "plain")      # what it gave before
    if KERNEL[head] == "wide":
        wq, wk = A.attention_wide_tiles(*head)
        assert wq >= 16 and wk >= 16 and wq % 16 == 0 and wk % 16 == 0
    else:
        with pytest.raises(ValueError):
            A.attention_wide_tiles(*head)


def test_vae_decoder_wide_micro_has_the_plan_of_the_micro_decoder_and_runs_on_the_cpu():
    assert VAE_DECODER["vae_decoder_wide_micro"] == ((160, 32, 16, 8), 1, 4, (8, 8, 4))
    assert "vae_decoder_wide_micro" in BUILDERS
    g, small = build_model("vae_decoder_wide_micro"), build_model("vae_decoder_micro")
    assert g.layers["mid_attn"].attrs == {"num_heads": 1, "key_dim": 160, "use_bias": True}
    assert A.attention_kernel(160, 160) == "wide"
    # op for op the plan of vae_decoder_micro, but for the 1x1 shortcut conv that the step from 160 to 32 channels
    # puts into the first block of level 1 (the micro decoder's first two levels have one width)
    extra = "up1_block1_shortcut"
    for fp32 in (True, False):
        steps = compile_plan(g, fp32=fp32)
        assert [s.kind for s in steps if s.out == extra] == ["conv"]
        assert [s.kind for s in steps if s.out != extra] == [s.kind for s in compile_plan(small, fp32=fp32)]
    w = init_weights(g, seed=0)
    x = np.random.default_rng(3).standard_normal((2, 8, 8, 4)).astype(np.float32) * 0.18215 * 4.0
    want = ReferenceExecutor(g, w, device="cpu")(torch.from_numpy(x)).numpy()
    got = cpu_executor.CpuExecutor(g, w)(x)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print(f"vae_decoder_wide_micro CpuExecutor rel err {rel:.3e}")
    assert got.shape == (2, 64, 64, 3) and np.isfinite(got).all() and rel <= 1e-3
