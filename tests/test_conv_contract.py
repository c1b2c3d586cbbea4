"""The conv launch contract against a recording of the functions it replaced.

tests/golden/conv_contract.json was recorded with the per-family if-chains this API replaced
(`f32_cfg_supported` / `cfg_supported`, `workspace_elems_f32` / `wino4s_ws_elems` / `f32_counter_elems`,
`workspace_elems` / `sk_plan`, and the candidate loops of `SliceExecutor.autotune_f32` / `autotune` copied
verbatim), on the problems below.  Per problem it holds the sorted supported config ids, the ordered
`(cfg, ksplit)` candidates the tuner times, and the `(workspace floats, int32 counters)` of each; `extra` holds
the scratch of the ids no candidate list reaches (ablation, measurement-only and untuned configs).  The tuner
keeps the first of equal timings, so the candidate order is behaviour: everything is compared with `==`.

Only host functions of the kernel library run here (launch plans and size formulas): no GPU.
"""
import json
import os

import numpy as np
import pytest

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_contract.json")

# name -> (dtype, (B, H, W, Cin, Cout, k, stride, pad), fused residual, n_split)
PROBLEMS = {
    # ResNet-50 bs=32, one per family trigger
    "f32 s2 3x3": ("f32", (32, 56, 56, 64, 64, 3, 1, 1), False, 0),
    "f32 s4 3x3": ("f32", (32, 14, 14, 256, 256, 3, 1, 1), False, 0),
    "f32 s4 3x3 res": ("f32", (32, 14, 14, 256, 256, 3, 1, 1), True, 0),
    "f32 s5 3x3": ("f32", (32, 7, 7, 512, 512, 3, 1, 1), False, 0),
    "f32 s2 1x1": ("f32", (32, 56, 56, 256, 64, 1, 1, 0), False, 0),
    "f32 s4 1x1": ("f32", (32, 14, 14, 1024, 256, 1, 1, 0), False, 0),
    "f32 s4 1x1/2": ("f32", (32, 28, 28, 512, 1024, 1, 2, 0), False, 0),
    "f32 stem": ("f32", (32, 224, 224, 3, 64, 7, 2, 3), False, 0),
    "f32 merged 1x1/2": ("f32", (32, 56, 56, 256, 512 + 128, 1, 2, 0), False, 512),
    # the small guard-band shapes
    "f32 guard 3x3 a": ("f32", (1, 5, 3, 16, 96, 3, 1, 1), False, 0),
    "f32 guard 3x3 b": ("f32", (2, 9, 7, 32, 96, 3, 1, 1), True, 0),
    "f32 guard 1x1": ("f32", (1, 5, 3, 32, 36, 1, 1, 0), True, 0),
    "bf16 s2 3x3": ("bf16", (32, 56, 56, 64, 64, 3, 1, 1), False, 0),
    "bf16 s4 3x3": ("bf16", (32, 14, 14, 256, 256, 3, 1, 1), False, 0),
    "bf16 s4 1x1": ("bf16", (32, 14, 14, 1024, 256, 1, 1, 0), False, 0),
    "bf16 s4 1x1/2": ("bf16", (32, 28, 28, 512, 1024, 1, 2, 0), False, 0),
}


def make_pc(name):
    """The problem's PackedConv on the CPU (zero weights: only shapes and which packings exist matter)."""
    dtype, (B, H, W, Cin, Cout, k, s, p), _, n_split = PROBLEMS[name]
    pack = C.pack_conv_f32 if dtype == "f32" else C.pack_conv
    pc = pack(np.zeros((k, k, Cin, Cout), np.float32), np.zeros(Cout, np.float32), s, ((p, p), (p, p)), "cpu")
    pc.n_split = n_split
    return pc


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_fixture_covers_the_problems(golden):
    assert sorted(golden["problems"]) == sorted(PROBLEMS)


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_contract_matches_recording(golden, name):
    dtype, (B, H, W, *_), residual, _ = PROBLEMS[name]
    want = golden["problems"][name]
    pc = make_pc(name)
    families, candidates, scratch = ((C.F32_FAMILIES, C.f32_candidates, C.f32_scratch) if dtype == "f32" else
                                     (C.BF16_FAMILIES, C.bf16_candidates, C.bf16_scratch))
    supported = sorted(cfg for fam in families for cfg in fam.cfgs if fam.supported(cfg, pc, residual))
    assert supported == want["supported"]
    cands = [list(ck) for ck in candidates(B, H, W, pc, residual)]
    assert cands == [row[:2] for row in want["candidates"]]
    OH, OW = pc.out_hw(H, W)
    M, N = B * OH * OW, pc.cout
    for cfg, ks, ws, ctr in want["candidates"]:
        assert list(scratch(cfg, ks, B, H, W, pc)) == [ws, ctr], f"cfg {cfg} ksplit {ks}"
        # the (M, N, Kpad) helpers of old answer from the same records
        if dtype == "bf16":
            assert C.workspace_elems(M, N, pc.Kpad, cfg, ks) == ws
        elif cfg in C.WINO4S_F32_CFGS:
            with pytest.raises(ValueError):
                C.workspace_elems_f32(M, N, pc.Kpad, cfg, ks)
        else:
            assert C.workspace_elems_f32(M, N, pc.Kpad, cfg, ks) == ws
        if dtype == "f32":
            assert C.f32_counter_elems(cfg, ks, B, H, W, OH, OW, N, pc.Kpad) == ctr


def test_scratch_of_untuned_ids(golden):
    """Ablation, measurement-only and untuned ids: sized by the same `scratch`, never candidates."""
    never = set(C.WINO_F32_ABLATE) | C.WINO_MEASURE_CFGS | C.F32_UNTUNED
    assert {row[1] for row in golden["extra"]} == never
    pcs = {}
    for name, cfg, ks, ws, ctr in golden["extra"]:
        pc = pcs.setdefault(name, make_pc(name))
        B, H, W = PROBLEMS[name][1][:3]
        assert list(C.f32_scratch(cfg, ks, B, H, W, pc)) == [ws, ctr], f"{name}: cfg {cfg} ksplit {ks}"
        assert (cfg, ks) not in set(C.f32_candidates(B, H, W, pc, PROBLEMS[name][2]))


def test_ksplits_are_unpruned():
    """`ksplits` is what a family knows; what the tuner leaves out of it is `f32_candidates`' business."""
    pc = make_pc("f32 s2 3x3")
    assert C.f32_family(80).ksplits(80, 32, 56, 56, pc) == (1, 2, 4, 8, 16, -2, -4)
    assert (80, -2) not in set(C.f32_candidates(32, 56, 56, pc, False))      # 1568 blocks: the CUs are full


def test_unknown_config_ids():
    assert not C.cfg_supported(9999, make_pc("bf16 s2 3x3"), False) and not C.f32_cfg_supported(9999, 64, 64)
    for lookup in (C.f32_family, C.bf16_family):
        with pytest.raises(ValueError):
            lookup(9999)
