#!/usr/bin/env python3
"""Per-layer timings of the grouped 3x3 convolutions of ResNeXt-50 (32x4d), hipGraph-timed like
tools/conv_bench_f32.py.  Per shape, in microseconds:

* gconv    csrc/kernels/gconv_f32.hip through ops/conv.py `gconv_forward_f32` (conv + bias + ReLU);
* dense    the only alternative the tree had: the same layer expanded to a dense block-diagonal HWIO kernel
           and run as a one-conv fp32 plan by SliceExecutor, i.e. `conv_forward_f32` with the config the
           executor chooses for it (tuning table, else its default rule);
* torch    `torch.nn.functional.conv2d(groups=G)` in fp32 channels-last: the library reference point,
           used the way tools/gemm_ceiling.py uses hipBLASLt (conv + bias, no ReLU);
* floor    input + output activation bytes over the HBM stream rate of tools/roofline_r50.py.

    python tools/gconv_bench.py [--batch 32] [--reps 20] [--shape H,W,C,stride ...]
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.graph.ir import Graph, Layer  # noqa: E402
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C  # noqa: E402
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import SliceExecutor  # noqa: E402

HBM_BW = 6.3e12            # tools/roofline_r50.py
GROUPS = 32
# (H, W, C, stride): the seven grouped 3x3 shapes of ResNeXt-50, input map -> C channels
RESNEXT50 = [(56, 56, 128, 1), (56, 56, 256, 2), (28, 28, 256, 1), (28, 28, 512, 2), (14, 14, 512, 1),
             (14, 14, 1024, 2), (7, 7, 1024, 1)]


def graph_time_us(run, reps, rounds=5):
    """Median microseconds per call of `run`, `reps` calls captured in one hipGraph."""
    run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(reps):
            run()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) / reps * 1e3)
    return sorted(times)[len(times) // 2]


def dense_executor(B, H, W, Cc, stride, kern_dense, bias):
    g = Graph("gconv_as_dense")
    g.add(Layer("in", "input", [], {"shape": (H, W, Cc), "stands_for": "activation"}))
    g.add(Layer("pad", "zeropad", ["in"], {"pad": ((1, 1), (1, 1))}))
    g.add(Layer("c", "conv", ["pad"], {"filters": Cc, "kernel": (3, 3), "stride": stride, "padding": "valid",
                                      "use_bias": True, "activation": "relu"}))
    g.output_names = ["c"]
    ex = SliceExecutor(g, {"c/kernel": kern_dense, "c/bias": bias}, batch=B, device="cuda:0", precision="fp32")
    assert [st.kind for st in ex.steps] == ["conv"], [st.kind for st in ex.steps]
    return ex


def bench(B, H, W, Cc, stride, reps):
    cg = Cc // GROUPS
    rng = np.random.default_rng(0)
    kern = (rng.standard_normal((3, 3, cg, Cc)) / math.sqrt(9 * cg)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(Cc)).astype(np.float32)
    pads = ((1, 1), (1, 1))
    x = torch.randn(B, H, W, Cc, device="cuda")
    pg = C.pack_gconv_f32(kern, bias, GROUPS, stride, pads, "cuda")
    OH, OW = pg.out_hw(H, W)
    out = torch.empty(B, OH, OW, Cc, device="cuda")
    t_g = graph_time_us(lambda: C.gconv_forward_f32(x, pg, out, relu=1), reps)

    dense = np.zeros((3, 3, Cc, Cc), np.float32)
    for gi in range(GROUPS):
        dense[:, :, gi * cg:(gi + 1) * cg, gi * cg:(gi + 1) * cg] = kern[..., gi * cg:(gi + 1) * cg]
    ex = dense_executor(B, H, W, Cc, stride, dense, bias)
    ex.sets[0]["in"].copy_(x)
    t_d = graph_time_us(lambda: ex._launch(0), reps)
    agree = (ex.sets[0]["c"] - out).abs().max().item()
    cfg = ex.cfg.get(0)
    del ex

    xt = x.permute(0, 3, 1, 2)                                   # NCHW view of NHWC memory: channels-last
    wt = torch.from_numpy(kern).cuda().permute(3, 2, 0, 1).contiguous(memory_format=torch.channels_last)
    bt = torch.from_numpy(bias).cuda()
    try:
        t_t = graph_time_us(lambda: F.conv2d(xt, wt, bt, stride=stride, padding=1, groups=GROUPS), reps)
    except RuntimeError as e:                                    # a library path that cannot be captured
        print(f"  torch conv2d not graph-timed: {str(e).splitlines()[0]}")
        t_t = float("nan")
    floor = (x.numel() + out.numel()) * 4 / HBM_BW * 1e6
    flop = 2.0 * B * OH * OW * Cc * 9 * cg
    print(f"B{B} {H}x{W}x{Cc} s{stride} CG{cg} [{pg.path}]: gconv {t_g:8.1f} us ({flop / t_g / 1e6:5.1f} TF/s useful)"
          f" | dense cfg {cfg} {t_d:8.1f} us ({t_d / t_g:5.1f}x) | torch {t_t:8.1f} us ({t_t / t_g:4.2f}x)"
          f" | traffic floor {floor:6.1f} us ({floor / t_g * 100:3.0f}%) | max diff vs dense {agree:.2e}", flush=True)
    return t_g, t_d, t_t, floor


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", action="append", help="H,W,C,stride (default: the seven ResNeXt-50 shapes)")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else RESNEXT50
    print(torch.cuda.get_device_name(0))
    rows = [bench(a.batch, *s, a.reps) for s in shapes]
    print(f"sum: gconv {sum(r[0] for r in rows):.1f} us, dense {sum(r[1] for r in rows):.1f} us, "
          f"torch {sum(r[2] for r in rows):.1f} us, floor {sum(r[3] for r in rows):.1f} us")


if __name__ == "__main__":
    main()
