#!/usr/bin/env python3
"""Per-layer timings of transposed convolutions and upsampling, hipGraph-timed like tools/gconv_bench.py.
Per deconv shape, in one process, the three implementations interleaved round by round, in microseconds:

* deconv   csrc/kernels/deconv_f32.hip through ops/conv.py `deconv_forward_f32` (deconv + bias + ReLU);
* torch    `torch.nn.functional.conv_transpose2d` in fp32 channels-last plus what 'same' needs (a slice of the
           full frame): the library reference point (deconv + bias, no ReLU);
* stuffed  the only alternative the tree had: the input spread with s - 1 zeros between pixels and padded, and
           a stride-1 dense conv with the flipped kernel run as a one-conv fp32 plan by SliceExecutor, i.e.
           `conv_forward_f32` with the config the executor chooses.  The zero-stuffing itself is NOT timed
           (the stuffed tensor is prepared once), which flatters this column.

TF/s is on the true MAC count, H * W * kh * kw * Cin * Cout per image, for all three.  Then nearest and bilinear
UpSampling2D(2) against `F.interpolate`.

    python tools/deconv_bench.py [--batch 32] [--reps 20] [--rounds 5]
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
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E  # noqa: E402
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import SliceExecutor  # noqa: E402

# (H, W, Cin, Cout, k, s): the four transposed convs of `unet` (256x256 input), then a 3x3 and a 4x4 stride 2
SHAPES = [(16, 16, 1024, 512, 2, 2), (32, 32, 512, 256, 2, 2), (64, 64, 256, 128, 2, 2), (128, 128, 128, 64, 2, 2),
          (32, 32, 256, 128, 3, 2), (32, 32, 256, 128, 4, 2)]
# (H, W, C): the inputs of the four UpSampling2D(2) of `unet_bilinear`
UPSAMPLE = [(16, 16, 1024), (32, 32, 512), (64, 64, 256), (128, 128, 128)]


def capture(run, reps):
    """A hipGraph of `reps` calls of `run`, warmed up."""
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
    return g


def interleaved_us(runs, reps, rounds):
    """Median microseconds per call of each of `runs` (name -> callable, None entries skipped): every round
    replays each implementation's graph once, in turn."""
    graphs = {}
    for name, run in runs.items():
        try:
            graphs[name] = capture(run, reps)
        except RuntimeError as e:                                # a library path that cannot be captured
            print(f"  {name} not graph-timed: {str(e).splitlines()[0]}")
    times = {name: [] for name in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps * 1e3)
    return {name: sorted(times[name])[rounds // 2] if times.get(name) else float("nan") for name in runs}


def stuffed_executor(B, rows, cols, cin, cout, k, kern_flipped, bias):
    g = Graph("deconv_as_stuffed_conv")
    g.add(Layer("in", "input", [], {"shape": (rows, cols, cin), "stands_for": "activation"}))
    g.add(Layer("c", "conv", ["in"], {"filters": cout, "kernel": (k, k), "stride": 1, "padding": "valid",
                                      "use_bias": True, "activation": "relu"}))
    g.output_names = ["c"]
    ex = SliceExecutor(g, {"c/kernel": kern_flipped, "c/bias": bias}, batch=B, device="cuda:0", precision="fp32")
    assert [st.kind for st in ex.steps] == ["conv"], [st.kind for st in ex.steps]
    return ex


def bench_deconv(B, H, W, cin, cout, k, s, reps, rounds):
    rng = np.random.default_rng(0)
    taps = (-(-k // s)) ** 2
    kern = (rng.standard_normal((k, k, cin, cout)) / math.sqrt(taps * cin)).astype(np.float32)     # (kh, kw, Cin, Cout)
    bias = (0.1 * rng.standard_normal(cout)).astype(np.float32)
    x = torch.randn(B, H, W, cin, device="cuda")
    pd = C.pack_deconv_f32(kern, bias, s, "same", "cuda")
    OH, OW = H * s, W * s
    out = torch.empty(B, OH, OW, cout, device="cuda")
    pb = pd.pad_t

    xt = x.permute(0, 3, 1, 2)                                   # NCHW view of NHWC memory: channels-last
    wt = torch.from_numpy(kern).cuda().permute(2, 3, 0, 1).contiguous(memory_format=torch.channels_last)
    bt = torch.from_numpy(bias).cuda()

    def torch_run():
        y = F.conv_transpose2d(xt, wt, bt, stride=s)
        return y[:, :, pb:pb + OH, pb:pb + OW] if y.shape[2] != OH else y

    rows, cols = OH + k - 1, OW + k - 1
    z = torch.zeros(B, rows, cols, cin, device="cuda")
    t0 = k - 1 - pb
    z[:, t0:t0 + (H - 1) * s + 1:s, t0:t0 + (W - 1) * s + 1:s] = x
    ex = stuffed_executor(B, rows, cols, cin, cout, k, np.ascontiguousarray(kern[::-1, ::-1]), bias)
    ex.sets[0]["in"].copy_(z)
    t = interleaved_us({"deconv": lambda: C.deconv_forward_f32(x, pd, out, relu=1), "torch": torch_run,
                        "stuffed": lambda: ex._launch(0)}, reps, rounds)
    agree = (ex.sets[0]["c"] - out).abs().max().item()
    vs_torch = (torch_run().permute(0, 2, 3, 1).clamp_min(0) - out).abs().max().item()
    cfg = ex.cfg.get(0)
    del ex
    flop = 2.0 * B * H * W * k * k * cin * cout
    tf = {n: flop / v / 1e6 for n, v in t.items()}
    print(f"B{B} {H}x{W}x{cin}->{cout} k{k} s{s} [{pd.path}]: deconv {t['deconv']:8.1f} us ({tf['deconv']:5.1f} TF/s)"
          f" | torch {t['torch']:8.1f} us ({tf['torch']:5.1f} TF/s, {t['torch'] / t['deconv']:5.2f}x)"
          f" | stuffed cfg {cfg} {t['stuffed']:8.1f} us ({tf['stuffed']:5.1f} TF/s, {t['stuffed'] / t['deconv']:5.2f}x)"
          f" | max diff vs stuffed {agree:.2e}, vs torch {vs_torch:.2e}", flush=True)
    return t


def bench_upsample(B, H, W, Cc, reps, rounds):
    x = torch.randn(B, H, W, Cc, device="cuda")
    out = torch.empty(B, 2 * H, 2 * W, Cc, device="cuda")
    xt = x.permute(0, 3, 1, 2)
    for bilinear, mode in ((False, "nearest"), (True, "bilinear")):
        kw = {"align_corners": False} if bilinear else {}
        t = interleaved_us({"ours": lambda: E.upsample(x, out, 2, bilinear),
                            "torch": lambda: F.interpolate(xt, scale_factor=2, mode=mode, **kw)}, reps, rounds)
        diff = (F.interpolate(xt, scale_factor=2, mode=mode, **kw).permute(0, 2, 3, 1) - out).abs().max().item()
        gbs = (x.numel() + out.numel()) * 4 / t["ours"] / 1e3
        print(f"B{B} {H}x{W}x{Cc} x2 {mode:8s}: ours {t['ours']:8.1f} us ({gbs:6.0f} GB/s) | F.interpolate "
              f"{t['torch']:8.1f} us ({t['torch'] / t['ours']:5.2f}x) | max diff {diff:.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    for shp in SHAPES:
        bench_deconv(a.batch, *shp, a.reps, a.rounds)
    for shp in UPSAMPLE:
        bench_upsample(a.batch, *shp, a.reps, a.rounds)


if __name__ == "__main__":
    main()
