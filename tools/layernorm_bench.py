#!/usr/bin/env python3
"""Timings of the LayerNormalization kernels (csrc/kernels/layernorm.hip) on the ConvNeXt-Tiny shapes at batch 32,
hipGraph-timed like tools/gconv_bench.py.  Per shape (rows x C) and precision:

* kernel   `ops/eltwise.py` `layernorm_f32` / `layernorm`, microseconds and GB/s over the compulsory bytes
           (the row read once and written once; gamma / beta are cache-resident and not counted);
* torch    `torch.nn.functional.layer_norm` on the same device tensors: the library reference point;
* split    lanes per row the kernel chose (64 / lanes rows per wave; 0 = the looped path);
* % HBM    the kernel's GB/s against the HBM stream rate of tools/roofline_r50.py.  The small shapes fit the
           256 MiB Infinity Cache and can exceed it.

    python tools/layernorm_bench.py [--reps 50] [--shape ROWS,C ...]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E  # noqa: E402
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops._lib import kernels  # noqa: E402

HBM_BW = 6.3e12            # tools/roofline_r50.py
# rows x C of ConvNeXt-Tiny at batch 32: the four stage maps and the head vector
CONVNEXT_TINY = [(100352, 96), (25088, 192), (6272, 384), (1568, 768), (32, 768)]
EPS = 1e-6


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


def bench(rows, C, dtype, reps):
    bf16 = dtype == torch.bfloat16
    x = torch.randn(rows, C, device="cuda").to(dtype)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda")
    out = torch.empty_like(x)
    if bf16:
        if C % 8:
            raise SystemExit("bf16 rows are stored padded to 8 channels: give a C that is a multiple of 8")
        run = lambda: E.layernorm(x, gamma, beta, out, C, EPS)            # noqa: E731
        lanes = kernels().layernorm_lanes(C // 8)
    else:
        run = lambda: E.layernorm_f32(x, gamma, beta, out, EPS)           # noqa: E731
        lanes = kernels().layernorm_lanes(C // 4) if C % 4 == 0 else 0
    t_k = graph_time_us(run, reps)
    gt, bt = gamma.to(dtype), beta.to(dtype)                              # the library wants one dtype throughout
    t_t = graph_time_us(lambda: F.layer_norm(x, (C,), gt, bt, EPS), reps)
    diff = (out.float() - F.layer_norm(x.float(), (C,), gamma, beta, EPS)).abs().max().item()
    nbytes = 2 * x.numel() * x.element_size()
    gbs = lambda t: nbytes / t / 1e3                                      # noqa: E731
    print(f"{'bf16' if bf16 else 'fp32'} {rows:6d} x {C:4d} [{lanes:2d} lanes/row]: kernel {t_k:7.2f} us "
          f"{gbs(t_k):7.0f} GB/s ({gbs(t_k) * 1e9 / HBM_BW * 100:3.0f}% HBM) | torch {t_t:7.2f} us {gbs(t_t):7.0f} GB/s "
          f"({t_t / t_k:4.2f}x) | max diff vs fp32 torch {diff:.2e}", flush=True)
    return t_k, t_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--shape", action="append", help="ROWS,C (default: the ConvNeXt-Tiny shapes at batch 32)")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else CONVNEXT_TINY
    print(torch.cuda.get_device_name(0))
    for dtype in (torch.float32, torch.bfloat16):
        rows = [bench(r, c, dtype, a.reps) for r, c in shapes]
        print(f"sum: kernel {sum(r[0] for r in rows):.1f} us, torch {sum(r[1] for r in rows):.1f} us")


if __name__ == "__main__":
    main()
