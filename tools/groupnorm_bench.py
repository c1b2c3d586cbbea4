#!/usr/bin/env python3
"""Timings of the GroupNormalization kernels (csrc/kernels/groupnorm.hip) on the GN shapes of the Stable Diffusion
VAE decoder at batch 4 (G = 32), hipGraph-timed like tools/layernorm_bench.py.  Per shape (H x W x C) and precision
the four implementations are captured once each and their graphs replayed in turn, round after round:

* kernel          `ops/eltwise.py` `groupnorm_f32` / `groupnorm`, microseconds and GB/s over the compulsory bytes
                  (the map read once and written once; gamma / beta and the partials are not counted);
* kernel + swish  the same launch with the activation folded in;
* torch           `torch.nn.functional.group_norm` on a channels-last tensor of the same values: the library
                  reference point; + `F.silu` for the swish column (a second pass over the map);
* path            what the kernel took: "single" (one launch, x read once), or "split S" / "scalar S" (statistics
                  over S slabs per image, finalize, apply: three launches, x read twice);
* % HBM           the kernel's GB/s against the HBM stream rate of tools/roofline_r50.py.  Byte floor: the time the
                  compulsory bytes take at that rate.  Maps of up to 256 MiB can sit in the Infinity Cache.

    python tools/groupnorm_bench.py [--batch 4] [--reps 10] [--shape H,W,C ...] [--groups 32]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E  # noqa: E402

HBM_BW = 6.3e12            # tools/roofline_r50.py
# H, W, C of the decoder's GroupNormalization inputs
VAE_DECODER = [(64, 64, 512), (128, 128, 512), (256, 256, 512), (256, 256, 256), (512, 512, 256), (512, 512, 128)]
EPS = 1e-5
SWISH = 3                  # csrc/kernels/common.h ActMode


def capture(run, reps):
    """`reps` calls of `run` captured in one hipGraph."""
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


def time_in_turn(graphs, reps, rounds=5):
    """Median microseconds per call of each graph, the graphs replayed in turn within every round."""
    times = [[] for _ in graphs]
    for _ in range(rounds):
        for i, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) / reps * 1e3)
    return [sorted(t)[len(t) // 2] for t in times]


def bench(B, H, W, C, groups, dtype, reps):
    bf16 = dtype == torch.bfloat16
    if bf16 and C % 8:
        raise SystemExit("bf16 rows are stored padded to 8 channels: give a C that is a multiple of 8")
    x = (torch.randn(B, H, W, C, device="cuda") * 1.5 + 0.5).to(dtype)
    gamma = torch.rand(C, device="cuda") + 0.5
    beta = torch.randn(C, device="cuda")
    out = torch.empty_like(x)
    need = E.groupnorm_workspace(B, H * W, C, groups, bf16)
    ws = torch.empty(max(need, 1), dtype=torch.float32, device="cuda")
    if bf16:
        ours = lambda act: (lambda: E.groupnorm(x, gamma, beta, out, C, groups, EPS, act=act, workspace=ws))  # noqa: E731
    else:
        ours = lambda act: (lambda: E.groupnorm_f32(x, gamma, beta, out, groups, EPS, act=act, workspace=ws))  # noqa: E731
    xl = x.permute(0, 3, 1, 2)                                          # NCHW view of the channels-last memory
    assert xl.is_contiguous(memory_format=torch.channels_last)
    gt, bt = gamma.to(dtype), beta.to(dtype)                            # the library wants one dtype throughout
    graphs = [capture(ours(0), reps), capture(ours(SWISH), reps),
              capture(lambda: F.group_norm(xl, groups, gt, bt, EPS), reps),
              capture(lambda: F.silu(F.group_norm(xl, groups, gt, bt, EPS)), reps)]
    t_k, t_ks, t_t, t_ts = time_in_turn(graphs, reps)
    ours(0)()
    ref = F.group_norm(x.float().permute(0, 3, 1, 2).contiguous(), groups, gamma, beta, EPS).permute(0, 2, 3, 1)
    diff = (out.float() - ref).abs().max().item()
    path = E.groupnorm_path(B, H * W, C, groups, bf16)
    slabs = E.groupnorm_slabs(B, H * W, C, groups, bf16)
    how = "single" if path == 2 else f"{'split' if path == 1 else 'scalar'} {slabs}"
    nbytes = 2 * x.numel() * x.element_size()
    gbs = lambda t: nbytes / t / 1e3                                    # noqa: E731
    floor = nbytes / HBM_BW * 1e6
    print(f"{'bf16' if bf16 else 'fp32'} {B}x{H:3d}x{W:3d}x{C:3d} G{groups} [{how:9s} {1 if path == 2 else 2} read]: "
          f"kernel {t_k:8.1f} us {gbs(t_k):6.0f} GB/s ({gbs(t_k) * 1e9 / HBM_BW * 100:3.0f}% HBM, floor {floor:7.1f} us) "
          f"+swish {t_ks:8.1f} us | torch {t_t:8.1f} us {gbs(t_t):6.0f} GB/s ({t_t / t_k:4.2f}x) +silu {t_ts:8.1f} us "
          f"({t_ts / t_ks:4.2f}x) | max diff vs fp32 torch {diff:.2e}", flush=True)
    return t_k, t_ks, t_t, t_ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--groups", type=int, default=32)
    ap.add_argument("--shape", action="append", help="H,W,C (default: the VAE decoder's GroupNormalization shapes)")
    ap.add_argument("--dtype", default="both", choices=["both", "fp32", "bf16"])
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(",")) for s in a.shape] if a.shape else VAE_DECODER
    print(torch.cuda.get_device_name(0))
    for dtype in (torch.float32, torch.bfloat16):
        if a.dtype != "both" and (a.dtype == "bf16") != (dtype == torch.bfloat16):
            continue
        rows = [bench(a.batch, h, w, c, a.groups, dtype, a.reps) for h, w, c in shapes]
        print(f"sum: kernel {sum(r[0] for r in rows):.1f} us, +swish {sum(r[1] for r in rows):.1f} us, "
              f"torch {sum(r[2] for r in rows):.1f} us, torch +silu {sum(r[3] for r in rows):.1f} us")


if __name__ == "__main__":
    main()
