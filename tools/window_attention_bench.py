#!/usr/bin/env python3
"""Timings of the Swin window attention core, hipGraph-timed like tools/attention_bench.py.  Per shape, in one
process, the implementations replayed in turn round by round, median of the rounds, in microseconds:

* ours     csrc/kernels/window_attention.hip through ops/attention.py `window_attention`, fp32 activations, on
           the NHWC [B * H * W][3 h d] map the QKV projection writes, bias and mask packed once (not timed);
* ours16   the same kernel on bf16 activations (fp32 MFMA math);
* library  the library composition in fp32 from the same map: `torch.roll`, the window partition (reshape /
           permute into [B * windows, h, M^2, d]), `scaled_dot_product_attention` with the additive float mask
           (relative position bias + shift mask, prepared once, scale 1: Q is already scaled), the reverse
           permute and the roll back.  All of it is timed: that is what a block has to run without the kernel.

Shapes: the four Swin-T stages at 224 x 224 (56^2 x 3 heads, 28^2 x 6, 14^2 x 12, 7^2 x 24; window 7, d = 32),
each unshifted and shifted by 3 (the 7 x 7 stage only unshifted, as in the model), and Swin-B stage 1
(56^2 x 4 heads).

    python tools/window_attention_bench.py [--batch 32] [--reps 20] [--rounds 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A  # noqa: E402

# (name, map side, heads, window, shift, key_dim)
SHAPES = [("swin_t s1", 56, 3, 7, 0, 32), ("swin_t s1 shifted", 56, 3, 7, 3, 32),
          ("swin_t s2", 28, 6, 7, 0, 32), ("swin_t s2 shifted", 28, 6, 7, 3, 32),
          ("swin_t s3", 14, 12, 7, 0, 32), ("swin_t s3 shifted", 14, 12, 7, 3, 32),
          ("swin_t s4", 7, 24, 7, 0, 32),
          ("swin_b s1", 56, 4, 7, 0, 32), ("swin_b s1 shifted", 56, 4, 7, 3, 32)]


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
    """Median microseconds per call of each of `runs` (name -> callable): every round replays each
    implementation's graph once, in turn."""
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


def bench(name, B, S, h, M, s, d, reps, rounds):
    H = W = S
    T, nw = M * M, (S // M) ** 2
    qkv = torch.randn(B * H * W, 3 * h * d, device="cuda")
    qkv[:, :h * d] *= d ** -0.5                                  # the scale the projection folds into Q
    table = torch.randn((2 * M - 1) ** 2, h) * 0.5
    bias = A.window_bias(table, M, s, device="cuda")
    out = torch.empty(B * H * W, h * d, device="cuda")
    qkv16, out16 = qkv.to(torch.bfloat16), torch.empty(B * H * W, h * d, device="cuda", dtype=torch.bfloat16)
    # the library's additive mask, one [h, T, T] slice per window of an image, from the packed classes
    wy, wx = torch.meshgrid(torch.arange(S // M), torch.arange(S // M), indexing="ij")
    cls = (2 * (wy == S // M - 1) + (wx == S // M - 1)).reshape(-1).cuda() if s else torch.zeros(nw, dtype=torch.long,
                                                                                                 device="cuda")
    mask = bias[cls][:, :, :T, :T].contiguous()                  # [nw, h, T, T]
    mask = mask.unsqueeze(0).expand(B, nw, h, T, T).reshape(B * nw, h, T, T).contiguous()

    def library():
        x = qkv.reshape(B, H, W, 3, h, d)
        if s:
            x = torch.roll(x, shifts=(-s, -s), dims=(1, 2))
        x = x.reshape(B, S // M, M, S // M, M, 3, h, d).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * nw, h, T, d)
        o = F.scaled_dot_product_attention(x[0], x[1], x[2], attn_mask=mask, scale=1.0)
        o = o.permute(0, 2, 1, 3).reshape(B, S // M, S // M, M, M, h * d).permute(0, 1, 3, 2, 4, 5)
        o = o.reshape(B, H, W, h * d)
        if s:
            o = torch.roll(o, shifts=(s, s), dims=(1, 2))
        return o.reshape(B * H * W, h * d)

    t = interleaved_us({"ours": lambda: A.window_attention(qkv, bias, out, B, H, W, M, s, h, d),
                        "ours16": lambda: A.window_attention(qkv16, bias, out16, B, H, W, M, s, h, d),
                        "library": library}, reps, rounds)
    want = library()
    diff = (want - out).abs().max().item()
    diff16 = (want - out16.float()).abs().max().item()
    ratio = t["library"] / t["ours"]
    verdict = "ours faster" if ratio > 1.0 else "OURS SLOWER"
    print(f"{name:18s} B{B} {S}x{S} M{M} s{s} h{h} d{d} [{A.window_attention_path(d)}]: ours {t['ours']:8.1f} us"
          f" | ours bf16 act {t['ours16']:8.1f} us | library {t['library']:8.1f} us ({ratio:5.2f}x, {verdict})"
          f" | max diff vs library {diff:.2e} (bf16 act {diff16:.2e})", flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    for name, S, h, M, s, d in SHAPES:
        bench(name, a.batch, S, h, M, s, d, a.reps, a.rounds)


if __name__ == "__main__":
    main()
