#!/usr/bin/env python3
"""Timings of the attention core with separate sources, hipGraph-timed like tools/attention_bench.py.  Per shape,
in one process, the implementations interleaved round by round, in microseconds:

* ours     csrc/kernels/cross_attention.hip through ops/attention.py `cross_attention`, fp32 activations;
* ours16   the same kernel on bf16 activations (fp32 MFMA math);
* sdpa     `torch.nn.functional.scaled_dot_product_attention` in fp32 on [B, h, T, d] tensors (scale 1: Q is already
           scaled, as in our layout): the library reference point;
* unfused  `torch.matmul`, `softmax`, `torch.matmul` in fp32, the Tq x Tk scores through memory.

The torch paths read Q, K, V from contiguous [B, h, T, d] tensors prepared once (not timed); ours reads the buffers
the projections write, in the plan's layout: [Q | K] side by side and V apart for the encoder (q = k from
`src + pos`, v from `src`) and for the decoder's self-attention, three buffers for the decoder's cross-attention.
TF/s is on the true 2 * Tq * Tk * h * (d + dv) MACs per image.  `blocks` is the MFMA path's grid, B x heads x
ceil(Tq / 64): the decoder's 100 queries make two query tiles per (image, head), 32 blocks at batch 2, on a chip
of 256 CUs.  Shapes: DETR at 480 x 640 (300 memory tokens) and at 800 x 1344 (1050), 8 heads of 32.

    python tools/cross_attention_bench.py [--batch 2] [--reps 20] [--rounds 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A  # noqa: E402

from attention_bench import interleaved_us  # noqa: E402

# (name, layout, query tokens, key tokens, heads, key_dim = value_dim)
SHAPES = [("encoder 300", "qk_v", 300, 300, 8, 32), ("encoder 1050", "qk_v", 1050, 1050, 8, 32),
          ("decoder self", "qk_v", 100, 100, 8, 32), ("decoder cross 300", "q_k_v", 100, 300, 8, 32),
          ("decoder cross 1050", "q_k_v", 100, 1050, 8, 32)]


def bench(name, layout, B, Tq, Tk, h, d, reps, rounds):
    hd = h * d
    if layout == "qk_v":                                            # [Q | K] in one buffer, V in its own
        qk = torch.randn(B * Tq, 2 * hd, device="cuda")
        qk[:, :hd] *= d ** -0.5                                     # the scale the projection folds into Q
        qv, kv, vv = qk[:, :hd], qk[:, hd:], torch.randn(B * Tk, hd, device="cuda")
    else:
        qv, kv, vv = (torch.randn(B * t, hd, device="cuda") for t in (Tq, Tk, Tk))
        qv *= d ** -0.5
    out = torch.empty(B * Tq, hd, device="cuda")
    if layout == "qk_v":
        qk16 = qk.to(torch.bfloat16)
        q16, k16, v16 = qk16[:, :hd], qk16[:, hd:], vv.to(torch.bfloat16)
    else:
        q16, k16, v16 = (t.to(torch.bfloat16) for t in (qv, kv, vv))
    out16 = torch.empty(B * Tq, hd, device="cuda", dtype=torch.bfloat16)
    q, k, v = (t.reshape(B, n, h, d).permute(0, 2, 1, 3).contiguous() for t, n in ((qv, Tq), (kv, Tk), (vv, Tk)))

    def unfused():
        return torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)), dim=-1), v)

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v, scale=1.0)

    t = interleaved_us({"ours": lambda: A.cross_attention(qv, kv, vv, out, B, Tq, Tk, h, d, d),
                        "ours16": lambda: A.cross_attention(q16, k16, v16, out16, B, Tq, Tk, h, d, d),
                        "sdpa": sdpa, "unfused": unfused}, reps, rounds)
    want = unfused().permute(0, 2, 1, 3).reshape(B * Tq, hd)
    diff = (want - out).abs().max().item()
    diff16 = (want - out16.float()).abs().max().item()
    flop = 2.0 * B * Tq * Tk * h * 2 * d
    tf = {n: flop / u / 1e6 for n, u in t.items()}
    blocks = B * h * -(-Tq // A.cross_attention_tiles()[0])
    print(f"{name:18s} B{B} Tq{Tq} Tk{Tk} h{h} d{d} [{A.cross_attention_path(qv, kv, vv, out, d, d)}, {blocks} blocks]:"
          f" ours {t['ours']:8.1f} us ({tf['ours']:5.2f} TF/s)"
          f" | ours bf16 act {t['ours16']:8.1f} us ({tf['ours16']:5.2f} TF/s)"
          f" | sdpa {t['sdpa']:8.1f} us ({tf['sdpa']:5.2f} TF/s, {t['sdpa'] / t['ours']:5.2f}x)"
          f" | unfused {t['unfused']:8.1f} us ({tf['unfused']:5.2f} TF/s, {t['unfused'] / t['ours']:5.2f}x)"
          f" | max diff vs unfused {diff:.2e} (bf16 act {diff16:.2e})", flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    for name, layout, Tq, Tk, h, d in SHAPES:
        bench(name, layout, a.batch, Tq, Tk, h, d, a.reps, a.rounds)


if __name__ == "__main__":
    main()
