#!/usr/bin/env python3
"""Timings of the self-attention core, hipGraph-timed like tools/deconv_bench.py.  Per shape, in one process, the
implementations interleaved round by round, in microseconds:

* ours     csrc/kernels/attention.hip through ops/attention.py `attention`, fp32 activations;
* ours16   the same kernel on bf16 activations (fp32 MFMA math; there is no bf16-MFMA attention);
* sdpa     `torch.nn.functional.scaled_dot_product_attention` in fp32 on [B, h, T, d] tensors (scale 1: Q is
           already scaled, as in our layout): the library reference point;
* unfused  `torch.matmul`, `softmax`, `torch.matmul` in fp32, the T x T scores through memory.

The torch paths read Q, K, V from contiguous [B, h, T, d] tensors prepared once (not timed); ours reads the
[B * T][h * (2 d + dv)] rows the QKV projection writes.  TF/s is on the true 2 * T^2 * h * (d + dv) MACs per image.
Shapes: ViT-Ti / S / B / L at 197 tokens (224 x 224 input) and ViT-B at 577 tokens (384 x 384).

    python tools/attention_bench.py [--batch 32] [--reps 20] [--rounds 5]

`--causal` times the causal instantiation instead, on GPT-2's shapes (12 heads of 64 at 128, 512 and 1024 tokens), in
fp32 and on bf16 activations, against `scaled_dot_product_attention(is_causal=True)` and against the same kernel
without the mask on the same shape.  The causal launch below the unmasked one is the evidence that the key tiles
above the diagonal are skipped and not merely masked; TF/s is on the T (T + 1) / 2 pairs the mask leaves.

    python tools/attention_bench.py --causal [--batch 8]

`--padding` times the padding-mask instantiation on DistilBERT's shapes (12 heads of 64 at 128 and 512 tokens): with
an all-kept mask against the unmasked entry point (the difference is the prologue's cost), and with random
right-padded lengths of mean T / 2 against the all-kept time (the gain from the key bound and the skipped query
waves) and against `scaled_dot_product_attention` with a boolean mask of the same lengths.

    python tools/attention_bench.py --padding [--batch 32]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A  # noqa: E402

# (name, tokens, heads, key_dim = value_dim)
SHAPES = [("vit_ti16", 197, 3, 64), ("vit_s16", 197, 6, 64), ("vit_b16", 197, 12, 64), ("vit_l16", 197, 16, 64),
          ("vit_b16@384", 577, 12, 64)]


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


def bench(name, B, T, h, d, reps, rounds):
    qkv = torch.randn(B * T, 3 * h * d, device="cuda")
    qkv[:, :h * d] *= d ** -0.5                                  # the scale the projection folds into Q
    out = torch.empty(B * T, h * d, device="cuda")
    qkv16, out16 = qkv.to(torch.bfloat16), torch.empty(B * T, h * d, device="cuda", dtype=torch.bfloat16)
    q, k, v = (qkv[:, i * h * d:(i + 1) * h * d].reshape(B, T, h, d).permute(0, 2, 1, 3).contiguous() for i in range(3))

    def unfused():
        return torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)), dim=-1), v)

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v, scale=1.0)

    t = interleaved_us({"ours": lambda: A.attention(qkv, out, B, T, h, d, d),
                        "ours16": lambda: A.attention(qkv16, out16, B, T, h, d, d),
                        "sdpa": sdpa, "unfused": unfused}, reps, rounds)
    want = unfused().permute(0, 2, 1, 3).reshape(B * T, h * d)
    diff = (want - out).abs().max().item()
    diff16 = (want - out16.float()).abs().max().item()
    flop = 2.0 * B * T * T * h * 2 * d
    tf = {n: flop / u / 1e6 for n, u in t.items()}
    print(f"{name:12s} B{B} T{T} h{h} d{d} [{A.attention_path(d, d)}]: ours {t['ours']:8.1f} us ({tf['ours']:5.1f} TF/s)"
          f" | ours bf16 act {t['ours16']:8.1f} us ({tf['ours16']:5.1f} TF/s)"
          f" | sdpa {t['sdpa']:8.1f} us ({tf['sdpa']:5.1f} TF/s, {t['sdpa'] / t['ours']:5.2f}x)"
          f" | unfused {t['unfused']:8.1f} us ({tf['unfused']:5.1f} TF/s, {t['unfused'] / t['ours']:5.2f}x)"
          f" | max diff vs unfused {diff:.2e} (bf16 act {diff16:.2e})", flush=True)
    return t


# (name, tokens, heads, key_dim = value_dim): GPT-2 (124M) at its default, a middle and its full context
CAUSAL_SHAPES = [("gpt2@128", 128, 12, 64), ("gpt2@512", 512, 12, 64), ("gpt2@1024", 1024, 12, 64)]


def bench_causal(name, B, T, h, d, reps, rounds):
    qkv = torch.randn(B * T, 3 * h * d, device="cuda")
    qkv[:, :h * d] *= d ** -0.5
    out, full = torch.empty(B * T, h * d, device="cuda"), torch.empty(B * T, h * d, device="cuda")
    qkv16 = qkv.to(torch.bfloat16)
    out16, full16 = (torch.empty(B * T, h * d, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    q, k, v = (qkv[:, i * h * d:(i + 1) * h * d].reshape(B, T, h, d).permute(0, 2, 1, 3).contiguous() for i in range(3))

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v, scale=1.0, is_causal=True)

    t = interleaved_us({"causal": lambda: A.attention(qkv, out, B, T, h, d, d, causal=True),
                        "full": lambda: A.attention(qkv, full, B, T, h, d, d),
                        "causal16": lambda: A.attention(qkv16, out16, B, T, h, d, d, causal=True),
                        "full16": lambda: A.attention(qkv16, full16, B, T, h, d, d),
                        "sdpa": sdpa}, reps, rounds)
    want = sdpa().permute(0, 2, 1, 3).reshape(B * T, h * d)
    diff = (want - out).abs().max().item()
    diff16 = (want - out16.float()).abs().max().item()
    flop = 2.0 * B * (T * (T + 1) // 2) * h * 2 * d
    print(f"{name:10s} B{B} T{T} h{h} d{d} [{A.attention_path(d, d)}, {-(-T // A.attention_tiles()[1])} key tiles]: "
          f"causal {t['causal']:8.1f} us ({flop / t['causal'] / 1e6:5.1f} TF/s) | unmasked {t['full']:8.1f} us "
          f"({t['causal'] / t['full']:4.2f}x) | bf16 act causal {t['causal16']:8.1f} us | unmasked {t['full16']:8.1f} us "
          f"({t['causal16'] / t['full16']:4.2f}x) | sdpa is_causal {t['sdpa']:8.1f} us ({t['sdpa'] / t['causal']:5.2f}x ours)"
          f" | max diff vs sdpa {diff:.2e} (bf16 act {diff16:.2e})", flush=True)
    return t


# (name, tokens, heads, key_dim = value_dim): DistilBERT at its default and its full context
PADDING_SHAPES = [("distilbert@128", 128, 12, 64), ("distilbert@512", 512, 12, 64)]


def bench_padding(name, B, T, h, d, reps, rounds):
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(B * T, 3 * h * d, device="cuda")
    qkv[:, :h * d] *= d ** -0.5
    qkv16 = qkv.to(torch.bfloat16)
    outs = {n: torch.empty(B * T, h * d, device="cuda") for n in ("full", "kept", "padded")}
    outs16 = {n: torch.empty(B * T, h * d, device="cuda", dtype=torch.bfloat16) for n in ("full", "kept", "padded")}
    lengths = torch.randint(1, T, (B, 1), generator=g)            # uniform on [1, T - 1]: mean T / 2
    keep = (torch.arange(T)[None, :] < lengths)
    all_kept = torch.ones(B, T, device="cuda")
    padded = keep.float().cuda()                                  # id 1 where kept, 0 where padded
    q, k, v = (qkv[:, i * h * d:(i + 1) * h * d].reshape(B, T, h, d).permute(0, 2, 1, 3).contiguous() for i in range(3))
    bmask = (keep[:, None, :, None] & keep[:, None, None, :]).cuda()
    bmask = bmask | ~keep[:, None, :, None].cuda()                # a padded query attends everything: no NaN row

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v, attn_mask=bmask, scale=1.0)

    t = interleaved_us({
        "full": lambda: A.attention(qkv, outs["full"], B, T, h, d, d),
        "kept": lambda: A.attention(qkv, outs["kept"], B, T, h, d, d, key_mask=all_kept),
        "padded": lambda: A.attention(qkv, outs["padded"], B, T, h, d, d, key_mask=padded),
        "full16": lambda: A.attention(qkv16, outs16["full"], B, T, h, d, d),
        "kept16": lambda: A.attention(qkv16, outs16["kept"], B, T, h, d, d, key_mask=all_kept),
        "padded16": lambda: A.attention(qkv16, outs16["padded"], B, T, h, d, d, key_mask=padded),
        "sdpa": sdpa}, reps, rounds)
    want = sdpa().permute(0, 2, 1, 3).reshape(B * T, h * d)
    rows = keep.reshape(-1).cuda()
    diff = (want - outs["padded"])[rows].abs().max().item()
    same = torch.equal(outs["full"], outs["kept"])
    print(f"{name:14s} B{B} T{T} h{h} d{d} [{A.attention_path(d, d)}] mean length {lengths.float().mean().item():.0f}: "
          f"unmasked {t['full']:8.1f} us | all-kept mask {t['kept']:8.1f} us ({t['kept'] / t['full']:4.2f}x, "
          f"+{t['kept'] - t['full']:.1f} us, bits equal: {same}) | right-padded {t['padded']:8.1f} us "
          f"({t['padded'] / t['kept']:4.2f}x of all-kept) | bf16 act unmasked {t['full16']:8.1f} us | all-kept "
          f"{t['kept16']:8.1f} us ({t['kept16'] / t['full16']:4.2f}x) | right-padded {t['padded16']:8.1f} us "
          f"({t['padded16'] / t['kept16']:4.2f}x) | sdpa bool mask {t['sdpa']:8.1f} us ({t['sdpa'] / t['padded']:5.2f}x "
          f"ours) | max diff vs sdpa at kept rows {diff:.2e}", flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--causal", action="store_true", help="the causal kernel on GPT-2 shapes (module docstring)")
    ap.add_argument("--padding", action="store_true", help="the padding-mask kernel on DistilBERT shapes")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    if a.padding:
        for name, T, h, d in PADDING_SHAPES:
            bench_padding(name, a.batch, T, h, d, a.reps, a.rounds)
        return
    if a.causal:
        for name, T, h, d in CAUSAL_SHAPES:
            bench_causal(name, a.batch, T, h, d, a.reps, a.rounds)
        return
    for name, T, h, d in SHAPES:
        bench(name, a.batch, T, h, d, a.reps, a.rounds)


if __name__ == "__main__":
    main()
