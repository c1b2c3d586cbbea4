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

`--wide` times the head-split kernel for wide heads (csrc/kernels/attention_wide.h) on the Stable Diffusion VAE
decoder's mid-block (one head of 512 over 4,096 tokens, 1 and 4 images), a Gemma-like shape (8 query heads over one
key / value head of 256, 1,024 tokens, causal, 8 images) and a U-Net-like shape (8 heads of 160, 1,024 tokens, 4
images), each in fp32 and on bf16 activations, against the plain kernel on the same values (rows of stride width + 1:
a stride off the 4-element grid takes the plain kernel, which is what these head sizes ran on before) and against
`scaled_dot_product_attention` in the same type.  The batch is part of the shape; the plain kernel's graph holds one
call, it runs for tens to hundreds of milliseconds.

    python tools/attention_bench.py --wide

`--math bf16` times the bf16-MFMA kernel (csrc/kernels/attention_bf16.h, `attention(..., math="bf16")`) on bf16 rows
against the fp32-math kernel on the same rows (the default launch) and against `scaled_dot_product_attention` in
bf16: the ViT shapes above at 32 images, GPT-2's causal shapes at 8 images, and Llama's grouped-query causal shapes
(32 query heads over 4 of 64; 4,096 rows each).  The batch is part of the shape.

    python tools/attention_bench.py --math bf16
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


def interleaved_us(runs, reps, rounds, reps_of=None):
    """Median microseconds per call of each of `runs` (name -> callable): every round replays each
    implementation's graph once, in turn.  `reps_of`: calls per graph of the implementations that differ from `reps`."""
    graphs = {}
    reps_of = {name: (reps_of or {}).get(name, reps) for name in runs}
    for name, run in runs.items():
        try:
            graphs[name] = capture(run, reps_of[name])
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
            times[name].append(e0.elapsed_time(e1) / reps_of[name] * 1e3)
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


# (name, batch, tokens, query heads, key / value heads, key_dim = value_dim, causal)
WIDE_SHAPES = [("sd_vae_mid", 1, 4096, 1, 1, 512, False), ("sd_vae_mid", 4, 4096, 1, 1, 512, False),
               ("gemma_like", 8, 1024, 8, 1, 256, True), ("unet_like", 4, 1024, 8, 8, 160, False)]


def bench_wide(name, B, T, h, hkv, d, causal, reps, rounds):
    w_in, w_out = (h + 2 * hkv) * d, h * d
    x = torch.randn(B * T, w_in, device="cuda")
    x[:, :h * d] *= d ** -0.5
    q = x[:, :h * d].reshape(B, T, h, d).permute(0, 2, 1, 3).contiguous()
    k, v = (x[:, h * d + i * hkv * d:h * d + (i + 1) * hkv * d].reshape(B, T, hkv, d).permute(0, 2, 1, 3)
            .repeat_interleave(h // hkv, dim=1).contiguous() for i in range(2))
    flop = 2.0 * B * (T * (T + 1) // 2 if causal else T * T) * h * 2 * d
    for dtype in (torch.float32, torch.bfloat16):
        xa = x.to(dtype)
        xo = torch.zeros(B * T, w_in + 1, device="cuda", dtype=dtype)              # the same values, stride off the grid
        xo[:, :w_in] = xa
        out = torch.empty(B * T, w_out, device="cuda", dtype=dtype)
        outo = torch.empty(B * T, w_out + 1, device="cuda", dtype=dtype)
        qt, kt, vt = q.to(dtype), k.to(dtype), v.to(dtype)

        def sdpa():
            return F.scaled_dot_product_attention(qt, kt, vt, scale=1.0, is_causal=causal)

        t = interleaved_us({"wide": lambda: A.attention(xa, out, B, T, h, d, d, causal=causal, kv_heads=hkv),
                            "plain": lambda: A.attention(xo, outo, B, T, h, d, d, causal=causal, kv_heads=hkv),
                            "sdpa": sdpa}, reps, rounds, reps_of={"plain": 1})
        want = sdpa().permute(0, 2, 1, 3).reshape(B * T, w_out).float()
        diff = (want - out.float()).abs().max().item()
        diffo = (outo[:, :w_out].float() - out.float()).abs().max().item()
        print(f"{name:10s} B{B} T{T} h{h}/{hkv} d{d} {'causal' if causal else 'full  '} {str(dtype)[6:]:8s} "
              f"[{A.attention_kernel(d, d)}, tiles {A.attention_wide_tiles(d, d)}]: wide {t['wide']:9.1f} us "
              f"({flop / t['wide'] / 1e6:5.1f} TF/s) | plain {t['plain']:11.1f} us ({t['plain'] / t['wide']:6.1f}x wide) | "
              f"sdpa {t['sdpa']:9.1f} us ({t['sdpa'] / t['wide']:5.2f}x wide) | max diff vs sdpa {diff:.2e}, vs plain "
              f"{diffo:.2e}", flush=True)


# (name, batch, tokens, query heads, key / value heads, key_dim = value_dim, causal)
MATH_SHAPES = ([(n, 32, T, h, h, d, False) for n, T, h, d in SHAPES] + [(n, 8, T, h, h, d, True) for n, T, h, d in CAUSAL_SHAPES]
               + [("llama_gqa", 32, 128, 32, 4, 64, True), ("llama_gqa", 8, 512, 32, 4, 64, True),
                  ("llama_gqa", 2, 2048, 32, 4, 64, True), ("llama_like", 2, 2048, 32, 8, 128, True)])


def bench_math(name, B, T, h, hkv, d, causal, reps, rounds):
    w_in, w_out = (h + 2 * hkv) * d, h * d
    x = torch.randn(B * T, w_in, device="cuda")
    x[:, :h * d] *= d ** -0.5
    x = x.to(torch.bfloat16)
    q = x[:, :h * d].reshape(B, T, h, d).permute(0, 2, 1, 3).contiguous()
    k, v = (x[:, h * d + i * hkv * d:h * d + (i + 1) * hkv * d].reshape(B, T, hkv, d).permute(0, 2, 1, 3)
            .repeat_interleave(h // hkv, dim=1).contiguous() for i in range(2))
    out, old = (torch.empty(B * T, w_out, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    flop = 2.0 * B * (T * (T + 1) // 2 if causal else T * T) * h * 2 * d

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v, scale=1.0, is_causal=causal)

    t = interleaved_us({"bf16": lambda: A.attention(x, out, B, T, h, d, d, causal=causal, kv_heads=hkv, math="bf16"),
                        "fp32": lambda: A.attention(x, old, B, T, h, d, d, causal=causal, kv_heads=hkv),
                        "sdpa": sdpa}, reps, rounds)
    want = F.scaled_dot_product_attention(q.float(), k.float(), v.float(), scale=1.0, is_causal=causal)
    want = want.permute(0, 2, 1, 3).reshape(B * T, w_out)
    print(f"{name:12s} B{B} T{T} h{h}/{hkv} d{d} {'causal' if causal else 'full  '} "
          f"[{A.attention_kernel(d, d, math='bf16')}, tiles {A.attention_bf16_tiles()}]: bf16 math {t['bf16']:8.1f} us "
          f"({flop / t['bf16'] / 1e6:6.1f} TF/s) | fp32 math, same rows {t['fp32']:8.1f} us ({t['fp32'] / t['bf16']:5.2f}x) | "
          f"sdpa bf16 {t['sdpa']:8.1f} us ({t['sdpa'] / t['bf16']:5.2f}x) | max diff vs fp32 sdpa: bf16 math "
          f"{(want - out.float()).abs().max().item():.2e}, fp32 math {(want - old.float()).abs().max().item():.2e}", flush=True)


# (name, heads, kv heads, key_dim = value_dim) of the decode rows; batches and cached lengths below
DECODE_HEADS = [("tinyllama", 32, 4, 64), ("llama2_7b", 32, 32, 128)]
DECODE_BATCHES, DECODE_LENGTHS = (1, 8, 32), (512, 2048, 8192)
HBM_PEAK = 8.0e12                                                # bytes/s, the MI355X figure


def bench_decode(name, B, L, h, hkv, d, dtype, reps, rounds):
    """One decode step at L cached keys per sequence (cache length L): the decode kernel against (a) the
    cross-attention kernel at tokens_q = 1 on rows with every K / V head repeated g times, the only path before the
    decode kernel, and (b) scaled_dot_product_attention(enable_gqa=True).  Bytes: K and V once, L rows each."""
    g = h // hkv
    q = (torch.randn(B, h * d, device="cuda") * d ** -0.5).to(dtype)
    kc, vc = (torch.randn(B, hkv, L, d, device="cuda").to(dtype) for _ in range(2))
    pos = torch.full((B,), L - 1, dtype=torch.int32, device="cuda")
    out, old = (torch.empty(B, h * d, device="cuda", dtype=dtype) for _ in range(2))
    ws = torch.empty(max(A.attention_decode_plan(B, hkv, L, h, d)[2], 1), device="cuda")
    # (a): [B * L][h d] rows, head-major
    kx, vx = (t.repeat_interleave(g, dim=1).permute(0, 2, 1, 3).reshape(B * L, h * d).contiguous() for t in (kc, vc))
    q4, k4, v4 = q.view(B, h, 1, d), kc, vc

    def sdpa():
        return F.scaled_dot_product_attention(q4, k4, v4, scale=1.0, enable_gqa=True)

    t = interleaved_us({"decode": lambda: A.attention_decode(q, kc, vc, pos, out, h, d, d, kv_heads=hkv, workspace=ws),
                        "cross": lambda: A.cross_attention(q, kx, vx, old, B, 1, L, h, d, d),
                        "sdpa": sdpa}, reps, rounds)
    want = sdpa().reshape(B, h * d).float()
    nbytes = 2.0 * B * hkv * L * d * q.element_size()
    S, KS, _ = A.attention_decode_plan(B, hkv, L)
    print(f"{name:10s} {str(dtype)[6:]:8s} B{B:<2d} L{L:<5d} h{h}/{hkv} d{d} S{S} KS{KS}: decode {t['decode']:8.1f} us "
          f"({nbytes / t['decode'] / 1e6:6.2f} TB/s K+V, {nbytes / t['decode'] * 1e6 / HBM_PEAK * 100:4.1f} % of HBM peak) | "
          f"(a) cross_attention tokens_q=1 {t['cross']:8.1f} us ({t['cross'] / t['decode']:5.2f}x) | (b) sdpa gqa "
          f"{t['sdpa']:8.1f} us ({t['sdpa'] / t['decode']:5.2f}x) | max diff vs sdpa: decode "
          f"{(want - out.float()).abs().max().item():.2e}, cross {(want - old.float()).abs().max().item():.2e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--causal", action="store_true", help="the causal kernel on GPT-2 shapes (module docstring)")
    ap.add_argument("--padding", action="store_true", help="the padding-mask kernel on DistilBERT shapes")
    ap.add_argument("--wide", action="store_true", help="the head-split kernel on wide heads (module docstring)")
    ap.add_argument("--math", choices=["fp32", "bf16"], default="fp32",
                    help="bf16: the bf16-MFMA kernel against the fp32-math kernel on bf16 rows (module docstring)")
    ap.add_argument("--decode", action="store_true", help="the decode kernel against cross_attention at one query "
                                                          "and sdpa (csrc/kernels/attention_decode.h)")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    if a.decode:
        for name, h, hkv, d in DECODE_HEADS:
            for dtype in (torch.float32, torch.bfloat16):
                for B in DECODE_BATCHES:
                    for L in DECODE_LENGTHS:
                        bench_decode(name, B, L, h, hkv, d, dtype, a.reps, a.rounds)
        return
    if a.math == "bf16":
        for name, B, T, h, hkv, d, causal in MATH_SHAPES:
            bench_math(name, B, T, h, hkv, d, causal, a.reps, a.rounds)
        return
    if a.wide:
        for name, B, T, h, hkv, d, causal in WIDE_SHAPES:
            bench_wide(name, B, T, h, hkv, d, causal, a.reps, a.rounds)
        return
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
