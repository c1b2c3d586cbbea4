"""The skinny GEMM (csrc/kernels/gemm_skinny.h) against the tile path and torch.matmul on the one-token GEMMs of
tinyllama_1_1b and llama2_7b (qkv, out, gate / up, down) at M = 1, 8, 16, 32 rows, fp32 and bf16.

Per shape the three implementations are timed interleaved, each as a hipGraph of 20 calls, median of 5 replays
(tools/attention_bench.py's `interleaved_us`).  The 20 calls walk over copies of the weights, enough of them that W
does not sit in a cache between replays.  Before timing, the skinny output is checked against the tile output
(fp32: 2e-5 of the largest value; bf16: one bf16 rounding).  Printed per row: microseconds, W bytes / time next to
the 8 TB/s figure, the ratio to each rival; a row where skinny is behind a rival is bold.

    python tools/skinny_bench.py [--models tinyllama_1_1b,llama2_7b] [--rows 1,8,16,32] [--dtypes fp32,bf16]
    python tools/skinny_bench.py --sweep     # every (F, KS) at M = 8 next to the plan's choice
    python tools/skinny_bench.py --weights mxfp4 [--sweep --rows 1,8,16]
        the MXFP4 kernel (csrc/kernels/gemm_skinny_mx.h) on random codes, next to the bf16 skinny kernel, the bf16
        tile path and torch.matmul on the dequantised weights; TB/s counts the codes and scales it streams
"""
import argparse
import dataclasses
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C  # noqa: E402

# (name, K, N): hidden 2048 / 32 heads / 4 kv heads of 64 / MLP 5632, and hidden 4096 / 32 heads of 128 / MLP 11008
SHAPES = [("tinyllama_1_1b qkv", 2048, 2560), ("tinyllama_1_1b out", 2048, 2048),
          ("tinyllama_1_1b gate/up", 2048, 5632), ("tinyllama_1_1b down", 5632, 2048),
          ("llama2_7b qkv", 4096, 12288), ("llama2_7b out", 4096, 4096),
          ("llama2_7b gate/up", 4096, 11008), ("llama2_7b down", 11008, 4096)]
ROWS = (1, 8, 16, 32)
REPS, ROUNDS, PEAK_TBS = 20, 5, 8.0
CACHE_BYTES = 512 << 20         # the copies of W a graph walks hold at least this much (L2 + infinity cache: 288 MB)


def packed(K, N, dtype, copies):
    """`copies` PackedConvs of one random 1x1 conv, laid out as pack_conv / pack_conv_f32 (zero padding)."""
    bk = C.F32_BK if dtype == torch.float32 else C.BK
    Kpad, Npad = math.ceil(K / bk) * bk, math.ceil(N / 256) * 256
    w = torch.zeros((Npad, Kpad), dtype=dtype, device="cuda")
    w[:N, :K] = (torch.randn((N, K), device="cuda", generator=torch.Generator("cuda").manual_seed(K + N))
                 * K ** -0.5).to(dtype)
    pc = C.PackedConv(w=w, bias=torch.randn(N, device="cuda"), kh=1, kw=1, cin=K, cout=N, stride=1, pad_t=0, pad_l=0,
                      pad_b=0, pad_r=0)
    return [pc] + [dataclasses.replace(pc, w=w.clone()) for _ in range(copies - 1)]


def packed_mx(K, N, copies):
    """`copies` PackedConvs of one random MXFP4 1x1 conv: random codes and block exponents within 2 of
    log2(K^-1/2) - 1 in the kernel's layout, and `w` their dequantised values, computed on the device."""
    gen = torch.Generator("cuda").manual_seed(K + N)
    Kpad, Npad, kp64 = math.ceil(K / C.MX_KC) * C.MX_KC, math.ceil(N / 256) * 256, math.ceil(K / C.BK) * C.BK
    nib = torch.randint(0, 16, (Npad, Kpad), device="cuda", generator=gen, dtype=torch.int32)
    nib[N:], nib[:, K:] = 0, 0
    exps = torch.randint(-2, 3, (Npad, Kpad // 32), device="cuda", generator=gen, dtype=torch.int32)
    exps += round(-0.5 * math.log2(K)) - 1
    lut = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], device="cuda")
    w = torch.ldexp(lut[nib.long()], exps.repeat_interleave(32, dim=1)).bfloat16()       # exact: two significant bits
    w = w[:, :kp64].contiguous()                          # pack_conv's row length; the columns past K are zero
    pairs = nib.view(Npad, -1, 4, 4, 4, 2)                # [n][chunk][s][q][byte][lower k, higher k]
    words = (pairs[..., 0] | pairs[..., 1] << 4).to(torch.uint8).transpose(2, 3).contiguous().view(torch.int32)[..., 0]
    scales = (exps + 127).to(torch.uint8).view(Npad, -1, 4).contiguous().view(torch.int32)[..., 0]
    pc = C.PackedConv(w=w, bias=torch.randn(N, device="cuda"), kh=1, kw=1, cin=K, cout=N, stride=1, pad_t=0, pad_l=0,
                      pad_b=0, pad_r=0, mx=C.MxWeights(words, scales))
    return [pc] + [dataclasses.replace(pc, w=w.clone(), mx=C.MxWeights(words.clone(), scales.clone()))
                   for _ in range(copies - 1)]


def bench_shape_mx(name, K, N, M, sweep=False):
    """A row of the MXFP4 table: the kernel with its plan against the bf16 skinny kernel, the bf16 tile path and
    torch.matmul on the dequantised weights, or (sweep) every (F, KS)."""
    from attention_bench import interleaved_us
    qbytes = N * math.ceil(K / 32) * 17                   # 16 bytes of codes and a scale byte per block
    pcs = packed_mx(K, N, min(REPS, max(2, math.ceil(CACHE_BYTES / (2 * N * K)))))
    x = torch.randn((M, K), device="cuda").bfloat16()
    out = {k: torch.empty((M, N), dtype=torch.bfloat16, device="cuda") for k in ("mx", "skinny", "tiles", "matmul")}
    ctr = torch.zeros(4096, dtype=torch.int32, device="cuda")
    ws = torch.empty(64 * M * N, dtype=torch.float32, device="cuda")
    cfg, ks = C.choose_cfg(M, N, pcs[0].Kpad)
    scratch = C.bf16_scratch(cfg, ks, M, 1, 1, pcs[0])
    tws = torch.empty(max(scratch[0], 1), dtype=torch.float32, device="cuda")
    tctr = torch.zeros(max(scratch[1], 1), dtype=torch.int32, device="cuda")
    turn = dict.fromkeys(out, 0)

    def pick(k):
        turn[k] += 1
        return pcs[turn[k] % len(pcs)]

    def mx(F=None, KS=None):
        return lambda: C.mx_forward(x, pick("mx"), out["mx"], F=F, ksplit=KS, workspace=ws, counters=ctr)

    runs = {"mx": mx(),
            "skinny": lambda: C.skinny_forward(x, pick("skinny"), out["skinny"], workspace=ws, counters=ctr),
            "tiles": lambda: C.conv_forward(x, pick("tiles"), out["tiles"], cfg=cfg, ksplit=ks, workspace=tws,
                                            counters=tctr),
            "matmul": lambda: torch.matmul(x, pick("matmul").w[:N, :K].t(), out=out["matmul"])}
    turn["mx"] = turn["skinny"] = -1                      # both on copy 0 for the comparison
    runs["mx"]()
    runs["skinny"]()
    torch.cuda.synchronize()
    a, b = out["mx"].double(), out["skinny"].double()
    if not bool(((a - b).abs() <= b.abs() * 2.0 ** -7 + 2e-5 * b.abs().max()).all()):
        raise SystemExit(f"{name} M {M}: mxfp4 differs from bf16 skinny by {float((a - b).abs().max()):.3e}")
    F, KS = C.mx_plan(M, N, K)
    if sweep:
        grid = [(f, k) for f in C.MX_F for k in (1, 2, 3, 4, 6, 8, 12, 16, 24) if k <= max(1, C.mx_chunks(K) // 4)]
        grid += [(F, KS)] if (F, KS) not in grid else []
        us = interleaved_us({f"F{f} KS{k}": mx(f, k) for f, k in grid}, REPS, ROUNDS)
        best = min(us, key=us.get)
        print(f"{name} M {M} mxfp4: plan F{F} KS{KS} {us[f'F{F} KS{KS}']:.1f} us, best {best} {us[best]:.1f} us | "
              + " ".join(f"{k}={v:.1f}" for k, v in us.items()), flush=True)
        return
    us = interleaved_us(runs, REPS, ROUNDS)
    row = (f"| {name} | {M} | F{F} KS{KS} | {us['mx']:.1f} | {qbytes / us['mx'] / 1e6:.2f} of {PEAK_TBS:.0f} | "
           + " | ".join(f"{us[k]:.1f} ({us[k] / us['mx']:.2f}x)" for k in ("skinny", "tiles", "matmul")) + " |")
    behind = us["mx"] > min(us["skinny"], us["tiles"])
    print("| " + " | ".join(f"**{c.strip()}**" for c in row.strip("|").split("|")) + " |" if behind else row, flush=True)


def bench_shape(name, K, N, M, dtype, sweep=False):
    from attention_bench import interleaved_us
    fp32 = dtype == torch.float32
    wbytes = N * K * (4 if fp32 else 2)
    pcs = packed(K, N, dtype, min(REPS, max(2, math.ceil(CACHE_BYTES / wbytes))))
    x = torch.randn((M, K), device="cuda").to(dtype)
    out = {k: torch.empty((M, N), dtype=dtype, device="cuda") for k in ("skinny", "tiles", "matmul")}
    ctr = torch.zeros(4096, dtype=torch.int32, device="cuda")
    ws = torch.empty(64 * M * N, dtype=torch.float32, device="cuda")
    cfg, ks = (C.choose_cfg_f32 if fp32 else C.choose_cfg)(M, N, pcs[0].Kpad)
    tile_fwd = C.conv_forward_f32 if fp32 else C.conv_forward
    scratch = (C.f32_scratch if fp32 else C.bf16_scratch)(cfg, ks, M, 1, 1, pcs[0])
    tws = torch.empty(max(scratch[0], 1), dtype=torch.float32, device="cuda")
    tctr = torch.zeros(max(scratch[1], 1), dtype=torch.int32, device="cuda")
    turn = {"skinny": 0, "tiles": 0, "matmul": 0}

    def pick(k):                                       # the next copy of W: call i of a graph reads copy i % copies
        turn[k] += 1
        return pcs[turn[k] % len(pcs)]

    def skinny(F=None, KS=None):
        return lambda: C.skinny_forward(x, pick("skinny"), out["skinny"], F=F, ksplit=KS, workspace=ws, counters=ctr)

    runs = {"skinny": skinny(),
            "tiles": lambda: tile_fwd(x, pick("tiles"), out["tiles"], cfg=cfg, ksplit=ks, workspace=tws, counters=tctr),
            "matmul": lambda: torch.matmul(x, pick("matmul").w[:N, :K].t(), out=out["matmul"])}
    turn["skinny"] = turn["tiles"] = -1                # both on copy 0 for the comparison
    runs["skinny"]()
    runs["tiles"]()
    torch.cuda.synchronize()
    a, b = out["skinny"].double(), out["tiles"].double()
    # bf16: the two fp32 sums may fall on either side of a rounding boundary, one bf16 step (2^-7 of the value) apart
    bound = 2e-5 * b.abs().max() if fp32 else b.abs() * 2.0 ** -7 + 2e-5 * b.abs().max()
    if not bool(((a - b).abs() <= bound).all()):
        raise SystemExit(f"{name} M {M} {dtype}: skinny differs from the tile path by {float((a - b).abs().max()):.3e}")
    F, KS = C.skinny_plan(M, N, K, dtype)
    if sweep:
        chunks = C.skinny_chunks(K, dtype)
        grid = [(f, k) for f in C.SKINNY_F for k in (1, 2, 3, 4, 6, 8, 12, 16, 24, 32) if k <= max(1, chunks // 4)]
        us = interleaved_us({f"F{f} KS{k}": skinny(f, k) for f, k in grid}, REPS, ROUNDS)
        best = min(us, key=us.get)
        print(f"{name} M {M} {'fp32' if fp32 else 'bf16'}: plan F{F} KS{KS} {us[f'F{F} KS{KS}']:.1f} us, best {best} "
              f"{us[best]:.1f} us | " + " ".join(f"{k}={v:.1f}" for k, v in us.items()), flush=True)
        return
    us = interleaved_us(runs, REPS, ROUNDS)
    behind = us["skinny"] > min(us["tiles"], us["matmul"])
    row = (f"| {name} | {M} | {'fp32' if fp32 else 'bf16'} | F{F} KS{KS} | {us['skinny']:.1f} | "
           f"{wbytes / us['skinny'] / 1e6:.2f} of {PEAK_TBS:.0f} | cfg {cfg} ks {ks}: {us['tiles']:.1f} "
           f"({us['tiles'] / us['skinny']:.2f}x) | {us['matmul']:.1f} ({us['matmul'] / us['skinny']:.2f}x) |")
    print("| " + " | ".join(f"**{c.strip()}**" for c in row.strip("|").split("|")) + " |" if behind else row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="tinyllama_1_1b,llama2_7b")
    ap.add_argument("--rows", default=None, help="default 1,8,16,32; with --sweep 8")
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--sweep", action="store_true", help="time every (F, KS) at M = 8 instead of the rivals")
    ap.add_argument("--weights", default=None, choices=["mxfp4"], help="the MXFP4 kernel's table or sweep instead")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    rows = [int(r) for r in a.rows.split(",")] if a.rows else ([8] if a.sweep else list(ROWS))
    if a.weights:
        if not a.sweep:
            print("| GEMM (W [N][K]) | M | plan | mxfp4 us | codes + scales TB/s | bf16 skinny us | bf16 tile path us "
                  "| torch.matmul us |\n|---|---|---|---|---|---|---|---|")
        for name, K, N in SHAPES:
            if name.split()[0] in a.models.split(","):
                for M in rows:
                    bench_shape_mx(name, K, N, M, sweep=a.sweep)
                    torch.cuda.empty_cache()
        return
    if not a.sweep:
        print("| GEMM (W [N][K]) | M | type | plan | skinny us | W TB/s | tile path us | torch.matmul us |\n"
              "|---|---|---|---|---|---|---|---|")
    for dt in a.dtypes.split(","):
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dt]
        for name, K, N in SHAPES:
            if name.split()[0] not in a.models.split(","):
                continue
            for M in rows:
                bench_shape(name, K, N, M, dtype, sweep=a.sweep)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
