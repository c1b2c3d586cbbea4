"""The MXFP4 tile GEMM (csrc/kernels/gemm_tile_mx.h) per GEMM of tinyllama_1_1b and llama2_7b (qkv, out, gate / up,
down) at M = 64, 256, 1024, 4096 rows, against what the same step runs with a bf16 copy of the weights: the bf16 tile
config `choose_cfg` gives an executor without a tuning entry, on the dequantised weights.

Per shape the implementations are timed interleaved, each as a hipGraph of REPS calls that walk over copies of the
weights (tools/skinny_bench.py's `packed_mx`), one replay each per round; printed: the median of the rounds and
their spread (max - min).  Before timing, the kernel's output is checked against the tile path's (one bf16 rounding).
A row where the kernel is behind is bold.

    python tools/mx_tile_bench.py [--models tinyllama_1_1b,llama2_7b] [--rows 64,256,1024,4096]
    python tools/mx_tile_bench.py --sweep      # every (F, MT, KS) next to the plan's choice and the bf16 tile config
"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import conv as C  # noqa: E402
from attention_bench import capture  # noqa: E402
from skinny_bench import CACHE_BYTES, SHAPES, packed_mx  # noqa: E402

ROWS = (64, 256, 1024, 4096)
REPS, ROUNDS = 10, 7


def interleaved(runs):
    """name -> (median, spread) microseconds per call: every round replays each implementation's graph once, in turn."""
    graphs = {name: capture(run, REPS) for name, run in runs.items()}
    times = {name: [] for name in runs}
    for _ in range(ROUNDS):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / REPS * 1e3)
    return {name: (sorted(t)[ROUNDS // 2], max(t) - min(t)) for name, t in times.items()}


def bench_shape(name, K, N, M, sweep):
    pcs = packed_mx(K, N, min(REPS, max(2, math.ceil(CACHE_BYTES / (2 * N * K)))))
    x = torch.randn((M, K), device="cuda").bfloat16()
    out = {k: torch.empty((M, N), dtype=torch.bfloat16, device="cuda") for k in ("mxt", "tiles")}
    ctr = torch.zeros(8192, dtype=torch.int32, device="cuda")
    ws = torch.empty(C.MX_TILE_MAX_KS * M * N, dtype=torch.float32, device="cuda")
    cfg, ks = C.choose_cfg(M, N, pcs[0].Kpad)
    scratch = C.bf16_scratch(cfg, ks, M, 1, 1, pcs[0])
    tws = torch.empty(max(scratch[0], 1), dtype=torch.float32, device="cuda")
    tctr = torch.zeros(max(scratch[1], 1), dtype=torch.int32, device="cuda")
    turn = {}

    def pick(k):                                          # the next copy of W: call i of a graph reads copy i % copies
        turn[k] = turn.get(k, -1) + 1
        return pcs[turn[k] % len(pcs)]

    def mxt(key, F=None, MT=None, KS=None):
        return lambda: C.mx_tile_forward(x, pick(key), out["mxt"], F=F, MT=MT, ksplit=KS, workspace=ws, counters=ctr)

    def tiles():
        return C.conv_forward(x, pick("tiles"), out["tiles"], cfg=cfg, ksplit=ks, workspace=tws, counters=tctr)

    mxt("check")()
    tiles()
    torch.cuda.synchronize()
    a, b = out["mxt"].double(), out["tiles"].double()
    if not bool(((a - b).abs() <= b.abs() * 2.0 ** -7 + 2e-5 * b.abs().max()).all()):
        raise SystemExit(f"{name} M {M}: the tile GEMM on the codes differs from the bf16 tile path by "
                         f"{float((a - b).abs().max()):.3e}")
    F, MT, KS = C.mx_tile_plan(M, N, K)
    plan = f"F{F} MT{MT} KS{KS}"
    if sweep:
        grid = []
        for f, mt in C.MX_TILES:
            tiles_n = math.ceil(M / (16 * mt)) * math.ceil(N / (64 * f))
            for k in (1, 2, 4, 8):
                if k == 1 or (k <= max(1, C.mx_chunks(K) // 4) and tiles_n * k <= 4 * C.NUM_CUS and M * N * 4 < 2 ** 31):
                    grid.append((f, mt, k))
        if (F, MT, KS) not in grid:
            grid.append((F, MT, KS))
        runs = {f"F{f} MT{mt} KS{k}": mxt((f, mt, k), f, mt, k) for f, mt, k in grid}
        runs[f"bf16 cfg {cfg} ks {ks}"] = tiles
        us = interleaved(runs)
        best = min((k for k in us if k[0] == "F"), key=lambda k: us[k][0])
        print(f"{name} M {M}: plan {plan} {us[plan][0]:.1f} us, best {best} {us[best][0]:.1f} us | "
              + " ".join(f"{k}={v[0]:.1f}(+-{v[1]:.1f})" for k, v in us.items()), flush=True)
        return
    us = interleaved({"mxt": mxt("mxt"), "tiles": tiles})
    flops = 2.0 * M * N * K
    row = (f"| {name} | {M} | {plan} | {us['mxt'][0]:.1f} ({us['mxt'][1]:.1f}) | {flops / us['mxt'][0] / 1e6:.0f} | "
           f"cfg {cfg} ks {ks}: {us['tiles'][0]:.1f} ({us['tiles'][1]:.1f}) | {us['tiles'][0] / us['mxt'][0]:.2f}x |")
    behind = us["mxt"][0] > us["tiles"][0]
    print("| " + " | ".join(f"**{c.strip()}**" for c in row.strip("|").split("|")) + " |" if behind else row, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="tinyllama_1_1b,llama2_7b")
    ap.add_argument("--rows", default=",".join(str(r) for r in ROWS))
    ap.add_argument("--sweep", action="store_true", help="time every (F, MT, KS) instead of the plan alone")
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    if not a.sweep:
        print("| GEMM (W [N][K]) | M | plan | mxfp4 tile GEMM us (spread) | TFLOP/s | bf16 tile config on the bf16 copy us "
              "(spread) | bf16 time / mxfp4 time |\n|---|---|---|---|---|---|---|")
    for name, K, N in SHAPES:
        if name.split()[0] in a.models.split(","):
            for M in (int(r) for r in a.rows.split(",")):
                bench_shape(name, K, N, M, a.sweep)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
