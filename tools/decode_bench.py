"""Per-token time of incremental decoding on a zoo model against the only alternative without a cache.

`Model.generate` (prefill once, then one replay of the captured one-token step graph per token) is timed end to end,
and the step graph alone with device events.  The alternative is a full-sequence forward pass per new token; it is
timed at the final length P + N on a captured graph (the passes at shorter lengths are cheaper, so this is its
upper end, and a plan per length is not counted).  Prints one line per precision and GEMM path.

`--gemm tiles,skinny` builds one executor pair per path (`SliceExecutor.decoder(gemm=...)`) and times their step
graphs alternately, round after round in one process, then prints each path's median with the spread of its
rounds and the ratio between the paths.

`--weight-quant mxfp4` adds, in bf16, every path once more on MXFP4 weights (`SliceExecutor(weight_quant=...)`,
a path named `skinny+mxfp4`): another model, so its tokens differ; what compares is the time.  The value may be a
comma-separated list: `mxfp4,mxfp4_only` times the codes next to a bf16 copy and the codes alone (the prefill on
csrc/kernels/gemm_tile_mx.h), round by round in one process, and prints the device memory of each path's executors.

    python tools/decode_bench.py --model tinyllama_1_1b --batch 8 --prompt-tokens 128 --new-tokens 128 \
        --gemm tiles,skinny [--weight-quant mxfp4,mxfp4_only]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.model import Model  # noqa: E402
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.resnet import init_weights  # noqa: E402
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.models.zoo import build_model  # noqa: E402
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.runtime.executor import SliceExecutor  # noqa: E402


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="tinyllama_1_1b")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--prompt-tokens", type=int, default=128)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gemm", default="tiles", help="comma-separated decoder GEMM paths: tiles, skinny")
    ap.add_argument("--weight-quant", default=None,
                    help="bf16: each path also on MXFP4 weights; comma-separated: mxfp4, mxfp4_only")
    a = ap.parse_args()
    B, P, N = a.batch, a.prompt_tokens, a.new_tokens
    print(torch.cuda.get_device_name(0), flush=True)
    g = build_model(a.model)
    w = init_weights(g, seed=0)
    print(f"{a.model}: {g.count_params():,} parameters initialised", flush=True)
    vocab = int(g.layers[g.output_names[0]].attrs["units"])
    ids = np.random.default_rng(0).integers(0, vocab, (B, P + N))
    m = Model(g, w)
    for precision in a.precisions.split(","):
        # a path: the decoder's GEMM and the weights' quantisation, named as it is printed
        paths = {gm: (gm, None) for gm in a.gemm.split(",")}
        if a.weight_quant and precision == "bf16":
            paths.update({f"{gm}+{wq}": (gm, wq) for wq in a.weight_quant.split(",") for gm in a.gemm.split(",")})
        gemms = list(paths)

        def generate(gm):
            return m.generate(ids[:, :P], N, precision=precision, decode_gemm=paths[gm][0], weight_quant=paths[gm][1])

        def pair(gm):
            return next(v for k, v in m._executors.items()
                        if k[0] == "generate" and k[-3:] == (precision, paths[gm][1], paths[gm][0]))

        toks, gen, steps, prefill, pre = {}, {}, {}, {}, {}
        for gm in gemms:
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            toks[gm] = generate(gm)                                         # build, capture, warm up
            gen[gm], steps[gm], pre[gm] = [], [], []
            print(f"{a.model} {precision} gemm={gm}: {(torch.cuda.memory_allocated() - before) / 2 ** 20:.0f} MiB of "
                  f"device memory for its executors (weights, caches, activations)", flush=True)
        for _ in range(a.rounds):                                           # the paths alternate within a round
            for gm in gemms:
                t0 = time.perf_counter()
                generate(gm)                                                # ends in a device synchronise
                gen[gm].append((time.perf_counter() - t0) * 1e3)
                ex, dec = pair(gm)
                ex.forward(0)                                               # pos = P again
                steps[gm].append(events_ms(lambda: dec.forward(0), N))      # N replays: positions P .. P + N - 1
                pre[gm].append(events_ms(lambda: ex.forward(0), 3))
        for gm in gemms:
            ex, dec = pair(gm)
            prefill[gm] = sorted(pre[gm])[a.rounds // 2]
            if ex.mx_tile_steps:
                print(f"{a.model} {precision} gemm={gm}: prefill with {len(ex.mx_tile_steps)} conv steps on the MXFP4 "
                      f"tile GEMM, (F, MT, KS) {sorted(set(ex._mx_tile.values()))}", flush=True)
            if dec.skinny_steps:
                print(f"{a.model} {precision} gemm={gm}: {len(dec.skinny_steps)} conv steps on the skinny GEMM, (F, KS) "
                      f"{sorted(set(dec._skinny.values()))}", flush=True)
            if dec.mx_steps:
                print(f"{a.model} {precision} gemm={gm}: {len(dec.mx_steps)} conv steps on the MXFP4 skinny GEMM, (F, KS) "
                      f"{sorted(set(dec._mx.values()))}", flush=True)
        del ex, dec
        m._executors.clear()
        torch.cuda.empty_cache()
        full = SliceExecutor(build_model(a.model, input_shape=(P + N,)), w, B, precision=precision)
        full.capture()
        full.input_buf(full.g.input).copy_(torch.from_numpy(ids.astype(np.float32)))
        full.forward(0)
        torch.cuda.synchronize()
        fwd = sorted(events_ms(lambda: full.forward(0), 5) for _ in range(a.rounds))[a.rounds // 2]
        del full
        torch.cuda.empty_cache()
        for gm in gemms:
            med, step = sorted(gen[gm])[a.rounds // 2], sorted(steps[gm])[a.rounds // 2]
            print(f"{a.model} {precision} gemm={gm} B{B} prompt {P} + {N} new: generate {med:.1f} ms end to end = "
                  f"{med / N:.3f} ms per token ({B * N / med * 1e3:.0f} tokens/s; prefill {prefill[gm]:.2f} ms (spread "
                  f"{max(pre[gm]) - min(pre[gm]):.2f}), step graph "
                  f"alone {step:.3f} ms per token, rounds {' '.join(f'{v:.3f}' for v in steps[gm])}, spread "
                  f"{max(steps[gm]) - min(steps[gm]):.3f}) | full forward pass at {P + N} tokens {fwd:.2f} ms per token "
                  f"({fwd / (med / N):.1f}x generate per token, {fwd / step:.1f}x the step graph) | first tokens "
                  f"{toks[gm][0, :4].tolist()}", flush=True)
        if len(gemms) > 1:
            base = sorted(steps[gemms[0]])[a.rounds // 2]
            for gm in gemms[1:]:
                step = sorted(steps[gm])[a.rounds // 2]
                spread = max(max(steps[g_]) - min(steps[g_]) for g_ in (gemms[0], gm))
                print(f"{a.model} {precision} step graph alone: {gm} {step:.3f} ms against {gemms[0]} {base:.3f} ms = "
                      f"{base / step:.2f}x, ahead by {base - step:.3f} ms (largest spread of the rounds {spread:.3f} ms)",
                      flush=True)


if __name__ == "__main__":
    main()
