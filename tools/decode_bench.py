"""Per-token time of incremental decoding on a zoo model against the only alternative without a cache.

`Model.generate` (prefill once, then one replay of the captured one-token step graph per token) is timed end to end,
and the step graph alone with device events.  The alternative is a full-sequence forward pass per new token; it is
timed at the final length P + N on a captured graph (the passes at shorter lengths are cheaper, so this is its
upper end, and a plan per length is not counted).  Prints one line per precision.

    python tools/decode_bench.py --model tinyllama_1_1b --batch 8 --prompt-tokens 128 --new-tokens 128
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
        toks = m.generate(ids[:, :P], N, precision=precision)               # build, capture, warm up
        gen = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            m.generate(ids[:, :P], N, precision=precision)                  # ends in a device synchronise
            gen.append((time.perf_counter() - t0) * 1e3)
        ex, dec = next(v for k, v in m._executors.items() if k[0] == "generate" and k[-1] == precision)
        prefill = sorted(events_ms(lambda: ex.forward(0), 3) for _ in range(a.rounds))[a.rounds // 2]
        ex.forward(0)                                                       # pos = P again
        step = sorted(events_ms(lambda: dec.forward(0), N) for _ in range(1))[0]      # N replays: positions P .. P + N - 1
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
        med = sorted(gen)[a.rounds // 2]
        print(f"{a.model} {precision} B{B} prompt {P} + {N} new: generate {med:.1f} ms end to end = {med / N:.3f} ms per "
              f"token ({B * N / med * 1e3:.0f} tokens/s; prefill {prefill:.2f} ms, step graph alone {step:.3f} ms per "
              f"token) | full forward pass at {P + N} tokens {fwd:.2f} ms per token ({fwd / (med / N):.1f}x generate per "
              f"token, {fwd / step:.1f}x the step graph) | first tokens {toks[0, :4].tolist()}", flush=True)


if __name__ == "__main__":
    main()
