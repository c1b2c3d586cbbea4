"""The three Llama kernels against the library on the shapes of TinyLlama 1.1B (32 query heads of 64 over 4 key /
value heads, width 2048) and Llama 2 7B (width 4096).

Timed the way tools/attention_bench.py times: every implementation is captured into its own hipGraph of `--reps`
calls and the graphs are replayed in turn, round after round, so clock and thermal state are shared; the median
round per implementation is reported.

* rmsnorm (csrc/kernels/layernorm.hip) against `F.rms_norm` at rows x C = 4096 x 2048 and 4096 x 4096, fp32 and
  bf16; GB/s counts one read and one write of the tensor.
* rope (csrc/kernels/layers.hip) against the torch composition (slice, multiply, concatenate) on the same buffer
  at B T = 4096 rows of 32 + 4 + 4 heads of 64, fp32 and bf16.
* the grouped-query attention core (csrc/kernels/attention.hip), causal, at T = 128, 512 and 2048 with 32 / 4 heads
  of 64, against `scaled_dot_product_attention(is_causal=True, enable_gqa=True)` and against the plain multi-head
  kernel on rows in which each K / V head stands 8 times.  The last comparison says what sharing K / V across the
  query heads buys or costs with the current block order; the rope time next to the core's says what fusing the
  rotation into the core could save.

    python tools/llama_bench.py [--rows 4096] [--reps 20] [--rounds 5] [--only rmsnorm|rope|gqa]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import attention as A  # noqa: E402
from adaptive_deep_learning_architecture_for_parallel_and_fault_tolerant_inference_amd.ops import eltwise as E  # noqa: E402

from attention_bench import interleaved_us  # noqa: E402

HQ, HKV, D, WAVELENGTH = 32, 4, 64, 10000.0


def bench_rmsnorm(rows, C, reps, rounds):
    x = torch.randn(rows, C, device="cuda")
    sc = torch.rand(C, device="cuda") + 0.5
    y = torch.empty_like(x)
    x16, y16 = x.to(torch.bfloat16), torch.empty(rows, C, device="cuda", dtype=torch.bfloat16)
    sc16 = sc.to(torch.bfloat16)
    t = interleaved_us({"ours": lambda: E.rmsnorm_f32(x, sc, y, 1e-5),
                        "ours16": lambda: E.rmsnorm(x16, sc, y16, C, 1e-5),
                        "torch": lambda: F.rms_norm(x, (C,), sc, 1e-5),
                        "torch16": lambda: F.rms_norm(x16, (C,), sc16, 1e-5)}, reps, rounds)
    diff = (F.rms_norm(x, (C,), sc, 1e-5) - y).abs().max().item()
    diff16 = (F.rms_norm(x16.float(), (C,), sc, 1e-5) - y16.float()).abs().max().item()
    gb = lambda us, size: 2.0 * rows * C * size / us / 1e3
    print(f"rmsnorm {rows} x {C}: fp32 ours {t['ours']:7.1f} us ({gb(t['ours'], 4):6.0f} GB/s) | F.rms_norm "
          f"{t['torch']:7.1f} us ({t['torch'] / t['ours']:5.2f}x ours) | bf16 ours {t['ours16']:7.1f} us "
          f"({gb(t['ours16'], 2):6.0f} GB/s) | F.rms_norm {t['torch16']:7.1f} us ({t['torch16'] / t['ours16']:5.2f}x "
          f"ours) | max diff {diff:.2e} (bf16 {diff16:.2e})", flush=True)


def bench_rope(rows, T, reps, rounds):
    ld = (HQ + 2 * HKV) * D
    rotw = (HQ + HKV) * D
    x = torch.randn(rows, ld, device="cuda")
    y = torch.empty_like(x)
    x16, y16 = x.to(torch.bfloat16), torch.empty(rows, ld, device="cuda", dtype=torch.bfloat16)
    table = A.rope_table(T, D, WAVELENGTH, device="cuda")
    cs = table[0].repeat(rows // T, 1)[:, None, :]
    sn = table[1].repeat(rows // T, 1)[:, None, :]
    cs16, sn16 = cs.to(torch.bfloat16), sn.to(torch.bfloat16)

    def composed(x, cs, sn):
        r = x[:, :rotw].reshape(rows, HQ + HKV, D)
        a, b = r[..., :D // 2], r[..., D // 2:]
        rot = torch.cat([a * cs - b * sn, b * cs + a * sn], dim=-1).reshape(rows, rotw)
        return torch.cat([rot, x[:, rotw:]], dim=1)

    t = interleaved_us({"ours": lambda: A.rope(x, table, y, T, HQ, D, D, kv_heads=HKV),
                        "ours16": lambda: A.rope(x16, table, y16, T, HQ, D, D, kv_heads=HKV),
                        "torch": lambda: composed(x, cs, sn),
                        "torch16": lambda: composed(x16, cs16, sn16)}, reps, rounds)
    diff = (composed(x, cs, sn) - y).abs().max().item()
    diff16 = (composed(x16.float(), cs, sn) - y16.float()).abs().max().item()
    gb = lambda us, size: 2.0 * rows * ld * size / us / 1e3
    print(f"rope {rows} rows of {HQ} + {HKV} + {HKV} heads of {D} (T {T}): fp32 ours {t['ours']:7.1f} us "
          f"({gb(t['ours'], 4):6.0f} GB/s) | torch {t['torch']:7.1f} us ({t['torch'] / t['ours']:5.2f}x ours) | bf16 ours "
          f"{t['ours16']:7.1f} us ({gb(t['ours16'], 2):6.0f} GB/s) | torch {t['torch16']:7.1f} us "
          f"({t['torch16'] / t['ours16']:5.2f}x ours) | max diff {diff:.2e} (bf16 {diff16:.2e})", flush=True)
    return t


def bench_gqa(rows, T, reps, rounds):
    B, g = max(1, rows // T), HQ // HKV
    w = HQ * D + 2 * HKV * D
    qkv = torch.randn(B * T, w, device="cuda")
    qkv[:, :HQ * D] *= D ** -0.5
    q = qkv[:, :HQ * D].reshape(B, T, HQ, D)
    k = qkv[:, HQ * D:(HQ + HKV) * D].reshape(B, T, HKV, D)
    v = qkv[:, (HQ + HKV) * D:].reshape(B, T, HKV, D)
    wide = torch.cat([q.reshape(B * T, -1), k.repeat_interleave(g, dim=2).reshape(B * T, -1),
                      v.repeat_interleave(g, dim=2).reshape(B * T, -1)], dim=1).contiguous()
    out, outw = torch.empty(B * T, HQ * D, device="cuda"), torch.empty(B * T, HQ * D, device="cuda")
    qkv16, wide16 = qkv.to(torch.bfloat16), wide.to(torch.bfloat16)
    out16, outw16 = (torch.empty(B * T, HQ * D, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    qs, ks, vs = (t.permute(0, 2, 1, 3).contiguous() for t in (q, k, v))

    def sdpa():
        return F.scaled_dot_product_attention(qs, ks, vs, scale=1.0, is_causal=True, enable_gqa=True)

    t = interleaved_us({"gqa": lambda: A.attention(qkv, out, B, T, HQ, D, D, causal=True, kv_heads=HKV),
                        "mha": lambda: A.attention(wide, outw, B, T, HQ, D, D, causal=True),
                        "gqa16": lambda: A.attention(qkv16, out16, B, T, HQ, D, D, causal=True, kv_heads=HKV),
                        "mha16": lambda: A.attention(wide16, outw16, B, T, HQ, D, D, causal=True),
                        "sdpa": sdpa}, reps, rounds)
    diff = (sdpa().permute(0, 2, 1, 3).reshape(B * T, HQ * D) - out).abs().max().item()
    flop = 2.0 * B * (T * (T + 1) // 2) * HQ * 2 * D
    print(f"gqa causal B{B} T{T} {HQ}/{HKV} heads of {D}: ours {t['gqa']:8.1f} us ({flop / t['gqa'] / 1e6:5.1f} TF/s) | "
          f"our MHA kernel on expanded rows {t['mha']:8.1f} us ({t['gqa'] / t['mha']:4.2f}x) | bf16 act ours "
          f"{t['gqa16']:8.1f} us | expanded {t['mha16']:8.1f} us ({t['gqa16'] / t['mha16']:4.2f}x) | sdpa is_causal "
          f"enable_gqa {t['sdpa']:8.1f} us ({t['sdpa'] / t['gqa']:5.2f}x ours) | equal to expanded: "
          f"{torch.equal(out, outw)} | max diff vs sdpa {diff:.2e}", flush=True)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096, help="B T of every measurement")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["rmsnorm", "rope", "gqa"])
    a = ap.parse_args()
    print(torch.cuda.get_device_name(0))
    print(f"B T = {a.rows} rows, median of {a.rounds} interleaved rounds of {a.reps} launches, microseconds", flush=True)
    if a.only in (None, "rmsnorm"):
        for C in (2048, 4096):
            bench_rmsnorm(a.rows, C, a.reps, a.rounds)
    for T in (128, 512, 2048):
        if a.only in (None, "rope"):
            rope = bench_rope(a.rows, T, a.reps, a.rounds)
        if a.only in (None, "gqa"):
            core = bench_gqa(a.rows, T, a.reps, a.rounds)
        if a.only is None:
            print(f"  T {T}: the rope step is {rope['ours'] / core['gqa']:4.2f}x the core's time in fp32, "
                  f"{rope['ours16'] / core['gqa16']:4.2f}x on bf16 activations", flush=True)


if __name__ == "__main__":
    main()
