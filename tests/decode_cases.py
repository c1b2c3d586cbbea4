"""Case tuples of the incremental-decoding tests (csrc/kernels/attention_decode.h)."""
import itertools

# (hq, hkv, d, dv, probe): every group size g = hq / hkv in 1, 2, 3, 8, 16 at every DMAX (16 and 32 -> 32, 64,
# 128) and dv != d, under both softmax probes of tests/llama_cases.py gqa_inputs
DECODE_CASES = [hh + dd + (probe,) for hh, dd, probe in itertools.product(
    [(4, 4), (4, 2), (6, 2), (8, 1), (16, 1)], [(16, 16), (32, 16), (64, 64), (128, 128)], ["ascending", "dominant"])]
# 16 sequences on 8 kv heads: 128 (sequence, kv head) pairs, where the plan of an MI355X gives KS = 128 at
# Tmax = 257, so a wave walks two 16-key fragments of a split: the in-wave rescale and the prefetch rotation
LONG_CASES = [(8, 8, 64, 64, "ascending"), (8, 8, 64, 64, "dominant"), (16, 8, 32, 16, "ascending"),
              (16, 8, 128, 128, "dominant")]


def decode_lengths(KS):
    """One sequence per length, all in one launch: the fragment edges (16), a wave's share of a split (64), the
    split edges, and the ragged ends 1 and T = 2 KS + 1, so the batch has empty splits."""
    return [1, 15, 16, 17, 63, 64, 65, KS - 1, KS, KS + 1, 2 * KS + 1]


def long_lengths(KS):
    """16 lengths for KS >= 128: around the second fragment 64 + 16 w of every wave w, the split edges, inside the
    second and third split, and the ragged ends."""
    return [1, 65, 79, 81, 95, 97, 111, 113, KS - 1, KS, KS + 1, KS + 65, KS + 81, 2 * KS - 1, 2 * KS, 2 * KS + 1]


# (B, hq, hkv, d, dv, W) of kv_append, head sizes of LC.ROPE_CASES: d = 6 on the scalar path, d = 8 one fp32 vector
# (scalar in bf16), dv != d, d = 64 on the vector path in both types
APPEND_CASES = [
    (2, 4, 2, 6, 6, 10000.0),
    (2, 4, 2, 8, 8, 500000.0),
    (2, 6, 2, 16, 24, 10000.0),
    (2, 2, 1, 64, 64, 500000.0),
]
APPEND_TMAX = 9
APPEND_POS = [2, APPEND_TMAX - 2]       # ragged and non-zero; 5 tokens from the second run past the cache
